"""The host side of dense and exact multi-graph batches with queries of more than 1023 symbols (POA_CFG_WIDE_QUERIES): the plan
check of tests/multi_wide_host under the address and undefined-behaviour sanitizers, the footprint with the flag, the binding's
rule for setting it, and the ABI's new macros — all without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from poasta_amd.graph import pack_queries

import test_multi_plan as TMP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_UNSUPPORTED = -7
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _compact_elems(dg, length):
    from poasta_amd import _lib
    v = C.c_uint64(0)
    _lib.check(_lib.lib().poa_graph_compact_elems(dg.handle, length, C.byref(v)))
    return int(v.value)


def _case(top):
    """test_multi_plan._case() (queries of 1100, 1023 and 1024 symbols among short ones) with every query cut to `top` symbols."""
    graphs, seqs = TMP._case()
    assert sorted(len(q) for qs in seqs for q in qs)[-3:] == [1023, 1024, 1100]
    return graphs, [[q[:top] for q in qs] for qs in seqs]


def test_multi_wide_host_plan_under_sanitizers(tmp_path):
    """tests/multi_wide_host: pitches, carry words (none up to pitch 1024, 2 x rows above), carry and plane regions disjoint,
    chunk coverage under caps, the carry-overflow refusal, the exact plan's tables and slot by the longest query, and the
    unchanged refusal without `wide` — a program of its own, address and undefined-behaviour sanitizers on, on the CPU."""
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    exe = os.path.join(str(tmp_path), "multi_wide_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "multi_wide_host", "multi_wide_host.cpp"), os.path.join(csrc, "poa_multi_plan.cpp"),
                           os.path.join(csrc, "poa_sweep_rows.cpp"), os.path.join(csrc, "poa_graph.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"multi_wide_host ok" in r.stdout


@pytest.mark.parametrize("kind", ["dense", "exact"])
def test_multi_wide_flag_lifts_the_refusal_and_keeps_the_footprint_rule(kind):
    from poasta_amd import _lib, aligner
    L = _lib.lib()
    exact = kind == "exact"
    fn = L.poa_multi_footprint_exact if exact else L.poa_multi_footprint_dense
    # the 1024-symbol case of test_multi_dense_plan / test_multi_exact_plan: every query at most 1023 symbols, the last one 1024
    graphs, seqs = _case(1023)
    seqs[-1][-1] = np.resize(seqs[-1][-1], 1024)
    dgs = [aligner._device_graph(g) for g in graphs]
    handles = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    _, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    total, largest = C.c_uint64(0), C.c_uint64(0)

    def footprint(cfg):
        return fn(handles, len(dgs), aligner._p(gq), aligner._p(qoff), C.byref(cfg) if cfg is not None else None, C.byref(total), C.byref(largest))

    mode = "exact" if exact else "dense"
    # without the flag: today's refusal and message, under a NULL config and under one with another flag set
    for cfg in (None, aligner.make_config(mode), aligner.make_config(mode, full_planes=True)):
        assert footprint(cfg) == ERR_UNSUPPORTED
        assert (b"poa_align_batch_ex" if exact else b"poa_multi_create") in L.poa_last_error()
    # with it: accepted, and the documented sum
    assert footprint(aligner.make_config(mode, wide_queries=True)) == 0
    dense_terms = [2 * _compact_elems(dg, len(q)) + 256 for dg, qs in zip(dgs, seqs) for q in qs]
    table_terms = [4 * 3 * g.n * TMP._pitch(len(q)) + 256 for g, qs in zip(graphs, seqs) for q in qs]
    if exact:
        terms = [a + b for a, b in zip(dense_terms, table_terms)]
        assert largest.value == max(terms) and total.value > sum(terms)   # (the slots' replay workspace on top)
        wide_total = total.value
        assert footprint(aligner.make_config("hybrid", wide_queries=True)) == 0 and total.value == wide_total
    else:
        assert total.value == sum(dense_terms) and largest.value == max(dense_terms)
    # the whole case of test_multi_plan, 1100 symbols included, through the binding: wide=None sets the flag by itself
    graphs, seqs = _case(1 << 30)
    dgs = [aligner._device_graph(g) for g in graphs]
    dense_terms = [2 * _compact_elems(dg, len(q)) + 256 for dg, qs in zip(dgs, seqs) for q in qs]
    table_terms = [4 * 3 * g.n * TMP._pitch(len(q)) + 256 for g, qs in zip(graphs, seqs) for q in qs]
    t, lg = aligner.multi_footprint(graphs, seqs, dense=not exact, exact=exact)
    if exact:
        assert lg == max(a + b for a, b in zip(dense_terms, table_terms)) and t > sum(dense_terms) + sum(table_terms)
    else:
        assert (t, lg) == (sum(dense_terms), max(dense_terms))
    assert aligner.multi_footprint(graphs, seqs, dense=not exact, exact=exact, wide=True) == (t, lg)
    assert aligner.multi_footprint(graphs, seqs, dense=not exact, exact=exact, config=aligner.make_config(mode, wide_queries=True)) == (t, lg)
    # forced off: the library's refusal comes through
    for kw in (dict(wide=False), dict(wide=False, config=aligner.make_config(mode, wide_queries=True))):
        with pytest.raises(_lib.PoaError):
            aligner.multi_footprint(graphs, seqs, dense=not exact, exact=exact, **kw)


def test_multi_wide_none_sets_the_flag_exactly_when_needed():
    from poasta_amd import _lib, aligner
    graphs, long_seqs = _case(1 << 30)
    _, edge_seqs = _case(1024)
    _, short_seqs = _case(1023)
    assert max(len(q) for s in edge_seqs for q in s) == 1024 and max(len(q) for s in short_seqs for q in s) == 1023
    mi = {k: aligner._MultiInput(graphs, s) for k, s in (("long", long_seqs), ("edge", edge_seqs), ("short", short_seqs), ("none", [[] for _ in graphs]))}
    W = _lib.CFG_WIDE_QUERIES

    def flag(which, config, dense, exact, wide):
        cfg, is_wide = aligner._multi_wide_config("test", mi[which], config, dense, exact, wide)
        assert is_wide == bool(cfg is not None and cfg.flags & W)
        return is_wide, cfg

    for dense, exact in ((True, False), (False, True)):
        mode = "exact" if exact else "dense"
        assert flag("long", None, dense, exact, None)[0] and flag("edge", None, dense, exact, None)[0]
        assert not flag("short", None, dense, exact, None)[0] and not flag("none", None, dense, exact, None)[0]
        # a config without the flag is copied, never modified, and keeps its other fields
        given = aligner.make_config("hybrid" if exact else "dense", pruning=False, queue_entries_per_cell=2.0, full_planes=True)
        is_wide, cfg = flag("long", given, dense, exact, None)
        assert is_wide and cfg is not given and given.flags == _lib.CFG_FULL_PLANES and cfg.flags == _lib.CFG_FULL_PLANES | W
        assert (cfg.mode, cfg.pruning, cfg.queue_entries_per_cell) == (given.mode, 0, 2.0)
        # short queries leave the caller's object as it is; without a config the library keeps getting NULL
        assert flag("short", given, dense, exact, None)[1] is given and flag("short", None, dense, exact, None)[1] is None
        # a config created without one: the mode the library reads NULL as
        assert flag("long", None, dense, exact, None)[1].mode == aligner.MODES[mode]
        # forced
        assert flag("short", None, dense, exact, True)[0] and not flag("long", None, dense, exact, False)[0]
        set_cfg = aligner.make_config(mode, wide_queries=True)
        is_wide, cfg = flag("long", set_cfg, dense, exact, False)
        assert not is_wide and cfg is not set_cfg and set_cfg.flags == W and cfg.flags == 0
        assert flag("short", set_cfg, dense, exact, None)[1].flags == 0   # None means "iff needed": cleared for short queries
    # the checkpointed kinds take any length: never flagged, and wide=True is an error
    assert flag("long", None, False, False, None) == (False, None) and flag("long", None, False, False, False) == (False, None)
    for call in (lambda: aligner.multi_footprint(graphs, long_seqs, wide=True), lambda: aligner.multi_footprint(graphs, long_seqs, two_piece=True, wide=True),
                 lambda: aligner.MultiGraphBatch(graphs, short_seqs, wide=True), lambda: aligner.MultiGraphBatch(graphs, short_seqs, two_piece=True, wide=True)):
        with pytest.raises(ValueError):
            call()
    assert aligner.multi_footprint(graphs, long_seqs, wide=False) == aligner.multi_footprint(graphs, long_seqs)
    assert aligner.make_config("dense", wide_queries=True).flags == W and aligner.make_config("dense").flags == 0


def test_multi_wide_macros_are_declared():
    from poasta_amd import _lib
    main_h = open(os.path.join(ROOT, "include", "poasta_amd.h")).read()
    m = re.search(r"^#define\s+POA_CFG_WIDE_QUERIES\s+(\d+)u\b", main_h, flags=re.M)
    assert m and int(m.group(1)) == 2 == _lib.CFG_WIDE_QUERIES
    m = re.search(r"^#define\s+POA_LAUNCH_STRIPS\s+(\d+)u\b", main_h, flags=re.M)
    assert m and int(m.group(1)) == 4 == _lib.LAUNCH_STRIPS
    # beside their precedents, and distinct from them
    assert re.search(r"^#define\s+POA_CFG_FULL_PLANES\s+1u\b", main_h, flags=re.M) and re.search(r"^#define\s+POA_LAUNCH_MW\s+2u\b", main_h, flags=re.M)
    for name in ("poasta_amd_multi_dense.h", "poasta_amd_multi_exact.h"):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert "POA_CFG_WIDE_QUERIES" in text and "POA_LAUNCH_STRIPS" in text, name
