"""The host side of exact multi-graph batches (poa_multi_*_exact): the footprint, the refusals and the ABI, all without a device,
and the stand-alone check of tests/multi_exact_host (the plan, and interleaved searches at the plan's slot strides) under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from poasta_amd.graph import pack_queries

import test_multi_plan as TMP
from test_multi_dense_plan import _case, _compact_elems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7


def test_multi_exact_host_plan_and_strides_under_sanitizers(tmp_path):
    """tests/multi_exact_host: regions, tables and slot workspaces disjoint and in bounds, chunk coverage exact, the footprint the
    documented sum; an interleaved batch of a bubble-rich graph and a chain searched slot by slot in one plan-sized buffer with
    canaries equals every search run alone — a program of its own, address and undefined-behaviour sanitizers on, on the CPU."""
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    exe = os.path.join(str(tmp_path), "multi_exact_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "multi_exact_host", "multi_exact_host.cpp"), os.path.join(csrc, "poa_multi_plan.cpp"),
                           os.path.join(csrc, "poa_sweep_rows.cpp"), os.path.join(csrc, "poa_graph.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"multi_exact_host ok" in r.stdout


def test_multi_exact_footprint_is_the_sum_the_header_documents():
    from poasta_amd import aligner
    graphs, seqs = _case()
    terms = []
    for g, qs in zip(graphs, seqs):
        dg = aligner._device_graph(g)
        for q in qs:
            terms.append(2 * _compact_elems(dg, len(q)) + 256 + 4 * 3 * g.n * TMP._pitch(len(q)) + 256)
    total, largest = aligner.multi_footprint(graphs, seqs, exact=True)
    assert largest == max(terms)
    # the rest is the slots' replay workspace, one slot per query without a cap: the same size for every slot, and at least the
    # default queue pool (64 x (3 x 64 + 8) + 256 entries of 16 bytes) and ring (3 x 64 words) of each
    slots = total - sum(terms)
    n = len(terms)
    assert slots > 0
    per_slot = slots // n
    assert per_slot >= (64 * (3 * 64 + 8) + 256) * 16 + 3 * 64 * 4
    for mode in ("exact", "hybrid"):
        assert aligner.multi_footprint(graphs, seqs, exact=True, config=aligner.make_config(mode)) == (total, largest)
    # a larger queue_entries_per_cell grows every slot's pool and nothing else
    more, largest2 = aligner.multi_footprint(graphs, seqs, exact=True, config=aligner.make_config("exact", queue_entries_per_cell=4.0))
    assert largest2 == largest and more > total and (more - total) % (n * 16) == 0
    # graph_qoff + packed queries, and a batch without queries
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    assert aligner.multi_footprint(graphs, graph_qoff=gq, qseq=qseq, qoff=qoff, exact=True) == (total, largest)
    assert aligner.multi_footprint(graphs, [[] for _ in graphs], exact=True) == (0, 0)
    # the dense kind's footprint is the dense part alone
    dense_total, _ = aligner.multi_footprint(graphs, seqs, dense=True)
    assert dense_total == sum(terms) - sum(4 * 3 * g.n * TMP._pitch(len(q)) + 256 for g, qs in zip(graphs, seqs) for q in qs)


def test_multi_exact_refusals_need_no_device():
    from poasta_amd import _lib, aligner
    L = _lib.lib()
    graphs, seqs = _case()
    dgs = [aligner._device_graph(g) for g in graphs]
    handles = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    total, largest = C.c_uint64(0), C.c_uint64(0)

    def footprint(gqoff=gq, hs=handles, cfg=None, qo=qoff, outs=True):
        return L.poa_multi_footprint_exact(hs, len(dgs), aligner._p(gqoff), aligner._p(qo), C.byref(cfg) if cfg is not None else None,
                                           C.byref(total) if outs else None, C.byref(largest) if outs else None)

    def create(gqoff=gq, hs=handles, cfg=None, qo=qoff, outs=True):
        h = C.c_void_p()
        rc = L.poa_multi_create_exact(hs, len(dgs), aligner._p(gqoff), 0, aligner._p(qseq), aligner._p(qo), C.byref(cfg) if cfg is not None else None,
                                      0, C.byref(h) if outs else None)
        assert rc != 0 or L.poa_device_count() > 0
        if rc == 0:
            L.poa_multi_destroy(h)
        return rc

    def one_shot(cfg=None, qo=qoff, costs=_lib.PoaCosts(4, 6, 2, 0)):
        rc = L.poa_align_multi_exact(handles, len(dgs), aligner._p(gq), C.byref(costs) if costs is not None else None,
                                     C.byref(cfg) if cfg is not None else None, aligner._p(qseq), aligner._p(qo), None, None, None, 0, None, None, 0)
        assert rc != 0 or L.poa_device_count() > 0
        return rc

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert L.poa_last_error() != b"", what

    assert footprint() == 0 and total.value > 0
    # every refusal names the single-graph call that takes the case
    seqs_wide = [list(qs) for qs in seqs]
    seqs_wide[-1][-1] = np.resize(seqs[-1][-1], 1024)
    _, qoff_wide = pack_queries([q for s in seqs_wide for q in s])
    for call in (footprint, create, one_shot):
        refused(call(qo=qoff_wide), ERR_UNSUPPORTED, ("1024 symbols", call.__name__))
        assert b"poa_align_batch_ex" in L.poa_last_error()
    for mode in ("dense", "score", "checkpoint", "checkpoint2"):
        for call in (footprint, create, one_shot):
            refused(call(cfg=aligner.make_config(mode)), ERR_UNSUPPORTED, (mode, call.__name__))
            assert b"poa_align_batch_ex" in L.poa_last_error()
    for mode in ("exact", "hybrid"):
        ef = aligner.make_config(mode, aln_type=aligner.AlignmentType.EndsFree())
        for call in (footprint, create, one_shot):
            refused(call(cfg=ef), ERR_UNSUPPORTED, ("ends-free", mode, call.__name__))
            assert b"poa_align_batch_ex" in L.poa_last_error()
    # the replay's own size limits, per graph: a queue pool past 2^32 entries
    big = aligner.make_config("exact", queue_entries_per_cell=1e7)
    for call in (footprint, create, one_shot):
        refused(call(cfg=big), ERR_UNSUPPORTED, ("queue pool", call.__name__))
        assert b"poa_align_batch_ex" in L.poa_last_error()
    bad_h = aligner.make_config("exact")
    bad_h.heuristic = 7
    for call in (footprint, create):
        refused(call(cfg=bad_h), ERR_INVALID_ARG, ("heuristic", call.__name__))
    # the argument errors of poa_multi_create
    bad0 = gq.copy(); bad0[0] = 1
    down = gq.copy(); down[1], down[2] = gq[2], gq[1]
    hole = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    hole[3] = None
    for what, kw in (("graph_qoff[0] != 0", dict(gqoff=bad0)), ("graph_qoff decreasing", dict(gqoff=down)), ("null graph", dict(hs=hole)),
                     ("null outputs", dict(outs=False))):
        for call in (footprint, create):
            refused(call(**kw), ERR_INVALID_ARG, (what, call.__name__))
    # null handles
    c = _lib.PoaCosts(4, 6, 2, 0)
    out4 = (C.c_uint32 * 4)()
    refused(L.poa_multi_run_exact(None, C.byref(c), None, None), ERR_INVALID_ARG, "run, null batch")
    refused(L.poa_multi_fetch_search_counters(None, out4), ERR_INVALID_ARG, "counters, null batch")
    refused(one_shot(costs=None), ERR_INVALID_ARG, "one-shot, null costs")
    # the binding: a two-piece exact batch does not exist, and a batch has one kind
    two = aligner.PoastaAligner(aligner.Affine2PieceMinGapCost(aligner.GapAffine2Piece(4, 2, 6, 1, 24)))
    for call in (lambda: aligner.multi_footprint(graphs, seqs, exact=True, two_piece=True),
                 lambda: aligner.multi_footprint(graphs, seqs, exact=True, dense=True),
                 lambda: two.align_multi(graphs, seqs, mode="exact"), lambda: two.align_multi(graphs, seqs, mode="hybrid"),
                 lambda: aligner.PoastaAligner(aligner.AffineMinGapCost(aligner.GapAffine(4, 2, 6)),
                                               aln_type=aligner.AlignmentType.EndsFree()).align_multi(graphs, seqs, mode="exact")):
        try:
            call()
            raise AssertionError("accepted")
        except ValueError:
            pass


def test_multi_exact_abi_symbols_declared_exported_bound():
    from poasta_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poasta_amd_multi_exact.h")).read(), flags=re.S)
    main_h = open(os.path.join(ROOT, "include", "poasta_amd.h")).read()
    assert '#include "poasta_amd_multi_exact.h"' in main_h
    raw = C.CDLL(_lib.LIB_PATH)
    declared = sorted(set(re.findall(r"\b(poa_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(_lib.EXPORTS_MULTI_EXACT)
    others = set(_lib.EXPORTS) | set(_lib.EXPORTS_MULTI_DENSE) | set(_lib.EXPORTS_TB) | set(_lib.EXPORTS_SCORESET_CAP) | set(_lib.EXPORTS_SCORESET_BEST)
    assert not set(_lib.EXPORTS_MULTI_EXACT) & others
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in _lib.EXPORTS_MULTI_EXACT:
        assert hasattr(raw, name), "libpoasta_amd.so does not export %s" % name
        assert getattr(_lib.lib(), name).argtypes is not None, name
        assert name in integration, name
