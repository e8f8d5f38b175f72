"""The host side of dense multi-graph batches (poa_multi_*_dense): the footprint, the refusals and the ABI, all without a device,
and the stand-alone plan check of tests/multi_dense_host under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from poasta_amd.graph import pack_queries

import test_multi_plan as TMP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _case():
    """test_multi_plan._case() with its 1100- and 1024-symbol queries shortened to 1023: one strip of the packed kernel."""
    graphs, seqs = TMP._case()
    rng = np.random.default_rng(4)
    seqs = [[q if len(q) <= 1023 else rng.choice(ACGT, 1023) for q in qs] for qs in seqs]
    assert sorted(len(q) for qs in seqs for q in qs)[-3:] == [1023, 1023, 1023]
    return graphs, seqs


def _compact_elems(dg, length):
    from poasta_amd import _lib
    v = C.c_uint64(0)
    _lib.check(_lib.lib().poa_graph_compact_elems(dg.handle, length, C.byref(v)))
    return int(v.value)


def test_multi_dense_footprint_is_the_sum_over_queries():
    from poasta_amd import aligner
    graphs, seqs = _case()
    terms, ckpt_terms = [], []
    for g, qs in zip(graphs, seqs):
        dg = aligner._device_graph(g)
        _, rpq = dg.checkpoint_plan(0)
        for q in qs:
            elems = _compact_elems(dg, len(q))
            # at least the M plane and its quarter plane of codes, at most all D rows on top
            rp = g.n * TMP._pitch(len(q))
            assert rp + rp // 4 <= elems <= 2 * rp + rp // 4
            terms.append(2 * elems + 256)
            ckpt_terms.append(rpq * TMP._pitch(len(q)) * 4 + 256)
    total, largest = aligner.multi_footprint(graphs, seqs, dense=True)
    assert total == sum(terms) and largest == max(terms)
    assert aligner.multi_footprint(graphs, seqs, dense=True, config=aligner.make_config("dense")) == (total, largest)
    # against the checkpointed footprint of the same queries: the 5-node graph and the 300-row one, each holding every query of
    # the case.  The direction is what the per-query terms give, computed here; the library's two sums must agree with it.
    ck_total, _ = aligner.multi_footprint(graphs, seqs)
    assert ck_total == sum(ckpt_terms)
    every = [q for qs in seqs for q in qs]
    sizes = [g.n for g in graphs]
    small, big = sizes.index(5 + 2), sizes.index(max(sizes))   # (two sentinel rows on top of the nodes)
    assert sizes[big] >= 300
    direction = {}
    for gi in (small, big):
        dg = aligner._device_graph(graphs[gi])
        _, rpq = dg.checkpoint_plan(0)
        dense_sum = sum(2 * _compact_elems(dg, len(q)) + 256 for q in every)
        ckpt_sum = sum(rpq * TMP._pitch(len(q)) * 4 + 256 for q in every)
        assert dense_sum != ckpt_sum
        dense_b = aligner.multi_footprint([graphs[gi]], [every], dense=True)[0]
        ckpt_b = aligner.multi_footprint([graphs[gi]], [every])[0]
        assert (dense_b, ckpt_b) == (dense_sum, ckpt_sum)
        direction[gi] = dense_b < ckpt_b
    # (5 nodes: the checkpointed plan keeps every row and a window on top; 300 rows: slots, snapshots and one window)
    assert direction[small] and not direction[big], direction
    # graph_qoff + packed queries, and a batch without queries
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    assert aligner.multi_footprint(graphs, graph_qoff=gq, qseq=qseq, qoff=qoff, dense=True) == (total, largest)
    assert aligner.multi_footprint(graphs, [[] for _ in graphs], dense=True) == (0, 0)


def test_multi_dense_refusals_need_no_device():
    from poasta_amd import _lib, aligner
    L = _lib.lib()
    graphs, seqs = _case()
    dgs = [aligner._device_graph(g) for g in graphs]
    handles = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    total, largest = C.c_uint64(0), C.c_uint64(0)

    def footprint(gqoff=gq, hs=handles, cfg=None, qo=qoff, outs=True):
        return L.poa_multi_footprint_dense(hs, len(dgs), aligner._p(gqoff), aligner._p(qo), C.byref(cfg) if cfg is not None else None,
                                           C.byref(total) if outs else None, C.byref(largest) if outs else None)

    def create(gqoff=gq, hs=handles, cfg=None, qo=qoff, outs=True):
        h = C.c_void_p()
        rc = L.poa_multi_create_dense(hs, len(dgs), aligner._p(gqoff), 0, aligner._p(qseq), aligner._p(qo), C.byref(cfg) if cfg is not None else None,
                                      0, C.byref(h) if outs else None)
        assert rc != 0 or L.poa_device_count() > 0
        if rc == 0:
            L.poa_multi_destroy(h)
        return rc

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert L.poa_last_error() != b"", what

    assert footprint() == 0 and total.value > 0
    # a 1024-symbol query is wider than one strip; the message names the batch that takes it
    seqs_wide = [list(qs) for qs in seqs]
    seqs_wide[-1][-1] = np.resize(seqs[-1][-1], 1024)
    _, qoff_wide = pack_queries([q for s in seqs_wide for q in s])
    for call in (footprint, create):
        refused(call(qo=qoff_wide), ERR_UNSUPPORTED, ("1024 symbols", call.__name__))
        assert b"poa_multi_create" in L.poa_last_error()
    for mode in ("exact", "hybrid", "score", "checkpoint", "checkpoint2"):
        for call in (footprint, create):
            refused(call(cfg=aligner.make_config(mode)), ERR_UNSUPPORTED, (mode, call.__name__))
    ef = aligner.make_config("dense", aln_type=aligner.AlignmentType.EndsFree())
    for call in (footprint, create):
        refused(call(cfg=ef), ERR_UNSUPPORTED, ("ends-free", call.__name__))
    # the argument errors of poa_multi_create
    bad0 = gq.copy(); bad0[0] = 1
    down = gq.copy(); down[1], down[2] = gq[2], gq[1]
    assert down[2] < down[1]
    hole = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    hole[3] = None
    for what, kw in (("graph_qoff[0] != 0", dict(gqoff=bad0)), ("graph_qoff decreasing", dict(gqoff=down)), ("null graph", dict(hs=hole)),
                     ("null outputs", dict(outs=False))):
        for call in (footprint, create):
            refused(call(**kw), ERR_INVALID_ARG, (what, call.__name__))
    # null handles
    c = _lib.PoaCosts(4, 6, 2, 0)
    out8 = (C.c_uint32 * 8)()
    refused(L.poa_multi_run_dense(None, C.byref(c), None, None), ERR_INVALID_ARG, "run, null batch")
    refused(L.poa_multi_last_launch(None, 0, out8), ERR_INVALID_ARG, "last launch, null batch")
    refused(L.poa_graph_compact_elems(None, 3, C.byref(total)), ERR_INVALID_ARG, "compact elems, null graph")
    refused(L.poa_graph_compact_elems(dgs[0].handle, 3, None), ERR_INVALID_ARG, "compact elems, null output")
    refused(L.poa_align_multi_dense(handles, len(dgs), aligner._p(gq), None, None, aligner._p(qseq), aligner._p(qoff), None, None, None, 0, None,
                                    None, 0), ERR_INVALID_ARG, "one-shot, null costs")
    # the binding: a two-piece dense batch does not exist
    for call in (lambda: aligner.multi_footprint(graphs, seqs, dense=True, two_piece=True),
                 lambda: aligner.PoastaAligner(aligner.Affine2PieceMinGapCost(aligner.GapAffine2Piece(4, 2, 6, 1, 24))).align_multi(graphs, seqs, mode="dense")):
        try:
            call()
            raise AssertionError("a two-piece dense batch was accepted")
        except ValueError:
            pass


def test_multi_dense_abi_symbols_declared_exported_bound():
    from poasta_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poasta_amd_multi_dense.h")).read(), flags=re.S)
    main_h = open(os.path.join(ROOT, "include", "poasta_amd.h")).read()
    assert '#include "poasta_amd_multi_dense.h"' in main_h
    raw = C.CDLL(_lib.LIB_PATH)
    declared = sorted(set(re.findall(r"\b(poa_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(_lib.EXPORTS_MULTI_DENSE)
    assert not set(_lib.EXPORTS_MULTI_DENSE) & set(_lib.EXPORTS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in _lib.EXPORTS_MULTI_DENSE:
        assert hasattr(raw, name), "libpoasta_amd.so does not export %s" % name
        assert getattr(_lib.lib(), name).argtypes is not None, name
        assert name in integration, name


def test_multi_dense_host_plan_under_sanitizers(tmp_path):
    """tests/multi_dense_host: offsets aligned and in bounds, regions disjoint, chunk coverage exact, quads by the largest pitch,
    one table copy per handle — a program of its own, address and undefined-behaviour sanitizers on, on the CPU."""
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    exe = os.path.join(str(tmp_path), "multi_dense_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "multi_dense_host", "multi_dense_host.cpp"), os.path.join(csrc, "poa_multi_plan.cpp"),
                           os.path.join(csrc, "poa_sweep_rows.cpp"), os.path.join(csrc, "poa_graph.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"multi_dense_host ok" in r.stdout
