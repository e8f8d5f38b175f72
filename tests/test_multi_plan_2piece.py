"""The host side of two-piece multi-graph batches (poa_multi_*_2piece): the footprint, the argument and mode errors and the ABI,
all without a device, and the stand-alone plan check of tests/multi_host2 under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from poasta_amd.graph import pack_queries

from test_multi_plan import ERR_INVALID_ARG, ERR_UNSUPPORTED, _case, _pitch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI2_SYMBOLS = ("poa_multi_footprint_2piece", "poa_multi_create_2piece", "poa_multi_run_2piece", "poa_align_multi_2piece")


def test_multi2_footprint_is_the_sum_over_queries():
    from poasta_amd import aligner
    graphs, seqs = _case()
    for k in (0, 1, 7):
        terms, terms1 = [], []
        for g, qs in zip(graphs, seqs):
            dg = aligner.DeviceGraph(g)
            _, rpq = dg.checkpoint_plan(k, two_piece=True)   # the graph alone
            terms += [rpq * _pitch(len(q)) * 4 + 256 for q in qs]
            terms1 += [dg.checkpoint_plan(k)[1] * _pitch(len(q)) * 4 + 256 for q in qs]
        cfg = aligner.make_config("checkpoint2", ckpt_rows=k) if k else None
        total, largest = aligner.multi_footprint(graphs, seqs, config=cfg, two_piece=True)
        assert total == sum(terms) and largest == max(terms), k
        # (not the one-piece batch's footprint: three kept planes and five window planes instead of two and three)
        assert sum(terms) > sum(terms1), k
    # graph_qoff + packed queries, and a batch without queries
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    assert aligner.multi_footprint(graphs, graph_qoff=gq, qseq=qseq, qoff=qoff, two_piece=True) == aligner.multi_footprint(graphs, seqs, two_piece=True)
    assert aligner.multi_footprint(graphs, [[] for _ in graphs], two_piece=True) == (0, 0)


def test_multi2_argument_and_mode_errors_need_no_device():
    from poasta_amd import _lib, aligner
    L = _lib.lib()
    graphs, seqs = _case()
    dgs = [aligner.DeviceGraph(g) for g in graphs]
    handles = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    total, largest = C.c_uint64(0), C.c_uint64(0)
    score = np.zeros(len(qoff) - 1, np.uint32)
    c2 = _lib.PoaCosts2(4, 6, 2, 24, 1, 0)

    def footprint(gqoff=gq, hs=handles, cfg=None):
        return L.poa_multi_footprint_2piece(hs, len(dgs), aligner._p(gqoff), aligner._p(qoff), C.byref(cfg) if cfg is not None else None,
                                            C.byref(total), C.byref(largest))

    def create(gqoff=gq, hs=handles, cfg=None):
        h = C.c_void_p()
        rc = L.poa_multi_create_2piece(hs, len(dgs), aligner._p(gqoff), 0, aligner._p(qseq), aligner._p(qoff),
                                       C.byref(cfg) if cfg is not None else None, 0, C.byref(h))
        assert rc != 0 or L.poa_device_count() > 0
        if rc == 0:
            L.poa_multi_destroy(h)
        return rc

    def one_shot(gqoff=gq, hs=handles, cfg=None, costs=c2):
        rc = L.poa_align_multi_2piece(hs, len(dgs), aligner._p(gqoff), C.byref(costs), C.byref(cfg) if cfg is not None else None,
                                      aligner._p(qseq), aligner._p(qoff), aligner._p(score), None, None, 0, None, None, 0)
        assert rc != 0 or L.poa_device_count() > 0
        return rc

    assert footprint() == 0 and total.value > 0
    assert footprint(cfg=aligner.make_config("checkpoint2")) == 0
    bad0 = gq.copy(); bad0[0] = 1
    down = gq.copy(); down[1], down[2] = gq[2], gq[1]
    assert down[2] < down[1]
    hole = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    hole[3] = None
    for what, kw in (("graph_qoff[0] != 0", dict(gqoff=bad0)), ("graph_qoff decreasing", dict(gqoff=down)), ("null graph", dict(hs=hole))):
        for call in (footprint, create, one_shot):
            assert call(**kw) == ERR_INVALID_ARG, (what, call.__name__)
            assert L.poa_last_error() != b"", what
    for mode in ("dense", "exact", "hybrid", "score", "checkpoint"):
        for call in (footprint, create, one_shot):
            assert call(cfg=aligner.make_config(mode)) == ERR_UNSUPPORTED, (mode, call.__name__)
            assert L.poa_last_error() != b""
    ef = aligner.make_config("checkpoint2", aln_type=aligner.AlignmentType.EndsFree())
    assert footprint(cfg=ef) == ERR_UNSUPPORTED and create(cfg=ef) == ERR_UNSUPPORTED and one_shot(cfg=ef) == ERR_UNSUPPORTED
    # extend1 < extend2, and null arguments
    assert one_shot(costs=_lib.PoaCosts2(4, 6, 1, 24, 2, 0)) == ERR_INVALID_ARG and L.poa_last_error() != b""
    assert L.poa_multi_run_2piece(None, C.byref(c2), None, None) == ERR_INVALID_ARG
    assert L.poa_multi_footprint_2piece(handles, len(dgs), aligner._p(gq), aligner._p(qoff), None, None, None) == ERR_INVALID_ARG
    assert L.poa_multi_create_2piece(handles, len(dgs), aligner._p(gq), 0, aligner._p(qseq), aligner._p(qoff), None, 0, None) == ERR_INVALID_ARG
    # the one-piece entry points keep refusing the two-piece mode
    ck2 = aligner.make_config("checkpoint2")
    assert L.poa_multi_footprint(handles, len(dgs), aligner._p(gq), aligner._p(qoff), C.byref(ck2), C.byref(total), C.byref(largest)) == ERR_UNSUPPORTED
    # the binding knows the query count and checks graph_qoff[n_graphs] against it
    short = gq.copy(); short[-1] -= 1
    try:
        aligner.multi_footprint(graphs, graph_qoff=short, qseq=qseq, qoff=qoff, two_piece=True)
        raise AssertionError("graph_qoff[n_graphs] != query count was accepted")
    except ValueError:
        pass


def test_multi2_chunk_plan_of_the_mixed_batch():
    """The shapes of tests/test_multi_graph_2piece.py test 3, on the host: under the two-piece plan a cap of largest + 256 cuts the
    mixed batch into three or more chunks, with a boundary inside a graph's range and one between two graphs."""
    from poasta_amd import aligner
    from test_multi_graph import _mixed
    graphs, seqs = _mixed()
    total, largest = aligner.multi_footprint(graphs, seqs, two_piece=True)
    terms = []
    for gi, (g, qs) in enumerate(zip(graphs, seqs)):
        _, rpq = aligner._device_graph(g).checkpoint_plan(0, two_piece=True)
        terms += [(gi, rpq * _pitch(len(q)) * 4 + 256) for q in qs]
    assert total == sum(t for _, t in terms) and largest == max(t for _, t in terms)
    cap, firsts, used = largest + 256, [0], 0
    for i, (_, t) in enumerate(terms):
        if used + t > cap and i > firsts[-1]:
            firsts.append(i)
            used = 0
        used += t
    assert len(firsts) >= 3, firsts
    assert any(terms[f][0] == terms[f - 1][0] for f in firsts[1:]) and any(terms[f][0] != terms[f - 1][0] for f in firsts[1:]), firsts
    # several segments under ckpt_rows = 7 (test 2)
    n_seg = [len(aligner._device_graph(g).checkpoint_plan(7, two_piece=True)[0]) - 1 for g in graphs]
    assert sum(s >= 3 for s in n_seg[:3]) >= 2 and n_seg[3] == 1, n_seg


def test_multi2_abi_symbols_declared_exported_bound():
    from poasta_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poasta_amd.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    declared = sorted(set(re.findall(r"\b(poa_(?:multi_[a-z_]+|align_multi)_2piece)\s*\(", hdr)))
    assert declared == sorted(MULTI2_SYMBOLS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in MULTI2_SYMBOLS:
        assert hasattr(raw, name), "libpoasta_amd.so does not export %s" % name
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name).argtypes is not None, name
        assert name in integration, name


def test_multi2_host_plan_under_sanitizers(tmp_path):
    """tests/multi_host2: the two-piece plan — offsets in bounds, regions disjoint, chunk coverage exact, six carry words per row
    for the carried query only — a program of its own, address and undefined-behaviour sanitizers on, on the CPU."""
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    exe = os.path.join(str(tmp_path), "multi_host2")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "multi_host2", "multi_host2.cpp"), os.path.join(csrc, "poa_multi_plan.cpp"),
                           os.path.join(csrc, "poa_sweep_rows.cpp"), os.path.join(csrc, "poa_graph.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"multi_host2 ok" in r.stdout
