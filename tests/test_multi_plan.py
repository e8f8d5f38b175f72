"""The host side of multi-graph batches (poa_multi_*): the footprint, the argument errors and the ABI, all without a device, and
the stand-alone plan check of tests/multi_host under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7
MULTI_SYMBOLS = ("poa_multi_footprint", "poa_multi_create", "poa_multi_run", "poa_multi_fetch", "poa_multi_stats",
                 "poa_multi_device_results", "poa_multi_workspace_bytes", "poa_multi_destroy", "poa_align_multi")


def _case():
    rng = np.random.default_rng(3)
    graphs = [W.random_dag(s, n_nodes=n, p_edge=0.3) for s, n in ((1, 12), (2, 30), (3, 5))]
    g, _ = W.scaled_linearish(300, 15, 8, 1, 50)
    graphs += [g, GraphBuilder().finish(), graphs[1]]
    lens = [[0, 1, 63, 64], [5, 200], [], [1100, 30], [4], [17, 1023, 1024]]
    seqs = [[rng.choice(np.frombuffer(b"ACGT", np.uint8), l) for l in ls] for ls in lens]
    return graphs, seqs


def _pitch(length):
    # the rule of a single-graph batch, poasta_amd/csrc/poa_engine.hip batch_create_impl:
    #     const uint32_t pitch = (uint32_t)(((L + 1 + 63) / 64) * 64);
    return ((length + 1 + 63) // 64) * 64


def test_multi_footprint_is_the_sum_over_queries():
    from poasta_amd import aligner
    graphs, seqs = _case()
    for k in (0, 1, 7):
        terms = []
        for g, qs in zip(graphs, seqs):
            _, rpq = aligner.DeviceGraph(g).checkpoint_plan(k)   # the graph alone
            terms += [rpq * _pitch(len(q)) * 4 + 256 for q in qs]
        cfg = aligner.make_config("checkpoint", ckpt_rows=k) if k else None
        total, largest = aligner.multi_footprint(graphs, seqs, config=cfg)
        assert total == sum(terms) and largest == max(terms), k
    # graph_qoff + packed queries, and a batch without queries
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    assert aligner.multi_footprint(graphs, graph_qoff=gq, qseq=qseq, qoff=qoff) == aligner.multi_footprint(graphs, seqs)
    assert aligner.multi_footprint(graphs, [[] for _ in graphs]) == (0, 0)


def test_multi_argument_errors_need_no_device():
    from poasta_amd import _lib, aligner
    L = _lib.lib()
    graphs, seqs = _case()
    dgs = [aligner.DeviceGraph(g) for g in graphs]
    handles = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    gq = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    total, largest = C.c_uint64(0), C.c_uint64(0)

    def footprint(gqoff=gq, hs=handles, cfg=None):
        return L.poa_multi_footprint(hs, len(dgs), aligner._p(gqoff), aligner._p(qoff), C.byref(cfg) if cfg is not None else None,
                                     C.byref(total), C.byref(largest))

    def create(gqoff=gq, hs=handles, cfg=None):
        h = C.c_void_p()
        rc = L.poa_multi_create(hs, len(dgs), aligner._p(gqoff), 0, aligner._p(qseq), aligner._p(qoff), C.byref(cfg) if cfg is not None else None,
                                0, C.byref(h))
        assert rc != 0 or L.poa_device_count() > 0
        if rc == 0:
            L.poa_multi_destroy(h)
        return rc

    assert footprint() == 0 and total.value > 0
    bad0 = gq.copy(); bad0[0] = 1
    down = gq.copy(); down[1], down[2] = gq[2], gq[1]
    assert down[2] < down[1]
    hole = (C.c_void_p * len(dgs))(*[d.handle for d in dgs])
    hole[3] = None
    for what, kw in (("graph_qoff[0] != 0", dict(gqoff=bad0)), ("graph_qoff decreasing", dict(gqoff=down)), ("null graph", dict(hs=hole))):
        for call in (footprint, create):
            assert call(**kw) == ERR_INVALID_ARG, (what, call.__name__)
            assert L.poa_last_error() != b"", what
    for mode in ("dense", "exact", "hybrid", "score", "checkpoint2"):
        for call in (footprint, create):
            assert call(cfg=aligner.make_config(mode)) == ERR_UNSUPPORTED, mode
            assert L.poa_last_error() != b""
    ef = aligner.make_config("checkpoint", aln_type=aligner.AlignmentType.EndsFree())
    assert footprint(cfg=ef) == ERR_UNSUPPORTED and create(cfg=ef) == ERR_UNSUPPORTED
    # null handles of the batch itself
    st = _lib.PoaStats()
    c = _lib.PoaCosts(4, 6, 2, 0)
    assert L.poa_multi_run(None, C.byref(c), None, None) == ERR_INVALID_ARG
    assert L.poa_multi_fetch(None, None, None, None, 0, None, None) == ERR_INVALID_ARG
    assert L.poa_multi_stats(None, C.byref(st)) == ERR_INVALID_ARG
    assert L.poa_multi_workspace_bytes(None, C.byref(total)) == ERR_INVALID_ARG
    assert L.poa_multi_device_results(None, None, None, None, None) == ERR_INVALID_ARG
    L.poa_multi_destroy(None)
    # the binding knows the query count and checks graph_qoff[n_graphs] against it
    short = gq.copy(); short[-1] -= 1
    try:
        aligner.multi_footprint(graphs, graph_qoff=short, qseq=qseq, qoff=qoff)
        raise AssertionError("graph_qoff[n_graphs] != query count was accepted")
    except ValueError:
        pass


def test_multi_abi_symbols_declared_exported_bound():
    from poasta_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poasta_amd.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    declared = sorted(set(re.findall(r"\b(poa_(?:multi_[a-z_]+|align_multi))\s*\(", hdr)))
    assert declared == sorted(MULTI_SYMBOLS)
    for name in MULTI_SYMBOLS:
        assert hasattr(raw, name), "libpoasta_amd.so does not export %s" % name
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name).argtypes is not None, name
    assert re.search(r"typedef\s+struct\s+poa_multi\s+poa_multi_t\s*;", hdr)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in MULTI_SYMBOLS:
        assert name in integration, name


def test_multi_host_plan_under_sanitizers(tmp_path):
    """tests/multi_host: offsets in bounds, regions disjoint, chunk coverage exact — a program of its own, address and
    undefined-behaviour sanitizers on, on the CPU."""
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    exe = os.path.join(str(tmp_path), "multi_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "multi_host", "multi_host.cpp"), os.path.join(csrc, "poa_multi_plan.cpp"),
                           os.path.join(csrc, "poa_sweep_rows.cpp"), os.path.join(csrc, "poa_graph.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"multi_host ok" in r.stdout
