"""Check rows of a capped score-set run (poa_graph_sweep_checks) against a restatement of their definition: row r is a cut row
if no edge (u, v) has row(u) < r < row(v); the check rows are the cut rows without the end row, thinned greedily in row order
so that two consecutive ones lie at least `stride` rows apart.  Host only."""
import ctypes as C

import numpy as np

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder

ACGT = np.frombuffer(b"ACGT", np.uint8)
DEFAULT_STRIDE = 8   # include/poasta_amd.h: stride 0


def _edge_rows(g, dg):
    rows = dg.node_rows()
    return [(int(rows[u]), int(rows[v])) for u in range(g.n) for v in g.successors(u)]


def _cut_rows(g, dg):
    """The definition, edge by edge."""
    edges = _edge_rows(g, dg)
    assert all(a < b for a, b in edges)
    return [r for r in range(g.n) if not any(a < r < b for a, b in edges)]


def _expected(g, dg, stride):
    stride = stride or DEFAULT_STRIDE
    check = np.zeros(g.n, np.uint8)
    last = None
    for r in _cut_rows(g, dg):
        if r == g.n - 1:
            continue   # the end row: the result is written there anyway
        if last is None or r - last >= stride:
            check[r] = 1
            last = r
    return check


def _verify(g, dg=None):
    from poasta_amd import aligner
    dg = dg or aligner.DeviceGraph(g)
    assert int(dg.node_rows()[g.end]) == g.n - 1 and int(dg.node_rows()[g.start]) == 0
    out = {}
    for stride in (1, 4, 0):
        got = dg.sweep_checks(stride)
        want = _expected(g, dg, stride)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (stride, got.tolist(), want.tolist())
        out[stride] = got
    assert np.array_equal(aligner.sweep_checks(dg, 1), out[1])
    return out


def _chain(seq):
    b = GraphBuilder()
    b.add_path(seq)
    return b.finish()


def test_chain_every_row_is_a_cut():
    g = _chain(np.random.default_rng(1).choice(ACGT, 30))
    out = _verify(g)
    assert out[1][:-1].all() and out[1][-1] == 0 and g.n == 32
    assert np.flatnonzero(out[4]).tolist() == list(range(0, 31, 4))
    assert np.flatnonzero(out[0]).tolist() == list(range(0, 31, DEFAULT_STRIDE))


def test_bubble_rows_inside_are_no_cuts():
    from poasta_amd import aligner
    rng = np.random.default_rng(2)
    b = GraphBuilder()
    back = b.add_path(rng.choice(ACGT, 12))
    br = b.add_path(rng.choice(ACGT, 3))
    b.add_edge(back[3], br[0])
    b.add_edge(br[-1], back[7])
    g = b.finish()
    dg = aligner.DeviceGraph(g)
    out = _verify(g, dg)
    rows = dg.node_rows()
    # the rows of both branches, between the fork and the join, are skipped by the other branch's edges
    inside = [int(rows[v]) for v in list(back[4:7]) + list(br)]
    assert not out[1][inside].any()
    for v in (back[0], back[3], back[7], back[11]):
        assert out[1][int(rows[v])] == 1
    assert 0 < out[1].sum() < g.n - 1


def test_edge_from_start_to_a_late_node():
    from poasta_amd import aligner
    rng = np.random.default_rng(3)
    b = GraphBuilder()
    back = b.add_path(rng.choice(ACGT, 16))
    g0 = b.finish()
    # the same chain with one more edge out of the start node, straight to node 12 of the backbone
    succ = [list(g0.successors(u)) for u in range(g0.n)]
    succ[g0.start].append(int(back[12]))
    g = _from_succ(g0, succ)
    dg = aligner.DeviceGraph(g)
    out = _verify(g, dg)
    r12 = int(dg.node_rows()[back[12]])
    assert out[1][0] == 1 and not out[1][1:r12].any() and out[1][r12:-1].all()


def _from_succ(g0, succ):
    from poasta_amd.graph import FlatGraph
    n = g0.n
    pred = [[] for _ in range(n)]
    for u in range(n):
        for v in succ[u]:
            pred[v].append(u)
    off = lambda lists: np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    flat = lambda lists: np.array([v for x in lists for v in x], np.uint32)
    return FlatGraph.from_dict(dict(n=n, start=g0.start, end=g0.end, symbol=np.asarray(g0.symbol, np.uint8), succ_off=off(succ),
                                    succ=flat(succ), pred_off=off(pred), pred=flat(pred)))


def test_random_dags():
    rng = np.random.default_rng(4)
    shares = []
    for seed in range(200):
        g = W.random_dag(900 + seed, n_nodes=int(rng.integers(5, 61)), p_edge=float(rng.choice([0.05, 0.1, 0.3])),
                         alphabet=b"AC" if seed % 2 else b"ACGT")
        out = _verify(g)
        shares.append(out[1].sum() / g.n)
    assert min(shares) < 0.3 and max(shares) > 0.5   # (the graphs range from tangled to chain-like)
    _verify(GraphBuilder().finish())


def test_checks_follow_graph_update():
    from poasta_amd import _lib, aligner
    g0 = W.random_dag(7, n_nodes=20, p_edge=0.3)
    dg = aligner.DeviceGraph(g0)
    _verify(g0, dg)
    for seed in (11, 12, 13):
        g1 = W.random_dag(seed, n_nodes=10 + seed, p_edge=0.1)
        _lib.check(_lib.lib().poa_graph_update(dg.handle, g1.n, g1.start, g1.end, aligner._p(g1.symbol), aligner._p(g1.succ_off),
                                               aligner._p(g1.succ), aligner._p(g1.pred_off), aligner._p(g1.pred)))
        dg.graph = g1
        _verify(g1, dg)
    # the count alone (check = NULL), and the null arguments
    n = C.c_uint32(123)
    _lib.check(_lib.lib().poa_graph_sweep_checks(dg.handle, 1, None, C.byref(n)))
    assert n.value == int(dg.sweep_checks(1).sum())
    assert _lib.lib().poa_graph_sweep_checks(None, 1, None, C.byref(n)) == -1
    assert _lib.lib().poa_graph_sweep_checks(dg.handle, 1, None, None) == -1


def test_capped_run_symbols_declared_exported_bound():
    """include/poasta_amd_scoreset_cap.h — the capped runs' part of the C ABI, included by include/poasta_amd.h — against the
    library and the binding, as tests/test_cpu_side.py holds the main header to its list."""
    import os
    import re
    from poasta_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cap_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "poasta_amd_scoreset_cap.h")).read(), flags=re.S)
    main_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "poasta_amd.h")).read(), flags=re.S)
    assert re.search(r'#include\s+"poasta_amd_scoreset_cap\.h"', main_h) and re.search(r'#include\s+"poasta_amd\.h"', cap_h)
    declared = sorted(set(re.findall(r"\b(poa_[a-z0-9_]+)\s*\(", cap_h)))
    assert declared == sorted(_lib.EXPORTS_SCORESET_CAP) and len(declared) == 3
    raw = C.CDLL(_lib.LIB_PATH)
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    for name in declared + ["poa_graph_sweep_checks"]:
        assert hasattr(raw, name), "libpoasta_amd.so does not export %s" % name
        assert getattr(_lib.lib(), name).argtypes is not None and name in integration, name
    assert re.search(r"#define\s+POA_FLAG_CAPPED\s+0x80u", main_h) and _lib.FLAG_CAPPED == 0x80
    assert _lib.TUNE_KEYS.index("CAP_STRIDE") == 31 and re.search(r"POA_TUNE_CAP_STRIDE,[^\n]*\n\s*POA_TUNE_COUNT = 32", open(os.path.join(root, "include", "poasta_amd.h")).read())
