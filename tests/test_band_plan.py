"""The band plan of the banded one-strip forward pass (poasta_amd/csrc/poa_band_plan.cpp), compiled for the host and checked
against the oracle's dense planes, for EVERY cell and each of the three states:

  * value >= e * ds                      (ds = dist(j, [a_min, a_max]) from the plan's own tables);
  * value + e * de <= e * D  =>  the cell lies inside the window of its row's segment, D and the windows being the plan's
                                         (de = dist(L - j, [c_min, c_max]), the tight interval);
  * the columns the plan takes for ds + de <= D are exactly those a brute-force evaluation gives, and they fit the windows.

No cell is left out: every row of the test graphs lies on a start -> end path, and the test counts the cells itself.  The graphs
are small, so the plan runs with a small window and short segments — the same code as for 512 columns and 64 rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from poasta_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
INF = 0xFFFFFFFF
COSTS = [(4, 6, 2), (2, 8, 1), (1, 10, 2), (3, 1, 1), (4, 4, 2), (4, 0, 2), (4, 0, 1), (255, 3, 1), (255, 6, 2), (1, 0, 1)]   # tests/test_derived_gap_flags.py


def _p(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def harness():
    src = os.path.join(ROOT, "tests", "band_host", "band_host.cpp")
    out = os.path.join(ROOT, "tests", "band_host", "libband_host.so")
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("poa_band_plan.cpp", "poa_band_plan.hpp", "poa_graph.cpp", "poa_graph.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, src, os.path.join(csrc, "poa_band_plan.cpp"),
                               os.path.join(csrc, "poa_graph.cpp")])
    X = C.CDLL(out)
    X.band_host_plan.argtypes = [C.c_uint32] * 3 + [vp] * 5 + [C.c_uint32] * 3 + [vp] * 4
    X.band_host_intervals.argtypes = [C.c_uint32] * 3 + [vp] * 5 + [C.c_uint32] * 2 + [vp] * 2
    return X


def _dist(v, lo, hi):
    return np.maximum(0, np.maximum(lo - v, v - hi))


class Plan:
    def __init__(self, X, g, L, seg_rows, window):
        d = g.as_dict()
        self.arrs = [np.ascontiguousarray(d[k], dtype=(np.uint8 if k == "symbol" else np.uint32)) for k in ("symbol", "succ_off", "succ", "pred_off", "pred")]
        self.head = (int(d["n"]), int(d["start"]), int(d["end"]))
        n = self.head[0]
        hdr = np.zeros(2, np.uint32)
        bases = np.zeros((n + seg_rows - 1) // seg_rows, np.uint32)
        node_row = np.zeros(n, np.uint32)
        tabs = np.zeros((4, n), np.uint32)
        assert X.band_host_plan(*self.head, *[_p(a) for a in self.arrs], L, seg_rows, window, _p(hdr), _p(bases), _p(node_row), _p(tabs)) == 0
        assert int(hdr[1]) == len(bases)
        self.X, self.n, self.L, self.seg_rows, self.window = X, n, L, seg_rows, window
        self.D, self.bases, self.node_row = int(hdr[0]), bases.astype(np.int64), node_row.astype(np.int64)
        assert (tabs != INF).all(), "a row of the test graph lies on no start -> end path: its cells would be left out"
        a_min, a_max, c_min, c_max = (tabs[k].astype(np.int64)[:, None] for k in range(4))
        j = np.arange(L + 1, dtype=np.int64)[None, :]
        self.ds = _dist(j, a_min, a_max)              # [row][column]
        self.de = _dist(L - j, c_min, c_max)
        self.row_base = self.bases[np.arange(n) // seg_rows][:, None]
        self.in_window = (j >= self.row_base) & (j < self.row_base + window)
        assert (self.bases % 8 == 0).all()

    def intervals(self, D):
        lo, hi = np.zeros(self.n, np.uint32), np.zeros(self.n, np.uint32)
        assert self.X.band_host_intervals(*self.head, *[_p(a) for a in self.arrs], self.L, D, _p(lo), _p(hi)) == 0
        return lo.astype(np.int64), hi.astype(np.int64)


def _check_band_columns(pl):
    """the plan's closed form for { j : ds + de <= D } against a brute-force evaluation, and the fit of band(D) (not of band(D + 1))"""
    j = np.arange(pl.L + 1, dtype=np.int64)[None, :]
    for D in sorted({0, 1, 2, 3, 7, pl.D, pl.D + 1, pl.D // 2, 2 * pl.D + 5}):
        lo, hi = pl.intervals(D)
        want = (pl.ds + pl.de) <= D
        got = (j >= lo[:, None]) & (j <= hi[:, None])
        assert np.array_equal(want, got), D
        if D <= pl.D and pl.D > 0:
            assert (want <= pl.in_window).all(), D
    if pl.D < 65535:
        # the plan's D is the largest that fits: at D + 1 some segment's rows span more than any aligned window holds
        want = (pl.ds + pl.de) <= pl.D + 1
        fits = True
        for s in range(len(pl.bases)):
            cols = np.nonzero(want[s * pl.seg_rows:(s + 1) * pl.seg_rows].any(axis=0))[0]
            if len(cols) and cols[-1] - (cols[0] // 8) * 8 >= pl.window:
                fits = False
        assert not fits


def _check_every_cell(X, oracle, g, qs, costs_list, seg_rows, window):
    """-> (cells checked, cells that had to lie inside a window)"""
    og = oracle.OracleGraph.from_csr(g.as_dict())
    orank = og.export_csr()["rank"]
    n_cells = n_must = 0
    for q in qs:
        q = np.ascontiguousarray(q, np.uint8)
        pl = Plan(X, g, len(q), seg_rows, window)
        _check_band_columns(pl)
        node_of_row = np.argsort(pl.node_row)
        for costs in costs_list:
            x, o, e = costs
            od = og.dense_align(q, oracle.Costs(*costs), planes=True)
            for name in ("M", "I", "D"):
                v = np.ascontiguousarray(od[name][orank])[node_of_row].astype(np.int64)    # by row
                assert v.shape == pl.ds.shape
                fin = v != INF
                assert (v[fin] >= e * pl.ds[fin]).all(), (name, costs, len(q))
                must = fin & (v + e * pl.de <= e * pl.D)
                if pl.D >= 2:
                    assert (must <= pl.in_window).all(), (name, costs, len(q), pl.D)
                n_cells += v.size
                n_must += int(must.sum())
    return n_cells, n_must


def test_linearish_graphs(harness, oracle):
    total = must = 0
    for seed, (nb, ns, ni) in enumerate(((300, 15, 8), (200, 30, 20), (260, 5, 25))):
        g, (qseq, qoff) = W.scaled_linearish(nb, ns, ni, 6, nb + 20, graph_seed=seed + 1, p_sub=0.05, p_ins=0.03, p_del=0.03)
        qs = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(6)]
        qs = [qs[0], qs[1][:30], np.concatenate([qs[2], qs[3][:40]]), qs[4][:nb - 25]]   # a stub, an over-long read, a short one
        c, m = _check_every_cell(harness, oracle, g, qs, COSTS, seg_rows=16, window=64)
        total += c; must += m
        n = g.as_dict()["n"]
        assert c == 3 * len(COSTS) * sum(int(n) * (len(q) + 1) for q in qs)   # no cell left out
    assert must > 100000


def test_bubble_rich_graphs(harness, oracle):
    rows = [b"ACGT-ACGTTGCA--ACGTAC", b"ACGTTACG-TGCAGGACGTAC", b"AC-T-ACGTTGAA--ACG-AC", b"ACGTTACCTTGCAG-ACGTAC"]
    g = W.msa_to_graph(rows)
    qs = [np.frombuffer(r.replace(b"-", b""), np.uint8) for r in rows] + [np.frombuffer(b"ACGTACGTGGGGACGTACACGTACGTAACC", np.uint8), np.frombuffer(b"TTTT", np.uint8)]
    c, m = _check_every_cell(harness, oracle, g, qs, COSTS, seg_rows=4, window=16)
    assert c == 3 * len(COSTS) * sum(int(g.as_dict()["n"]) * (len(q) + 1) for q in qs) and m > 1000
    lay = W.LayeredPOA(n_layers=70, width=4, indeg=4, seed=5)
    qs = lay.queries(3, length=0) + [lay.queries(1, length=0, seed=8)[0][:20], np.concatenate(lay.queries(2, length=0, seed=9))[:110]]
    c, m = _check_every_cell(harness, oracle, lay.graph, qs, COSTS, seg_rows=32, window=32)
    assert c == 3 * len(COSTS) * sum(int(lay.graph.as_dict()["n"]) * (len(q) + 1) for q in qs) and m > 5000
    poa = W.PangenomePOA(ref_len=300, n_hap=6, p_snp=0.02, p_indel=0.01, max_indel=6, seed=4)
    qs = poa.queries(3, length=120) + poa.queries(2, length=330, seed=9)
    c, m = _check_every_cell(harness, oracle, poa.graph, qs, [(4, 6, 2), (4, 0, 2), (1, 0, 1), (255, 3, 1)], seg_rows=64, window=128)
    assert m > 5000


def test_headline_shape_fits(harness):
    """the 1 002-row graph of the headline workload with 1 kbp reads: the 512-column windows of 64-row segments hold a band wide
    enough for every score up to e * (D - 2) with D in the hundreds"""
    g, (qseq, qoff) = W.config2(n_queries=4)
    for L in (1000, 980, 1015):
        pl = Plan(harness, g, L, 64, 512)
        assert pl.D >= 300, pl.D
        assert (np.diff(pl.bases) >= 0).all() and pl.bases[0] == 0
        _check_band_columns(pl)
    assert Plan(harness, g, 400, 64, 512).D == 65535          # everything fits: no bound at all
