"""The banded one-strip forward kernel (poasta_amd/csrc/poa_forward_band.hpp) and its fallback to the full kernel: every case
compares score, flags, pair_off and pairs bit for bit with the same batch under POA_BAND=0 and with the oracle's dense batch, and
says through poa_batch_band_info which path the queries took.  Which queries the banded pass certifies is no matter of luck: a
query is kept exactly if the oracle's score is <= e * (D - 4), D the host plan's band distance for its length (tests/band_host,
the harness of tests/test_band_plan.py) capped by POA_BAND_DELTA, so every case asserts the exact split and the smallest D.
Those path assertions are skipped only when the environment carries one of the overrides that take the batch to another
forward kernel (scripts/variant_sweep.sh); the results are compared in every case.  Shapes: the smallest that reach the kernel
(more than 512 plane columns) and cross several 64-row segments."""
import os

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries
from test_band_plan import Plan, harness   # noqa: F401  (the host build of the band plan)

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _run(engine, g, qseq, qoff, costs, env, first=None):
    """costs = (mismatch, open, extend); first = (costs, env): a run of the same batch before the one that is fetched"""
    def one(rb, costs, env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            rb.run(engine.GapAffine(costs[0], costs[2], costs[1]))
            return rb.fetch(), rb.band_info()
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    rb = engine.ResidentBatch(g, qseq, qoff)
    try:
        if first is not None:
            one(rb, *first)
        return one(rb, costs, env)
    finally:
        rb.close()


def _same(a, b):
    return (np.array_equal(a.score, b.score) and np.array_equal(a.flags, b.flags) and np.array_equal(a.pair_off, b.pair_off)
            and np.array_equal(a.pairs, b.pairs))


def _overridden():
    """an override that reroutes the one-strip dense pass (or the banded kernel itself) is set for the whole session"""
    return any(k in os.environ for k in ("POA_BAND", "POA_BAND_DELTA", "POA_MF", "POA_PX", "POA_PLANES", "POA_COMPACT", "POA_PACKED",
                                         "POA_RELATIVE", "POA_FWD_QUADS", "POA_FUSE_TB"))


class Case:
    """a batch, its full-kernel result and the oracle's dense batch, computed once"""
    def __init__(self, engine, oracle, g, qs, costs=(4, 6, 2)):
        self.engine, self.oracle, self.g, self.qs, self.costs = engine, oracle, g, qs, costs
        self.qseq, self.qoff = pack_queries(qs)
        self.full, info = _run(engine, g, self.qseq, self.qoff, costs, {"POA_BAND": "0"})
        assert not info["used"]
        og = oracle.OracleGraph.from_csr(g.as_dict())
        self.D = og.dense_batch(self.qseq, self.qoff, oracle.Costs(*costs), threads=4)
        self.check(self.full)

    def check(self, r):
        assert _same(r, self.full)
        assert np.array_equal(r.score, self.D["score"]) and np.array_equal(r.flags, self.D["flags"])
        for i in range(len(self.qs)):
            assert r.raw_alignment(i) == self.oracle.batch_alignment(self.D, i), i

    def banded(self, X, env=None, first=None):
        """run banded, compare the results, and assert the split that the plan's D and the oracle's scores predict"""
        r, info = _run(self.engine, self.g, self.qseq, self.qoff, self.costs, env or {}, first)
        self.check(r)
        cap = int((env or {}).get("POA_BAND_DELTA", 1 << 30))
        e = self.costs[2]
        d_of = {L: min(Plan(X, self.g, L, 64, 512).D, cap) for L in {len(q) for q in self.qs}}
        keep = [d_of[len(q)] >= 4 and int(s) <= min(e * (d_of[len(q)] - 4), 0x3FFE) for q, s in zip(self.qs, self.D["score"])]
        want = {"used": True, "banded": sum(keep), "fell_back": len(keep) - sum(keep), "min_d": min(d_of.values())}
        if not _overridden():
            assert info == want, (info, want)
        return want


def _linearish(n_queries=24, **err):
    g, (qseq, qoff) = W.scaled_linearish(560, 28, 14, n_queries, 600, **err)
    return g, [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(n_queries)]


def _bubble_graph(seed=11, n_backbone=520):
    """about 600 rows: SNP nodes, two-node branches and edges that skip up to six backbone nodes, spread over the whole
    backbone so that predecessor rows are read from memory on both sides of segment boundaries"""
    rng = np.random.default_rng(seed)
    backbone = ACGT[rng.integers(0, 4, n_backbone)]
    b = GraphBuilder()
    ids = b.add_path(backbone)
    for i in range(4, n_backbone - 8, 9):
        kind = (i // 9) % 3
        if kind == 0:
            v = b.add_node(int(ACGT[rng.integers(0, 4)]))
            b.add_edge(ids[i - 1], v); b.add_edge(v, ids[i + 1])
        elif kind == 1:
            v1, v2 = b.add_node(int(ACGT[rng.integers(0, 4)])), b.add_node(int(ACGT[rng.integers(0, 4)]))
            b.add_edge(ids[i], v1); b.add_edge(v1, v2); b.add_edge(v2, ids[i + 1])
        else:
            b.add_edge(ids[i], ids[i + int(rng.integers(2, 7))])
    g = b.finish()
    qs = []
    for k in range(16):
        q = W.mutate(rng, backbone, 0.03, 0.01, 0.01)
        qs.append(np.concatenate([q, ACGT[rng.integers(0, 4, 40)]])[:int(rng.integers(530, 570))])
    return g, qs


@pytest.fixture(scope="module")
def linearish(engine, oracle):
    g, qs = _linearish()
    return Case(engine, oracle, g, qs)


def test_default_run_certifies_every_query(linearish, harness):
    want = linearish.banded(harness)
    assert want["fell_back"] == 0 and want["banded"] == len(linearish.qs)


def test_bubble_graph_across_segments(engine, oracle, harness):
    g, qs = _bubble_graph()
    assert g.as_dict()["n"] > 9 * 64
    want = Case(engine, oracle, g, qs).banded(harness)
    assert want["banded"] == len(qs)
    # deep bubbles: 600 rows in layers of four, short reads padded to the one-strip kernel by one long query
    poa = W.LayeredPOA(n_layers=150, width=4, indeg=4, seed=5)
    qs = poa.queries(10, length=0)
    qs.append(np.concatenate([qs[0]] * 5)[:600])
    want = Case(engine, oracle, poa.graph, qs).banded(harness)
    assert want["banded"] >= 10


def test_forced_fallback(linearish, harness):
    for cap in ("4", "0"):   # T = 0: every wave computes its band and fails the test; no band at all: the waves only queue
        want = linearish.banded(harness, {"POA_BAND_DELTA": cap})
        assert want["banded"] == 0


def test_mixed_chunk_takes_both_paths(engine, oracle, harness):
    g, clean = _linearish(12)
    _, divergent = _linearish(12, query_seed=7, p_sub=0.10, p_ins=0.05, p_del=0.05)
    case = Case(engine, oracle, g, [q for pair in zip(clean, divergent) for q in pair])
    score = case.D["score"].astype(np.int64)
    lo, hi = int(score[0::2].max()), int(score[1::2].min())
    assert lo + 8 < hi, (lo, hi)   # the oracle's scores alone separate the two kinds of read
    e = case.costs[2]
    cap = ((lo + hi) // 2) // e + 4   # T = e * (cap - 4) lies between them
    want = case.banded(harness, {"POA_BAND_DELTA": str(cap)})
    assert want["min_d"] == cap and want["banded"] == 12 and want["fell_back"] == 12, want   # every length's own D is wider than the cap


def test_varied_lengths_in_one_chunk(engine, oracle, harness):
    g, (qseq, qoff) = W.scaled_linearish(880, 40, 20, 8, 1000, p_sub=0.04, p_ins=0.02, p_del=0.02)
    full = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(8)]
    qs = [full[0], full[1][:520], full[2][:600], full[3][:777], full[4][:900], full[5][:100], full[6][:1000], full[7][:512], full[0][:960],
          full[1][:1023]]
    want = Case(engine, oracle, g, qs).banded(harness)
    assert want["banded"] >= 4 and want["fell_back"] >= 1, want   # both paths in one chunk, by the plan and the oracle alone


def test_stale_planes_of_an_earlier_run(linearish, harness):
    # the planes hold a full run under other costs; the banded run writes its windows only and must not read the rest
    want = linearish.banded(harness, {}, first=((3, 1, 1), {"POA_BAND": "0"}))
    assert want["fell_back"] == 0
    linearish.banded(harness, {"POA_BAND_DELTA": "60"}, first=((3, 1, 1), {}))


@pytest.mark.parametrize("costs", [(4, 0, 2), (255, 3, 1)])
def test_other_costs(engine, oracle, harness, costs):
    g, qs = _linearish(12)
    want = Case(engine, oracle, g, qs, costs).banded(harness)
    assert want["banded"] == len(qs), want
