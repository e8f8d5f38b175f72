"""The paired banded forward pass (poa_forward_band2_kernel in poasta_amd/csrc/poa_forward_band.hpp): two queries of one length per
wave, query A in the low and query B in the high 16-bit half of every register.  It must store what poa_forward_band_kernel<false>
stores, cell for cell, so the cases are those of tests/test_band_forward.py and tests/test_compact_planes.py with POA_BAND_PAIR=1:
results against the unpaired run, the full kernel and the oracle; every window cell against the windowed model of
tests/band_model.py, every other cell against what was there before; band_info against the plan's D and the oracle's scores.

Who pairs is predicted here from the lengths and the plan alone (_pairing: within the chunk, in query order, every second query of a
length whose D is >= 4 joins the waiting one) and compared with poa_batch_band_pair_info in every case.  Batches are one chunk of
at most 16 reads of 512..1023 bases (the default rule leaves such chunks unpaired: the override forces the kernel); the rule itself
is checked from both sides on a graph of four rows."""
import os

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries
from band_model import fork_graph
from test_band_forward import _overridden, _same
from test_band_plan import Plan, harness   # noqa: F401  (the host build of the band plan)
from test_compact_planes import ACGT, SEG_ROWS, WINDOW, Batch, _environ, _reads, _snp_graph

pytestmark = pytest.mark.gpu
PAIR = {"POA_BAND_PAIR": "1"}


def _pairing(lengths, d_of):
    """-> (pairs [(a, b)], singles [i]) of one chunk, as prepare_band_pairs of poa_engine.hip forms them (launch_band launches them)"""
    waiting, pairs, singles = {}, [], []
    for i, L in enumerate(lengths):
        if d_of[L] < 4:
            singles.append(i)
        elif L in waiting:
            pairs.append((waiting.pop(L), i))
        else:
            waiting[L] = i
    return pairs, sorted(singles + list(waiting.values()))


def _check_pair_info(b, X, rb, want_pairs=None):
    pairs, singles = _pairing([len(q) for q in b.qs], {len(q): b.plan(X, len(q)).D for q in b.qs})
    if want_pairs is not None:
        assert pairs == want_pairs, pairs
    info = rb.band_pair_info()
    if not _overridden():
        assert (info["paired"], info["single"], info["ran_paired"]) == (2 * len(pairs), len(singles), bool(pairs)), (info, pairs, singles)
    return pairs, singles


def _paired_case(b, X, costs=(4, 6, 2), env=None, want_pairs=None, stale_costs=None, want_keep=None):
    """a paired run (after a full run under stale_costs, if given): cells, band_info, results (Batch.check_banded), pair_info"""
    env = {**PAIR, **(env or {})}
    rb = b.open()
    try:
        stale = None
        if stale_costs is not None:
            b.run(rb, stale_costs, {"POA_BAND": "0"})
            stale = b.check_full(rb, stale_costs)
        b.run(rb, costs, env)
        want, keep = b.check_banded(X, rb, costs, env, stale=stale, want_keep=want_keep)
        _check_pair_info(b, X, rb, want_pairs)
        return want, keep
    finally:
        rb.close()


def _substituted(rng, q, n):
    """q with n substitutions: another read of the same length"""
    q = q.copy()
    at = rng.choice(len(q), n, replace=False)
    q[at] = ACGT[(np.searchsorted(ACGT, q[at]) + rng.integers(1, 4, n)) % 4]
    return q


# ---- 1. pairs and singles in one chunk ----------------------------------------------------------------------------------------------
def test_pairs_and_singles_in_one_chunk(engine, oracle, harness):
    g, full = _reads(W.scaled_linearish(560, 28, 14, 8, 600), 8)
    lens = [540, 540, 540, 540, 540, 531, 531, 522]
    assert min(len(q) for q in full) >= 540
    b = Batch(engine, oracle, g, [q[:L] for q, L in zip(full, lens)])
    rb = b.open()
    try:
        runs = {}
        for name, env in (("full", {"POA_BAND": "0"}), ("single", {"POA_BAND_PAIR": "0"}), ("paired", PAIR)):
            res = b.run(rb, (4, 6, 2), env)
            b.check_results()
            runs[name] = (res, rb.band_info(), rb.band_pair_info())
        assert _same(runs["paired"][0], runs["single"][0]) and _same(runs["paired"][0], runs["full"][0])
        _check_pair_info(b, harness, rb, want_pairs=[(0, 1), (2, 3), (5, 6)])      # singles: 4 and 7
        if not _overridden():
            assert runs["paired"][1] == runs["single"][1] and runs["paired"][1]["used"] and not runs["full"][1]["used"]
            assert runs["paired"][1]["banded"] == 8, runs["paired"][1]
            assert (runs["paired"][2]["paired"], runs["paired"][2]["single"]) == (6, 2)
            assert (runs["single"][2]["paired"], runs["single"][2]["single"], runs["single"][2]["ran_paired"]) == (0, 8, False)
            assert (runs["full"][2]["paired"], runs["full"][2]["single"]) == (0, 0)
        b.check_banded(harness, rb, (4, 6, 2), PAIR)      # the planes of the last, paired, run
    finally:
        rb.close()


# ---- 2. cells: both members, both orders, a second cost set ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_reads():
    g, full = _reads(W.scaled_linearish(560, 28, 14, 2, 600), 2)
    L = min(len(q) for q in full) - 3
    return g, [full[0][:L], full[1][:L]]


@pytest.mark.parametrize("costs", [(4, 6, 2), (4, 0, 2)])
@pytest.mark.parametrize("swap", [False, True])
def test_paired_run_writes_window_cells_only(engine, oracle, harness, two_reads, swap, costs):
    g, qs = two_reads
    b = Batch(engine, oracle, g, qs[::-1] if swap else qs)
    want, keep = _paired_case(b, harness, costs, want_pairs=[(0, 1)], stale_costs=(3, 1, 1))
    assert all(keep), want
    for i in range(2):
        assert 2 * int((~b.window(harness, i)).any(axis=1).sum()) >= b.g.n      # cells outside the windows in at least half the rows


# ---- 3. one half fails ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("failing", ["A", "B"])
def test_one_member_falls_back(engine, oracle, harness, failing):
    g, clean = _reads(W.scaled_linearish(560, 28, 14, 1, 600), 1)
    _, divergent = _reads(W.scaled_linearish(560, 28, 14, 1, 600, query_seed=7, p_sub=0.10, p_ins=0.05, p_del=0.05), 1)
    L = min(len(clean[0]), len(divergent[0]))
    qs = [clean[0][:L], divergent[0][:L]]
    b = Batch(engine, oracle, g, qs[::-1] if failing == "A" else qs)
    score = b.dense((4, 6, 2))["score"].astype(np.int64)
    lo, hi = int(score.min()), int(score.max())
    assert lo + 8 < hi and (score[0] == hi) == (failing == "A"), score      # the oracle's scores alone tell the two reads apart
    cap = ((lo + hi) // 2) // 2 + 4                                         # T = e * (cap - 4) lies between them
    assert b.plan(harness, L).D > cap
    want, keep = _paired_case(b, harness, env={"POA_BAND_DELTA": str(cap)}, want_pairs=[(0, 1)], stale_costs=(3, 1, 1),
                              want_keep=[failing != "A", failing != "B"])
    # (Batch.check_banded: the failing read's planes equal the oracle's in every cell, the partner's window cells the model's and
    # its other cells what the run before left there)
    assert (want["banded"], want["fell_back"], want["min_d"]) == (1, 1, cap), want


def test_cap_takes_the_band_away(engine, oracle, harness, two_reads):
    """POA_BAND_DELTA below 4: the pair's wave only queues both reads for the full pass"""
    g, qs = two_reads
    want, keep = _paired_case(Batch(engine, oracle, g, qs), harness, env={"POA_BAND_DELTA": "0"}, want_pairs=[(0, 1)])
    assert not any(keep) and want["fell_back"] == 2


# ---- 4. window moves ------------------------------------------------------------------------------------------------------------------------
def test_windows_move_right(engine, oracle, harness):
    g, full = _reads(W.scaled_linearish(880, 40, 20, 4, 1000, p_sub=0.04, p_ins=0.02, p_del=0.02), 4)
    b = Batch(engine, oracle, g, [full[0][:900], full[1][:900], full[2][:777], full[3][:777]])
    for q in b.qs:
        assert (np.diff(b.plan(harness, len(q)).bases) > 0).sum() >= 3, b.plan(harness, len(q)).bases
    want, keep = _paired_case(b, harness, want_pairs=[(0, 1), (2, 3)])
    assert sum(keep) >= 2, want


def test_fork_graph_window_goes_back(engine, oracle, harness):
    g, walks = fork_graph(300, 150, 150, 200, seed=1)
    rng = np.random.default_rng(42)
    reads = [W.mutate(rng, walks[k % 2], 0.03, 0.01, 0.01) for k in range(4)]
    L = min(len(q) for q in reads)
    b = Batch(engine, oracle, g, [q[:L] for q in reads])      # each pair: one read of either branch
    assert (np.diff(b.plan(harness, L).bases) < 0).sum() >= 1, b.plan(harness, L).bases
    want, keep = _paired_case(b, harness, want_pairs=[(0, 1), (2, 3)])
    assert all(keep), want


def test_sibling_row_opens_a_segment(engine, oracle, harness):
    poa = W.LayeredPOA(n_layers=150, width=3, indeg=3, seed=5)
    qs = poa.queries(6, length=0)
    L = min(len(q) for q in qs)
    long_read = np.concatenate([qs[0]] * 5)[:600]      # pads the chunk to the one-strip kernel
    b = Batch(engine, oracle, poa.graph, [long_read, _substituted(np.random.default_rng(2), long_read, 9)] + [q[:L] for q in qs])
    layer_of_row = np.full(poa.graph.n, -1)
    layer_of_row[b.rows[poa.ids.reshape(-1)]] = np.repeat(np.arange(150), 3)
    starts = np.arange(SEG_ROWS, poa.graph.n, SEG_ROWS)
    assert ((layer_of_row[starts] >= 0) & (layer_of_row[starts] == layer_of_row[starts - 1])).any()
    want, keep = _paired_case(b, harness)
    pairs, singles = _pairing([len(q) for q in b.qs], {len(q): b.plan(harness, len(q)).D for q in b.qs})
    assert len(pairs) >= 3 and sum(keep) >= 6, (pairs, want)


# ---- 5. edges of a row -----------------------------------------------------------------------------------------------------------------------
def test_edge_lengths(engine, oracle, harness):
    """512: the smallest length that reaches the kernel (pitch 576); 575: L + 1 equals the pitch; 1023: pitch 1024"""
    g, full = _reads(W.scaled_linearish(880, 40, 20, 6, 1000, p_sub=0.04, p_ins=0.02, p_del=0.02), 6)
    tail = ACGT[np.random.default_rng(3).integers(0, 4, 2 * 60)].reshape(2, 60)
    qs = [full[0][:512], full[1][:575], np.concatenate([full[2], tail[0]])[:1023], full[3][:512], full[4][:575],
          np.concatenate([full[5], tail[1]])[:1023]]
    b = Batch(engine, oracle, g, qs)
    assert [len(q) for q in b.qs] == [512, 575, 1023] * 2
    _paired_case(b, harness, want_pairs=[(0, 3), (1, 4), (2, 5)], stale_costs=(3, 1, 1))


def test_non_acgt_symbols(engine, oracle, harness):
    """'N' rows take the path that computes the symbol masks of both reads instead of reading the tables"""
    g, backbone = _snp_graph(600, 20, 8, n_every=37)
    assert (g.symbol == ord("N")).sum() >= 20
    rng = np.random.default_rng(9)
    qs = []
    for k in range(2):
        q = W.mutate(rng, backbone, 0.02, 0.01, 0.01)[:590]
        q[rng.integers(0, len(q), 12)] = ord("N")
        twin = q.copy()
        twin[rng.integers(0, len(q), 12)] = ord("N")      # N's at other places than its partner's
        qs += [q, _substituted(rng, twin, 7) if k else twin]
    assert all(len(q) == 590 for q in qs)
    want, keep = _paired_case(Batch(engine, oracle, g, qs), harness, want_pairs=[(0, 1), (2, 3)])
    assert all(keep), want


def test_end_cell_in_every_register(engine, oracle, harness):
    """the certificate reads M[end][L] of both reads out of one register: window column L - bases[-1] in each of a lane's eight"""
    rng = np.random.default_rng(31)
    backbone = ACGT[rng.integers(0, 4, 640)]
    gb = GraphBuilder()
    ids = gb.add_path(backbone)
    starts = list(range(7, 640 - 6, 15))
    for i in starts:
        gb.add_edge(ids[i], ids[i + 6])
    g = gb.finish()
    skip = np.zeros(640, bool)
    for i in starts[::2]:      # a read that follows every second bypass
        skip[i + 1:i + 6] = True
    short = backbone[~skip]
    assert 531 <= len(short) <= 536, len(short)
    qs = []
    for L in range(529, 537):
        q = short[:L] if L <= len(short) else np.concatenate([short, backbone[:L - len(short)]])
        qs += [q, _substituted(rng, q, 5)]      # the partner scores otherwise: the halves must not be mixed up
    b = Batch(engine, oracle, g, qs)
    wc = [len(q) - int(b.plan(harness, len(q)).bases[-1]) for q in qs[::2]]
    assert sorted(w % 8 for w in wc) == list(range(8)) and 0 <= min(wc) and max(wc) < WINDOW, wc
    score = b.dense((4, 6, 2))["score"]
    assert (score[0::2] != score[1::2]).all(), score
    want, keep = _paired_case(b, harness, want_pairs=[(2 * k, 2 * k + 1) for k in range(8)])
    assert all(keep), want


# ---- 6. the rule from both sides --------------------------------------------------------------------------------------------------------
def test_default_rule_from_both_sides(engine, harness):
    """the default pairs a chunk from rule_count queries in pairs on: one chunk below it and one at it, on the smallest graph whose
    reads still have more than 512 plane columns"""
    gb = GraphBuilder()
    gb.add_path(ACGT[[0, 1, 2, 3]])
    g = gb.finish()
    assert Plan(harness, g, 512, SEG_ROWS, WINDOW).D >= 4
    read = ACGT[np.random.default_rng(1).integers(0, 4, 512)]
    rb = engine.ResidentBatch(g, *pack_queries([read, read]))
    try:
        with _environ({"POA_BAND_PAIR": "0"}):
            rb.run(engine.GapAffine(4, 2, 6))
        count = rb.band_pair_info()["rule_count"]
    finally:
        rb.close()
    assert 1024 <= count <= 10000 and count % 2 == 0, count
    for n, paired in ((count - 1, False), (count, True), (count + 1, True)):
        rb = engine.ResidentBatch(g, *pack_queries([read] * n))
        try:
            rb.run(engine.GapAffine(4, 2, 6))
            res, info, band = rb.fetch(), rb.band_pair_info(), rb.band_info()
            assert res.stats["n_chunks"] == 1 and (res.score == res.score[0]).all()
            if not _overridden() and "POA_BAND_PAIR" not in os.environ:
                assert band["used"] and band["banded"] + band["fell_back"] == n
                assert info == {"paired": 2 * (n // 2) if paired else 0, "single": n % 2 if paired else n, "rule_count": count,
                                "ran_paired": paired}, (n, info)
        finally:
            rb.close()
