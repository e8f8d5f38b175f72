"""The narrow tier of the paired banded forward pass (poa_forward_band2_kernel<6> in poasta_amd/csrc/poa_forward_band.hpp): the
paired pass over a window of 384 columns, six registers per row array, under the class's narrow plan (plan_band with that window,
the 512 plan's segments and base alignment), and the cascade behind it: a read the tier cannot certify runs the 512-column pass,
and the full pass after that.

Every case is one chunk of at most 16 reads of 512..1023 bases under POA_BAND_PAIR=1 POA_BAND_NARROW=1 (the default rule leaves
such chunks to the 512 kernels).  Which tier certifies a read follows from the two plans' D and the oracle's score alone (_tiers);
the stored words are then compared in this order: the cells of the windows of that tier against the windowed model of
tests/band_model.py, every other word against what a POA_BAND=0 run under other costs left there, then band_narrow_info and
band_info against the prediction, then scores, flags and alignments against the oracle.  For a read the 512 pass certified after
the narrow tier missed it, the cells of the narrow windows outside the 512 ones hold what the narrow pass stored and are left out.

A lane of the narrow kernel owns six columns = three dwords, and window bases are multiples of 8: each case below is named for
the place where a dword, not a whole lane, decides."""
import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder
from band_model import INF, fork_graph, in_window, windowed_planes
from test_band_forward import _overridden, _same
from test_band_pairs import _pairing, _substituted
from test_band_plan import Plan, harness   # noqa: F401  (the host build of the band plan)
from test_compact_planes import ACGT, SEG_ROWS, WINDOW, Batch, _assert_words, _cap, _reads, _snp_graph

pytestmark = pytest.mark.gpu
NARROW = 384      # poa_band_plan.hpp: BAND_WINDOW_NARROW
ENV = {"POA_BAND_PAIR": "1", "POA_BAND_NARROW": "1"}
COSTS, STALE_COSTS = (4, 6, 2), (3, 1, 1)


class NarrowBatch(Batch):
    """Batch with the narrow plan, model and windows beside the 512 ones"""
    def plan_n(self, X, L):
        key = ("n", L)
        if key not in self._plan:
            pl = Plan(X, self.g, L, SEG_ROWS, NARROW)
            assert np.array_equal(pl.node_row, self.rows)
            self._plan[key] = pl
        return self._plan[key]

    def model_n(self, X, i, costs):
        key = ("n", i, costs)
        if key not in self._model:
            q = self.qs[i]
            self._model[key] = windowed_planes(self.g, self.rows, q, costs, SEG_ROWS, NARROW, self.plan_n(X, len(q)).bases)
        return self._model[key]

    def window_n(self, X, i):
        L = len(self.qs[i])
        return in_window(self.g.n, L, SEG_ROWS, NARROW, self.plan_n(X, L).bases)


def _tiers(b, X, costs, cap, narrow=True):
    """-> (tier per read: "narrow" / "wide" / "full", band_narrow_info, band_info) of a run under ENV, from the plans' D, the
    oracle's scores and the pairing alone"""
    e = costs[2]
    lens = [len(q) for q in b.qs]
    pairs, singles = _pairing(lens, {L: b.plan(X, L).D for L in lens})
    paired = sorted(i for p in pairs for i in p)
    score = b.dense(costs)["score"]

    def certifies(D, s):
        D = min(D, cap)
        return D >= 4 and int(s) <= min(e * (D - 4), 0x3FFE)
    tiers, first_d, ran = [], [], []
    for i, L in enumerate(lens):
        in_tier = narrow and i in paired and b.plan_n(X, L).D >= 4
        first_d.append(min(b.plan_n(X, L).D if in_tier else b.plan(X, L).D, cap))
        if in_tier:
            ran.append(i)
        if in_tier and certifies(b.plan_n(X, L).D, score[i]):
            tiers.append("narrow")
        else:
            tiers.append("wide" if certifies(b.plan(X, L).D, score[i]) else "full")
    n_info = {"ran": len(ran), "certified": sum(tiers[i] == "narrow" for i in ran), "certified_512": sum(tiers[i] == "wide" for i in ran),
              "chosen_by": "override" if ran else None}
    info = {"used": True, "banded": sum(t != "full" for t in tiers), "fell_back": sum(t == "full" for t in tiers), "min_d": min(first_d)}
    return tiers, n_info, info


def _check(b, X, rb, costs, env, stale=None, narrow=True):
    """the planes, the two info records and the results of the run that just ended -> the tiers"""
    tiers, n_info, info = _tiers(b, X, costs, _cap(env), narrow)
    for i, tier in enumerate(tiers):
        if tier == "full":
            b.check_full(rb, costs, [i], results=False)
            continue
        f = rb.compact_planes(i)
        assert np.array_equal(f[2], b.kept), i
        b.true(i, costs)      # (asserts that the oracle's finite values fit the score field)
        win = b.window_n(X, i) if tier == "narrow" else b.window(X, i)
        planes = b.model_n(X, i, costs) if tier == "narrow" else b.model(X, i, costs)
        for p in (planes[0], planes[2]):
            assert int(p[p != INF].max()) < 0x3FFF
        _assert_words(f, planes, win, "query %d, the %s windows' cells against the model" % (i, tier))
        if stale is not None:
            written = win | b.window_n(X, i) if narrow and n_info["ran"] else win
            m0, d0, _ = stale[i]
            assert np.array_equal(f[0][~written], m0[~written]), "query %d: an M cell outside the windows was written" % i
            out_d = ~written & b.kept[:, None]
            assert np.array_equal(f[1][out_d], d0[out_d]), "query %d: a D cell outside the windows was written" % i
    if not _overridden():
        assert rb.band_narrow_info() == n_info, (rb.band_narrow_info(), n_info, tiers)
        assert rb.band_info() == info, (rb.band_info(), info, tiers)
    b.check_results()
    return tiers


def _case(b, X, costs=COSTS, env=None, stale=True, want=None):
    env = {**ENV, **(env or {})}
    rb = b.open()
    try:
        before = None
        if stale:
            b.run(rb, STALE_COSTS, {"POA_BAND": "0"})
            before = b.check_full(rb, STALE_COSTS)
        b.run(rb, costs, env)
        tiers = _check(b, X, rb, costs, env, stale=before)
        if want is not None:
            assert tiers == want, (tiers, b.dense(costs)["score"], [(b.plan_n(X, len(q)).D, b.plan(X, len(q)).D) for q in b.qs])
        return tiers
    finally:
        rb.close()


def _pitch(L):
    return (L + 1 + 63) // 64 * 64


# ---- 1. the end of a plane row -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,backbone", [(575, 560), (1015, 980), (1023, 980)])
def test_row_end(engine, oracle, harness, L, backbone):
    """the lane that straddles the end of the plane row stores and loads only its dwords inside it: pitch - base is no multiple of 6
    in the last segment (one dword of that lane inside the row for 575 and 1015, one or two for 1023), for every row down to the
    last row of the last read of the batch"""
    g, full = _reads(W.scaled_linearish(backbone, backbone // 20, backbone // 40, 2, backbone + 60), 2)
    rng = np.random.default_rng(L)
    qs = [np.concatenate([q, ACGT[rng.integers(0, 4, 64)]])[:L] for q in full]
    b = NarrowBatch(engine, oracle, g, qs)
    bases = b.plan_n(harness, L).bases
    over = [int(_pitch(L) - c) % 6 for c in bases if c + NARROW > _pitch(L)]      # the segments whose window passes the row's end
    assert len(over) >= 2 and over[-1] != 0 and (L != 1023 or {2, 4} <= set(over)), (bases, over)
    _case(b, harness, want=["narrow", "narrow"])


# ---- 2. window moves ---------------------------------------------------------------------------------------------------------------
def _layered_chain(widths, seed):
    """one layer of widths[k] nodes per column, every node of a layer an edge to every node of the next -> (graph, a walk)"""
    rng = np.random.default_rng(seed)
    gb = GraphBuilder()
    prev, walk = [], []
    for w in widths:
        syms = ACGT[rng.permutation(4)[:w]] if w <= 4 else ACGT[rng.integers(0, 4, w)]
        layer = [gb.add_node(int(s)) for s in syms]
        for u in prev:
            for v in layer:
                gb.add_edge(u, v)
        walk.append(int(syms[rng.integers(0, w)]))
        prev = layer
    return gb.finish(), np.array(walk, np.uint8)


def test_windows_move_right_by_8_16_24(engine, oracle, harness):
    """segments of 64 rows that hold 8, 16 and 24 columns (layers of 8 rows, of 4 rows, and of 3, 3 and 2 rows): the window moves by
    as much, and a lane's three dwords come out of the hand-over buffer at every offset mod 3"""
    widths = [1] * 250 + [8] * 32 + [4] * 64 + [3, 3, 2] * 32 + [1] * 200
    g, walk = _layered_chain(widths, seed=11)
    assert g.n > 128
    rng = np.random.default_rng(5)
    qs = [W.mutate(rng, walk, 0.02, 0.0, 0.0), W.mutate(rng, walk, 0.03, 0.0, 0.0)]
    b = NarrowBatch(engine, oracle, g, qs)
    moves = set(np.diff(b.plan_n(harness, len(walk)).bases).tolist())
    assert {8, 16, 24} <= moves, moves
    _case(b, harness, want=["narrow", "narrow"])


@pytest.fixture(scope="module")
def fork(engine, oracle):
    g, walks = fork_graph(290, 170, 170, 200, seed=1)
    rng = np.random.default_rng(42)
    reads = [W.mutate(rng, walks[k % 2], 0.03, 0.01, 0.01) for k in range(4)]
    L = min(len(q) for q in reads)
    return NarrowBatch(engine, oracle, g, [q[:L] for q in reads])      # each pair: one read of either branch


def test_fork_graph_window_goes_back(fork, harness):
    """a move to the left, and a predecessor row read from memory whose segment has another base, at an offset that is no
    multiple of 6: a lane's dwords lie partly inside that row's window"""
    b = fork
    bases = b.plan_n(harness, len(b.qs[0])).bases
    assert (np.diff(bases) < 0).sum() >= 1, bases
    offs = set()
    for v in range(b.g.n):
        r = int(b.rows[v])
        for p in b.rows[b.g.predecessors(v).astype(np.int64)]:
            if p + 1 != r:
                offs.add(int(bases[r // SEG_ROWS] - bases[p // SEG_ROWS]))
    assert any(o % 6 for o in offs), offs
    _case(b, harness, want=["narrow"] * 4)


def test_sibling_row_opens_a_segment(engine, oracle, harness):
    poa = W.LayeredPOA(n_layers=150, width=3, indeg=3, seed=5)
    qs = poa.queries(6, length=0)
    L = min(len(q) for q in qs)
    long_read = np.concatenate([qs[0]] * 5)[:600]      # pads the chunk to the one-strip kernel
    b = NarrowBatch(engine, oracle, poa.graph, [long_read, _substituted(np.random.default_rng(2), long_read, 9)] + [q[:L] for q in qs])
    layer_of_row = np.full(poa.graph.n, -1)
    layer_of_row[b.rows[poa.ids.reshape(-1)]] = np.repeat(np.arange(150), 3)
    starts = np.arange(SEG_ROWS, poa.graph.n, SEG_ROWS)
    assert ((layer_of_row[starts] >= 0) & (layer_of_row[starts] == layer_of_row[starts - 1])).any()
    tiers = _case(b, harness)
    assert tiers.count("narrow") >= 6, tiers


# ---- 3. the end cell ------------------------------------------------------------------------------------------------------------------
def test_end_cell_in_every_register(engine, oracle, harness):
    """the certificate reads M[end][L] of both reads out of lane wc / 6, register wc % 6, wc = L - bases[-1]: lengths stepped by one
    put it into each of the six registers"""
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
    b = NarrowBatch(engine, oracle, g, qs)
    wc = [len(q) - int(b.plan_n(harness, len(q)).bases[-1]) for q in qs[::2]]
    assert {w % 6 for w in wc} == set(range(6)) and 0 <= min(wc) and max(wc) < NARROW, wc
    score = b.dense(COSTS)["score"]
    assert (score[0::2] != score[1::2]).all(), score
    _case(b, harness, stale=False, want=["narrow"] * 16)


@pytest.mark.parametrize("branch,lane", [(372, "first"), (40, "last")])
def test_end_cell_in_the_outer_lanes(engine, oracle, harness, branch, lane):
    """the lowest and a high lane the plan puts the end cell into.  Two branches of 372 rows leave the narrow window a band of
    D_n = 7, and a last segment of two rows starts its window four columns before L: lane 0.  The last window starts at most
    about 64 + D_n / 2 columns before L (the last segment's rows and half the band), which D_n < 384 keeps below lane 40: a
    short fork after a long chain reaches lane 34."""
    if lane == "first":
        g, walks = fork_graph(120, branch, branch, 160, seed=4)
    else:
        g, walks = fork_graph(500, branch, branch, 43, seed=4)
    rng = np.random.default_rng(branch)
    qs = [walks[0], _substituted(rng, walks[0], 1), walks[1], _substituted(rng, walks[1], 1)]
    b = NarrowBatch(engine, oracle, g, qs)
    pl = b.plan_n(harness, len(qs[0]))
    wc = len(qs[0]) - int(pl.bases[-1])
    assert pl.D >= 4 and (wc // 6 == 0 if lane == "first" else wc // 6 >= 34), (pl.D, wc, pl.bases)
    _case(b, harness, stale=False, want=["narrow"] * 4)


# ---- 4. symbols, members ------------------------------------------------------------------------------------------------------------
def test_non_acgt_symbols(engine, oracle, harness):
    """'N' rows take the path that computes the symbol masks of both reads instead of reading the tables"""
    g, backbone = _snp_graph(600, 20, 8, n_every=37)
    rng = np.random.default_rng(9)
    qs = []
    for k in range(2):
        q = W.mutate(rng, backbone, 0.02, 0.01, 0.01)[:590]
        q[rng.integers(0, len(q), 12)] = ord("N")
        twin = q.copy()
        twin[rng.integers(0, len(q), 12)] = ord("N")      # N's at other places than its partner's
        qs += [q, _substituted(rng, twin, 7) if k else twin]
    assert all(len(q) == 590 for q in qs)
    _case(NarrowBatch(engine, oracle, g, qs), harness, want=["narrow"] * 4)


@pytest.mark.parametrize("swap", [False, True])
def test_both_members_swapped(engine, oracle, harness, swap):
    """A's words must not land in B's plane: the same two reads in either order, each plane against its own read's model"""
    g, full = _reads(W.scaled_linearish(560, 28, 14, 2, 600), 2)
    L = min(len(q) for q in full) - 3
    qs = [full[0][:L], full[1][:L]]
    b = NarrowBatch(engine, oracle, g, qs[::-1] if swap else qs)
    _case(b, harness, want=["narrow", "narrow"])
    for i in range(2):
        assert 2 * int((~b.window_n(harness, i)).any(axis=1).sum()) >= b.g.n      # cells outside the windows in at least half the rows


# ---- 5. the cascade -----------------------------------------------------------------------------------------------------------------------
def test_cascade_three_tiers(engine, oracle, harness):
    """six reads of 1 000 bases on the headline graph, two the narrow tier certifies, two only the 512 pass does, two neither
    (random reads), paired across the kinds; chosen on the CPU by the oracle's score with 40 to spare on either side of T_n and T_512"""
    g, (qseq, qoff) = W.config2(n_queries=2)
    clean = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(2)]
    rng = np.random.default_rng(77)
    probe = NarrowBatch(engine, oracle, g, clean)
    t_n, t_w = 2 * (probe.plan_n(harness, 1000).D - 4), 2 * (probe.plan(harness, 1000).D - 4)
    assert t_n + 100 < t_w, (t_n, t_w)
    og, costs = probe.og, oracle.Costs(*COSTS)
    middle = []
    for k in range(40):      # divergent reads of the same walks: those whose score lies between the two thresholds
        q = W.fit_length(rng, W.mutate(rng, clean[k % 2], 0.05 + 0.002 * k, 0.01, 0.01), 1000)
        s = int(og.dense_align(q, costs)["score"])
        if t_n + 40 <= s <= t_w - 40:
            middle.append(q)
        if len(middle) == 2:
            break
    assert len(middle) == 2
    random_reads = [ACGT[rng.integers(0, 4, 1000)] for _ in range(2)]
    b = NarrowBatch(engine, oracle, g, [clean[0], middle[0], middle[1], random_reads[0], random_reads[1], clean[1]])
    score = b.dense(COSTS)["score"].astype(np.int64)
    assert (score[[0, 5]] <= t_n - 40).all() and (score[[3, 4]] >= t_w + 40).all(), (score, t_n, t_w)
    rb = b.open()
    try:
        full = b.run(rb, COSTS, {"POA_BAND": "0"})
        res = b.run(rb, COSTS, ENV)
        assert _same(res, full)
        b.check_results()
        if not _overridden():
            assert rb.band_narrow_info() == {"ran": 6, "certified": 2, "certified_512": 2, "chosen_by": "override"}, rb.band_narrow_info()
            info = rb.band_info()
            assert (info["used"], info["banded"], info["fell_back"]) == (True, 4, 2), info
        tiers, _, _ = _tiers(b, harness, COSTS, 1 << 30)
        assert tiers == ["narrow", "wide", "wide", "full", "full", "narrow"], tiers
    finally:
        rb.close()


def test_cap_takes_the_band_away(engine, oracle, harness):
    """POA_BAND_DELTA below 4: both reads of the pair go to the full pass, neither banded pass computes a cell"""
    g, full = _reads(W.scaled_linearish(560, 28, 14, 2, 600), 2)
    L = min(len(q) for q in full) - 3
    b = NarrowBatch(engine, oracle, g, [full[0][:L], full[1][:L]])
    tiers = _case(b, harness, env={"POA_BAND_DELTA": "0"}, stale=False, want=["full", "full"])
    assert tiers == ["full", "full"]


def test_default_untouched(engine, oracle, harness):
    """without POA_BAND_NARROW a 16-read chunk under POA_BAND_PAIR=1 runs the 512 kernels alone: no narrow reads, the planes those
    of the 512-window model and nothing written outside the 512 windows"""
    g, full = _reads(W.scaled_linearish(560, 28, 14, 16, 600), 16)
    L = min(len(q) for q in full)
    b = NarrowBatch(engine, oracle, g, [q[:L] for q in full])
    env = {"POA_BAND_PAIR": "1"}
    rb = b.open()
    try:
        b.run(rb, STALE_COSTS, {"POA_BAND": "0"})
        before = b.check_full(rb, STALE_COSTS)
        b.run(rb, COSTS, env)
        assert rb.band_narrow_info() == {"ran": 0, "certified": 0, "certified_512": 0, "chosen_by": None}
        want, keep = b.check_banded(harness, rb, COSTS, env, stale=before)
        assert all(keep) and rb.band_pair_info()["paired"] == 16
    finally:
        rb.close()
