"""Cell-by-cell parity of the compact derived-gaps layout (TbParams::code_fmt 4: the u16 M plane with I == M in bit 14 and D == M in
bit 15, plus the kept D rows), fetched with poa_batch_fetch_compact / ResidentBatch.compact_planes, for the three kernels that
store it: poa_forward_px_kernel<3> (POA_BAND=0) and both instantiations of poa_forward_band_kernel.

What a stored word must be, for planes (M, I, D) - the oracle's, or for the window cells of a certified banded query those of the
windowed model (tests/band_model.py) under the plan of poa_band_plan.cpp:
  * a value below 0x3FFF is stored exactly, with bit 14 = (I == M) and bit 15 = (D == M);
  * INF (or a value >= 0x3FFF) reads 0x3FFF in the score field; nothing finer is defined there (memory reads turn it into INF);
  * the same for the kept D rows against 0x3FFF.
So that the second rule hides nothing, every case asserts from the oracle's planes alone that all finite M and D values are below
0x3FFF (the cases of tests/test_clamped_cells.py open their Batch with clamped=True and assert the opposite: that finite values at
and above 0x3FFF are there, in M and in the kept D rows).  Only columns 0..L are compared.  The banded kernel writes its windows only: outside them the planes hold what was there
before, which one case checks word for word.  All comparisons are bit-exact.

Which queries the banded pass certifies follows from the plan's D and the oracle's score (tests/test_band_forward.py); those path
assertions are skipped under the environment overrides named there, the cell comparisons run whenever the layout is derived-gaps."""
import contextlib
import os

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries
from band_model import INF, fork_graph, in_window, stored_words, windowed_planes
from test_band_forward import _overridden
from test_band_plan import Plan, harness   # noqa: F401  (the host build of the band plan)

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", np.uint8)
SEG_ROWS, WINDOW = 64, 512     # poa_band_plan.hpp: BAND_SEG_ROWS, BAND_WINDOW
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _cap(env):
    v = {**os.environ, **env}.get("POA_BAND_DELTA")
    return (1 << 30) if v is None else max(int(v), 0)


def _kept_rows(g, rows):
    """the D rows the compact layout keeps, restated: the end row, and every predecessor of a non-chain row (a chain row has
    exactly one predecessor and it is the row right above)"""
    kept = np.zeros(g.n, bool)
    kept[rows[g.end]] = True
    for v in range(g.n):
        prs = rows[g.predecessors(v).astype(np.int64)]
        if not (len(prs) == 1 and prs[0] + 1 == rows[v]):
            kept[prs] = True
    return kept


def _where(sel, got, want):
    bad = np.argwhere(sel & (got != want))
    if len(bad) == 0:
        return None
    r, c = (int(t) for t in bad[0])
    return "%d cells differ, first at row %d column %d: stored 0x%04X, expected 0x%04X" % (len(bad), r, c, int(got[r, c]), int(want[r, c]))


def _assert_words(fetched, planes, mask, what):
    """the stored words of the cells in `mask` against planes (M, I, D)"""
    m_raw, d, kept = fetched
    m_exact, m_word, d_exact, d_word = stored_words(*planes)
    assert _where(mask & m_exact, m_raw, m_word) is None, (what, "M", _where(mask & m_exact, m_raw, m_word))
    sel = mask & ~m_exact
    assert ((m_raw[sel] & 0x3FFF) == 0x3FFF).all(), (what, "M: a cell that is INF does not read 0x3FFF")
    km = mask & kept[:, None]
    assert _where(km & d_exact, d, d_word) is None, (what, "D", _where(km & d_exact, d, d_word))
    assert (d[km & ~d_exact] >= 0x3FFF).all(), (what, "D: a cell that is INF reads below 0x3FFF")


class Batch:
    """a graph and its reads; the oracle's planes (by engine row), the plans and the model's planes, each computed once"""
    def __init__(self, engine, oracle, g, qs, clamped=False):
        self.engine, self.oracle, self.g, self.clamped = engine, oracle, g, clamped
        self.qs = [np.ascontiguousarray(q, np.uint8) for q in qs]
        assert len(qs) <= 16 and 512 <= max(len(q) for q in qs) <= 1023, [len(q) for q in qs]      # one chunk of the one-strip kernel
        self.qseq, self.qoff = pack_queries(self.qs)
        self.og = oracle.OracleGraph.from_csr(g.as_dict())
        self.orank = self.og.export_csr()["rank"]
        self.rows = engine._device_graph(g).node_rows().astype(np.int64)      # node -> engine row
        self.node_of_row = np.argsort(self.rows)
        self.kept = _kept_rows(g, self.rows)
        self._true, self._model, self._plan, self._dense = {}, {}, {}, {}

    def true(self, i, costs):
        if (i, costs) not in self._true:
            od = self.og.dense_align(self.qs[i], self.oracle.Costs(*costs), planes=True)
            planes = [np.ascontiguousarray(od[name][self.orank])[self.node_of_row] for name in ("M", "I", "D")]
            self._fits(planes)
            self._true[(i, costs)] = planes
        return self._true[(i, costs)]

    def _fits(self, planes):
        """from the planes alone: every finite value fits the 14-bit score field, so only true INF cells fall under the ">=" rule;
        clamped: finite M values and finite values of the kept D rows at and above 0x3FFF are there (a query of two columns or
        more: an empty or one-symbol query rides along under the others' pitch)"""
        m, d = planes[0], planes[2][self.kept]
        if not self.clamped:
            for p in (planes[0], planes[2]):
                assert int(p[p != INF].max()) < 0x3FFF
        elif m.shape[1] > 2:
            assert ((m != INF) & (m >= 0x3FFF)).any() and ((d != INF) & (d >= 0x3FFF)).any()

    def dense(self, costs):
        if costs not in self._dense:
            self._dense[costs] = self.og.dense_batch(self.qseq, self.qoff, self.oracle.Costs(*costs), threads=4)
        return self._dense[costs]

    def plan(self, X, L):
        if L not in self._plan:
            pl = Plan(X, self.g, L, SEG_ROWS, WINDOW)
            assert np.array_equal(pl.node_row, self.rows)      # the harness and the engine order the rows alike
            self._plan[L] = pl
        return self._plan[L]

    def model(self, X, i, costs):
        if (i, costs) not in self._model:
            q = self.qs[i]
            planes = windowed_planes(self.g, self.rows, q, costs, SEG_ROWS, WINDOW, self.plan(X, len(q)).bases)
            self._fits(planes)
            self._model[(i, costs)] = planes
        return self._model[(i, costs)]

    def window(self, X, i):
        L = len(self.qs[i])
        return in_window(self.g.n, L, SEG_ROWS, WINDOW, self.plan(X, L).bases)

    def predict(self, X, costs, cap):
        """as Case.banded of tests/test_band_forward.py: -> (band_info of a banded run, [query certified])"""
        e = costs[2]
        d_of = {L: min(self.plan(X, L).D, cap) for L in {len(q) for q in self.qs}}
        keep = [d_of[len(q)] >= 4 and int(s) <= min(e * (d_of[len(q)] - 4), 0x3FFE) for q, s in zip(self.qs, self.dense(costs)["score"])]
        return {"used": True, "banded": sum(keep), "fell_back": len(keep) - sum(keep), "min_d": min(d_of.values())}, keep

    def open(self, **kw):
        return self.engine.ResidentBatch(self.g, self.qseq, self.qoff, **kw)

    def run(self, rb, costs, env):
        with _environ(env):
            rb.run(self.engine.GapAffine(costs[0], costs[2], costs[1]))
        self.res, self.res_costs = rb.fetch(), costs
        if "derived_gaps" not in rb.layout() or "relative" in rb.layout():
            self.check_results()
            pytest.skip("an environment override took the run to another layout: %s" % sorted(rb.layout()))
        return self.res

    def check_results(self):
        """score, flags and pairs of the last run against the oracle's dense batch (after the cells, so that a wrong cell is
        reported as the cell it is)"""
        D = self.dense(self.res_costs)
        assert np.array_equal(self.res.score, D["score"]), (self.res.score, D["score"])
        assert np.array_equal(self.res.flags, D["flags"]), (self.res.flags, D["flags"])
        for i in range(len(self.qs)):
            assert self.res.raw_alignment(i) == self.oracle.batch_alignment(D, i), i

    def check_full(self, rb, costs, queries=None, results=True):
        """every cell of m_raw and every kept D row against the oracle -> the fetched planes"""
        out = {}
        for i in (range(len(self.qs)) if queries is None else queries):
            f = rb.compact_planes(i)
            assert np.array_equal(f[2], self.kept), i
            assert (f[1][~f[2]] == 0xFFFF).all()
            _assert_words(f, self.true(i, costs), np.ones(f[0].shape, bool), "query %d, all cells against the oracle" % i)
            out[i] = f
        if results:
            self.check_results()
        return out

    def check_banded(self, X, rb, costs, env, queries=None, stale=None, want_keep=None):
        """after a banded run, for the queries the plan and the oracle's scores say are certified: window cells against the model
        (and, given `stale`, every other cell against those planes, fetched before the run); for the others: all cells against the
        oracle; then band_info against that prediction, then the results"""
        info = rb.band_info()
        want, keep = self.predict(X, costs, _cap(env))
        if want_keep is not None:
            assert keep == want_keep, keep
        for i in (range(len(self.qs)) if queries is None else queries):
            if not info["used"] or not keep[i]:
                self.check_full(rb, costs, [i], results=False)
                continue
            f = rb.compact_planes(i)
            assert np.array_equal(f[2], self.kept), i
            self.true(i, costs)      # (asserts that the oracle's finite values fit the score field)
            win = self.window(X, i)
            _assert_words(f, self.model(X, i, costs), win, "query %d, window cells against the model" % i)
            if stale is not None:
                m0, d0, _ = stale[i]
                assert np.array_equal(f[0][~win], m0[~win]), "query %d: an M cell outside the windows was written" % i
                out_d = ~win & self.kept[:, None]
                assert np.array_equal(f[1][out_d], d0[out_d]), "query %d: a D cell outside the windows was written" % i
        if not _overridden():
            assert info == want, (info, want)
        self.check_results()
        return want, keep


def _reads(g_qs, n):
    g, (qseq, qoff) = g_qs
    return g, [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(n)]


def _fork_batch(engine, oracle):
    g, walks = fork_graph(300, 150, 150, 200, seed=1)
    rng = np.random.default_rng(42)
    return Batch(engine, oracle, g, [W.mutate(rng, walks[k % 2], 0.03, 0.01, 0.01) for k in range(8)])


@pytest.fixture(scope="module")
def linearish(engine, oracle):
    return Batch(engine, oracle, *_reads(W.scaled_linearish(560, 28, 14, 12, 600), 12))


@pytest.fixture(scope="module")
def fork(engine, oracle):
    return _fork_batch(engine, oracle)


# ---- 1. poa_forward_px_kernel<3> ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["linearish", "fork"])
def test_full_kernel_every_cell(request, which):
    b = request.getfixturevalue(which)
    assert 600 <= b.g.n <= 820
    rb = b.open()
    try:
        b.run(rb, (4, 6, 2), {"POA_BAND": "0"})
        assert not rb.band_info()["used"]
        b.check_full(rb, (4, 6, 2))
    finally:
        rb.close()


# ---- 2. banded, all certified ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["linearish", "fork"])
def test_banded_window_cells(request, harness, which):
    b = request.getfixturevalue(which)
    if which == "fork":   # the second branch's rows come after the first's: the window goes back to the left for them
        assert all((np.diff(b.plan(harness, len(q)).bases) < 0).sum() >= 1 for q in b.qs), [b.plan(harness, len(q)).bases for q in b.qs]
    rb = b.open()
    try:
        b.run(rb, (4, 6, 2), {})
        want, keep = b.check_banded(harness, rb, (4, 6, 2), {})
        assert all(keep), (want, b.dense((4, 6, 2))["score"])
    finally:
        rb.close()


# ---- 3. only window cells are written ------------------------------------------------------------------------------------------
def test_banded_run_writes_window_cells_only(linearish, harness):
    b = linearish
    rb = b.open()
    try:
        b.run(rb, (3, 1, 1), {"POA_BAND": "0"})
        before = b.check_full(rb, (3, 1, 1))
        b.run(rb, (4, 6, 2), {})
        want, keep = b.check_banded(harness, rb, (4, 6, 2), {}, stale=before)
        assert all(keep)
        for i in range(len(b.qs)):
            assert 2 * int((~b.window(harness, i)).any(axis=1).sum()) >= b.g.n      # cells outside the windows in at least half the rows
    finally:
        rb.close()


# ---- 4. the fallback instantiation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", ["0", "4"])
def test_forced_fallback_every_cell(linearish, harness, cap):
    b = linearish
    rb = b.open()
    try:
        b.run(rb, (4, 6, 2), {"POA_BAND_DELTA": cap})
        want, keep = b.check_banded(harness, rb, (4, 6, 2), {"POA_BAND_DELTA": cap})
        assert not any(keep)
    finally:
        rb.close()


def _mixed(engine, oracle, n_each):
    """interleaved clean and divergent reads, and the cap that puts T = e * (cap - 4) between the two groups' scores"""
    g, clean = _reads(W.scaled_linearish(560, 28, 14, n_each, 600), n_each)
    _, divergent = _reads(W.scaled_linearish(560, 28, 14, n_each, 600, query_seed=7, p_sub=0.10, p_ins=0.05, p_del=0.05), n_each)
    b = Batch(engine, oracle, g, [q for pair in zip(clean, divergent) for q in pair])
    score = b.dense((4, 6, 2))["score"].astype(np.int64)
    lo, hi = int(score[0::2].max()), int(score[1::2].min())
    assert lo + 8 < hi, (lo, hi)      # the oracle's scores alone separate the two kinds of read
    return b, ((lo + hi) // 2) // 2 + 4


def test_mixed_chunk_both_kinds_of_planes(engine, oracle, harness):
    b, cap = _mixed(engine, oracle, 6)
    env = {"POA_BAND_DELTA": str(cap)}
    rb = b.open()
    try:
        b.run(rb, (4, 6, 2), env)
        want, keep = b.check_banded(harness, rb, (4, 6, 2), env, want_keep=[True, False] * 6)
        assert want["min_d"] == cap, want
    finally:
        rb.close()


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------------------
def _banded_case(b, X, costs=(4, 6, 2), full_too=False):
    rb = b.open()
    try:
        if full_too:
            b.run(rb, costs, {"POA_BAND": "0"})
            b.check_full(rb, costs)
        b.run(rb, costs, {})
        return b.check_banded(X, rb, costs, {})
    finally:
        rb.close()


def test_edge_lengths(engine, oracle, harness):
    """512: the smallest length that reaches the kernel (513 columns, pitch 576); 575: L + 1 equals the pitch; 1023: pitch 1024"""
    g, full = _reads(W.scaled_linearish(880, 40, 20, 3, 1000, p_sub=0.04, p_ins=0.02, p_del=0.02), 3)
    tail = ACGT[np.random.default_rng(3).integers(0, 4, 23)]
    b = Batch(engine, oracle, g, [full[0][:512], full[1][:575], np.concatenate([full[2], tail])])
    assert [len(q) for q in b.qs] == [512, 575, 1023]
    _banded_case(b, harness, full_too=True)


def _snp_graph(n_backbone, n_snp, seed, n_every=0):
    """a backbone with one-node SNP bubbles; n_every > 0: every n_every-th backbone node and every second SNP node is an 'N'"""
    rng = np.random.default_rng(seed)
    backbone = ACGT[rng.integers(0, 4, n_backbone)]
    if n_every:
        backbone[n_every // 2::n_every] = ord("N")
    gb = GraphBuilder()
    ids = gb.add_path(backbone)
    for k, p in enumerate(np.linspace(5, n_backbone - 6, n_snp).astype(int)):
        v = gb.add_node(ord("N") if n_every and k % 2 else int(ACGT[rng.integers(0, 4)]))
        gb.add_edge(ids[p - 1], v)
        gb.add_edge(v, ids[p + 1])
    return gb.finish(), backbone


def test_non_acgt_symbols(engine, oracle, harness):
    """'N' nodes and 'N's in the reads: the rows whose symbol masks are computed instead of read from the LDS tables, in the full
    kernel and in the banded one; an 'N' equals an 'N' and nothing else, in the engine as in the oracle"""
    g, backbone = _snp_graph(600, 20, 8, n_every=37)
    assert (g.symbol == ord("N")).sum() >= 20
    rng = np.random.default_rng(9)
    qs = []
    for k in range(4):
        q = W.mutate(rng, backbone, 0.02, 0.01, 0.01)
        q[rng.integers(0, len(q), 12)] = ord("N")      # besides the 'N's of the backbone that survived
        qs.append(q)
    assert all((q == ord("N")).sum() >= 12 for q in qs)
    _, keep = _banded_case(Batch(engine, oracle, g, qs), harness, full_too=True)
    assert all(keep)


@pytest.mark.parametrize("n_rows", [641, 640])
def test_row_counts(engine, oracle, harness, n_rows):
    """an odd number of rows (the kernel takes two rows per turn) and a multiple of 64 (the last segment is full)"""
    g, backbone = _snp_graph(n_rows - 2 - 12, 12, 21)
    assert g.n == n_rows
    rng = np.random.default_rng(n_rows)
    _, keep = _banded_case(Batch(engine, oracle, g, [W.mutate(rng, backbone, 0.02, 0.01, 0.01) for _ in range(3)]), harness)
    assert all(keep)


def test_end_cell_in_both_halves(engine, oracle, harness):
    """the certificate reads M[end][L] out of the registers: window column L - bases[-1] in the low and in the high half of the
    window, and in each of a lane's four registers"""
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
    qs = [backbone] + [short[:L] if L <= len(short) else np.concatenate([short, backbone[:L - len(short)]]) for L in (533, 534, 535)]
    b = Batch(engine, oracle, g, qs)
    wc = [len(q) - int(b.plan(harness, len(q)).bases[-1]) for q in qs]
    assert sorted(w % 4 for w in wc) == [0, 1, 2, 3] and min(wc) < 256 <= max(wc) < 512, wc
    _, keep = _banded_case(b, harness)
    assert all(keep)


def test_sibling_rows_across_segment_starts(engine, oracle, harness):
    """layers of three sibling rows: some segment starts with a non-first row of a layer, whose predecessor minima the kernel
    recomputes under the new window instead of taking the cached ones"""
    poa = W.LayeredPOA(n_layers=150, width=3, indeg=3, seed=5)
    qs = poa.queries(7, length=0)
    long_read = np.concatenate([qs[0]] * 5)[:600]      # pads the chunk to the one-strip kernel
    b = Batch(engine, oracle, poa.graph, [long_read] + qs)
    layer_of_row = np.full(poa.graph.n, -1)
    layer_of_row[b.rows[poa.ids.reshape(-1)]] = np.repeat(np.arange(150), 3)
    starts = np.arange(SEG_ROWS, poa.graph.n, SEG_ROWS)
    assert ((layer_of_row[starts] >= 0) & (layer_of_row[starts] == layer_of_row[starts - 1])).any()
    want, keep = _banded_case(b, harness)
    assert sum(keep) >= 7, want


# ---- 6. several chunks ----------------------------------------------------------------------------------------------------------------
def test_several_chunks(engine, oracle, harness):
    from poasta_amd import _lib
    b, cap = _mixed(engine, oracle, 6)
    env = {"POA_BAND_DELTA": str(cap)}
    rb = b.open(workspace_bytes=1)      # the smallest workspace: one query's u32 planes, which hold four queries' compact ones
    try:
        full = b.run(rb, (4, 6, 2), {"POA_BAND": "0"})
        b.check_results()
        res = b.run(rb, (4, 6, 2), env)
        assert res.stats["n_chunks"] >= 3, res.stats
        assert np.array_equal(res.score, full.score) and np.array_equal(res.flags, full.flags)
        assert np.array_equal(res.pair_off, full.pair_off) and np.array_equal(res.pairs, full.pairs)
        with pytest.raises(_lib.PoaError) as err:
            rb.compact_planes(0)      # overwritten by the later chunks
        assert err.value.code == ERR_INVALID_ARG
        last = []      # the queries of the last chunk: those the fetch still serves
        for i in reversed(range(len(b.qs))):
            try:
                rb.compact_planes(i)
            except _lib.PoaError:
                break
            last.append(i)
        assert 2 <= len(last) < len(b.qs), last      # both kinds of read
        want, keep = b.check_banded(harness, rb, (4, 6, 2), env, queries=last, want_keep=[True, False] * 6)
        assert want["banded"] == 6 and want["fell_back"] == 6 and want["min_d"] == cap
    finally:
        rb.close()


# ---- the fetch refuses what it cannot serve ------------------------------------------------------------------------------------------
def test_fetch_refuses_other_layouts_and_modes(engine):
    from poasta_amd import _lib
    g, (qseq, qoff) = W.scaled_linearish(200, 10, 5, 4, 220)
    costs = engine.GapAffine(4, 2, 6)

    def refused(rb, code):
        with pytest.raises(_lib.PoaError) as err:
            rb.compact_planes(0)
        assert err.value.code == code, err.value

    rb = engine.ResidentBatch(g, qseq, qoff)
    try:
        refused(rb, ERR_INVALID_ARG)      # not run
        with _environ({"POA_PLANES": "32"}):
            rb.run(costs)
        rb.fetch()
        refused(rb, ERR_UNSUPPORTED)
        rb.run(costs, None, engine.make_config("hybrid"))
        rb.fetch()
        refused(rb, ERR_UNSUPPORTED)
        rb.run(costs)
        rb.fetch()
        if "derived_gaps" not in rb.layout():      # (rows of at most 512 columns take another kernel and another compact format)
            refused(rb, ERR_UNSUPPORTED)
    finally:
        rb.close()
    for mode in ("score", "checkpoint"):
        cfg = engine.make_config(mode)
        rb = engine.ResidentBatch(g, qseq, qoff, config=cfg)
        try:
            rb.run(costs, None, cfg)
            rb.fetch(want_pairs=mode != "score")
            refused(rb, ERR_UNSUPPORTED)
        finally:
            rb.close()
