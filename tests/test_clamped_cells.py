"""Parity where FINITE cells exceed the narrow cell format.  The launcher bounds only the optimal score (ub = [o + e * L] +
[o + e * min_path_nodes]); every other cell may hold a larger finite value, which each format clamps to its INF — 0xFFFF for u16
cells, 0x3FFF for the flags-in-score formats code_fmt 2 and 4, 0x0FFF for code_fmt 3 — on the argument that nothing the result
depends on changes.  The graphs of tests/clamp_shapes.py (a long arm beside a short backbone) put a tenth to a fifth of every
plane above the format's limit while ub still selects it, and every case asserts that from the oracle's planes alone
(clamp_shapes.clamp_profile) before an engine result is looked at.

CPU: `CASES` lists the batches of the dense one-piece and sweep-family GPU tests (the relative, two-piece, dense multi-graph and
hybrid tests assert their own conditions and what ran); one test walks it through clamp_profile and through the restated launcher
rules (predict of test_dense_launch_matrix.py, sweep_model.py, predict of test_two_piece_shapes.py) and asserts that every
format and kernel family of REQUIRED is reached, so a trimmed table fails rather than passes.  The derivation of the gap-state
flags (poa_tb_derive.hpp, compiled for the host) runs over planes clamped as the formats store them.

GPU: every comparison is bit for bit against the oracle (oracle.two_piece for that model).  What ran is asserted through
launches(), layout(), band_info() or poa_stats_t.plane_bytes against those restatements, so no case can pass by running u32
planes.  Cell-level comparisons leave no cell of columns 0..L out: a value below the limit is stored exactly (with its flag
bits), a value at or above it, or INF, reads as the limit (u16 full planes: as INF); the same for the kept D rows.

Two-piece model: under (4, 30, 6, 1, 24) the second piece makes long gaps cheap, and the oracle shows that no plane exceeds u16
on the arm graph (the largest finite value is 38 526, in I1); checkpoint2 runs under those costs as one more cost model and asserts
that absence.  The clamped two-piece cases run under (4, 30, 6, 28, 60): u16 cells by the first piece's bound, and more than
100 000 finite values above 65534 in each of the five planes, asserted from the oracle's planes.

Value-only mutants of the clamps and which tests fail under each: profiles/pr_clamped_cells/README.md."""
import functools
from collections import OrderedDict, namedtuple

import numpy as np
import pytest

from poasta_amd.graph import GraphBuilder, pack_queries

import clamp_shapes as CS
import sweep_model as SM
import test_dense_launch_matrix as DLM
import test_two_piece_shapes as TPS
from band_model import stored_words
from test_band_plan import Plan, harness as band_harness   # noqa: F401  (the host build of the band plan)
from test_derived_gap_flags import harness as derive_harness, _p   # noqa: F401  (the host build of the derivation)
from test_two_piece_shapes import min_path_nodes

INF = 0xFFFFFFFF
NONE = 0xFFFFFFFF
SHORT_QUERY, CAPPED = 0x08, 0x80
L16, L14, L12 = CS.LIMIT_U16, CS.LIMIT_14, CS.LIMIT_12
ALL3 = ("rejoin", "into_end", "arm_first")
ONE = ("rejoin",)
WRAP2 = ("rejoin", "wrap")      # the sweep family has no plane to fetch: it also runs the arm whose wrapped values would win
Q600 = ("r600", "r600b", "empty", "one")
QN600 = ("n600", "r600", "empty", "one")
Q400 = ("r400", "empty", "one")
Q1300 = ("r1300", "r600", "empty", "one")
PX600, PXN600 = ("r600", "r600b", "n600"), ("n600", "r600", "r600b")      # whole pitches only: the packed sweep
C468, C462, C4630, C25530 = (4, 6, 8), (4, 6, 2), (4, 6, 30), (255, 6, 30)      # (mismatch, open, extend)
C2P, C2P_STEEP = (4, 30, 6, 1, 24), (4, 30, 6, 28, 60)                          # (m, e1, o1, e2, o2)
CKPT_ROWS = 50


# ---- the arm graphs with everything the oracle says about them, computed once ---------------------------------------------------
class ArmData:
    def __init__(self, oracle, variant):
        from poasta_amd import aligner
        self.oracle, self.variant = oracle, variant
        self.arm = CS.headline_arm(variant)
        self.g = self.arm.graph
        self.reads = CS.reads(variant)
        self.og = oracle.OracleGraph.from_csr(self.g.as_dict())
        self.orank = self.og.export_csr()["rank"]
        self.rows = aligner._device_graph(self.g).node_rows().astype(np.int64)      # node -> engine row
        self.node_of_row = np.argsort(self.rows)
        self.kept = CS.kept_rows(self.g, self.rows)                                   # by engine row
        self.mpn = min_path_nodes(self.g)
        self._planes, self._dense, self._profiles = OrderedDict(), {}, {}

    def qs(self, names):
        return [self.reads[k] for k in names]

    def planes(self, name, costs):
        """the oracle's (M, I, D) by engine row; one-piece costs"""
        key = (name, costs)
        if key not in self._planes:
            od = self.og.dense_align(self.reads[name], self.oracle.Costs(*costs), planes=True)
            self._planes[key] = tuple(np.ascontiguousarray(od[k][self.orank])[self.node_of_row] for k in "MID") + (int(od["score"]),)
            while len(self._planes) > 3:      # (23 MB per query)
                self._planes.popitem(last=False)
        return self._planes[key][:3]

    def planes2(self, name, costs2):
        """the oracle's (M, I1, D1, I2, D2) by engine row; two-piece costs"""
        m, e1, o1, e2, o2 = costs2
        with self.oracle.two_piece(o2, e2):
            d = self.og.dense_align(self.reads[name], self.oracle.Costs(m, o1, e1), planes=True)
            i2, d2 = self.og.dense_planes2(self.reads[name], self.oracle.Costs(m, o1, e1))
        return [np.ascontiguousarray(p[self.orank])[self.node_of_row] for p in (d["M"], d["I"], d["D"], i2, d2)]

    def dense(self, names, costs):
        """dense_batch of the reads `names`; two-piece costs run under oracle.two_piece"""
        key = (names, costs)
        if key not in self._dense:
            qseq, qoff = pack_queries(self.qs(names))
            if len(costs) == 3:
                D = self.og.dense_batch(qseq, qoff, self.oracle.Costs(*costs), threads=4)
            else:
                m, e1, o1, e2, o2 = costs
                with self.oracle.two_piece(o2, e2):
                    D = self.og.dense_batch(qseq, qoff, self.oracle.Costs(m, o1, e1), threads=4)
            self._dense[key] = D
        return self._dense[key]

    def profile(self, name, costs, limit, max_len, all_d=False):
        """clamp_profile of one read under a batch whose longest query has max_len symbols; all_d: every D row is stored (full
        planes, the sweeps' live rows), else the rows of the compact layouts"""
        key = (name, costs, limit, max_len, all_d)
        if key not in self._profiles:
            planes = self.planes(name, costs)
            score = self._planes[(name, costs)][3]
            feeders = tuple(int(self.rows[v]) for v in self.arm.feeders)
            self._profiles[key] = CS.clamp_profile(planes, limit, costs[0], ub=CS.score_ub(costs[1], costs[2], max_len, self.mpn),
                                                   kept=np.ones(self.g.n, bool) if all_d else self.kept,
                                                   feeders=feeders, score=score)
        return self._profiles[key]


_ARMS = {}


def _arm_data(oracle, variant):
    if variant not in _ARMS:
        _ARMS[variant] = ArmData(oracle, variant)
    return _ARMS[variant]


@functools.lru_cache(maxsize=None)
def _chain_graph():
    """a 40-node chain and a read of it: the small member of the multi-graph batches and score sets"""
    rng = np.random.default_rng(41)
    seq = CS.ACGT[rng.integers(0, 4, 40)]
    gb = GraphBuilder()
    gb.add_path(seq)
    q = seq.copy()
    q[7] = CS.ACGT[(int(np.searchsorted(CS.ACGT, q[7])) + 1) % 4]
    return gb.finish(), np.delete(q, [20, 21])


# ---- the case table: the batches of test_gpu_dense_clamped, the banded test and the sweep-family tests ------------------------------------------------------------------------------
# family "dense": runs = ((tune, site), ...), one dense run each, all on the same queries; words: the stored words of code_fmt 4
# are compared; full: full u16 planes, compared cell for cell.  family "sweep": runs = ((path, reads), ...).
Case = namedtuple("Case", "name family variants reads profiled costs limit runs full words")


def _dense(name, variants, reads, profiled, costs, limit, runs, full=False, words=False):
    return Case(name, "dense", variants, reads, profiled, costs, limit, tuple((tuple(sorted(t.items())), s) for t, s in runs), full, words)


CASES = [
    # the one-strip kernel poa_forward_px_kernel<MF>; the run without flags in the score (mf 0) is the others' yardstick among the formats
    _dense("px-4_6_8", ALL3, Q600, ("r600", "r600b"), C468, L14, [({"band": 0}, "px<3>"), ({"mf": 1}, "px<1>"), ({"mf": 0}, "px<0>")], words=True),
    _dense("px-4_6_2", ALL3, Q600, ("r600", "r600b"), C462, L12, [({"band": 0, "mf": 2}, "px<2>"), ({"mf": 0}, "px<0>")]),
    _dense("px-4_6_30", ALL3, Q600, ("r600", "r600b"), C4630, L16, [({}, "px<0>")]),
    _dense("px-255_6_30", ALL3, QN600, ("n600", "r600"), C25530, L16, [({}, "px<0>")]),
    # the packed kernel: one quad, two quads, several strips in both multi-wave forms
    _dense("packed-q1", ONE, Q400, ("r400",), C4630, L16, [({"px": 0}, "packed<1,false,false>")]),
    _dense("packed-q2", ONE, Q600, ("r600", "r600b"), C4630, L16, [({"px": 0}, "packed<2,false,false>")]),
    _dense("packed-q2-255", ONE, QN600, ("n600", "r600"), C25530, L16, [({"px": 0}, "packed<2,false,false>")]),
    _dense("packed-strips", ONE, Q1300, ("r1300", "r600"), C4630, L16, [({"px": 0, "pxmw": 0}, "packed<1,false,true>"), ({"px": 0, "pxmw": 1}, "pxmw")]),
    # full u16 planes, poa_forward_kernel<uint16_t>: one strip, several strips of 1024 and of 512 columns
    _dense("full-one-strip", ALL3, Q600, ("r600", "r600b"), C4630, L16, [({}, "LAUNCH_FWD(2,u16)")], full=True),
    _dense("full-one-strip-255", ONE, QN600, ("n600", "r600"), C25530, L16, [({}, "LAUNCH_FWD(2,u16)")], full=True),
    _dense("full-strips", ONE, Q1300, ("r1300", "r600"), C4630, L16, [({}, "LAUNCH_FWD(2,u16)"), ({"fwd_quads": 1}, "LAUNCH_FWD(1,u16)")], full=True),
    # the banded pair, no override: what the band plan of the arm graph decides
    _dense("band", ALL3, Q600, ("r600", "r600b"), C468, L14, [({}, "band")], words=True),
]
for _costs, _px in ((C4630, PX600), (C25530, PXN600)):
    _t = "_".join(map(str, _costs))
    _prof = tuple(k for k in _px if k != "r600b" or _costs == C4630)[:2]
    CASES += [
        Case("sweep-score-" + _t, "sweep", ("rejoin", "into_end", "wrap"), None, _prof, _costs, L16, (("score", _px), ("score", Q1300)), False, False),
        Case("sweep-ckpt-" + _t, "sweep", WRAP2, None, ("r1300", "r600"), _costs, L16, (("ckpt", Q1300),), False, False),
        Case("sweep-multi-" + _t, "sweep", WRAP2, None, ("r1300", "r600"), _costs, L16, (("multi", Q1300),), False, False),
        Case("sweep-scoreset-" + _t, "sweep", WRAP2, None, ("r1300",) + _prof, _costs, L16, (("ss", _px + ("r1300", "empty", "one")),
                                                                                           ("ss_cap", _px + ("r1300", "empty", "one")),
                                                                                           ("ss_best", _px + ("r1300", "empty", "one"))), False, False),
    ]
CASES_2P = [      # two-piece under C2P_STEEP: (name, path or "dense2", reads)
    ("ckpt2", "ckpt2", Q1300), ("multi2", "multi2", Q1300), ("dense2", "dense2", Q600),
]
BY_NAME = {c.name: c for c in CASES}

REQUIRED_DENSE = {"px<3>", "px<2>", "px<1>", "px<0>", "packed<1,false,false>", "packed<2,false,false>", "packed<1,false,true>", "pxmw",
                  "LAUNCH_FWD(2,u16)", "LAUNCH_FWD(1,u16)", "band"}
REQUIRED_FORMATS = {(4, L14), (3, L12), (2, L14), (1, L16), (0, L16), ("u16-full", L16)}      # (storage format, limit)
REQUIRED_SWEEP = {"poa_sweep_px_kernel", "poa_sweep_kernel<2,u16>", "poa_ckpt<2,u16>", "poa_ckpt_multi<2,u16>", "scoreset<PX>", "scoreset<2,u16>",
                  "scoreset<1,u16>", "scoreset_capped<PX>", "scoreset_capped<2,u16>", "scoreset_best<PX>", "scoreset_best<2,u16>"}
REQUIRED_2P = {"poa2_ckpt<u16,2>", "poa2_ckpt_multi<u16,2>", "dense2-u16"}


def _lengths(variant, names):
    return [len(CS.reads(variant)[k]) for k in names]


def _predict_dense(case, variant, tune):
    return DLM.predict(CS.headline_arm(variant).graph, _lengths(variant, case.reads), case.costs, tune=dict(tune), full_planes=case.full)


def _predict_sweep(path, variant, names, costs):
    groups = [(min_path_nodes(CS.headline_arm(variant).graph), _lengths(variant, names))]
    if path in ("multi", "multi2"):
        groups.append((min_path_nodes(_chain_graph()[0]), [len(_chain_graph()[1]), 0]))
    if path.startswith("ss"):
        groups.append((min_path_nodes(_chain_graph()[0]), _lengths(variant, names)))
    return SM.predict_chunk(path, groups, costs)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_arm_graph_is_what_it_says():
    """rows, min_path_nodes, the predecessor order at the rejoin row under both switches, kept D rows all along the arm"""
    from poasta_amd import aligner
    for variant in ALL3:
        arm = CS.headline_arm(variant)
        g = arm.graph
        assert g.n == 2 + 600 + 2500 + 99 and min_path_nodes(g) == 600
        preds = g.predecessors(arm.rejoin).tolist()
        assert preds == ([arm.feeders[1], arm.feeders[0]] if variant == "arm_first" else list(arm.feeders))
        assert (arm.rejoin == g.end) == (variant == "into_end")
        rows = aligner.DeviceGraph(g).node_rows().astype(np.int64)
        kept = CS.kept_rows(g, rows)
        on_arm = np.zeros(g.n, bool)
        on_arm[rows[np.array(arm.arm_ids)]] = True
        assert int((kept & on_arm).sum()) >= 190, int((kept & on_arm).sum())
    bare = CS.arm_graph(600, 2500, 300, 17)
    assert bare.graph.n == 3102 and min_path_nodes(bare.graph) == 600
    # the relative encoding's shapes: the rejoin edge's offset pred_k = depth(arm's last node) + 1 - depth(rejoin node) is the arm's
    # length, and e * pred_k does not fit 16 bits (poa_graph.cpp: pred_k; poa_forward_px.hpp: pack16 / clamp16 on pred_k * e)
    for shape, site in (("one-strip", "px<0>,relative"), ("strips", "pxmw,relative")):
        A, costs, L = CS.RELATIVE_SHAPES[shape]
        rel = CS.relative_arm(shape)
        depth = _depths(rel.graph)
        pred_k = depth[rel.feeders[1]] + 1 - depth[rel.rejoin]
        assert pred_k == A and pred_k * costs[2] > 65535
        lengths = [len(q) for q in CS.relative_reads(shape)]
        assert lengths == [L, L, 0, 1]
        p = DLM.predict(rel.graph, lengths, costs)
        assert CS.score_ub(costs[1], costs[2], L, 1500) > 65534 >= 2 * (costs[1] + costs[2] * L)
        assert DLM.site_of(p) == site and p["layout"] == {"u16", "compact", "relative"}, (shape, DLM.site_of(p))
    assert DLM.predict(CS.relative_arm("strips").graph, [1300, 1300, 0, 1], CS.RELATIVE_SHAPES["strips"][1])["strips"] == 2


def _depths(g):
    """nodes on the shortest path from the start, per node"""
    depth = {g.start: 0}
    frontier = [g.start]
    while frontier:
        nxt = []
        for v in frontier:
            for s in g.successors(v).tolist():
                if s not in depth:
                    depth[s] = depth[v] + 1
                    nxt.append(s)
        frontier = nxt
    return depth


def test_case_table_meets_the_conditions_and_reaches_every_family(oracle):
    """Every case through clamp_profile (per variant and profiled read, under the batch's own ub) and through the restated rules:
    the launch each run stands for is the one its entry names, the cells are u16, and together the table reaches every kernel
    family and every (storage format, limit) pair of REQUIRED_*."""
    assert len(BY_NAME) == len(CASES)
    sites, formats, sweep_sites = set(), set(), set()
    n_profiles = 0
    for c in CASES:
        for variant in c.variants:
            d = _arm_data(oracle, variant)
            assert c.variants[0] == "rejoin"
            if c.family == "dense":
                assert len(c.reads) <= 16 and {"empty", "one"} <= set(c.reads)
                max_len = max(_lengths(variant, c.reads))
                for tune, site in c.runs:
                    p = _predict_dense(c, variant, tune)
                    assert DLM.site_of(p) == site and p["cells"] == "u16", (c.name, tune, DLM.site_of(p))
                    fmt = DLM.tb_format_of(p)
                    # a run whose own format has a higher limit than the case's is there as the yardstick among the formats
                    own = {4: L14, 3: L12, 2: L14, 1: L16, 0: L16, "u16-full": L16}[fmt]
                    assert own >= c.limit
                    if own == c.limit:
                        formats.add((fmt, own))
                    sites.add(site)
                assert any({4: L14, 3: L12, 2: L14, 1: L16, 0: L16, "u16-full": L16}[DLM.tb_format_of(_predict_dense(c, variant, t))] == c.limit
                           for t, _ in c.runs), c.name
                for name in c.profiled:
                    assert name in c.reads
                    d.profile(name, c.costs, c.limit, max_len, all_d=c.full)
                    n_profiles += 1
            else:
                for path, names in c.runs:
                    assert len(names) <= 16
                    launches = _predict_sweep(path, variant, names, c.costs)
                    assert all(la.cells == "u16" for la in launches), (c.name, path)
                    sweep_sites.update(la.site for la in launches)
                    max_len = max(_lengths(variant, names))
                    for name in c.profiled:
                        if name in names:
                            d.profile(name, c.costs, c.limit, max_len, all_d=True)
                            n_profiles += 1
                assert all(any(name in names for _, names in c.runs) for name in c.profiled), c.name
                assert "wrap" in c.variants, c.name      # every results-level case also runs the wrap-sensitive arm
                if variant == "wrap":
                    for name in c.profiled:
                        _wrap_would_win(d, name, c.costs)
    assert REQUIRED_DENSE <= sites, sorted(REQUIRED_DENSE - sites)
    assert REQUIRED_FORMATS <= formats, sorted(map(str, REQUIRED_FORMATS - formats))
    assert REQUIRED_SWEEP <= sweep_sites, sorted(REQUIRED_SWEEP - sweep_sites)
    assert n_profiles >= 60
    # several strips where the table says so: the carries of the arm rows cross a strip boundary
    p = _predict_dense(BY_NAME["packed-strips"], "rejoin", BY_NAME["packed-strips"].runs[0][0])
    assert (p["strip"], p["strips"], p["waves"]) == (512, 3, 3)
    p = _predict_dense(BY_NAME["packed-strips"], "rejoin", BY_NAME["packed-strips"].runs[1][0])
    assert (p["strip"], p["strips"], p["waves"]) == (1024, 2, 2)
    assert [_predict_dense(BY_NAME["full-strips"], "rejoin", t)["strips"] for t, _ in BY_NAME["full-strips"].runs] == [2, 3]
    assert {s for la in _predict_sweep("score", "rejoin", Q1300, C4630) for s in SM.strips_of(la)} == {1, 2}
    # two-piece: u16 cells by the first piece's costs
    two = set()
    d = _arm_data(oracle, "rejoin")
    for name, path, names in CASES_2P:
        if path == "dense2":
            p = TPS.predict(d.g, _lengths("rejoin", names), C2P_STEEP, False)
            assert p["elem"] == 2 and p["ub"] == 36012
            two.add("dense2-u16")
        else:
            for c2 in (C2P, C2P_STEEP):
                launches = _predict_sweep(path, "rejoin", names, c2)
                assert all(la.cells == "u16" for la in launches)
                two.update(la.site for la in launches)
    assert REQUIRED_2P <= two, sorted(REQUIRED_2P - two)
    _two_piece_presence(d, "r600")
    _two_piece_presence(d, "r1300")
    assert max(int(p[p != INF].max()) for p in d.planes2("r1300", C2P)) <= 65534      # the cheap second piece: nothing to clamp


def _wrap_would_win(d, name, costs):
    """from the oracle alone, on the "wrap" arm: in at least 300 columns of the rejoin row's predecessors the arm's value is
    finite, at least 65 536, and less 65 536 below the backbone's"""
    feeders = tuple(int(d.rows[v]) for v in d.arm.feeders)
    n = CS.wrap_margin(d.planes(name, costs)[0], feeders)
    assert n >= 300, (name, costs, n)


def _two_piece_presence(d, name):
    """from the oracle alone: under C2P_STEEP each of the five planes holds at least 10 000 finite values above 65534, and the
    score is below that"""
    planes = d.planes2(name, C2P_STEEP)
    over = [int(((p != INF) & (p > 65534)).sum()) for p in planes]
    assert min(over) >= 10000, over
    assert int(planes[0][d.rows[d.g.end], len(d.reads[name])]) < 65535
    return planes


DERIVE_COSTS = ((4, 6, 8), (255, 6, 8))


@pytest.mark.parametrize("variant", ALL3)
def test_derivation_on_clamped_planes(derive_harness, oracle, variant):
    """tbd_i_extends / tbd_d_extends on the planes as code_fmt 4 stores them: M and the kept D rows at or above 0x3FFF read INF,
    and the flag bits of such an M cell are undefined, so the derivation runs once with them cleared and once with them set.
    The derived flag equals the true one for EVERY cell whose carried value is finite and below the limit (the walks' targets
    are at most the carried value, a clamped cell lies above all of them); the test counts those cells itself."""
    X = derive_harness
    d = _arm_data(oracle, variant)
    g = d.g.as_dict()
    arrs = [np.ascontiguousarray(g[k], dtype=(np.uint8 if k == "symbol" else np.uint32)) for k in ("symbol", "succ_off", "succ", "pred_off", "pred")]
    head = (int(g["n"]), int(g["start"]), int(g["end"]))
    is_chain = np.zeros(head[0], np.uint8)
    assert X.derive_host_chain_nodes(*head, *[_p(a) for a in arrs], _p(is_chain)) == 0
    for costs in DERIVE_COSTS:
        for name in ("r600", "n600") if costs[0] == 255 else ("r600",):
            q = np.ascontiguousarray(d.reads[name], np.uint8)
            od = d.og.dense_align(q, oracle.Costs(*costs), planes=True)
            m, i, dd = (np.ascontiguousarray(od[k][d.orank]) for k in "MID")      # by node
            kept_by_node = d.kept[d.rows]
            assert int(((m != INF) & (m >= L14)).sum()) >= 10000 and int(((dd[kept_by_node] != INF) & (dd[kept_by_node] >= L14)).sum()) >= 10000
            want_b = int(((i != INF) & (i < L14)).sum())
            want_d = int(((dd[is_chain != 0] != INF) & (dd[is_chain != 0] < L14)).sum())
            assert (i[:, 0] == INF).all() and want_b > 100000 and want_d > 100000
            for fill in (0, 1):
                out = np.zeros(8, np.uint64)
                assert X.derive_host_check_clamped(*head, *[_p(a) for a in arrs], costs[1], costs[2], _p(q), len(q), _p(m), _p(i), _p(dd), L14, fill,
                                                   _p(out)) == 0
                assert int(out[2]) == 0 and int(out[3]) == 0, "derived flag differs: state %d row %d column %d (B: %d, D: %d cells differ), %s %r flags %d" % (
                    int(out[5]), int(out[6]), int(out[7]), int(out[2]), int(out[3]), name, costs, fill)
                assert int(out[4]) == 0, "the derivation read a D row the compact layout does not keep"
                assert (int(out[0]), int(out[1])) == (want_b, want_d)      # no cell left out


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------------
def _costs_obj(engine, costs):
    if len(costs) == 3:
        return engine.GapAffine(costs[0], costs[2], costs[1])      # the reference's order: (mismatch, extend, open)
    return engine.GapAffine2Piece(*costs)


def _same(a, b, tag):
    assert np.array_equal(a.score, b.score), (tag, "score", a.score.tolist(), b.score.tolist())
    assert np.array_equal(a.flags, b.flags), (tag, "flags")
    assert np.array_equal(a.pair_off, b.pair_off) and np.array_equal(a.pairs, b.pairs), (tag, "pairs")


def _where(sel, got, want):
    bad = np.argwhere(sel & (got != want))
    if len(bad) == 0:
        return None
    r, c = (int(t) for t in bad[0])
    return "%d cells differ, first at row %d column %d: got %d (0x%X), want %d (0x%X)" % (len(bad), r, c, int(got[r, c]), int(got[r, c]),
                                                                                         int(want[r, c]), int(want[r, c]))


def _assert_words(fetched, planes, kept, tag):
    """code_fmt 4, every cell of columns 0..L: a value below 0x3FFF is stored exactly with its two flag bits; a value at or above
    it, or INF, reads 0x3FFF in the score field; a kept D value below 0x3FFF is stored exactly, any other reads at least 0x3FFF.
    Nothing finer is defined for such a D cell: the kernel computes D = min(D[p] + e, M[p] + o + e) from an M that reads INF
    from 0x3FFF on, so where the oracle's D >= 0x3FFF comes from such an M the stored u16 is another value >= 0x3FFF, and every
    reader (the forward rows: a sum with M < 0x3FFF wins; the traceback: targets are at most the score) treats both alike."""
    m_raw, d, d_kept = fetched
    assert np.array_equal(d_kept, kept), tag
    assert (d[~d_kept] == 0xFFFF).all(), tag
    m_exact, m_word, d_exact, d_word = stored_words(*planes)
    assert _where(m_exact, m_raw, m_word) is None, (tag, "M", _where(m_exact, m_raw, m_word))
    assert ((m_raw[~m_exact] & 0x3FFF) == 0x3FFF).all(), (tag, "M: a value at or above the limit does not read 0x3FFF",
                                                           _where(~m_exact, m_raw & 0x3FFF, np.full(m_raw.shape, 0x3FFF, np.uint16)))
    km = np.broadcast_to(kept[:, None], d.shape)
    assert _where(km & d_exact, d, d_word) is None, (tag, "D", _where(km & d_exact, d, d_word))
    assert (d[km & ~d_exact] >= 0x3FFF).all(), (tag, "D: a value at or above the limit reads below 0x3FFF")
    return int(m_exact.sum()) + int((~m_exact).sum()), int(km.sum())


def _assert_full_planes(rb, d, case, i, name, tag):
    """u16 full planes of query i, every cell of M, I and D: the oracle's value if it is at most 65534, else INF"""
    got3 = rb.planes(i)
    want3 = d.planes(name, case.costs)
    over = 0
    for pname, got, want in zip("MID", got3, want3):
        exp = CS.expected_u16(want)
        over += int(((want != INF) & (want > 65534)).sum())
        assert _where(np.ones(exp.shape, bool), got, exp) is None, (tag, name, pname, _where(np.ones(exp.shape, bool), got, exp))
    return over


# ---- GPU: the dense one-piece pass ----------------------------------------------------------------------------------------------
DENSE_PARAMS = [(c.name, v) for c in CASES if c.family == "dense" and c.name != "band" for v in c.variants]


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", DENSE_PARAMS, ids=["%s-%s" % p for p in DENSE_PARAMS])
def test_gpu_dense_clamped(engine, oracle, name, variant):
    """One dense run per entry of the case's `runs`: the launch record and the layout equal the restated rule's; score, flags and
    every (rpos, qpos) equal the oracle's and hence each other's across the formats; code_fmt 4: every stored word of every
    query; full planes: every M / I / D cell of every query."""
    case = BY_NAME[name]
    d = _arm_data(oracle, variant)
    qs = d.qs(case.reads)
    max_len = max(len(q) for q in qs)
    for r in case.profiled:
        d.profile(r, case.costs, case.limit, max_len, all_d=case.full)      # the conditions, before any engine result
    D = d.dense(case.reads, case.costs)
    first, n_words, n_full = None, 0, 0
    for tune, site in case.runs:
        pred = _predict_dense(case, variant, tune)
        rb, res = DLM._run(engine, d.g, qs, case.costs, dict(tune), case.full)
        try:
            tag = (name, variant, site)
            if not DLM._ambient():
                assert rb.launches() == [DLM.launch_of(pred)], (tag, rb.launches(), DLM.launch_of(pred))
                assert rb.layout() == pred["layout"], (tag, rb.layout())
                assert not rb.band_info()["used"], tag
            DLM._assert_equals_oracle(res, D, len(qs), str(tag))
            if first is None:
                first = res
            _same(res, first, tag)
            if case.words and pred["code_fmt"] == 4 and "derived_gaps" in rb.layout():
                for i, r in enumerate(case.reads):
                    cells, d_cells = _assert_words(rb.compact_planes(i), d.planes(r, case.costs), d.kept, tag + (r,))
                    assert cells == d.g.n * (len(qs[i]) + 1) and d_cells == int(d.kept.sum()) * (len(qs[i]) + 1)      # no cell left out
                    n_words += 1
            if case.full and "compact" not in rb.layout() and "u16" in rb.layout():
                over = sum(_assert_full_planes(rb, d, case, i, r, tag) for i, r in enumerate(case.reads))
                assert over >= 30000, over      # finite values above 65534 in the planes compared
                n_full += len(case.reads)
        finally:
            rb.close()
    if not DLM._ambient():      # the cell-level comparisons ran: every query once under code_fmt 4, every query under every full-plane run
        assert n_words == (len(case.reads) if case.words else 0) and n_full == (len(case.reads) * len(case.runs) if case.full else 0), (n_words, n_full)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["one-strip", "strips"])
def test_gpu_relative_edge_cost_clamps(engine, oracle, shape):
    """The relative encoding (cells hold score - e * (depth of the row - column)) on arm_graph(1500, A, 700): ub rules the absolute
    u16 cells out, 2 (o + e L) lets the relative ones in (clamp_shapes.RELATIVE_SHAPES; one strip: px<0>, two strips: pxmw).  The
    relative cell values themselves stay at or below 2 (o + e j): what clamps here is the edge cost alone, e * pred_k = 65 580
    resp. 65 550 on the edge from the arm's last node into the rejoin node (pack16 / clamp16 in poa_forward_px.hpp), asserted
    from the graph in test_arm_graph_is_what_it_says.  Both are just above 65 535: wrapped, they would be 44 resp. 14, and the
    read that follows the arm's tail would align through the arm; the oracle's alignment of it passes the arm by, which is
    asserted first.  Results equal the u32 planes' (planes = 32) and the oracle's."""
    rel = CS.relative_arm(shape)
    g, costs = rel.graph, CS.RELATIVE_SHAPES[shape][1]
    qs = CS.relative_reads(shape)
    depth = _depths(g)
    assert (depth[rel.feeders[1]] + 1 - depth[rel.rejoin]) * costs[2] > 65535
    qseq, qoff = pack_queries(qs)
    D = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq, qoff, oracle.Costs(*costs), threads=3)
    assert not set(rel.arm_ids) & {rpos for rpos, _ in oracle.batch_alignment(D, 1)}      # the arm-tail read's alignment uses no arm node
    pred = DLM.predict(g, [len(q) for q in qs], costs)
    rb, res = DLM._run(engine, g, qs, costs, {})
    try:
        if not DLM._ambient():
            assert rb.launches() == [DLM.launch_of(pred)] and rb.layout() == {"u16", "compact", "relative"}, (rb.launches(), rb.layout())
        DLM._assert_equals_oracle(res, D, len(qs), "relative " + shape)
    finally:
        rb.close()
    rb, u32 = DLM._run(engine, g, qs, costs, {"planes": 32})
    try:
        assert rb.layout() == set()
        _same(res, u32, "relative against u32 planes")
    finally:
        rb.close()


# ---- GPU: the banded pair -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ALL3)
def test_gpu_banded_default_run(engine, oracle, band_harness, variant):
    """A default run (POA_BAND unset) under (4, 6, 8).  The band plan of every arm graph has a band (D = 413 resp. 385 for 600
    symbols, asserted), and the reads' scores are within e * (D - 4): the banded kernel certifies them, and its windows take in
    arm rows, whose cells are clamped.  band_info equals the prediction from the plan's D and the oracle's scores; the window
    words of every certified query equal those of the windowed model (tests/band_model.py) under the three-part rule; results
    equal the oracle's."""
    from test_compact_planes import Batch
    case = BY_NAME["band"]
    d = _arm_data(oracle, variant)
    for r in case.profiled:
        d.profile(r, case.costs, case.limit, 600)
    b = Batch(engine, oracle, d.g, d.qs(case.reads), clamped=True)
    assert np.array_equal(b.kept, d.kept)
    assert b.plan(band_harness, 600).D == (385 if variant == "into_end" else 413)
    want, keep = b.predict(band_harness, case.costs, 1 << 30)
    assert keep[0] and keep[1] and want["min_d"] >= 4, (want, keep)
    # the windows of the certified reads hold clamped cells: the banded pass meets them
    win = b.window(band_harness, 0)
    model = b.model(band_harness, 0, case.costs)
    assert int((win & (model[0] != INF) & (model[0] >= L14)).sum()) >= 10000
    rb = b.open()
    try:
        b.run(rb, case.costs, {})
        b.check_banded(band_harness, rb, case.costs, {}, want_keep=keep)
        if not DLM._ambient():
            assert rb.band_info() == want, (rb.band_info(), want)
    finally:
        rb.close()


# ---- GPU: the sweep family ------------------------------------------------------------------------------------------------------
def _sm():
    import test_sweep_matrix as TSM
    return TSM


SWEEP_COSTS = [C4630, C25530]
SWEEP_IDS = ["4_6_30", "255_6_30"]


def _profiles(d, case, names):
    max_len = max(len(d.reads[k]) for k in names)
    for r in case.profiled:
        if r in names:
            d.profile(r, case.costs, case.limit, max_len, all_d=True)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["rejoin", "into_end", "wrap"])
@pytest.mark.parametrize("costs", SWEEP_COSTS, ids=SWEEP_IDS)
def test_gpu_score_mode_clamped(engine, oracle, costs, variant):
    """Score mode in u16: three 600-symbol reads run the packed sweep (poa_sweep_px_kernel), the 1 300-symbol batch the general
    one at one and two strips; plane_bytes says which ran."""
    TSM = _sm()
    case = BY_NAME["sweep-score-" + "_".join(map(str, costs))]
    d = _arm_data(oracle, variant)
    ran = set()
    for path, names in case.runs:
        _profiles(d, case, names)
        la, = _predict_sweep(path, variant, names, costs)
        qs = d.qs(names)
        cfg = engine.make_config("score")
        rb = engine.ResidentBatch(d.g, *pack_queries(qs), config=cfg)
        try:
            rb.run(_costs_obj(engine, costs), None, cfg)
            res = rb.fetch(want_pairs=False)
            assert rb.layout() == {"u16"} and res.stats["n_chunks"] == 1
            assert res.stats["plane_bytes"] == SM.sweep_plane_bytes([(la, TSM._sweep_rows_of(engine, d.g)[1])]), (la.site, res.stats["plane_bytes"])
        finally:
            rb.close()
        TSM._assert_equals_oracle(res, d.dense(names, costs), np.arange(len(qs)), (variant, la.site), pairs=False)
        ran.add(la.site)
    assert ran == {"poa_sweep_px_kernel", "poa_sweep_kernel<2,u16>"}


CKPT_PARAMS = [(c, v) for c in SWEEP_COSTS for v in WRAP2] + [(C2P, "rejoin"), (C2P_STEEP, "rejoin")]
CKPT_IDS = ["%s-%s" % (i, v) for i in SWEEP_IDS for v in WRAP2] + ["2piece", "2piece-steep"]
MULTI_PARAMS, MULTI_IDS = CKPT_PARAMS[:4] + CKPT_PARAMS[5:], CKPT_IDS[:4] + CKPT_IDS[5:]


@pytest.mark.gpu
@pytest.mark.parametrize("costs,variant", CKPT_PARAMS, ids=CKPT_IDS)
def test_gpu_checkpointed_clamped(engine, oracle, costs, variant):
    """Checkpointed mode (two-piece costs: POA_MODE_CHECKPOINT2) under the default plan and under segments of 50 rows, whose
    snapshot rows are arm rows full of clamped cells (asserted from the plan and the oracle's plane): score, flags and the
    full pair list.  Under (4, 30, 6, 1, 24) no plane exceeds u16 (module docstring): that run is there for the cost model."""
    TSM = _sm()
    two = len(costs) == 5
    d = _arm_data(oracle, variant)
    names = Q1300
    if costs == C2P:
        over = None
    elif two:
        planes = _two_piece_presence(d, "r600")
        over = (planes[0] != INF) & (planes[0] > 65534)
    else:
        case = BY_NAME["sweep-ckpt-" + "_".join(map(str, costs))]
        _profiles(d, case, names)
        m = d.planes("r600", costs)[0]
        over = (m != INF) & (m >= L16)
    boundary, _ = engine._device_graph(d.g).checkpoint_plan(CKPT_ROWS, two_piece=two)
    snap_rows = np.asarray(boundary, np.int64)[1:-1]
    assert len(snap_rows) >= 50 and (over is None or int(over[snap_rows - 1].any(axis=1).sum()) >= 5)      # snapshot rows that hold clamped cells
    la, = _predict_sweep("ckpt2" if two else "ckpt", variant, names, costs)
    assert la.site == ("poa2_ckpt<u16,2>" if two else "poa_ckpt<2,u16>")
    qs = d.qs(names)
    D = d.dense(names, costs)
    for plan in (0, CKPT_ROWS):
        cfg = engine.make_config("checkpoint2" if two else "checkpoint", **({"ckpt_rows": plan} if plan else {}))
        rb = engine.ResidentBatch(d.g, *pack_queries(qs), config=cfg)
        try:
            rb.run(_costs_obj(engine, costs), None, cfg)
            res = rb.fetch()
            assert rb.layout() == {"u16"} and res.stats["n_chunks"] == 1, (plan, rb.layout())
            assert res.stats["plane_bytes"] == SM.ckpt_plane_bytes("u16", TSM._stored_rows(engine, d.g, plan, two), [len(q) for q in qs]), plan
        finally:
            rb.close()
        TSM._assert_equals_oracle(res, D, np.arange(len(qs)), (la.site, plan))


def _split(engine, res, counts):
    """a multi-graph result cut into one BatchResult per graph"""
    out, first = [], 0
    for n in counts:
        lo, hi = int(res.pair_off[first]), int(res.pair_off[first + n])
        out.append(engine.BatchResult(res.score[first:first + n], res.pairs[lo:hi], res.pair_off[first:first + n + 1] - res.pair_off[first],
                                      res.flags[first:first + n], res.stats))
        first += n
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("costs,variant", MULTI_PARAMS, ids=MULTI_IDS)
def test_gpu_multi_graph_checkpointed_clamped(engine, oracle, costs, variant):
    """MultiGraphBatch, one-piece and two-piece: the arm graph beside a 40-node chain and the empty graph.  The arm graph's and
    the chain's queries against the oracle on that graph; the empty graph's against the one-shot dense call on it."""
    TSM = _sm()
    two = len(costs) == 5
    d = _arm_data(oracle, variant)
    if two:
        _two_piece_presence(d, "r600")
    else:
        _profiles(d, BY_NAME["sweep-multi-" + "_".join(map(str, costs))], Q1300)
    chain, chain_read = _chain_graph()
    empty = GraphBuilder().finish()
    graphs = [d.g, chain, empty]
    seqs = [d.qs(Q1300), [chain_read, np.zeros(0, np.uint8)], [np.frombuffer(b"ACGT", np.uint8), np.zeros(0, np.uint8)]]
    la, = _predict_sweep("multi2" if two else "multi", variant, Q1300, costs)
    assert la.site == ("poa2_ckpt_multi<u16,2>" if two else "poa_ckpt_multi<2,u16>")
    cfg = engine.make_config("checkpoint2" if two else "checkpoint")
    mb = engine.MultiGraphBatch(graphs, seqs, config=cfg, two_piece=two)
    try:
        mb.run(_costs_obj(engine, costs), None, cfg)
        res = mb.fetch()
    finally:
        mb.close()
    assert res.stats["n_chunks"] == 1
    want_bytes = sum(SM.ckpt_plane_bytes("u16", TSM._stored_rows(engine, g, 0, two), [len(q) for q in s]) for g, s in zip(graphs, seqs))
    assert res.stats["plane_bytes"] == want_bytes, (res.stats["plane_bytes"], want_bytes)      # u16 cells
    parts = _split(engine, res, [len(s) for s in seqs])
    TSM._assert_equals_oracle(parts[0], d.dense(Q1300, costs), np.arange(len(Q1300)), "arm graph")
    cq, co = pack_queries(seqs[1])
    og = oracle.OracleGraph.from_csr(chain.as_dict())
    if two:
        with oracle.two_piece(costs[4], costs[3]):
            Dc = og.dense_batch(cq, co, oracle.Costs(costs[0], costs[2], costs[1]))
    else:
        Dc = og.dense_batch(cq, co, oracle.Costs(*costs))
    TSM._assert_equals_oracle(parts[1], Dc, np.arange(2), "chain")
    al = engine.PoastaAligner((engine.Affine2PieceDijkstra if two else engine.AffineMinGapCost)(_costs_obj(engine, costs)))
    _same(parts[2], al.align_batch(empty, seqs[2]), "empty graph")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", WRAP2)
@pytest.mark.parametrize("costs", SWEEP_COSTS, ids=SWEEP_IDS)
def test_gpu_score_sets_clamped(engine, oracle, costs, variant):
    """The full matrix of six reads x (arm graph, chain) in one score set, u16 cells: the plain form; capped at the score (no pair
    is CAPPED), at 65 535 (0xFFFF is the cells' INF: such a cap never fires and every score comes back), at score - 1 and at 3/4 of
    the score (every pair is CAPPED, and with cap_stride = 1 the one-strip pairs stop after the first check row whose smallest M
    of the oracle's plane is above the cap, as in tests/test_scoreset_cap.py: at 3/4 that row lies behind the arm and the rejoin
    row); the best-of form field by field, and under a ceiling at 3/4 of each query's best score, where every wave stops at the
    row the oracle's plane says."""
    from test_scoreset_best import _check as check_best
    from test_scoreset_cap import _expected_swept
    TSM = _sm()
    case = BY_NAME["sweep-scoreset-" + "_".join(map(str, costs))]
    d = _arm_data(oracle, variant)
    names = case.runs[0][1]
    _profiles(d, case, names)
    chain, _ = _chain_graph()
    graphs, seqs = [d.g, chain], d.qs(names)
    nq, ng = len(seqs), 2
    qseq, qoff = pack_queries(seqs)
    Dc = oracle.OracleGraph.from_csr(chain.as_dict()).dense_batch(qseq, qoff, oracle.Costs(*costs), threads=4)
    want = np.stack([d.dense(names, costs)["score"], Dc["score"]], axis=1).reshape(-1).astype(np.uint32)      # pair p = (p // 2, p % 2)
    assert int(want.max()) < 65535
    flags0 = np.repeat(np.array([SHORT_QUERY if len(q) == 1 else 0 for q in seqs], np.uint32), ng)
    pq = np.repeat(np.arange(nq), ng)
    rows = np.tile(np.array([d.g.n, chain.n]), nq) * np.repeat([2 if len(q) + 1 > 1024 else 1 for q in seqs], ng)
    sites = {la.site for la in _predict_sweep("ss", variant, names, costs)}
    assert sites == {"scoreset<PX>", "scoreset<2,u16>", "scoreset<1,u16>"}, sites
    cells = "u16"
    want_bytes = 0
    for qi in range(nq):
        for g in graphs:
            cls = SM.scoreset_class(cells, True, SM.pitch_of(len(seqs[qi])))
            want_bytes += 2 * TSM._sweep_rows_of(engine, g)[1] * (2048 if cls == "PX" else SM.pitch_of(len(seqs[qi])) * 2)
    cobj = _costs_obj(engine, costs)
    cfg = engine.make_config("score", cap_stride=1)
    ss = engine.ScoreSet(graphs, seqs)
    try:
        ss.run(cobj, config=cfg)
        score, flags, st = ss.fetch()
        assert st["n_chunks"] == 1 and st["plane_bytes"] == want_bytes, (st["plane_bytes"], want_bytes)
        assert np.array_equal(score, want) and np.array_equal(flags, flags0), ("plain", score.tolist(), want.tolist())
        for cap_name, cap in (("score", want), ("65535", np.full(len(want), 65535, np.uint32))):
            ss.run(cobj, config=cfg, cap=cap)
            score, flags, _ = ss.fetch()
            assert np.array_equal(score, want) and np.array_equal(flags, flags0), ("cap = " + cap_name, score.tolist())
            assert np.array_equal(ss.swept_rows(), rows), "cap = " + cap_name
        assert (want > 0).all()
        m_planes = {k: d.planes(k, costs)[0].copy() for k in names if 400 <= len(d.reads[k]) <= 1023}
        assert len(m_planes) == 3
        arm_rows = d.rows[np.array(d.arm.arm_ids)]
        for cap_name, cap in (("score - 1", want - 1), ("3/4 score", (3 * want.astype(np.int64)) // 4)):
            cap = cap.astype(np.uint32)
            ss.run(cobj, config=cfg, cap=cap)
            score, flags, _ = ss.fetch()
            assert (score == NONE).all() and np.array_equal(flags, flags0 | CAPPED), ("cap = " + cap_name, score.tolist())
            swept = ss.swept_rows()
            stops = {k: _expected_swept(engine, d.g, m_planes[k], int(cap[qi * ng]), 1) for qi, k in enumerate(names) if k in m_planes}
            for qi, k in enumerate(names):
                if k in m_planes:
                    assert swept[qi * ng] == stops[k], ("cap = " + cap_name, k, int(swept[qi * ng]), stops[k])
            if cap_name == "3/4 score" and variant == "rejoin":      # stops behind the arm's rows and the rejoin row: the row minima there rest on the clamped rows
                assert sum(int(arm_rows.max()) + 1 < s < d.g.n for s in stops.values()) >= 2, stops
        for slack in (0, 3):
            ss.run(cobj, config=cfg, best=True, slack=slack)
            check_best(ss, want, pq, nq, slack, None, flags0, ("best", slack))
            swept = ss.swept_rows()
            _, fl, _ = ss.fetch()
            assert (swept <= rows).all() and (swept[(fl & CAPPED) == 0] == rows[(fl & CAPPED) == 0]).all()
        # a ceiling at 3/4 of the query's best score: nothing is ever published, every pair's cap is the ceiling throughout
        best = want.reshape(nq, ng).min(axis=1).astype(np.int64)
        limit = ((3 * best) // 4).astype(np.uint32)
        ss.run(cobj, config=cfg, best=True, slack=0, limit=limit)
        check_best(ss, want, pq, nq, 0, limit, flags0, "best under a ceiling")
        swept = ss.swept_rows()
        for qi, k in enumerate(names):
            if k in m_planes:
                assert swept[qi * ng] == _expected_swept(engine, d.g, m_planes[k], int(limit[qi]), 1), ("ceiling", k)
    finally:
        ss.close()


# ---- GPU: the two-piece dense pass ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_two_piece_dense_clamped(engine, oracle):
    """Two-piece dense pass in u16 cells under (4, 30, 6, 28, 60): the batch's results, and the five planes of a 600-symbol read
    cell for cell under the rule of tests/test_two_piece_shapes.py (the oracle's value if it is at most 65534, INF otherwise) —
    here with at least 10 000 finite values above 65534 in every plane, asserted from the oracle's planes."""
    d = _arm_data(oracle, "rejoin")
    oplanes = _two_piece_presence(d, "r600")
    qs = d.qs(Q600)
    pred = TPS.predict(d.g, [len(q) for q in qs], C2P_STEEP, False)
    assert pred["elem"] == 2
    al = TPS._aligner(engine, C2P_STEEP)
    res = al.align_batch(d.g, qs)
    assert TPS._elem_of(res.stats, d.g, [len(q) for q in qs]) == 2 and res.stats["n_chunks"] == 1
    TPS._assert_batch_equals_oracle(res, d.dense(Q600, C2P_STEEP), oracle, len(qs), "two-piece dense")
    got = al.planes_2piece(d.g, qs[0])
    over = 0
    for pname, a, b in zip(("M", "I1", "D1", "I2", "D2"), got, oplanes):
        want = CS.expected_u16(b)
        over += int(((b != INF) & (b > 65534)).sum())
        assert _where(np.ones(want.shape, bool), a, want) is None, (pname, _where(np.ones(want.shape, bool), a, want))
    assert over >= 50000


# ---- GPU: dense multi-graph batches and hybrid mode ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["one-strip", "wide"])
def test_gpu_multi_graph_dense_clamped(engine, oracle, wide):
    """MultiGraphBatch(dense=True) under (4, 6, 30): the arm graph beside the chain and the empty graph; wide: with the
    1 300-symbol read (POA_CFG_WIDE_QUERIES set by wide=None, the chunk runs the strip loop).  Per graph the results equal the
    one-shot dense call's on that graph and the oracle's, and the whole batch equals the checkpointed batch."""
    TSM = _sm()
    costs = C4630
    d = _arm_data(oracle, "rejoin")
    names = Q1300 if wide else Q600
    d.profile(names[0], costs, L16, max(len(d.reads[k]) for k in names))
    d.profile("r600", costs, L16, max(len(d.reads[k]) for k in names))
    chain, chain_read = _chain_graph()
    empty = GraphBuilder().finish()
    graphs = [d.g, chain, empty]
    seqs = [d.qs(names), [chain_read, np.zeros(0, np.uint8)], [np.frombuffer(b"ACGT", np.uint8), np.zeros(0, np.uint8)]]
    cobj = _costs_obj(engine, costs)
    mb = engine.MultiGraphBatch(graphs, seqs, dense=True)
    try:
        assert mb.wide == wide
        mb.run(cobj)
        res = mb.fetch()
        launches = mb.launches()
    finally:
        mb.close()
    assert launches and all(la["kernel"] == "packed" for la in launches), launches
    assert any(la.get("strips") for la in launches) == wide, launches
    ck = engine.MultiGraphBatch(graphs, seqs)
    try:
        ck.run(cobj)
        _same(res, ck.fetch(), "dense against checkpointed")
    finally:
        ck.close()
    parts = _split(engine, res, [len(s) for s in seqs])
    TSM._assert_equals_oracle(parts[0], d.dense(names, costs), np.arange(len(names)), "arm graph")
    al = engine.PoastaAligner(engine.AffineMinGapCost(cobj))
    for part, g, s in zip(parts, graphs, seqs):
        _same(part, al.align_batch(g, s), "one-shot dense call")


@pytest.mark.gpu
def test_gpu_hybrid_on_clamped_planes(engine, oracle):
    """Hybrid mode under (4, 6, 8) on a resident batch: the replay takes its order and its flags from a dense pass whose planes are
    full of clamped cells.  A hybrid run never bands (plan_dense_run: want_band needs dense mode) and keeps the generic walk, so
    its dense pass is px<3> over code_fmt 4: layout(), band_info() and tb_info() must say so (poa_batch_last_launch serves dense
    runs only), and a dense run of the same batch with band = 0, whose launch record and layout equal the rule's, must leave
    the same layout.  Every result equals the reference's search (astar_batch)."""
    d = _arm_data(oracle, "rejoin")
    names = ("r600", "r600b")
    for r in names:
        d.profile(r, C468, L14, 600)
    qs = d.qs(names)
    qseq, qoff = pack_queries(qs)
    pred = DLM.predict(d.g, [len(q) for q in qs], C468, tune={"band": 0})
    assert DLM.site_of(pred) == "px<3>" and pred["layout"] == {"u16", "compact", "derived_gaps"}
    rb = engine.ResidentBatch(d.g, qseq, qoff)
    try:
        rb.run(_costs_obj(engine, C468), None, engine.make_config("dense", band=0))
        rb.fetch()
        if not DLM._ambient():
            assert rb.launches() == [DLM.launch_of(pred)] and rb.layout() == pred["layout"], (rb.launches(), rb.layout())
        rb.run(_costs_obj(engine, C468), None, engine.make_config("hybrid"))
        res = rb.fetch()
        if not DLM._ambient():
            assert rb.layout() == pred["layout"], rb.layout()
            assert not rb.band_info()["used"], rb.band_info()
            assert rb.tb_info()["kernel"] == "generic", rb.tb_info()
    finally:
        rb.close()
    A = d.og.astar_batch(qseq, qoff, oracle.Costs(*C468), oracle.H_MINGAP, True, threads=2)
    for i in range(len(qs)):
        assert A["status"][i] == 0
        assert int(res.score[i]) == int(A["score"][i]), i
        assert res.raw_alignment(i) == oracle.batch_alignment(A, i), i
    assert np.array_equal(res.score, d.dense(names, C468)["score"])
