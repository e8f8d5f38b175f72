"""The one-wavefront-per-query kernels — sweep_rows / sweep_px_rows (poa_forward_sweep.hpp), ckpt_rows and the walk behind it
(poa_checkpoint.hpp), their two-piece form in poa_checkpoint2.hpp and their wrappers in poa_multi.hpp and poa_scoreset.hpp — at
every instantiation the launchers can pick and at the column, strip and segment edges.

CPU: tests/sweep_model.py restates what the eight paths launch; `CASES` lists every batch the GPU tests below run, and one test
walks the table through the restatement and asserts that it reaches every instantiation of REQUIRED, two, three and four strips
of the 1024-column classes, and queries of 0, 1 and 3 symbols inside every class wider than 64 columns that a chunk's widest pitch selects.

GPU: every comparison is bit for bit against the oracle (oracle.OracleGraph.dense_batch, under oracle.two_piece for the
two-piece model).  What ran is held against the restatement through layout() and poa_stats_t.plane_bytes.
  * the prefix ladder: the 1 101 prefixes of one read put the result column M[end][len] at every lane, register and column group
    of the first strip and at the first columns of the second, third and fourth.  On the 162-row graph the oracle's end row of
    the whole read equals the prefix scores, which is asserted once per ladder; on the chain-like graph it only bounds them (the
    recurrence opens a gap by the read's next symbol, see _ladder), so there the ladder is asserted to hold 300 distinct scores;
  * the top half of u16: costs at the largest extend the u16 bound allows, scores up to the bound itself;
  * walks that cross strip and segment boundaries: planted insertion and deletion runs, each asserted from the oracle's pair list
    before any GPU result is looked at.

Value-only mutants of the kernels and what these tests and the older ones make of them: profiles/pr_sweep_matrix/README.md."""
import functools
from collections import namedtuple

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

import sweep_model as SM
from test_two_piece_shapes import min_path_nodes

NONE = 0xFFFFFFFF
SHORT_QUERY, CAPPED = 0x08, 0x80
ACGT = np.frombuffer(b"ACGT", np.uint8)
FOREIGN = ord("N")      # a symbol no graph here holds

C1, C0, C101, C255 = (4, 6, 2), (4, 0, 2), (1, 0, 1), (255, 3, 1)      # (mismatch, open, extend)
T1, T0 = (4, 2, 6, 1, 24), (4, 2, 6, 0, 24)                            # (m, e1, o1, e2, o2): 4 / 6,24 / 2,1 and extend2 = 0
U32 = {"planes": 32}


# ---- graphs and reads ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _poa(kind):
    if kind == "small":     # 162 rows, in-degree 4: the slots are reused all the time
        return W.LayeredPOA(n_layers=40, width=4, indeg=4, seed=5)
    if kind == "chain":     # a backbone as long as the ladder's read
        return W.LinearishPOA(1100, 30, 15, seed=2)
    if kind == "walk":      # 1 382 rows
        return W.LinearishPOA(1300, 40, 20, seed=1)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _graph(kind):
    if kind == "five":      # 5 rows
        b = GraphBuilder()
        b.add_path(np.frombuffer(b"ACG", np.uint8))
        return b.finish()
    return _poa(kind).graph


@functools.lru_cache(maxsize=None)
def _mpn(kind):
    return min_path_nodes(_graph(kind))


@functools.lru_cache(maxsize=None)
def _read(kind):
    """the one read of a graph whose prefixes are its ladder and its windows"""
    if kind == "small":
        r = _poa(kind).queries(1, length=3100)[0]
    elif kind == "chain":
        r = _poa(kind).queries(1, length=2100)[0]
    else:
        r = ACGT[np.random.default_rng(31).integers(0, 4, 2100)]
    r = np.ascontiguousarray(r, np.uint8)
    r.setflags(write=False)
    return r


def _prefixes(kind, lengths):
    r = _read(kind)
    assert max(lengths) <= len(r)
    return [r[:L] for L in lengths]


def upto(n):
    return tuple(range(n + 1))


LADDER = upto(1100)
SHORT = (0, 1, 3)
WIN23 = SHORT + tuple(k * 1024 + d for k in (2, 3) for d in range(-4, 5))
EDGES = SHORT + (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
EDGES4 = EDGES + (3071, 3072)      # ... and the first column of the fourth strip: the 162-row graph's read is long enough
EDGES_Q1 = SHORT + (255, 256, 257, 510, 511)
EDGES_W1 = SHORT + (254, 255)


# ---- the case table: every batch the GPU tests run ------------------------------------------------------------------------------
Case = namedtuple("Case", "name path groups costs tune wide")     # groups: ((graph kind, query lengths), ...)


def _tune_id(tune, wide=False):
    return ("-".join("%s%d" % kv for kv in sorted(tune.items())) or "default") + ("-wide" if wide else "")


def _case(name, path, groups, costs, tune=None, wide=False):
    tune = tune or {}
    return Case("%s-%s-%s-%s" % (path, name, "_".join(map(str, costs)), _tune_id(tune, wide)), path, tuple(groups), costs,
                tuple(sorted(tune.items())), wide)


LADDER_BATCHES = (      # (name, lengths, tune, paths)
    ("q1", upto(511), {}, ("score", "ckpt")),
    ("one-strip", upto(1023), {}, ("score", "ckpt")),                   # score mode: the packed one-strip kernel
    ("one-strip", upto(1023), {"px": 0}, ("score",)),
    ("all", LADDER, {}, ("score", "ckpt")),
    ("win", WIN23, {}, ("score", "ckpt")),
    ("q1", upto(255), U32, ("score", "ckpt")),
    ("q2", upto(511), U32, ("score", "ckpt")),
    ("all", LADDER, U32, ("score", "ckpt")),
    ("win", WIN23, U32, ("score", "ckpt")),
)
LADDER_COSTS = {"small": (C1, C0, C101, C255), "chain": (C1, C0)}
TOP_L0 = (500, 1000, 1500)          # the Q1 class, one strip of the 1024-column classes, two strips


def top_extend(L0, mpn):
    """the largest extend that keeps u16 cells with open = 6 for a longest query of L0 symbols"""
    return (SM.U16_BOUND - 12) // (L0 + mpn)


# lengths of the planted reads of _cross_reads (short, ins1024, ins2048, del, diag, ins_del), one-piece / two-piece plants
WALK_LENGTHS = {False: (3, 1335, 2093, 1270, 1269, 1266), True: (3, 1335, 2093, 1269, 1304, 1266)}
WALK_SIDE = SHORT + (1023, 1024, 2048)      # the 162-row graph's prefixes that run beside them in a multi-graph batch


def _cases():
    out = []
    # -- the prefix ladder, score mode and checkpointed mode
    for kind, cost_sets in LADDER_COSTS.items():
        for costs in cost_sets:
            for name, lengths, tune, paths in LADDER_BATCHES:
                if name == "win" and kind != "small":
                    continue
                for path in paths:
                    out.append(_case("ladder-%s-%s" % (kind, name), path, [(kind, lengths)], costs, tune))
    # -- score sets: both ladders in one set, the three forms
    for costs in (C1, C0):
        for tune in ({}, U32, {"px": 0}):
            for path in ("ss", "ss_cap", "ss_best"):
                out.append(_case("ladder", path, [("small", LADDER + WIN23[3:]), ("chain", LADDER)], costs, tune))
    # -- two-piece: score mode, POA_MODE_CHECKPOINT2 and the score-set form at the window edges
    for costs in (T1, T0):
        for kind in ("small", "chain"):
            for wide in (False, True):
                lengths = EDGES4 if kind == "small" else EDGES
                out.append(_case("edges-" + kind, "score2", [(kind, lengths)], costs, U32 if wide else {}))
                out.append(_case("edges-" + kind, "ckpt2", [(kind, lengths)], costs, {}, wide))
        for tune in ({}, U32):
            out.append(_case("edges", "ss2", [("small", EDGES), ("chain", EDGES)], costs, tune))
    # -- multi-graph batches, one-piece and two-piece: the window edges per graph, batch by kernel class
    for path, cost_sets in (("multi", (C1, C0)), ("multi2", (T1, T0))):
        for costs in cost_sets:
            for name, lengths, tune in (("q1", EDGES_Q1, {}), ("q2", EDGES_Q1, U32), ("q1", EDGES_W1, U32), ("all", EDGES, {}), ("all", EDGES, U32)):
                out.append(_case("edges-" + name, path, [(k, EDGES4 if (k == "small" and name == "all") else lengths) for k in ("small", "chain", "five")],
                                 costs, tune))
    # -- the top half of u16: e* per batch, and e* + 1 (u32 by the bound)
    for L0 in TOP_L0:
        for de in (0, 1):
            costs = (255, 6, top_extend(L0, _mpn("small")) + de)
            name = "top-%d" % L0
            for path, tune in (("score", {}), ("score", {"px": 0}), ("ckpt", {}), ("ss", {}), ("ss_cap", {})):
                out.append(_case(name, path, [("small", SHORT + (L0, L0, L0, L0 - 1, L0))], costs, tune))
            out.append(_case(name, "multi", [("small", SHORT + (L0, L0, L0, L0 - 1, L0)), ("five", SHORT + (L0, L0, L0, L0 - 1, L0))], costs))
    # -- walks that cross strip and segment boundaries: the planted reads (WALK_LENGTHS), alone and next to the 162-row graph
    for costs in (C1, C0, T1):
        two = len(costs) == 5
        for wide in (False, True):
            out.append(_case("cross", "ckpt2" if two else "ckpt", [("walk", WALK_LENGTHS[two])], costs, {} if (two or not wide) else U32, wide and two))
        for tune in ({}, U32):
            out.append(_case("cross", "multi2" if two else "multi", [("small", WALK_SIDE), ("walk", WALK_LENGTHS[two])], costs, tune))
    return out


CASES = _cases()


def _launches(case):
    return SM.predict_chunk(case.path, [(_mpn(k), ls) for k, ls in case.groups], case.costs, dict(case.tune), case.wide)


def _select(path, name=None, **kw):
    sel = [c for c in CASES if c.path == path and (name is None or ("-%s-" % name) in c.name) and all(getattr(c, k) == v for k, v in kw.items())]
    assert sel, (path, name, kw)
    return sel


FIVE = [(1, "u16"), (2, "u16"), (1, "u32"), (2, "u32"), (4, "u32")]
REQUIRED = (
    {"poa_sweep_px_kernel"} | {"poa_sweep_kernel<%d,%s>" % qc for qc in FIVE}
    | {"poa_ckpt<%d,%s>" % qc for qc in FIVE}
    | {"poa_ckpt_multi<%d,%s>" % qc for qc in FIVE}
    | {"poa2_ckpt_multi<%s,%d>" % (c, q) for q, c in FIVE}
    | {"poa2_ckpt<u16,2>", "poa2_ckpt<u32,4>"}
    | {"%s<%s>" % (form, cls) for form in ("scoreset", "scoreset_capped", "scoreset_best")
       for cls in ("PX", "1,u16", "2,u16", "1,u32", "2,u32", "4,u32")})


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_selection_restated():
    """sweep_model.predict_chunk on shapes worked out by hand from run_sweep, run_ckpt, run_ckpt2, poa_multi_run and scoreset_run
    (poasta_amd/csrc/poa_engine.hip), launch_by_pitch and scoreset_class."""
    assert [SM.pitch_of(L) for L in (0, 62, 63, 64, 511, 512, 1023, 1024)] == [64, 64, 64, 128, 512, 576, 1024, 1088]
    assert SM.score_bound(6, 2, 1000, 900) == 12 + 2 * 1900 and SM.score_bound(6, 2, 0, 900) == 6 + 1800 and SM.score_bound(6, 2, 0, 0) == 0
    one = lambda path, lengths, costs=C1, mpn=40, **tune: SM.predict_chunk(path, [(mpn, lengths)], costs, tune)
    site = lambda *a, **k: [la.site for la in one(*a, **k)]
    # run_sweep: Q by the chunk's widest pitch; the packed kernel for one strip wider than 512 whose rows fit the chunk's regions
    assert site("score", (0, 511)) == ["poa_sweep_kernel<1,u16>"] and site("score", (0, 900, 600)) == ["poa_sweep_px_kernel"]      # 64 + 960 + 640 >= 512 * 3
    assert site("score", (512,) + (0,) * 8) == ["poa_sweep_kernel<2,u16>"]       # pitch_sum 576 + 8 * 64 < 512 * 9
    assert site("score", (512,) + (0,) * 8, mpn=40) != site("score", (512,) + (600,) * 8)
    assert site("score", (600,), px=0) == ["poa_sweep_kernel<2,u16>"] and site("score", (1024,)) == ["poa_sweep_kernel<2,u16>"]
    assert [site("score", (L,), planes=32)[0] for L in (255, 256, 511, 512)] == ["poa_sweep_kernel<%d,u32>" % q for q in (1, 2, 2, 4)]
    # the bound: 2 * 60 + 40 * (1000 + 900) > 65534
    assert site("score", (1000,), (255, 60, 40), 900) == ["poa_sweep_kernel<4,u32>"]
    assert one("score", (1000,), (255, 6, 63))[0].cells == "u16" and one("score", (1000,), (255, 6, 64))[0].cells == "u32"
    assert top_extend(1000, 40) == 63 and 12 + 63 * 1040 <= 65534 < 12 + 64 * 1040
    # two-piece: the sweeps run open' = open1 + extend1 - extend2, extend' = extend2; the checkpointed passes bound by the first piece
    assert SM.reduced(T1) == (4, 7, 1) and SM.reduced((4, 255, 255, 0, 9)) == (4, 510, 0)
    assert site("score2", (600,), T1) == ["poa_sweep_px_kernel"] and site("ckpt2", (3,), T1) == ["poa2_ckpt<u16,2>"]
    assert [la.site for la in SM.predict_chunk("ckpt2", [(40, (3,))], T1, None, True)] == ["poa2_ckpt<u32,4>"]
    # run_ckpt2 takes no tunables: planes = 32 does not widen it, wide_planes does; poa_multi_run_2piece honours either; the sweeps
    # of a two-piece model read the tunable and not wide_planes
    assert site("ckpt2", (3,), T1, planes=32) == ["poa2_ckpt<u16,2>"]
    assert [la.site for la in SM.predict_chunk("multi2", [(40, (3,))], T1, None, True)] == ["poa2_ckpt_multi<u32,1>"]
    assert [la.site for la in SM.predict_chunk("score2", [(40, (3,))], T1, None, True)] == ["poa_sweep_kernel<1,u16>"]
    assert site("ckpt2", (20000,), (4, 3, 6, 1, 24), 2000) == ["poa2_ckpt<u32,4>"]      # 12 + 3 * 22000 > 65534; the reduced costs would fit
    assert site("score2", (20000,), (4, 3, 6, 1, 24), 2000) == ["poa_sweep_kernel<2,u16>"]
    # checkpointed: no packed kernel
    assert site("ckpt", (600,)) == ["poa_ckpt<2,u16>"] and site("ckpt", (300,), planes=32) == ["poa_ckpt<2,u32>"]
    # multi-graph: u16 only if every graph's own bound allows it; one Q for the chunk
    multi = lambda groups, costs=C1, **tune: [la.site for la in SM.predict_chunk("multi", groups, costs, tune)]
    assert multi([(40, (100,)), (3, (511,))]) == ["poa_ckpt_multi<1,u16>"] and multi([(40, (100,)), (3, (512,))]) == ["poa_ckpt_multi<2,u16>"]
    assert multi([(40, (100,)), (3, (1100,))], (255, 40, 60)) == ["poa_ckpt_multi<4,u32>"]
    assert multi([(40, (100,)), (3, ())], planes=32) == ["poa_ckpt_multi<1,u32>"]
    assert [la.site for la in SM.predict_chunk("multi2", [(40, (300,))], T1, U32)] == ["poa2_ckpt_multi<u32,2>"]
    # score sets: a class per pair
    ss = SM.predict_chunk("ss_cap", [(40, (0, 511, 512, 1023, 1024))], C1)
    assert [(la.site, la.lengths) for la in ss] == [("scoreset_capped<PX>", (512, 1023)), ("scoreset_capped<1,u16>", (0, 511)), ("scoreset_capped<2,u16>", (1024,))]
    ss = SM.predict_chunk("ss_best", [(40, (0, 255, 256, 511, 512))], C1, U32)
    assert [(la.site, la.lengths) for la in ss] == [("scoreset_best<1,u32>", (0, 255)), ("scoreset_best<2,u32>", (256, 511)), ("scoreset_best<4,u32>", (512,))]
    assert [la.site for la in SM.predict_chunk("ss", [(40, (600,))], C1, {"px": 0})] == ["scoreset<2,u16>"]
    assert SM.strips_of(one("score", (1023, 1024, 2047, 2048, 3071, 3072))[0]) == {1, 2, 3, 4}
    assert one("ckpt", (255, 511), planes=32)[0].strip == 512 and SM.strips_of(one("ckpt", (255, 2047), planes=32)[0]) == {1, 2}


def test_case_table_reaches_every_instantiation():
    """CASES, walked through the restatement: every instantiation of REQUIRED; two, three and four strips of <2,u16> and <4,u32> in
    every family that has them; a query of 0, 1 and 3 symbols in a chunk of every class wider than 64 columns that launch_by_pitch picks (a score set classes
    each pair by its own pitch, so there only the Q1 classes hold them); the result column at
    every position of the first strip of every sweep and checkpoint class."""
    assert len({c.name for c in CASES}) == len(CASES)
    sites, strips, short, cols = set(), {}, {}, {}
    for c in CASES:
        las = _launches(c)
        chunk = {L for _, ls in c.groups for L in ls}
        for la in las:
            sites.add(la.site)
            strips.setdefault(la.site, set()).update(SM.strips_of(la))
            # (a score set classes every pair by its own pitch: its short pairs run in the Q1 class, never inside a wide kernel)
            if la.strip > 64 and set(SHORT) <= (set(la.lengths) if c.path.startswith("ss") else chunk):
                short[la.site] = True
            cols.setdefault(la.site, set()).update(L for L in la.lengths)
    assert REQUIRED <= sites, sorted(REQUIRED - sites)
    for site in sorted(REQUIRED):
        if site.startswith("scoreset"):
            assert bool(short.get(site)) == ("<1," in site), site
        else:
            assert short.get(site), (site, "no chunk with queries of 0, 1 and 3 symbols")
    for fam in ("poa_sweep_kernel<%s>", "poa_ckpt<%s>"):
        for cls, width in (("2,u16", 1024), ("4,u32", 1024), ("1,u16", 512), ("1,u32", 256), ("2,u32", 512)):
            assert {2, 3, 4} <= strips[fam % cls] or width < 1024, (fam % cls, strips[fam % cls])
            assert set(range(width)) <= cols[fam % cls], (fam % cls, "the result column at every position of a strip")
    assert set(range(512, 1024)) <= cols["poa_sweep_px_kernel"]
    for site in ("poa_ckpt_multi<2,u16>", "poa_ckpt_multi<4,u32>", "poa2_ckpt_multi<u16,2>", "poa2_ckpt_multi<u32,4>", "poa2_ckpt<u16,2>", "poa2_ckpt<u32,4>"):
        # L = 2048, L = 3072: the first column of the third and of the fourth strip
        assert {2, 3, 4} <= strips[site] and {2047, 2048, 3071, 3072} <= cols[site], (site, strips[site])
    for form in ("scoreset", "scoreset_capped", "scoreset_best"):
        assert {2, 3, 4} <= strips[form + "<2,u16>"] and {2, 3, 4} <= strips[form + "<4,u32>"], form
        assert set(range(512, 1024)) <= cols[form + "<PX>"] and set(range(512)) <= cols[form + "<1,u16>"]
    # the top half of u16: every batch at e* is u16, every batch at e* + 1 is u32, in each of the three classes
    top = {}
    for c in CASES:
        if "-top-" in c.name:
            for la in _launches(c):
                top.setdefault(la.cells, set()).add(la.site)
    assert {"poa_sweep_px_kernel", "poa_sweep_kernel<1,u16>", "poa_sweep_kernel<2,u16>", "poa_ckpt<1,u16>", "poa_ckpt<2,u16>",
            "scoreset<PX>", "scoreset_capped<PX>", "poa_ckpt_multi<2,u16>"} <= top["u16"]
    assert {"poa_sweep_kernel<4,u32>", "poa_ckpt<4,u32>", "poa_ckpt_multi<4,u32>"} <= top["u32"]


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
def _costs_obj(engine, costs, wide=False):
    if len(costs) == 3:
        return engine.GapAffine(costs[0], costs[2], costs[1])      # the reference's order: (mismatch, extend, open)
    c = engine.GapAffine2Piece(*costs)
    if wide:
        class Wide(engine.GapAffine2Piece):      # poa_costs2_t.wide_planes = 1
            def _c(self):
                k = engine.GapAffine2Piece._c(self)
                k.wide_planes = 1
                return k
        c = Wide(*costs)
    return c


_ORACLE = {}


def _oracle_batch(oracle, kind, queries_key, qs, costs):
    """dense_batch of a query list on one graph, once per (graph, query list, costs); two-piece costs run under oracle.two_piece"""
    key = (kind, queries_key, costs)
    if key not in _ORACLE:
        og = oracle.OracleGraph.from_csr(_graph(kind).as_dict())
        qseq, qoff = pack_queries(qs)
        if len(costs) == 3:
            D = og.dense_batch(qseq, qoff, oracle.Costs(*costs), threads=16)
        else:
            m, e1, o1, e2, o2 = costs
            with oracle.two_piece(o2, e2):
                D = og.dense_batch(qseq, qoff, oracle.Costs(m, o1, e1), threads=16)
        for a in D.values():
            a.setflags(write=False)
        _ORACLE[key] = D
    return _ORACLE[key]


def _ladder_lengths(kind):
    return tuple(sorted(set(LADDER) | set(EDGES) | (set(WIN23) if kind == "small" else set())))


def _ladder(oracle, kind, costs):
    """-> (D, row_of): the oracle's dense_batch over every prefix length any case uses on this graph, and length -> row of D.
    One-piece costs: asserts first, from the oracle's own M plane of the whole read, that the end row holds these prefix scores
    and that they are no ladder of equal values."""
    lengths = _ladder_lengths(kind)
    D = _oracle_batch(oracle, kind, "ladder", _prefixes(kind, lengths), costs)
    row_of = {L: i for i, L in enumerate(lengths)}
    key = ("identity", kind, costs)
    if key not in _ORACLE:
        og = oracle.OracleGraph.from_csr(_graph(kind).as_dict())
        full = _read(kind)[:max(lengths)]
        if len(costs) == 3:
            od = og.dense_align(full, oracle.Costs(*costs), planes=True)
        else:
            m, e1, o1, e2, o2 = costs
            with oracle.two_piece(o2, e2):
                od = og.dense_align(full, oracle.Costs(m, o1, e1), planes=True)
        end = od["M"][og.export_csr()["rank"][_graph(kind).end]]
        if kind == "small":
            assert np.array_equal(end[np.array(lengths)], D["score"]), (kind, costs, "M[end][c] is not the score of the prefix q[:c]")
        else:
            # The recurrence opens a gap at column c only where the read's NEXT symbol q[c] allows it (open_d / open_i of
            # oracle/dense.hpp, ROW_OPENI_* of the kernels), which leaves M[end][len] exact and may leave M[end][c], c < len,
            # above the score of the prefix.  On the chain graph it does: the whole read's end row bounds the prefix scores from
            # above and is no copy of them.  The prefixes themselves are what runs and what is compared either way.
            assert (end[np.array(lengths)] >= D["score"]).all() and end[lengths[-1]] == D["score"][-1], (kind, costs)
        # (two-piece costs run the window edges only, and with extend2 = 0 a long gap has one price whatever its length)
        assert len(np.unique(D["score"][:len(LADDER)])) >= (300 if len(costs) == 3 else 3), (kind, costs, "a ladder of equal scores")
        _ORACLE[key] = True
    return D, row_of


def _assert_equals_oracle(res, D, idx, tag, pairs=True):
    """score, flags and (pairs) every (rpos, qpos) of the queries D[idx], in that order, bit for bit"""
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    assert np.array_equal(res.score, D["score"][idx]), (tag, "score", [(int(i), int(res.score[i]), int(D["score"][idx[i]])) for i in np.flatnonzero(res.score != D["score"][idx])[:6]])
    want_flags = D["flags"][idx] if pairs else D["flags"][idx] & SHORT_QUERY
    assert np.array_equal(res.flags, want_flags), (tag, "flags", np.flatnonzero(res.flags != want_flags)[:8].tolist())
    if not pairs:
        return
    npairs = D["n_pairs"][idx].astype(np.int64)
    got_n = np.diff(res.pair_off.astype(np.int64))
    assert np.array_equal(got_n, npairs), (tag, "n_pairs", np.flatnonzero(got_n != npairs)[:8].tolist())
    start = np.cumsum(npairs) - npairs
    src = np.repeat(D["pair_off"][idx].astype(np.int64) - start, npairs) + np.arange(int(npairs.sum()))
    want, got = D["pairs"][src], res.pairs[:int(npairs.sum())]
    if not np.array_equal(got, want):
        k = int(np.flatnonzero((got != want).any(axis=1))[0])
        i = int(np.searchsorted(start, k, side="right")) - 1
        pytest.fail("%s: alignment of query %d differs at pair %d: got %s, want %s" % (tag, i, k - int(start[i]), got[k].tolist(), want[k].tolist()))


def _sweep_rows_of(engine, g):
    """(n_slots, n_slotted) of a graph"""
    slot, n_slots = engine._device_graph(g).sweep_slots()
    return int(n_slots), int((np.asarray(slot) != NONE).sum())


def _stored_rows(engine, g, ckpt_rows=0, two_piece=False):
    """plane rows a checkpointed run stores per query: kept planes x (slotted + snapshot rows) + window planes x rows"""
    keep, win = (3, 5) if two_piece else (2, 3)
    n_slots, n_slotted = _sweep_rows_of(engine, g)
    boundary, rpq = engine._device_graph(g).checkpoint_plan(ckpt_rows, two_piece=two_piece)
    snap, rem = divmod(rpq - keep * n_slots - win * int(np.diff(boundary.astype(np.int64)).max()), keep)
    assert rem == 0 and snap >= 0
    return keep * (n_slotted + snap) + win * g.n


def _run_resident(engine, case, qs, plan=0):
    """one case on a resident batch of its path; -> (BatchResult, layout)"""
    (kind, _), = case.groups
    g, tune = _graph(kind), dict(case.tune)
    mode = {"score": "score", "score2": "score", "ckpt": "checkpoint", "ckpt2": "checkpoint2"}[case.path]
    if plan:
        tune["ckpt_rows"] = plan
    cfg = engine.make_config(mode, **tune)
    qseq, qoff = pack_queries(qs)
    rb = engine.ResidentBatch(g, qseq, qoff, config=cfg)
    try:
        rb.run(_costs_obj(engine, case.costs, case.wide), None, cfg)
        res = rb.fetch(want_pairs=mode != "score")
        return res, rb.layout()
    finally:
        rb.close()


def _check_resident(engine, case, qs, D, idx, plans=(0,)):
    """Run the case under every plan; the launch the restatement predicts is held against layout() and plane_bytes; results
    against D[idx]."""
    la, = _launches(case)
    (kind, lengths), = case.groups
    g = _graph(kind)
    assert [len(q) for q in qs] == list(lengths)
    for plan in plans:
        res, layout = _run_resident(engine, case, qs, plan)
        tag = (case.name, plan)
        assert res.stats["n_chunks"] == 1, tag
        assert layout == ({"u16"} if la.cells == "u16" else set()), (tag, layout)
        if case.path in ("score", "score2"):
            assert res.stats["plane_bytes"] == SM.sweep_plane_bytes([(la, _sweep_rows_of(engine, g)[1])]), (tag, "px" if la.px else "general")
        else:
            assert res.stats["plane_bytes"] == SM.ckpt_plane_bytes(la.cells, _stored_rows(engine, g, plan, case.path == "ckpt2"), lengths), tag
        _assert_equals_oracle(res, D, idx, tag, pairs=case.path in ("ckpt", "ckpt2"))


# ---- GPU: the prefix ladder -------------------------------------------------------------------------------------------------------
LADDER_PARAMS = [(kind, costs) for kind, cs in LADDER_COSTS.items() for costs in cs]
LADDER_IDS = ["%s-%s" % (k, "_".join(map(str, c))) for k, c in LADDER_PARAMS]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,costs", LADDER_PARAMS, ids=LADDER_IDS)
def test_ladder_score_mode(engine, oracle, kind, costs):
    """Score mode: every prefix of the read, batch by kernel class (<1,u16>, the packed kernel, <2,u16> at one strip and at two to
    four, <1|2|4,u32>); the px batch meets the pitch_sum condition by the restatement, which plane_bytes confirms."""
    D, row_of = _ladder(oracle, kind, costs)
    ran = set()
    for case in _select("score", "ladder-" + kind, costs=costs):
        lengths = case.groups[0][1]
        _check_resident(engine, case, _prefixes(kind, lengths), D, [row_of[L] for L in lengths])
        ran.add(_launches(case)[0].site)
    assert ran == {"poa_sweep_px_kernel"} | {"poa_sweep_kernel<%d,%s>" % qc for qc in FIVE}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,costs", LADDER_PARAMS, ids=LADDER_IDS)
def test_ladder_checkpointed(engine, oracle, kind, costs):
    """Checkpointed mode under the default plan and segments of 7 rows: score, flags and the full pair list of every prefix."""
    D, row_of = _ladder(oracle, kind, costs)
    ran = set()
    for case in _select("ckpt", "ladder-" + kind, costs=costs):
        lengths = case.groups[0][1]
        _check_resident(engine, case, _prefixes(kind, lengths), D, [row_of[L] for L in lengths], plans=(0, 7))
        ran.add(_launches(case)[0].site)
    assert ran == {"poa_ckpt<%d,%s>" % qc for qc in FIVE}


def _set_input(case):
    """graphs, the pool of queries and the (query, graph) pairs of a score-set case: one pair per prefix of each graph's own read;
    every third pair of the first graph is listed a second time at the end (a query with two candidates of equal score)"""
    graphs = [_graph(k) for k, _ in case.groups]
    seqs, pairs = [], []
    for gi, (kind, lengths) in enumerate(case.groups):
        for q in _prefixes(kind, lengths):
            pairs.append((len(seqs), gi))
            seqs.append(q)
    n_first = len(case.groups[0][1])
    pairs += [pairs[i] for i in range(0, n_first, 3)]
    return graphs, seqs, pairs


def _set_plane_bytes(engine, case, graphs, seqs, pairs):
    cells = _launches(case)[0].cells
    px = dict(case.tune).get("px", 1) != 0
    total = 0
    for qi, gi in pairs:
        cls = SM.scoreset_class(cells, px, SM.pitch_of(len(seqs[qi])))
        total += 2 * _sweep_rows_of(engine, graphs[gi])[1] * (2048 if cls == "PX" else SM.pitch_of(len(seqs[qi])) * (2 if cells == "u16" else 4))
    return total


def _set_expected(oracle, case, pairs, ladder):
    """the oracle's score of every pair of _set_input(case); ladder(kind) -> (D, row_of)"""
    per_graph = []
    for kind, lengths in case.groups:
        D, row_of = ladder(kind)
        per_graph.append(D["score"][[row_of[L] for L in lengths]])
    own = np.concatenate(per_graph)
    return own[[qi for qi, _ in pairs]]      # (query index == position among the own pairs)


@pytest.mark.gpu
@pytest.mark.parametrize("costs", [C1, C0], ids=["4_6_2", "4_0_2"])
def test_ladder_score_sets(engine, oracle, costs):
    """Both ladders in one set, so that the classes mix in a chunk: the plain form; capped at the score (every pair returns it,
    none is CAPPED) and one below it (every pair with a score above 0 is CAPPED and unvisited); the best-of form field by field."""
    from test_scoreset_best import _check as check_best
    for tune in ({}, U32, {"px": 0}):
        plain, = _select("ss", "ladder", costs=costs, tune=tuple(sorted(tune.items())))
        graphs, seqs, pairs = _set_input(plain)
        want = _set_expected(oracle, plain, pairs, lambda kind: _ladder(oracle, kind, costs))
        flags0 = np.array([SHORT_QUERY if len(seqs[qi]) == 1 else 0 for qi, _ in pairs], np.uint32)
        assert (want > 0).sum() > len(pairs) // 2 and int(want.max()) < NONE
        sites = {la.site for la in _launches(plain)}
        assert sites == ({"scoreset<1,u32>", "scoreset<2,u32>", "scoreset<4,u32>"} if tune == U32 else
                         {"scoreset<1,u16>", "scoreset<2,u16>"} | ({"scoreset<PX>"} if not tune else set())), sites
        cfg = engine.make_config("score", **tune)
        ss = engine.ScoreSet(graphs, seqs, pairs=pairs)
        try:
            ss.run(_costs_obj(engine, costs), config=cfg)
            score, flags, st = ss.fetch()
            assert st["n_chunks"] == 1 and st["plane_bytes"] == _set_plane_bytes(engine, plain, graphs, seqs, pairs), (tune, "plane_bytes")
            assert np.array_equal(score, want) and np.array_equal(flags, flags0), (tune, "plain", np.flatnonzero(score != want)[:8].tolist())
            ss.run(_costs_obj(engine, costs), config=cfg, cap=want)
            score, flags, _ = ss.fetch()
            assert np.array_equal(score, want) and np.array_equal(flags, flags0), (tune, "cap = score", np.flatnonzero(score != want)[:8].tolist())
            cap = np.where(want > 0, want - 1, NONE).astype(np.uint32)
            ss.run(_costs_obj(engine, costs), config=cfg, cap=cap)
            score, flags, _ = ss.fetch()
            below = want > 0
            assert (score[below] == NONE).all() and (flags[below] == (flags0[below] | CAPPED)).all(), (tune, "cap = score - 1", np.flatnonzero(below & (score != NONE))[:8].tolist())
            assert np.array_equal(score[~below], want[~below]) and np.array_equal(flags[~below], flags0[~below])
            pq = np.array([qi for qi, _ in pairs], np.int64)
            for slack, limit in ((0, None), (2, None), (0, np.where(np.arange(len(seqs)) % 2, want[:len(seqs)], NONE).astype(np.uint32))):
                ss.run(_costs_obj(engine, costs), config=cfg, best=True, slack=slack, limit=limit)
                check_best(ss, want, pq, len(seqs), slack, limit, flags0, (tune, "best", slack, limit is not None))
        finally:
            ss.close()


# ---- GPU: two-piece at the window edges -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("costs", [T1, T0], ids=["e2_1", "e2_0"])
def test_two_piece_window_edges(engine, oracle, costs):
    """Two-piece score mode, POA_MODE_CHECKPOINT2 (plans default and 7) and the two-piece score set, u16 and u32 cells, with the
    result column around 256, 512, 1024 and 2048 (on the 162-row graph 3072 too: four strips) and queries of 0, 1 and 3 symbols,
    against the oracle's two-piece restatement."""
    for kind in ("small", "chain"):
        D, row_of = _ladder(oracle, kind, costs)
        for path, plans in (("score2", (0,)), ("ckpt2", (0, 7))):
            for case in _select(path, "edges-" + kind, costs=costs):
                (_, lengths), = case.groups
                _check_resident(engine, case, _prefixes(kind, lengths), D, [row_of[L] for L in lengths], plans=plans)
    for case in _select("ss2", "edges", costs=costs):
        graphs, seqs, pairs = _set_input(case)
        want = _set_expected(oracle, case, pairs, lambda kind: _ladder(oracle, kind, costs))
        ss = engine.ScoreSet(graphs, seqs, pairs=pairs)
        try:
            ss.run(_costs_obj(engine, costs), config=engine.make_config("score", **dict(case.tune)))
            score, flags, st = ss.fetch()
        finally:
            ss.close()
        assert st["plane_bytes"] == _set_plane_bytes(engine, case, graphs, seqs, pairs), case.name
        assert np.array_equal(score, want), (case.name, np.flatnonzero(score != want)[:8].tolist())
        assert np.array_equal(flags, np.array([SHORT_QUERY if len(seqs[qi]) == 1 else 0 for qi, _ in pairs], np.uint32)), case.name


# ---- GPU: multi-graph batches -----------------------------------------------------------------------------------------------------
def _run_multi(engine, case, seqs_per_graph, plan=0):
    graphs = [_graph(k) for k, _ in case.groups]
    two = case.path == "multi2"
    tune = dict(case.tune)
    if plan:
        tune["ckpt_rows"] = plan
    cfg = engine.make_config("checkpoint2" if two else "checkpoint", **tune)
    mb = engine.MultiGraphBatch(graphs, seqs_per_graph, config=cfg, two_piece=two)
    try:
        mb.run(_costs_obj(engine, case.costs, case.wide), None, cfg)
        return mb.fetch()
    finally:
        mb.close()


def _check_multi(engine, case, seqs_per_graph, expected, plans=(0,)):
    """expected: per graph (D, idx).  The cell width the restatement predicts is held against plane_bytes; every graph's queries
    against its own oracle batch."""
    la, = _launches(case)
    two = case.path == "multi2"
    for plan in plans:
        res = _run_multi(engine, case, seqs_per_graph, plan)
        tag = (case.name, plan)
        assert res.stats["n_chunks"] == 1, tag
        want_bytes = sum(SM.ckpt_plane_bytes(la.cells, _stored_rows(engine, _graph(k), plan, two), ls) for k, ls in case.groups)
        assert res.stats["plane_bytes"] == want_bytes, (tag, la.cells)
        first = 0
        for (kind, lengths), (D, idx) in zip(case.groups, expected):
            n = len(lengths)
            lo, hi = int(res.pair_off[first]), int(res.pair_off[first + n])
            part = engine.BatchResult(res.score[first:first + n], res.pairs[lo:hi], res.pair_off[first:first + n + 1] - res.pair_off[first],
                                      res.flags[first:first + n], res.stats)
            _assert_equals_oracle(part, D, idx, tag + (kind,))
            first += n


@pytest.mark.gpu
@pytest.mark.parametrize("path,costs", [("multi", C1), ("multi", C0), ("multi2", T1), ("multi2", T0)], ids=["4_6_2", "4_0_2", "2piece-e2_1", "2piece-e2_0"])
def test_multi_graph_window_edges(engine, oracle, path, costs):
    """Both ladder graphs and a 5-row graph in one batch, the window edges per graph, batch by kernel class (all five), one-piece
    and two-piece: every graph's results against the oracle on that graph."""
    ran = set()
    for case in _select(path, "edges", costs=costs):
        seqs, expected = [], []
        for kind, lengths in case.groups:
            qs = _prefixes(kind, lengths)
            if kind == "five":
                D = _oracle_batch(oracle, kind, "edges", _prefixes(kind, EDGES + EDGES_Q1 + EDGES_W1), costs)
                row_of = {L: i for i, L in enumerate(EDGES + EDGES_Q1 + EDGES_W1)}
            else:
                D, row_of = _ladder(oracle, kind, costs)
            seqs.append(qs)
            expected.append((D, [row_of[L] for L in lengths]))
        _check_multi(engine, case, seqs, expected, plans=(0, 7) if "-all-" in case.name else (0,))
        ran.add(_launches(case)[0].site)
    assert ran == ({"poa_ckpt_multi<%d,%s>" % qc for qc in FIVE} if path == "multi" else {"poa2_ckpt_multi<%s,%d>" % (c, q) for q, c in FIVE})


# ---- GPU: the top half of u16 -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _top_reads(L0):
    """0, 1 and 3 foreign symbols; L0 foreign symbols; a walk through the graph followed by foreign symbols up to L0; foreign
    symbols followed by the walk; L0 - 1 foreign symbols; and the walk with k0 foreign symbols behind its fifth base (the rest
    behind its last), k0 such that at e* the insertion run ends just below 0x8000 in a cell whose other candidate, the mismatch,
    lies above it — and the next base is a match, so the optimal path reads that cell's minimum back.  (Five long reads to three
    short ones: a batch whose longest read is one strip wide meets the packed kernel's pitch_sum condition.)"""
    poa = _poa("small")
    walk = poa.walk(np.random.Generator(np.random.PCG64(77)))
    assert 5 < len(walk) < L0 // 2 and FOREIGN not in set(_graph("small").symbol.tolist())
    foreign = np.full(L0, FOREIGN, np.uint8)
    pad = foreign[:L0 - len(walk)]
    k0 = top_straddle(L0)
    assert 0 < k0 < len(pad)
    straddle = np.concatenate([walk[:5], pad[:k0], walk[5:], pad[k0:]])
    return (foreign[:0], foreign[:1], foreign[:3], foreign, np.concatenate([walk, pad]), np.concatenate([pad, walk]), foreign[:L0 - 1], straddle)


def top_straddle(L0):
    """the longest insertion run that costs less than 0x8000 at e*"""
    return (0x8000 - 1 - 6) // top_extend(L0, _mpn("small"))


def _top(oracle, L0, de):
    """-> (costs, reads, D), after the conditions on the input: at e* the all-foreign read scores the u16 bound itself, above
    0xF000, the walk-then-foreign and foreign-then-walk reads score above 0x8000, and the oracle aligns the straddling read as
    five bases, k0 insertions that end just below 0x8000, and a match"""
    mpn = _mpn("small")
    e = top_extend(L0, mpn)
    assert 255 >= 2 * e and SM.score_bound(6, e, L0, mpn) <= SM.U16_BOUND < SM.score_bound(6, e + 1, L0, mpn)
    costs = (255, 6, e + de)
    reads = _top_reads(L0)
    D = _oracle_batch(oracle, "small", "top-%d" % L0, list(reads), costs)
    assert int(D["score"][3]) == 2 * 6 + (e + de) * (L0 + mpn)
    assert int(D["score"][4]) > 0x8000 and int(D["score"][5]) > 0x8000
    assert [len(q) for q in reads] == list(SHORT + (L0, L0, L0, L0 - 1, L0))
    # the straddling read: five aligned bases, the run of exactly k0 insertions, then a match; two insertion runs in all
    k0, runs = top_straddle(L0), _gap_runs(oracle.batch_alignment(D, 7))
    assert [(k, len(x)) for k, x in runs[:2]] == [("M", 5), ("I", k0)] and runs[1][1] == list(range(5, 5 + k0)), [(k, len(x)) for k, x in runs]
    node, qpos = runs[2][1][0]
    assert runs[2][0] == "M" and qpos == 5 + k0 and _graph("small").symbol[node] == reads[7][qpos]
    assert int(D["score"][7]) == 2 * 6 + (e + de) * (L0 - mpn)
    if de == 0:
        assert 0xF000 < int(D["score"][3]) <= SM.U16_BOUND
        # at e* the run ends below 0x8000 in a cell whose other candidates — the mismatch of the run's last symbol from the rows
        # before, and the deletion — lie at or above it: from the oracle's own planes of that read
        g = _graph("small")
        og = oracle.OracleGraph.from_csr(g.as_dict())
        od, rank = og.dense_align(reads[7], oracle.Costs(*costs), planes=True), og.export_csr()["rank"]
        last = runs[0][1][-1][0]      # the node the fifth base sits on: the run's row
        r, c = int(rank[last]), 5 + k0
        diag = min(int(od["M"][int(rank[p])][c - 1]) for p in g.predecessors(last).tolist()) + 255
        assert int(od["I"][r][c]) == int(od["M"][r][c]) == 6 + e * k0 < 0x8000 <= min(diag, int(od["D"][r][c])), (L0, int(od["I"][r][c]), diag, int(od["D"][r][c]))
    return costs, reads, D


@pytest.mark.gpu
@pytest.mark.parametrize("L0", TOP_L0)
@pytest.mark.parametrize("de", [0, 1], ids=["e_star", "e_star_plus_1"])
def test_top_half_of_u16(engine, oracle, L0, de):
    """Scores between 0x8000 and the u16 bound through score mode (packed and general kernel), checkpointed mode (plans default
    and 7, pairs and flags), a score set (plain, capped at the score and one below) and a multi-graph batch; u16 cells at e*, u32
    cells at e* + 1, asserted for every run."""
    costs, reads, D = _top(oracle, L0, de)
    idx = list(range(len(reads)))
    cells = "u32" if de else "u16"
    for path in ("score", "ckpt"):
        for case in _select(path, "top-%d" % L0, costs=costs):
            assert _launches(case)[0].cells == cells
            _check_resident(engine, case, list(reads), D, idx, plans=(0, 7) if path == "ckpt" else (0,))
    plain, = _select("ss", "top-%d" % L0, costs=costs)
    assert {la.cells for la in _launches(plain)} == {cells}
    graphs, seqs, pairs = [_graph("small")], list(reads), [(i, 0) for i in idx]
    want = np.array(D["score"])
    flags0 = np.array([SHORT_QUERY if len(q) == 1 else 0 for q in reads], np.uint32)
    ss = engine.ScoreSet(graphs, seqs, pairs=pairs)
    try:
        for cap in (None, want, np.where(want > 0, want - 1, NONE).astype(np.uint32)):
            ss.run(_costs_obj(engine, costs), cap=cap)
            score, flags, st = ss.fetch()
            assert st["plane_bytes"] == _set_plane_bytes(engine, plain, graphs, seqs, pairs), (L0, de, "plane_bytes")
            if cap is None or cap is want:
                assert np.array_equal(score, want) and np.array_equal(flags, flags0), (L0, de, cap is not None, score.tolist(), want.tolist())
            else:
                below = want > 0
                assert (score[below] == NONE).all() and (flags[below] == (flags0[below] | CAPPED)).all(), (L0, de, score.tolist())
                assert np.array_equal(score[~below], want[~below])
    finally:
        ss.close()
    multi, = _select("multi", "top-%d" % L0, costs=costs)
    assert _launches(multi)[0].cells == cells
    D5 = _oracle_batch(oracle, "five", "top-%d" % L0, list(reads), costs)
    _check_multi(engine, multi, [list(reads), list(reads)], [(D, idx), (D5, idx)])


# ---- GPU: walks that cross strip and segment boundaries ---------------------------------------------------------------------------
# Plants on the clean walk through the 1 382-row graph, by row of the walk's nodes.  The rows were chosen so that the oracle keeps
# every planted run in one piece under (4, 6, 2), (4, 0, 2) and 4 / 6,24 / 2,1 alike (with gap-open 0 a deletion run may be split
# or shifted at no cost wherever a neighbouring base repeats); each test asserts that it did before it looks at a GPU result.
PLAN7_BOUNDARY = 252              # a boundary of the 7-row plan: rows 246..258 are dropped
DEFAULT_BOUNDARY = {False: 672, True: 651}      # ... of the default plan, one-piece (32-row segments) / two-piece (31): b - 6 .. b + 6
LONG_DELETION = (1008, 1037)      # 30 consecutive rows: whole 7-row segments without an aligned base
DIAG_TRIM = {False: 55, True: 20}     # bases trimmed off the head: the pair at qpos 1023 lands on a segment's first row
INS_DEL = (55, 5, 8)              # trim, inserted symbols at qpos 1023.., walk nodes dropped behind them (rows 1120..1127)


@functools.lru_cache(maxsize=None)
def _walk_read():
    w = np.ascontiguousarray(_poa("walk").queries(1, length=0, p_sub=0.0, p_ins=0.0, p_del=0.0)[0], np.uint8)
    w.setflags(write=False)
    return w


def _walk_rows(engine, oracle):
    """-> (rows by node, rows of the walk's nodes by position in the clean walk), the latter from the oracle's alignment of it"""
    key = ("walk-rows",)
    if key not in _ORACLE:
        rows = engine._device_graph(_graph("walk")).node_rows().astype(np.int64)
        D = _oracle_batch(oracle, "walk", "clean", [_walk_read()], C1)
        al = oracle.batch_alignment(D, 0)
        assert [q for _, q in al] == list(range(len(_walk_read()))) and int(D["score"][0]) <= 4       # every base on a node of its own
        _ORACLE[key] = (rows, rows[np.array([r for r, _ in al])])
    return _ORACLE[key]


def _cross_reads(engine, oracle, two_piece):
    """name -> read"""
    w = _walk_read()
    _, wr = _walk_rows(engine, oracle)
    n = lambda k: np.full(k, FOREIGN, np.uint8)
    keep = np.ones(len(w), bool)
    b = DEFAULT_BOUNDARY[two_piece]
    for lo, hi in ((PLAN7_BOUNDARY - 6, PLAN7_BOUNDARY + 6), (b - 6, b + 6), LONG_DELETION):
        keep &= ~((wr >= lo) & (wr <= hi))
    t, (te, m, k) = DIAG_TRIM[two_piece], INS_DEL
    return {
        "short": w[:3],
        "ins1024": np.concatenate([w[:1019], n(11), w[1019:]]),                          # columns 1020..1030
        "ins2048": np.concatenate([w[:600], n(760), w[600:1283], n(9), w[1283:]]),       # columns 601..1360 and 2044..2052
        "del": w[keep],
        "diag": w[t:],
        "ins_del": np.concatenate([w[te:te + 1023], n(m), w[te + 1023 + k:]]),
    }


def _gap_runs(al):
    """maximal runs of an alignment: [("I", [qpos...]) | ("D", [node...]) | ("M", [(node, qpos)...])] in alignment order"""
    out = []
    for r, q in al:
        kind, item = ("I", q) if r == NONE else (("D", r) if q == NONE else ("M", (r, q)))
        if out and out[-1][0] == kind:
            out[-1][1].append(item)
        else:
            out.append((kind, [item]))
    return out


def _assert_crossings(engine, oracle, reads, als, two_piece, adjacent_runs):
    """The conditions on the input, from the oracle's pair lists alone.  als: name -> [(rpos, qpos)]."""
    g = _graph("walk")
    rows, _ = _walk_rows(engine, oracle)
    dg = engine._device_graph(g)
    b7 = set(dg.checkpoint_plan(7, two_piece=two_piece)[0].tolist())
    bdef = set(dg.checkpoint_plan(0, two_piece=two_piece)[0].tolist())
    assert PLAN7_BOUNDARY in b7 and DEFAULT_BOUNDARY[two_piece] in bdef and len(bdef) > 8
    ins = lambda name: [set(x) for k, x in _gap_runs(als[name]) if k == "I"]
    dels = lambda name: [rows[np.array(x)] for k, x in _gap_runs(als[name]) if k == "D"]
    # an insertion run over columns 1020..1030 (column = qpos + 1): the walk steps left across the strip boundary inside a run
    assert any(set(range(1019, 1030)) <= s for s in ins("ins1024")), "ins1024"
    # ... over columns 2044..2052, the first columns of the third strip, and a long one across column 1024
    assert any(set(range(2043, 2052)) <= s for s in ins("ins2048")) and any(set(range(700, 1300)) <= s for s in ins("ins2048")), "ins2048"
    # deletion runs over the rows b - 6 .. b + 6 of a 7-row and of a default boundary; 30 rows in one run
    for b in (PLAN7_BOUNDARY, DEFAULT_BOUNDARY[two_piece]):
        assert any(d.min() <= b - 6 and d.max() >= b + 6 for d in dels("del")), ("del", b)
    lo, hi = LONG_DELETION
    assert any(d.min() <= lo and d.max() >= hi for d in dels("del")), "del 30 rows"
    whole = [s for s in sorted(b7) if lo <= s and s + 7 <= hi + 1]
    assert len(whole) >= 3      # segments of the 7-row plan the walk passes without aligning a base
    # a diagonal step across a strip and a segment boundary at once
    at = {q: r for r, q in als["diag"] if q != NONE}
    n1, n0 = at[1023], at[1022]
    assert n1 != NONE and n0 != NONE and reads["diag"][1023] == g.symbol[n1] and reads["diag"][1022] == g.symbol[n0]
    assert int(rows[n1]) in b7 and int(rows[n1]) in bdef and rows[n0] == rows[n1] - 1, ("diag", int(rows[n0]), int(rows[n1]))
    # opposite gap runs side by side at (a segment's first row, column 1024).  Under one-piece costs no optimum has them: one step
    # of each run exchanged for a mismatch costs 2 * extend = mismatch the same and saves an open where a run ends, and with
    # open 0 the oracle's walk takes the mismatches.  Under the two-piece costs it does: the insertion run, then the deletion run.
    # Either way the plant is asserted for what the oracle makes of it, not only for what it does not.
    runs = _gap_runs(als["ins_del"])
    side_by_side = [(a, b) for a, b in zip(runs, runs[1:]) if a[0] == "I" and b[0] == "D" and a[1][0] == 1023]
    assert bool(side_by_side) == adjacent_runs, ("ins_del", [(k, len(x)) for k, x in runs])
    _, m, k = INS_DEL
    if adjacent_runs:
        (_, iq), (_, dn) = side_by_side[0]
        assert iq == list(range(1023, 1023 + m)) and len(dn) == k and int(rows[dn[0]]) in b7, ("ins_del", iq, rows[np.array(dn)].tolist())
    else:
        # what the one-piece optimum is instead: the k - m surplus nodes deleted in one run that starts on a segment's first row,
        # in the last column of the first strip, and directly behind it the m foreign symbols as mismatches from column 1024 on
        i = next(j for j, (kind, x) in enumerate(runs) if kind == "D" and int(rows[x[0]]) in b7 and len(x) == k - m)
        assert runs[i - 1][0] == "M" and runs[i - 1][1][-1][1] == 1022 and runs[i + 1][0] == "M", ("ins_del", [(kind, len(x)) for kind, x in runs])
        assert [q for _, q in runs[i + 1][1][:m]] == list(range(1023, 1023 + m)) and all(reads["ins_del"][q] == FOREIGN for q in range(1023, 1023 + m))
        assert [int(rows[n]) for n, _ in runs[i + 1][1][:m]] == [int(rows[runs[i][1][-1]]) + 1 + j for j in range(m)]


def _walk_case(oracle, engine, costs):
    two = len(costs) == 5
    reads = _cross_reads(engine, oracle, two)
    names = list(reads)
    D = _oracle_batch(oracle, "walk", "cross-%d" % two, [reads[k] for k in names], costs)
    als = {k: oracle.batch_alignment(D, i) for i, k in enumerate(names)}
    _assert_crossings(engine, oracle, reads, als, two, adjacent_runs=two)
    return names, reads, D


@pytest.mark.gpu
@pytest.mark.parametrize("costs", [C1, C0, T1], ids=["4_6_2", "4_0_2", "2piece"])
def test_walks_cross_strip_and_segment_boundaries(engine, oracle, costs):
    """POA_MODE_CHECKPOINT / POA_MODE_CHECKPOINT2 under segments of 1 row, of 7 rows, the default plan and one segment, u16 and u32
    cells: score, flags and pairs of the planted reads against the oracle."""
    names, reads, D = _walk_case(oracle, engine, costs)
    qs = [reads[k] for k in names]
    two = len(costs) == 5
    ran = set()
    for case in _select("ckpt2" if two else "ckpt", "cross", costs=costs):
        ran.add(_launches(case)[0].site)
        _check_resident(engine, case, qs, D, list(range(len(qs))), plans=(1, 7, 0, _graph("walk").n))      # (asserts the reads' lengths are the table's)
    assert ran == ({"poa2_ckpt<u16,2>", "poa2_ckpt<u32,4>"} if two else {"poa_ckpt<2,u16>", "poa_ckpt<4,u32>"})


@pytest.mark.gpu
@pytest.mark.parametrize("costs", [C1, C0, T1], ids=["4_6_2", "4_0_2", "2piece"])
def test_walks_cross_boundaries_in_a_multi_graph_batch(engine, oracle, costs):
    """The same reads next to the 162-row graph's, so that the tables differ from wave to wave: poa_multi_* / poa_multi_*_2piece."""
    names, reads, D = _walk_case(oracle, engine, costs)
    qs = [reads[k] for k in names]
    Ds, row_of = _ladder(oracle, "small", costs)
    two = len(costs) == 5
    ran = set()
    for case in _select("multi2" if two else "multi", "cross", costs=costs):
        assert case.groups == (("small", WALK_SIDE), ("walk", tuple(len(q) for q in qs)))
        ran.add(_launches(case)[0].site)      # (the cell width of it is what plane_bytes can confirm; the chunk's widest pitch gives Q)
        _check_multi(engine, case, [_prefixes("small", WALK_SIDE), qs], [(Ds, [row_of[L] for L in WALK_SIDE]), (D, list(range(len(qs))))], plans=(7, 0))
    assert ran == ({"poa2_ckpt_multi<u16,2>", "poa2_ckpt_multi<u32,4>"} if two else {"poa_ckpt_multi<2,u16>", "poa_ckpt_multi<4,u32>"})
