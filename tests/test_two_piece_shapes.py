"""Two-piece dense pass (poasta_amd/csrc/poa_twopiece.hpp; the one-shot call is a resident batch's poa_batch_run_2piece in
poa_engine.hip) at the shapes that decide which
of its code paths run: both cell widths (u16: 8 columns per lane, 512 per pass, previous row in registers for up to 2
passes; u32: 4 per lane, 256 per pass, up to 4 passes), rows of exactly one pass / one pass and a column, rows exactly at
and just past the 1024-column register limit, rows of several passes read back from the planes, empty and one-base
queries beside a long query (each at its own pitch), chain rows, rows with several predecessors and chain rows behind such rows.

CPU: the host's selection rule restated in plain Python (`predict`) and a case table (`CASES`); a test proves that the table
reaches every path above for each width, so a trimmed table fails here rather than passing silently.
GPU: every case's scores, flags and alignments against oracle/dense.hpp (forward2 / traceback2) bit for bit, the five
planes of chosen queries cell for cell, the kernel that ran read back from the call's stats (plane_bytes) and held against
the table's prediction; scores above 65 535 on a 36 602-row graph; a batch larger than the 64 GiB plane budget (the chunk
loop with first_query > 0); POA_ERR_CAPACITY and the extend1 < extend2 refusal through the raw C ABI.

Expected plane cell under u16: the oracle's value if it is at most 65534, INF otherwise (what PlaneIO<uint16_t> stores and
reads back); nothing here requires that a finite value above 65534 occurs.

`poa_planes_2piece` takes one query; in a batch every query has its own pitch as well, so the planes it returns are laid out
as the batch's are.  The planes of a short query INSIDE a batch of long ones (first query empty beside a 2 133-base query) are
fetched in tests/test_two_piece_resident.py (poa_batch_fetch_planes_2piece); here that shape is covered by the batch-level
comparison of scores, flags and alignments."""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import pack_queries

from test_two_piece import COSTS2, _oracle_planes_by_row

INF = 0xFFFFFFFF
NP_OF = {2: 2, 4: 4}   # passes whose previous row stays in registers: poa2_forward_kernel<uint16_t, 2> / <uint32_t, 4>


# ---- the host's selection rule (poa_batch_run_2piece), in plain Python ------------------------------------------------------
def min_path_nodes(g):
    """Real nodes on the shortest start -> end path (FlatGraph::min_path_nodes)."""
    dist = {g.start: 0}
    frontier = [g.start]
    while frontier and g.end not in dist:
        nxt = []
        for v in frontier:
            for s in g.successors(v).tolist():
                if s not in dist:
                    dist[s] = dist[v] + 1
                    nxt.append(s)
        frontier = nxt
    d = dist.get(g.end, 0)
    return d - 1 if d > 0 else 0


def predict(g, lengths, costs, wide):
    """What poa_batch_run_2piece picks for a batch: ub, elem (2: u16 cells, 4: u32), K columns per lane, PW columns per pass, the
    longest query's pitch (every query has its own: (L + 64) & ~63), and per query (n_pass, keep: previous row in registers)."""
    m, e1, o1, e2, o2 = costs
    max_len, mpn = max(lengths), min_path_nodes(g)
    ub = (o1 + e1 * max_len if max_len else 0) + (o1 + e1 * mpn if mpn else 0)
    narrow = ub <= 65534 and not wide
    elem = 2 if narrow else 4
    K = 16 // elem
    PW = 64 * K
    per_query = []
    for L in lengths:
        n_pass = (L + 1 + PW - 1) // PW
        per_query.append((n_pass, n_pass <= NP_OF[elem]))
    return dict(ub=ub, elem=elem, K=K, PW=PW, pitch=(max_len + 64) & ~63, per_query=per_query)


# ---- graphs and queries: seeded generators of poasta_amd/workloads.py ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _poa(kind):
    if kind == "chain":    # 1 582 rows, nearly all of them chain rows
        return W.LinearishPOA(1500, 40, 20, seed=1)
    if kind == "multi":    # 1 602 rows, four predecessors each
        return W.LayeredPOA(n_layers=400, width=4, indeg=4, seed=5)
    if kind == "mixed":    # MSA import: runs of chain rows between SNP / indel bubbles
        return W.PangenomePOA(ref_len=1200, n_hap=8, p_snp=0.02, p_indel=0.004, max_indel=12, seed=4)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _queries(kind, lengths):
    poa = _poa(kind)
    return [poa.queries(1, length=L, first=i)[0] if L else np.zeros(0, np.uint8) for i, L in enumerate(lengths)]


def graph_profile(g, node_rows):
    """(fraction of chain rows, fraction of rows with several predecessors, chain rows that follow a non-chain row)."""
    n = g.n
    pred_rows = [None] * n
    for v in range(n):
        pred_rows[int(node_rows[v])] = [int(node_rows[p]) for p in g.predecessors(v).tolist()]
    chain = [len(p) == 1 and p[0] + 1 == r for r, p in enumerate(pred_rows)]
    several = sum(len(p) >= 2 for p in pred_rows)
    after = sum(1 for r in range(1, n) if chain[r] and not chain[r - 1])
    return sum(chain) / n, several / n, after


# ---- the case table ---------------------------------------------------------------------------------------------------------
# query lengths of every batch: the empty and the one-base query first (64 columns each beside the longest query's 2 176), then
# L + 1 in {63, 64, 65}, around the u32 pass (256), the u16 pass (512), the register limit (1024), 2 134 columns (u16: five
# passes, u32: nine, the last one partial, no registers), and fillers between them (2 048: whole passes only)
LENS = (0, 1, 62, 63, 64, 254, 255, 256, 510, 511, 512, 1022, 1023, 1024, 2133, 300, 777, 1087, 1500, 2047, 2048)
MISMATCH_255 = (255, 2, 6, 1, 24)
# ub = 2 * o1 + e1 * (2133 + 1500) on the chain graph: 65534 exactly, and 65536
UB_AT, UB_ABOVE = (4, 18, 70, 5, 90), (4, 18, 71, 5, 90)

Case = namedtuple("Case", "name kind lengths costs wide")


def _cases():
    out = []
    for wide in (False, True):
        w = "u32" if wide else "u16"
        for i, c in enumerate(COSTS2 + [MISMATCH_255]):
            out.append(Case("chain-%s-c%d" % (w, i), "chain", LENS, c, wide))
        for i in (0, 3, 4, 5):   # 3: e2 == e1, 4: e2 == 0, 5: mismatch 255
            out.append(Case("multi-%s-c%d" % (w, i), "multi", LENS, (COSTS2 + [MISMATCH_255])[i], wide))
        for i in (0, 1):
            out.append(Case("mixed-%s-c%d" % (w, i), "mixed", LENS, COSTS2[i], wide))
    # the width rule itself, no override: ub at the bound, one above it by the costs, above it by one more column
    out.append(Case("chain-ub-at", "chain", LENS, UB_AT, False))
    out.append(Case("chain-ub-above-costs", "chain", LENS, UB_ABOVE, False))
    out.append(Case("chain-ub-above-length", "chain", LENS + (2134,), UB_AT, False))
    return out


CASES = _cases()


def plane_lengths(pred, lengths):
    """Queries whose five planes are compared: the longest, and L + 1 in {64, PW, PW + 1, 1024, 1025}."""
    want = [max(lengths)] + [c - 1 for c in (64, pred["PW"], pred["PW"] + 1, 1024, 1025)]
    return [L for L in dict.fromkeys(want) if L in lengths]


def features(pred, lengths):
    """Names of the paths a batch reaches under the prediction `pred`."""
    PW, f = pred["PW"], set()
    for L, (n_pass, keep) in zip(lengths, pred["per_query"]):
        cols = L + 1
        for d, tag in ((-1, "-1"), (0, ""), (1, "+1")):
            if cols == PW + d:
                f.add("pass" + tag)
                assert (n_pass, keep) == ((1, True) if d <= 0 else (2, True))
            if cols == 1024 + d:
                f.add("reglimit" + tag)
                assert keep == (d <= 0) and n_pass == (1024 // PW if d <= 0 else 1024 // PW + 1)
            if cols == 64 + d:
                f.add("cols64" + tag)
        if not keep and n_pass >= 3 and cols % PW:
            f.add("planes-3-passes-partial")
        if L in (0, 1) and pred["pitch"] >= 1088:
            f.add("short-L%d-long-pitch" % L)
    return f


REQUIRED = {"pass-1", "pass", "pass+1", "reglimit-1", "reglimit", "reglimit+1", "planes-3-passes-partial",
            "cols64-1", "cols64", "cols64+1", "short-L0-long-pitch", "short-L1-long-pitch"}


def test_case_table_reaches_every_path():
    """Every path of REQUIRED for each cell width, on the chain-dominated graph and on the graph whose rows all have several
    predecessors; the mixed graph under both widths; every cost set of COSTS2, mismatch 255, and the width rule from both
    sides of 65534 without the override."""
    from poasta_amd import aligner
    prof = {k: graph_profile(_poa(k).graph, aligner.DeviceGraph(_poa(k).graph).node_rows()) for k in ("chain", "multi", "mixed")}
    assert prof["chain"][0] > 0.9, prof                                  # chain-dominated
    assert prof["multi"][0] < 0.01 and prof["multi"][1] > 0.99, prof     # every row (but the first layer) has several predecessors
    assert prof["mixed"][2] >= 30 and prof["mixed"][1] > 0.03 and prof["mixed"][0] > 0.5, prof   # chain rows behind non-chain rows
    reached, costs_seen, mixed_seen = {}, {2: set(), 4: set()}, set()
    for c in CASES:
        g = _poa(c.kind).graph
        p = predict(g, c.lengths, c.costs, c.wide)
        assert [len(q) for q in _queries(c.kind, c.lengths)] == list(c.lengths)
        assert c.lengths[0] == 0 and p["pitch"] >= 1088                  # the first query is empty, in a batch whose longest pitch is long
        reached.setdefault((p["elem"], c.kind), set()).update(features(p, c.lengths))
        costs_seen[p["elem"]].add(c.costs)
        if c.kind == "mixed":
            mixed_seen.add(p["elem"])
        # the planes that are compared include the longest query and one per boundary
        pl = plane_lengths(p, c.lengths)
        assert max(c.lengths) in pl and {63, p["PW"] - 1, p["PW"], 1023, 1024} <= set(pl)
        if c.wide:
            assert p["elem"] == 4 and p["ub"] <= 65534                   # the override is what widens these
    for elem in (2, 4):
        for kind in ("chain", "multi"):
            assert REQUIRED <= reached[(elem, kind)], (elem, kind, REQUIRED - reached[(elem, kind)])
        assert set(COSTS2) | {MISMATCH_255} <= costs_seen[elem]
        assert any(e2 == 0 for _, _, _, e2, _ in costs_seen[elem]) and any(e2 == e1 for _, e1, _, e2, _ in costs_seen[elem])
    assert mixed_seen == {2, 4}
    by = {c.name: predict(_poa(c.kind).graph, c.lengths, c.costs, c.wide) for c in CASES if c.name.startswith("chain-ub")}
    assert (by["chain-ub-at"]["ub"], by["chain-ub-at"]["elem"]) == (65534, 2)
    assert (by["chain-ub-above-costs"]["ub"], by["chain-ub-above-costs"]["elem"]) == (65536, 4)
    assert (by["chain-ub-above-length"]["ub"], by["chain-ub-above-length"]["elem"]) == (65534 + 18, 4)


def test_selection_rule_restated():
    """`predict` on hand-computed shapes: K, PW, passes, the register limit and the pitch."""
    g = _poa("chain").graph
    assert min_path_nodes(g) == 1500
    p = predict(g, [0, 511, 512, 1023, 1024, 2133], COSTS2[0], False)
    assert (p["elem"], p["K"], p["PW"], p["pitch"], p["ub"]) == (2, 8, 512, 2176, 6 + 2 * 2133 + 6 + 2 * 1500)
    assert p["per_query"] == [(1, True), (1, True), (2, True), (2, True), (3, False), (5, False)]
    p = predict(g, [0, 255, 256, 1023, 1024, 2133], COSTS2[0], True)
    assert (p["elem"], p["K"], p["PW"], p["pitch"]) == (4, 4, 256, 2176)
    assert p["per_query"] == [(1, True), (1, True), (2, True), (4, True), (5, False), (9, False)]
    assert [predict(g, [L], COSTS2[0], False)["pitch"] for L in (0, 63, 64, 1000, 1023, 1024)] == [64, 64, 128, 1024, 1024, 1088]


# ---- GPU --------------------------------------------------------------------------------------------------------------------
class _planes_env:
    """POA_PLANES=32 around a call (GapAffine2Piece._c() reads it: poa_costs2_t.wide_planes), restored afterwards."""

    def __init__(self, wide):
        self.wide = wide

    def __enter__(self):
        self.old = os.environ.get("POA_PLANES")
        if self.wide:
            os.environ["POA_PLANES"] = "32"
        else:
            os.environ.pop("POA_PLANES", None)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("POA_PLANES", None)
        else:
            os.environ["POA_PLANES"] = self.old
        return False


def _aligner(engine, costs):
    m, e1, o1, e2, o2 = costs
    return engine.PoastaAligner(engine.Affine2PieceDijkstra(engine.GapAffine2Piece(m, e1, o1, e2, o2)))


@functools.lru_cache(maxsize=None)
def _oracle_graph(oracle, kind):
    return oracle.OracleGraph.from_csr(_poa(kind).graph.as_dict())


def _elem_of(stats, g, lengths):
    """Bytes per plane cell of the kernel that ran: plane_bytes == cells * 5 * elem."""
    cells = g.n * sum(L + 1 for L in lengths)
    assert stats["cells"] == cells
    assert stats["plane_bytes"] % (cells * 5) == 0
    return stats["plane_bytes"] // (cells * 5)


def _assert_batch_equals_oracle(res, D, oracle, n, tag):
    assert np.array_equal(res.score, D["score"]), (tag, np.flatnonzero(res.score != D["score"])[:8].tolist())
    assert np.array_equal(res.flags, D["flags"]), (tag, np.flatnonzero(res.flags != D["flags"])[:8].tolist())
    assert np.array_equal(np.diff(res.pair_off.astype(np.int64)), D["n_pairs"].astype(np.int64)), tag
    for i in range(n):
        assert res.raw_alignment(i) == oracle.batch_alignment(D, i), (tag, i)


_results = {}   # case name -> (score, flags, pair_off, pairs) of the GPU run, for the both-sides-of-the-bound comparison


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gpu_two_piece_shapes(engine, oracle, case):
    """One batch per case: score, flags and alignment of every query equal dense_batch bit for bit; the cell width that ran is
    the predicted one; the five planes of the chosen queries equal the oracle's cell for cell (u16: values above 65534 read INF)."""
    g, qs = _poa(case.kind).graph, _queries(case.kind, case.lengths)
    m, e1, o1, e2, o2 = case.costs
    pred = predict(g, case.lengths, case.costs, case.wide)
    og = _oracle_graph(oracle, case.kind)
    qseq, qoff = pack_queries(qs)
    al = _aligner(engine, case.costs)
    with _planes_env(case.wide):
        res = al.align_batch(g, qseq=qseq, qoff=qoff)
    with oracle.two_piece(o2, e2):
        D = og.dense_batch(qseq, qoff, oracle.Costs(m, o1, e1), threads=8)
    assert _elem_of(res.stats, g, case.lengths) == pred["elem"], (case.name, res.stats)
    assert res.stats["n_chunks"] == 1
    _assert_batch_equals_oracle(res, D, oracle, len(qs), case.name)
    _results[case.name] = (res.score.copy(), res.flags.copy(), res.pair_off.copy(), res.pairs.copy())
    rows = engine._device_graph(g).node_rows()
    for L in plane_lengths(pred, case.lengths):
        i = case.lengths.index(L)
        q = qs[i]
        # a batch of one query is what planes_2piece runs: its own pitch, its own ub
        p1 = predict(g, [L], case.costs, case.wide)
        with _planes_env(case.wide):
            one = al.align_batch(g, [q])
            gp = al.planes_2piece(g, q)
        assert _elem_of(one.stats, g, [L]) == p1["elem"], (case.name, L)
        assert int(one.score[0]) == int(D["score"][i]) and one.raw_alignment(0) == oracle.batch_alignment(D, i), (case.name, L)
        d, oplanes = _oracle_planes_by_row(oracle, engine, og, g, q, case.costs)
        assert d["score"] == int(D["score"][i])
        for name, a, b in zip(("M", "I1", "D1", "I2", "D2"), gp, oplanes):
            want = np.where(b <= 65534, b, np.uint32(INF)) if p1["elem"] == 2 else b
            got = a[rows]
            if not np.array_equal(got, want):
                r, c = np.argwhere(got != want)[0].tolist()
                pytest.fail("%s L=%d plane %s: first difference at oracle row %d column %d (pass %d): got %d, want %d; %d cells differ"
                            % (case.name, L, name, r, c, c // p1["PW"], int(got[r, c]), int(want[r, c]), int((got != want).sum())))


@pytest.mark.gpu
def test_gpu_two_piece_width_rule_both_sides(engine, oracle):
    """ub == 65534 runs u16 cells, ub one step above (by open1, or by one more column in the batch) runs u32 — no override —
    and the queries both batches share come out identical: the width changes nothing but the bytes."""
    g = _poa("chain").graph
    runs = {}
    for c in CASES:
        if not c.name.startswith("chain-ub"):
            continue
        if c.name not in _results:   # (run alone: -k)
            qseq, qoff = pack_queries(_queries(c.kind, c.lengths))
            with _planes_env(False):
                r = _aligner(engine, c.costs).align_batch(g, qseq=qseq, qoff=qoff)
            assert _elem_of(r.stats, g, c.lengths) == predict(g, c.lengths, c.costs, False)["elem"]
            _results[c.name] = (r.score, r.flags, r.pair_off, r.pairs)
        runs[c.name] = _results[c.name]
    at, longer = runs["chain-ub-at"], runs["chain-ub-above-length"]
    n = len(LENS)
    assert np.array_equal(at[0], longer[0][:n]) and np.array_equal(at[1], longer[1][:n])
    assert np.array_equal(at[2], longer[2][:n + 1])
    assert np.array_equal(at[3], longer[3][:int(at[2][n])])
    # one more unit of open1: every gap opening costs one more, nothing else moves; both runs equal the oracle (the cases above)
    og = _oracle_graph(oracle, "chain")
    qseq, qoff = pack_queries(_queries("chain", LENS))
    for name, costs in (("chain-ub-at", UB_AT), ("chain-ub-above-costs", UB_ABOVE)):
        m, e1, o1, e2, o2 = costs
        with oracle.two_piece(o2, e2):
            D = og.dense_batch(qseq, qoff, oracle.Costs(m, o1, e1), threads=8)
        assert np.array_equal(runs[name][0], D["score"]) and np.array_equal(runs[name][1], D["flags"])


@pytest.mark.gpu
def test_gpu_two_piece_scores_above_u16(engine, oracle):
    """36 602 rows x 1 501 columns under (4, 2, 6, 2, 24): every score is above 65534, so the u32 kernel runs by the rule and
    carries real u32 values; scores, flags and alignments equal dense_batch (planes are not fetched: 5 x 36 602 x 1 501 words)."""
    g, (qseq, qoff) = W.scaled_linearish(36000, 300, 150, 3, 1500)
    costs = (4, 2, 6, 2, 24)
    lengths = [1500, 1500, 1500]
    assert predict(g, lengths, costs, False)["elem"] == 4
    with _planes_env(False):
        res = _aligner(engine, costs).align_batch(g, qseq=qseq, qoff=qoff)
    assert _elem_of(res.stats, g, lengths) == 4
    assert int(res.score.min()) > 65534
    og = oracle.OracleGraph.from_csr(g.as_dict())
    with oracle.two_piece(24, 2):
        D = og.dense_batch(qseq, qoff, oracle.Costs(4, 6, 2), threads=3)
    assert int(D["score"][0]) == 69336
    _assert_batch_equals_oracle(res, D, oracle, 3, "u32 values")


@pytest.mark.gpu
def test_gpu_two_piece_chunk_loop(engine, oracle):
    """A batch whose planes exceed the 64 GiB budget whatever memory is free: the chunk loop runs with first_query > 0 (per-slot
    planes and scratch reused, results at their batch index).  Every result equals dense_batch; scores equal score_batch
    of the same aligner (the sweep kernel, which stores no planes and has no chunks)."""
    g, _ = W.config2(n_queries=1)
    pitch = (1000 + 64) & ~63
    n = (64 << 30) // (5 * g.n * pitch * 4) + 200
    g, (qseq, qoff) = W.config2(n_queries=n)
    lengths = np.diff(qoff.astype(np.int64)).tolist()
    assert max(lengths) == 1000 and 3400 < n < 3700
    costs = (4, 2, 6, 1, 24)
    al = _aligner(engine, costs)
    with _planes_env(True):
        res = al.align_batch(g, qseq=qseq, qoff=qoff)
    assert _elem_of(res.stats, g, lengths) == 4
    assert res.stats["n_chunks"] >= 2, res.stats
    og = oracle.OracleGraph.from_csr(g.as_dict())
    with oracle.two_piece(24, 1):
        D = og.dense_batch(qseq, qoff, oracle.Costs(4, 6, 2), threads=16)
    _assert_batch_equals_oracle(res, D, oracle, n, "chunks")
    sc, _ = al.score_batch(g, qseq=qseq, qoff=qoff)
    assert np.array_equal(sc, res.score)


# ---- POA_ERR_CAPACITY and the cost check through the raw C ABI ------------------------------------------------------------------
GUARD = 0xA5A5A5A5


def _raw_call(engine, fn, g, costs_struct, qseq, qoff, cap, room):
    """fn(graph, costs, n, qseq, qoff, score, pairs, pair_off, cap, flags, stats, device) on guard-filled buffers of `room`
    pairs; returns (rc, last error, score, flags, pair_off, pairs, stats)."""
    lib, p = engine._lib.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    dg = engine._device_graph(g)
    n = len(qoff) - 1
    score, flags = np.full(n, GUARD, np.uint32), np.full(n, GUARD, np.uint32)
    pair_off = np.full(n + 1, GUARD, np.uint64)
    pairs = np.full((room, 2), GUARD, np.uint32)
    st = engine._lib.PoaStats()
    rc = fn(dg.handle, C.byref(costs_struct), n, p(qseq), p(qoff), p(score), p(pairs), p(pair_off), cap, p(flags), C.byref(st), 0)
    return rc, lib.poa_last_error().decode(errors="replace"), score, flags, pair_off, pairs, st.as_dict()


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["two_piece", "one_piece"])
def test_gpu_pair_capacity_error(engine, oracle, model):
    """pair_capacity one short of the total, and 0: POA_ERR_CAPACITY (-5), pair_off[n] holds the needed total, poa_last_error()
    says why, nothing is written past the capacity given, and the same call with room returns what it returned before."""
    lib = engine._lib.lib()
    g, (qseq, qoff) = W.scaled_linearish(200, 10, 5, 12, 220)
    n = len(qoff) - 1
    if model == "two_piece":
        fn, cs = lib.poa_align_batch_2piece, engine._lib.PoaCosts2(4, 6, 2, 24, 1, 0)
    else:
        fn, cs = lib.poa_align_batch, engine._lib.PoaCosts(4, 6, 2, 0)
    room = int(qoff[-1]) + n * g.n + 16
    rc, _, score, flags, pair_off, pairs, _ = _raw_call(engine, fn, g, cs, qseq, qoff, room - 16, room)
    assert rc == 0
    total = int(pair_off[n])
    assert 0 < total <= room - 16 and (pairs[total:] == GUARD).all()
    og = oracle.OracleGraph.from_csr(g.as_dict())
    if model == "two_piece":
        with oracle.two_piece(24, 1):
            D = og.dense_batch(qseq, qoff, oracle.Costs(4, 6, 2))
    else:
        D = og.dense_batch(qseq, qoff, oracle.Costs(4, 6, 2))
    assert np.array_equal(score, D["score"]) and np.array_equal(np.diff(pair_off.astype(np.int64)), D["n_pairs"].astype(np.int64))
    for cap in (total - 1, 0):
        rc2, err, _, _, po2, pr2, _ = _raw_call(engine, fn, g, cs, qseq, qoff, cap, room)
        assert rc2 == -5 and engine._lib.ERRORS[rc2] == "POA_ERR_CAPACITY"
        assert int(po2[n]) == total, (cap, int(po2[n]), total)
        assert np.array_equal(po2, pair_off)
        assert err != ""
        assert (pr2[cap:] == GUARD).all()              # no pair lands past the capacity the caller gave
    assert fn(engine._device_graph(g).handle, C.byref(cs), n, qseq.ctypes.data_as(C.c_void_p), qoff.ctypes.data_as(C.c_void_p),
              None, None, None, 0, None, None, 0) == 0   # no pairs asked for: no capacity needed
    rc3, _, s3, f3, po3, pr3, _ = _raw_call(engine, fn, g, cs, qseq, qoff, total, room)   # exactly enough
    assert rc3 == 0
    assert np.array_equal(s3, score) and np.array_equal(f3, flags) and np.array_equal(po3, pair_off) and np.array_equal(pr3, pairs)


@pytest.mark.gpu
def test_gpu_two_piece_raw_costs_refused(engine):
    """extend1 < extend2 in a raw poa_costs2_t: POA_ERR_INVALID_ARG (-1) before anything runs — no output is touched."""
    lib = engine._lib.lib()
    g, (qseq, qoff) = W.scaled_linearish(200, 10, 5, 4, 220)
    n = len(qoff) - 1
    bad = engine._lib.PoaCosts2(4, 6, 1, 24, 2, 0)   # (mismatch, open1, extend1, open2, extend2): extend1 1 < extend2 2
    rc, err, score, flags, pair_off, pairs, st = _raw_call(engine, lib.poa_align_batch_2piece, g, bad, qseq, qoff, 4096, 4096)
    assert rc == -1 and "gap_extend1" in err
    assert (score == GUARD).all() and (flags == GUARD).all() and (pair_off == GUARD).all() and (pairs == GUARD).all()
    assert st["n_chunks"] == 0 and st["cells"] == 0 and st["n_forward_launches"] == 0
    good = engine._lib.PoaCosts2(4, 6, 2, 24, 1, 0)
    rc, _, score, _, pair_off, _, st = _raw_call(engine, lib.poa_align_batch_2piece, g, good, qseq, qoff, 4096, 4096)
    assert rc == 0 and st["n_chunks"] == 1 and int(pair_off[n]) > 0 and (score != GUARD).all()
