"""The one-shot calls of the two-piece model (poa_align_batch_2piece, poa_align_batch_2piece_ex) on the resident batch they
now run on: a batch, one run through the run frame, fetch, destroy.

1. The replay with queries of several pitches in one chunk: every query addresses its own region of the workspace with its own
   pitch (poa2_exact_kernel, poa2_traceback_kernel), so queries of 64, 128 and 192 columns side by side are the smallest shape
   at which that addressing can go wrong.
2. Back-to-back calls that take over the workspace the call before parked: replay, dense, replay.
3. What the calls report in poa_stats_t.
4. The refusals, their codes and texts, with every output left as the caller filled it.
5. A replay whose pair_capacity is too small: POA_ERR_CAPACITY, and scores, offsets and search counters all the same.

Every comparison is against the oracle (dense_batch, astar_align under oracle.two_piece), never against the engine."""
import ctypes as C
import functools

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import pack_queries

import test_run_frame as TRF

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7
GUARD = 0xA5A5A5A5
COSTS2 = TRF.COSTS2   # (mismatch, extend1, open1, extend2, open2) = (4, 2, 6, 1, 24)

# ---- 1. mixed pitches ------------------------------------------------------------------------------------------------------------
# 136 backbone nodes, 8 SNP bubbles, 4 two-node insertion branches: 152 nodes, 154 rows with the start and the end.  Lengths 0, 1, 63 have a pitch of 64 columns, 64 and
# 127 of 128, 128 and 150 of 192; the longest is neither first nor last.  The ends-free span is the unbounded one of test_two_piece.py.
MIXED_LENGTHS = (63, 128, 0, 150, 1, 127, 64)
MIXED_SEARCHES = (("Affine2PieceMinGapCost", "H_MINGAP", True), ("Affine2PieceDijkstra", "H_DIJKSTRA", False))


@functools.lru_cache(maxsize=None)
def _mixed():
    poa = W.LinearishPOA(136, 8, 4, seed=1)
    qs = [poa.queries(1, length=L, first=i)[0] if L else np.zeros(0, np.uint8) for i, L in enumerate(MIXED_LENGTHS)]
    return poa.graph, qs


def _engine_span(engine, ends_free):
    U = engine.Bound.Unbounded
    return engine.EndsFree(engine.Bound.Included(0), U, U, U) if ends_free else engine.AlignmentType.Global


def _oracle_span(oracle, ends_free):
    return oracle.ends_free((oracle.INCLUDED, 0), oracle.UNBOUNDED, oracle.UNBOUNDED, oracle.UNBOUNDED) if ends_free else None


def _search(oracle, og, q, costs, heur, prune, ospec):
    """The oracle's literal two-piece search of one query; RefPanic propagates."""
    m, e1, o1, e2, o2 = costs
    with oracle.two_piece(o2, e2):
        if ospec is None:
            return og.astar_align(q, oracle.Costs(m, o1, e1), heur, prune)
        with oracle.alignment_type(ospec):
            return og.astar_align(q, oracle.Costs(m, o1, e1), heur, prune)


@functools.lru_cache(maxsize=None)
def _mixed_expected(oracle, heur_name, prune, ends_free):
    g, qs = _mixed()
    og = oracle.OracleGraph.from_csr(g.as_dict())
    ospec = _oracle_span(oracle, ends_free)
    return [_search(oracle, og, q, COSTS2, getattr(oracle, heur_name), prune, ospec) for q in qs]


def test_mixed_pitch_shape_and_oracle_searches_complete(oracle):
    """The shape is what section 1 says it is, and the oracle's search ends without a RefPanic on every query of every case: the
    GPU test below skips nothing."""
    g, qs = _mixed()
    assert g.n == 154 and [len(q) for q in qs] == list(MIXED_LENGTHS)
    assert [(L + 64) & ~63 for L in MIXED_LENGTHS] == [64, 192, 64, 192, 64, 128, 128]
    assert max(MIXED_LENGTHS) not in (MIXED_LENGTHS[0], MIXED_LENGTHS[-1])
    for _, heur_name, prune in MIXED_SEARCHES:
        for ends_free in (False, True):
            for a in _mixed_expected(oracle, heur_name, prune, ends_free):   # (a RefPanic raises here)
                assert a["score"] >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("ends_free", [False, True], ids=["global", "ends-free"])
@pytest.mark.parametrize("search", MIXED_SEARCHES, ids=["mingap-pruned", "dijkstra-unpruned"])
def test_gpu_replay_mixed_pitches_in_one_chunk(engine, oracle, search, ends_free):
    """Score, alignment and the three search counters of every query equal the oracle's search."""
    cfg_name, heur_name, prune = search
    g, qs = _mixed()
    aln_type = _engine_span(engine, ends_free)
    al = engine.PoastaAligner(getattr(engine, cfg_name)(engine.GapAffine2Piece(*COSTS2)), aln_type, mode="exact")
    res = al.align_batch(g, qs, pruning=prune)
    assert res.stats["n_chunks"] == 1, res.stats
    want = _mixed_expected(oracle, heur_name, prune, ends_free)
    for i, (q, a) in enumerate(zip(qs, want)):
        tag = (cfg_name, prune, ends_free, i, len(q))
        print(tag, "score", int(res.score[i]), a["score"], "counters", res.search_counters[i, :3].tolist())
        assert int(res.flags[i]) & ~engine._lib.FLAG_TRUNCATED == 0, (tag, int(res.flags[i]))
        assert int(res.score[i]) == a["score"], tag
        assert res.raw_alignment(i) == a["alignment"], tag
        assert res.search_counters[i, :3].tolist() == [a["num_queued"], a["num_visited"], a["num_pruned"]], tag


# ---- 2. and 3.: the tiny inputs of test_run_frame.py ---------------------------------------------------------------------------
def _aligner(engine, mode):
    cls = engine.Affine2PieceMinGapCost if mode == "exact" else engine.Affine2PieceDijkstra
    return engine.PoastaAligner(cls(engine.GapAffine2Piece(*COSTS2)), mode=mode)


def _check_replay(engine, oracle, res, queries, what):
    og = oracle.OracleGraph.from_csr(TRF.GRAPHS[0].as_dict())
    for i, q in enumerate(queries):
        a = _search(oracle, og, np.frombuffer(q, np.uint8), COSTS2, oracle.H_MINGAP, True, None)
        assert int(res.flags[i]) & ~engine._lib.FLAG_TRUNCATED == 0, (what, i)
        assert int(res.score[i]) == a["score"] and res.raw_alignment(i) == a["alignment"], (what, i)
        assert res.search_counters[i, :3].tolist() == [a["num_queued"], a["num_visited"], a["num_pruned"]], (what, i)


def _check_dense(oracle, res, first, count, what):
    D = TRF._oracle_dense(oracle, 0, True)   # all of QUERIES against graph 0
    for i in range(count):
        assert int(res.score[i]) == int(D["score"][first + i]) and int(res.flags[i]) == int(D["flags"][first + i]), (what, i)
        assert res.raw_alignment(i) == oracle.batch_alignment(D, first + i), (what, i)


@pytest.mark.gpu
def test_gpu_back_to_back_calls_reuse_the_parked_workspace(engine, oracle):
    """A replay of four queries, a dense call of two, a replay of two: the second and third call take over the workspace the
    call before parked, with its contents.  The replay's tables start unvisited by its own memsets, not by fresh memory."""
    Q = TRF.QUERIES
    r1 = _aligner(engine, "exact").align_batch(TRF.GRAPHS[0], [np.frombuffer(q, np.uint8) for q in Q])
    _check_replay(engine, oracle, r1, Q, "first replay")
    r2 = _aligner(engine, "dense").align_batch(TRF.GRAPHS[0], [np.frombuffer(q, np.uint8) for q in Q[:2]])
    _check_dense(oracle, r2, 0, 2, "dense")
    r3 = _aligner(engine, "exact").align_batch(TRF.GRAPHS[0], [np.frombuffer(q, np.uint8) for q in Q[2:]])
    _check_replay(engine, oracle, r3, Q[2:], "second replay")


@pytest.mark.gpu
def test_gpu_one_shot_stats(engine, oracle, monkeypatch):
    """What poa_stats_t says after a one-shot call, dense under both cell widths and replayed."""
    g, Q = TRF.GRAPHS[0], TRF.QUERIES
    qs = [np.frombuffer(q, np.uint8) for q in Q]
    cells, bases = g.n * sum(len(q) + 1 for q in Q), sum(len(q) for q in Q)
    for wide, elem in ((False, 2), (True, 4)):
        if wide:
            monkeypatch.setenv("POA_PLANES", "32")   # GapAffine2Piece._c() reads it: poa_costs2_t.wide_planes
        else:
            monkeypatch.delenv("POA_PLANES", raising=False)
        res = _aligner(engine, "dense").align_batch(g, qs)
        st = res.stats
        print("dense", "wide" if wide else "narrow", st)
        _check_dense(oracle, res, 0, len(Q), ("stats", wide))
        assert (st["cells"], st["bases"], st["n_queries"]) == (cells, bases, len(Q)), st
        assert st["n_chunks"] == 1 and st["n_forward_launches"] == 1, st
        assert st["plane_bytes"] == cells * 5 * elem, st
        assert st["n_flagged"] == int(np.count_nonzero(res.flags)), st
    monkeypatch.delenv("POA_PLANES", raising=False)
    res = _aligner(engine, "exact").align_batch(g, qs)
    st = res.stats
    print("replay", st)
    _check_replay(engine, oracle, res, Q, "stats")
    assert st["n_exact"] == len(Q) and st["ms_forward"] == 0 and st["ms_exact"] > 0, st
    assert (st["cells"], st["bases"], st["n_queries"], st["n_chunks"]) == (cells, bases, len(Q), 1), st


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
# (code, text) as run_two_piece returned them before the one-shot calls moved onto the resident batch
REFUSALS = {
    "checkpoint": (ERR_UNSUPPORTED, b"checkpointed mode: one-piece gap-affine model only"),
    "mode above checkpoint2": (ERR_INVALID_ARG, b"poa_align_batch_2piece_ex: unknown mode"),
    "span above ends-free": (ERR_INVALID_ARG, b"poa_align_batch_2piece_ex: unknown alignment span"),
    "ends-free dense": (ERR_UNSUPPORTED, b"two-piece model: ends-free alignment needs the exact replay (mode EXACT)"),
    "ends-free score": (ERR_UNSUPPORTED, b"score-only mode is Global: an ends-free result is defined by the reference's search"),
    "ends-free checkpoint2": (ERR_UNSUPPORTED, b"checkpointed mode is Global: an ends-free result is defined by the reference's search"),
    "extend1 < extend2": (ERR_INVALID_ARG, b"gap_extend1 must be greater than or equal to gap_extend2 for two-piece model"),
    "null graph": (ERR_INVALID_ARG, b"poa_align_batch_2piece: null argument"),
    "null costs": (ERR_INVALID_ARG, b"poa_align_batch_2piece: null argument"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSALS))
def test_gpu_one_shot_refusals(engine, name):
    """The code, the text of poa_last_error(), and no output touched: score, flags, pair_off, pairs, counters and stats."""
    L, lib = engine._lib.lib(), engine._lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    qseq, qoff = pack_queries([np.frombuffer(q, np.uint8) for q in TRF.QUERIES])
    qseq, qoff = np.ascontiguousarray(qseq, np.uint8), np.ascontiguousarray(qoff, np.uint64)
    n = len(qoff) - 1
    handle = engine._device_graph(TRF.GRAPHS[0]).handle
    m, e1, o1, e2, o2 = COSTS2
    costs = lib.PoaCosts2(m, o1, e1, o2, e2, 0)   # (mismatch, open1, extend1, open2, extend2, wide_planes)
    ends_free = engine.EndsFree(engine.Bound.Included(0), engine.Bound.Unbounded, engine.Bound.Unbounded, engine.Bound.Unbounded)
    if name == "checkpoint":
        cfg = engine.make_config("checkpoint")
    elif name == "mode above checkpoint2":
        cfg = engine.make_config(lib.MODE_CHECKPOINT2 + 1)
    elif name == "span above ends-free":
        cfg = engine.make_config("dense")
        cfg.span = lib.SPAN_ENDS_FREE + 1
    elif name.startswith("ends-free"):
        cfg = engine.make_config(name.split()[1], aln_type=ends_free)
    else:
        cfg = engine.make_config("dense")
    if name == "extend1 < extend2":
        costs = lib.PoaCosts2(m, o1, 1, o2, 2, 0)
    room = int(qoff[-1]) + n * TRF.GRAPHS[0].n
    score, flags = np.full(n, GUARD, np.uint32), np.full(n, GUARD, np.uint32)
    pair_off, pairs = np.full(n + 1, GUARD, np.uint64), np.full((room, 2), GUARD, np.uint32)
    counters = np.full((n, 4), GUARD, np.uint32)
    st = lib.PoaStats()
    C.memset(C.byref(st), 0xA5, C.sizeof(st))
    before = bytes(st)
    rc = L.poa_align_batch_2piece_ex(None if name == "null graph" else handle, None if name == "null costs" else C.byref(costs), C.byref(cfg), n,
                                     p(qseq), p(qoff), p(score), p(pairs), p(pair_off), room, p(flags), C.byref(st), p(counters), 0)
    assert (rc, L.poa_last_error()) == REFUSALS[name], (name, rc, L.poa_last_error())
    for a in (score, flags, pair_off, pairs, counters):
        assert (a == GUARD).all(), name
    assert bytes(st) == before, name


@pytest.mark.gpu
def test_gpu_replay_capacity_error_keeps_the_rest(engine, oracle):
    """pair_capacity 0 on a replay: POA_ERR_CAPACITY, and scores, pair_off and the search counters are there all the same."""
    L, lib = engine._lib.lib(), engine._lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    qseq, qoff = pack_queries([np.frombuffer(q, np.uint8) for q in TRF.QUERIES])
    qseq, qoff = np.ascontiguousarray(qseq, np.uint8), np.ascontiguousarray(qoff, np.uint64)
    n = len(qoff) - 1
    m, e1, o1, e2, o2 = COSTS2
    costs = lib.PoaCosts2(m, o1, e1, o2, e2, 0)
    cfg = engine.make_config("exact")
    score, flags = np.full(n, GUARD, np.uint32), np.full(n, GUARD, np.uint32)
    pair_off, pairs = np.full(n + 1, GUARD, np.uint64), np.full((64, 2), GUARD, np.uint32)
    counters = np.full((n, 4), GUARD, np.uint32)
    st = lib.PoaStats()
    rc = L.poa_align_batch_2piece_ex(engine._device_graph(TRF.GRAPHS[0]).handle, C.byref(costs), C.byref(cfg), n, p(qseq), p(qoff), p(score),
                                     p(pairs), p(pair_off), 0, p(flags), C.byref(st), p(counters), 0)
    assert rc == -5 and (pairs == GUARD).all(), rc
    og = oracle.OracleGraph.from_csr(TRF.GRAPHS[0].as_dict())
    for i, q in enumerate(TRF.QUERIES):
        a = _search(oracle, og, np.frombuffer(q, np.uint8), COSTS2, oracle.H_MINGAP, True, None)
        assert int(score[i]) == a["score"] and int(pair_off[i + 1] - pair_off[i]) == len(a["alignment"]), i
        assert counters[i, :3].tolist() == [a["num_queued"], a["num_visited"], a["num_pruned"]], i
