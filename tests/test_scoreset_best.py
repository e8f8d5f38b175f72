"""Best-of score-set runs (poa_scoreset_run_best / _run_2piece_best, poa_scoreset_fetch_best, poa_score_best*).

The contract, with s_p the oracle's score of pair p and T_q = min(best score of q + slack, limit[q]) (include/
poasta_amd_scoreset_best.h): poa_best_t is checked field by field against numpy over the oracle's scores; per pair, s_p <= T_q
gives (s_p, the uncapped flags), a pair reported as capped has s_p > T_q, and a pair above T_q is either.  That the cap really
tightens is checked separately, where scheduling cannot matter: in a second chunk, which runs after the first has finished."""
import ctypes as C

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

from test_scoreset_cap import (ACGT, CAPPED, COSTS, COSTS2, EMPTY_GRAPH, NONE, SHORT_QUERY, _bubble_graph, _chain, _costs, _expected_swept,
                               _m_rows, _oracle_scores, _small)

ERR_INVALID_ARG = -1
FIELDS = ("pair", "score", "flags", "second_score", "n_within")


def _flags0(graphs, seqs, pairs):
    """The uncapped flags of every pair: they follow from the input alone."""
    return np.array([EMPTY_GRAPH if graphs[gi].n == 2 else (SHORT_QUERY if len(seqs[qi]) == 1 else 0) for qi, gi in pairs], np.uint32)


def _best_ref(s, pair_query, nq, slack, limit, flags0):
    """poa_best_t per query and T per query, from the uncapped scores s (u32, in pair order)."""
    s = s.astype(np.int64)
    lim = np.full(nq, NONE, np.int64) if limit is None else np.asarray(limit, np.int64)
    out = {k: np.zeros(nq, np.uint32) for k in FIELDS}
    T = np.zeros(nq, np.int64)
    for q in range(nq):
        idx = np.flatnonzero(pair_query == q)
        e = idx[(s[idx] != NONE) & (s[idx] <= lim[q])]
        if len(e):
            bs = int(s[e].min())
            bp = int(e[s[e] == bs][0])
            T[q] = min(min(bs + slack, NONE), lim[q])
            fl = int(flags0[bp])
        else:
            bs, bp, fl = NONE, NONE, 0
            T[q] = lim[q]
        within = idx[s[idx] <= T[q]]
        others = within[within != bp]
        out["pair"][q], out["score"][q], out["flags"][q] = bp, bs, fl
        out["second_score"][q] = int(s[others].min()) if len(others) else NONE
        out["n_within"][q] = len(within)
    return out, T


def _check(ss, s, pair_query, nq, slack, limit, flags0, what):
    """fetch_best against _best_ref, fetch against the per-pair rule; returns (best, T per pair)."""
    want, T = _best_ref(s, pair_query, nq, slack, limit, flags0)
    got = ss.fetch_best()
    for k in FIELDS:
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, (what, k, [(int(q), int(got[k][q]), int(want[k][q])) for q in bad[:5]])
    score, flags, _ = ss.fetch()
    Tp = T[pair_query] if len(pair_query) else np.zeros(0, np.int64)
    within = s.astype(np.int64) <= Tp
    capped = (flags & CAPPED) != 0
    assert not (capped & within).any(), (what, "a pair within T is reported as capped", np.flatnonzero(capped & within)[:5])
    assert np.array_equal(score[within], s[within]) and np.array_equal(flags[within], flags0[within]), (what, "pairs within T")
    exact = (score == s) & (flags == flags0)
    stopped = (score == NONE) & (flags == (flags0 | CAPPED))
    assert (exact | stopped)[~within].all(), (what, "pairs above T", np.flatnonzero(~within & ~(exact | stopped))[:5])
    return got, Tp


def _matrix_pq(nq, ng):
    return np.repeat(np.arange(nq), ng)


def _limits(ref, rng=None):
    """Per query, by turns: none; below every score of the query (where its smallest score is not 0); exactly its second
    smallest score; exactly its smallest."""
    srt = np.sort(ref.astype(np.int64), axis=1)
    kind = np.arange(len(ref)) % 4
    lim = np.select([kind == 0, (kind == 1) & (srt[:, 0] > 0), kind == 2], [NONE + 0 * srt[:, 0], srt[:, 0] - 1, srt[:, 1]], srt[:, 0])
    assert ((lim < srt[:, 0]).sum() >= 2) and (lim == srt[:, 1]).any() and (lim == NONE).any()
    return lim.astype(np.uint32)


# ---- 1. the contract, every kernel class ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("costs", [COSTS, COSTS2], ids=["one-piece", "two-piece"])
def test_best_contract_every_kernel_class(engine, oracle, costs):
    d = _small(oracle)
    graphs, seqs = d["graphs"], d["seqs"]
    ref = d["ref"] if costs is COSTS else d["ref2"]
    s = ref.reshape(-1)
    nq, ng = len(seqs), len(graphs)
    # pitches of every class: Q1 (pitch <= 512), packed (512 < pitch <= 1024), two strips; u32: Q1 <= 256 < Q2 <= 512 < Q4
    lens = sorted(len(q) for q in seqs)
    assert lens[0] == 0 and any(256 < l + 1 <= 512 for l in lens) and any(512 < l + 1 <= 1024 for l in lens) and lens[-1] + 1 > 1024
    pq = _matrix_pq(nq, ng)
    flags0 = _flags0(graphs, seqs, [(qi, gi) for qi in range(nq) for gi in range(ng)])
    ss = engine.ScoreSet(graphs, seqs)
    ss.run(_costs(engine, costs))
    score0, f0, _ = ss.fetch()
    assert np.array_equal(score0, s) and np.array_equal(f0, flags0)
    seen_capped = seen_none = 0
    for tune in ({}, {"planes": 32}, {"cap_stride": 1}, {"planes": 32, "cap_stride": 1}):
        cfg = engine.make_config("score", **tune)
        for slack in (0, 3, 0xFFFFFFFF):
            for limit in (None, _limits(ref)):
                ss.run(_costs(engine, costs), config=cfg, best=True, slack=slack, limit=limit)
                got, Tp = _check(ss, s, pq, nq, slack, limit, flags0, (tune, slack, limit is not None))
                _, flags, _ = ss.fetch()
                seen_capped += int(((flags & CAPPED) != 0).sum())
                seen_none += int((got["pair"] == NONE).sum())
                swept = ss.swept_rows()
                rows = np.array([0 if g.n == 2 else g.n * (2 if len(q) + 1 > 1024 else 1) for q in seqs for g in graphs], np.uint32)
                assert (swept <= rows).all() and (swept[(flags & CAPPED) == 0] == rows[(flags & CAPPED) == 0]).all()
                if slack == 0xFFFFFFFF and limit is None:   # no cap can form: the uncapped run, bit for bit
                    sc, fl, _ = ss.fetch()
                    assert np.array_equal(sc, s) and np.array_equal(fl, flags0) and np.array_equal(swept, rows)
                    assert (got["n_within"] == ng).all()
    assert seen_capped > 0 and seen_none > 0
    ss.close()


# ---- 2. ties and order ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_best_ties_and_order(engine, oracle):
    rng = np.random.default_rng(60)
    bubble = _bubble_graph()
    chain_seqs = [rng.choice(ACGT, n) for n in (20, 31, 38)]
    chains = [_chain(c) for c in chain_seqs]
    graphs = [bubble, chains[0], bubble, chains[1], chains[2]]   # the bubble graph twice: the same object, the same handle
    seqs = [W.random_walk_query(rng, bubble, 0.1), W.mutate(rng, chain_seqs[0], 0.1, 0.05, 0.05), rng.choice(ACGT, 33),
            W.random_walk_query(rng, bubble, 0.3), rng.choice(ACGT, 48), rng.choice(ACGT, 7)]
    ref = _oracle_scores(oracle, graphs, seqs, COSTS)
    assert np.array_equal(ref[:, 0], ref[:, 2])
    # query 0: its best graph is the bubble graph, listed at pairs 1 and 3 (a tie between two listings) and again at 6 (a
    # repeated pair); query 2: the same pair three times; query 5 has no pair at all; query 4: one pair
    pairs = [(0, 1), (0, 2), (2, 3), (0, 0), (2, 3), (3, 4), (0, 2), (3, 0), (2, 3), (1, 1), (3, 2), (4, 3), (1, 3), (1, 4)]
    assert ref[0, 0] < min(ref[0, 1], ref[0, 3], ref[0, 4])
    pr = np.asarray(pairs)
    s = ref[pr[:, 0], pr[:, 1]]
    flags0 = _flags0(graphs, seqs, pairs)
    ss = engine.ScoreSet(graphs, seqs, pairs=pairs)
    for slack in (0, 5, 0xFFFFFFFF):
        ss.run(_costs(engine, COSTS), best=True, slack=slack)
        got, _ = _check(ss, s, pr[:, 0], len(seqs), slack, None, flags0, ("ties", slack))
        assert got["pair"][0] == 1 and got["second_score"][0] == got["score"][0] and got["n_within"][0] >= 3   # the lowest index of three
        assert got["pair"][2] == 2 and got["n_within"][2] == 3
        assert got["pair"][5] == NONE and got["score"][5] == NONE and got["flags"][5] == 0 and got["n_within"][5] == 0
        assert got["pair"][4] == 11 and got["second_score"][4] == NONE and got["n_within"][4] == 1
    ss.close()
    # permuting the pair list leaves every query's winning graph and score unchanged where its scores are distinct
    graphs = [bubble] + chains
    ref = _oracle_scores(oracle, graphs, seqs, COSTS)
    distinct = np.array([len(set(row)) == len(row) for row in ref.tolist()])
    assert distinct.sum() >= 4
    base = [(qi, gi) for qi in range(len(seqs)) for gi in range(len(graphs))]
    winners = []
    for seed in range(4):
        order = np.random.default_rng(seed).permutation(len(base)) if seed else np.arange(len(base))
        pairs = [base[i] for i in order]
        pr = np.asarray(pairs)
        ss = engine.ScoreSet(graphs, seqs, pairs=pairs)
        ss.run(_costs(engine, COSTS), best=True)
        got, _ = _check(ss, ref[pr[:, 0], pr[:, 1]], pr[:, 0], len(seqs), 0, None, _flags0(graphs, seqs, pairs), ("permutation", seed))
        ss.close()
        winners.append((pr[got["pair"], 1][distinct], got["score"][distinct]))
        assert np.array_equal(winners[-1][0], ref.argmin(axis=1)[distinct]) and np.array_equal(winners[-1][1], ref.min(axis=1)[distinct])
        assert np.array_equal(winners[-1][0], winners[0][0]) and np.array_equal(winners[-1][1], winners[0][1])


# ---- 3. the cap really tightens ---------------------------------------------------------------------------------------------
_TIGHT = {}


def _tight(oracle, engine):
    """Chains of 38 nodes (40 rows) and the bubble graph, reads of each; one chain of 1100 nodes and its read of 1100 symbols
    (stated exception to the small shapes: the wide pair needs an own graph it scores low on).  First every query against its
    own graph, then the hopeless pairs: every read on the other graphs, the wide read on the short chains only (so that the
    largest pair of the set, wide read x chain, lies in the first group and the workspace cap is not raised)."""
    if not _TIGHT:
        rng = np.random.default_rng(61)
        chain_seqs = [rng.choice(ACGT, 38) for _ in range(4)]
        wide_seq = rng.choice(ACGT, 1100)
        graphs = [_chain(c) for c in chain_seqs] + [_bubble_graph(), _chain(wide_seq)]
        assert all(g.n == 40 for g in graphs[:4]) and graphs[4].n <= 40
        seqs, own = [], []
        for gi in range(4):
            for _ in range(3):
                seqs.append(W.mutate(rng, chain_seqs[gi], 0.08, 0.04, 0.04)[:48])
                own.append(gi)
        for _ in range(4):
            seqs.append(W.random_walk_query(rng, graphs[4], 0.1))
            own.append(4)
        wide = W.mutate(rng, wide_seq, 0.02, 0.0, 0.0)
        assert len(wide) == 1100
        seqs.append(wide)
        own.append(5)
        first = [(qi, gi) for qi, gi in enumerate(own)]
        second = [(qi, gi) for qi in range(len(seqs) - 1) for gi in range(5) if gi != own[qi]] + [(len(seqs) - 1, gi) for gi in range(4)]
        planes = {p: _m_rows(oracle, engine, graphs[p[1]], seqs[p[0]], COSTS) for p in first + second}
        _TIGHT.update(graphs=graphs, seqs=seqs, first=first, second=second, planes=planes)
    return _TIGHT


@pytest.mark.gpu
def test_best_cap_tightens_in_the_second_chunk(engine, oracle):
    d = _tight(oracle, engine)
    graphs, seqs, first, second, planes = d["graphs"], d["seqs"], d["first"], d["second"], d["planes"]
    pairs = first + second
    pr = np.asarray(pairs)
    s = np.array([planes[p][1] for p in pairs], np.int64)
    nq, wide_q = len(seqs), len(seqs) - 1
    # the own graph is the best one of every query: after chunk 0 the bests are final, T_q = s(own) at slack 0
    T = s[:nq].copy()
    assert (s[nq:] >= T[pr[nq:, 0]]).all()
    stride = 1

    def predicted(p, cap):
        g, (m_plane, _) = graphs[p[1]], planes[p]
        if len(seqs[p[0]]) + 1 > 1024:   # two strips: the end of the first one, on M of its last column
            return g.n if int(m_plane[:, 1023].min()) > cap else 2 * g.n
        return _expected_swept(engine, g, m_plane, cap, stride)

    for slack in (0, 4):
        want = np.array([predicted(p, int(T[p[0]]) + slack) for p in second])
        full = np.array([graphs[gi].n * (2 if qi == wide_q else 1) for qi, gi in second])
        early = want < full
        print("slack %d: the oracle predicts an early stop for %d of %d second-chunk pairs, mean swept fraction %.3f"
              % (slack, early.sum(), len(second), float((want / full).mean())))
        assert early.sum() * 4 >= 3 * len(second)
        assert all(want[i] == graphs[gi].n for i, (qi, gi) in enumerate(second) if qi == wide_q)   # the wide pairs: at the strip end
        # chunk 0 closes exactly behind the first group
        ws, _ = engine.scoreset_footprint(graphs, seqs, pairs=first)
        ss = engine.ScoreSet(graphs, seqs, pairs=pairs, workspace_bytes=ws)
        ss.run(_costs(engine, COSTS), config=engine.make_config("score", cap_stride=stride), best=True, slack=slack)
        st = ss.stats()
        assert st["n_chunks"] >= 2
        _check(ss, s.astype(np.uint32), pr[:, 0], nq, slack, None, _flags0(graphs, seqs, pairs), ("tight", slack))
        swept = ss.swept_rows()
        bad = [(second[i], int(swept[nq + i]), int(want[i])) for i in range(len(second)) if swept[nq + i] != want[i]]
        assert not bad, bad[:8]
        score, flags, _ = ss.fetch()
        assert ((flags[nq:] & CAPPED) != 0).sum() >= early.sum()
        ss.close()


# ---- 4. alternation ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_best_alternation_errors_and_one_shots(engine, oracle):
    from poasta_amd import _lib
    L = _lib.lib()
    p = engine._p
    d = _small(oracle)
    graphs, seqs = d["graphs"], d["seqs"]
    nq, ng = len(seqs), len(graphs)
    s1, s2 = d["ref"].reshape(-1), d["ref2"].reshape(-1)
    pq = _matrix_pq(nq, ng)
    flags0 = _flags0(graphs, seqs, [(qi, gi) for qi in range(nq) for gi in range(ng)])
    rec = np.zeros((nq, 8), np.uint32)
    ss = engine.ScoreSet(graphs, seqs)
    ptr = C.c_void_p()
    assert L.poa_scoreset_fetch_best(ss.handle, p(rec)) == ERR_INVALID_ARG and L.poa_last_error() != b""   # before any run
    assert L.poa_scoreset_device_best(ss.handle, C.byref(ptr)) == ERR_INVALID_ARG
    lim1 = _limits(d["ref"])
    ss.run(_costs(engine, COSTS), best=True, slack=0, limit=lim1)
    first, _ = _check(ss, s1, pq, nq, 0, lim1, flags0, "best 1")
    assert L.poa_scoreset_device_best(ss.handle, C.byref(ptr)) == 0 and ptr.value
    ss.run(_costs(engine, COSTS))                                       # uncapped
    score, flags, _ = ss.fetch()
    assert np.array_equal(score, s1) and np.array_equal(flags, flags0)
    assert L.poa_scoreset_fetch_best(ss.handle, p(rec)) == ERR_INVALID_ARG and b"best-of" in L.poa_last_error()
    cap = np.full(len(s1), int(np.median(s1)), np.uint32)
    ss.run(_costs(engine, COSTS), cap=cap)                              # capped
    score, flags, _ = ss.fetch()
    over = s1 > cap
    assert np.array_equal(score, np.where(over, NONE, s1)) and np.array_equal(flags, np.where(over, flags0 | CAPPED, flags0))
    assert L.poa_scoreset_fetch_best(ss.handle, p(rec)) == ERR_INVALID_ARG
    # best again, higher costs, other slack and no limit: nothing of the first run's bests may survive — every score is at least
    # what it was, so an inherited best would win wherever the score went up
    high = (8, 12, 4)
    s3 = _oracle_scores(oracle, graphs, seqs, high).reshape(-1)
    assert (s3 >= s1).all() and (s3 > s1).any()
    ss.run(_costs(engine, high), best=True, slack=7)
    second, _ = _check(ss, s3, pq, nq, 7, None, flags0, "best 2")
    assert (second["score"] != first["score"]).any()
    ss.run(_costs(engine, COSTS2), best=True, slack=2, limit=lim1)       # and the two-piece model on the same set
    _check(ss, s2, pq, nq, 2, lim1, flags0, "best 3, two-piece")
    ss.run(_costs(engine, high), best=True, slack=7)
    second, _ = _check(ss, s3, pq, nq, 7, None, flags0, "best 4")
    # a refused call in between leaves the set and its result as they were
    c = _costs(engine, COSTS)._c()
    assert L.poa_scoreset_run_best(ss.handle, None, None, 0, None, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_run_best(ss.handle, C.byref(c), C.byref(engine.make_config("dense")), 0, None, None) == -7
    bad2 = _lib.PoaCosts2(4, 6, 1, 24, 2, 0)
    assert L.poa_scoreset_run_2piece_best(ss.handle, C.byref(bad2), None, 0, None, None) == ERR_INVALID_ARG
    again = ss.fetch_best()
    assert all(np.array_equal(again[k], second[k]) for k in FIELDS)
    with pytest.raises(ValueError):
        ss.run(_costs(engine, COSTS), best=True, limit=[1, 2, 3])
    with pytest.raises(ValueError):
        ss.run(_costs(engine, COSTS), best=True, cap=5)
    # the one-shots equal the resident runs
    si = ss.input
    for costs, s, slack, limit in ((COSTS, s1, 0, lim1), (COSTS2, s2, 7, None)):
        ss.run(_costs(engine, costs), best=True, slack=slack, limit=limit)
        resident = ss.fetch_best()
        r_score, r_flags, _ = ss.fetch()
        rec[:] = 0
        score, flags = np.zeros(len(s), np.uint32), np.zeros(len(s), np.uint32)
        st = _lib.PoaStats()
        cc = _costs(engine, costs)._c()
        fn = L.poa_score_best if len(costs) == 3 else L.poa_score_best_2piece
        _lib.check(fn(si.handles, ng, C.byref(cc), None, nq, p(si.qseq), p(si.qoff), nq * ng, None, None, slack, p(limit), p(rec), p(score),
                      p(flags), C.byref(st), 0))
        for i, k in enumerate(FIELDS):
            assert np.array_equal(rec[:, i], resident[k]), k
        assert (rec[:, 5:] == 0).all() and st.n_queries == nq * ng
        T = _best_ref(s, pq, nq, slack, limit, flags0)[1][pq]
        within = s.astype(np.int64) <= T
        assert np.array_equal(score[within], r_score[within]) and np.array_equal(flags[within], r_flags[within])
        rec[:] = 0
        _lib.check(fn(si.handles, ng, C.byref(cc), None, nq, p(si.qseq), p(si.qoff), nq * ng, None, None, slack, p(limit), p(rec), None, None, None, 0))
        assert np.array_equal(rec[:, 0], resident["pair"])
    ss.close()
    # a set without pairs: every query gets POA_NONE
    empty = engine.ScoreSet(graphs, seqs, pairs=np.zeros((0, 2), np.int64))
    empty.run(_costs(engine, COSTS), best=True)
    got = empty.fetch_best()
    assert (got["pair"] == NONE).all() and (got["score"] == NONE).all() and (got["n_within"] == 0).all() and len(got["pair"]) == nq
    empty.close()


# ---- 5. soundness on random input -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_best_random_input_is_sound(engine, oracle):
    rng = np.random.default_rng(62)
    graphs, seqs, pairs = [], [], []
    for seed in range(36):
        alpha = b"AC" if seed % 2 else b"ACGT"
        g = W.random_dag(900 + seed, n_nodes=int(rng.integers(3, 31)), p_edge=float(rng.choice([0.05, 0.15, 0.3])), alphabet=alpha)
        graphs.append(g)
        for _ in range(2):
            seqs.append(W.random_walk_query(rng, g, 0.3, alpha)[:48])
    seqs += [np.zeros(0, np.uint8), rng.choice(ACGT, 1), rng.choice(ACGT, 9)]   # (the last one gets no pair)
    for qi in range(len(seqs) - 1):
        others = rng.choice(len(graphs), int(rng.integers(1, 6)), replace=False)
        pairs += [(qi, int(k)) for k in others] + ([(qi, qi // 2)] if qi // 2 < len(graphs) else [])
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    assert 250 <= len(pairs) <= 400
    pr = np.asarray(pairs)
    nq = len(seqs)
    flags0 = _flags0(graphs, seqs, pairs)
    ss = engine.ScoreSet(graphs, seqs, pairs=pairs)
    seen_capped = 0
    for turn, (m, o, e) in enumerate(((4, 6, 2), (3, 0, 1), (1, 0, 5), (9, 12, 1))):   # o = 0 included
        s = _oracle_scores(oracle, graphs, seqs, (m, o, e))[pr[:, 0], pr[:, 1]]
        slack = int(rng.integers(0, 6))
        limit = None if turn % 2 == 0 else rng.integers(0, int(s.max()) + 2, nq).astype(np.uint32)
        ss.run(_costs(engine, (m, o, e)), config=engine.make_config("score", cap_stride=1), best=True, slack=slack, limit=limit)
        _check(ss, s, pr[:, 0], nq, slack, limit, flags0, ("random", m, o, e))
        seen_capped += int(((ss.fetch()[1] & CAPPED) != 0).sum())
    assert seen_capped > 0
    ss.close()


# ---- 6. Python --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_best_python_assign(engine, oracle):
    d = _small(oracle)
    graphs, seqs = d["graphs"], d["seqs"]
    nq, ng = len(seqs), len(graphs)
    for costs, ref in ((COSTS, d["ref"]), (COSTS2, d["ref2"])):
        cfg = engine.AffineMinGapCost(_costs(engine, costs)) if len(costs) == 3 else engine.Affine2PieceDijkstra(_costs(engine, costs))
        al = engine.PoastaAligner(cfg)
        m = al.score_matrix(graphs, seqs)
        assert np.array_equal(m, ref)
        a = al.assign(graphs, seqs)
        assert np.array_equal(a["graph"], m.argmin(axis=1)) and np.array_equal(a["score"], m.min(axis=1))
        assert np.array_equal(a["n_within"], (m == m.min(axis=1)[:, None]).sum(axis=1))
        a = al.assign(graphs, seqs, slack=10)
        srt = np.sort(m.astype(np.int64), axis=1)
        assert np.array_equal(a["second_score"], np.where(srt[:, 1] <= srt[:, 0] + 10, srt[:, 1], NONE))
        assert np.array_equal(a["n_within"], (m.astype(np.int64) <= srt[:, :1] + 10).sum(axis=1))
        limit = int(np.median(m.min(axis=1)))
        a = al.assign(graphs, seqs, max_score=limit)
        assert np.array_equal(a["graph"], np.where(m.min(axis=1) <= limit, m.argmin(axis=1), -1)) and (a["graph"] == -1).any()
        # a pair list: the graph index comes from the winning pair
        pairs = [(9, 1), (0, 0), (8, 1), (3, 0), (10, 2), (1, 2), (5, 1), (3, 1), (0, 2)]
        a = al.assign(graphs, seqs, pairs=pairs)
        want = np.full(nq, -1)
        for q, g in pairs:
            if want[q] < 0 or m[q, g] < m[q, want[q]]:
                want[q] = g
        assert np.array_equal(a["graph"], want)
    with pytest.raises(ValueError):
        al.assign(graphs, seqs, max_score=[1, 2])


@pytest.mark.gpu
@pytest.mark.parametrize("two_piece", [False, True], ids=["one-piece", "two-piece"])
def test_best_python_assign_and_align(engine, oracle, two_piece):
    rng = np.random.default_rng(63)
    chains = [rng.choice(ACGT, n) for n in (20, 31, 38)]
    graphs = [_bubble_graph()] + [_chain(c) for c in chains]
    seqs = [W.random_walk_query(rng, graphs[0], 0.1), W.mutate(rng, chains[1], 0.1, 0.05, 0.05), W.mutate(rng, chains[0], 0.1, 0.05, 0.05),
            rng.choice(ACGT, 40), W.random_walk_query(rng, graphs[0], 0.2), W.mutate(rng, chains[2], 0.05, 0.02, 0.02), chains[1][:6]]
    costs = COSTS2 if two_piece else COSTS
    cfg = engine.Affine2PieceDijkstra(_costs(engine, costs)) if two_piece else engine.AffineMinGapCost(_costs(engine, costs))
    al = engine.PoastaAligner(cfg)
    ref = _oracle_scores(oracle, graphs, seqs, costs)
    best = ref.min(axis=1)
    limit = int(np.sort(best)[-2])   # the query with the highest best score stays unassigned
    assert (best > limit).sum() == 1
    want_graph = np.where(best <= limit, ref.argmin(axis=1), -1)
    a, res = al.assign_and_align(graphs, seqs, max_score=limit)
    assert np.array_equal(a["graph"], want_graph) and len(res) == len(seqs)
    # against align_multi of the hand-grouped winners
    groups = [[qi for qi in range(len(seqs)) if want_graph[qi] == gi] for gi in range(len(graphs))]
    hand = al.align_multi(graphs, [[seqs[qi] for qi in grp] for grp in groups])
    k = 0
    for grp in groups:
        for qi in grp:
            assert res.score[qi] == hand.score[k] == ref[qi, want_graph[qi]] and res.flags[qi] == hand.flags[k]
            assert res.raw_alignment(qi) == hand.raw_alignment(k)
            k += 1
    # against the oracle's alignments
    for qi, gi in enumerate(want_graph):
        if gi < 0:
            assert res.score[qi] == NONE and res.flags[qi] == 0 and res.raw_alignment(qi) == []
            continue
        og = oracle.OracleGraph.from_csr(graphs[gi].as_dict())
        qseq, qoff = pack_queries([seqs[qi]])
        if two_piece:
            m, e1, o1, e2, o2 = costs
            with oracle.two_piece(o2, e2):
                D = og.dense_batch(qseq, qoff, oracle.Costs(m, o1, e1), threads=1)
        else:
            D = og.dense_batch(qseq, qoff, oracle.Costs(*costs), threads=1)
        assert int(D["score"][0]) == res.score[qi] and oracle.batch_alignment(D, 0) == res.raw_alignment(qi), qi
    _, no_pairs = al.assign_and_align(graphs, seqs, max_score=limit, want_pairs=False)
    assert no_pairs.pairs is None and np.array_equal(no_pairs.score, res.score)
