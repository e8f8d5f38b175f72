"""Capped score-set runs (poa_scoreset_run_capped / _run_2piece_capped, poa_scoreset_fetch_swept).

The contract, with s the oracle's score of the pair: s <= cap gives (s, the uncapped flags), s > cap gives (POA_SCORE_UNVISITED,
the uncapped flags | POA_FLAG_CAPPED) — wherever the wave stopped, if it stopped.  Where it stops is checked separately, against
the oracle's M plane: after the first check row whose smallest M value over columns 0..len is above the cap."""
import ctypes as C

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

ERR_INVALID_ARG = -1
NONE = 0xFFFFFFFF
EMPTY_GRAPH, SHORT_QUERY, CAPPED = 0x20, 0x08, 0x80
ACGT = np.frombuffer(b"ACGT", np.uint8)
COSTS = (4, 6, 2)              # (m, o, e)
COSTS2 = (4, 2, 6, 1, 24)      # (m, e1, o1, e2, o2): 4 / 6,24 / 2,1
KINDS = 5                      # caps around s: 0, s - 1, s, s + 1, none


def _chain(seq):
    b = GraphBuilder()
    b.add_path(seq)
    return b.finish()


def _bubble_graph():
    """tests/test_scoreset.py: a backbone of 12 nodes, three branches from node 2 to node 8, an edge from node 1 to node 10."""
    rng = np.random.default_rng(21)
    b = GraphBuilder()
    back = b.add_path(rng.choice(ACGT, 12))
    for length in (1, 2, 4):
        br = b.add_path(rng.choice(ACGT, length))
        b.add_edge(back[2], br[0])
        b.add_edge(br[-1], back[8])
    b.add_edge(back[1], back[10])
    return b.finish()


def _costs(engine, costs):
    return engine.GapAffine(costs[0], costs[2], costs[1]) if len(costs) == 3 else engine.GapAffine2Piece(*costs)


def _oracle_scores(oracle, graphs, seqs, costs):
    """[n_queries, n_graphs] by the oracle's dense restatement (tests/test_scoreset.py: _oracle_matrix)."""
    qseq, qoff = pack_queries(seqs)
    out = np.zeros((len(seqs), len(graphs)), np.uint32)
    for gi, g in enumerate(graphs):
        if g.n == 2:
            out[:, gi] = [4 * len(q) for q in seqs]
            continue
        og = oracle.OracleGraph.from_csr(g.as_dict())
        if len(costs) == 3:
            out[:, gi] = og.dense_batch(qseq, qoff, oracle.Costs(*costs), threads=4)["score"]
        else:
            m, e1, o1, e2, o2 = costs
            with oracle.two_piece(o2, e2):
                out[:, gi] = og.dense_batch(qseq, qoff, oracle.Costs(m, o1, e1), threads=4)["score"]
    out.setflags(write=False)
    return out


def _caps_around(s, shift):
    """cap of pair p: kind (p + shift) % 5 of {0, s - 1, s, s + 1, none}; over five shifts every pair meets every kind."""
    s = s.astype(np.int64)
    kind = (np.arange(len(s)) + shift) % KINDS
    cap = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0 * s, np.maximum(s - 1, 0), s, s + 1], NONE)
    return cap.astype(np.uint32)


def _expect(s, flags0, cap):
    over = s.astype(np.int64) > cap.astype(np.int64)
    return np.where(over, NONE, s).astype(np.uint32), np.where(over, flags0 | CAPPED, flags0).astype(np.uint32)


def _run(ss, engine, costs, cap=None, **tune):
    ss.run(_costs(engine, costs), config=engine.make_config("score", **tune) if tune else None, cap=cap)
    score, flags, _ = ss.fetch()
    return score, flags


_SMALL = {}


def _small(oracle):
    """Three small graphs — a chain, the bubble graph, one without real nodes — and queries of every kernel class: 0, 1, 2 symbols,
    about 40 and 300 (general kernel), 600 and 1023 (packed kernel on a u16 run), 1100 (two strips)."""
    if not _SMALL:
        rng = np.random.default_rng(50)
        chain_seq = rng.choice(ACGT, 20)
        graphs = [_chain(chain_seq), _bubble_graph(), GraphBuilder().finish()]

        def ends(length):   # a long query that begins and ends like the chain
            return np.concatenate([chain_seq[:10], rng.choice(ACGT, length - 20), chain_seq[10:]])

        seqs = [np.zeros(0, np.uint8), chain_seq[3:4], chain_seq[5:7], W.mutate(rng, np.concatenate([chain_seq, chain_seq]), 0.1, 0.05, 0.05),
                W.random_walk_query(rng, graphs[1], 0.2), rng.choice(ACGT, 40), ends(600), ends(1023), rng.choice(ACGT, 600), ends(1100),
                rng.choice(ACGT, 1100), ends(300)]   # (300: the general kernel at Q = 2 on a u32 run)
        assert [len(q) for q in seqs][:3] == [0, 1, 2] and 30 <= len(seqs[3]) <= 50
        _SMALL.update(graphs=graphs, seqs=seqs, ref=_oracle_scores(oracle, graphs, seqs, COSTS), ref2=_oracle_scores(oracle, graphs, seqs, COSTS2))
    return _SMALL


# ---- the contract, every kernel class ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("costs", [COSTS, COSTS2], ids=["one-piece", "two-piece"])
def test_cap_contract_every_kernel_class(engine, oracle, costs):
    d = _small(oracle)
    graphs, seqs = d["graphs"], d["seqs"]
    s = (d["ref"] if costs is COSTS else d["ref2"]).reshape(-1)
    ss = engine.ScoreSet(graphs, seqs)
    score0, flags0 = _run(ss, engine, costs)
    assert np.array_equal(score0, s)
    want_flags = np.array([EMPTY_GRAPH if g.n == 2 else (SHORT_QUERY if len(q) == 1 else 0) for q in seqs for g in graphs], np.uint32)
    assert np.array_equal(flags0, want_flags)
    rows = np.array([0 if g.n == 2 else g.n * (2 if len(q) + 1 > 1024 else 1) for q in seqs for g in graphs], np.uint32)
    assert np.array_equal(ss.swept_rows(), rows)   # after an uncapped run: the full counts
    none = np.full(len(s), NONE, np.uint32)
    seen_capped = 0
    for tune in ({}, {"planes": 32}):          # u16 run (general and packed kernels), u32 run (general kernel at Q = 1, 2, 4)
        for stride in (1, 0):
            t = dict(tune, cap_stride=stride) if stride else dict(tune)
            # no cap at all: the uncapped run, bit for bit, and nothing stops
            score, flags = _run(ss, engine, costs, cap=none, **t)
            assert np.array_equal(score, score0) and np.array_equal(flags, flags0), (tune, stride)
            assert np.array_equal(ss.swept_rows(), rows), (tune, stride)
            for shift in range(KINDS):
                cap = _caps_around(s, shift)
                score, flags = _run(ss, engine, costs, cap=cap, **t)
                want_s, want_f = _expect(s, flags0, cap)
                bad = np.flatnonzero((score != want_s) | (flags != want_f))
                assert len(bad) == 0, (tune, stride, shift, [(int(p), int(p) // len(graphs), int(p) % len(graphs), int(cap[p]), int(s[p]),
                                                              int(score[p]), int(flags[p])) for p in bad[:5]])
                swept = ss.swept_rows()
                assert (swept <= rows).all() and (swept[(want_f & CAPPED) == 0] == rows[(want_f & CAPPED) == 0]).all(), (tune, stride, shift)
                seen_capped += int(((flags & CAPPED) != 0).sum())
    assert seen_capped > 0
    # a scalar cap, through the binding
    score, flags = _run(ss, engine, costs, cap=int(np.median(s)))
    want_s, want_f = _expect(s, flags0, np.full(len(s), int(np.median(s)), np.uint32))
    assert np.array_equal(score, want_s) and np.array_equal(flags, want_f)
    ss.close()


# ---- where the wave stops ---------------------------------------------------------------------------------------------------
def _m_rows(oracle, engine, g, q, costs):
    """The oracle's M plane of q on g, by engine row (the plane poa_batch_fetch_planes is tested against)."""
    og = oracle.OracleGraph.from_csr(g.as_dict())
    orank = og.export_csr()["rank"]
    node_of_row = np.argsort(engine._device_graph(g).node_rows())
    od = og.dense_align(np.ascontiguousarray(q, np.uint8), oracle.Costs(*costs), planes=True)
    return np.ascontiguousarray(od["M"][orank])[node_of_row], od["score"]


def _expected_swept(engine, g, m_plane, cap, stride):
    """r + 1 for the first check row r whose smallest M value over columns 0..len is above the cap, else rows."""
    row_min = m_plane.min(axis=1).astype(np.int64)
    for r in np.flatnonzero(engine.sweep_checks(g, stride)):
        if row_min[r] > cap:
            return int(r) + 1
    return g.n


@pytest.mark.gpu
def test_cap_where_the_wave_stops(engine, oracle):
    rng = np.random.default_rng(51)
    chain_seq = rng.choice(ACGT, 40)
    graphs = [_chain(chain_seq), _bubble_graph()]
    related = W.mutate(rng, chain_seq, 0.1, 0.05, 0.05)
    walk = W.random_walk_query(rng, graphs[1], 0.2)

    def ends(length):
        q = rng.choice(ACGT, length)
        q[:20], q[-20:] = chain_seq[:20], chain_seq[20:]
        return q

    # general kernel: 63 symbols fill the pitch exactly (no padding column), the others leave some; packed kernel: 639 symbols
    # fill a pitch of 640, 1023 the whole strip, 700 leaves padding in both halves
    seqs = [related, walk, rng.choice(ACGT, 63), rng.choice(ACGT, 40), chain_seq[:7], ends(639), ends(1023), rng.choice(ACGT, 639), rng.choice(ACGT, 700)]
    nq, ng = len(seqs), len(graphs)
    planes = [[_m_rows(oracle, engine, g, q, COSTS) for g in graphs] for q in seqs]
    s = np.array([[planes[qi][gi][1] for gi in range(ng)] for qi in range(nq)], np.int64).reshape(-1)
    ss = engine.ScoreSet(graphs, seqs)
    early = late = never = 0
    for name, cap in (("0", 0 * s), ("s - 1", np.maximum(s - 1, 0)), ("s", s), ("s / 2", s // 2)):
        score, flags = _run(ss, engine, COSTS, cap=cap.astype(np.uint32), cap_stride=1)
        swept = ss.swept_rows()
        for qi in range(nq):
            for gi, g in enumerate(graphs):
                p = qi * ng + gi
                want = _expected_swept(engine, g, planes[qi][gi][0], int(cap[p]), 1)
                print("cap %s query %d (len %d) graph %d: swept %d, expected %d of %d rows" % (name, qi, len(seqs[qi]), gi, swept[p], want, g.n))
                assert swept[p] == want, (name, qi, gi)
                assert (score[p] == NONE) == (s[p] > cap[p]) and (want == g.n or s[p] > cap[p])
                early += want <= g.n // 4
                late += g.n // 2 < want < g.n
                never += want == g.n
    assert early > 0 and late > 0 and never > 0, (early, late, never)
    # the default stride stops at its own check rows: never before stride 1 does
    cap = (s // 2).astype(np.uint32)
    _run(ss, engine, COSTS, cap=cap)
    swept = ss.swept_rows()
    for qi in range(nq):
        for gi, g in enumerate(graphs):
            assert swept[qi * ng + gi] == _expected_swept(engine, g, planes[qi][gi][0], int(cap[qi * ng + gi]), 0), (qi, gi)
    ss.close()


@pytest.mark.gpu
def test_cap_two_strips_stop_at_the_strip_end(engine, oracle):
    """A pair wider than 1024 columns tests M of the strip's last column at the end of every strip but the last."""
    rng = np.random.default_rng(52)
    chain_seq = rng.choice(ACGT, 40)
    g = _chain(chain_seq)
    q = rng.choice(ACGT, 1100)
    m_plane, s = _m_rows(oracle, engine, g, q, COSTS)
    col_min = int(m_plane[:, 1023].min())
    assert 0 < col_min <= s
    ss = engine.ScoreSet([g], [q])
    for cap, want_swept in ((col_min - 1, g.n), (col_min, 2 * g.n), (s - 1, 2 * g.n), (s, 2 * g.n)):
        score, flags = _run(ss, engine, COSTS, cap=cap, cap_stride=1)
        assert score[0] == (NONE if s > cap else s) and flags[0] == (CAPPED if s > cap else 0), cap
        assert ss.swept_rows()[0] == want_swept, cap
    ss.close()


# ---- exit soundness, random -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cap_random_exits_are_sound(engine, oracle):
    rng = np.random.default_rng(53)
    graphs, seqs, pairs = [], [], []
    for seed in range(40):
        alpha = b"AC" if seed % 2 else b"ACGT"
        g = W.random_dag(700 + seed, n_nodes=int(rng.integers(3, 31)), p_edge=float(rng.choice([0.05, 0.15, 0.3])), alphabet=alpha)
        graphs.append(g)
        for _ in range(2):
            seqs.append(W.random_walk_query(rng, g, 0.3, alpha))
            qi = len(seqs) - 1
            pairs += [(qi, seed)] + [(qi, int(k)) for k in rng.choice([k for k in range(40) if k != seed], 3, replace=False)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    assert 300 <= len(pairs) <= 340
    planes = [_m_rows(oracle, engine, graphs[gi], seqs[qi], COSTS) for qi, gi in pairs]
    s = np.array([pl[1] for pl in planes], np.int64)
    cap = rng.integers(0, 2 * s + 1)   # uniform in [0, 2 s]
    rows = np.array([graphs[gi].n for _, gi in pairs])
    ss = engine.ScoreSet(graphs, seqs, pairs=pairs)
    _, flags0 = _run(ss, engine, COSTS)
    score, flags = _run(ss, engine, COSTS, cap=cap.astype(np.uint32), cap_stride=1)
    swept = ss.swept_rows()
    want_s, want_f = _expect(s.astype(np.uint32), flags0, cap.astype(np.uint32))
    assert np.array_equal(score, want_s) and np.array_equal(flags, want_f)
    assert (s[swept < rows] > cap[swept < rows]).all()
    want_swept = np.array([_expected_swept(engine, graphs[gi], planes[i][0], int(cap[i]), 1) for i, (_, gi) in enumerate(pairs)])
    assert np.array_equal(swept, want_swept)
    assert (swept < rows).any() and (want_s != NONE).any()
    ss.close()


# ---- alternation and errors -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cap_alternation_and_errors(engine, oracle):
    from poasta_amd import _lib
    L = _lib.lib()
    d = _small(oracle)
    graphs, seqs = d["graphs"], d["seqs"]
    s1, s2 = d["ref"].reshape(-1), d["ref2"].reshape(-1)
    n = len(s1)
    p = engine._p
    c, c2 = _costs(engine, COSTS)._c(), _costs(engine, COSTS2)._c()
    ss = engine.ScoreSet(graphs, seqs)
    swept, cap = np.zeros(n, np.uint32), np.full(n, 10, np.uint32)
    # before any run
    assert L.poa_scoreset_fetch_swept(ss.handle, p(swept)) == ERR_INVALID_ARG and b"has not been called" in L.poa_last_error()
    assert L.poa_scoreset_run_capped(ss.handle, C.byref(c), None, None, None) == ERR_INVALID_ARG and L.poa_last_error() != b""
    assert L.poa_scoreset_run_2piece_capped(ss.handle, C.byref(c2), None, None, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_run_capped(ss.handle, None, None, p(cap), None) == ERR_INVALID_ARG
    assert L.poa_scoreset_run_capped(None, C.byref(c), None, p(cap), None) == ERR_INVALID_ARG
    bad2 = _lib.PoaCosts2(4, 6, 1, 24, 2, 0)
    assert L.poa_scoreset_run_2piece_capped(ss.handle, C.byref(bad2), None, p(cap), None) == ERR_INVALID_ARG
    dense = engine.make_config("dense")
    assert L.poa_scoreset_run_capped(ss.handle, C.byref(c), C.byref(dense), p(cap), None) == -7
    assert L.poa_scoreset_fetch_swept(ss.handle, p(swept)) == ERR_INVALID_ARG   # the refused calls were no runs
    assert L.poa_scoreset_fetch_swept(ss.handle, None) == ERR_INVALID_ARG
    # capped, uncapped and two-piece capped in turn on the one set
    _, f1 = _run(engine.ScoreSet(graphs, seqs), engine, COSTS)
    for turn in range(2):
        cap1 = _caps_around(s1, turn)
        score, flags = _run(ss, engine, COSTS, cap=cap1)
        want = _expect(s1, f1, cap1)
        assert np.array_equal(score, want[0]) and np.array_equal(flags, want[1]), turn
        score, flags = _run(ss, engine, COSTS)
        assert np.array_equal(score, s1) and np.array_equal(flags, f1), turn
        cap2 = _caps_around(s2, turn + 2)
        score, flags = _run(ss, engine, COSTS2, cap=cap2)
        want = _expect(s2, f1, cap2)
        assert np.array_equal(score, want[0]) and np.array_equal(flags, want[1]), turn
        score, flags = _run(ss, engine, COSTS2)
        assert np.array_equal(score, s2) and np.array_equal(flags, f1), turn
        # a refused call in between leaves the set as it was
        assert L.poa_scoreset_run_capped(ss.handle, C.byref(c), None, None, None) == ERR_INVALID_ARG
        assert L.poa_scoreset_fetch_swept(ss.handle, p(swept)) == 0
    ss.close()
    # a set without pairs
    empty = engine.ScoreSet(graphs, seqs, pairs=np.zeros((0, 2), np.int64))
    score, flags = _run(empty, engine, COSTS, cap=5)
    assert len(score) == 0 and len(empty.swept_rows()) == 0
    empty.close()
    with pytest.raises(ValueError):
        engine.ScoreSet(graphs, seqs).run(_costs(engine, COSTS), cap=[1, 2, 3])


# ---- Python -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cap_python_max_score(engine, oracle):
    d = _small(oracle)
    graphs, seqs = d["graphs"], d["seqs"]
    nq, ng = len(seqs), len(graphs)
    for costs, ref in ((COSTS, d["ref"]), (COSTS2, d["ref2"])):
        cfg = engine.AffineMinGapCost(_costs(engine, costs)) if len(costs) == 3 else engine.Affine2PieceDijkstra(_costs(engine, costs))
        al = engine.PoastaAligner(cfg)
        plain = al.score_matrix(graphs, seqs)
        assert np.array_equal(plain, ref) and np.array_equal(al.score_matrix(graphs, seqs, max_score=None), plain)
        # per query: its best graph's score, so the winners stay and most losers go
        best = ref.min(axis=1)
        m = al.score_matrix(graphs, seqs, max_score=best)
        assert m.shape == (nq, ng) and m.dtype == np.uint32
        assert np.array_equal(m, np.where(ref <= best[:, None], ref, NONE)) and (m == NONE).any()
        limit = int(np.median(ref))
        assert np.array_equal(al.score_matrix(graphs, seqs, max_score=limit), np.where(ref <= limit, ref, NONE))
        pairs = [(9, 1), (0, 0), (8, 1), (3, 0), (10, 2), (1, 2), (5, 1), (3, 0)]
        s0, f0 = al.score_pairs(graphs, seqs, pairs)
        s_none, f_none = al.score_pairs(graphs, seqs, pairs, max_score=None)
        assert np.array_equal(s0, s_none) and np.array_equal(f0, f_none)
        caps = _caps_around(s0, 1)
        sc, fl = al.score_pairs(graphs, seqs, pairs, max_score=caps)
        want = _expect(s0, f0, caps)
        assert np.array_equal(sc, want[0]) and np.array_equal(fl, want[1])
        sc, fl = al.score_pairs(graphs, seqs, pairs, max_score=limit)
        want = _expect(s0, f0, np.full(len(pairs), limit, np.uint32))
        assert np.array_equal(sc, want[0]) and np.array_equal(fl, want[1])
    with pytest.raises(ValueError):
        al.score_matrix(graphs, seqs, max_score=[1, 2])
