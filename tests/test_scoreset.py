"""Score sets (poa_scoreset_*): score-only runs over (query, graph) pairs of many graphs.

Every score has two references: the oracle's dense restatement of that query on that graph, and the per-graph one-shot
score-mode call of the same library (poa_align_batch_ex / poa_align_batch_2piece_ex in POA_MODE_SCORE) on the same inputs,
which also gives the flags.  Equal, not close."""
import ctypes as C
import os

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7
EMPTY_GRAPH, SHORT_QUERY = 0x20, 0x08
ACGT = np.frombuffer(b"ACGT", np.uint8)
COSTS2 = [(4, 2, 6, 1, 24), (1, 2, 10, 1, 8), (3, 3, 12, 1, 6), (2, 2, 4, 2, 4), (4, 3, 5, 0, 9)]   # (m, e1, o1, e2, o2), tests/test_two_piece.py
WIDE_OPEN2 = (4, 255, 255, 0, 9)   # open' = open1 + extend1 - extend2 = 510 does not fit poa_costs_t

# A strip of the widest sweep variant is 64 lanes x PlaneIO<T>::K x Q columns: 64 x 8 x 2 (u16) or 64 x 4 x 4 (u32) = 1024.
# 600 symbols: pitch 640, one strip, the packed one-strip class on a u16 run.  1100 symbols: pitch 1152, two strips, carries.
MID, LONG = 600, 1100


# ---- the small graphs of tests/test_multi_graph.py (copied: that file stays as it is) --------------------------------------------
def _gfa_graph():
    b = GraphBuilder()
    ids, links = {}, []
    for line in open(os.path.join(ROOT, "tests", "golden", "test.gfa")):
        f = line.strip().split("\t")
        if f[0] == "S":
            ids[f[1]] = b.add_path(np.frombuffer(f[2].upper().encode(), np.uint8))
        elif f[0] == "L":
            links.append((f[1], f[3]))
    for a, c in links:
        b.add_edge(ids[a][-1], ids[c][0])
    return b.finish()


def _bubble_graph():
    """A backbone of 12 nodes; three branches of different lengths leave node 2 and join at node 8, which then has four
    predecessors; an edge from node 1 to node 10 skips the rows between them."""
    rng = np.random.default_rng(21)
    b = GraphBuilder()
    back = b.add_path(rng.choice(ACGT, 12))
    for length in (1, 2, 4):
        br = b.add_path(rng.choice(ACGT, length))
        b.add_edge(back[2], br[0])
        b.add_edge(br[-1], back[8])
    b.add_edge(back[1], back[10])
    g = b.finish()
    assert max(len(g.predecessors(v)) for v in range(g.n)) >= 3
    return g


def _chain(seq):
    b = GraphBuilder()
    b.add_path(seq)
    return b.finish()


_MIXED = None


def _mixed():
    """graphs (the bubble graph is listed twice: the same object, so the same handle) and the pool of queries: lengths 0, 1,
    2, about 30-48, 600 and 1100."""
    global _MIXED
    if _MIXED is None:
        rng = np.random.default_rng(20)
        chain_seq = rng.choice(ACGT, 20)
        chain, bubble, gfa, empty = _chain(chain_seq), _bubble_graph(), _gfa_graph(), GraphBuilder().finish()
        idle = _chain(rng.choice(ACGT, 9))
        graphs = [chain, bubble, gfa, empty, idle, bubble]
        long_q = np.concatenate([chain_seq[:10], rng.choice(ACGT, LONG - 20), chain_seq[10:]])
        mid_q = np.concatenate([chain_seq[:10], rng.choice(ACGT, MID - 20), chain_seq[10:]])
        seqs = [np.zeros(0, np.uint8), chain_seq[3:4], chain_seq[5:7], W.mutate(rng, np.concatenate([chain_seq, chain_seq[:10]]), 0.1, 0.05, 0.05),
                W.random_walk_query(rng, bubble, 0.2), W.random_walk_query(rng, gfa, 0.25), rng.choice(ACGT, 40), rng.choice(ACGT, 48),
                mid_q, long_q, rng.choice(ACGT, 1)]
        assert len(mid_q) == MID and len(long_q) == LONG and all(g.n <= 40 for g in graphs)
        _MIXED = (graphs, seqs)
    return _MIXED


def _costs(engine, m, o, e):
    return engine.GapAffine(m, e, o)   # reference ctor order: (mismatch, extend, open)


def _costs2(engine, m, e1, o1, e2, o2):
    return engine.GapAffine2Piece(m, e1, o1, e2, o2)


def _pitch(length):
    return ((length + 1 + 63) // 64) * 64


def _sweep(engine, g):
    """(n_slots, n_slotted, rows) of a graph, from the C ABI."""
    from poasta_amd import _lib
    dg = engine._device_graph(g)
    slot, n_slots = dg.sweep_slots()
    return int(n_slots), int((np.asarray(slot) != 0xFFFFFFFF).sum()), int(_lib.lib().poa_graph_rows(dg.handle))


def _term(engine, g, q):
    return 2 * max(_sweep(engine, g)[0], 1) * _pitch(len(q)) * 4 + 256


def _plane_bytes(engine, graphs, seqs, pairs, narrow, px):
    """The rule of run_sweep, pair by pair: kept rows x 2 planes x (2048 bytes in the packed kernel's layout, else pitch cells)."""
    total = 0
    for qi, gi in pairs:
        if graphs[gi].n == 2:
            continue   # no real nodes: the shortcut, nothing stored
        pitch = _pitch(len(seqs[qi]))
        packed = narrow and px and 512 < pitch <= 1024
        total += 2 * _sweep(engine, graphs[gi])[1] * (2048 if packed else pitch * (2 if narrow else 4))
    return total


def _matrix_pairs(nq, ng):
    return [(qi, gi) for qi in range(nq) for gi in range(ng)]


_REF = {}


def _oracle_matrix(oracle, key, graphs, seqs, costs, two_piece=None):
    """[n_queries, n_graphs] scores by the oracle's dense restatement, once per (case, costs)."""
    k = ("oracle", key, costs, two_piece)
    if k not in _REF:
        qseq, qoff = pack_queries(seqs)
        out = np.zeros((len(seqs), len(graphs)), np.uint32)
        for gi, g in enumerate(graphs):
            if g.n == 2:   # no real nodes: the aligner's shortcut (mod.rs:124-142), score 4 * len
                out[:, gi] = [4 * len(q) for q in seqs]
                continue
            og = oracle.OracleGraph.from_csr(g.as_dict())
            if two_piece is None:
                out[:, gi] = og.dense_batch(qseq, qoff, oracle.Costs(*costs), threads=4)["score"]
            else:
                with oracle.two_piece(*two_piece):
                    out[:, gi] = og.dense_batch(qseq, qoff, oracle.Costs(*costs), threads=4)["score"]
        out.setflags(write=False)
        _REF[k] = out
    return _REF[k]


def _one_shot_matrix(engine, key, graphs, seqs, costs, **tune):
    """[n_queries, n_graphs] (score, flags) by the one-shot score-mode call, graph by graph; costs of three are one-piece
    (m, o, e), of five two-piece (m, e1, o1, e2, o2)."""
    k = ("one-shot", key, costs, tuple(sorted(tune.items())))
    if k not in _REF:
        from poasta_amd import _lib
        L = _lib.lib()
        cfg = engine.make_config("score", **tune)
        qseq, qoff = pack_queries(seqs)
        n = len(seqs)
        score, flags = np.zeros((n, len(graphs)), np.uint32), np.zeros((n, len(graphs)), np.uint32)
        for gi, g in enumerate(graphs):
            dg = engine._device_graph(g)
            s, f, po = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
            if len(costs) == 3:
                c = _costs(engine, *costs)._c()
                _lib.check(L.poa_align_batch_ex(dg.handle, C.byref(c), C.byref(cfg), n, engine._p(qseq), engine._p(qoff), engine._p(s), None,
                                                engine._p(po), 0, engine._p(f), None, 0))
            else:
                c = _costs2(engine, *costs)._c()
                _lib.check(L.poa_align_batch_2piece_ex(dg.handle, C.byref(c), C.byref(cfg), n, engine._p(qseq), engine._p(qoff), engine._p(s),
                                                       None, engine._p(po), 0, engine._p(f), None, None, 0))
            score[:, gi], flags[:, gi] = s, f
        score.setflags(write=False)
        flags.setflags(write=False)
        _REF[k] = (score, flags)
    return _REF[k]


def _run(engine, graphs, seqs, costs, pairs=None, workspace_bytes=0, **tune):
    cfg = engine.make_config("score", **tune) if tune else None
    ss = engine.ScoreSet(graphs, seqs, pairs=pairs, workspace_bytes=workspace_bytes)
    ss.run(_costs(engine, *costs) if len(costs) == 3 else _costs2(engine, *costs), config=cfg)
    score, flags, st = ss.fetch()
    ws = ss.workspace_bytes()
    ss.close()
    return score, flags, st, ws


def _at(matrix, pairs):
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    return matrix[pr[:, 0], pr[:, 1]]


def _hip(engine):
    """The HIP runtime the engine itself is linked against (already mapped into this process)."""
    engine._lib.lib()
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in os.path.basename(path):
            hip = C.CDLL(path)
            hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipStreamDestroy.argtypes = [C.c_void_p]
            return hip
    pytest.fail("the engine's HIP runtime is not mapped")


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scoreset_full_matrix(engine, oracle):
    graphs, seqs = _mixed()
    nq, ng = len(seqs), len(graphs)
    pairs = _matrix_pairs(nq, ng)
    for costs in ((4, 6, 2), (1, 1, 1)):
        ref, (one, one_flags) = _oracle_matrix(oracle, "mixed", graphs, seqs, costs), _one_shot_matrix(engine, "mixed", graphs, seqs, costs)
        score, flags, st, ws = _run(engine, graphs, seqs, costs)
        assert np.array_equal(score.reshape(nq, ng), ref), ("vs the dense restatement", costs)
        assert np.array_equal(score.reshape(nq, ng), one) and np.array_equal(flags.reshape(nq, ng), one_flags), ("vs the one-shot call", costs)
        # one chunk; the statistics and the workspace are their formulas
        terms = [_term(engine, graphs[gi], seqs[qi]) for qi, gi in pairs]
        assert st["n_chunks"] == 1 and st["n_queries"] == nq * ng and ws == sum(terms)
        assert ws == engine.scoreset_footprint(graphs, seqs)[0]
        assert st["cells"] == sum(_sweep(engine, graphs[gi])[2] * (len(seqs[qi]) + 1) for qi, gi in pairs)
        assert st["plane_bytes"] == _plane_bytes(engine, graphs, seqs, pairs, True, True)
        assert st["ms_traceback"] == 0.0 and st["n_runs"] == 1
        # pairs against the graph without real nodes: the shortcut; one-symbol queries: SHORT_QUERY; nothing else
        f = flags.reshape(nq, ng)
        for qi, q in enumerate(seqs):
            for gi, g in enumerate(graphs):
                want = EMPTY_GRAPH if g.n == 2 else (SHORT_QUERY if len(q) == 1 else 0)
                assert f[qi, gi] == want, (qi, gi)
                if g.n == 2:
                    assert score.reshape(nq, ng)[qi, gi] == 4 * len(q)
        assert st["n_flagged"] == int((f != 0).sum())
        # the same handle listed twice: the same column
        assert np.array_equal(score.reshape(nq, ng)[:, 1], score.reshape(nq, ng)[:, 5])
        al = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, *costs)))
        m = al.score_matrix(graphs, seqs)
        assert m.shape == (nq, ng) and m.dtype == np.uint32 and np.array_equal(m, ref)
    # the graph id is used: some query scores differently on another graph than on the chain
    assert (ref[:, 0:1] != ref).any()


@pytest.mark.gpu
def test_scoreset_pair_list(engine, oracle):
    graphs, seqs = _mixed()
    costs = (4, 6, 2)
    ref, (one, one_flags) = _oracle_matrix(oracle, "mixed", graphs, seqs, costs), _one_shot_matrix(engine, "mixed", graphs, seqs, costs)
    # unsorted, with repeats; graph 4 and query 7 have no pair
    pairs = [(9, 2), (0, 0), (8, 1), (9, 2), (3, 5), (10, 3), (1, 2), (8, 0), (2, 1), (9, 0), (6, 3), (5, 2), (8, 1), (4, 5), (0, 3), (9, 5)]
    assert all(gi != 4 and qi != 7 for qi, gi in pairs) and len(set(pairs)) < len(pairs)
    score, flags, st, ws = _run(engine, graphs, seqs, costs, pairs=pairs)
    assert np.array_equal(score, _at(ref, pairs)) and np.array_equal(score, _at(one, pairs)) and np.array_equal(flags, _at(one_flags, pairs))
    assert st["n_queries"] == len(pairs) and ws == sum(_term(engine, graphs[gi], seqs[qi]) for qi, gi in pairs)
    assert st["cells"] == sum(_sweep(engine, graphs[gi])[2] * (len(seqs[qi]) + 1) for qi, gi in pairs)
    al = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, *costs)))
    s2, f2 = al.score_pairs(graphs, seqs, pairs)
    assert np.array_equal(s2, score) and np.array_equal(f2, flags)
    # no pairs at all
    score, flags, st, ws = _run(engine, graphs, seqs, costs, pairs=np.zeros((0, 2), np.int64))
    assert len(score) == 0 and len(flags) == 0 and st["n_queries"] == 0 and ws == 0


@pytest.mark.gpu
def test_scoreset_chunk_boundaries(engine, oracle):
    graphs, seqs = _mixed()
    costs = (4, 6, 2)
    nq, ng = len(seqs), len(graphs)
    ref, (one, one_flags) = _oracle_matrix(oracle, "mixed", graphs, seqs, costs), _one_shot_matrix(engine, "mixed", graphs, seqs, costs)
    terms = [_term(engine, graphs[gi], seqs[qi]) for qi, gi in _matrix_pairs(nq, ng)]
    total, largest = engine.scoreset_footprint(graphs, seqs)
    assert (total, largest) == (sum(terms), max(terms))

    def greedy(cap):
        chunks, used = [], 0
        for t in terms:
            if used and used + t > cap:
                chunks.append(used)
                used = 0
            used += t
        return chunks + [used]

    for cap in (largest + 256, 1, largest, total - 1):
        want = greedy(max(cap, largest))
        score, flags, st, ws = _run(engine, graphs, seqs, costs, workspace_bytes=cap)
        assert st["n_chunks"] == len(want) and ws == max(want), cap
        assert np.array_equal(score.reshape(nq, ng), ref) and np.array_equal(score.reshape(nq, ng), one), cap
        assert np.array_equal(flags.reshape(nq, ng), one_flags), cap
        if cap == largest + 256:
            assert len(want) >= 3
        if cap == 1:
            assert ws == largest


_EDGES = None


def _edges():
    """A chain of 40 nodes and the bubble graph (which keeps rows in slots), queries of exactly 511, 512, 1023 and 1024 symbols:
    pitches 512, 576, 1024 and 1088 — the last column of the one-strip general class, the first and the last pitch of the packed
    class, the first pitch of two strips."""
    global _EDGES
    if _EDGES is None:
        rng = np.random.default_rng(44)
        chain_seq = rng.choice(ACGT, 40)
        graphs = [_chain(chain_seq), _bubble_graph()]
        seqs = []
        for length in (511, 512, 1023, 1024):
            q = rng.choice(ACGT, length)
            q[:20], q[-20:] = chain_seq[:20], chain_seq[20:]
            seqs.append(q)
        assert [_pitch(len(q)) for q in seqs] == [512, 576, 1024, 1088]
        _EDGES = (graphs, seqs)
    return _EDGES


@pytest.mark.gpu
def test_scoreset_strip_and_class_edges(engine, oracle):
    graphs, seqs = _edges()
    costs = (4, 6, 2)
    nq, ng = len(seqs), len(graphs)
    pairs = _matrix_pairs(nq, ng)
    ref = _oracle_matrix(oracle, "edges", graphs, seqs, costs)
    assert _sweep(engine, graphs[1])[1] > 0
    for px in (None, 0):
        tune = {} if px is None else {"px": px}
        one, one_flags = _one_shot_matrix(engine, "edges", graphs, seqs, costs, **tune)
        score, flags, st, _ = _run(engine, graphs, seqs, costs, **tune)
        assert np.array_equal(score.reshape(nq, ng), ref) and np.array_equal(score.reshape(nq, ng), one), px
        assert np.array_equal(flags.reshape(nq, ng), one_flags) and not flags.any(), px
        # 2048 bytes per slot row only for the pairs of pitch in (512, 1024] on the default u16 run
        assert st["plane_bytes"] == _plane_bytes(engine, graphs, seqs, pairs, True, px is None), px
    assert _plane_bytes(engine, graphs, seqs, pairs, True, True) != _plane_bytes(engine, graphs, seqs, pairs, True, False)


@pytest.mark.gpu
def test_scoreset_cell_width(engine, oracle):
    graphs, seqs = _mixed()
    nq, ng = len(seqs), len(graphs)
    pairs = _matrix_pairs(nq, ng)
    # extend 60 x 1100 symbols is past 65534: every graph paired with the long query fails the bound, the run is u32
    dear = (255, 40, 60)
    assert dear[1] + dear[2] * LONG > 65534
    ref, (one, one_flags) = _oracle_matrix(oracle, "mixed", graphs, seqs, dear), _one_shot_matrix(engine, "mixed", graphs, seqs, dear)
    score, flags, st, _ = _run(engine, graphs, seqs, dear)
    assert np.array_equal(score.reshape(nq, ng), ref) and np.array_equal(score.reshape(nq, ng), one)
    assert np.array_equal(flags.reshape(nq, ng), one_flags)
    assert int(score.max()) > 65534
    assert st["plane_bytes"] == _plane_bytes(engine, graphs, seqs, pairs, False, True)
    # without the long query the same costs stay under the bound: u16
    short = [(qi, gi) for qi, gi in pairs if len(seqs[qi]) < MID]
    score, flags, st, _ = _run(engine, graphs, seqs, dear, pairs=short)
    assert np.array_equal(score, _at(ref, short)) and st["plane_bytes"] == _plane_bytes(engine, graphs, seqs, short, True, True)
    # u32 forced on the cheap costs: the same scores, twice the bytes for the pairs outside the packed class
    cheap = (4, 6, 2)
    ref = _oracle_matrix(oracle, "mixed", graphs, seqs, cheap)
    score, flags, st, _ = _run(engine, graphs, seqs, cheap, planes=32)
    assert np.array_equal(score.reshape(nq, ng), ref)
    assert np.array_equal(flags.reshape(nq, ng), _one_shot_matrix(engine, "mixed", graphs, seqs, cheap)[1])
    assert st["plane_bytes"] == _plane_bytes(engine, graphs, seqs, pairs, False, True) == 2 * _plane_bytes(engine, graphs, seqs, pairs, True, False)


@pytest.mark.gpu
def test_scoreset_two_piece(engine, oracle):
    graphs, seqs = _mixed()
    nq, ng = len(seqs), len(graphs)
    for c2 in COSTS2 + [WIDE_OPEN2]:
        m, e1, o1, e2, o2 = c2
        ref = _oracle_matrix(oracle, "mixed", graphs, seqs, (m, o1, e1), two_piece=(o2, e2))
        one, one_flags = _one_shot_matrix(engine, "mixed", graphs, seqs, c2)
        score, flags, st, _ = _run(engine, graphs, seqs, c2)
        assert np.array_equal(score.reshape(nq, ng), ref), ("vs the dense restatement", c2)
        assert np.array_equal(score.reshape(nq, ng), one) and np.array_equal(flags.reshape(nq, ng), one_flags), ("vs the one-shot call", c2)
        # the scores poa_align_batch_2piece returns, graph by graph
        al = engine.PoastaAligner(engine.Affine2PieceDijkstra(_costs2(engine, *c2)))
        filled = [qi for qi, q in enumerate(seqs) if len(q) >= 1]
        for gi, g in enumerate(graphs[:4]):
            dense = al.align_batch(g, [seqs[qi] for qi in filled], want_pairs=False).score
            assert np.array_equal(dense, score.reshape(nq, ng)[filled, gi]), (c2, gi)
        assert np.array_equal(al.score_matrix(graphs, seqs), ref), c2
    # one-piece and two-piece runs alternate on one set, on a stream of the caller's; each equals a fresh set's
    hip = _hip(engine)
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    ss = engine.ScoreSet(graphs, seqs)
    for costs in ((4, 6, 2), COSTS2[0], (1, 1, 1), WIDE_OPEN2, (255, 40, 60), COSTS2[3]):
        ss.run(_costs(engine, *costs) if len(costs) == 3 else _costs2(engine, *costs), stream=stream.value)
        score, flags, st = ss.fetch()
        fresh = _run(engine, graphs, seqs, costs)
        assert np.array_equal(score, fresh[0]) and np.array_equal(flags, fresh[1]) and st["plane_bytes"] == fresh[2]["plane_bytes"], costs
        assert np.array_equal(score.reshape(nq, ng), _one_shot_matrix(engine, "mixed", graphs, seqs, costs)[0]), costs
    ss.close()
    assert hip.hipStreamDestroy(stream) == 0


@pytest.mark.gpu
def test_scoreset_random_sweep(engine, oracle):
    rng = np.random.default_rng(7)
    graphs, seqs, pairs, own = [], [], [], []
    for seed in range(40):
        alpha = b"AC" if seed % 2 else b"ACGT"
        g = W.random_dag(300 + seed, n_nodes=int(rng.integers(3, 31)), p_edge=0.3, alphabet=alpha)
        graphs.append(g)
        for _ in range(int(rng.integers(1, 9))):
            seqs.append(W.random_walk_query(rng, g, 0.3, alpha))
            own.append(seed)
    for qi, gi in enumerate(own):
        others = rng.choice([k for k in range(40) if k != gi], 3, replace=False)
        pairs += [(qi, gi)] + [(qi, int(k)) for k in others]
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    for costs in ((4, 6, 2), (1, 1, 1)):
        ref, (one, one_flags) = _oracle_matrix(oracle, "random", graphs, seqs, costs), _one_shot_matrix(engine, "random", graphs, seqs, costs)
        score, flags, st, _ = _run(engine, graphs, seqs, costs, pairs=pairs)
        assert np.array_equal(score, _at(ref, pairs)) and np.array_equal(score, _at(one, pairs)), costs
        assert np.array_equal(flags, _at(one_flags, pairs)), costs
        # the graph id is really used: some pair scores differently from its query on its own graph
        own_score = np.array([ref[qi, own[qi]] for qi, _ in pairs])
        assert (score != own_score).any(), costs


@pytest.mark.gpu
def test_scoreset_contract(engine, oracle):
    from poasta_amd import _lib
    L = _lib.lib()
    graphs, seqs = _mixed()
    nq, ng = len(seqs), len(graphs)
    costs = (4, 6, 2)
    ref = _oracle_matrix(oracle, "mixed", graphs, seqs, costs)
    dgs = [engine._device_graph(g) for g in graphs]
    handles = (C.c_void_p * ng)(*[d.handle for d in dgs])
    qseq, qoff = pack_queries(seqs)
    pq, pg = np.array([9, 0, 8, 3], np.uint32), np.array([2, 3, 1, 5], np.uint32)
    c, c2 = _costs(engine, *costs)._c(), _lib.PoaCosts2(4, 6, 2, 24, 1, 0)
    p = engine._p
    score, flags = np.zeros(nq * ng, np.uint32), np.zeros(nq * ng, np.uint32)
    byref = lambda cfg: C.byref(cfg) if cfg is not None else None

    def create(hs=handles, off=qoff, n=4, q=pq, g=pg, cfg=None):
        h = C.c_void_p()
        rc = L.poa_scoreset_create(hs, ng, 0, nq, p(qseq), p(off), n, p(q), p(g), byref(cfg), 0, C.byref(h))
        if rc == 0:
            L.poa_scoreset_destroy(h)
        return rc

    def one_shot(hs=handles, off=qoff, n=4, q=pq, g=pg, cfg=None):
        return L.poa_score_pairs(hs, ng, C.byref(c), byref(cfg), nq, p(qseq), p(off), n, p(q), p(g), p(score), p(flags), None, 0)

    def one_shot2(hs=handles, off=qoff, n=4, q=pq, g=pg, cfg=None):
        return L.poa_score_pairs_2piece(hs, ng, C.byref(c2), byref(cfg), nq, p(qseq), p(off), n, p(q), p(g), p(score), p(flags), None, 0)

    hole = (C.c_void_p * ng)(*[d.handle for d in dgs])
    hole[2] = None
    bad_q, bad_g = pq.copy(), pg.copy()
    bad_q[1], bad_g[3] = nq, ng
    for call in (create, one_shot, one_shot2):
        assert call() == 0, call.__name__
        for what, kw in (("null graph", dict(hs=hole)), ("query out of range", dict(q=bad_q)), ("graph out of range", dict(g=bad_g)),
                         ("null qoff", dict(off=None)), ("one pair array null", dict(g=None)), ("matrix count", dict(n=nq * ng - 1, q=None, g=None))):
            assert call(**kw) == ERR_INVALID_ARG and L.poa_last_error() != b"", (what, call.__name__)
        for mode in ("dense", "exact", "hybrid", "checkpoint", "checkpoint2"):
            assert call(cfg=engine.make_config(mode)) == ERR_UNSUPPORTED and L.poa_last_error() != b"", (mode, call.__name__)
        assert call(cfg=engine.make_config("score", aln_type=engine.AlignmentType.EndsFree())) == ERR_UNSUPPORTED
        assert call(n=0) == 0 and call(n=0, q=None, g=None) == 0
    assert one_shot() == 0 and np.array_equal(score[:4], ref[pq, pg]) and not flags[0] and flags[1] == EMPTY_GRAPH
    bad2 = _lib.PoaCosts2(4, 6, 1, 24, 2, 0)
    assert L.poa_score_pairs_2piece(handles, ng, C.byref(bad2), None, nq, p(qseq), p(qoff), 4, p(pq), p(pg), p(score), p(flags), None, 0) == ERR_INVALID_ARG

    # a resident set: refusals on run and fetch, then it still works
    ss = engine.ScoreSet(graphs, seqs)
    st = _lib.PoaStats()
    assert L.poa_scoreset_fetch(ss.handle, p(score), p(flags), C.byref(st)) == ERR_INVALID_ARG and b"has not been called" in L.poa_last_error()
    for mode in ("dense", "exact", "hybrid", "checkpoint", "checkpoint2"):
        cfg = engine.make_config(mode)
        assert L.poa_scoreset_run(ss.handle, C.byref(c), C.byref(cfg), None) == ERR_UNSUPPORTED, mode
        assert L.poa_scoreset_run_2piece(ss.handle, C.byref(c2), C.byref(cfg), None) == ERR_UNSUPPORTED, mode
    ef = engine.make_config("score", aln_type=engine.AlignmentType.EndsFree())
    assert L.poa_scoreset_run(ss.handle, C.byref(c), C.byref(ef), None) == ERR_UNSUPPORTED
    assert L.poa_scoreset_run_2piece(ss.handle, C.byref(bad2), None, None) == ERR_INVALID_ARG and b"gap_extend1" in L.poa_last_error()
    assert L.poa_scoreset_run(ss.handle, None, None, None) == ERR_INVALID_ARG
    assert L.poa_scoreset_fetch(ss.handle, p(score), p(flags), C.byref(st)) == ERR_INVALID_ARG   # still no run
    assert L.poa_scoreset_run(ss.handle, C.byref(c), None, None) == 0   # cfg NULL is score mode
    assert L.poa_scoreset_fetch(ss.handle, p(score), None, None) == 0   # flags and stats may be NULL
    assert np.array_equal(score.reshape(nq, ng), ref)
    ptrs = ss.device_results()
    assert ptrs["score"] and ptrs["flags"]
    assert ss.stats()["n_runs"] == 1
    ss.run(_costs(engine, *costs))
    s, f, st2 = ss.fetch()
    assert np.array_equal(s.reshape(nq, ng), ref) and st2["n_runs"] == 1
    ss.close()
    ss.close()
    # the binding refuses a pair out of range before the call
    with pytest.raises(ValueError):
        engine.ScoreSet(graphs, seqs, pairs=[(0, ng)])
