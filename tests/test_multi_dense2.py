"""Dense two-piece multi-graph batches (poa_multi_*_dense_2piece): the queries of many graphs through the dense two-piece pass in
one forward launch (a wavefront per query) and one walk launch (a lane per query) per chunk.

Every comparison demands equality with three references: the oracle's two-piece dense restatement and walk of every query
against its own graph; poa_align_batch_2piece graph by graph; poa_multi_run_2piece (the checkpointed batch) on the same inputs.

Costs are written in GapAffine2Piece's order: (mismatch, extend1, open1, extend2, open2)."""
import ctypes as C

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

import test_multi_graph_2piece as T2
from test_multi_graph import EMPTY_GRAPH, ERR_INVALID_ARG, ERR_UNSUPPORTED, _hip

COSTS = T2.COSTS                  # (4, 2, 6, 1, 24): -g 6,24 -e 2,1
COSTS_EQ = (3, 2, 4, 2, 9)        # extend1 == extend2
COSTS_U32 = (255, 60, 40, 3, 200) # open1 + extend1 x 1100 > 65534: the u16 rule fails for the 40-row graph of the mixed batch
ACGT = np.frombuffer(b"ACGT", np.uint8)
INF = 0xFFFFFFFF
PASS_EDGES = (511, 512, 1023, 1024, 1100)   # the 512-column pass edge, the edge of the two passes kept in registers, the loop path


def _pitch(length):
    return ((length + 1 + 63) // 64) * 64


def _terms(graphs, seqs):
    """Per query (graph index, bytes): 2 x 5 x rows x pitch + 256, the formula of include/poasta_amd_multi_dense2.h."""
    return [(gi, 10 * g.n * _pitch(len(q)) + 256) for gi, (g, qs) in enumerate(zip(graphs, seqs)) for q in qs]


def _forty_rows():
    """A backbone of 28 nodes; two branches leave node 2 and join at node 12, which then has three predecessors that are not the
    row above it; an edge from node 1 to node 20 skips the rows between them.  39 rows with the two sentinels.
    Returns the graph and the backbone's symbols."""
    rng = np.random.default_rng(31)
    b = GraphBuilder()
    back_seq = rng.choice(ACGT, 28)
    back = b.add_path(back_seq)
    for length in (3, 6):
        br = b.add_path(rng.choice(ACGT, length))
        b.add_edge(back[2], br[0])
        b.add_edge(br[-1], back[12])
    b.add_edge(back[1], back[20])
    g = b.finish()
    assert 36 <= g.n <= 42 and max(len(g.predecessors(v)) for v in range(g.n)) == 3
    return g, back_seq


_MIXED = None


def _mixed():
    """chain of 6 nodes; the 40-row graph; a graph without real nodes; the 40-row handle again; a graph without queries."""
    global _MIXED
    if _MIXED is None:
        rng = np.random.default_rng(32)
        b = GraphBuilder()
        chain_seq = rng.choice(ACGT, 6)
        b.add_path(chain_seq)
        chain = b.finish()
        (forty, back), empty = _forty_rows(), GraphBuilder().finish()
        b = GraphBuilder()
        b.add_path(rng.choice(ACGT, 9))
        idle = b.finish()

        def long_read(n):   # the backbone, random bases, the backbone's tail: aligned ends, a long insertion between them
            return np.concatenate([back[:14], rng.choice(ACGT, n - 28), back[14:]])
        graphs = [chain, forty, empty, forty, idle]
        seqs = [[np.zeros(0, np.uint8), chain_seq[2:3], chain_seq[1:3], rng.choice(ACGT, 63), np.concatenate([chain_seq, rng.choice(ACGT, 58)])],
                [long_read(n) for n in PASS_EDGES],
                [rng.choice(ACGT, 4), np.zeros(0, np.uint8), rng.choice(ACGT, 1)],
                [W.random_walk_query(rng, forty, 0.2) for _ in range(3)] + [np.zeros(0, np.uint8), rng.choice(ACGT, 40)],
                []]
        assert [len(q) for q in seqs[0]] == [0, 1, 2, 63, 64] and [len(q) for q in seqs[1]] == list(PASS_EDGES)
        _MIXED = (graphs, seqs)
    return _MIXED


_PER_GRAPH = {}


def _per_graph(engine, key, graphs, seqs, costs):
    """poa_align_batch_2piece, graph by graph: (score, flags, per-query pair counts, pairs) concatenated."""
    k = (key, costs)
    if k not in _PER_GRAPH:
        from poasta_amd import _lib
        c = T2._gc2(engine, costs)._c()
        score, flags, counts, pairs = [], [], [], []
        for g, qs in zip(graphs, seqs):
            if not qs:
                continue
            dg = engine._device_graph(g)
            qseq, qoff = pack_queries(qs)
            n = len(qs)
            cap = int(qoff[-1]) + n * g.n
            s, f, po, pr = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros((max(cap, 1), 2), np.uint32)
            _lib.check(_lib.lib().poa_align_batch_2piece(dg.handle, C.byref(c), n, engine._p(qseq), engine._p(qoff), engine._p(s),
                                                         engine._p(pr), engine._p(po), cap, engine._p(f), None, 0))
            score.append(s); flags.append(f); counts.append(np.diff(po.astype(np.int64))); pairs.append(pr[:int(po[n])])
        _PER_GRAPH[k] = (np.concatenate(score), np.concatenate(flags), np.concatenate(counts), np.concatenate(pairs))
    return _PER_GRAPH[k]


_CKPT = {}


def _checkpointed(engine, key, graphs, seqs, costs):
    """poa_multi_run_2piece on the same inputs, once per (batch, costs)."""
    k = (key, costs)
    if k not in _CKPT:
        _CKPT[k] = T2._run(engine, graphs, seqs, costs)
    return _CKPT[k]


def _check3(engine, oracle, res, key, graphs, seqs, costs, what):
    T2._check(res, T2._oracle_case(oracle, "dense2-" + key, graphs, seqs, costs), _per_graph(engine, key, graphs, seqs, costs), what)
    T2._same(res, _checkpointed(engine, key, graphs, seqs, costs), ("poa_multi_run_2piece", what))


def _run(engine, graphs, seqs, costs, workspace_bytes=0, run_cfg=None, wide=False):
    mb = engine.MultiGraphBatch(graphs, seqs, workspace_bytes=workspace_bytes, dense2=True)
    try:
        mb.run(T2._gc2(engine, costs, wide), None, run_cfg)
        res = mb.fetch()
        res.workspace_bytes = mb.workspace_bytes()
    finally:
        mb.close()
    return res


def _oracle_planes(oracle, g, q, costs):
    """The oracle's (M, I1, D1, I2, D2) of one query, by node."""
    m, e1, o1, e2, o2 = costs
    og = oracle.OracleGraph.from_csr(g.as_dict())
    with oracle.two_piece(o2, e2):
        d = og.dense_align(q, oracle.Costs(m, o1, e1), planes=True)
        i2, d2 = og.dense_planes2(q, oracle.Costs(m, o1, e1))
    orank = og.export_csr()["rank"]
    return [p[orank] for p in (d["M"], d["I"], d["D"], i2, d2)]


# ---- 1. mixed graphs, one run -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_dense2_mixed_graphs_one_run(engine, oracle):
    graphs, seqs = _mixed()
    terms = _terms(graphs, seqs)
    mb = engine.MultiGraphBatch(graphs, seqs, dense2=True)
    try:
        mb.run(T2._gc2(engine, COSTS))
        res = mb.fetch()
        _check3(engine, oracle, res, "mixed", graphs, seqs, COSTS, "one run")
        n = sum(len(s) for s in seqs)
        assert res.stats["n_chunks"] == 1 and res.stats["n_forward_launches"] == 1 and res.stats["n_queries"] == n
        assert res.stats["cells"] == sum(g.n * (len(q) + 1) for g, s in zip(graphs, seqs) for q in s)
        assert res.stats["plane_bytes"] == sum(t - 256 for _, t in terms)
        assert res.stats["ms_forward"] > 0 and res.stats["ms_traceback"] > 0
        assert mb.workspace_bytes() == sum(t for _, t in terms) == engine.multi_footprint(graphs, seqs, dense2=True)[0]
        # the queries of the graph without real nodes
        first = len(seqs[0]) + len(seqs[1])
        for i, q in enumerate(seqs[2]):
            assert res.flags[first + i] == EMPTY_GRAPH and res.score[first + i] == 4 * len(q) and res.raw_alignment(first + i) == []
        # the five planes of the reads at the pass edges, cell by cell, rows by node
        forty = graphs[1]
        rows = engine._device_graph(forty).node_rows()
        for k, q in enumerate(seqs[1]):
            got = mb.planes_2piece(len(seqs[0]) + k)
            for name, a, b in zip(("M", "I1", "D1", "I2", "D2"), got, _oracle_planes(oracle, forty, q, COSTS)):
                assert a.shape == (forty.n, len(q) + 1) and int(b[b != INF].max()) <= 65534
                assert np.array_equal(a[rows], b), (name, len(q))
        # a query of the chain and one of the second listing of the 40-row handle
        for qi, (g, q) in ((3, (graphs[0], seqs[0][3])), (first + len(seqs[2]) + 4, (forty, seqs[3][4]))):
            got = mb.planes_2piece(qi)
            r = engine._device_graph(g).node_rows()
            for name, a, b in zip(("M", "I1", "D1", "I2", "D2"), got, _oracle_planes(oracle, g, q, COSTS)):
                assert np.array_equal(a[r], b), (name, qi)
    finally:
        mb.close()


# ---- 2. one wave, several graphs --------------------------------------------------------------------------------------------------
_WAVE = None


def _wave_case():
    """80 short queries over four graphs of different shapes, 30 + 5 + 20 + 25: the walk's first wave (queries 0 to 63) spans
    three graph boundaries, one of them into and one out of a graph without real nodes, and the wave boundary at query 64 falls
    inside the last graph's range."""
    global _WAVE
    if _WAVE is None:
        rng = np.random.default_rng(33)
        graphs = [W.random_dag(11, n_nodes=8, p_edge=0.3), GraphBuilder().finish(), W.random_dag(12, n_nodes=20, p_edge=0.2),
                  W.random_dag(13, n_nodes=29, p_edge=0.15)]
        sizes = (30, 5, 20, 25)
        seqs = [[W.random_walk_query(rng, g, 0.25) if g.n > 2 else rng.choice(ACGT, int(rng.integers(0, 6))) for _ in range(k)]
                for g, k in zip(graphs, sizes)]
        assert len({g.n for g in graphs}) == 4 and sum(sizes) >= 70
        bounds = np.cumsum(sizes)
        assert sum(0 < b < 64 for b in bounds) >= 2 and bounds[2] < 64 < bounds[3]
        _WAVE = (graphs, seqs)
    return _WAVE


@pytest.mark.gpu
def test_multi_dense2_one_wave_several_graphs(engine, oracle):
    """Catches a uniform (readfirstlane) read of per-lane data in the walk: every lane of a wave would then walk lane 0's graph."""
    graphs, seqs = _wave_case()
    res = _run(engine, graphs, seqs, COSTS)
    _check3(engine, oracle, res, "wave", graphs, seqs, COSTS, "80 queries, one chunk")
    assert res.stats["n_chunks"] == 1
    # a cap that cuts in front of query 40: the second chunk's first query is no multiple of 64, and its first wave spans the
    # boundary between the last two graphs
    terms = _terms(graphs, seqs)
    cap = sum(t for _, t in terms[:40])
    firsts = T2._greedy(terms, cap)
    assert len(firsts) >= 2 and firsts[1] == 40 and firsts[1] % 64 != 0, firsts
    second = [gi for gi, _ in terms[firsts[1]:(firsts + [len(terms)])[2]]]
    assert second[0] == 2 and second[-1] == 3 and len(second) <= 64, second
    cut = _run(engine, graphs, seqs, COSTS, workspace_bytes=cap)
    assert cut.stats["n_chunks"] == len(firsts)
    T2._same(cut, res, "cut in front of query 40")
    _check3(engine, oracle, cut, "wave", graphs, seqs, COSTS, "80 queries, cut")


# ---- 3. chunk boundaries ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_dense2_chunk_boundaries(engine, oracle):
    graphs, seqs = _mixed()
    terms = _terms(graphs, seqs)
    total, largest = engine.multi_footprint(graphs, seqs, dense2=True)
    assert total == sum(t for _, t in terms) and largest == max(t for _, t in terms)
    whole = _run(engine, graphs, seqs, COSTS)
    assert whole.stats["n_chunks"] == 1 and whole.workspace_bytes == total
    for cap in (largest + 256, 1):   # just above the largest query; below it (raised to it)
        firsts = T2._greedy(terms, max(cap, largest))
        inside = [f for f in firsts[1:] if terms[f][0] == terms[f - 1][0]]
        between = [f for f in firsts[1:] if terms[f][0] != terms[f - 1][0]]
        assert len(firsts) >= 3 and inside and between, firsts
        res = _run(engine, graphs, seqs, COSTS, workspace_bytes=cap)
        assert res.stats["n_chunks"] == len(firsts) and res.stats["n_forward_launches"] == len(firsts), cap
        ends = firsts[1:] + [len(terms)]
        assert res.workspace_bytes == max(sum(t for _, t in terms[a:b]) for a, b in zip(firsts, ends)) <= max(cap, largest)
        T2._same(res, whole, ("chunked against one chunk", cap))
    _check3(engine, oracle, res, "mixed", graphs, seqs, COSTS, "cap 1")


# ---- 4. reruns ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_dense2_reruns_on_a_stream(engine, oracle):
    from poasta_amd import _lib
    graphs, seqs = _mixed()
    hip = _hip(engine)
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0 and s.value
    mb = engine.MultiGraphBatch(graphs, seqs, dense2=True)
    try:
        runs = []
        for costs in (COSTS, COSTS_EQ, (1, 1, 1, 1, 3), COSTS):
            mb.run(T2._gc2(engine, costs), s.value)
            res = mb.fetch()
            assert res.stats["n_runs"] == 1
            _check3(engine, oracle, res, "mixed", graphs, seqs, costs, ("stream", costs))
            runs.append(res)
        assert not np.array_equal(runs[0].score, runs[1].score)
        T2._same(runs[3], runs[0], "the first costs again")
        assert mb.stats()["n_runs"] == 0 and all(mb.device_results().values())
        # the one-shot entry point, raw and through the aligner
        mi = mb.input
        n = mb.n
        score, flags, pair_off = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
        pairs = np.zeros((mb.pair_capacity, 2), np.uint32)
        c = T2._gc2(engine, COSTS)._c()
        st = _lib.PoaStats()
        _lib.check(_lib.lib().poa_align_multi_dense_2piece(mi.handles, mi.n_graphs, engine._p(mi.graph_qoff), C.byref(c), None, engine._p(mi.qseq),
                                                           engine._p(mi.qoff), engine._p(score), engine._p(pairs), engine._p(pair_off),
                                                           mb.pair_capacity, engine._p(flags), C.byref(st), 0))
        assert np.array_equal(score, runs[0].score) and np.array_equal(flags, runs[0].flags) and np.array_equal(pair_off, runs[0].pair_off)
        assert np.array_equal(pairs[:int(pair_off[n])], runs[0].pairs) and st.n_chunks == 1
        al = engine.PoastaAligner(engine.Affine2PieceDijkstra(T2._gc2(engine, COSTS)))
        T2._same(al.align_multi(graphs, seqs, mode="dense2"), runs[0], "align_multi(mode=dense2)")
    finally:
        mb.close()
        hip.hipStreamDestroy(s)


# ---- 5. cell width ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_dense2_refuses_u32_cells(engine, oracle):
    from poasta_amd import _lib
    graphs, seqs = _mixed()
    m, e1, o1, e2, o2 = COSTS_U32
    assert e1 >= e2 and o1 + e1 * max(PASS_EDGES) > 65534
    mb = engine.MultiGraphBatch(graphs, seqs, dense2=True)
    try:
        for what, call in (("the u16 rule", lambda: mb.run(T2._gc2(engine, COSTS_U32))),
                           ("wide_planes", lambda: mb.run(T2._gc2(engine, COSTS, wide=True))),
                           ("POA_PLANES=32", lambda: mb.run(T2._gc2(engine, COSTS), None, engine.make_config("dense", planes=32)))):
            with pytest.raises(_lib.PoaError) as ei:
                call()
            assert ei.value.code == ERR_UNSUPPORTED, what
            assert "poa_multi_create_2piece" in str(ei.value), what
        # nothing ran: the batch has no result yet, and the next run with allowed costs is correct
        with pytest.raises(_lib.PoaError) as ei:
            mb.fetch()
        assert ei.value.code == ERR_INVALID_ARG
        mb.run(T2._gc2(engine, COSTS))
        _check3(engine, oracle, mb.fetch(), "mixed", graphs, seqs, COSTS, "after the refusals")
        with pytest.raises(_lib.PoaError) as ei:
            mb.run(T2._gc2(engine, COSTS_U32))
        assert ei.value.code == ERR_UNSUPPORTED
        mb.run(T2._gc2(engine, COSTS_EQ))
        _check3(engine, oracle, mb.fetch(), "mixed", graphs, seqs, COSTS_EQ, "after a refusal between two runs")
    finally:
        mb.close()


@pytest.mark.gpu
def test_multi_dense2_clamped_cells(engine, oracle):
    """Finite cells above 65 534 while the rule still allows u16: the arm graph and reads of tests/test_clamped_cells.py under its
    steep two-piece costs, beside a small chain.  Results against the oracle and the single-graph pass; the five planes of the
    600-symbol read cell for cell under that file's rule (the oracle's value if it is at most 65534, INF otherwise)."""
    import clamp_shapes as CS
    import test_clamped_cells as TCC
    d = TCC._arm_data(oracle, "rejoin")
    oplanes = TCC._two_piece_presence(d, "r600")   # (asserts at least 10 000 finite values above 65534 in every plane)
    costs = TCC.C2P_STEEP
    chain, chain_qs = _mixed()[0][0], _mixed()[1][0]
    graphs, seqs = [chain, d.g], [chain_qs, d.qs(TCC.Q600)]
    mb = engine.MultiGraphBatch(graphs, seqs, dense2=True)
    try:
        mb.run(T2._gc2(engine, costs))
        res = mb.fetch()
        T2._check(res, T2._oracle_case(oracle, "dense2-clamped", graphs, seqs, costs), _per_graph(engine, "clamped", graphs, seqs, costs), "steep costs")
        got = mb.planes_2piece(len(chain_qs))
        over = 0
        for pname, a, b in zip(("M", "I1", "D1", "I2", "D2"), got, oplanes):
            over += int(((b != INF) & (b > 65534)).sum())
            assert np.array_equal(a, CS.expected_u16(b)), pname
        assert over >= 50000
    finally:
        mb.close()


# ---- 6. contract --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_dense2_contract(engine):
    from poasta_amd import _lib
    L = _lib.lib()
    graphs, seqs = _mixed()
    graphs, seqs = graphs[:2], [seqs[0], seqs[1][:1]]
    n = sum(len(s) for s in seqs)
    c2 = T2._gc2(engine, COSTS)._c()
    c1 = engine.GapAffine(4, 2, 6)._c()
    bad = _lib.PoaCosts2(4, 6, 1, 24, 2, 0)   # extend1 < extend2
    score = np.zeros(n, np.uint32)
    out8 = (C.c_uint32 * 8)()
    buf = np.zeros(4, np.uint32)
    p = engine._p(buf)

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert L.poa_last_error() != b"", what

    mb = engine.MultiGraphBatch(graphs, seqs, dense2=True)
    others = {"checkpoint": engine.MultiGraphBatch(graphs, seqs), "checkpoint2": engine.MultiGraphBatch(graphs, seqs, two_piece=True),
              "dense": engine.MultiGraphBatch(graphs, seqs, dense=True), "exact": engine.MultiGraphBatch(graphs, seqs, exact=True)}
    try:
        refused(L.poa_multi_fetch(mb.handle, engine._p(score), None, None, 0, None, None), ERR_INVALID_ARG, "fetch before run")
        refused(L.poa_multi_fetch_planes_2piece(mb.handle, 0, p, p, p, p, p), ERR_INVALID_ARG, "planes before run")
        # every other kind's run call on this batch, and this run call on every other kind's batch
        refused(L.poa_multi_run(mb.handle, C.byref(c1), None, None), ERR_INVALID_ARG, "poa_multi_run")
        refused(L.poa_multi_run_2piece(mb.handle, C.byref(c2), None, None), ERR_INVALID_ARG, "poa_multi_run_2piece")
        refused(L.poa_multi_run_dense(mb.handle, C.byref(c1), None, None), ERR_INVALID_ARG, "poa_multi_run_dense")
        refused(L.poa_multi_run_exact(mb.handle, C.byref(c1), None, None), ERR_INVALID_ARG, "poa_multi_run_exact")
        for kind, other in others.items():
            refused(L.poa_multi_run_dense_2piece(other.handle, C.byref(c2), None, None), ERR_INVALID_ARG, ("this run call", kind))
            refused(L.poa_multi_fetch_planes_2piece(other.handle, 0, p, p, p, p, p), ERR_INVALID_ARG, ("planes", kind))
        with pytest.raises(ValueError):
            mb.run(engine.GapAffine(4, 2, 6))
        refused(L.poa_multi_run_dense_2piece(mb.handle, C.byref(bad), None, None), ERR_INVALID_ARG, "extend1 < extend2")
        for mode in ("exact", "hybrid", "score", "checkpoint", "checkpoint2"):
            refused(L.poa_multi_run_dense_2piece(mb.handle, C.byref(c2), C.byref(engine.make_config(mode)), None), ERR_UNSUPPORTED, ("run", mode))
        ef = engine.make_config("dense", aln_type=engine.AlignmentType.EndsFree())
        refused(L.poa_multi_run_dense_2piece(mb.handle, C.byref(c2), C.byref(ef), None), ERR_UNSUPPORTED, "ends-free, run")
        refused(L.poa_multi_fetch(mb.handle, engine._p(score), None, None, 0, None, None), ERR_INVALID_ARG, "still no run")
        # the batch is still usable; the records of the other kinds are not this kind's
        mb.run(T2._gc2(engine, COSTS))
        got = mb.fetch()
        T2._same(got, _run(engine, graphs, seqs, COSTS), "after the refusals")
        refused(L.poa_multi_last_launch(mb.handle, 0, out8), ERR_INVALID_ARG, "poa_multi_last_launch")
        refused(L.poa_multi_replay_info(mb.handle, 0, out8), ERR_INVALID_ARG, "poa_multi_replay_info")
        refused(L.poa_multi_fetch_planes_2piece(mb.handle, n, p, p, p, p, p), ERR_INVALID_ARG, "planes past the last query")
        # the other batches still run under their own calls
        others["checkpoint2"].run(T2._gc2(engine, COSTS))
        T2._same(others["checkpoint2"].fetch(), got, "the checkpointed two-piece batch")
    finally:
        mb.close()
        for other in others.values():
            other.close()
    # a cap of one query per chunk: the planes of a query of an earlier chunk are gone
    mb = engine.MultiGraphBatch(graphs, seqs, dense2=True, workspace_bytes=1)
    try:
        mb.run(T2._gc2(engine, COSTS))
        assert mb.fetch().stats["n_chunks"] >= 2
        refused(L.poa_multi_fetch_planes_2piece(mb.handle, 0, p, p, p, p, p), ERR_INVALID_ARG, "planes of an earlier chunk")
        assert len(mb.planes_2piece(n - 1)) == 5
    finally:
        mb.close()
    # an empty batch
    mb = engine.MultiGraphBatch(graphs, [[], []], dense2=True)
    try:
        mb.run(T2._gc2(engine, COSTS))
        res = mb.fetch()
        assert len(res.score) == 0 and res.pair_off.tolist() == [0] and res.stats["n_queries"] == 0
    finally:
        mb.close()
    assert len(engine.PoastaAligner(engine.Affine2PieceDijkstra(T2._gc2(engine, COSTS))).align_multi(graphs, [[], []], mode="dense2").score) == 0


# ---- 7. random sweep ----------------------------------------------------------------------------------------------------------------
_SWEEP = None


def _sweep():
    """24 seeded random DAGs of at most 30 rows, one to four reads each."""
    global _SWEEP
    if _SWEEP is None:
        graphs, seqs = [], []
        for seed in range(24):
            rng = np.random.Generator(np.random.PCG64(9100 + seed))
            alpha = b"AC" if seed % 2 else b"ACGT"
            g = W.random_dag(100 + seed, n_nodes=int(rng.integers(3, 29)), p_edge=float(rng.choice([0.15, 0.3])), alphabet=alpha)
            graphs.append(g)
            seqs.append([W.random_walk_query(rng, g, 0.3, alpha) for _ in range(int(rng.integers(1, 5)))])
        assert all(g.n <= 30 for g in graphs) and all(len(q) <= 80 for s in seqs for q in s)
        _SWEEP = (graphs, seqs)
    return _SWEEP


@pytest.mark.gpu
def test_multi_dense2_random_sweep(engine, oracle):
    graphs, seqs = _sweep()
    flagged = 0
    for costs in (COSTS, COSTS_EQ):
        res = _run(engine, graphs, seqs, costs)
        _check3(engine, oracle, res, "sweep", graphs, seqs, costs, ("sweep", costs))
        flagged += int((res.flags != 0).sum())
    assert flagged > 0   # (the certificate's bits do occur: they are compared, not just zero)


# ---- 8. which graph, then align -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_dense2_which_graph_then_align(engine):
    graphs, seqs = _sweep()
    graphs, reads = graphs[3:6], [q for s in seqs[3:6] for q in s]
    rng = np.random.default_rng(34)
    while len(reads) < 12:
        reads.append(W.random_walk_query(rng, graphs[len(reads) % 3], 0.2, b"ACGT"))
    reads = reads[:12]
    al = engine.PoastaAligner(engine.Affine2PieceDijkstra(T2._gc2(engine, COSTS)))
    a0, r0 = al.assign_and_align(graphs, reads)
    a1, r1 = al.assign_and_align(graphs, reads, mode="dense2")
    assert np.array_equal(a0["graph"], a1["graph"]) and np.array_equal(a0["score"], a1["score"])
    T2._same(r1, r0, "assign_and_align(mode=dense2) against the default mode")
    assert len(r1.score) == 12 and len({int(g) for g in a1["graph"]}) > 1
