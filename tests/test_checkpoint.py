"""Checkpointed mode (POA_MODE_CHECKPOINT): the segment plan on the CPU, and on the GPU the two passes against dense mode of
the same library — score, flags, pair_off and pairs equal as arrays, for every query of every case — and, on a sample,
against the oracle's dense restatement."""
import ctypes as C

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

NONE = 0xFFFFFFFF
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7


# ---- CPU: the segment plan ------------------------------------------------------------------------------------------------------
def _rows_view(g, dg):
    """Predecessors and successors in row space, the chain rows, and per row the rows that read it from memory."""
    rows = dg.node_rows()
    n = g.n
    node_of = np.zeros(n, np.int64)
    node_of[rows] = np.arange(n)
    pred_rows = [[int(rows[p]) for p in g.predecessors(int(node_of[r]))] for r in range(n)]
    succ_rows = [[int(rows[s]) for s in g.successors(int(node_of[r]))] for r in range(n)]
    chain = [len(pred_rows[r]) == 1 and pred_rows[r][0] + 1 == r for r in range(n)]
    readers = [[s for s in succ_rows[r] if not (s == r + 1 and chain[s])] for r in range(n)]
    return pred_rows, chain, readers


def _brute_force_plan_check(g, dg, segment_rows=0):
    """Recompute the snapshots from the CSR arrays and poa_graph_node_rows; check the exported plan against them."""
    boundary, rpq = dg.checkpoint_plan(segment_rows)
    _, n_slots = dg.sweep_slots()
    n = g.n
    pred_rows, chain, readers = _rows_view(g, dg)
    b = [int(v) for v in boundary]
    assert b[0] == 0 and b[-1] == n and all(x < y for x, y in zip(b, b[1:])), b
    seg_len = [y - x for x, y in zip(b, b[1:])]
    if segment_rows:
        k = min(segment_rows, n)
        assert all(s == k for s in seg_len[:-1]) and 0 < seg_len[-1] <= k, (segment_rows, seg_len)
    snap_rows = 0
    for bb in b[1:-1]:
        snap = {p for p in range(bb) if readers[p] and max(readers[p]) >= bb}
        if chain[bb]:
            snap.add(bb - 1)
        # every (reader row >= bb, read row < bb) pair of the graph has the read row in this snapshot
        for r in range(bb, n):
            for p in pred_rows[r]:
                assert p >= bb or p in snap, "row %d reads row %d across boundary %d: not in its snapshot" % (r, p, bb)
        assert len(snap) <= n_slots + 1
        snap_rows += len(snap)
    assert rpq == 2 * n_slots + 2 * snap_rows + 3 * max(seg_len), (rpq, n_slots, snap_rows, seg_len)
    assert rpq <= 2 * n_slots + 2 * (n_slots + 1) * len(seg_len) + 3 * max(seg_len)
    assert rpq <= 2 * n_slots + 3 * n or segment_rows   # the engine's own choice never holds more than one segment of all rows
    return len(seg_len), rpq


def _plan_checks(g):
    from poasta_amd import aligner
    dg = aligner.DeviceGraph(g)
    n_seg, rpq = _brute_force_plan_check(g, dg)
    for k in (1, 2, 7, g.n):
        s, r = _brute_force_plan_check(g, dg, k)
        assert s == -(-g.n // min(k, g.n))
        if k == g.n:
            assert s == 1 and rpq <= r   # "one segment" is the most the default may cost
    return n_seg


def test_checkpoint_plan_against_brute_force():
    from poasta_amd import aligner
    seen = set()
    for seed in range(300):
        rng = np.random.Generator(np.random.PCG64(5000 + seed))
        g = W.random_dag(seed, n_nodes=int(rng.integers(3, 40)), p_edge=float(rng.choice([0.1, 0.25, 0.5])), alphabet=b"AC" if seed % 2 else b"ACGT")
        seen.add(_plan_checks(g))
    assert len(seen) >= 3   # (the random graphs are cut into different numbers of segments)
    b = GraphBuilder()
    b.add_path(np.frombuffer(b"ACGTACGTACGTTTGA", np.uint8))
    _plan_checks(b.finish())
    g, _ = W.scaled_linearish(300, 15, 8, 1, 50)
    assert _plan_checks(g) > 1
    _plan_checks(W.LayeredPOA(n_layers=60, width=4, indeg=4, seed=5).graph)
    _plan_checks(W.PangenomePOA(ref_len=600, n_hap=8, seed=4).graph)
    _plan_checks(GraphBuilder().finish())
    # n_segments and rows_per_query alone (boundary = NULL)
    from poasta_amd import _lib
    dg = aligner.DeviceGraph(g)
    ns, rpq = C.c_uint32(0), C.c_uint32(0)
    _lib.check(_lib.lib().poa_graph_checkpoint_plan(dg.handle, 0, C.byref(ns), None, C.byref(rpq)))
    boundary, rpq2 = dg.checkpoint_plan()
    assert ns.value == len(boundary) - 1 and rpq.value == rpq2


def test_checkpoint_plan_follows_graph_update():
    from poasta_amd import _lib, aligner
    g0 = W.random_dag(7, n_nodes=20, p_edge=0.3)
    dg = aligner.DeviceGraph(g0)
    _brute_force_plan_check(g0, dg)
    for seed in (11, 12, 13):
        g1 = W.random_dag(seed, n_nodes=10 + seed, p_edge=0.25)
        _lib.check(_lib.lib().poa_graph_update(dg.handle, g1.n, g1.start, g1.end, aligner._p(g1.symbol), aligner._p(g1.succ_off),
                                               aligner._p(g1.succ), aligner._p(g1.pred_off), aligner._p(g1.pred)))
        dg.graph = g1
        _brute_force_plan_check(g1, dg)
        _brute_force_plan_check(g1, dg, 3)


def _memory_claim_graph():
    return W.scaled_linearish(4800, 240, 120, 24, 480)


def test_checkpoint_memory_claim():
    """A chain-like graph of more than 4 000 rows, the engine's own plan: a query holds at most 3/8 of the rows dense mode's
    planes have (with n_slots <= 8 the minimum of 2 * 9 * S + 3 * rows / S is 2 * sqrt(54 * rows), below rows / 4 from 4 000 rows
    on; the real snapshots are smaller than n_slots + 1 rows)."""
    from poasta_amd import aligner
    g, _ = _memory_claim_graph()
    dg = aligner.DeviceGraph(g)
    assert g.n >= 4000
    _, n_slots = dg.sweep_slots()
    assert n_slots <= 8
    boundary, rpq = dg.checkpoint_plan()
    assert len(boundary) - 1 > 1
    assert rpq <= 3 * g.n // 8, (rpq, g.n)


def test_checkpoint_mode_in_the_python_mirror():
    from poasta_amd import _lib, aligner
    assert aligner.make_config(mode="checkpoint").mode == 4 == _lib.MODE_CHECKPOINT
    with pytest.raises(KeyError):
        aligner.make_config(mode="checkpoints")
    cfg = aligner.make_config(mode="checkpoint", ckpt_rows=7)
    assert cfg.tune[_lib.TUNE_KEYS.index("CKPT_ROWS")] == 8 and len(_lib.TUNE_KEYS) <= 32
    assert b"0.2" in _lib.lib().poa_version()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _costs(engine, m, o, e):
    return engine.GapAffine(m, e, o)   # reference ctor order: (mismatch, extend, open)


def _run(engine, g, qseq, qoff, costs, cfg=None, workspace_bytes=0):
    rb = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=workspace_bytes, config=cfg if (cfg is not None and cfg.mode == 4) else None)
    rb.run(_costs(engine, *costs), None, cfg)
    res = rb.fetch()
    res.workspace_bytes = rb.workspace_bytes()
    rb.close()
    return res


def _equal(a, b, what):
    assert np.array_equal(a.score, b.score), ("score", what)
    assert np.array_equal(a.flags, b.flags), ("flags", what)
    assert np.array_equal(a.pair_off, b.pair_off), ("pair_off", what)
    assert np.array_equal(a.pairs, b.pairs), ("pairs", what)


PLANS = (0, 1, 2, 7, "one")


def _parity(engine, g, qs, costs, plans=PLANS, oracle=None, **tune):
    """Checkpointed mode, resident and one-shot, under every plan, against dense mode of the same library."""
    qseq, qoff = pack_queries(qs)
    dense = _run(engine, g, qseq, qoff, costs)
    for k in plans:
        kw = dict(tune)
        if k:
            kw["ckpt_rows"] = g.n if k == "one" else k
        cfg = engine.make_config("checkpoint", **kw)
        _equal(_run(engine, g, qseq, qoff, costs, cfg), dense, (costs, k, tune))
    # one-shot, through the aligner (poa_align_batch_ex)
    al = engine.PoastaAligner(engine.AffineDijkstra(_costs(engine, *costs)), mode="checkpoint")
    _equal(al.align_batch(g, qseq=qseq, qoff=qoff), dense, (costs, "one-shot"))
    if oracle is not None and g.n > 2:
        og = oracle.OracleGraph.from_csr(g.as_dict())
        D = og.dense_batch(qseq, qoff, oracle.Costs(*costs), threads=4)
        assert np.array_equal(dense.score, D["score"])
        for i in range(len(qs)):
            assert dense.raw_alignment(i) == oracle.batch_alignment(D, i)
    return dense


def _with_short(qs, rng, alpha=b"ACGT"):
    a = np.frombuffer(alpha, np.uint8)
    return list(qs) + [np.zeros(0, np.uint8), rng.choice(a, 1), rng.choice(a, 2), rng.choice(a, 3)]


COST_SETS = [(4, 6, 2), (1, 1, 1), (255, 6, 2), (2, 8, 1), (3, 1, 1)]


@pytest.mark.gpu
def test_checkpoint_parity_random_dags(engine, oracle):
    flagged = 0
    for seed in range(40):
        rng = np.random.Generator(np.random.PCG64(1000 + seed))
        alpha = b"AC" if seed % 2 else b"ACGT"
        g = W.random_dag(seed, n_nodes=int(rng.integers(3, 30)), p_edge=float(rng.choice([0.15, 0.3])), alphabet=alpha)
        qs = _with_short([W.random_walk_query(rng, g, 0.3, alpha) for _ in range(12)], rng, alpha)
        for costs in (COST_SETS[seed % 5], COST_SETS[(seed + 1) % 5]):
            d = _parity(engine, g, qs, costs, oracle=oracle if seed < 12 else None)
            flagged += int((d.flags != 0).sum())
        if seed < 8:
            _parity(engine, g, qs, (255, 6, 2), planes=32)   # the u32 cells on the same inputs
    assert flagged > 0   # (the certificate's bits do occur in these cases: they are compared, not just zero)


def _skip_graph():
    """A chain of 64 nodes with one edge from node 4 of the chain to node 57: with seven rows per segment it skips seven
    segments.  Returns the graph and the sequence of the path through that edge."""
    rng = np.random.default_rng(11)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 64)
    b = GraphBuilder()
    ids = b.add_path(seq)
    b.add_edge(ids[4], ids[57])
    return b.finish(), np.concatenate([seq[:5], seq[57:]])


@pytest.mark.gpu
def test_checkpoint_edge_that_skips_segments(engine, oracle):
    g, through = _skip_graph()
    rng = np.random.default_rng(12)
    qs = [through, through[:-1], np.concatenate([through[:3], through[4:]])] + [W.random_walk_query(rng, g, 0.1) for _ in range(6)]
    for costs in ((4, 6, 2), (1, 1, 1)):
        d = _parity(engine, g, qs, costs, oracle=oracle)
        assert d.score[0] == 0 and len(d.raw_alignment(0)) == len(through)   # the walk took the long edge: 12 pairs, not 64
    boundary, _ = engine._device_graph(g).checkpoint_plan(7)
    assert len(boundary) - 1 >= 9


@pytest.mark.gpu
def test_checkpoint_parity_strips_and_workloads(engine, oracle):
    """One, two and three strips (> 1 024, > 2 048 columns), mixed lengths in one batch, the u16 and the u32 cells, and the
    workload graphs at reduced size."""
    rng = np.random.default_rng(4)
    poa = W.LayeredPOA(n_layers=160, width=4, indeg=4, seed=5)
    qs = _with_short(poa.queries(2, length=1500) + poa.queries(2, length=2500, seed=9) + poa.queries(3, length=700, seed=10) +
                     poa.queries(3, length=140, seed=11), rng)
    _parity(engine, poa.graph, qs, (4, 6, 2))
    _parity(engine, poa.graph, qs, (4, 6, 2), planes=32)
    _parity(engine, poa.graph, qs, (255, 60, 40))   # a bound beyond u16: u32 cells by the engine's own choice
    _parity(engine, poa.graph, poa.queries(6, length=300), (1, 1, 1), oracle=oracle)
    g, (qseq, qoff) = W.scaled_linearish(900, 50, 25, 16, 1000, p_sub=0.1, p_ins=0.03, p_del=0.03)
    qs = _with_short([qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(16)], rng)
    qs.append(rng.choice(np.frombuffer(b"ACGT", np.uint8), 1023))
    _parity(engine, g, qs, (4, 6, 2))
    _parity(engine, g, qs, (255, 6, 2))
    g, (qseq, qoff) = W.scaled_linearish(1500, 40, 20, 4, 0)
    _parity(engine, g, [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(4)], (4, 6, 2))
    pg = W.PangenomePOA(ref_len=1500, n_hap=12, seed=4)
    _parity(engine, pg.graph, _with_short(pg.queries(4, length=1200) + pg.queries(4, length=300, seed=8), rng), (4, 6, 2))
    # cell widths the engine chose
    sseq, soff = pack_queries(qs)
    cfg = engine.make_config("checkpoint")
    rb = engine.ResidentBatch(g, sseq, soff, config=cfg)
    for costs, narrow in (((4, 6, 2), True), ((255, 60, 40), False)):
        rb.run(_costs(engine, *costs), None, cfg)
        assert ("u16" in rb.layout()) == narrow, costs
    rb.close()


@pytest.mark.gpu
def test_checkpoint_empty_graph_and_empty_batch(engine, oracle):
    empty = GraphBuilder().finish()
    costs = (4, 6, 2)
    al = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, *costs)), mode="checkpoint")
    dense = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, *costs)))
    _equal(al.align_batch(empty, [b"ACGT", b"", b"A"]), dense.align_batch(empty, [b"ACGT", b"", b"A"]), "empty graph, one-shot")
    qseq, qoff = pack_queries([b"ACGT", b"", b"A"])
    # the resident entry point on the empty graph: both passes over the two sentinel rows, as in dense mode
    _equal(_run(engine, empty, qseq, qoff, costs, engine.make_config("checkpoint")), _run(engine, empty, qseq, qoff, costs), "empty graph, resident")
    b = GraphBuilder()
    b.add_path(np.frombuffer(b"ACGT", np.uint8))
    r = al.align_batch(b.finish(), [])
    assert len(r.score) == 0 and len(r.pairs) == 0


@pytest.mark.gpu
def test_checkpoint_workspace_and_chunks(engine, oracle):
    """The graph of the memory claim: the batch holds rows_per_query x pitch x 4 bytes per query (+ 256 bytes of padding);
    under a cap it runs in chunks, fewer than dense mode needs under the same cap, with the same arrays."""
    g, (qseq, qoff) = _memory_claim_graph()
    n_q = len(qoff) - 1
    costs = (4, 6, 2)
    _, rpq = engine._device_graph(g).checkpoint_plan()
    pitches = [((int(qoff[i + 1] - qoff[i]) + 1 + 63) // 64) * 64 for i in range(n_q)]
    cfg = engine.make_config("checkpoint")
    whole = _run(engine, g, qseq, qoff, costs, cfg)
    assert whole.workspace_bytes == sum(rpq * p * 4 for p in pitches) + 256
    assert whole.stats["n_chunks"] == 1 and whole.stats["ms_forward"] > 0 and whole.stats["ms_traceback"] > 0
    dense = _run(engine, g, qseq, qoff, costs)
    _equal(whole, dense, "one chunk")
    cap = 3 * g.n * max(pitches) * 4   # one query's full u32 planes: dense mode needs chunks under it, this mode far fewer
    capped = _run(engine, g, qseq, qoff, costs, cfg, workspace_bytes=cap)
    dense_capped = _run(engine, g, qseq, qoff, costs, workspace_bytes=cap)
    assert capped.workspace_bytes <= cap + 256
    assert capped.stats["n_chunks"] < dense_capped.stats["n_chunks"], (capped.stats["n_chunks"], dense_capped.stats["n_chunks"])
    _equal(capped, dense, "capped")
    _equal(dense_capped, dense, "dense, chunked")
    # five queries' footprint in u32 cells: ten queries a chunk in the u16 cells these costs allow, at least two chunks either way
    cap = 5 * rpq * max(pitches) * 4
    chunked = _run(engine, g, qseq, qoff, costs, cfg, workspace_bytes=cap)
    dense_chunked = _run(engine, g, qseq, qoff, costs, workspace_bytes=cap)
    assert chunked.workspace_bytes <= cap + 256
    assert 2 <= chunked.stats["n_chunks"] <= -(-n_q // 5) and chunked.stats["n_chunks"] < dense_chunked.stats["n_chunks"]
    _equal(chunked, dense, "chunked")
    wide = _run(engine, g, qseq, qoff, costs, engine.make_config("checkpoint", planes=32), workspace_bytes=cap)   # u32 cells: five a chunk
    assert wide.stats["n_chunks"] == -(-n_q // 5)
    _equal(wide, dense, "chunked, u32 cells")
    tiny = _run(engine, g, qseq, qoff, costs, cfg, workspace_bytes=1)   # a cap below one query: one query per chunk
    assert tiny.stats["n_chunks"] >= n_q // 2   # (u16 cells: two queries share what one query's u32 cells need)
    _equal(tiny, dense, "one query per chunk")


@pytest.mark.gpu
def test_checkpoint_guards_and_resident_reuse(engine, oracle):
    from poasta_amd import _lib
    g, (qseq, qoff) = W.scaled_linearish(200, 10, 5, 8, 180)
    cfg = engine.make_config("checkpoint")
    rb = engine.ResidentBatch(g, qseq, qoff, config=cfg)
    rd = engine.ResidentBatch(g, qseq, qoff)
    # a resident batch runs twice with two cost sets and matches dense both times
    for costs in ((4, 6, 2), (1, 1, 1), (4, 6, 2)):
        rb.run(_costs(engine, *costs), None, cfg)
        rd.run(_costs(engine, *costs))
        _equal(rb.fetch(), rd.fetch(), costs)
    costs = _costs(engine, 4, 6, 2)
    ef = engine.make_config("checkpoint", aln_type=engine.AlignmentType.EndsFree())
    with pytest.raises(_lib.PoaError) as e:
        rb.run(costs, None, ef)
    assert e.value.code == ERR_UNSUPPORTED
    for other in ("dense", "exact", "hybrid", "score"):
        with pytest.raises(_lib.PoaError) as e:
            rb.run(costs, None, engine.make_config(other))
        assert e.value.code == ERR_INVALID_ARG, other
    with pytest.raises(_lib.PoaError) as e:
        rb.run(costs)   # poa_batch_run: dense
    assert e.value.code == ERR_INVALID_ARG
    with pytest.raises(_lib.PoaError) as e:
        rb.planes(0)
    assert e.value.code == ERR_UNSUPPORTED
    rb.run(costs, None, cfg)   # the batch is still usable
    rd.run(costs)
    _equal(rb.fetch(), rd.fetch(), "after the refused calls")
    # the other way round: a dense batch and a score batch in this mode
    with pytest.raises(_lib.PoaError) as e:
        rd.run(costs, None, cfg)
    assert e.value.code == ERR_INVALID_ARG
    rs = engine.ResidentBatch(g, qseq, qoff, config=engine.make_config("score"))
    with pytest.raises(_lib.PoaError) as e:
        rs.run(costs, None, cfg)
    assert e.value.code == ERR_INVALID_ARG
    for b in (rb, rd, rs):
        b.close()
    with pytest.raises(_lib.PoaError) as e:
        engine.ResidentBatch(g, qseq, qoff, config=ef)
    assert e.value.code == ERR_UNSUPPORTED
    n = len(qoff) - 1
    score = np.zeros(n, np.uint32)
    c = costs._c()
    rc = _lib.lib().poa_align_batch_ex(engine._device_graph(g).handle, C.byref(c), C.byref(ef), n, engine._p(qseq), engine._p(qoff),
                                       engine._p(score), None, None, 0, None, None, 0)
    assert rc == ERR_UNSUPPORTED
    two = engine.PoastaAligner(engine.Affine2PieceDijkstra(engine.GapAffine2Piece(4, 2, 6, 1, 24)), mode="checkpoint")
    with pytest.raises(_lib.PoaError) as e:
        two.align_batch(g, qseq=qseq, qoff=qoff)
    assert e.value.code == ERR_UNSUPPORTED
