"""Multi-graph batches under the two-piece affine model (poa_multi_*_2piece): the queries of many graphs in one run.

Every comparison has two references and demands equality: the oracle's two-piece dense restatement and walk of every query
against its own graph (score, flags, pair counts, alignment), and the per-graph one-shot poa_align_batch_2piece_ex in
POA_MODE_CHECKPOINT2 of the same library on the same inputs (score, flags, per-query pair counts, pairs).

Costs are written in GapAffine2Piece's order: (mismatch, extend1, open1, extend2, open2)."""
import ctypes as C

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import pack_queries

from test_multi_graph import EMPTY_GRAPH, ERR_INVALID_ARG, ERR_UNSUPPORTED, LONG, _hip, _mixed

COSTS = (4, 2, 6, 1, 24)   # -g 6,24 -e 2,1


def _pitch(length):
    return ((length + 1 + 63) // 64) * 64


def _gc2(engine, costs, wide=False):
    c = engine.GapAffine2Piece(*costs)
    if wide:
        class Wide(engine.GapAffine2Piece):   # poa_costs2_t.wide_planes = 1
            def _c(self):
                k = engine.GapAffine2Piece._c(self)
                k.wide_planes = 1
                return k
        c = Wide(*costs)
    return c


_ORACLE = {}


def _oracle_case(oracle, key, graphs, seqs, costs):
    """Per query (score, flags, pair count, raw alignment) by the oracle, computed once per (batch, costs)."""
    k = (key, costs)
    if k not in _ORACLE:
        m, e1, o1, e2, o2 = costs
        out = []
        for g, qs in zip(graphs, seqs):
            if not qs:
                continue
            if g.n == 2:   # no real nodes: the aligner's shortcut, score 4 * len, no alignment
                out += [(4 * len(q), EMPTY_GRAPH, 0, []) for q in qs]
                continue
            qseq, qoff = pack_queries(qs)
            with oracle.two_piece(o2, e2):
                D = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq, qoff, oracle.Costs(m, o1, e1), threads=4)
            out += [(int(D["score"][i]), int(D["flags"][i]), int(D["n_pairs"][i]), oracle.batch_alignment(D, i)) for i in range(len(qs))]
        _ORACLE[k] = out
    return _ORACLE[k]


_PER_GRAPH = {}


def _per_graph(engine, key, graphs, seqs, costs, **tune):
    """poa_align_batch_2piece_ex in POA_MODE_CHECKPOINT2, graph by graph: (score, flags, per-query pair counts, pairs) concatenated."""
    k = (key, costs, tuple(sorted(tune.items())))
    if k not in _PER_GRAPH:
        from poasta_amd import _lib
        cfg = engine.make_config("checkpoint2", **tune)
        c = _gc2(engine, costs)._c()
        score, flags, counts, pairs = [], [], [], []
        for g, qs in zip(graphs, seqs):
            if not qs:
                continue
            dg = engine._device_graph(g)
            qseq, qoff = pack_queries(qs)
            n = len(qs)
            cap = int(qoff[-1]) + n * g.n
            s, f, po, pr = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros((max(cap, 1), 2), np.uint32)
            _lib.check(_lib.lib().poa_align_batch_2piece_ex(dg.handle, C.byref(c), C.byref(cfg), n, engine._p(qseq), engine._p(qoff), engine._p(s),
                                                            engine._p(pr), engine._p(po), cap, engine._p(f), None, None, 0))
            score.append(s); flags.append(f); counts.append(np.diff(po.astype(np.int64))); pairs.append(pr[:int(po[n])])
        _PER_GRAPH[k] = (np.concatenate(score), np.concatenate(flags), np.concatenate(counts), np.concatenate(pairs))
    return _PER_GRAPH[k]


def _check(res, oracle_case, per_graph, what):
    score, flags, counts, pairs = per_graph
    assert np.array_equal(res.score, score), ("score", what)
    assert np.array_equal(res.flags, flags), ("flags", what)
    assert np.array_equal(np.diff(res.pair_off.astype(np.int64)), counts), ("pair counts", what)
    assert np.array_equal(res.pairs, pairs), ("pairs", what)
    assert len(res.score) == len(oracle_case)
    got_counts = np.diff(res.pair_off.astype(np.int64))
    for i, (s, f, c, aln) in enumerate(oracle_case):
        assert int(res.score[i]) == s, ("oracle score", what, i)
        assert int(res.flags[i]) == f, ("oracle flags", what, i)
        assert int(got_counts[i]) == c, ("oracle pair count", what, i)
        assert res.raw_alignment(i) == aln, ("oracle alignment", what, i)


def _same(a, b, what):
    for name in ("score", "flags", "pair_off", "pairs"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (name, what)


def _run(engine, graphs, seqs, costs, workspace_bytes=0, run_cfg=None, create_cfg=None, wide=False):
    mb = engine.MultiGraphBatch(graphs, seqs, workspace_bytes=workspace_bytes, config=create_cfg, two_piece=True)
    try:
        mb.run(_gc2(engine, costs, wide), None, run_cfg if run_cfg is not None else create_cfg)
        res = mb.fetch()
        res.workspace_bytes = mb.workspace_bytes()
    finally:
        mb.close()
    return res


def _terms(engine, graphs, seqs, segment_rows=0):
    """Per query: (graph index, bytes it holds) — rows_per_query2 of its graph's own two-piece plan x pitch x 4 + 256."""
    out = []
    for gi, (g, qs) in enumerate(zip(graphs, seqs)):
        _, rpq = engine._device_graph(g).checkpoint_plan(segment_rows, two_piece=True)
        out += [(gi, rpq * _pitch(len(q)) * 4 + 256) for q in qs]
    return out


def _greedy(terms, cap):
    """First query of every chunk: greedy in query order, a chunk ends in front of the first query that no longer fits."""
    firsts, used = [0], 0
    for i, (_, t) in enumerate(terms):
        if used + t > cap and i > firsts[-1]:
            firsts.append(i)
            used = 0
        used += t
    return firsts


# ---- 1. mixed small graphs in one run ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi2_mixed_graphs_one_run(engine, oracle):
    graphs, seqs = _mixed()
    res = _run(engine, graphs, seqs, COSTS)
    _check(res, _oracle_case(oracle, "mixed", graphs, seqs, COSTS), _per_graph(engine, "mixed", graphs, seqs, COSTS), "one run")
    n = sum(len(s) for s in seqs)
    assert res.stats["n_chunks"] == 1 and res.stats["n_queries"] == n
    assert res.stats["cells"] == sum(g.n * (len(q) + 1) for g, s in zip(graphs, seqs) for q in s)
    assert res.stats["ms_forward"] > 0 and res.stats["ms_traceback"] > 0
    assert res.workspace_bytes == sum(t for _, t in _terms(engine, graphs, seqs))
    # the queries of the graph without real nodes
    first = sum(len(s) for s in seqs[:3])
    for i, q in enumerate(seqs[3]):
        assert res.flags[first + i] == EMPTY_GRAPH and res.score[first + i] == 4 * len(q) and res.raw_alignment(first + i) == []
    # the one-shot entry point through the aligner
    one = engine.PoastaAligner(engine.Affine2PieceDijkstra(_gc2(engine, COSTS))).align_multi(graphs, seqs)
    _same(one, res, "align_multi")
    # ends-free still raises
    with pytest.raises(ValueError):
        engine.PoastaAligner(engine.Affine2PieceDijkstra(_gc2(engine, COSTS)), engine.AlignmentType.EndsFree()).align_multi(graphs, seqs)


# ---- 2. several segments ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi2_several_segments(engine, oracle):
    graphs, seqs = _mixed()
    k = 7
    n_seg = [len(engine._device_graph(g).checkpoint_plan(k, two_piece=True)[0]) - 1 for g in graphs]
    assert sum(s >= 3 for s in n_seg[:3]) >= 2 and n_seg[3] == 1, n_seg   # chain, bubble, GFA graph: 3 or more; the empty graph: one
    cfg = engine.make_config("checkpoint2", ckpt_rows=k)
    res = _run(engine, graphs, seqs, COSTS, create_cfg=cfg)
    _check(res, _oracle_case(oracle, "mixed", graphs, seqs, COSTS), _per_graph(engine, "mixed", graphs, seqs, COSTS, ckpt_rows=k), "ckpt_rows 7")
    assert res.workspace_bytes == sum(t for _, t in _terms(engine, graphs, seqs, k))


# ---- 3. chunk boundaries ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi2_chunk_boundaries(engine, oracle):
    graphs, seqs = _mixed()
    total, largest = engine.multi_footprint(graphs, seqs, two_piece=True)
    terms = _terms(engine, graphs, seqs)
    assert total == sum(t for _, t in terms) and largest == max(t for _, t in terms)
    cap = largest + 256   # just above the largest query
    firsts = _greedy(terms, cap)
    inside = [f for f in firsts[1:] if terms[f][0] == terms[f - 1][0]]
    between = [f for f in firsts[1:] if terms[f][0] != terms[f - 1][0]]
    assert len(firsts) >= 3 and inside and between, firsts
    res = _run(engine, graphs, seqs, COSTS, workspace_bytes=cap)
    assert res.stats["n_chunks"] == len(firsts)
    ends = firsts[1:] + [len(terms)]
    assert res.workspace_bytes == max(sum(t for _, t in terms[a:b]) for a, b in zip(firsts, ends)) <= cap
    _check(res, _oracle_case(oracle, "mixed", graphs, seqs, COSTS), _per_graph(engine, "mixed", graphs, seqs, COSTS), "chunked")
    whole = _run(engine, graphs, seqs, COSTS)
    assert whole.stats["n_chunks"] == 1
    _same(res, whole, "chunked against one chunk")
    # a cap below the largest query is raised to it
    low = _run(engine, graphs, seqs, COSTS, workspace_bytes=1)
    assert low.stats["n_chunks"] == len(_greedy(terms, largest)) >= len(firsts) and low.workspace_bytes == largest
    _same(low, whole, "cap 1")
    # the same under u32 cells: the same chunks, the same results
    p32 = engine.make_config("checkpoint2", planes=32)
    for ws, want_chunks in ((cap, len(firsts)), (1, len(_greedy(terms, largest)))):
        wide = _run(engine, graphs, seqs, COSTS, workspace_bytes=ws, run_cfg=p32)
        assert wide.stats["n_chunks"] == want_chunks and wide.workspace_bytes == (res.workspace_bytes if ws == cap else largest)
        _same(wide, whole, ("planes 32", ws))


# ---- 4. cell width ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi2_cell_width(engine, oracle):
    graphs, seqs = _mixed()
    narrow = _run(engine, graphs, seqs, COSTS)
    # open1 + extend1 x longest query + open1 + extend1 x shortest path: beyond 65534 for the chain graph alone (its 1100-symbol query)
    costs = (255, 60, 40, 3, 200)
    m, e1, o1, e2, o2 = costs
    assert e1 >= e2
    longest = [max(len(q) for q in qs) if qs else 0 for qs in seqs]
    assert longest[0] == LONG and o1 + e1 * longest[0] > 65534   # (whatever its shortest path)
    assert all(o1 + e1 * l + o1 + e1 * g.n <= 65534 for g, l in list(zip(graphs, longest))[1:])   # (a shortest path has fewer than n nodes)
    wide = _run(engine, graphs, seqs, costs)
    assert wide.stats["plane_bytes"] == 2 * narrow.stats["plane_bytes"]   # the same cells stored, four bytes each: the whole run is u32
    _check(wide, _oracle_case(oracle, "mixed", graphs, seqs, costs), _per_graph(engine, "mixed", graphs, seqs, costs), "u32 by the bound")
    # u32 cells forced on the run that would be u16: identical results
    for tag, kw in (("planes 32", dict(run_cfg=engine.make_config("checkpoint2", planes=32))), ("wide_planes", dict(wide=True))):
        forced = _run(engine, graphs, seqs, COSTS, **kw)
        assert forced.stats["plane_bytes"] == 2 * narrow.stats["plane_bytes"], tag
        _same(forced, narrow, tag)


# ---- 5. re-run and streams --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi2_rerun_on_a_stream(engine, oracle):
    graphs, seqs = _mixed()
    hip = _hip(engine)
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0 and s.value
    mb = engine.MultiGraphBatch(graphs, seqs, two_piece=True)
    try:
        second = (1, 1, 1, 1, 3)
        for costs in (COSTS, second):
            mb.run(_gc2(engine, costs), s.value)
            res = mb.fetch()
            assert res.stats["n_runs"] == 1
            _check(res, _oracle_case(oracle, "mixed", graphs, seqs, costs), _per_graph(engine, "mixed", graphs, seqs, costs), ("stream", costs))
        _same(_run(engine, graphs, seqs, second), res, "fresh batch")
        assert mb.stats()["n_runs"] == 0 and all(mb.device_results().values())
    finally:
        mb.close()
        hip.hipStreamDestroy(s)


# ---- 6. random sweep --------------------------------------------------------------------------------------------------------------
_SWEEP = None
SWEEP_COSTS = (COSTS, (3, 2, 4, 2, 9))   # the second with extend1 == extend2


def _sweep():
    """The 40 seeded graphs of test_multi_graph.test_multi_random_sweep."""
    global _SWEEP
    if _SWEEP is None:
        graphs, seqs = [], []
        for seed in range(40):
            rng = np.random.Generator(np.random.PCG64(7000 + seed))
            alpha = b"AC" if seed % 2 else b"ACGT"
            g = W.random_dag(seed, n_nodes=int(rng.integers(3, 30)), p_edge=float(rng.choice([0.15, 0.3])), alphabet=alpha)
            graphs.append(g)
            seqs.append([W.random_walk_query(rng, g, 0.3, alpha) for _ in range(int(rng.integers(1, 9)))])
        _SWEEP = (graphs, seqs)
    return _SWEEP


@pytest.mark.gpu
def test_multi2_random_sweep(engine, oracle):
    graphs, seqs = _sweep()
    assert SWEEP_COSTS[1][1] == SWEEP_COSTS[1][3]
    flagged = 0
    for costs in SWEEP_COSTS:
        res = _run(engine, graphs, seqs, costs)
        _check(res, _oracle_case(oracle, "sweep", graphs, seqs, costs), _per_graph(engine, "sweep", graphs, seqs, costs), ("sweep", costs))
        flagged += int((res.flags != 0).sum())
    assert flagged > 0   # (the certificate's bits do occur: they are compared, not just zero)


# ---- 7. which graph, then align ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi2_which_graph_then_align(engine):
    graphs, seqs = _sweep()
    al = engine.PoastaAligner(engine.Affine2PieceDijkstra(_gc2(engine, COSTS)))
    reads = [q for s in seqs for q in s]
    own = [gi for gi, s in enumerate(seqs) for _ in s]
    n_g = len(graphs)
    pairs = np.array([(r, g) for r, gi in enumerate(own) for g in (gi, (gi + 1) % n_g, (gi + 17) % n_g)], np.uint32)
    score, _ = al.score_pairs(graphs, reads, pairs)
    score = score.reshape(len(reads), 3)
    pick = np.argmin(score, axis=1)
    winner = pairs.reshape(len(reads), 3, 2)[np.arange(len(reads)), pick, 1]
    best = score[np.arange(len(reads)), pick]
    # group the reads by their winner, graph order
    by_graph = [[r for r in range(len(reads)) if winner[r] == g] for g in range(n_g)]
    res = al.align_multi(graphs, [[reads[r] for r in rs] for rs in by_graph])
    order = [r for rs in by_graph for r in rs]
    assert len(order) == len(reads)
    assert np.array_equal(res.score, best[order])
    assert len({int(w) for w in winner}) > 1


# ---- 8. contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi2_contract(engine):
    from poasta_amd import _lib
    L = _lib.lib()
    graphs, seqs = _mixed()
    graphs, seqs = graphs[1:3], seqs[1:3]
    handles = (C.c_void_p * 2)(*[engine._device_graph(g).handle for g in graphs])
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    n0, n = len(seqs[0]), len(qoff) - 1
    gq = np.array([0, n0, n], np.uint64)
    c2 = _gc2(engine, COSTS)._c()
    c1 = engine.GapAffine(4, 2, 6)._c()
    bad = _lib.PoaCosts2(4, 6, 1, 24, 2, 0)   # extend1 < extend2
    score = np.zeros(n, np.uint32)

    def create(cfg, gqoff=gq, hs=handles):
        h = C.c_void_p()
        rc = L.poa_multi_create_2piece(hs, 2, engine._p(gqoff), 0, engine._p(qseq), engine._p(qoff), C.byref(cfg) if cfg is not None else None, 0, C.byref(h))
        if rc == 0:
            L.poa_multi_destroy(h)
        return rc

    def one_shot(costs, cfg):
        return L.poa_align_multi_2piece(handles, 2, engine._p(gq), C.byref(costs), C.byref(cfg) if cfg is not None else None, engine._p(qseq),
                                        engine._p(qoff), engine._p(score), None, None, 0, None, None, 0)

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert L.poa_last_error() != b"", what

    assert create(None) == 0 and create(engine.make_config("checkpoint2")) == 0
    mb = engine.MultiGraphBatch(graphs, seqs, two_piece=True)
    old = engine.MultiGraphBatch(graphs, seqs)
    try:
        for mode in ("dense", "exact", "hybrid", "score", "checkpoint"):
            cfg = engine.make_config(mode)
            refused(create(cfg), ERR_UNSUPPORTED, ("create", mode))
            refused(L.poa_multi_run_2piece(mb.handle, C.byref(c2), C.byref(cfg), None), ERR_UNSUPPORTED, ("run", mode))
            refused(one_shot(c2, cfg), ERR_UNSUPPORTED, ("one-shot", mode))
        ef = engine.make_config("checkpoint2", aln_type=engine.AlignmentType.EndsFree())
        refused(create(ef), ERR_UNSUPPORTED, "ends-free, create")
        refused(L.poa_multi_run_2piece(mb.handle, C.byref(c2), C.byref(ef), None), ERR_UNSUPPORTED, "ends-free, run")
        refused(one_shot(c2, ef), ERR_UNSUPPORTED, "ends-free, one-shot")
        refused(L.poa_multi_fetch(mb.handle, engine._p(score), None, None, 0, None, None), ERR_INVALID_ARG, "fetch before run")
        # the batch and the run belong to one model
        refused(L.poa_multi_run(mb.handle, C.byref(c1), None, None), ERR_INVALID_ARG, "poa_multi_run on a two-piece batch")
        refused(L.poa_multi_run_2piece(old.handle, C.byref(c2), None, None), ERR_INVALID_ARG, "poa_multi_run_2piece on a one-piece batch")
        with pytest.raises(_lib.PoaError) as ei:
            mb.run(engine.GapAffine(4, 2, 6))
        assert ei.value.code == ERR_INVALID_ARG
        with pytest.raises(_lib.PoaError) as ei:
            old.run(_gc2(engine, COSTS))
        assert ei.value.code == ERR_INVALID_ARG
        refused(L.poa_multi_run_2piece(mb.handle, C.byref(bad), None, None), ERR_INVALID_ARG, "extend1 < extend2, run")
        refused(one_shot(bad, None), ERR_INVALID_ARG, "extend1 < extend2, one-shot")
        refused(L.poa_multi_fetch(mb.handle, engine._p(score), None, None, 0, None, None), ERR_INVALID_ARG, "still no run")
        # both batches are still usable, each under its own model
        mb.run(_gc2(engine, COSTS))
        got = mb.fetch()
        assert len(got.score) == n
        _same(got, _run(engine, graphs, seqs, COSTS), "after the refusals")
        old.run(engine.GapAffine(4, 2, 6))
        assert len(old.fetch().score) == n
        # the old entry points keep refusing the two-piece mode
        refused(L.poa_multi_run(old.handle, C.byref(c1), C.byref(engine.make_config("checkpoint2")), None), ERR_UNSUPPORTED, "poa_multi_run, checkpoint2")
    finally:
        mb.close()
        old.close()
    refused(create(None, np.array([1, n0, n], np.uint64)), ERR_INVALID_ARG, "graph_qoff[0] != 0")
    refused(create(None, np.array([0, n, n0], np.uint64)), ERR_INVALID_ARG, "graph_qoff decreasing")
    refused(create(None, gq, (C.c_void_p * 2)(handles[0], None)), ERR_INVALID_ARG, "null graph")
    # graph_qoff[n_graphs] IS the query count for the C ABI; the binding, which knows the count, refuses a mismatch
    with pytest.raises(ValueError):
        engine.MultiGraphBatch(graphs, graph_qoff=np.array([0, n0, n - 1], np.uint64), qseq=qseq, qoff=qoff, two_piece=True)
