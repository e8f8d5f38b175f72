"""Dense multi-graph batches (poa_multi_*_dense): the queries of many graphs through the packed dense forward pass in one run.

Every comparison has three references, equal not close: the oracle's dense restatement and walk of every query against its own
graph (score and alignment), the per-graph one-shot poa_align_batch_ex in POA_MODE_DENSE of the same library (score, flags,
pairs and the per-query pair counts), and the checkpointed MultiGraphBatch on the same inputs."""
import ctypes as C

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

from test_multi_graph import ACGT, EMPTY_GRAPH, ERR_INVALID_ARG, ERR_UNSUPPORTED, LONG, _bubble_graph, _costs, _hip, _mixed, _oracle_case

pytestmark = pytest.mark.gpu
MID = 600   # replaces the 1100-symbol query of the mixed batch: pitch 640, one strip of the two-quad kernel


_MIXED_DENSE = None


def _mixed_dense():
    """test_multi_graph._mixed() with its 1100-symbol query replaced by one of 600 symbols."""
    global _MIXED_DENSE
    if _MIXED_DENSE is None:
        graphs, seqs = _mixed()
        rng = np.random.default_rng(22)
        seqs = [list(qs) for qs in seqs]
        at = [i for i, q in enumerate(seqs[0]) if len(q) == LONG]
        assert at == [len(seqs[0]) - 1]
        long_q = seqs[0][at[0]]
        seqs[0][at[0]] = np.concatenate([long_q[:10], rng.choice(ACGT, MID - 20), long_q[-10:]])
        assert len(seqs[0][at[0]]) == MID and max(len(q) for s in seqs for q in s) == MID
        _MIXED_DENSE = (graphs, seqs)
    return _MIXED_DENSE


def _without_widest(seqs):
    return [[q for q in qs if len(q) != MID] for qs in seqs]


_PER_GRAPH = {}


def _per_graph(engine, key, graphs, seqs, costs):
    """poa_align_batch_ex in POA_MODE_DENSE, graph by graph: (score, flags, per-query pair counts, pairs) concatenated."""
    k = (key, costs)
    if k not in _PER_GRAPH:
        from poasta_amd import _lib
        cfg = engine.make_config("dense")
        c = _costs(engine, *costs)._c()
        score, flags, counts, pairs = [], [], [], []
        for g, qs in zip(graphs, seqs):
            if not qs:
                continue
            dg = engine._device_graph(g)
            qseq, qoff = pack_queries(qs)
            n = len(qs)
            cap = int(qoff[-1]) + n * g.n
            s, f, po, pr = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros((max(cap, 1), 2), np.uint32)
            _lib.check(_lib.lib().poa_align_batch_ex(dg.handle, C.byref(c), C.byref(cfg), n, engine._p(qseq), engine._p(qoff), engine._p(s),
                                                     engine._p(pr), engine._p(po), cap, engine._p(f), None, 0))
            score.append(s); flags.append(f); counts.append(np.diff(po.astype(np.int64))); pairs.append(pr[:int(po[n])])
        _PER_GRAPH[k] = (np.concatenate(score), np.concatenate(flags), np.concatenate(counts), np.concatenate(pairs))
    return _PER_GRAPH[k]


_CKPT = {}


def _run(engine, graphs, seqs, costs, workspace_bytes=0, dense=True):
    mb = engine.MultiGraphBatch(graphs, seqs, workspace_bytes=workspace_bytes, dense=dense)
    try:
        mb.run(_costs(engine, *costs))
        res = mb.fetch()
        res.workspace_bytes = mb.workspace_bytes()
        res.launches = mb.launches() if dense else None
    finally:
        mb.close()
    return res


def _ckpt(engine, key, graphs, seqs, costs):
    """The checkpointed multi-graph batch on the same inputs, once per (batch, costs)."""
    k = (key, costs)
    if k not in _CKPT:
        _CKPT[k] = _run(engine, graphs, seqs, costs, dense=False)
    return _CKPT[k]


def _same(a, b, what):
    for name in ("score", "flags", "pair_off", "pairs"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (name, what)


def _check(engine, oracle, res, key, graphs, seqs, costs, what):
    """The three references."""
    score, flags, counts, pairs = _per_graph(engine, key, graphs, seqs, costs)
    assert np.array_equal(res.score, score), ("score", what)
    assert np.array_equal(res.flags, flags), ("flags", what)
    assert np.array_equal(np.diff(res.pair_off.astype(np.int64)), counts), ("pair counts", what)
    assert np.array_equal(res.pairs, pairs), ("pairs", what)
    # (the sweep batch is test_multi_random_sweep's own, graph for graph: one oracle run serves both files)
    oracle_case = _oracle_case(oracle, key if key == "sweep" else "dense/" + key, graphs, seqs, costs)
    assert len(res.score) == len(oracle_case)
    for i, (s, aln) in enumerate(oracle_case):
        assert int(res.score[i]) == s, ("oracle score", what, i)
        assert res.raw_alignment(i) == aln, ("oracle alignment", what, i)
    _same(res, _ckpt(engine, key, graphs, seqs, costs), ("checkpointed batch", what))


def _terms(engine, graphs, seqs):
    """Per query: (graph index, bytes it holds) — 2 x poa_graph_compact_elems + 256."""
    from poasta_amd import _lib
    out = []
    for gi, (g, qs) in enumerate(zip(graphs, seqs)):
        for q in qs:
            v = C.c_uint64(0)
            _lib.check(_lib.lib().poa_graph_compact_elems(engine._device_graph(g).handle, len(q), C.byref(v)))
            out.append((gi, 2 * int(v.value) + 256))
    return out


def _record(quads, queries):
    return {"kernel": "packed", "quads": quads, "fuse": False, "mw": False, "waves": 4, "code_fmt": 0, "tb_lanes": 64, "tb_depth": 32, "queries": queries}


# ---- 1. mixed small graphs in one run ---------------------------------------------------------------------------------------------
def test_multi_dense_mixed_graphs_one_run(engine, oracle):
    graphs, seqs = _mixed_dense()
    costs = (4, 6, 2)
    res = _run(engine, graphs, seqs, costs)
    _check(engine, oracle, res, "mixed", graphs, seqs, costs, "one run")
    n = sum(len(s) for s in seqs)
    terms = _terms(engine, graphs, seqs)
    assert res.stats["n_chunks"] == 1 and res.stats["n_queries"] == n
    assert res.launches == [_record(2, n)]   # the 600-symbol query: pitch 640, two quads
    assert res.stats["cells"] == sum(g.n * (len(q) + 1) for g, s in zip(graphs, seqs) for q in s)
    assert res.stats["plane_bytes"] == sum(t - 256 for _, t in terms)
    assert res.stats["ms_forward"] > 0 and res.stats["ms_traceback"] > 0
    assert res.workspace_bytes == sum(t for _, t in terms)
    # the queries of the graph without real nodes
    first = sum(len(s) for s in seqs[:3])
    assert len(seqs[3]) == 3
    for i, q in enumerate(seqs[3]):
        assert res.flags[first + i] == EMPTY_GRAPH and res.score[first + i] == 4 * len(q) and res.raw_alignment(first + i) == []
    # without the widest query every pitch is at most 512: one quad
    short = _without_widest(seqs)
    assert max(len(q) for s in short for q in s) <= 48
    res1 = _run(engine, graphs, short, costs)
    assert res1.launches == [_record(1, n - 1)]
    _check(engine, oracle, res1, "mixed-short", graphs, short, costs, "one quad")
    # the one-shot entry point through the aligner
    al = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, *costs)))
    _same(al.align_multi(graphs, seqs, mode="dense"), res, "one-shot")
    _same(al.align_multi(graphs, seqs), res, "one-shot, checkpointed")


# ---- 2. column edges --------------------------------------------------------------------------------------------------------------
def _chain(rng, n):
    b = GraphBuilder()
    seq = rng.choice(ACGT, n)
    b.add_path(seq)
    return b.finish(), seq


def test_multi_dense_column_edges(engine, oracle):
    rng = np.random.default_rng(23)
    chain, _ = _chain(rng, 28)
    bubble = _bubble_graph()
    assert chain.n == 30
    lens = (0, 1, 62, 63, 64, 510, 511, 512, 1023)

    def query(g, length):
        if length <= 20:
            return W.random_walk_query(rng, g, 0.2)[:length] if length else np.zeros(0, np.uint8)
        return rng.choice(ACGT, length)   # longer than the graph: random

    graphs = [chain, bubble]
    seqs = [[query(g, length) for length in lens] for g in graphs]
    assert [len(q) for q in seqs[0]] == list(lens) and [len(q) for q in seqs[1]] == list(lens)
    costs = (4, 6, 2)
    res = _run(engine, graphs, seqs, costs)
    assert res.launches == [_record(2, 2 * len(lens))]
    _check(engine, oracle, res, "edges", graphs, seqs, costs, "column edges")
    # pitch 512 is the last one-quad shape, pitch 576 the first two-quad one
    upto = lambda top: [[q for q in qs if len(q) <= top] for qs in seqs]
    r511, r512 = _run(engine, graphs, upto(511), costs), _run(engine, graphs, upto(512), costs)
    assert r511.launches == [_record(1, 2 * 7)] and r512.launches == [_record(2, 2 * 8)]
    _check(engine, oracle, r511, "edges-511", graphs, upto(511), costs, "pitch 512")
    _check(engine, oracle, r512, "edges-512", graphs, upto(512), costs, "pitch 576")


# ---- 3. four graphs in one block --------------------------------------------------------------------------------------------------
def _by_row_dag():
    """A random DAG that keeps more than half of its D rows, so that it stores them by row (no d_slot table): its compact
    planes hold rows x pitch D elements."""
    from poasta_amd import aligner, _lib
    for seed in range(200):
        g = W.random_dag(900 + seed, n_nodes=24, p_edge=0.45)
        v = C.c_uint64(0)
        _lib.check(_lib.lib().poa_graph_compact_elems(aligner._device_graph(g).handle, 63, C.byref(v)))
        if int(v.value) == g.n * 64 + g.n * 16 + g.n * 64:
            # all rows kept is also what a d_slot table of n entries would give: it is by row iff more than half are kept, and a
            # table is only built when at most half are — so the full D plane means "by row"
            return g
    raise AssertionError("no random DAG stores its D rows by row")


def test_multi_dense_four_graphs_in_one_block(engine, oracle):
    rng = np.random.default_rng(24)
    chain, _ = _chain(rng, 25)
    bubble, dag, empty = _bubble_graph(), _by_row_dag(), GraphBuilder().finish()
    assert max(len(bubble.predecessors(v)) for v in range(bubble.n)) >= 3 and empty.n == 2
    # one query per listing, the four graphs in turn: the four waves of a block belong to four graphs; the bubble graph is the
    # same object in every block, so one handle is listed eight times
    graphs = [chain, bubble, dag, empty] * 8
    seqs = [[W.random_walk_query(rng, g, 0.25) if g.n > 2 else rng.choice(ACGT, int(rng.integers(0, 9)))] for g in graphs]
    assert len(graphs) == 32 and all(g.n <= 40 for g in graphs)
    for costs in ((4, 6, 2), (1, 1, 1)):
        res = _run(engine, graphs, seqs, costs)
        assert res.launches == [_record(1, 32)]
        _check(engine, oracle, res, "four", graphs, seqs, costs, ("four graphs", costs))
        for k in range(3, 32, 4):
            assert res.flags[k] == EMPTY_GRAPH and res.score[k] == 4 * len(seqs[k][0])


# ---- 4. chunk boundaries ----------------------------------------------------------------------------------------------------------
def test_multi_dense_chunk_boundaries(engine, oracle):
    graphs, seqs = _mixed_dense()
    costs = (4, 6, 2)
    total, largest = engine.multi_footprint(graphs, seqs, dense=True)
    terms = _terms(engine, graphs, seqs)
    assert total == sum(t for _, t in terms) and largest == max(t for _, t in terms)
    cap = largest + 256   # just above the largest query
    # the plan: greedy in query order, a chunk ends in front of the first query that no longer fits
    firsts, used = [0], 0
    for i, (_, t) in enumerate(terms):
        if used + t > cap and i > firsts[-1]:
            firsts.append(i)
            used = 0
        used += t
    inside = [f for f in firsts[1:] if terms[f][0] == terms[f - 1][0]]
    between = [f for f in firsts[1:] if terms[f][0] != terms[f - 1][0]]
    assert len(firsts) >= 3 and inside and between, firsts
    res = _run(engine, graphs, seqs, costs, workspace_bytes=cap)
    assert res.stats["n_chunks"] == len(firsts)
    ends = firsts[1:] + [len(terms)]
    assert res.workspace_bytes == max(sum(t for _, t in terms[a:b]) for a, b in zip(firsts, ends)) <= cap
    lens = [len(q) for s in seqs for q in s]
    quads = [2 if max(lens[a:b]) + 1 > 512 else 1 for a, b in zip(firsts, ends)]
    assert 1 in quads and 2 in quads
    assert res.launches == [_record(q, b - a) for q, a, b in zip(quads, firsts, ends)]
    _check(engine, oracle, res, "mixed", graphs, seqs, costs, "chunked")
    whole = _run(engine, graphs, seqs, costs)
    _same(whole, res, "chunked against one chunk")
    # a cap below the largest query is raised to it
    tight = _run(engine, graphs, seqs, costs, workspace_bytes=1)
    assert tight.stats["n_chunks"] >= len(firsts) and tight.workspace_bytes == largest
    _same(tight, whole, "cap 1")


# ---- 5. random sweep --------------------------------------------------------------------------------------------------------------
def test_multi_dense_random_sweep(engine, oracle):
    graphs, seqs = [], []
    for seed in range(40):
        rng = np.random.Generator(np.random.PCG64(7000 + seed))
        alpha = b"AC" if seed % 2 else b"ACGT"
        g = W.random_dag(seed, n_nodes=int(rng.integers(3, 30)), p_edge=float(rng.choice([0.15, 0.3])), alphabet=alpha)
        graphs.append(g)
        seqs.append([W.random_walk_query(rng, g, 0.3, alpha) for _ in range(int(rng.integers(1, 9)))])
    flagged = 0
    for costs in ((4, 6, 2), (1, 1, 1)):
        res = _run(engine, graphs, seqs, costs)
        _check(engine, oracle, res, "sweep", graphs, seqs, costs, ("sweep", costs))
        flagged += int((res.flags != 0).sum())
    assert flagged > 0   # (the certificate's bits do occur: they are compared, not just zero)


# ---- 6. re-run and contract -------------------------------------------------------------------------------------------------------
def test_multi_dense_rerun_and_contract(engine, oracle):
    from poasta_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(25)
    graphs, seqs = _mixed_dense()
    seqs = [list(qs) for qs in seqs]
    seqs[1] = seqs[1] + [rng.choice(ACGT, 1000)]   # with gap_extend 70 its insertion alone costs more than a u16 cell holds
    hip = _hip(engine)
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0 and s.value
    n = sum(len(qs) for qs in seqs)
    score = np.zeros(n, np.uint32)

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert L.poa_last_error() != b"", what

    mb = engine.MultiGraphBatch(graphs, seqs, dense=True)
    ck = engine.MultiGraphBatch(graphs, seqs)
    try:
        refused(L.poa_multi_fetch(mb.handle, engine._p(score), None, None, 0, None, None), ERR_INVALID_ARG, "fetch before run")
        refused(L.poa_multi_last_launch(mb.handle, 0, (C.c_uint32 * 8)()), ERR_INVALID_ARG, "last launch before run")
        # the cell width: the batch holds u16 cells only
        wide = _costs(engine, 255, 40, 70)._c()
        assert 40 + 70 * 1000 > 65534
        refused(L.poa_multi_run_dense(mb.handle, C.byref(wide), None, None), ERR_UNSUPPORTED, "u32 by the bound")
        assert b"poa_multi_create" in L.poa_last_error()
        c = _costs(engine, 4, 6, 2)._c()
        p32 = engine.make_config("dense", planes=32)
        refused(L.poa_multi_run_dense(mb.handle, C.byref(c), C.byref(p32), None), ERR_UNSUPPORTED, "planes=32")
        for mode in ("exact", "hybrid", "score", "checkpoint", "checkpoint2"):
            cfg = engine.make_config(mode)
            refused(L.poa_multi_run_dense(mb.handle, C.byref(c), C.byref(cfg), None), ERR_UNSUPPORTED, ("run", mode))
        ef = engine.make_config("dense", aln_type=engine.AlignmentType.EndsFree())
        refused(L.poa_multi_run_dense(mb.handle, C.byref(c), C.byref(ef), None), ERR_UNSUPPORTED, "ends-free, run")
        # kind mismatches between run functions and batches
        c2 = engine.GapAffine2Piece(4, 2, 6, 1, 24)._c()
        refused(L.poa_multi_run(mb.handle, C.byref(c), None, None), ERR_INVALID_ARG, "poa_multi_run on a dense batch")
        refused(L.poa_multi_run_2piece(mb.handle, C.byref(c2), None, None), ERR_INVALID_ARG, "poa_multi_run_2piece on a dense batch")
        refused(L.poa_multi_run_dense(ck.handle, C.byref(c), None, None), ERR_INVALID_ARG, "poa_multi_run_dense on a checkpointed batch")
        refused(L.poa_multi_last_launch(ck.handle, 0, (C.c_uint32 * 8)()), ERR_INVALID_ARG, "last launch on a checkpointed batch")
        refused(L.poa_multi_fetch(mb.handle, engine._p(score), None, None, 0, None, None), ERR_INVALID_ARG, "fetch after refused runs")
        # the batch then runs: twice, with other costs, on a non-default stream
        for costs in ((4, 6, 2), (1, 1, 1)):
            mb.run(_costs(engine, *costs), s.value)
            res = mb.fetch()
            assert res.stats["n_runs"] == 1 and res.stats["n_chunks"] == 1
            _check(engine, oracle, res, "contract", graphs, seqs, costs, ("stream", costs))
        fresh = _run(engine, graphs, seqs, (1, 1, 1))
        _same(fresh, res, "second run against a fresh batch")
        assert mb.stats()["n_runs"] == 0 and all(mb.device_results().values())
    finally:
        mb.close()
        ck.close()
        hip.hipStreamDestroy(s)


# ---- 7. assign, then align --------------------------------------------------------------------------------------------------------
def test_multi_dense_assign_and_align(engine):
    rng = np.random.default_rng(26)
    graphs = [_chain(rng, 30)[0], _bubble_graph(), W.random_dag(5, n_nodes=20, p_edge=0.3), W.random_dag(6, n_nodes=26, p_edge=0.2)]
    seqs = [W.random_walk_query(rng, graphs[k % 4], 0.15) for k in range(16)]
    al = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, 4, 6, 2)))
    a0, r0 = al.assign_and_align(graphs, seqs)
    a1, r1 = al.assign_and_align(graphs, seqs, mode="dense")
    assert sorted(a0) == sorted(a1)
    for k in a0:
        assert np.array_equal(a0[k], a1[k]), k
    assert len(set(a0["graph"].tolist())) >= 2
    _same(r1, r0, "assign_and_align")
    two = engine.PoastaAligner(engine.Affine2PieceMinGapCost(engine.GapAffine2Piece(4, 2, 6, 1, 24)))
    with pytest.raises(ValueError):
        two.assign_and_align(graphs, seqs, mode="dense")
