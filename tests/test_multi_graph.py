"""Multi-graph checkpointed batches (poa_multi_*): the queries of many graphs in one run.

Every comparison has two references: the oracle's dense restatement and walk of every query against its own graph (score and
alignment), and the per-graph one-shot poa_align_batch_ex in POA_MODE_CHECKPOINT of the same library on the same inputs (score,
flags, pairs and the per-query pair counts).  Equal, not close."""
import ctypes as C
import os

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7
EMPTY_GRAPH = 0x20
ACGT = np.frombuffer(b"ACGT", np.uint8)

# The widest query of the mixed batch has 1100 symbols: pitch 1152.  LAUNCH_CKPT takes, for a chunk whose largest pitch is above
# 512, Q = 2 with u16 cells and Q = 4 with u32 cells; a strip is 64 lanes x PlaneIO<T>::K x Q columns — 64 x 8 x 2 = 1024 (u16,
# K = 8) or 64 x 4 x 4 = 1024 (u32, K = 4).  1101 columns are two strips under either: the strip carries are exercised.
STRIP_COLUMNS = 1024
LONG = 1100


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


_MIXED = None


def _mixed():
    """graphs (the bubble graph is listed twice: the same object, so the same handle), queries per graph."""
    global _MIXED
    if _MIXED is None:
        rng = np.random.default_rng(20)
        b = GraphBuilder()
        chain_seq = rng.choice(ACGT, 20)
        b.add_path(chain_seq)
        chain = b.finish()
        long_q = np.concatenate([chain_seq[:10], rng.choice(ACGT, LONG - 20), chain_seq[10:]])
        assert len(long_q) == LONG and LONG + 1 > STRIP_COLUMNS
        chain_qs = [np.zeros(0, np.uint8), chain_seq[3:4], chain_seq[5:7], W.mutate(rng, np.concatenate([chain_seq, chain_seq[:10]]), 0.1, 0.05, 0.05), long_q]
        bubble, gfa, empty = _bubble_graph(), _gfa_graph(), GraphBuilder().finish()
        b = GraphBuilder()
        b.add_path(rng.choice(ACGT, 9))
        idle = b.finish()
        walks = lambda g, n, p: [W.random_walk_query(rng, g, p) for _ in range(n)]
        graphs = [chain, bubble, gfa, empty, idle, bubble]
        seqs = [chain_qs, walks(bubble, 5, 0.2) + [rng.choice(ACGT, 40)], walks(gfa, 6, 0.25) + [rng.choice(ACGT, 48), rng.choice(ACGT, 1)],
                [rng.choice(ACGT, 4), np.zeros(0, np.uint8), rng.choice(ACGT, 1)], [], walks(bubble, 3, 0.1) + [np.zeros(0, np.uint8)]]
        assert all(g.n <= 40 for g in graphs) and all(len(q) <= 48 for s in seqs for q in s if len(q) != LONG)
        _MIXED = (graphs, seqs)
    return _MIXED


_ORACLE = {}


def _oracle_case(oracle, key, graphs, seqs, costs):
    """Per query (score, raw alignment) by the oracle, computed once per (batch, costs)."""
    k = (key, costs)
    if k not in _ORACLE:
        out = []
        for g, qs in zip(graphs, seqs):
            if not qs:
                continue
            if g.n == 2:   # no real nodes: the aligner's shortcut (mod.rs:124-142), score 4 * len, no alignment
                out += [(4 * len(q), []) for q in qs]
                continue
            qseq, qoff = pack_queries(qs)
            D = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq, qoff, oracle.Costs(*costs), threads=4)
            out += [(int(D["score"][i]), oracle.batch_alignment(D, i)) for i in range(len(qs))]
        _ORACLE[k] = out
    return _ORACLE[k]


def _costs(engine, m, o, e):
    return engine.GapAffine(m, e, o)   # reference ctor order: (mismatch, extend, open)


_PER_GRAPH = {}


def _per_graph(engine, key, graphs, seqs, costs, **tune):
    """poa_align_batch_ex in POA_MODE_CHECKPOINT, graph by graph: (score, flags, per-query pair counts, pairs) concatenated."""
    k = (key, costs, tuple(sorted(tune.items())))
    if k not in _PER_GRAPH:
        from poasta_amd import _lib
        cfg = engine.make_config("checkpoint", **tune)
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


def _check(res, oracle_case, per_graph, what):
    score, flags, counts, pairs = per_graph
    assert np.array_equal(res.score, score), ("score", what)
    assert np.array_equal(res.flags, flags), ("flags", what)
    assert np.array_equal(np.diff(res.pair_off.astype(np.int64)), counts), ("pair counts", what)
    assert np.array_equal(res.pairs, pairs), ("pairs", what)
    assert len(res.score) == len(oracle_case)
    for i, (s, aln) in enumerate(oracle_case):
        assert int(res.score[i]) == s, ("oracle score", what, i)
        assert res.raw_alignment(i) == aln, ("oracle alignment", what, i)


def _run(engine, graphs, seqs, costs, workspace_bytes=0, run_cfg=None, create_cfg=None):
    mb = engine.MultiGraphBatch(graphs, seqs, workspace_bytes=workspace_bytes, config=create_cfg)
    try:
        mb.run(_costs(engine, *costs), None, run_cfg if run_cfg is not None else create_cfg)
        res = mb.fetch()
        res.workspace_bytes = mb.workspace_bytes()
    finally:
        mb.close()
    return res


def _terms(engine, graphs, seqs, segment_rows=0):
    """Per query: (graph index, bytes it holds) — rows_per_query of its graph's own plan x pitch x 4 + 256."""
    out = []
    for gi, (g, qs) in enumerate(zip(graphs, seqs)):
        _, rpq = engine._device_graph(g).checkpoint_plan(segment_rows)
        out += [(gi, rpq * (((len(q) + 1 + 63) // 64) * 64) * 4 + 256) for q in qs]
    return out


# ---- 1. mixed small graphs in one run ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_mixed_graphs_one_run(engine, oracle):
    graphs, seqs = _mixed()
    costs = (4, 6, 2)
    res = _run(engine, graphs, seqs, costs)
    _check(res, _oracle_case(oracle, "mixed", graphs, seqs, costs), _per_graph(engine, "mixed", graphs, seqs, costs), "one run")
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
    al = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, *costs)))
    one = al.align_multi(graphs, seqs)
    for a, b in ((one.score, res.score), (one.flags, res.flags), (one.pair_off, res.pair_off), (one.pairs, res.pairs)):
        assert np.array_equal(a, b)


# ---- 2. several segments ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_several_segments(engine, oracle):
    graphs, seqs = _mixed()
    costs = (4, 6, 2)
    k = 7
    n_seg = [len(engine._device_graph(g).checkpoint_plan(k)[0]) - 1 for g in graphs]
    assert sum(s >= 3 for s in n_seg[:3]) >= 2 and n_seg[3] == 1, n_seg   # chain, bubble, GFA graph: 3 or more; the empty graph: one
    cfg = engine.make_config("checkpoint", ckpt_rows=k)
    res = _run(engine, graphs, seqs, costs, create_cfg=cfg)
    _check(res, _oracle_case(oracle, "mixed", graphs, seqs, costs), _per_graph(engine, "mixed", graphs, seqs, costs, ckpt_rows=k), "ckpt_rows 7")
    assert res.workspace_bytes == sum(t for _, t in _terms(engine, graphs, seqs, k))


# ---- 3. chunk boundaries ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_chunk_boundaries(engine, oracle):
    graphs, seqs = _mixed()
    costs = (4, 6, 2)
    total, largest = engine.multi_footprint(graphs, seqs)
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
    _check(res, _oracle_case(oracle, "mixed", graphs, seqs, costs), _per_graph(engine, "mixed", graphs, seqs, costs), "chunked")
    whole = _run(engine, graphs, seqs, costs)
    for a, b in ((whole.score, res.score), (whole.flags, res.flags), (whole.pair_off, res.pair_off), (whole.pairs, res.pairs)):
        assert np.array_equal(a, b)
    # u32 cells under the same cap, and a cap below the largest query (raised to it)
    wide = _run(engine, graphs, seqs, costs, workspace_bytes=1, run_cfg=engine.make_config("checkpoint", planes=32))
    assert wide.stats["n_chunks"] >= len(firsts) and wide.workspace_bytes == largest
    assert np.array_equal(wide.score, whole.score) and np.array_equal(wide.pairs, whole.pairs) and np.array_equal(wide.flags, whole.flags)


# ---- 4. cell width ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_cell_width(engine, oracle):
    graphs, seqs = _mixed()
    narrow = _run(engine, graphs, seqs, (4, 6, 2))
    # open + extend x longest query + open + extend x shortest path: beyond 65534 for the chain graph alone (its 1100-symbol query)
    costs = (255, 40, 60)
    longest = [max(len(q) for q in qs) if qs else 0 for qs in seqs]
    assert 40 + 60 * longest[0] > 65534   # (whatever its shortest path)
    assert all(40 + 60 * l + 40 + 60 * g.n <= 65534 for g, l in list(zip(graphs, longest))[1:])   # (a shortest path has fewer than n nodes)
    wide = _run(engine, graphs, seqs, costs)
    assert wide.stats["plane_bytes"] == 2 * narrow.stats["plane_bytes"]   # the same cells stored, four bytes each: the whole run is u32
    _check(wide, _oracle_case(oracle, "mixed", graphs, seqs, costs), _per_graph(engine, "mixed", graphs, seqs, costs), "u32 by the bound")
    # u32 cells forced on the run that would be u16: identical results
    forced = _run(engine, graphs, seqs, (4, 6, 2), run_cfg=engine.make_config("checkpoint", planes=32))
    assert forced.stats["plane_bytes"] == 2 * narrow.stats["plane_bytes"]
    for a, b in ((forced.score, narrow.score), (forced.flags, narrow.flags), (forced.pair_off, narrow.pair_off), (forced.pairs, narrow.pairs)):
        assert np.array_equal(a, b)


# ---- 5. re-run and streams --------------------------------------------------------------------------------------------------------
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


@pytest.mark.gpu
def test_multi_rerun_on_a_stream(engine, oracle):
    graphs, seqs = _mixed()
    hip = _hip(engine)
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0 and s.value
    mb = engine.MultiGraphBatch(graphs, seqs)
    try:
        for costs in ((4, 6, 2), (1, 1, 1)):
            mb.run(_costs(engine, *costs), s.value)
            res = mb.fetch()
            assert res.stats["n_runs"] == 1
            _check(res, _oracle_case(oracle, "mixed", graphs, seqs, costs), _per_graph(engine, "mixed", graphs, seqs, costs), ("stream", costs))
        fresh = _run(engine, graphs, seqs, (1, 1, 1))
        for a, b in ((fresh.score, res.score), (fresh.flags, res.flags), (fresh.pair_off, res.pair_off), (fresh.pairs, res.pairs)):
            assert np.array_equal(a, b)
        assert mb.stats()["n_runs"] == 0 and all(mb.device_results().values())
    finally:
        mb.close()
        hip.hipStreamDestroy(s)


# ---- 6. random sweep --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_random_sweep(engine, oracle):
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
        _check(res, _oracle_case(oracle, "sweep", graphs, seqs, costs), _per_graph(engine, "sweep", graphs, seqs, costs), ("sweep", costs))
        flagged += int((res.flags != 0).sum())
    assert flagged > 0   # (the certificate's bits do occur: they are compared, not just zero)


# ---- 7. contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_contract(engine):
    from poasta_amd import _lib
    L = _lib.lib()
    graphs, seqs = _mixed()
    graphs, seqs = graphs[1:3], seqs[1:3]
    handles = (C.c_void_p * 2)(*[engine._device_graph(g).handle for g in graphs])
    qseq, qoff = pack_queries([q for s in seqs for q in s])
    n0, n = len(seqs[0]), len(qoff) - 1
    gq = np.array([0, n0, n], np.uint64)
    c = _costs(engine, 4, 6, 2)._c()
    score = np.zeros(n, np.uint32)

    def create(cfg, gqoff=gq, hs=handles):
        h = C.c_void_p()
        rc = L.poa_multi_create(hs, 2, engine._p(gqoff), 0, engine._p(qseq), engine._p(qoff), C.byref(cfg) if cfg is not None else None, 0, C.byref(h))
        if rc == 0:
            L.poa_multi_destroy(h)
        return rc

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert L.poa_last_error() != b"", what

    assert create(None) == 0 and create(engine.make_config("checkpoint")) == 0
    mb = engine.MultiGraphBatch(graphs, seqs)
    try:
        for mode in ("dense", "exact", "hybrid", "score", "checkpoint2"):
            cfg = engine.make_config(mode)
            refused(create(cfg), ERR_UNSUPPORTED, ("create", mode))
            refused(L.poa_multi_run(mb.handle, C.byref(c), C.byref(cfg), None), ERR_UNSUPPORTED, ("run", mode))
            refused(L.poa_align_multi(handles, 2, engine._p(gq), C.byref(c), C.byref(cfg), engine._p(qseq), engine._p(qoff), engine._p(score),
                                      None, None, 0, None, None, 0), ERR_UNSUPPORTED, ("one-shot", mode))
        ef = engine.make_config("checkpoint", aln_type=engine.AlignmentType.EndsFree())
        refused(create(ef), ERR_UNSUPPORTED, "ends-free, create")
        refused(L.poa_multi_run(mb.handle, C.byref(c), C.byref(ef), None), ERR_UNSUPPORTED, "ends-free, run")
        refused(L.poa_multi_fetch(mb.handle, engine._p(score), None, None, 0, None, None), ERR_INVALID_ARG, "fetch before run")
        mb.run(_costs(engine, 4, 6, 2))   # the batch is still usable
        assert len(mb.fetch().score) == n
    finally:
        mb.close()
    refused(create(None, np.array([1, n0, n], np.uint64)), ERR_INVALID_ARG, "graph_qoff[0] != 0")
    refused(create(None, np.array([0, n, n0], np.uint64)), ERR_INVALID_ARG, "graph_qoff decreasing")
    refused(create(None, gq, (C.c_void_p * 2)(handles[0], None)), ERR_INVALID_ARG, "null graph")
    # graph_qoff[n_graphs] IS the query count for the C ABI; the binding, which knows the count, refuses a mismatch
    with pytest.raises(ValueError):
        engine.MultiGraphBatch(graphs, graph_qoff=np.array([0, n0, n - 1], np.uint64), qseq=qseq, qoff=qoff)
