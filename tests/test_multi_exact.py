"""Exact multi-graph batches (poa_multi_*_exact): the replay of the reference's search for the queries of many graphs in one run.

Everything is bit-exact.  Two references per query: the oracle's astar_align of the query against its own graph (score, alignment,
num_queued / num_visited / num_pruned), and the single-graph calls of the same library in the same mode, graph by graph
(poa_align_batch_ex: score, flags, pairs, pair counts; a ResidentBatch: the four search-counter words)."""
import ctypes as C
import os

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

from test_multi_graph import ACGT, EMPTY_GRAPH, ERR_INVALID_ARG, ERR_UNSUPPORTED, _bubble_graph, _costs

pytestmark = pytest.mark.gpu
START_QUIRK, REF_PANIC, OVERFLOW = 2, 4, 0x40
QPC = 3.0   # queue entries per cell: enough for every search below under either heuristic


def _path(seq):
    b = GraphBuilder()
    b.add_path(np.frombuffer(seq, np.uint8) if isinstance(seq, bytes) else seq)
    return b.finish()


def _ladder(rng, bubbles=12):
    """An SNP ladder: `bubbles` times two alternative nodes between two backbone nodes; returns the graph and one path through it."""
    b = GraphBuilder()
    prev = b.add_node(int(ACGT[0]))
    path = [int(ACGT[0])]
    for i in range(bubbles):
        s0, s1, sj = int(ACGT[i & 3]), int(ACGT[(i + 2) & 3]), int(ACGT[(i + 1) & 3])
        a, c, j = b.add_node(s0), b.add_node(s1), b.add_node(sj)
        b.add_edge(prev, a); b.add_edge(prev, c); b.add_edge(a, j); b.add_edge(c, j)
        path += [s0 if rng.random() < 0.5 else s1, sj]
        prev = j
    return b.finish(), np.array(path, np.uint8)


_MIXED = None


def _mixed():
    """graphs and queries per graph: a 3-row graph, a chain, an SNP ladder, the bypass graph of test_multi_graph (listed twice: one
    handle), an MSA-imported graph, a graph without real nodes.  Query lengths 0, 1, 2, 3, 63, 64 and about 200 all occur."""
    global _MIXED
    if _MIXED is None:
        rng = np.random.default_rng(31)
        tiny = _path(b"A")
        chain_seq = rng.choice(ACGT, 70)
        chain = _path(chain_seq)
        ladder, lpath = _ladder(rng)
        bypass = _bubble_graph()
        msa = W.PangenomePOA(ref_len=180, n_hap=5, p_snp=0.03, p_indel=0.02, max_indel=4, seed=9)
        empty = GraphBuilder().finish()
        assert tiny.n == 3 and empty.n == 2
        mut = lambda s: W.mutate(rng, s, 0.08, 0.04, 0.04)
        graphs = [tiny, chain, ladder, bypass, msa.graph, empty, bypass]
        seqs = [[np.zeros(0, np.uint8), ACGT[:1], ACGT[1:2], rng.choice(ACGT, 3)],
                [mut(chain_seq)[:63], np.resize(mut(chain_seq), 64), chain_seq[4:6], np.zeros(0, np.uint8), np.resize(mut(chain_seq), 200)],
                [mut(lpath), lpath[:3], mut(np.concatenate([lpath, lpath])), lpath[:1], np.resize(mut(lpath), 63)],
                [W.random_walk_query(rng, bypass, 0.2) for _ in range(3)] + [rng.choice(ACGT, 64), rng.choice(ACGT, 2)],
                msa.queries(3, length=150) + [np.resize(msa.queries(1, length=150)[0], 201), rng.choice(ACGT, 3)],
                [rng.choice(ACGT, 4), np.zeros(0, np.uint8)],
                [W.random_walk_query(rng, bypass, 0.1), np.zeros(0, np.uint8), rng.choice(ACGT, 1)]]
        seqs = [[np.ascontiguousarray(q, np.uint8) for q in qs] for qs in seqs]
        lens = {len(q) for qs in seqs for q in qs}
        assert {0, 1, 2, 3, 63, 64, 200, 201} <= lens and max(lens) <= 201
        _MIXED = (graphs, seqs)
    return _MIXED


HEUR = {"mingap": 1, "dijkstra": 0}
_ORACLE, _SINGLE, _DENSE = {}, {}, {}


def _oracle_case(oracle, key, graphs, seqs, costs, heur, prune):
    """Per query (status, score, raw alignment, (queued, visited, pruned)) by the oracle's search, once per case."""
    k = (key, costs, heur, prune)
    if k not in _ORACLE:
        out = []
        for g, qs in zip(graphs, seqs):
            if not qs:
                continue
            if g.n == 2:   # no real nodes: the aligner's shortcut (mod.rs:124-142), no search
                out += [(0, 4 * len(q), [], (0, 0, 0)) for q in qs]
                continue
            qseq, qoff = pack_queries(qs)
            A = oracle.OracleGraph.from_csr(g.as_dict()).astar_batch(qseq, qoff, oracle.Costs(*costs), oracle.H_MINGAP if heur == "mingap" else oracle.H_DIJKSTRA,
                                                                     prune, threads=4, want_counters=True)
            out += [(int(A["status"][i]), int(A["score"][i]), oracle.batch_alignment(A, i), tuple(int(v) for v in A["counters"][i])) for i in range(len(qs))]
        _ORACLE[k] = out
    return _ORACLE[k]


def _cfg(engine, mode, heur, prune, qpc=QPC):
    return engine.make_config(mode, HEUR[heur], prune, qpc)


def _single(engine, key, graphs, seqs, costs, mode, heur, prune, qpc=QPC):
    """The single-graph calls in the same mode, graph by graph: (score, flags, pair counts, pairs, counters) concatenated."""
    k = (key, costs, mode, heur, prune, qpc)
    if k not in _SINGLE:
        from poasta_amd import _lib
        c = _costs(engine, *costs)
        score, flags, counts, pairs, counters = [], [], [], [], []
        for g, qs in zip(graphs, seqs):
            if not qs:
                continue
            dg = engine._device_graph(g)
            qseq, qoff = pack_queries(qs)
            n = len(qs)
            cap = int(qoff[-1]) + n * g.n
            s, f, po, pr = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros((max(cap, 1), 2), np.uint32)
            cfg = _cfg(engine, mode, heur, prune, qpc)
            cc = c._c()
            _lib.check(_lib.lib().poa_align_batch_ex(dg.handle, C.byref(cc), C.byref(cfg), n, engine._p(qseq), engine._p(qoff), engine._p(s),
                                                     engine._p(pr), engine._p(po), cap, engine._p(f), None, 0))
            score.append(s); flags.append(f); counts.append(np.diff(po.astype(np.int64))); pairs.append(pr[:int(po[n])])
            if g.n == 2:
                counters.append(np.zeros((n, 4), np.uint32))
            else:
                rb = engine.ResidentBatch(g, qseq, qoff)
                try:
                    rb.run(c, None, _cfg(engine, mode, heur, prune, qpc))
                    counters.append(rb.search_counters().reshape(n, 4).copy())
                    rb.fetch()
                finally:
                    rb.close()
        _SINGLE[k] = tuple(np.concatenate(a) for a in (score, flags, counts, pairs, counters))
    return _SINGLE[k]


def _dense(engine, key, graphs, seqs, costs):
    """The dense kind on the same inputs."""
    k = (key, costs)
    if k not in _DENSE:
        mb = engine.MultiGraphBatch(graphs, seqs, dense=True)
        try:
            mb.run(_costs(engine, *costs))
            _DENSE[k] = mb.fetch()
        finally:
            mb.close()
    return _DENSE[k]


def _fetch(mb):
    res = mb.fetch()
    res.counters = mb.search_counters()
    res.launches = mb.launches()
    res.replay = mb.replay_info()      # poa_multi_replay_info: the replay's own record, `win` included
    assert [r["kernel"] for r in res.replay] == [{"lds": "wave_lds", "generic": "wave_generic"}[l["replay"]] for l in res.launches]
    assert all(r["lanes"] == 64 and r["waves"] == 1 and r["blocks"] == l["queries"] and r["ring_global"] == (l["replay"] == "generic")
               for r, l in zip(res.replay, res.launches))
    return res


def _run(engine, graphs, seqs, costs, mode="exact", heur="mingap", prune=True, qpc=QPC, workspace_bytes=0):
    mb = engine.MultiGraphBatch(graphs, seqs, exact=True, workspace_bytes=workspace_bytes, config=_cfg(engine, mode, heur, prune, qpc))
    try:
        mb.run(_costs(engine, *costs), config=_cfg(engine, mode, heur, prune, qpc))
        return _fetch(mb)
    finally:
        mb.close()


def _same(a, b, what):
    for name in ("score", "flags", "pair_off", "pairs", "counters"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (name, what)


def _check(engine, oracle, res, key, graphs, seqs, costs, mode, heur, prune, what, qpc=QPC):
    n = sum(len(s) for s in seqs)
    assert len(res.score) == n
    # the single-graph calls, graph by graph
    score, flags, counts, pairs, counters = _single(engine, key, graphs, seqs, costs, mode, heur, prune, qpc)
    assert np.array_equal(res.score, score), ("score", what)
    assert np.array_equal(res.flags, flags), ("flags", what)
    assert np.array_equal(np.diff(res.pair_off.astype(np.int64)), counts), ("pair_off", what)
    assert np.array_equal(res.pairs, pairs), ("pairs", what)
    assert np.array_equal(res.counters, counters), ("counters", what)
    # the oracle's search
    dense = _dense(engine, key, graphs, seqs, costs)
    case = _oracle_case(oracle, key, graphs, seqs, costs, heur, prune)
    assert len(case) == n
    replayed = 0
    for i, (status, s, aln, cnt) in enumerate(case):
        if mode == "hybrid" and int(dense.flags[i]) == 0:
            # not replayed: the dense kind's result untouched, counter words 0
            assert int(res.score[i]) == int(dense.score[i]) and int(res.flags[i]) == 0 and res.raw_alignment(i) == dense.raw_alignment(i), (what, i)
            assert not res.counters[i].any(), (what, i)
            # ... and a dense result without flags is the search's own
            assert status == 0 and int(res.score[i]) == s and res.raw_alignment(i) == aln, ("certified dense result", what, i)
            continue
        if int(dense.flags[i]) & EMPTY_GRAPH:
            assert int(res.flags[i]) == EMPTY_GRAPH and int(res.score[i]) == s and res.raw_alignment(i) == [] and not res.counters[i].any(), (what, i)
            continue
        replayed += 1
        assert not int(res.flags[i]) & OVERFLOW, (what, i)
        if status != 0:
            assert int(res.flags[i]) & REF_PANIC, ("the reference panics", what, i)
            continue
        assert int(res.flags[i]) & ~0x10 == 0, ("flags", what, i, int(res.flags[i]))   # (TRUNCATED: informational, as in test_exact_replay)
        assert int(res.score[i]) == s, ("oracle score", what, i)
        assert res.raw_alignment(i) == aln, ("oracle alignment", what, i)
        assert tuple(int(v) for v in res.counters[i][:3]) == cnt, ("oracle counters", what, i)
        assert 0 < int(res.counters[i][3]) <= cnt[0]
    assert res.stats["n_exact"] <= replayed
    return replayed


# ---- 1. mixed graphs in one run ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "hybrid"])
@pytest.mark.parametrize("heur,prune", [("mingap", True), ("mingap", False), ("dijkstra", True)], ids=["mingap_pruned", "mingap", "dijkstra"])
def test_multi_exact_mixed_graphs_one_run(engine, oracle, mode, heur, prune):
    graphs, seqs = _mixed()
    costs = (4, 6, 2)
    res = _run(engine, graphs, seqs, costs, mode, heur, prune)
    n = sum(len(s) for s in seqs)
    replayed = _check(engine, oracle, res, "mixed", graphs, seqs, costs, mode, heur, prune, (mode, heur, prune))
    assert res.stats["n_chunks"] == 1 and res.stats["n_queries"] == n
    assert [l["replay"] for l in res.launches] == ["lds"] and res.launches[0]["queries"] == n
    assert res.replay[0]["win"] in (64, 128) and res.replay[0]["graph_lds"] and res.replay[0]["lds_bytes"] >= 12 * res.replay[0]["win"]
    if mode == "exact":
        assert replayed == n - len(seqs[5])   # every query but those of the graph without real nodes
    else:
        dense = _dense(engine, "mixed", graphs, seqs, costs)
        assert 0 < replayed == int(np.count_nonzero(dense.flags & ~np.uint32(EMPTY_GRAPH)))


# ---- 2. slot strides --------------------------------------------------------------------------------------------------------------
def test_multi_exact_slot_strides(engine, oracle):
    """The ladder and the chain alternately, eight times, in one chunk, pruning on: graphs whose exit counts differ, so a slot
    addressed by its own graph's stride would overlap its neighbour and prune against that query's marks."""
    rng = np.random.default_rng(32)
    ladder, lpath = _ladder(rng, 14)
    chain_seq = rng.choice(ACGT, 70)
    chain = _path(chain_seq)
    graphs, seqs = [], []
    for k in range(8):
        graphs += [ladder, chain]
        seqs += [[W.mutate(rng, np.concatenate([lpath, lpath[::-1], lpath]), 0.1, 0.05, 0.05)], [W.mutate(rng, np.concatenate([chain_seq, chain_seq[:30]]), 0.1, 0.05, 0.05)]]
    costs = (4, 6, 2)
    case = _oracle_case(oracle, "strides", graphs, seqs, costs, "mingap", True)
    assert all(c[0] == 0 and c[3][2] > 0 for c in case), "reached marks must be set and used: num_pruned > 0 for every query"
    res = _run(engine, graphs, seqs, costs, "exact", "mingap", True)
    assert res.stats["n_chunks"] == 1
    for i, (status, s, aln, cnt) in enumerate(case):
        assert int(res.score[i]) == s and res.raw_alignment(i) == aln, i
        assert tuple(int(v) for v in res.counters[i][:3]) == cnt, i
    _check(engine, oracle, res, "strides", graphs, seqs, costs, "exact", "mingap", True, "strides")


# ---- 3. both instantiations, and a ring wider than 64 -----------------------------------------------------------------------------
def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize("env,kernel", [(dict(POA_EXACT_LDS="0"), "generic"), (dict(POA_WS_RING_GLOBAL="1"), "generic"), (dict(POA_WS_REC="0"), "lds"),
                                        (dict(POA_WS_LANES="1", POA_WS_ADAPT="0"), "lds")],
                         ids=["graph_in_global_memory", "ring_in_global_memory", "no_row_records", "one_entry_per_step"])
def test_multi_exact_both_instantiations(engine, oracle, env, kernel):
    graphs, seqs = _mixed()
    costs = (4, 6, 2)
    default = _run(engine, graphs, seqs, costs)
    assert [l["replay"] for l in default.launches] == ["lds"]
    res = _with_env(env, lambda: _run(engine, graphs, seqs, costs))
    assert [l["replay"] for l in res.launches] == [kernel]
    if "POA_WS_LANES" in env:   # the steps differ by construction: fewer entries tested per step
        res.counters[:, 3] = default.counters[:, 3]
    _same(res, default, env)
    _check(engine, oracle, res, "mixed", graphs, seqs, costs, "exact", "mingap", True, env)


def test_multi_exact_wide_ring(engine, oracle):
    """Costs 40 / 30 / 3: the descriptor ring's rule gives more than 64 priorities; both instantiations."""
    graphs, seqs = _mixed()
    costs = (40, 30, 3)
    x, o, e = costs
    # the win rule on the host, with a spread of 0 (a lower bound of every graph's)
    need = max(x, o + e) + o + 3 * e + 8
    assert need > 64
    res = _run(engine, graphs, seqs, costs)
    _check(engine, oracle, res, "mixed", graphs, seqs, costs, "exact", "mingap", True, "40/30/3")
    glob = _with_env(dict(POA_EXACT_LDS="0"), lambda: _run(engine, graphs, seqs, costs))
    assert [l["replay"] for l in glob.launches] == ["generic"] and [l["replay"] for l in res.launches] == ["lds"]
    win = res.replay[0]["win"]
    assert win >= 128 and win & (win - 1) == 0 and win >= need and glob.replay[0]["win"] == win
    assert res.replay[0]["lds_bytes"] >= 12 * win and glob.replay[0]["lds_bytes"] == 0 and not glob.replay[0]["graph_lds"]
    _same(glob, res, "40/30/3, generic pointers")


def test_multi_exact_refused_variants(engine):
    graphs, seqs = _mixed()
    from poasta_amd import _lib
    mb = engine.MultiGraphBatch(graphs, seqs, exact=True)
    dense = engine.MultiGraphBatch(graphs, seqs, dense=True)
    try:
        for env in (dict(POA_EXACT_IMPL="lane"), dict(POA_EXACT_IMPL="flat"), dict(POA_WS_GROUP="16")):
            with pytest.raises(_lib.PoaError) as ei:
                _with_env(env, lambda: mb.run(_costs(engine, 4, 6, 2)))
            assert ei.value.code == ERR_UNSUPPORTED and "poa_align_batch_ex" in str(ei.value)
        _with_env(dict(POA_EXACT_IMPL="wave", POA_WS_GROUP="64"), lambda: mb.run(_costs(engine, 4, 6, 2)))
        mb.fetch()
        # the kinds refuse each other's run calls
        c = _costs(engine, 4, 6, 2)._c()
        L = _lib.lib()
        for call, handle in ((L.poa_multi_run, mb.handle), (L.poa_multi_run_dense, mb.handle), (L.poa_multi_run_exact, dense.handle)):
            assert call(handle, C.byref(c), None, None) == ERR_INVALID_ARG
        c2 = engine.GapAffine2Piece(4, 2, 6, 1, 24)._c()
        assert L.poa_multi_run_2piece(mb.handle, C.byref(c2), None, None) == ERR_INVALID_ARG
        out = np.zeros(4 * mb.n, np.uint32)
        assert L.poa_multi_fetch_search_counters(dense.handle, engine._p(out)) == ERR_INVALID_ARG
        # costs that need u32 dense cells
        with pytest.raises(_lib.PoaError) as ei:
            _with_env(dict(POA_PLANES="32"), lambda: mb.run(_costs(engine, 4, 6, 2)))
        assert ei.value.code == ERR_UNSUPPORTED
    finally:
        mb.close()
        dense.close()


# ---- 4. chunks ----------------------------------------------------------------------------------------------------------------------
def test_multi_exact_chunks_and_reruns(engine, oracle):
    rng = np.random.default_rng(33)
    ladder, lpath = _ladder(rng)
    bypass = _bubble_graph()
    graphs = [ladder, bypass]
    seqs = [[W.mutate(rng, lpath, 0.1, 0.05, 0.05) for _ in range(4)], [W.random_walk_query(rng, bypass, 0.2) for _ in range(3)]]
    assert len({len(q) // 64 for q in seqs[0]}) == 1
    # a workspace that holds three of the seven queries: the first boundary falls inside the ladder's range
    _, largest = engine.multi_footprint(graphs, seqs, exact=True)
    first3 = engine.multi_footprint([ladder], [seqs[0][:3]], exact=True)
    slot_part = first3[0] - 3 * first3[1]   # (the three queries have one pitch: equal terms)
    assert slot_part > 0
    ws = 3 * first3[1]
    cfg = _cfg(engine, "exact", "mingap", True)
    mb = engine.MultiGraphBatch(graphs, seqs, exact=True, workspace_bytes=ws, config=cfg)
    try:
        mb.run(_costs(engine, 4, 6, 2), config=cfg)
        a = _fetch(mb)
        assert a.stats["n_chunks"] >= 2 and [l["queries"] for l in a.launches][0] == 3 and len(a.launches) == a.stats["n_chunks"]
        _check(engine, oracle, a, "chunks", graphs, seqs, (4, 6, 2), "exact", "mingap", True, "chunks")
        whole = _run(engine, graphs, seqs, (4, 6, 2))
        assert whole.stats["n_chunks"] == 1
        _same(a, whole, "chunked against one chunk")
        # the same batch again: other costs, the other mode, then the first run once more
        mb.run(_costs(engine, 40, 30, 3), config=cfg)
        _check(engine, oracle, _fetch(mb), "chunks", graphs, seqs, (40, 30, 3), "exact", "mingap", True, "chunks, 40/30/3")
        hy = _cfg(engine, "hybrid", "mingap", True)
        mb.run(_costs(engine, 4, 6, 2), config=hy)
        _check(engine, oracle, _fetch(mb), "chunks", graphs, seqs, (4, 6, 2), "hybrid", "mingap", True, "chunks, hybrid")
        mb.run(_costs(engine, 4, 6, 2), config=cfg)
        _same(_fetch(mb), a, "two runs of the same input")
    finally:
        mb.close()


# ---- 5. the reference's own sub-optimum ---------------------------------------------------------------------------------------------
def test_multi_exact_reproduces_the_start_quirk(engine):
    g = _path(b"GAAC")
    res = _run(engine, [g, g], [[b"AC"], [b"AC"]], (4, 6, 2))
    assert res.score.tolist() == [14, 14] and res.flags.tolist() == [0, 0]
    dense = _dense(engine, "gaac", [g, g], [[np.frombuffer(b"AC", np.uint8)]] * 2, (4, 6, 2))
    assert dense.score.tolist() == [10, 10] and all(int(f) & START_QUIRK for f in dense.flags)
    hy = _run(engine, [g, g], [[b"AC"], [b"AC"]], (4, 6, 2), mode="hybrid")
    assert hy.score.tolist() == [14, 14] and hy.stats["n_exact"] == 2


# ---- 6. overflow --------------------------------------------------------------------------------------------------------------------
def test_multi_exact_overflow_keeps_the_dense_result(engine, oracle):
    graphs, seqs = _mixed()
    costs = (4, 6, 2)
    res = _with_env(dict(POA_WS_CHUNK_CAP="6"), lambda: _run(engine, graphs, seqs, costs, qpc=1e-6))
    dense = _dense(engine, "mixed", graphs, seqs, costs)
    case = _oracle_case(oracle, "mixed", graphs, seqs, costs, "mingap", True)
    over = 0
    for i, (status, s, aln, cnt) in enumerate(case):
        if int(res.flags[i]) & OVERFLOW:
            over += 1
            assert int(res.flags[i]) == int(dense.flags[i]) | OVERFLOW and int(res.score[i]) == int(dense.score[i]), i
            assert res.raw_alignment(i) == dense.raw_alignment(i), i
        elif not int(dense.flags[i]) & EMPTY_GRAPH and status == 0:
            assert int(res.score[i]) == s and res.raw_alignment(i) == aln, i
    assert 0 < over < len(case)


# ---- 7. the Python surface ------------------------------------------------------------------------------------------------------------
def test_multi_exact_align_multi_equals_align_batch(engine):
    graphs, seqs = _mixed()
    for mode in ("hybrid", "exact"):
        al = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, 4, 6, 2)), mode=mode, queue_entries_per_cell=QPC)
        res = al.align_multi(graphs, seqs, mode=mode)
        at = 0
        for g, qs in zip(graphs, seqs):
            one = al.align_batch(g, qs)
            for i in range(len(qs)):
                assert int(res.score[at]) == int(one.score[i]) and int(res.flags[at]) == int(one.flags[i]), (mode, at)
                assert res.raw_alignment(at) == one.raw_alignment(i), (mode, at)
                at += 1
        assert at == len(res.score)
    empty = al.align_multi(graphs, [[] for _ in graphs], mode="exact")
    assert len(empty.score) == 0
