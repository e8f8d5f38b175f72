"""Exact replay: parity at every launch the launcher can pick, at the smallest shapes that pick it.

replay_chunk (poa_engine.hip) chooses between the lane kernel, the wave search (all in LDS, several queries per wave, generic
pointers) and the flat search; replay_wave places the graph arrays, the per-row records and the descriptor ring by three LDS
budgets and switches to the persistent schedule when the chunk has more blocks than are resident at once.  Every test here

  * compares score, flags and raw_alignment of EVERY query with the oracle's search (astar_batch), asserts that the oracle
    aligned every query it was sent (no "reference panics" escape) and that POA_FLAG_EXACT_OVERFLOW (0x40) is not set;
  * reads back what was launched (ResidentBatch.replay_info, poa_batch_replay_info) and compares it with `predict_wave`, a
    restatement of replay_wave's rule, so a test that claims a path proves that it took it.

The ring's width comes from exact_replay_win (poa_multi_plan.hpp), restated in test_exact_replay.py and checked there on the CPU.
"""
import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

from test_exact_replay import harness, _chain, _graph_spread, _win_jump, _win_rule, _p, WIN_COSTS   # noqa: F401 (harness: fixture)

U, INC, EXC = 0, 1, 2
LDS_CAP = 160 * 1024        # LDS bytes one workgroup may hold on gfx950 (hipDeviceAttributeMaxSharedMemoryPerBlock)
GRAPH_RING_BUDGET = 80 * 1024    # replay_wave: graph arrays + descriptor rings of a block
RECORDS_BUDGET = 150 * 1024      # ... + the per-row records
RING_BYTES_PER_PRIORITY = 12     # three stacks' descriptors per priority and query
ROW_REC_BYTES, NODE_BUBBLE_BYTES = 32, 12   # sizeof(FlatGraph::RowRec), sizeof(FlatGraph::NodeBubble)


def _pad16(b):
    return (b + 15) & ~15


def exact_lds_bytes(n_rows, n_succ, n_nbm):
    """poa_exact_kernel.hpp: symbols, two CSR offset arrays, successors, dist_min / dist_max / exit_idx, node-bubble entries."""
    return _pad16(n_rows) + 2 * _pad16(4 * (n_rows + 1)) + _pad16(4 * n_succ) + 3 * _pad16(4 * n_rows) + _pad16(NODE_BUBBLE_BYTES * n_nbm)


def _n_nbm(X, g):
    n = g.n
    dmin, dmax, ex = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    off, nbm = np.zeros(n + 1, np.uint32), np.zeros((1, 3), np.uint32)
    assert X.exact_host_bubbles(g.n, g.start, g.end, _p(g.symbol), _p(g.succ_off), _p(g.succ), _p(g.pred_off), _p(g.pred),
                                _p(dmin), _p(dmax), _p(ex), _p(off), _p(nbm), 1) == 0
    return int(off[n])


def graph_lds_bytes(X, g):
    return exact_lds_bytes(g.n, len(g.succ), _n_nbm(X, g))


def predict_wave(graph_lds, n_rows, win, group=64, waves=None, ring_global=False, exact_lds=True, rec=True):
    """replay_wave's rule.  group / waves / ring_global / exact_lds / rec: the POA_WS_GROUP, POA_WS_WAVES, POA_WS_RING_GLOBAL,
    POA_EXACT_LDS and POA_WS_REC overrides (None / default: unset).  Returns what replay_info reports of the placement."""
    wpb = waves or 16
    budget = min(LDS_CAP, GRAPH_RING_BUDGET)
    while True:
        rb = wpb * (64 // group) * win * RING_BYTES_PER_PRIORITY
        ring_lds = rb <= budget and not ring_global
        stage = graph_lds + (rb if ring_lds else 0) <= budget and exact_lds
        if group == 64 or (ring_lds and stage):
            break
        if wpb > 2 and not waves:     # several queries per wave need everything in LDS: fewer waves first, then fewer queries
            wpb //= 2
        else:
            group *= 2
            if not waves:
                wpb = 16
    ring_bytes = rb if ring_lds else 0
    rec_lds = 0
    if group == 64 and stage and ring_lds and rec and n_rows < 0xFFFF:
        r = _pad16(ROW_REC_BYTES * n_rows)
        if graph_lds + r + ring_bytes <= min(LDS_CAP, RECORDS_BUDGET):
            rec_lds = r
    kernel = "wave_groups" if group != 64 else ("wave_lds" if (stage and ring_lds) else "wave_generic")
    return {"kernel": kernel, "win": win, "lanes": group, "waves": wpb, "graph_lds": bool(stage), "rec_lds": rec_lds > 0,
            "ring_global": not ring_lds, "lds_bytes": (graph_lds if stage else 0) + rec_lds + ring_bytes}


def _check_info(info, want, count, static=False):
    """One chunk's record against the prediction; the schedule against the record's own `resident` (the occupancy the
    runtime reports is the one input the rule has that a test cannot restate)."""
    got = {k: info[k] for k in want}
    assert got == want, (got, want)
    per_block = info["waves"] * (64 // info["lanes"])
    n_blocks = (count + per_block - 1) // per_block
    if info["lanes"] == 64 and not static:
        assert info["resident"] > 0
        assert info["persistent"] == (n_blocks > info["resident"]), info
        assert info["blocks"] == min(n_blocks, info["resident"]), info
    else:
        assert not info["persistent"] and info["blocks"] == n_blocks, info


def _bound(engine, b):
    return engine.Bound.Unbounded if b[0] == U else (engine.Bound.Included(b[1]) if b[0] == INC else engine.Bound.Excluded(b[1]))


NAMES = ("qry_free_begin", "qry_free_end", "graph_free_begin", "graph_free_end")


def _oracle_batch(oracle, g, qseq, qoff, costs, mingap, pruning, bounds, counters=False):
    og = oracle.OracleGraph.from_csr(g.as_dict())
    heur = oracle.H_MINGAP if mingap else oracle.H_DIJKSTRA
    if bounds is None:
        A = og.astar_batch(qseq, qoff, oracle.Costs(*costs), heur, pruning, threads=4, want_counters=counters)
    else:
        spec = oracle.ends_free(*[bounds.get(k, (U, 0)) if bounds.get(k, (U, 0))[0] else 0 for k in NAMES])
        with oracle.alignment_type(spec):
            A = og.astar_batch(qseq, qoff, oracle.Costs(*costs), heur, pruning, threads=4, want_counters=counters)
    assert (np.asarray(A["status"]) == 0).all(), "the oracle must align every query of these inputs"
    return A


def _replay(engine, g, qseq, qoff, costs, mingap=True, pruning=True, bounds=None, mode="exact", qepc=4.0, workspace_bytes=0,
            counters=False, **tune):
    """One resident run through poa_batch_run_ex.  bounds: None (Global) or a dict of (kind, value) keyed like
    AlignmentType::EndsFree's fields (a missing one: Unbounded).  Returns (result, replay_info, search counters or None)."""
    x, o, e = costs
    at = engine.AlignmentType.Global if bounds is None else engine.AlignmentType.EndsFree(**{k: _bound(engine, bounds.get(k, (U, 0))) for k in NAMES})
    cfg = engine.make_config(mode, heuristic=1 if mingap else 0, pruning=pruning, queue_entries_per_cell=qepc, aln_type=at, **tune)
    rb = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=workspace_bytes)
    try:
        rb.run(engine.GapAffine(x, e, o), None, cfg)
        sc = rb.search_counters() if counters else None
        res = rb.fetch()
        info = rb.replay_info()
        assert len(info) == res.stats["n_chunks"]
    finally:
        rb.close()
    return res, info, sc


def _same_as_oracle(oracle, res, A, n, ends_free, what=""):
    """Every query: no overflow, no flag but TRUNCATED (ends-free: informational), the oracle's score and alignment."""
    compared = 0
    for i in range(n):
        f = int(res.flags[i])
        assert f & 0x40 == 0, ("POA_FLAG_EXACT_OVERFLOW", what, i)
        assert f & ~(0x10 if ends_free else 0) == 0, ("flags", what, i, f)
        assert int(res.score[i]) == int(A["score"][i]), ("score", what, i)
        assert res.raw_alignment(i) == oracle.batch_alignment(A, i), ("alignment", what, i)
        compared += 1
    assert compared == n == len(res.score)


def _bubble_dag(n, snps, deletion=None):
    """A chain of n nodes with one SNP bubble at each of `snps` and, optionally, one deletion edge: n + len(snps) nodes."""
    rng = np.random.Generator(np.random.PCG64(61))
    alpha = np.frombuffer(b"ACGT", np.uint8)
    sym = alpha[rng.integers(0, 4, n)]
    b = GraphBuilder()
    ids = b.add_path(sym)
    for p in snps:
        alt = b.add_node(alpha[(alpha.tolist().index(int(sym[p])) + 1) % 4])
        b.add_edge(ids[p - 1], alt)
        b.add_edge(alt, ids[p + 1])
    if deletion:
        b.add_edge(ids[deletion[0]], ids[deletion[1]])
    return b.finish(), sym


FREE_BEGIN_SPANS = [dict(),                                                         # all Unbounded
                    dict(qry_free_end=(INC, 0), graph_free_end=(INC, 0)),           # free begin, Included(0) ends
                    dict(qry_free_end=(EXC, 1), graph_free_end=(EXC, 1)),           # free begin only: Excluded(1) frees nothing
                    dict(graph_free_begin=(INC, 0))]                                # control: bounded begin, free ends


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [28, 32, 40, 300, "dag60"], ids=["chain28_control", "chain32", "chain40", "chain300_ring_global", "dag60_bubbles"])
def test_gpu_free_graph_begin_beyond_the_jump_window(engine, oracle, harness, shape):
    """graph_free_begin = Unbounded queues every real node at offset 0: the initial priorities spread over
    o + e * max(len, dist_max), which the ring must hold.  With the jump term alone (win = 64 here) a chain of 32 nodes came
    back with POA_FLAG_EXACT_OVERFLOW and the dense pass's GLOBAL alignment.  The 300-node chain needs win = 1024 at 4/6/2:
    16 waves x 1024 priorities x 12 bytes exceed the 80 KB budget, so the launcher itself moves the ring to global memory
    (poa_wsearch_global_kernel)."""
    if shape == "dag60":
        g, sym = _bubble_dag(60, (10, 25, 40), (30, 33))
    else:
        g, sym = _chain(shape, seed=shape)
    n = len(sym)
    skew, dist_max = _graph_spread(harness, g)
    glds = graph_lds_bytes(harness, g)
    qs = [sym[(n - ln) // 3:(n - ln) // 3 + ln] for ln in (1, 8, n // 2, n)]
    qseq, qoff = pack_queries(qs)
    kernels = set()
    for costs in ((4, 6, 2), (2, 8, 1)):
        for si, span in enumerate(FREE_BEGIN_SPANS):
            for mingap in (True, False):
                A = _oracle_batch(oracle, g, qseq, qoff, costs, mingap, True, span)
                res, info, _ = _replay(engine, g, qseq, qoff, costs, mingap, True, span)
                what = (shape, costs, si, mingap)
                _same_as_oracle(oracle, res, A, len(qs), True, what)
                win = _win_rule(*costs, skew, mingap, si < 3, n, dist_max)
                if si == 3 or not mingap:
                    assert win == _win_jump(*costs, skew) == 64, what          # the control and Dijkstra order keep the old ring
                assert len(info) == 1
                _check_info(info[0], predict_wave(glds, g.n, win), len(qs))
                kernels.add((info[0]["kernel"], info[0]["win"]))
    if shape == 300:
        assert ("wave_generic", 1024) in kernels and ("wave_generic", 512) in kernels and ("wave_lds", 64) in kernels, kernels
    elif shape != 28:
        assert any(k == "wave_lds" and w > 64 for k, w in kernels), kernels     # beyond the 64 priorities of the jump term


def _tier_costs(skew):
    """For each ring width the first cost set of the candidates that the rule puts there for a graph of this skew (2/2/1: the
    64-priority ring on the bypass graph, whose skew of 30 puts 4/6/2 at 128)."""
    out = {}
    for c in WIN_COSTS + [(2, 2, 1)]:
        out.setdefault(_win_jump(*c, skew), c)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ["snp_bubbles", "bypass"])
def test_gpu_ring_tiers_under_global_alignment(engine, oracle, harness, graph):
    """Global runs whose costs put the ring at 64, 128 and 256 priorities (in LDS: 16 waves x win x 12 bytes <= 80 KB) and at
    512 and 1024 (in global memory, poa_wsearch_global_kernel, by the launcher's own choice).  With four waves per block the
    two wide rings fit the LDS again: same results.  Search counters equal the oracle's on every path."""
    if graph == "bypass":
        g, sym = _chain(34, seed=5, bypass=(1, 32))
    else:
        g, sym = _bubble_dag(40, (8, 18, 30), (22, 25))
    skew, _ = _graph_spread(harness, g)
    assert skew <= 9 if graph == "snp_bubbles" else skew == 30
    glds = graph_lds_bytes(harness, g)
    rng = np.random.Generator(np.random.PCG64(77))
    qs = [W.random_walk_query(rng, g, 0.15) for _ in range(16)]
    qseq, qoff = pack_queries(qs)
    tiers = _tier_costs(skew)
    for win in (64, 128, 256, 512, 1024):
        costs = tiers[win]
        A = _oracle_batch(oracle, g, qseq, qoff, costs, True, True, None, counters=True)
        res, info, sc = _replay(engine, g, qseq, qoff, costs, counters=True)
        _same_as_oracle(oracle, res, A, 16, False, (graph, win))
        assert np.array_equal(sc[:, :3].astype(np.uint64), A["counters"]), (graph, win)
        want = predict_wave(glds, g.n, win)
        assert want["ring_global"] == (win >= 512) and want["kernel"] == ("wave_generic" if win >= 512 else "wave_lds")
        _check_info(info[0], want, 16)
        if win >= 512:
            res4, info4, sc4 = _replay(engine, g, qseq, qoff, costs, counters=True, ws_waves=4)
            want4 = predict_wave(glds, g.n, win, waves=4)
            assert want4["kernel"] == "wave_lds" and not want4["ring_global"]
            _check_info(info4[0], want4, 16)
            _same_as_oracle(oracle, res4, A, 16, False, (graph, win, "four waves"))
            assert np.array_equal(sc4[:, :3], sc[:, :3])


VARIANTS = [("groups_of_16", dict(ws_group=16)), ("groups_of_8", dict(ws_group=8, ws_waves=2)), ("graph_in_global_memory", dict(exact_lds=0)),
            ("records_off", dict(ws_rec=0)), ("static_schedule", dict(ws_static=1)), ("lane_kernel", dict(exact_impl="lane")),
            ("flat", dict(exact_impl="flat")), ("flat_generic", dict(exact_impl="flat", ps_lean=0))]


@pytest.mark.gpu
@pytest.mark.parametrize("tune", [v[1] for v in VARIANTS], ids=[v[0] for v in VARIANTS])
def test_gpu_replay_variants_under_ends_free(engine, oracle, harness, tune):
    """The forcing overrides of test_gpu_replay_variants_are_bit_identical on ends-free runs: the 40-node chain under a free
    graph begin (win = 128) and a random DAG under a span with every bound set.  The record names the kernel that ran; the
    flat search reports the generic kernel even without POA_PS_LEAN = 0, since replay_flat runs the lean step on Global
    runs only."""
    g1, sym = _chain(40, seed=40)
    rng = np.random.Generator(np.random.PCG64(5100))
    g2 = W.random_dag(17, n_nodes=13, p_edge=0.3)
    cases = [(g1, [sym[13:14], sym[10:18], sym[6:26], sym], (4, 6, 2), dict()),
             (g2, [W.random_walk_query(rng, g2, 0.3) for _ in range(12)], (2, 8, 1),
              dict(graph_free_begin=(INC, 0), qry_free_end=(INC, 0), graph_free_end=(EXC, 3)))]
    for g, qs, costs, span in cases:
        qseq, qoff = pack_queries(qs)
        skew, dist_max = _graph_spread(harness, g)
        win = _win_rule(*costs, skew, True, span.get("graph_free_begin", (U, 0))[0] == U, max(len(q) for q in qs), dist_max)
        A = _oracle_batch(oracle, g, qseq, qoff, costs, True, True, span)
        res, info, _ = _replay(engine, g, qseq, qoff, costs, True, True, span, **tune)
        _same_as_oracle(oracle, res, A, len(qs), True, (tune, g.n))
        i = info[0]
        assert i["win"] == win == (128 if g is g1 else 64)
        impl = tune.get("exact_impl")
        if impl == "lane":
            assert i["kernel"] == "lane" and i["lanes"] == 1
        elif impl == "flat":
            assert i["kernel"] == "flat_generic" and i["lanes"] == 16
        else:
            want = predict_wave(graph_lds_bytes(harness, g), g.n, win, group=tune.get("ws_group", 64), waves=tune.get("ws_waves"),
                                exact_lds=tune.get("exact_lds", 1) != 0, rec=tune.get("ws_rec", 1) != 0)
            _check_info(i, want, len(qs), static="ws_static" in tune)
            if "ws_group" in tune:
                assert want["kernel"] == "wave_groups" and want["lanes"] == tune["ws_group"]
            if "exact_lds" in tune:
                assert want["kernel"] == "wave_generic" and not want["graph_lds"] and not want["ring_global"]
            if "ws_rec" in tune:
                assert want["kernel"] == "wave_lds" and not want["rec_lds"]


@pytest.mark.gpu
def test_gpu_flat_search_runs_the_lean_kernel_on_global_runs_only(engine, oracle, harness):
    """The other side of the flat rule: the same 40-node chain as a Global run takes poa_fsearch_lean_kernel (8 lanes a query)."""
    g, sym = _chain(40, seed=40)
    qs = [sym, sym[3:30], np.concatenate([sym[:10], sym[12:]])]
    qseq, qoff = pack_queries(qs)
    A = _oracle_batch(oracle, g, qseq, qoff, (4, 6, 2), True, True, None)
    res, info, _ = _replay(engine, g, qseq, qoff, (4, 6, 2), exact_impl="flat")
    _same_as_oracle(oracle, res, A, len(qs), False)
    assert info[0]["kernel"] == "flat_lean" and info[0]["lanes"] == 8 and info[0]["win"] == 64


@pytest.mark.gpu
def test_gpu_persistent_schedule_by_the_launchers_own_choice(engine, oracle, harness):
    """More blocks than are resident at once: the wave search hands the queries out from a work counter, longest expected
    search (highest dense score) first, so the order of the searches is not the order of the queries."""
    g = W.random_dag(23, n_nodes=12, p_edge=0.3)
    glds = graph_lds_bytes(harness, g)
    rng = np.random.Generator(np.random.PCG64(2300))
    first = [W.random_walk_query(rng, g, 0.3) for _ in range(16)]
    qseq, qoff = pack_queries(first)
    _, info, _ = _replay(engine, g, qseq, qoff, (4, 6, 2))
    want = predict_wave(glds, g.n, 64)
    _check_info(info[0], want, 16)
    assert not info[0]["persistent"]
    resident, waves = info[0]["resident"], info[0]["waves"]
    n = resident * waves + 100
    alpha = np.frombuffer(b"ACGT", np.uint8)
    qs = [alpha[rng.integers(0, 4, int(rng.integers(2, 7)))] for _ in range(n)]
    qseq, qoff = pack_queries(qs)
    A = _oracle_batch(oracle, g, qseq, qoff, (4, 6, 2), True, True, None)
    assert len(set(np.asarray(A["score"]).tolist())) > 3     # the schedule's sort key differs from query to query
    res, info, _ = _replay(engine, g, qseq, qoff, (4, 6, 2))
    assert len(info) == 1
    _check_info(info[0], want, n)
    assert info[0]["persistent"] and info[0]["resident"] == resident and info[0]["blocks"] == resident
    _same_as_oracle(oracle, res, A, n, False)


@pytest.mark.gpu
@pytest.mark.parametrize("span", [None, dict(graph_free_begin=(INC, 0), qry_free_end=(INC, 2), graph_free_end=(INC, 1))], ids=["global", "ends_free"])
def test_gpu_second_chunk_of_an_exact_and_a_hybrid_run(engine, oracle, harness, span):
    """A workspace cap that cuts the batch into chunks: the replay of a later chunk addresses statuses, counters, planes and
    results from ch.first.  Exact and hybrid runs equal their one-chunk runs and the oracle; hybrid replays exactly the
    queries the dense pass flagged (an ends-free run replays every query: its mode is exact whatever was asked)."""
    g, (qseq, qoff) = W.scaled_linearish(300, 15, 8, 24, 330)
    n = 24
    A = _oracle_batch(oracle, g, qseq, qoff, (4, 6, 2), True, True, span)
    dense = engine.PoastaAligner(engine.AffineMinGapCost(engine.GapAffine(4, 2, 6))).align_batch(g, qseq=qseq, qoff=qoff)
    flagged = int(np.count_nonzero(dense.flags))
    # three u32 planes of rows x pitch cells per query (the pitch: columns rounded up to 64); a cap of 0.4 of the batch cuts it
    # into three chunks (a batch's own workspace_bytes() may be a larger cached buffer's, so the cap is worked out here)
    whole = sum(3 * g.n * ((int(qoff[i + 1] - qoff[i]) + 64) // 64 * 64) * 4 for i in range(n))
    for mode in ("exact", "hybrid"):
        one, info1, _ = _replay(engine, g, qseq, qoff, (4, 6, 2), bounds=span, mode=mode)
        cut, info, _ = _replay(engine, g, qseq, qoff, (4, 6, 2), bounds=span, mode=mode, workspace_bytes=whole * 2 // 5)
        assert len(info1) == 1 and len(info) >= 2 and cut.stats["n_chunks"] == len(info)
        assert all(i["kernel"] == info1[0]["kernel"] == "wave_lds" and i["win"] == info1[0]["win"] for i in info)
        assert np.array_equal(one.score, cut.score) and np.array_equal(one.flags, cut.flags)
        assert np.array_equal(one.pair_off, cut.pair_off) and np.array_equal(one.pairs, cut.pairs)
        _same_as_oracle(oracle, cut, A, n, span is not None, (mode, "two chunks"))
        if mode == "hybrid" and span is None:
            assert 0 < flagged and cut.stats["n_exact"] == flagged == one.stats["n_exact"]
        else:
            assert cut.stats["n_exact"] == n == one.stats["n_exact"]


@pytest.mark.gpu
def test_gpu_graph_arrays_just_under_and_just_over_the_staging_budget(engine, oracle, harness):
    """A chain whose arrays (exact_lds_bytes: 25 bytes a row, two node-bubble entries of 12 bytes a row, padding) fit the 80 KB
    budget beside the ring of 16 waves x 64 priorities x 12 bytes, and one of 16 rows more that does not: the record flips from the all-LDS kernel to the
    generic-pointer one with the graph read from global memory and the ring still in LDS.  Four 30-symbol queries under
    ends-free with a bounded begin (win = 64) keep the searches short."""
    ring = 16 * 64 * RING_BYTES_PER_PRIORITY
    chain_lds = lambda n: exact_lds_bytes(n + 2, n + 1, 2 * (n + 1))   # rows with both sentinels, edges, node-bubble entries
    n_under = max(n for n in range(1300, 1500) if chain_lds(n) + ring <= GRAPH_RING_BUDGET)
    span = dict(graph_free_begin=(INC, 0), qry_free_end=(INC, 0))
    for n, staged in ((n_under, True), (n_under + 16, False)):
        g, sym = _chain(n, seed=3)
        glds = graph_lds_bytes(harness, g)
        assert glds == chain_lds(n) and (glds + ring <= GRAPH_RING_BUDGET) == staged
        qs = [sym[:30], sym[2:32], np.concatenate([sym[:12], sym[13:31]]), np.concatenate([sym[:20], sym[19:29]])]
        qseq, qoff = pack_queries(qs)
        A = _oracle_batch(oracle, g, qseq, qoff, (4, 6, 2), True, True, span)
        res, info, _ = _replay(engine, g, qseq, qoff, (4, 6, 2), bounds=span)
        _same_as_oracle(oracle, res, A, 4, True, n)
        want = predict_wave(glds, g.n, 64)
        assert want["kernel"] == ("wave_lds" if staged else "wave_generic") and want["graph_lds"] == staged and not want["ring_global"]
        _check_info(info[0], want, 4)


@pytest.mark.gpu
def test_gpu_replay_info_argument_errors(engine):
    from poasta_amd import _lib
    import ctypes as C
    g, (qseq, qoff) = W.scaled_linearish(60, 3, 2, 4, 60)
    rb = engine.ResidentBatch(g, qseq, qoff)
    out = (C.c_uint32 * 8)()
    L = _lib.lib()
    try:
        assert L.poa_batch_replay_info(rb.handle, 0, out) == -1 and L.poa_batch_replay_info(None, 0, out) == -1
        rb.run(engine.GapAffine(4, 2, 6))
        assert L.poa_batch_replay_info(rb.handle, 0, out) == -7          # a dense run replays nothing
        rb.run(engine.GapAffine(4, 2, 6), None, engine.make_config("exact"))
        assert L.poa_batch_replay_info(rb.handle, 0, out) == 0 and out[0] == 2 and out[1] == 64
        assert L.poa_batch_replay_info(rb.handle, 1, out) == -1 and L.poa_batch_replay_info(rb.handle, 0, None) == -1
        rb.fetch()
    finally:
        rb.close()
