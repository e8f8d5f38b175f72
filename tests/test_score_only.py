"""Score-only mode (POA_MODE_SCORE): the row liveness table on the CPU, and on the GPU the forward sweep against dense mode of the
same library and against the oracle — scores bit for bit, the two input-derived flags, no pairs, the slot-sized workspace."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

NONE = 0xFFFFFFFF
EMPTY_GRAPH, SHORT_QUERY, START_QUIRK = 0x20, 0x08, 0x02
INPUT_FLAGS = EMPTY_GRAPH | SHORT_QUERY
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7
PARENT_KERNEL_HASH = "ce74a6d3f19ea528"   # bench.forward_kernel_source_hash() at the parent commit


# ---- CPU: row liveness and slots ---------------------------------------------------------------------------------------------
def _brute_force_slots_check(g, dg):
    """Recompute liveness from the CSR arrays and poa_graph_node_rows; check the exported table against it."""
    slot, n_slots = dg.sweep_slots()
    rows = dg.node_rows()
    n = g.n
    node_of = np.zeros(n, np.int64)
    node_of[rows] = np.arange(n)
    succ_rows = [sorted(int(rows[s]) for s in g.successors(int(node_of[r]))) for r in range(n)]
    pred_rows = [[int(rows[p]) for p in g.predecessors(int(node_of[r]))] for r in range(n)]
    chain = [len(pred_rows[r]) == 1 and pred_rows[r][0] + 1 == r for r in range(n)]
    intervals = []
    for r in range(n):
        readers = [s for s in succ_rows[r] if not (s == r + 1 and chain[s])]
        if readers:
            assert slot[r] != NONE, "row %d is read back by rows %s but has no slot" % (r, readers)
            assert slot[r] < n_slots
            intervals.append((r, max(succ_rows[r]), int(slot[r])))
        else:
            assert slot[r] == NONE, "row %d is never read back but has a slot" % r
    # no two rows whose live intervals overlap share a slot; n_slots == the maximum overlap
    depth = np.zeros(n + 1, np.int64)
    for a, b, _ in intervals:
        depth[a:b + 1] += 1
    assert n_slots == (int(depth.max()) if intervals else 0)
    by_slot = {}
    for a, b, s in intervals:
        by_slot.setdefault(s, []).append((a, b))
    for s, iv in by_slot.items():
        iv.sort()
        for (a0, b0), (a1, b1) in zip(iv, iv[1:]):
            assert b0 < a1, "slot %d shared by rows %d and %d, both live at row %d" % (s, a0, a1, a1)
    return n_slots


def test_sweep_slots_against_brute_force():
    from poasta_amd import aligner
    seen = set()
    for seed in range(300):
        rng = np.random.Generator(np.random.PCG64(5000 + seed))
        g = W.random_dag(seed, n_nodes=int(rng.integers(3, 40)), p_edge=float(rng.choice([0.1, 0.25, 0.5])), alphabet=b"AC" if seed % 2 else b"ACGT")
        seen.add(_brute_force_slots_check(g, aligner.DeviceGraph(g)))
    assert len(seen) >= 4   # (the random graphs do exercise different depths of overlap)
    # a pure chain needs at most one slot
    b = GraphBuilder()
    b.add_path(np.frombuffer(b"ACGTACGTACGTTTGA", np.uint8))
    chain = b.finish()
    assert _brute_force_slots_check(chain, aligner.DeviceGraph(chain)) <= 1
    # the workload graphs at reduced size
    g, _ = W.scaled_linearish(300, 15, 8, 1, 50)
    few = _brute_force_slots_check(g, aligner.DeviceGraph(g))
    assert 1 <= few <= 8   # chain-like: a handful of rows alive at once, whatever the length
    _brute_force_slots_check(W.LayeredPOA(n_layers=60, width=4, indeg=4, seed=5).graph, aligner.DeviceGraph(W.LayeredPOA(n_layers=60, width=4, indeg=4, seed=5).graph))
    pg = W.PangenomePOA(ref_len=600, n_hap=8, seed=4).graph
    _brute_force_slots_check(pg, aligner.DeviceGraph(pg))
    _brute_force_slots_check(GraphBuilder().finish(), aligner.DeviceGraph(GraphBuilder().finish()))


def test_sweep_slots_follow_graph_update():
    from poasta_amd import _lib, aligner
    g0 = W.random_dag(7, n_nodes=20, p_edge=0.3)
    dg = aligner.DeviceGraph(g0)
    _brute_force_slots_check(g0, dg)
    for seed in (11, 12, 13):
        g1 = W.random_dag(seed, n_nodes=10 + seed, p_edge=0.25)
        _lib.check(_lib.lib().poa_graph_update(dg.handle, g1.n, g1.start, g1.end, aligner._p(g1.symbol), aligner._p(g1.succ_off),
                                               aligner._p(g1.succ), aligner._p(g1.pred_off), aligner._p(g1.pred)))
        dg.graph = g1
        _brute_force_slots_check(g1, dg)
    # n_slots alone (slot = NULL)
    n = C.c_uint32(123)
    _lib.check(_lib.lib().poa_graph_sweep_slots(dg.handle, None, C.byref(n)))
    assert n.value == dg.sweep_slots()[1]


def test_score_mode_in_the_python_mirror():
    from poasta_amd import _lib, aligner
    assert aligner.make_config(mode="score").mode == 3 == _lib.MODE_SCORE
    with pytest.raises(KeyError):
        aligner.make_config(mode="scores")
    assert b"0.2" in _lib.lib().poa_version()


def test_hashed_kernel_sources_unchanged():
    """bench.py takes the committed PMC counters for the tree's only while these five files keep their hash."""
    import bench
    h = bench.forward_kernel_source_hash()
    assert (h if isinstance(h, str) else h[0]) == PARENT_KERNEL_HASH


def _build_score_host(tmp_path):
    """The C++ mirror's score_batch, instantiated for the one-piece and the two-piece configuration (tests/score_host)."""
    from poasta_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    exe = os.path.join(str(tmp_path), "score_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(root, "tests", "score_host", "score_host.cpp"),
                           "-L" + libdir, "-lpoasta_amd", "-Wl,-rpath," + libdir])
    return exe, os.path.join(root, "tests", "golden")


def test_cpp_mirror_score_batch_compiles(tmp_path):
    exe, _ = _build_score_host(tmp_path)
    assert subprocess.run([exe]).returncode == 64   # (usage: it links and starts; the GPU test below runs it)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _costs(engine, m, o, e):
    return engine.GapAffine(m, e, o)   # reference ctor order: (mismatch, extend, open)


def _parity(engine, oracle, g, qs, costs, astar=True, **tune):
    """Score mode (one-shot and resident) against dense mode of the same library, the oracle's dense restatement and the
    oracle's A* in Dijkstra order without pruning.  Returns the scores."""
    qseq, qoff = pack_queries(qs)
    n = len(qs)
    al = engine.PoastaAligner(engine.AffineDijkstra(_costs(engine, *costs)))
    dense = al.align_batch(g, qseq=qseq, qoff=qoff)
    # one-shot, pairs = NULL and pair_capacity 0, straight through the C ABI
    from poasta_amd import _lib
    cfg = engine.make_config("score", **tune)
    score, flags = np.full(n, 12345, np.uint32), np.full(n, 0xFF, np.uint32)
    pair_off = np.full(n + 1, 77, np.uint64)
    st = _lib.PoaStats()
    c = _costs(engine, *costs)._c()
    dg = engine._device_graph(g)
    _lib.check(_lib.lib().poa_align_batch_ex(dg.handle, C.byref(c), C.byref(cfg), n, engine._p(qseq), engine._p(qoff), engine._p(score),
                                             None, engine._p(pair_off), 0, engine._p(flags), C.byref(st), 0))
    assert np.array_equal(score, dense.score), ("one-shot score mode vs dense mode", costs, tune)
    assert np.array_equal(flags, dense.flags & INPUT_FLAGS), ("flags", costs, tune)
    assert not pair_off.any()
    assert st.ms_traceback == 0.0 and st.n_queries == n
    # resident
    rb = engine.ResidentBatch(g, qseq, qoff, config=cfg)
    rb.run(_costs(engine, *costs), None, cfg)
    r = rb.fetch(want_pairs=False)
    assert np.array_equal(r.score, dense.score) and np.array_equal(r.flags, dense.flags & INPUT_FLAGS) and not r.pair_off.any()
    rb.run(_costs(engine, *costs), None, cfg)   # again on the same slots
    assert np.array_equal(rb.fetch(want_pairs=False).score, dense.score)
    rb.close()
    og = oracle.OracleGraph.from_csr(g.as_dict())
    oc = oracle.Costs(*costs)
    if g.n > 2:
        D = og.dense_batch(qseq, qoff, oc, threads=4)
        assert np.array_equal(score, D["score"]), ("vs the dense restatement", costs)
        if astar:
            A = og.astar_batch(qseq, qoff, oc, oracle.H_DIJKSTRA, False, threads=4)
            _ASTAR_COUNT[0] += int((A["status"] == 0).sum())
            _ASTAR_COUNT[1] += n
            for i in range(n):
                if A["status"][i] == 0:   # (else the restated reference panicked: it has no score for this query)
                    assert int(score[i]) == int(A["score"][i]), ("vs A*, Dijkstra order, no pruning", costs, i)
    return score


_ASTAR_COUNT = [0, 0]   # queries that reached the comparison with A* / queries offered to it


def _astar_coverage(since, fraction):
    """Most queries must really have been compared with A* (it has no score only where the restated reference panics)."""
    done, offered = _ASTAR_COUNT[0] - since[0], _ASTAR_COUNT[1] - since[1]
    assert offered > 0 and done >= fraction * offered, (done, offered)


def _with_short(qs, rng, alpha=b"ACGT"):
    a = np.frombuffer(alpha, np.uint8)
    return list(qs) + [np.zeros(0, np.uint8), rng.choice(a, 1), rng.choice(a, 2)]


COST_SETS = [(4, 6, 2), (2, 8, 1), (1, 10, 2), (3, 1, 1), (4, 4, 2)]


@pytest.mark.gpu
def test_score_parity_random_dags(engine, oracle):
    since = list(_ASTAR_COUNT)
    for seed in range(30):
        rng = np.random.Generator(np.random.PCG64(1000 + seed))
        alpha = b"AC" if seed % 2 else b"ACGT"
        g = W.random_dag(seed, n_nodes=int(rng.integers(3, 14)), p_edge=0.3, alphabet=alpha)
        qs = _with_short([W.random_walk_query(rng, g, 0.3, alpha) for _ in range(12)], rng, alpha)
        for costs in (COST_SETS[seed % 5], COST_SETS[(seed + 2) % 5]):
            _parity(engine, oracle, g, qs, costs)
        if seed < 6:
            _parity(engine, oracle, g, qs, COST_SETS[seed % 5], astar=False, planes=32)   # the u32 path on the same inputs
    _astar_coverage(since, 0.9)   # (26 of these 900 queries make the restated reference panic)


@pytest.mark.gpu
def test_score_parity_one_strip(engine, oracle):
    """pitch <= 512 (general path, u16), 512 < pitch <= 1024 (the packed one-strip kernel; and the general u16 / u32 kernels
    on the same inputs), mismatch cost 255 within the u16 bound, and a cost set whose bound leaves u16."""
    rng = np.random.default_rng(3)
    since = list(_ASTAR_COUNT)
    g, (qseq, qoff) = W.scaled_linearish(420, 20, 10, 12, 400, p_sub=0.2, p_ins=0.05, p_del=0.05)
    qs = _with_short([qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(12)], rng)
    qs.append(rng.choice(np.frombuffer(b"ACGT", np.uint8), 400))
    for costs in ((4, 6, 2), (255, 3, 1), (255, 6, 2)):
        _parity(engine, oracle, g, qs, costs)
    g, (qseq, qoff) = W.scaled_linearish(900, 50, 25, 24, 1000)
    qs = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(24)]
    qs.append(rng.choice(np.frombuffer(b"ACGT", np.uint8), 1023))
    qs.append(qs[0][:600])
    a = _parity(engine, oracle, g, qs, (4, 6, 2))
    assert np.array_equal(a, _parity(engine, oracle, g, qs, (4, 6, 2), astar=False, px=0))
    assert np.array_equal(a, _parity(engine, oracle, g, qs, (4, 6, 2), astar=False, planes=32))
    _parity(engine, oracle, g, qs, (255, 6, 2))
    # bound beyond u16: [o + e L] + [o + e (shortest path)] = 2 * 60 + 40 * (1000 + ~900) > 65534 -> u32 cells
    _parity(engine, oracle, g, qs, (255, 60, 40))
    sseq, soff = pack_queries(qs)
    cfg = engine.make_config("score")
    rb = engine.ResidentBatch(g, sseq, soff, config=cfg)
    for costs, narrow in (((4, 6, 2), True), ((255, 6, 2), True), ((255, 60, 40), False)):
        rb.run(_costs(engine, *costs), None, cfg)
        assert ("u16" in rb.layout()) == narrow, costs   # the cell width the sweep chose from the bound
    rb.close()
    # in-degree-4 bubbles, one strip
    poa = W.LayeredPOA(n_layers=150, width=4, indeg=4, seed=7)
    qs = _with_short(poa.queries(6, length=140), rng) + poa.queries(4, length=900)
    _parity(engine, oracle, poa.graph, qs, (4, 6, 2))
    _parity(engine, oracle, poa.graph, qs, (255, 2, 1))
    _parity(engine, oracle, poa.graph, poa.queries(8, length=900), (4, 6, 2))   # all of them in (512, 1024]: packed kernel
    _astar_coverage(since, 0.9)


@pytest.mark.gpu
def test_score_parity_several_strips(engine, oracle):
    """Queries of two and three 1024-column strips: the carries between strips, double-buffered by strip parity, on a
    bubble graph whose slots are reused all the time."""
    rng = np.random.default_rng(4)
    since = list(_ASTAR_COUNT)
    poa = W.LayeredPOA(n_layers=200, width=4, indeg=4, seed=5)
    qs = _with_short(poa.queries(3, length=1500) + poa.queries(3, length=2500, seed=9) + poa.queries(2, length=700, seed=10), rng)
    a = _parity(engine, oracle, poa.graph, qs, (4, 6, 2))
    assert np.array_equal(a, _parity(engine, oracle, poa.graph, qs, (4, 6, 2), astar=False, planes=32))
    _parity(engine, oracle, poa.graph, qs, (255, 60, 40))
    g, (qseq, qoff) = W.scaled_linearish(1500, 40, 20, 4, 0)
    qs = [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(4)]
    _parity(engine, oracle, g, qs, (4, 6, 2))
    pg = W.PangenomePOA(ref_len=1500, n_hap=12, seed=4)
    _parity(engine, oracle, pg.graph, pg.queries(4, length=1200), (4, 6, 2))
    _astar_coverage(since, 0.9)


@pytest.mark.gpu
def test_score_empty_graph_and_empty_batch(engine, oracle):
    al = engine.PoastaAligner(engine.AffineMinGapCost(_costs(engine, 4, 6, 2)))
    empty = GraphBuilder().finish()
    score, flags = al.score_batch(empty, [b"ACGT", b"", b"A"])
    dense = al.align_batch(empty, [b"ACGT", b"", b"A"])
    assert score.tolist() == [16, 0, 4] == dense.score.tolist()
    assert np.array_equal(flags, dense.flags & INPUT_FLAGS) and (flags & EMPTY_GRAPH).all()
    b = GraphBuilder()
    b.add_path(np.frombuffer(b"ACGT", np.uint8))
    score, flags = al.score_batch(b.finish(), [])
    assert len(score) == 0 and len(flags) == 0
    # the resident entry point on the empty graph: the forward pass over the two sentinel rows, as in dense mode
    qseq, qoff = pack_queries([b"ACGT", b"", b"A"])
    cfg = engine.make_config("score")
    rb = engine.ResidentBatch(empty, qseq, qoff, config=cfg)
    rb.run(_costs(engine, 4, 6, 2), None, cfg)
    r = rb.fetch(want_pairs=False)
    rd = engine.ResidentBatch(empty, qseq, qoff)
    rd.run(_costs(engine, 4, 6, 2))
    d = rd.fetch()
    assert np.array_equal(r.score, d.score) and np.array_equal(r.flags, d.flags & INPUT_FLAGS)
    rb.close()
    rd.close()


@pytest.mark.gpu
def test_score_config2_full_size(engine, oracle):
    """configs[1] at full size: the 10 000 scores of dense mode, checksum 3 720 720 (tests/test_gpu_full_size.py)."""
    g, (qseq, qoff) = W.config2(n_queries=10000)
    costs = _costs(engine, 4, 6, 2)
    rd = engine.ResidentBatch(g, qseq, qoff)
    rd.run(costs)
    dense = rd.fetch(want_pairs=False)
    rd.close()
    cfg = engine.make_config("score")
    rb = engine.ResidentBatch(g, qseq, qoff, config=cfg)
    rb.run(costs, None, cfg)
    res = rb.fetch(want_pairs=False)
    assert np.array_equal(res.score, dense.score)
    assert int(res.score.astype(np.uint64).sum()) == 3720720
    assert res.stats["n_chunks"] == 1 and res.stats["cells"] == 10000 * 1002 * 1001 and res.stats["ms_traceback"] == 0.0
    assert not (res.flags & ~np.uint32(INPUT_FLAGS)).any() and not res.pair_off.any()
    rb.close()
    al = engine.PoastaAligner(engine.AffineMinGapCost(costs))
    score, _ = al.score_batch(g, qseq=qseq, qoff=qoff)
    assert np.array_equal(score, dense.score)


@pytest.mark.gpu
def test_score_workspace_is_the_slot_footprint(engine, oracle):
    """The point of the mode, as conditions that follow from the design: a chain-like graph of several thousand rows, a few
    hundred queries of several kbp, a workspace cap far below ONE query's full planes — the score-only batch holds at most
    n_queries * max(n_slots, 1) * pitch * 2 planes * 4 bytes (+ 256 bytes of padding, include/poasta_amd.h), runs as one
    chunk and returns dense mode's scores."""
    n_q, length = 256, 3000
    g, (qseq, qoff) = W.scaled_linearish(3000, 120, 60, n_q, length)
    costs = _costs(engine, 4, 6, 2)
    dg = engine._device_graph(g)
    _, n_slots = dg.sweep_slots()
    pitches = [((int(qoff[i + 1] - qoff[i]) + 1 + 63) // 64) * 64 for i in range(n_q)]
    one_query_full = 3 * g.n * max(pitches) * 4
    bound = sum(max(n_slots, 1) * p * 2 * 4 for p in pitches) + 256
    cap = one_query_full // 4
    assert bound <= cap, "the test's own premise: every query's slots fit a quarter of one query's planes"
    cfg = engine.make_config("score")
    rb = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=cap, config=cfg)
    assert rb.workspace_bytes() <= bound
    rb.run(costs, None, cfg)
    res = rb.fetch(want_pairs=False)
    assert res.stats["n_chunks"] == 1
    rd = engine.ResidentBatch(g, qseq, qoff)
    rd.run(costs)
    dense = rd.fetch(want_pairs=False)
    assert rd.workspace_bytes() >= one_query_full // 8   # (the dense batch does hold planes: the accessor reports them)
    rd.close()
    assert np.array_equal(res.score, dense.score)
    # chunked on purpose (a cap of three queries' slots): same scores
    small = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=3 * max(n_slots, 1) * max(pitches) * 8, config=cfg)
    small.run(costs, None, cfg)
    r2 = small.fetch(want_pairs=False)
    assert r2.stats["n_chunks"] > 1 and np.array_equal(r2.score, dense.score)
    small.close()
    rb.close()


@pytest.mark.gpu
def test_score_mode_errors_leave_the_batch_usable(engine, oracle):
    from poasta_amd import _lib
    g, (qseq, qoff) = W.scaled_linearish(200, 10, 5, 8, 180)
    costs = _costs(engine, 4, 6, 2)
    cfg = engine.make_config("score")
    want = engine.PoastaAligner(engine.AffineMinGapCost(costs)).align_batch(g, qseq=qseq, qoff=qoff).score
    rb = engine.ResidentBatch(g, qseq, qoff, config=cfg)
    ef = engine.make_config("score", aln_type=engine.AlignmentType.EndsFree())
    with pytest.raises(_lib.PoaError) as e:
        rb.run(costs, None, ef)
    assert e.value.code == ERR_UNSUPPORTED
    rb.run(costs, None, cfg)
    assert np.array_equal(rb.fetch(want_pairs=False).score, want)
    for other in ("dense", "exact", "hybrid"):
        with pytest.raises(_lib.PoaError) as e:
            rb.run(costs, None, engine.make_config(other))
        assert e.value.code == ERR_INVALID_ARG
    with pytest.raises(_lib.PoaError) as e:
        rb.run(costs)   # poa_batch_run: dense
    assert e.value.code == ERR_INVALID_ARG
    rb.run(costs, None, cfg)
    assert np.array_equal(rb.fetch(want_pairs=False).score, want)
    rb.close()
    # the other way round, and the creation / one-shot calls
    rd = engine.ResidentBatch(g, qseq, qoff)
    with pytest.raises(_lib.PoaError) as e:
        rd.run(costs, None, cfg)
    assert e.value.code == ERR_INVALID_ARG
    rd.run(costs)
    assert np.array_equal(rd.fetch().score, want)
    rd.close()
    with pytest.raises(_lib.PoaError) as e:
        engine.ResidentBatch(g, qseq, qoff, config=ef)
    assert e.value.code == ERR_UNSUPPORTED
    n = len(qoff) - 1
    score = np.zeros(n, np.uint32)
    c = costs._c()
    rc = _lib.lib().poa_align_batch_ex(engine._device_graph(g).handle, C.byref(c), C.byref(ef), n, engine._p(qseq), engine._p(qoff),
                                       engine._p(score), None, None, 0, None, None, 0)
    assert rc == ERR_UNSUPPORTED


COSTS2 = [(4, 2, 6, 1, 24), (1, 2, 10, 1, 8), (3, 3, 12, 1, 6), (2, 2, 4, 2, 4), (4, 3, 5, 0, 9)]   # (m, e1, o1, e2, o2), tests/test_two_piece.py


@pytest.mark.gpu
def test_score_two_piece(engine, oracle):
    """Score mode under the two-piece model == the scores poa_align_batch_2piece returns: the random cases of
    tests/test_two_piece.py and configs[1]-shaped reads under the CLI's example costs (4 / 6,24 / 2,1)."""
    n = 0
    for seed in range(40):
        rng = np.random.Generator(np.random.PCG64(7000 + seed))
        alpha = b"AC" if seed % 2 else b"ACGT"
        g = W.random_dag(seed, n_nodes=int(rng.integers(3, 14)), p_edge=0.3, alphabet=alpha)
        m, e1, o1, e2, o2 = COSTS2[seed % len(COSTS2)]
        al = engine.PoastaAligner(engine.Affine2PieceDijkstra(engine.GapAffine2Piece(m, e1, o1, e2, o2)))
        qs = [q for q in (W.random_walk_query(rng, g, 0.35, alpha) for _ in range(8)) if len(q) >= 1]
        res = al.align_batch(g, qs)
        score, flags = al.score_batch(g, qs)
        assert np.array_equal(score, res.score), (seed, (m, e1, o1, e2, o2))
        assert np.array_equal(flags, res.flags & INPUT_FLAGS)
        n += len(qs)
    assert n > 250
    g, (qseq, qoff) = W.config2(n_queries=48)
    al = engine.PoastaAligner(engine.Affine2PieceDijkstra(engine.GapAffine2Piece(4, 2, 6, 1, 24)))
    res = al.align_batch(g, qseq=qseq, qoff=qoff)
    score, _ = al.score_batch(g, qseq=qseq, qoff=qoff)
    assert np.array_equal(score, res.score)
    # open' = 255 + 255 - 0 does not fit poa_costs_t: the sweep's own cost fields are wider
    al = engine.PoastaAligner(engine.Affine2PieceDijkstra(engine.GapAffine2Piece(4, 255, 255, 0, 9)))
    g, (qseq, qoff) = W.scaled_linearish(60, 5, 3, 12, 70)
    assert np.array_equal(al.score_batch(g, qseq=qseq, qoff=qoff)[0], al.align_batch(g, qseq=qseq, qoff=qoff).score)


@pytest.mark.gpu
def test_cpp_mirror_score_batch(engine, tmp_path):
    """include/poasta_amd.hpp: score_batch returns align_batch's scores, no alignment, input-derived flags only —
    one-piece (4 / 6 / 2) and two-piece (4 / 6,24 / 2,1) on the golden MSA graph and reads."""
    exe, gold = _build_score_host(tmp_path)
    out = subprocess.check_output([exe, os.path.join(gold, "test2_half.msa.fa"), os.path.join(gold, "test2_from_abpoa.fa")]).decode().split()
    rows = np.array(out, np.int64).reshape(-1, 3)
    assert len(rows) == 20   # ten reads under each of the two models
    assert np.array_equal(rows[:, 0], rows[:, 2]) and not (rows[:, 1] & ~INPUT_FLAGS).any()
