"""Checkpointed mode of the two-piece model (POA_MODE_CHECKPOINT2; kernels of poa_checkpoint2.hpp, the walk of poa_twopiece.hpp
behind a window-and-snapshot addressing policy).

CPU: the mode constant and the new export; poa_graph_checkpoint_plan2 against a brute-force restatement of the snapshots; the
memory claim.  GPU: score, flags, pair_off and pairs equal as arrays, for every query of every case, to poa_align_batch_2piece —
the one-shot dense call, whose code path this mode does not touch — and, on a sample, to oracle/dense.hpp under two-piece costs."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import GraphBuilder, pack_queries

from test_checkpoint import _memory_claim_graph, _rows_view, _skip_graph, _with_short
from test_two_piece_resident import COST_CASES, LENS, _gc2, _one_shot, _run2, _same
from test_two_piece_shapes import _assert_batch_equals_oracle, _planes_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -7
C0 = COST_CASES["cli"][0]
ROTATION = [COST_CASES[k][0] for k in ("cli", "e2-zero", "e2-eq-e1", "mismatch-255")]
PLANS = (0, 1, 2, 7, "one")
FLAG_SHORT_QUERY = 8   # set for every one-symbol query: not what "the certificate's bits occur" means


# ---- CPU: the ABI -----------------------------------------------------------------------------------------------------------------
def test_checkpoint2_mode_in_the_python_mirror():
    from poasta_amd import _lib, aligner
    assert aligner.make_config(mode="checkpoint2").mode == 5 == _lib.MODE_CHECKPOINT2
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poasta_amd.h")).read(), flags=re.S)
    assert re.search(r"#define\s+POA_MODE_CHECKPOINT2\s+5u", hdr)
    assert re.search(r"\bint\s+poa_graph_checkpoint_plan2\s*\(\s*const\s+poa_graph_t\s*\*", hdr)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "poa_graph_checkpoint_plan2") and "poa_graph_checkpoint_plan2" in _lib.EXPORTS
    ns, rpq = C.c_uint32(0), C.c_uint32(0)
    assert _lib.lib().poa_graph_checkpoint_plan2(None, 0, C.byref(ns), None, C.byref(rpq)) == ERR_INVALID_ARG
    assert _lib.lib().poa_last_error() != b""
    assert b"0.2" in _lib.lib().poa_version()


# ---- CPU: the segment plan --------------------------------------------------------------------------------------------------------
def _brute_force_plan2_check(g, dg, segment_rows=0):
    """The snapshots recomputed from the CSR arrays and poa_graph_node_rows; the exported two-piece plan checked against them."""
    boundary, rpq = dg.checkpoint_plan(segment_rows, two_piece=True)
    _, n_slots = dg.sweep_slots()
    n = g.n
    pred_rows, chain, readers = _rows_view(g, dg)
    b = [int(v) for v in boundary]
    if n == 0:
        assert b == [0] and rpq == 0
        return 0, 0
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
        for r in range(bb, n):   # every (reader row >= bb, read row < bb) pair has the read row in this snapshot
            for p in pred_rows[r]:
                assert p >= bb or p in snap, "row %d reads row %d across boundary %d: not in its snapshot" % (r, p, bb)
        snap_rows += len(snap)
    assert rpq == 3 * n_slots + 3 * snap_rows + 5 * max(seg_len), (rpq, n_slots, snap_rows, seg_len)
    # the boundaries rule is the one-piece plan's: at the same segment length the two plans cut the same rows
    if segment_rows:
        assert [int(v) for v in dg.checkpoint_plan(segment_rows)[0]] == b
    return len(seg_len), rpq


def _plan2_checks(g):
    from poasta_amd import aligner
    dg = aligner.DeviceGraph(g)
    n_seg, rpq = _brute_force_plan2_check(g, dg)
    for k in (1, 2, 7, g.n):
        if g.n == 0 and k == 0:
            continue
        s, r = _brute_force_plan2_check(g, dg, k)
        if g.n:
            assert s == -(-g.n // min(k, g.n))
        if g.n and k == g.n:
            assert s == 1 and rpq <= r   # the default is never more than what one segment of all rows costs
    return n_seg


def test_checkpoint2_plan_against_brute_force():
    from poasta_amd import _lib, aligner
    seen = set()
    for seed in range(300):
        rng = np.random.Generator(np.random.PCG64(5000 + seed))
        g = W.random_dag(seed, n_nodes=int(rng.integers(3, 40)), p_edge=float(rng.choice([0.1, 0.25, 0.5])), alphabet=b"AC" if seed % 2 else b"ACGT")
        seen.add(_plan2_checks(g))
    assert len(seen) >= 3
    b = GraphBuilder()
    b.add_path(np.frombuffer(b"ACGTACGTACGTTTGA", np.uint8))
    _plan2_checks(b.finish())
    g, _ = W.scaled_linearish(300, 15, 8, 1, 50)
    assert _plan2_checks(g) > 1
    _plan2_checks(W.LayeredPOA(n_layers=60, width=4, indeg=4, seed=5).graph)
    _plan2_checks(W.PangenomePOA(ref_len=600, n_hap=8, seed=4).graph)
    _plan2_checks(GraphBuilder().finish())
    # after poa_graph_update the plan follows the new graph
    g0 = W.random_dag(7, n_nodes=20, p_edge=0.3)
    dg = aligner.DeviceGraph(g0)
    _brute_force_plan2_check(g0, dg)
    for seed in (11, 12, 13):
        g1 = W.random_dag(seed, n_nodes=10 + seed, p_edge=0.25)
        _lib.check(_lib.lib().poa_graph_update(dg.handle, g1.n, g1.start, g1.end, aligner._p(g1.symbol), aligner._p(g1.succ_off),
                                               aligner._p(g1.succ), aligner._p(g1.pred_off), aligner._p(g1.pred)))
        dg.graph = g1
        _brute_force_plan2_check(g1, dg)
        _brute_force_plan2_check(g1, dg, 3)


def test_checkpoint2_memory_claim():
    """The engine's own plan on a chain-like graph of more than 4 000 rows: a query holds at most 5 * rows / 8 plane rows, an
    eighth of the dense two-piece pass's 5 * rows.  With n_slots <= 8 the sum is at most 24 + 27 * rows / k + 5 * k, whose
    minimum 24 + 2 * sqrt(135 * rows) is about 1 630 at 4 800 rows; 5 * rows / 8 is 3 000."""
    from poasta_amd import aligner
    g, _ = _memory_claim_graph()
    dg = aligner.DeviceGraph(g)
    assert g.n >= 4000
    _, n_slots = dg.sweep_slots()
    assert n_slots <= 8
    boundary, rpq = dg.checkpoint_plan(two_piece=True)
    assert len(boundary) - 1 > 1
    assert rpq <= 5 * g.n // 8, (rpq, g.n)
    # the window weighs 5 instead of 3: the two-piece default cuts segments no longer than the one-piece default's
    assert int(boundary[1]) <= int(dg.checkpoint_plan()[0][1])


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
def _cfg(engine, plan=0, n=0):
    kw = {}
    if plan:
        kw["ckpt_rows"] = n if plan == "one" else plan
    return engine.make_config("checkpoint2", **kw)


def _resident(engine, g, qseq, qoff, costs, wide, cfg, workspace_bytes=0):
    rb = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=workspace_bytes, config=cfg)
    try:
        _run2(engine, rb, costs, wide, config=cfg)
        res = rb.fetch()
        res.workspace_bytes = rb.workspace_bytes()
        res.layout = rb.layout()
    finally:
        rb.close()
    return res


def _one_shot_ckpt(engine, g, qseq, qoff, costs, wide, cfg):
    """poa_align_batch_2piece_ex with mode 5: create, run, fetch, destroy inside the call."""
    lib, p = engine._lib.lib(), engine._p
    dg = engine._device_graph(g)
    qseq, qoff = np.ascontiguousarray(qseq, np.uint8), np.ascontiguousarray(qoff, np.uint64)
    n = len(qoff) - 1
    cap = int(qoff[-1]) + n * dg.graph.n
    score, flags, pair_off = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
    pairs = np.zeros((max(cap, 1), 2), np.uint32)
    st = engine._lib.PoaStats()
    with _planes_env(wide):
        c = _gc2(engine, costs)._c()
    engine._lib.check(lib.poa_align_batch_2piece_ex(dg.handle, C.byref(c), C.byref(cfg), n, p(qseq), p(qoff), p(score), p(pairs),
                                                    p(pair_off), cap, p(flags), C.byref(st), None, 0))
    return engine.BatchResult(score, pairs[:int(pair_off[n])], pair_off, flags, st.as_dict())


def _parity2(engine, g, qs, costs, wide=False, plans=PLANS, oracle=None, one_shot=True):
    """The mode, resident and one-shot, under every plan, against the one-shot dense two-piece call."""
    qseq, qoff = pack_queries(qs)
    want = _one_shot(engine, g, qseq, qoff, costs, wide)
    for k in plans:
        cfg = _cfg(engine, k, g.n)
        _same(_resident(engine, g, qseq, qoff, costs, wide, cfg), want, (costs, wide, k, "resident"))
        if one_shot:
            _same(_one_shot_ckpt(engine, g, qseq, qoff, costs, wide, cfg), want, (costs, wide, k, "one-shot"))
    if oracle is not None:
        m, e1, o1, e2, o2 = costs
        with oracle.two_piece(o2, e2):
            D = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq, qoff, oracle.Costs(m, o1, e1), threads=4)
        _assert_batch_equals_oracle(want, D, oracle, len(qs), (costs, "oracle"))
    return want


def _dag_case(seed):
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    alpha = b"AC" if seed % 2 else b"ACGT"
    g = W.random_dag(seed, n_nodes=int(rng.integers(3, 30)), p_edge=float(rng.choice([0.15, 0.3])), alphabet=alpha)
    qs = _with_short([W.random_walk_query(rng, g, 0.3, alpha) for _ in range(12)], rng, alpha)
    return g, qs, (ROTATION[seed % 4], ROTATION[(seed + 1) % 4])


# ---- 4. random DAGs ---------------------------------------------------------------------------------------------------------------
def test_checkpoint2_random_dag_cases_carry_flags(oracle):
    """The seeds of the GPU test below, under the oracle alone: non-zero certificate flags occur among the twelve seeds it
    compares, so the GPU comparison of flags is a comparison of set bits."""
    flagged = 0
    for seed in range(12):
        g, qs, cost_sets = _dag_case(seed)
        qseq, qoff = pack_queries(qs)
        for m, e1, o1, e2, o2 in cost_sets:
            with oracle.two_piece(o2, e2):
                D = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq, qoff, oracle.Costs(m, o1, e1), threads=4)
            flagged += int(((D["flags"] & ~np.uint32(FLAG_SHORT_QUERY)) != 0).sum())
    assert flagged > 0


@pytest.mark.gpu
def test_gpu_checkpoint2_random_dags(engine, oracle):
    flagged = 0
    for seed in range(40):
        g, qs, cost_sets = _dag_case(seed)
        for costs in cost_sets:
            d = _parity2(engine, g, qs, costs, oracle=oracle if seed < 12 else None)
            flagged += int(((d.flags & ~np.uint32(FLAG_SHORT_QUERY)) != 0).sum())
        if seed < 8:
            _parity2(engine, g, qs, cost_sets[0], wide=True)   # the u32 cells on the same inputs
    assert flagged > 0


# ---- 5. an edge that skips segments -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_checkpoint2_edge_that_skips_segments(engine, oracle):
    g, through = _skip_graph()
    rng = np.random.default_rng(12)
    qs = [through, through[:-1], np.concatenate([through[:3], through[4:]])] + [W.random_walk_query(rng, g, 0.1) for _ in range(6)]
    boundary, _ = engine._device_graph(g).checkpoint_plan(7, two_piece=True)
    assert len(boundary) - 1 >= 9
    for costs in (C0, COST_CASES["e2-eq-e1"][0]):
        d = _parity2(engine, g, qs, costs, plans=(7, 0), oracle=oracle)
        assert d.score[0] == 0 and len(d.raw_alignment(0)) == len(through) == 12   # the walk took the long edge


# ---- 6. pass and register boundaries ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_poa(kind):
    if kind == "chain":
        return W.LinearishPOA(96, 4, 2, seed=1)
    if kind == "multi":
        return W.LayeredPOA(n_layers=25, width=4, indeg=4, seed=5)
    return W.PangenomePOA(ref_len=80, n_hap=8, p_snp=0.03, p_indel=0.01, max_indel=6, seed=4)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["u16", "u32"])
@pytest.mark.parametrize("kind", ["chain", "multi", "mixed"])
def test_gpu_checkpoint2_pass_and_register_boundaries(engine, kind, wide):
    """Lengths around the u32 pass (256 columns), the u16 pass (512) and the strip (1 024: the previous row's registers), and
    2 134 columns (three strips, the last pass partial), mixed in one batch and in reverse order."""
    poa = _small_poa(kind)
    g = poa.graph
    assert 60 <= g.n <= 160, g.n
    qs = [poa.queries(1, length=L, first=i)[0] if L else np.zeros(0, np.uint8) for i, L in enumerate(LENS)]
    assert [len(q) for q in qs] == list(LENS)
    for order in (qs, qs[::-1]):
        d = _parity2(engine, g, order, C0, wide=wide, plans=(0, 7), one_shot=False)
        assert np.array_equal(np.diff(d.pair_off.astype(np.int64)) > 0, np.array([len(q) > 0 for q in order]))


# ---- 7. scores above 65 535 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_checkpoint2_scores_above_u16(engine, oracle):
    g, (qseq, qoff) = W.scaled_linearish(36000, 300, 150, 2, 1500)
    costs = (4, 2, 6, 2, 24)
    got = _resident(engine, g, qseq, qoff, costs, False, _cfg(engine))
    assert got.layout == set()          # u32 by the engine's own choice
    assert int(got.score.min()) > 65534
    _same(got, _one_shot(engine, g, qseq, qoff, costs, False), "u32 values")
    with oracle.two_piece(24, 2):
        D = oracle.OracleGraph.from_csr(g.as_dict()).dense_batch(qseq[:int(qoff[1])], qoff[:2], oracle.Costs(4, 6, 2), threads=2)
    assert int(D["score"][0]) == 69336 == int(got.score[0])


# ---- 8. workspace and chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_checkpoint2_workspace_and_chunks(engine):
    g, (qseq, qoff) = _memory_claim_graph()
    n_q = len(qoff) - 1
    _, rpq = engine._device_graph(g).checkpoint_plan(two_piece=True)
    pitches = [((int(qoff[i + 1] - qoff[i]) + 1 + 63) // 64) * 64 for i in range(n_q)]
    cfg = _cfg(engine)
    want = _one_shot(engine, g, qseq, qoff, C0, False)
    whole = _resident(engine, g, qseq, qoff, C0, False, cfg)
    assert whole.workspace_bytes == sum(rpq * p * 4 for p in pitches) + 256
    assert whole.stats["n_chunks"] == 1 and whole.stats["ms_forward"] > 0 and whole.stats["ms_traceback"] > 0
    assert whole.layout == {"u16"}
    _same(whole, want, "one chunk")

    def dense_resident(cap, wide):
        rb = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=cap)
        try:
            _run2(engine, rb, C0, wide)
            return rb.fetch()
        finally:
            rb.close()

    cap = 5 * g.n * max(pitches) * 4   # one query's five full u32 planes
    for wide in (False, True):
        capped, dense_capped = _resident(engine, g, qseq, qoff, C0, wide, cfg, cap), dense_resident(cap, wide)
        assert capped.workspace_bytes <= cap + 256
        assert capped.stats["n_chunks"] < dense_capped.stats["n_chunks"], (wide, capped.stats["n_chunks"], dense_capped.stats["n_chunks"])
        ref = want if not wide else _one_shot(engine, g, qseq, qoff, C0, True)
        _same(capped, ref, ("capped", wide))
        _same(dense_capped, ref, ("dense, chunked", wide))
    cap = 5 * rpq * max(pitches) * 4   # five queries' footprint in u32 cells
    chunked = _resident(engine, g, qseq, qoff, C0, False, cfg, cap)
    assert chunked.workspace_bytes <= cap + 256 and chunked.layout == {"u16"}
    assert 2 <= chunked.stats["n_chunks"] <= -(-n_q // 5)
    _same(chunked, want, "chunked")
    wide = _resident(engine, g, qseq, qoff, C0, True, cfg, cap)
    assert wide.stats["n_chunks"] == -(-n_q // 5) and wide.layout == set()
    _same(wide, _one_shot(engine, g, qseq, qoff, C0, True), "chunked, u32 cells")
    _same(_resident(engine, g, qseq, qoff, C0, False, cfg, 1), want, "a cap below one query")


# ---- 9. guards and reuse ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_checkpoint2_guards_and_resident_reuse(engine):
    lib, L = engine._lib.lib(), engine._lib
    g, (qseq, qoff) = W.scaled_linearish(200, 10, 5, 8, 180)
    n = len(qoff) - 1
    cfg = _cfg(engine)
    rb = engine.ResidentBatch(g, qseq, qoff, config=cfg)
    dense = engine.ResidentBatch(g, qseq, qoff)
    sweep = engine.ResidentBatch(g, qseq, qoff, config=engine.make_config("score"))
    ck1 = engine.ResidentBatch(g, qseq, qoff, config=engine.make_config("checkpoint"))
    want = _one_shot(engine, g, qseq, qoff, C0, False)
    try:
        # one batch, three cost sets, alternating u16 and u32 cells
        for costs, wide in ((C0, False), (COST_CASES["e2-zero"][0], True), (COST_CASES["mismatch-255"][0], False)):
            _run2(engine, rb, costs, wide, config=cfg)
            got = rb.fetch()
            assert rb.layout() == (set() if wide else {"u16"})
            assert got.stats["plane_bytes"] > 0
            _same(got, _one_shot(engine, g, qseq, qoff, costs, wide), (costs, wide))

        def still_runs(tag):
            _run2(engine, rb, C0, False, config=cfg)
            _same(rb.fetch(), want, ("after", tag))

        def refused(fn, code, tag):
            with pytest.raises(L.PoaError) as e:
                fn()
            assert e.value.code == code, (tag, e.value.code)
            assert lib.poa_last_error() != b"", tag
            still_runs(tag)

        two, one = _gc2(engine, C0), engine.GapAffine(4, 2, 6)
        # a CHECKPOINT2 batch in any other mode, and through the one-piece run
        for other in ("dense", "exact", "hybrid", "score", "checkpoint"):
            refused(lambda: rb.run(two, config=engine.make_config(other)), ERR_INVALID_ARG, ("2piece", other))
            refused(lambda: rb.run(one, config=engine.make_config(other)), ERR_INVALID_ARG, ("1piece", other))
        refused(lambda: rb.run(two), ERR_INVALID_ARG, "2piece, cfg NULL")
        refused(lambda: rb.run(one), ERR_INVALID_ARG, "poa_batch_run")
        refused(lambda: rb.run(one, config=cfg), ERR_INVALID_ARG, "poa_batch_run_ex, mode 5")
        # any other batch in mode 5
        for name, other in (("dense", dense), ("score", sweep), ("checkpoint", ck1)):
            refused(lambda: other.run(two, config=cfg), ERR_INVALID_ARG, (name, "mode 5"))
        # the one-piece entry points asked for mode 5
        refused(lambda: dense.run(one, config=cfg), ERR_UNSUPPORTED, "poa_batch_run_ex")
        with pytest.raises(L.PoaError) as e:
            engine.PoastaAligner(engine.AffineMinGapCost(one), mode="checkpoint2").align_batch(g, qseq=qseq, qoff=qoff)
        assert e.value.code == ERR_UNSUPPORTED and b"2piece" in lib.poa_last_error()
        # ends-free, extend1 < extend2
        ef = engine.make_config("checkpoint2", aln_type=engine.AlignmentType.EndsFree())
        refused(lambda: rb.run(two, config=ef), ERR_UNSUPPORTED, "ends-free run")
        with pytest.raises(L.PoaError) as e:
            engine.ResidentBatch(g, qseq, qoff, config=ef)
        assert e.value.code == ERR_UNSUPPORTED
        bad = L.PoaCosts2(4, 6, 1, 24, 2, 0)   # (the Python cost class refuses these itself: straight to the library)
        refused(lambda: L.check(lib.poa_batch_run_2piece(rb.handle, C.byref(bad), C.byref(cfg), None)), ERR_INVALID_ARG, "extend1 < extend2")
        # what a run leaves to ask for
        refused(lambda: rb.planes(0), ERR_UNSUPPORTED, "planes")
        refused(lambda: rb.planes_2piece(0), ERR_UNSUPPORTED, "planes_2piece")
        refused(lambda: rb.search_counters(), ERR_INVALID_ARG, "search counters")
        # the aligner's one-shot form
        al = engine.PoastaAligner(engine.Affine2PieceDijkstra(two), mode="checkpoint2")
        _same(al.align_batch(g, qseq=qseq, qoff=qoff), want, "aligner")
    finally:
        for b in (rb, dense, sweep, ck1):
            b.close()
    # empty graph and empty batch: as in dense two-piece mode
    empty = GraphBuilder().finish()
    eseq, eoff = pack_queries([b"ACGT", b"", b"A"])
    _same(_one_shot_ckpt(engine, empty, eseq, eoff, C0, False, cfg), _one_shot(engine, empty, eseq, eoff, C0, False), "empty graph, one-shot")
    de = engine.ResidentBatch(empty, eseq, eoff)
    try:
        _run2(engine, de, C0, False)
        _same(_resident(engine, empty, eseq, eoff, C0, False, cfg), de.fetch(), "empty graph, resident")
    finally:
        de.close()
    r = _one_shot_ckpt(engine, g, np.zeros(0, np.uint8), np.zeros(1, np.uint64), C0, False, cfg)
    assert len(r.score) == 0 and len(r.pairs) == 0
    r = _resident(engine, g, np.zeros(0, np.uint8), np.zeros(1, np.uint64), C0, False, cfg)
    assert len(r.score) == 0 and int(r.pair_off[0]) == 0 and n > 0
