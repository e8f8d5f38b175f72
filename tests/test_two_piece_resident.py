"""Two-piece model on resident batches: poa_batch_run_2piece / poa_batch_fetch_planes_2piece (poa_engine.hip; kernels of
poa_twopiece.hpp: per-query pitch, plane offset and scratch region).

Yardsticks, bit for bit on score, flags, pair_off and pairs: oracle/dense.hpp through pyoracle, and the one-shot
poa_align_batch_2piece on the same queries (itself a batch run through poa_batch_run_2piece: the same path on a batch of its own).  Graphs and queries are the seeded builders of
tests/test_two_piece_shapes.py: the chain graph, the four-predecessor graph and the MSA graph.

CPU: both symbols exported, declared and refusing a null batch; the chunk count restated in plain Python (`predict_chunks`).
GPU: mixed lengths in one batch in both orders with the planes of the empty, the 512-base and the 2 133-base query (the gap the
shapes test names: a short query's planes inside a batch of long ones); chunked runs against the one-chunk run; five runs of
one batch alternating models and widths; streams; POA_ERR_CAPACITY; score mode; every refusal; scores above 65 535.

Expected plane cell under u16: the oracle's value if it is at most 65534, INF otherwise (the rule of the shapes test)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from poasta_amd import workloads as W
from poasta_amd.graph import pack_queries

from test_two_piece import COSTS2, _oracle_planes_by_row
from test_two_piece_shapes import MISMATCH_255, _assert_batch_equals_oracle, _oracle_graph, _planes_env, _poa, _queries, predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 0xFFFFFFFF
LENS = (0, 1, 63, 64, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2133)
PLANE_LENS = (0, 512, 2133)
C0 = COSTS2[0]                      # (4, 2, 6, 1, 24): mismatch 4, -g 6,24 -e 2,1
COST_CASES = {"cli": (C0, False), "cli-wide": (C0, True), "e2-zero": (COSTS2[4], False), "e2-eq-e1": (COSTS2[3], False),
              "mismatch-255": (MISMATCH_255, False)}
assert COSTS2[4][3] == 0 and COSTS2[3][1] == COSTS2[3][3] and MISMATCH_255[0] == 255


# ---- the engine's chunk plan, in plain Python ---------------------------------------------------------------------------------
def pitch_of(L):
    return (L + 1 + 63) // 64 * 64


def predict_chunks(rows, lengths, workspace_bytes, elem):
    """Chunks of a dense two-piece run as [(first, count)]: a u16 run (elem 2) uses the batch's 4-byte plan, three planes of
    rows x pitch 4-byte elements per query; a u32 run (elem 4) its own plan of five.  The workspace is `workspace_bytes`, raised
    to the largest query's footprint; a chunk closes when the next query does not fit.  (The engine then evens the chunks out
    without changing their number.)"""
    planes = 3 if elem == 2 else 5
    fp3 = [3 * 4 * rows * pitch_of(L) for L in lengths]
    ws = max(workspace_bytes, max(fp3))
    fp = [planes * 4 * rows * pitch_of(L) for L in lengths]
    if elem == 4:
        ws = max(ws, max(fp))
    chunks, first, used = [], 0, 0
    for i, need in enumerate(fp):
        if used + need > ws and i > first:
            chunks.append((first, i - first))
            first, used = i, 0
        used += need
    chunks.append((first, len(fp) - first))
    return chunks


def test_chunk_prediction_on_hand_computed_shapes():
    """Pitches of LENS: 64 64 64 128 256 320 320 512 576 576 1024 1088 1088 2176.  With room for 3 000 columns of three 4-byte
    planes a u16 run cuts after 10, 12 and 13 queries; the u32 run's five planes of the longest query need more than that, its
    workspace grows to 2 176 columns of five planes and it cuts after 8, 11 and 13: three boundaries each, all different."""
    rows = 100
    assert [pitch_of(L) for L in LENS] == [64, 64, 64, 128, 256, 320, 320, 512, 576, 576, 1024, 1088, 1088, 2176]
    ws = 3 * 4 * rows * 3000
    assert predict_chunks(rows, LENS, ws, 2) == [(0, 10), (10, 2), (12, 1), (13, 1)]
    assert predict_chunks(rows, LENS, ws, 4) == [(0, 8), (8, 3), (11, 2), (13, 1)]
    assert predict_chunks(rows, LENS, 0, 2) == [(0, 8), (8, 3), (11, 2), (13, 1)]          # raised to the largest query
    assert predict_chunks(rows, LENS, 3 * 4 * rows * 8256, 2) == [(0, 14)]
    assert len(predict_chunks(rows, LENS, 3 * 4 * rows * 8256, 4)) == 2                     # what held three planes holds 3/5 of five


# ---- CPU: the ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_two_piece_resident_symbols():
    """Exported, declared, bound, and a null batch is POA_ERR_INVALID_ARG before anything touches a device."""
    from poasta_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poasta_amd.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("poa_batch_run_2piece", "poa_batch_fetch_planes_2piece"):
        assert re.search(r"\bint\s+%s\s*\(\s*poa_batch_t\s*\*" % name, hdr), name
        assert hasattr(raw, name) and name in _lib.EXPORTS
    assert re.search(r"poa_batch_run_2piece\(poa_batch_t\* b, const poa_costs2_t\* costs, const poa_config_t\* cfg, void\* stream\);", hdr)
    lib = _lib.lib()
    cs = _lib.PoaCosts2(4, 6, 2, 24, 1, 0)
    assert lib.poa_batch_run_2piece(None, C.byref(cs), None, None) == -1
    assert b"null" in lib.poa_last_error()
    buf = np.zeros(4, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.poa_batch_fetch_planes_2piece(None, 0, p, p, p, p, p) == -1
    from poasta_amd import aligner
    assert hasattr(aligner.ResidentBatch, "planes_2piece")


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
def _gc2(engine, costs):
    m, e1, o1, e2, o2 = costs
    return engine.GapAffine2Piece(m, e1, o1, e2, o2)


def _one_shot(engine, g, qseq, qoff, costs, wide):
    """The yardstick: poa_align_batch_2piece (the one-shot call, unchanged code path)."""
    with _planes_env(wide):
        return engine.PoastaAligner(engine.Affine2PieceDijkstra(_gc2(engine, costs))).align_batch(g, qseq=qseq, qoff=qoff)


def _run2(engine, batch, costs, wide, stream=None, config=None):
    with _planes_env(wide):
        batch.run(_gc2(engine, costs), stream=stream, config=config)


def _same(a, b, tag):
    n = len(a.score)
    assert np.array_equal(a.score, b.score), (tag, "score", np.flatnonzero(a.score != b.score)[:8].tolist())
    assert np.array_equal(a.flags, b.flags), (tag, "flags", np.flatnonzero(a.flags != b.flags)[:8].tolist())
    assert np.array_equal(a.pair_off, b.pair_off), (tag, "pair_off")
    assert np.array_equal(a.pairs[:int(a.pair_off[n])], b.pairs[:int(b.pair_off[n])]), (tag, "pairs")


def _elem(stats, g, lengths):
    cells = g.n * sum(L + 1 for L in lengths)
    assert stats["cells"] == cells and stats["plane_bytes"] % (cells * 5) == 0, stats
    return stats["plane_bytes"] // (cells * 5)


def _one_chunk_bytes(g, lengths):
    """Workspace in which five u32 planes of every query fit at once."""
    return 5 * 4 * g.n * sum(pitch_of(L) for L in lengths)


@functools.lru_cache(maxsize=None)
def _mixed(kind, rev):
    qs = list(_queries(kind, LENS))
    lens = list(LENS)
    if rev:
        qs, lens = qs[::-1], lens[::-1]
    qseq, qoff = pack_queries(qs)
    return qs, lens, qseq, qoff


_oracle_cache = {}


def _oracle_batch(oracle, kind, rev, costs):
    key = (kind, rev, costs)
    if key not in _oracle_cache:
        _, _, qseq, qoff = _mixed(kind, rev)
        m, e1, o1, e2, o2 = costs
        with oracle.two_piece(o2, e2):
            _oracle_cache[key] = _oracle_graph(oracle, kind).dense_batch(qseq, qoff, oracle.Costs(m, o1, e1), threads=8)
    return _oracle_cache[key]


_plane_cache = {}


def _oracle_planes(oracle, engine, kind, L, costs):
    key = (kind, L, costs)
    if key not in _plane_cache:
        g = _poa(kind).graph
        q = _queries(kind, LENS)[LENS.index(L)]
        _plane_cache[key] = _oracle_planes_by_row(oracle, engine, _oracle_graph(oracle, kind), g, q, costs)[1]
    return _plane_cache[key]


# ---- 1. mixed lengths in one batch ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [False, True], ids=["as-listed", "reversed"])
@pytest.mark.parametrize("cname", list(COST_CASES))
@pytest.mark.parametrize("kind", ["chain", "multi", "mixed"])
def test_gpu_resident_mixed_lengths(engine, oracle, kind, cname, rev):
    """Lengths 0 .. 2 133 in one batch, every query under its own pitch: equal to the one-shot call and to the oracle; the cell
    width is the predicted one; the planes of the empty, the 512-base and the 2 133-base query equal the oracle's cell for cell
    (the empty query sits at the first plane offset as listed and at the last one, beside the longest, reversed)."""
    costs, wide = COST_CASES[cname]
    g = _poa(kind).graph
    qs, lens, qseq, qoff = _mixed(kind, rev)
    pred = predict(g, lens, costs, wide)
    want = _one_shot(engine, g, qseq, qoff, costs, wide)
    D = _oracle_batch(oracle, kind, rev, costs)
    rb = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=_one_chunk_bytes(g, lens))
    try:
        _run2(engine, rb, costs, wide)
        got = rb.fetch()
        assert _elem(got.stats, g, lens) == pred["elem"] == _elem(want.stats, g, lens)
        assert got.stats["n_chunks"] == 1 and got.stats["n_forward_launches"] == 1
        assert rb.layout() == ({"u16"} if pred["elem"] == 2 else set())
        _same(got, want, (kind, cname, rev))
        _assert_batch_equals_oracle(got, D, oracle, len(qs), (kind, cname, rev))
        rows = engine._device_graph(g).node_rows()
        for L in PLANE_LENS:
            i = lens.index(L)
            gp = rb.planes_2piece(i)
            for name, a, b in zip(("M", "I1", "D1", "I2", "D2"), gp, _oracle_planes(oracle, engine, kind, L, costs)):
                exp = np.where(b <= 65534, b, np.uint32(INF)) if pred["elem"] == 2 else b
                have = a[rows]
                if not np.array_equal(have, exp):
                    r, c = np.argwhere(have != exp)[0].tolist()
                    pytest.fail("%s %s rev=%s L=%d plane %s: first difference at oracle row %d column %d: got %d, want %d; %d cells differ"
                                % (kind, cname, rev, L, name, r, c, int(have[r, c]), int(exp[r, c]), int((have != exp).sum())))
    finally:
        rb.close()


# ---- 2. chunks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["u16", "u32"])
@pytest.mark.parametrize("kind", ["chain", "multi"])
def test_gpu_resident_chunks(engine, kind, wide):
    """A workspace of 3 000 columns of three 4-byte planes: four chunks at either width, at different boundaries (see
    test_chunk_prediction_on_hand_computed_shapes); results equal the one-chunk run's and the one-shot call's, n_chunks and the
    forward launches are the predicted number, and the planes of the last chunk's query can be fetched, an earlier chunk's not."""
    g = _poa(kind).graph
    qs, lens, qseq, qoff = _mixed(kind, False)
    ws = 3 * 4 * g.n * 3000
    chunks = predict_chunks(g.n, lens, ws, 4 if wide else 2)
    assert len(chunks) >= 4 and len({f for f, _ in chunks}) >= 4
    assert [f for f, _ in chunks] != [f for f, _ in predict_chunks(g.n, lens, ws, 2 if wide else 4)]
    whole = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=_one_chunk_bytes(g, lens))
    cut = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=ws)
    try:
        _run2(engine, whole, C0, wide)
        _run2(engine, cut, C0, wide)
        a, b = whole.fetch(), cut.fetch()
        assert a.stats["n_chunks"] == 1
        assert b.stats["n_chunks"] == len(chunks) == b.stats["n_forward_launches"], (b.stats, chunks)
        assert _elem(b.stats, g, lens) == (4 if wide else 2)
        _same(b, a, (kind, wide, "chunks"))
        _same(b, _one_shot(engine, g, qseq, qoff, C0, wide), (kind, wide, "one-shot"))
        last_first, last_count = chunks[-1]
        gp_cut, gp_whole = cut.planes_2piece(last_first + last_count - 1), whole.planes_2piece(last_first + last_count - 1)
        for x, y in zip(gp_cut, gp_whole):
            assert np.array_equal(x, y)
        with pytest.raises(engine._lib.PoaError) as ei:
            cut.planes_2piece(0)
        assert ei.value.code == -1
        # a second run of the same width reuses the plan: same chunks, same results
        _run2(engine, cut, C0, wide)
        c = cut.fetch()
        assert c.stats["n_chunks"] == len(chunks)
        _same(c, a, (kind, wide, "second run"))
    finally:
        whole.close()
        cut.close()


# ---- 3. one batch, five runs ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_resident_alternating_models(engine):
    """Two-piece costs A, one-piece costs, two-piece costs B in u32 planes, A again, one-piece again on ONE batch with a workspace
    that cuts chunks: every run equals its own yardstick, and after a two-piece run the one-piece plane and counter queries
    answer as after any run that left nothing for them."""
    g = _poa("mixed").graph
    qs, lens, qseq, qoff = _mixed("mixed", False)
    A, B = C0, COSTS2[2]
    one_costs = engine.GapAffine(4, 2, 6)
    y2a = _one_shot(engine, g, qseq, qoff, A, False)
    y2b = _one_shot(engine, g, qseq, qoff, B, True)
    y1 = engine.PoastaAligner(engine.AffineMinGapCost(one_costs)).align_batch(g, qseq=qseq, qoff=qoff)
    rb = engine.ResidentBatch(g, qseq, qoff, workspace_bytes=3 * 4 * g.n * 3000)
    try:
        for step, (model, costs, wide, want) in enumerate([(2, A, False, y2a), (1, None, False, y1), (2, B, True, y2b), (2, A, False, y2a),
                                                            (1, None, False, y1)]):
            if model == 2:
                _run2(engine, rb, costs, wide)
            else:
                with _planes_env(False):
                    rb.run(one_costs)
            got = rb.fetch()
            _same(got, want, ("step", step))
            if model == 2:
                assert _elem(got.stats, g, lens) == (4 if wide else 2)
                assert rb.layout() == (set() if wide else {"u16"})
                with pytest.raises(engine._lib.PoaError) as ei:
                    rb.planes(len(lens) - 1)
                assert ei.value.code == -7
                with pytest.raises(engine._lib.PoaError) as ei:
                    rb.search_counters()
                assert ei.value.code == -1
                assert len(rb.planes_2piece(len(lens) - 1)) == 5
            else:
                with pytest.raises(engine._lib.PoaError) as ei:
                    rb.planes_2piece(len(lens) - 1)
                assert ei.value.code == -1
    finally:
        rb.close()


# ---- 4. streams -------------------------------------------------------------------------------------------------------------------
def _hip(engine):
    """The HIP runtime the engine itself is linked against (already mapped into this process), for streams and copies."""
    engine._lib.lib()
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in os.path.basename(path):
            hip = C.CDLL(path)
            hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipStreamDestroy.argtypes = [C.c_void_p]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return hip
    pytest.fail("the engine's HIP runtime is not mapped")


def _copy_down(hip, ptr, shape, dtype):
    out = np.zeros(shape, dtype)
    if out.nbytes:
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return out


@pytest.mark.gpu
def test_gpu_resident_streams_and_device_results(engine):
    """A run on a non-default stream, two batches in flight on two streams: the sequential results; the device-side result
    buffers (poa_batch_device_results, what poasta_amd/dist.py gathers from), copied down, equal fetch."""
    hip = _hip(engine)
    g = _poa("chain").graph
    _, lens, qseq, qoff = _mixed("chain", False)
    _, _, qseq_r, qoff_r = _mixed("chain", True)
    want, want_r = _one_shot(engine, g, qseq, qoff, C0, False), _one_shot(engine, g, qseq_r, qoff_r, C0, False)
    s1, s2 = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s1)) == 0 and hip.hipStreamCreate(C.byref(s2)) == 0
    assert s1.value and s2.value and s1.value != s2.value
    b1 = engine.ResidentBatch(g, qseq, qoff)
    b2 = engine.ResidentBatch(g, qseq_r, qoff_r)
    try:
        _run2(engine, b1, C0, False, stream=s1.value)
        _same(b1.fetch(), want, "one stream")
        for _ in range(2):   # both in flight, twice: the second round finds the first round's planes and results in place
            _run2(engine, b1, C0, False, stream=s1.value)
            _run2(engine, b2, C0, False, stream=s2.value)
        r1, r2 = b1.fetch(), b2.fetch()
        _same(r1, want, "two streams, first")
        _same(r2, want_r, "two streams, second")
        assert r1.stats["n_runs"] == 2 and r2.stats["n_runs"] == 2
        n = len(lens)
        ptrs = b2.device_results()
        assert np.array_equal(_copy_down(hip, ptrs["score"], n, np.uint32), r2.score)
        assert np.array_equal(_copy_down(hip, ptrs["flags"], n, np.uint32), r2.flags)
        assert np.array_equal(_copy_down(hip, ptrs["pair_off"], n + 1, np.uint64), r2.pair_off)
        total = int(r2.pair_off[n])
        assert total > 0 and np.array_equal(_copy_down(hip, ptrs["pairs"], (total, 2), np.uint32), r2.pairs[:total])
    finally:
        b1.close()
        b2.close()
        hip.hipStreamDestroy(s1)
        hip.hipStreamDestroy(s2)


# ---- 5. POA_ERR_CAPACITY ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_resident_pair_capacity(engine):
    """poa_batch_fetch with a pair buffer one short: POA_ERR_CAPACITY, pair_off[n] holds the needed total, nothing is written
    to the pairs; the batch runs and fetches afterwards as before."""
    lib, p = engine._lib.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    g, (qseq, qoff) = W.scaled_linearish(200, 10, 5, 12, 220)
    n = len(qoff) - 1
    want = _one_shot(engine, g, qseq, qoff, C0, False)
    total = int(want.pair_off[n])
    rb = engine.ResidentBatch(g, qseq, qoff)
    try:
        _run2(engine, rb, C0, False)
        score, flags, pair_off = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
        pairs = np.full((total, 2), 0xA5A5A5A5, np.uint32)
        st = engine._lib.PoaStats()
        rc = lib.poa_batch_fetch(rb.handle, p(score), p(pairs), p(pair_off), total - 1, p(flags), C.byref(st))
        assert rc == -5 and lib.poa_last_error() != b""
        assert int(pair_off[n]) == total and np.array_equal(pair_off, want.pair_off)
        assert (pairs == 0xA5A5A5A5).all()
        assert np.array_equal(score, want.score)
        _same(rb.fetch(), want, "after the refusal, same run")
        _run2(engine, rb, C0, False)
        _same(rb.fetch(), want, "after the refusal, next run")
    finally:
        rb.close()


# ---- 6. score mode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("costs", [C0, (4, 200, 250, 3, 9), (9, 255, 255, 0, 0)], ids=["cli", "open-above-255", "open-510"])
def test_gpu_resident_score_mode(engine, costs):
    """POA_MODE_SCORE on a score batch, under open' = open1 + extend1 - extend2, extend' = extend2: the scores of the dense
    two-piece run, no pairs.  Two of the cost sets have open' above 255 (447 and 510): more than a poa_costs_t could carry."""
    m, e1, o1, e2, o2 = costs
    if costs is not C0:
        assert o1 + e1 - e2 > 255
    g, (qseq, qoff) = W.scaled_linearish(200, 10, 5, 12, 220)
    n = len(qoff) - 1
    cfg = engine.make_config(mode="score")
    dense = engine.ResidentBatch(g, qseq, qoff)
    sweep = engine.ResidentBatch(g, qseq, qoff, config=cfg)
    try:
        _run2(engine, dense, costs, False)
        _run2(engine, sweep, costs, False, config=cfg)
        d, s = dense.fetch(), sweep.fetch(want_pairs=False)
        _same(d, _one_shot(engine, g, qseq, qoff, costs, False), "dense")
        assert np.array_equal(s.score, d.score)
        assert (s.pair_off == 0).all() and int(s.stats["n_queries"]) == n
    finally:
        dense.close()
        sweep.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_resident_refusals(engine):
    """EXACT, HYBRID, CHECKPOINT and ends-free: POA_ERR_UNSUPPORTED with a message; a mode the batch was not created for, an
    unknown mode and extend1 < extend2: POA_ERR_INVALID_ARG.  After each the batch still runs and returns what it returned."""
    lib, L = engine._lib.lib(), engine._lib
    g, (qseq, qoff) = W.scaled_linearish(200, 10, 5, 6, 220)
    want = _one_shot(engine, g, qseq, qoff, C0, False)
    good, bad = L.PoaCosts2(4, 6, 2, 24, 1, 0), L.PoaCosts2(4, 6, 1, 24, 2, 0)
    dense = engine.ResidentBatch(g, qseq, qoff)
    sweep = engine.ResidentBatch(g, qseq, qoff, config=engine.make_config(mode="score"))
    ckpt = engine.ResidentBatch(g, qseq, qoff, config=engine.make_config(mode="checkpoint"))

    def call(batch, costs, **kw):
        cfg = L.PoaConfig()
        for k, v in kw.items():
            setattr(cfg, k, v)
        rc = lib.poa_batch_run_2piece(batch.handle, C.byref(costs), C.byref(cfg), None)
        return rc, lib.poa_last_error().decode(errors="replace")

    try:
        cases = [(dense, good, dict(mode=L.MODE_EXACT), -7), (dense, good, dict(mode=L.MODE_HYBRID), -7),
                 (dense, good, dict(mode=L.MODE_CHECKPOINT), -7), (ckpt, good, dict(mode=L.MODE_CHECKPOINT), -7),
                 (dense, good, dict(span=L.SPAN_ENDS_FREE), -7), (sweep, good, dict(mode=L.MODE_SCORE, span=L.SPAN_ENDS_FREE), -7),
                 (dense, good, dict(mode=L.MODE_SCORE), -1), (sweep, good, dict(mode=L.MODE_DENSE), -1),
                 (ckpt, good, dict(mode=L.MODE_DENSE), -1), (dense, good, dict(mode=5), -1), (dense, good, dict(span=2), -1),
                 (dense, bad, dict(), -1), (sweep, bad, dict(mode=L.MODE_SCORE), -1)]
        for batch, costs, kw, code in cases:
            rc, err = call(batch, costs, **kw)
            assert rc == code and err != "", (kw, rc, err)
            if costs is bad:
                assert "gap_extend1" in err
            assert call(dense, good)[0] == 0
            _same(dense.fetch(), want, ("after", kw))
        assert lib.poa_batch_run_2piece(dense.handle, None, None, None) == -1
        assert call(sweep, good, mode=L.MODE_SCORE)[0] == 0
        assert np.array_equal(sweep.fetch(want_pairs=False).score, want.score)
        # the checkpointed batch still runs in its own mode (one-piece)
        ckpt.run(engine.GapAffine(4, 2, 6), config=engine.make_config(mode="checkpoint"))
        one = engine.PoastaAligner(engine.AffineMinGapCost(engine.GapAffine(4, 2, 6))).align_batch(g, qseq=qseq, qoff=qoff)
        _same(ckpt.fetch(), one, "checkpointed batch afterwards")
    finally:
        for b in (dense, sweep, ckpt):
            b.close()


# ---- 8. scores above 65 535 -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_resident_scores_above_u16(engine, oracle):
    """The 36 602-row graph of test_gpu_two_piece_scores_above_u16 with two of its queries: u32 cells by the rule, real u32
    values.  The batch's workspace was sized for three planes per query, so this also runs the five-plane plan's chunks."""
    g, (qseq, qoff) = W.scaled_linearish(36000, 300, 150, 2, 1500)
    costs, lengths = (4, 2, 6, 2, 24), [1500, 1500]
    assert predict(g, lengths, costs, False)["elem"] == 4
    rb = engine.ResidentBatch(g, qseq, qoff)
    try:
        _run2(engine, rb, costs, False)
        got = rb.fetch()
    finally:
        rb.close()
    assert _elem(got.stats, g, lengths) == 4 and rb.n == 2
    assert got.stats["n_chunks"] == len(predict_chunks(g.n, lengths, 3 * 4 * g.n * 2 * pitch_of(1500), 4)) == 2
    assert int(got.score.min()) > 65534
    _same(got, _one_shot(engine, g, qseq, qoff, costs, False), "u32 values")
    og = oracle.OracleGraph.from_csr(g.as_dict())
    with oracle.two_piece(24, 2):
        D = og.dense_batch(qseq, qoff, oracle.Costs(4, 6, 2), threads=2)
    assert int(D["score"][0]) == 69336
    _assert_batch_equals_oracle(got, D, oracle, 2, "u32 values")
