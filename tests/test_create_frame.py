"""The host-side frame of a create, pinned over the engine's batch constructors: the device refusals and their texts, a null
`out`, the workspace and chunks a cap gives, the upload time a batch reports, and creation after destruction.  With it the
stand-alone check of the pure rules the constructors and the one-shot two-piece calls share (tests/create_host), on the CPU
under the sanitizers.

Every constructor gets the inputs of test_run_frame.py: the two graphs of thirteen nodes with one bubble, the four queries of
at most ten bases (one pitch of 64 columns), costs 4/6/2 and -g 6,24 -e 2,1.  All items of a batch (queries; pairs of a score
set) then hold as many bytes, so the greedy rule is a division: a workspace of k items gives ceil(n / k) chunks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from poasta_amd.graph import pack_queries

import test_run_frame as TRF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = -1
GRAPHS, QUERIES = TRF.GRAPHS, TRF.QUERIES
PITCH = 64

# name -> (kind, mode of the batch, two-piece costs, the run returns pairs): test_run_frame's resident batches (the dense
# two-piece run is a run path, not a constructor), both checkpointed multi-graph batches, the dense one, the score set
KINDS = {
    "dense": ("resident", "dense", False, True),
    "score": ("resident", "score", False, False),
    "checkpoint": ("resident", "checkpoint", False, True),
    "checkpoint2": ("resident", "checkpoint2", True, True),
    "multi": ("multi", "checkpoint", False, True),
    "multi_2piece": ("multi", "checkpoint2", True, True),
    "multi_dense": ("multi", "dense", False, True),
    "scoreset": ("scoreset", "score", False, False),
}
# The text of the device refusal, copied from the constructors as they stood before they shared the frame:
#   batch_create_impl (poa_batch_create and poa_batch_create_ex):  "poa_batch_create: device ordinal out of range"
#   multi_create_impl:                                             who + ": device ordinal out of range", who the entry point
#   poa_multi_create_dense:                                        who + ": device ordinal out of range"
#   poa_scoreset_create:                                           "poa_scoreset_create: device ordinal out of range"
DEVICE_REFUSAL = {
    "dense": b"poa_batch_create: device ordinal out of range",
    "score": b"poa_batch_create: device ordinal out of range",
    "checkpoint": b"poa_batch_create: device ordinal out of range",
    "checkpoint2": b"poa_batch_create: device ordinal out of range",
    "multi": b"poa_multi_create: device ordinal out of range",
    "multi_2piece": b"poa_multi_create_2piece: device ordinal out of range",
    "multi_dense": b"poa_multi_create_dense: device ordinal out of range",
    "scoreset": b"poa_scoreset_create: device ordinal out of range",
}


def _config(engine, name):
    mode = KINDS[name][1]
    return None if name == "dense" else engine.make_config(mode)


def _raw_create(engine, name, device, out, empty=False, cap=0):
    """The constructor of the kind through the C ABI itself: its return code, with `out` as given (None: a null pointer)."""
    from poasta_amd import _lib
    L = _lib.lib()
    kind, mode, two_piece, _ = KINDS[name]
    cfg = _config(engine, name)
    cfg_p = C.byref(cfg) if cfg is not None else None
    p = engine._p
    if kind == "resident":
        dg = engine._device_graph(GRAPHS[0])
        qseq, qoff = pack_queries([] if empty else QUERIES)
        qseq, qoff = np.ascontiguousarray(qseq, np.uint8), np.ascontiguousarray(qoff, np.uint64)
        if cfg is None:
            return L.poa_batch_create(dg.handle, device, len(qoff) - 1, p(qseq), p(qoff), cap, out)
        return L.poa_batch_create_ex(dg.handle, device, len(qoff) - 1, p(qseq), p(qoff), cfg_p, cap, out)
    if kind == "multi":
        mi = engine._MultiInput(GRAPHS, [[], []] if empty else TRF.MULTI_SEQS)
        create = L.poa_multi_create_2piece if two_piece else (L.poa_multi_create_dense if mode == "dense" else L.poa_multi_create)
        return create(mi.handles, mi.n_graphs, p(mi.graph_qoff), device, p(mi.qseq), p(mi.qoff), cfg_p, cap, out)
    si = engine._ScoreSetInput(GRAPHS, seqs=TRF.SET_SEQS, pairs=np.zeros((0, 2), np.int64) if empty else None)
    return L.poa_scoreset_create(si.handles, si.n_graphs, device, si.n_queries, p(si.qseq), p(si.qoff), *si.pair_args(), cfg_p, cap, out)


def _make(engine, name, cap=0, empty=False):
    from poasta_amd import _lib
    kind, mode, two_piece, _ = KINDS[name]
    if kind == "resident":
        if name == "dense":
            # a dense-mode batch takes any parked workspace that is large enough: with nothing parked it holds what it planned for
            _lib.lib().poa_release_cache()
        qseq, qoff = pack_queries([] if empty else QUERIES)
        return engine.ResidentBatch(GRAPHS[0], qseq, qoff, workspace_bytes=cap, config=_config(engine, name))
    if kind == "multi":
        return engine.MultiGraphBatch(GRAPHS, [[], []] if empty else TRF.MULTI_SEQS, workspace_bytes=cap, two_piece=two_piece, dense=mode == "dense")
    return engine.ScoreSet(GRAPHS, seqs=TRF.SET_SEQS, pairs=np.zeros((0, 2), np.int64) if empty else None, workspace_bytes=cap)


def _run(engine, name, b):
    kind, mode, two_piece, _ = KINDS[name]
    costs = engine.GapAffine2Piece(*TRF.COSTS2) if two_piece else engine.GapAffine(*TRF.COSTS)
    if kind != "resident":
        cfg = None   # (the binding passes the batch's own mode)
    elif name == "dense":
        cfg = engine.make_config("dense", full_planes=True)   # three full u16 planes: half the u32 footprint whatever the graph
    else:
        cfg = engine.make_config(mode)
    b.run(costs, None, cfg)


def _fetch(name, b):
    kind, _, _, has_pairs = KINDS[name]
    if kind == "scoreset":
        score, flags, st = b.fetch()
        return (score, flags), st
    r = b.fetch(want_pairs=has_pairs)
    return ((r.score, r.flags, r.pair_off, r.pairs) if has_pairs else (r.score, r.flags, r.pair_off)), r.stats


def _items(engine, name):
    """(n, bytes the batch is sized for per item, bytes a run addresses per item): from the kind's footprint call, and for a
    resident batch, which has none, from the graph's own numbers.  The costs allow u16 cells (6 + 2 x 10 + 6 + 2 x 13 is far
    below 65534), so a resident dense, checkpointed or two-piece checkpointed run packs two queries where the batch, sized for
    u32 cells, counts one; a score-only batch and the batches built around a plan cut their chunks once, for both widths."""
    kind, mode, two_piece, _ = KINDS[name]
    if kind == "resident":
        dg = engine._device_graph(GRAPHS[0])
        if mode == "dense":
            rows = 3 * GRAPHS[0].n
        elif mode == "score":
            rows = 2 * max(dg.sweep_slots()[1], 1)
        else:
            rows = dg.checkpoint_plan(two_piece=two_piece)[1]
        sized = rows * PITCH * 4
        return len(QUERIES), sized, sized if mode == "score" else sized // 2
    if kind == "multi":
        total, largest = engine.multi_footprint(GRAPHS, TRF.MULTI_SEQS, two_piece=two_piece, dense=mode == "dense")
        n = len(QUERIES)
    else:
        total, largest = engine.scoreset_footprint(GRAPHS, seqs=TRF.SET_SEQS)
        n = len(TRF.SET_SEQS) * len(GRAPHS)
    assert total == n * largest, (name, total, largest)   # equal items: the premise of this module
    return n, largest, largest


def _predict(engine, name, cap):
    """(workspace_bytes(), n_chunks) by the workspace rule and the greedy rule.  Device memory is ample for a few kilobytes, so
    a cap of 0 is the whole footprint; a cap below the largest item is raised to it; a resident batch adds 256 bytes."""
    n, sized, addressed = _items(engine, name)
    ws = max(n * sized if cap == 0 else cap, sized)
    per_chunk = ws // addressed if ws < n * sized else n   # (a batch in one chunk has one plan, the u32 one)
    n_chunks = -(-n // per_chunk)
    if KINDS[name][0] == "resident":
        return ws + 256, n_chunks
    return min(per_chunk, n) * sized, n_chunks   # what the largest chunk holds


def _two_chunk_cap(engine, name):
    """Half the footprint at the run's cell width."""
    n, sized, addressed = _items(engine, name)
    return n * addressed // 2


# ---- 0. the pure rules, on the CPU ---------------------------------------------------------------------------------------------
def test_create_host_rules_under_sanitizers(tmp_path):
    """tests/create_host: choose_workspace against a table written out from the constructors' former code, two_piece_workspace
    against the budgets and chunk counts of the one-shot two-piece call's former workspace of its own, concat_tables with a
    repeated handle and an empty table — a program of its own, address and undefined-behaviour sanitizers on."""
    csrc = os.path.join(ROOT, "poasta_amd", "csrc")
    exe = os.path.join(str(tmp_path), "create_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "create_host", "create_host.cpp"), os.path.join(csrc, "poa_dense_plan.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert b"create_host ok" in r.stdout


# ---- 1. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KINDS))
def test_device_refusals(engine, name):
    """device = -1 and device = poa_device_count(): POA_ERR_INVALID_ARG, the handle stays null, the text is the entry point's."""
    from poasta_amd import _lib
    for empty in (False, True):
        for device in (-1, _lib.lib().poa_device_count()):
            h = C.c_void_p(0xDEAD)   # (the constructor clears it before anything else)
            rc = _raw_create(engine, name, device, C.byref(h), empty=empty)
            assert rc == ERR_INVALID_ARG, (name, device, rc)
            assert not h.value, (name, device)
            assert _lib.lib().poa_last_error() == DEVICE_REFUSAL[name], (name, device, _lib.lib().poa_last_error())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KINDS))
def test_null_out(engine, name):
    for empty in (False, True):
        assert _raw_create(engine, name, 0, None, empty=empty) == ERR_INVALID_ARG, name


# ---- 2. what a cap gives -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KINDS))
def test_caps(engine, oracle, name):
    """Caps of 0, half the footprint and 1: the workspace and the chunks are the rule's, the results are equal."""
    n, sized, _ = _items(engine, name)
    seen = []
    for cap in (0, _two_chunk_cap(engine, name), 1):
        b = _make(engine, name, cap=cap)
        try:
            held = b.workspace_bytes()
            _run(engine, name, b)
            arrays, st = _fetch(name, b)
        finally:
            b.close()
        want = _predict(engine, name, cap)
        print(name, "cap", cap, "workspace", held, "chunks", st["n_chunks"], "predicted", want)
        assert (held, st["n_chunks"]) == want, (name, cap)
        assert st["n_queries"] == n and st["n_runs"] == 1, (name, cap, st)
        seen.append((cap, st["n_chunks"], arrays))
    assert [c for _, c, _ in seen][:2] == [1, 2], name   # one chunk without a cap, two at half the footprint
    assert held == sized + (256 if KINDS[name][0] == "resident" else 0), (name, held)   # cap 1: the largest item alone
    for cap, _, arrays in seen[1:]:
        TRF._same(arrays, seen[0][2], (name, "cap", cap))
    if name in TRF.PATHS:
        TRF._check_oracle(oracle, name, seen[0][2], "no cap")


# ---- 3. the upload time belongs to creation ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KINDS))
def test_ms_h2d(engine, name):
    """poa_stats_t.ms_h2d is there after create and no run changes it."""
    b = _make(engine, name)
    try:
        created = b.stats()["ms_h2d"]
        assert created > 0.0, (name, created)
        _run(engine, name, b)
        first = b.stats()
        _run(engine, name, b)
        second = b.stats()
    finally:
        b.close()
    print(name, "ms_h2d", created)
    assert first["n_runs"] == 1 and second["n_runs"] == 1, (name, first, second)
    assert first["ms_h2d"] == created and second["ms_h2d"] == created, (name, created, first["ms_h2d"], second["ms_h2d"])


# ---- 4. create, destroy, create again ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("empty", [False, True], ids=["queries", "empty"])
def test_create_again(engine, name, empty):
    """The second batch takes the buffers the first released; it holds as much and returns the same."""
    got = []
    for _ in range(2):
        b = _make(engine, name, empty=empty)
        try:
            held = b.workspace_bytes()
            _run(engine, name, b)
            arrays, st = _fetch(name, b)
        finally:
            b.close()
        assert st["n_runs"] == 1 and st["n_queries"] == (0 if empty else _items(engine, name)[0]), (name, st)
        assert st["ms_h2d"] >= 0.0, (name, st)
        got.append((held, arrays))
    assert got[0][0] == got[1][0] == (0 if empty else _predict(engine, name, 0)[0]), (name, got[0][0], got[1][0])
    TRF._same(got[1][1], got[0][1], (name, "second batch"))
    if empty:
        assert len(got[0][1][0]) == 0 and len(got[0][1][1]) == 0, name
