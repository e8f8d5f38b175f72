"""The host-side frame of a run, pinned over the engine's eight resident run paths: the cap of 256 runs between two stats /
fetch calls, the reuse of a run's event set by a later run with another chunk count, and the run of a batch without queries.

Every path runs the same tiny inputs: graphs of thirteen nodes with one bubble, queries of at most ten bases (one pitch of 64
columns), gap-affine costs x/o/e = 4/6/2 and the two-piece costs -g 6,24 -e 2,1.  Where a constructor takes workspace_bytes
the batch is capped so that it runs in two chunks: the smallest shape at which the per-chunk layout of the event set matters.
Results are compared with a fresh batch's single run and with the oracle's dense restatement, and equality is demanded."""
import numpy as np
import pytest

from poasta_amd.graph import GraphBuilder, pack_queries

ERR_UNSUPPORTED = -7
COSTS = (4, 2, 6)            # GapAffine's order: mismatch, extend, open
COSTS2 = (4, 2, 6, 1, 24)    # GapAffine2Piece's order: mismatch, extend1, open1, extend2, open2
QUERIES = [b"ACGTACGTAC", b"ACGTTCGAC", b"CGTACGT", b"ACGACGTACA"]


def _bubble_graph(backbone, at, alt):
    """A chain for `backbone` and one more node `alt` beside node `at` of it."""
    b = GraphBuilder()
    ids = b.add_path(np.frombuffer(backbone, np.uint8))
    v = b.add_node(ord(alt))
    b.add_edge(ids[at - 1], v)
    b.add_edge(v, ids[at + 1])
    return b.finish()


# (the same shape under other letters: every query of a multi-graph batch then holds as many bytes, and half the footprint is two of them)
GRAPHS = [_bubble_graph(b"ACGTACGTAC", 4, "T"), _bubble_graph(b"TTGACCAGTA", 4, "C")]

# name -> (kind, mode of the batch, two-piece costs, the run returns pairs)
PATHS = {
    "dense": ("resident", "dense", False, True),
    "score": ("resident", "score", False, False),
    "checkpoint": ("resident", "checkpoint", False, True),
    "dense_2piece": ("resident", "dense", True, True),
    "checkpoint2": ("resident", "checkpoint2", True, True),
    "multi": ("multi", "checkpoint", False, True),
    "multi_2piece": ("multi", "checkpoint2", True, True),
    "scoreset": ("scoreset", "score", False, False),
}
# the text of the refusal, by entry point
REFUSED = {"resident": ": poa_batch_run: call poa_batch_stats/fetch at least every 256 runs",
           "multi": ": poa_multi_run: call poa_multi_stats/fetch at least every 256 runs",
           "multi_2piece": ": poa_multi_run_2piece: call poa_multi_stats/fetch at least every 256 runs",
           "scoreset": ": poa_scoreset_run: call poa_scoreset_stats/fetch at least every 256 runs"}
# what a multi-graph batch and a score set run: queries 0, 1 on graph 0 and 2, 3 on graph 1; the matrix of queries 0..2 x both graphs
MULTI_SEQS = [QUERIES[:2], QUERIES[2:]]
SET_SEQS = QUERIES[:3]


def _make(engine, name, cap=0, empty=False):
    kind, mode, two_piece, _ = PATHS[name]
    if kind == "resident":
        qseq, qoff = pack_queries([] if empty else QUERIES)
        cfg = None if mode == "dense" else engine.make_config(mode)
        return engine.ResidentBatch(GRAPHS[0], qseq, qoff, workspace_bytes=cap, config=cfg)
    if kind == "multi":
        return engine.MultiGraphBatch(GRAPHS, [[], []] if empty else MULTI_SEQS, workspace_bytes=cap, two_piece=two_piece)
    return engine.ScoreSet(GRAPHS, seqs=SET_SEQS, pairs=np.zeros((0, 2), np.int64) if empty else None, workspace_bytes=cap)


def _run(engine, name, b, **tune):
    kind, mode, two_piece, _ = PATHS[name]
    costs = engine.GapAffine2Piece(*COSTS2) if two_piece else engine.GapAffine(*COSTS)
    if kind != "resident":
        cfg = None   # (the binding passes the batch's own mode)
    elif name == "dense":
        # three full u16 planes unless a case says otherwise: half the u32 footprint per query whatever the graph, so that
        # the cap that gives two chunks does not depend on how many D rows the compact layout keeps
        cfg = engine.make_config("dense", **(tune or {"full_planes": True}))
    elif name == "dense_2piece":
        cfg = None
    else:
        cfg = engine.make_config(mode)
    b.run(costs, None, cfg)


def _fetch(name, b):
    """(arrays, stats): score, flags and, where the path has them, pair_off and pairs."""
    kind, _, _, has_pairs = PATHS[name]
    if kind == "scoreset":
        score, flags, st = b.fetch()
        return (score, flags), st
    r = b.fetch(want_pairs=has_pairs)
    return ((r.score, r.flags, r.pair_off, r.pairs) if has_pairs else (r.score, r.flags, r.pair_off)), r.stats


_DENSE = {}


def _oracle_dense(oracle, gi, two_piece):
    """The oracle's dense restatement of all of QUERIES against graph gi, computed once per (graph, model)."""
    if (gi, two_piece) not in _DENSE:
        og = oracle.OracleGraph.from_csr(GRAPHS[gi].as_dict())
        qseq, qoff = pack_queries(QUERIES)
        if two_piece:
            m, e1, o1, e2, o2 = COSTS2
            with oracle.two_piece(o2, e2):
                D = og.dense_batch(qseq, qoff, oracle.Costs(m, o1, e1))
        else:
            m, e, o = COSTS
            D = og.dense_batch(qseq, qoff, oracle.Costs(m, o, e))
        _DENSE[(gi, two_piece)] = D
    return _DENSE[(gi, two_piece)]


def _check_oracle(oracle, name, arrays, what):
    kind, _, two_piece, has_pairs = PATHS[name]
    if kind == "scoreset":   # pair p = (query p // n_graphs, graph p % n_graphs)
        want = [(p % len(GRAPHS), p // len(GRAPHS)) for p in range(len(SET_SEQS) * len(GRAPHS))]
    elif kind == "multi":
        want = [(0, 0), (0, 1), (1, 2), (1, 3)]
    else:
        want = [(0, i) for i in range(len(QUERIES))]
    score = arrays[0]
    assert len(score) == len(want), (name, what)
    counts = np.diff(arrays[2].astype(np.int64)) if has_pairs else None
    for i, (gi, qi) in enumerate(want):
        D = _oracle_dense(oracle, gi, two_piece)
        assert int(score[i]) == int(D["score"][qi]), ("oracle score", name, what, i)
        if has_pairs:
            assert int(counts[i]) == int(D["n_pairs"][qi]), ("oracle pair count", name, what, i)
            got = [tuple(x) for x in arrays[3][int(arrays[2][i]):int(arrays[2][i + 1])].tolist()]
            assert got == oracle.batch_alignment(D, qi), ("oracle alignment", name, what, i)


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, k)


def _footprint(engine, name):
    """Bytes of workspace the uncapped batch plans for.  A dense-mode batch takes any parked workspace that is large enough, so
    what it holds says nothing about its plan: three u32 planes of rows x pitch cells per query, one pitch of 64 columns here."""
    if PATHS[name][:2] == ("resident", "dense"):
        return len(QUERIES) * 3 * GRAPHS[0].n * 64 * 4
    whole = _make(engine, name)
    try:
        return whole.workspace_bytes()
    finally:
        whole.close()


_CAPS = {}


def _two_chunk_cap(engine, name):
    """workspace_bytes under which a run of the path takes two chunks, found once per path from stats() of single runs: half the
    footprint where the run's cells are as wide as those the batch is sized for, a quarter where a u16 run packs twice the
    queries of the u32 cells the batch is sized for."""
    if name not in _CAPS:
        total = _footprint(engine, name)
        seen = []
        for div in (2, 4, 3):
            b = _make(engine, name, cap=total // div)
            try:
                _run(engine, name, b)
                seen.append((total // div, b.stats()["n_chunks"]))
            finally:
                b.close()
            if seen[-1][1] == 2:
                _CAPS[name] = total // div
                break
        else:
            pytest.fail("%s: no cap gave two chunks: %r of %d bytes" % (name, seen, total))
    return _CAPS[name]


_FRESH = {}


def _fresh(engine, name):
    """What a fresh batch's single run returns under the path's two-chunk cap."""
    if name not in _FRESH:
        b = _make(engine, name, cap=_two_chunk_cap(engine, name))
        try:
            _run(engine, name, b)
            arrays, st = _fetch(name, b)
        finally:
            b.close()
        assert st["n_runs"] == 1 and st["n_chunks"] == 2 and st["n_forward_launches"] == 2, (name, st)
        _FRESH[name] = arrays
    return _FRESH[name]


# ---- 1. the cap of 256 event sets ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PATHS))
def test_event_cap(engine, oracle, name):
    """256 runs without stats() or fetch() in between; the 257th is refused with POA_ERR_UNSUPPORTED and costs nothing: the
    statistics count 256 runs of two chunks, a further run succeeds and returns what a fresh batch's single run returns."""
    from poasta_amd import _lib
    fresh = _fresh(engine, name)
    b = _make(engine, name, cap=_two_chunk_cap(engine, name))
    try:
        for _ in range(256):
            _run(engine, name, b)
        with pytest.raises(_lib.PoaError) as ei:
            _run(engine, name, b)
        assert ei.value.code == ERR_UNSUPPORTED, (name, str(ei.value))
        assert str(ei.value).endswith(REFUSED[PATHS[name][0] if name != "multi_2piece" else name]), (name, str(ei.value))
        st = b.stats()
        print(name, "after 256 runs:", {k: st[k] for k in ("n_runs", "n_chunks", "n_forward_launches")})
        assert st["n_runs"] == 256 and st["n_chunks"] == 2 and st["n_forward_launches"] == 256 * 2, (name, st)
        _run(engine, name, b)
        arrays, st = _fetch(name, b)
        assert st["n_runs"] == 1 and st["n_forward_launches"] == 2, (name, st)
    finally:
        b.close()
    _same(arrays, fresh, (name, "after the refused run"))
    _check_oracle(oracle, name, arrays, "after the refused run")


# ---- 2. an event set is reused only by a run with as many chunks ---------------------------------------------------------------
@pytest.mark.gpu
def test_event_set_reuse_across_chunk_counts(engine, oracle):
    """A dense batch capped at half its u32 footprint: a planes=32 run takes the u32 plan, the default run the compact u16 plan
    with fewer chunks.  Both event sets go back to the free list at stats(); the next two runs take the set of their own size."""
    name = "dense"
    b = _make(engine, name, cap=_footprint(engine, name) // 2)
    try:
        _run(engine, name, b, planes=32)
        c32 = b.stats()["n_forward_launches"]
        assert "u16" not in b.layout()
        _run(engine, name, b, full_planes=False)
        c16 = b.stats()["n_forward_launches"]
        assert "u16" in b.layout()
        print("chunks of the u32 plan:", c32, "of the u16 plan:", c16)
        assert c32 == 2 and c16 >= 1 and c16 != c32, (c32, c16)
        for round_ in range(2):
            _run(engine, name, b, planes=32)
            _run(engine, name, b, full_planes=False)
            st = b.stats()
            assert st["n_runs"] == 2 and st["n_forward_launches"] == c32 + c16, (round_, st)
        _run(engine, name, b, planes=32)
        wide, st = _fetch(name, b)
        assert st["n_runs"] == 1 and st["n_forward_launches"] == c32, st
        _run(engine, name, b, full_planes=False)
        narrow, st = _fetch(name, b)
        assert st["n_runs"] == 1 and st["n_forward_launches"] == c16, st
    finally:
        b.close()
    _check_oracle(oracle, name, wide, "u32 plan")
    _check_oracle(oracle, name, narrow, "u16 plan")


# ---- 3. a batch without queries -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PATHS))
def test_empty_batch(engine, name):
    """Zero queries (a score set: zero pairs): the run is recorded as one run, fetch() returns empty arrays, and it does so twice."""
    b = _make(engine, name, empty=True)
    try:
        for _ in range(2):
            _run(engine, name, b)
            st = b.stats()
            assert st["n_runs"] == 1 and st["n_queries"] == 0 and st["n_forward_launches"] == 0, (name, st)
            _run(engine, name, b)
            arrays, st = _fetch(name, b)
            assert st["n_runs"] == 1, (name, st)
            assert len(arrays[0]) == 0 and len(arrays[1]) == 0, name
            if PATHS[name][0] != "scoreset":
                assert arrays[2].tolist() == [0], name
            if PATHS[name][3]:
                assert len(arrays[3]) == 0, name
    finally:
        b.close()
