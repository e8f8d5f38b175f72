"""Host-side mirror of the reference's aligner entry point, running on the gfx950 engine.

Mirrors `poasta::aligner::PoastaAligner` (/root/reference/src/aligner/mod.rs:40-146) and the types a
caller touches: `GapAffine` (scoring/gap_affine.rs:20-30), the `AlignmentConfig` bindings
`AffineMinGapCost` / `AffineDijkstra` (config.rs:49,:104), `AlignmentType` (scoring/mod.rs:50-62),
`AstarResult` (astar.rs:81-90) and `AlignedPair` (alignment.rs:4-13).  Same names, same argument
meaning; errors are exceptions where the reference panics.

What differs, by design: a call computes the full M/I/D score planes on the GPU instead of searching
them with A*; `AstarResult.flags` reports when the reference's own search order could have picked
a different co-optimal alignment (0 = provably the reference's alignment).
`align_batch` is the data-parallel shape of `lasagna align` (src/bin/lasagna.rs:184-276).
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .graph import FlatGraph, pack_queries


class GapAffine:
    """`GapAffine::new(cost_mismatch, cost_gap_extend, cost_gap_open)` — NB the argument order
    (scoring/gap_affine.rs:27)."""

    def __init__(self, cost_mismatch, cost_gap_extend, cost_gap_open):
        for v in (cost_mismatch, cost_gap_extend, cost_gap_open):
            if not 0 <= int(v) <= 255:
                raise ValueError("GapAffine costs are u8")
        self.cost_mismatch, self.cost_gap_extend, self.cost_gap_open = int(cost_mismatch), int(cost_gap_extend), int(cost_gap_open)

    def mismatch(self):
        return self.cost_mismatch

    def gap_open(self):
        return self.cost_gap_open

    def gap_extend(self):
        return self.cost_gap_extend

    def gap_cost(self, in_gap_state, length):
        """gap_affine.rs:68-80; in_gap_state False == AlignState::Match."""
        if length == 0:
            return 0
        return (0 if in_gap_state else self.cost_gap_open) + length * self.cost_gap_extend

    def _c(self):
        return _lib.PoaCosts(self.cost_mismatch, self.cost_gap_open, self.cost_gap_extend, 0)


class GapAffine2Piece:
    """`GapAffine2Piece::new(cost_mismatch, cost_gap_extend1, cost_gap_open1, cost_gap_extend2, cost_gap_open2)` — the
    reference's argument order (gap_affine_2piece.rs:28-33); it panics unless extend1 >= extend2."""

    def __init__(self, cost_mismatch, cost_gap_extend1, cost_gap_open1, cost_gap_extend2, cost_gap_open2):
        if cost_gap_extend1 < cost_gap_extend2:
            raise ValueError("gap_extend1 must be greater than or equal to gap_extend2 for two-piece model")
        self.cost_mismatch, self.cost_gap_extend1, self.cost_gap_open1 = cost_mismatch, cost_gap_extend1, cost_gap_open1
        self.cost_gap_extend2, self.cost_gap_open2 = cost_gap_extend2, cost_gap_open2

    def mismatch(self):
        return self.cost_mismatch

    def gap_open(self):
        return self.cost_gap_open1

    def gap_extend(self):
        return self.cost_gap_extend1

    def gap_open2(self):
        return self.cost_gap_open2

    def gap_extend2(self):
        return self.cost_gap_extend2

    def breakpoint(self):
        """gap_affine_2piece.rs:36-66"""
        if self.cost_gap_extend1 == self.cost_gap_extend2:
            return (1 << 64) - 1 if self.cost_gap_open1 <= self.cost_gap_open2 else 0
        den = self.cost_gap_extend1 - self.cost_gap_extend2
        if self.cost_gap_open2 >= self.cost_gap_open1:
            return (self.cost_gap_open2 - self.cost_gap_open1) // den
        return (self.cost_gap_open1 - self.cost_gap_open2 + den - 1) // den

    def _c(self):
        return _lib.PoaCosts2(self.cost_mismatch, self.cost_gap_open1, self.cost_gap_extend1, self.cost_gap_open2, self.cost_gap_extend2,
                              1 if os.environ.get("POA_PLANES") == "32" else 0)


class Affine2PieceDijkstra:
    """config.rs:160-213.  The engine's two-piece pass is the dense one (Global): the optimum of the reference's two-piece
    alignment graph = what this configuration's search returns without pruning (`align_no_pruning`)."""
    heuristic = _lib.HEURISTIC_DIJKSTRA
    two_piece = True

    def __init__(self, costs):
        self.costs = costs


class Affine2PieceMinGapCost:
    """config.rs:215-272 — what `poasta align -g o1,o2 -e e1,e2` constructs (src/bin/poasta.rs:319-445).  Its results are
    those of the reference's SEARCH (min-gap heuristic over a gap_cost that charges the open cost again inside a gap,
    pruning): run it with `PoastaAligner(config, aln_type, mode="exact")`."""
    heuristic = _lib.HEURISTIC_MINGAP
    two_piece = True

    def __init__(self, costs):
        self.costs = costs


class Bound:
    """std::ops::Bound<usize> as the reference's AlignmentType::EndsFree uses it."""
    Unbounded = (_lib.BOUND_UNBOUNDED, 0)

    @staticmethod
    def Included(n):
        return (_lib.BOUND_INCLUDED, int(n))

    @staticmethod
    def Excluded(n):
        return (_lib.BOUND_EXCLUDED, int(n))


class EndsFree:
    """AlignmentType::EndsFree {qry_free_begin, qry_free_end, graph_free_begin, graph_free_end} (scoring/mod.rs:56-61).
    What the reference returns for it is defined by its search (gap_affine.rs:136-248), so the engine replays that
    search for every query (exact mode is implied)."""

    def __init__(self, qry_free_begin=Bound.Unbounded, qry_free_end=Bound.Unbounded, graph_free_begin=Bound.Unbounded,
                 graph_free_end=Bound.Unbounded):
        self.bounds = (qry_free_begin, qry_free_end, graph_free_begin, graph_free_end)


class AlignmentType:
    """scoring/mod.rs:50-62: `AlignmentType.Global` (what `lasagna` hard-codes, src/bin/lasagna.rs:256) or
    `AlignmentType.EndsFree(...)`."""
    Global = "global"
    EndsFree = EndsFree


class AffineMinGapCost:
    """config.rs:104 — the default config of both reference CLIs.  The heuristic only fixes the
    reference's search order: the dense GPU pass has none, the exact replay emulates it."""
    heuristic = _lib.HEURISTIC_MINGAP

    def __init__(self, costs):
        self.costs = costs


class AffineDijkstra(AffineMinGapCost):
    """config.rs:49."""
    heuristic = _lib.HEURISTIC_DIJKSTRA


MODES = {"dense": _lib.MODE_DENSE, "exact": _lib.MODE_EXACT, "hybrid": _lib.MODE_HYBRID, "score": _lib.MODE_SCORE,
         "checkpoint": _lib.MODE_CHECKPOINT, "checkpoint2": _lib.MODE_CHECKPOINT2}


def make_config(mode="dense", heuristic=_lib.HEURISTIC_MINGAP, pruning=True, queue_entries_per_cell=0.0, full_planes=False,
                aln_type=AlignmentType.Global, wide_queries=False, **tune):
    """poa_config_t: `mode` "dense" | "exact" (replay the reference's A* for every query: bit-identical
    tie-breaks) | "hybrid" (replay only the queries the dense pass could not certify) | "score" (forward sweep only: dense
    mode's scores, no alignment, memory for the live rows only) | "checkpoint" (dense mode's results from a slot-sized
    workspace: sweep with snapshots, then recompute-and-walk per segment; ckpt_rows=k overrides the segment length) |
    "checkpoint2" (the same for the two-piece model: the dense two-piece pass's results, two-piece entry points only);
    `aln_type` Global or EndsFree(...).  `wide_queries`: POA_CFG_WIDE_QUERIES, read when a dense or exact multi-graph batch is
    sized or created (queries of more than 1023 symbols); multi_footprint and MultiGraphBatch set it themselves where needed."""
    cfg = _lib.PoaConfig(MODES[mode] if isinstance(mode, str) else int(mode), int(heuristic), 1 if pruning else 0,
                         float(queue_entries_per_cell),
                         (_lib.CFG_FULL_PLANES if full_planes else 0) | (_lib.CFG_WIDE_QUERIES if wide_queries else 0))
    if isinstance(aln_type, EndsFree):
        cfg.span = _lib.SPAN_ENDS_FREE
        for name, (kind, value) in zip(("qry_free_begin", "qry_free_end", "graph_free_begin", "graph_free_end"), aln_type.bounds):
            setattr(cfg, name, _lib.PoaBound(kind, value))
    _lib.tune_from_env(cfg, **tune)   # kernel / layout overrides: POA_<NAME> variables, keyword arguments (poa_config_t.tune)
    return cfg


LAUNCH_KERNELS = ("none", "forward", "packed", "px", "pxmw", "band")   # POA_KERNEL_* of include/poasta_amd.h
REPLAY_KERNELS = ("none", "lane", "wave_lds", "wave_groups", "wave_generic", "flat_generic", "flat_lean")   # POA_REPLAY_*


def _replay_records(call, handle, n_queries):
    """The per-chunk records of poa_batch_replay_info / poa_multi_replay_info as dicts."""
    out = []
    while True:
        v = (C.c_uint32 * 8)()
        rc = call(handle, len(out), v)
        if rc == -1 and (out or n_queries == 0):   # past the last chunk
            return out
        _lib.check(rc)
        out.append({"kernel": REPLAY_KERNELS[v[0]], "win": int(v[1]), "lanes": int(v[2]), "waves": int(v[3]),
                    "graph_lds": bool(v[4] & 1), "rec_lds": bool(v[4] & 2), "ring_global": bool(v[4] & 4), "persistent": bool(v[4] & 8),
                    "resident": int(v[5]), "blocks": int(v[6]), "lds_bytes": int(v[7])})


class AlignedPair:
    __slots__ = ("rpos", "qpos")

    def __init__(self, rpos, qpos):
        self.rpos, self.qpos = rpos, qpos

    def is_aligned(self):
        return self.rpos is not None and self.qpos is not None

    def is_indel(self):
        return not self.is_aligned()

    def __eq__(self, o):
        return (self.rpos, self.qpos) == (o.rpos, o.qpos)

    def __repr__(self):
        return "AlignedPair(rpos=%r, qpos=%r)" % (self.rpos, self.qpos)


class AstarResult:
    """astar.rs:81-90.  `num_*` search counters have no meaning for a dense pass and are 0;
    `cells` = rows x (len + 1) computed for this query."""

    def __init__(self, score, alignment, flags=0, cells=0):
        self.score, self.alignment, self.flags, self.cells = score, alignment, flags, cells
        self.num_queued = self.num_visited = self.num_pruned = 0

    def pairs(self):
        return [(p.rpos, p.qpos) for p in self.alignment]


class BatchResult:
    """Struct-of-arrays result of `align_batch`."""

    def __init__(self, score, pairs, pair_off, flags, stats):
        self.score, self.pairs, self.pair_off, self.flags, self.stats = score, pairs, pair_off, flags, stats

    def __len__(self):
        return len(self.score)

    def alignment(self, i):
        """[(rpos|None, qpos|None), ...] of query i."""
        a = self.pairs[int(self.pair_off[i]):int(self.pair_off[i + 1])]
        return [(None if r == _lib.POA_NONE else int(r), None if q == _lib.POA_NONE else int(q)) for r, q in a.tolist()]

    def raw_alignment(self, i):
        return [tuple(x) for x in self.pairs[int(self.pair_off[i]):int(self.pair_off[i + 1])].tolist()]

    def result(self, i):
        return AstarResult(int(self.score[i]), [AlignedPair(r, q) for r, q in self.alignment(i)], int(self.flags[i]))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class DeviceGraph:
    """Owns a `poa_graph_t` (the flattened AlignableRefGraph)."""

    def __init__(self, graph):
        if not isinstance(graph, FlatGraph):
            graph = FlatGraph.from_dict(graph)
        self.graph = graph
        h = C.c_void_p()
        _lib.check(_lib.lib().poa_graph_create(graph.n, graph.start, graph.end, _p(graph.symbol), _p(graph.succ_off),
                                               _p(graph.succ), _p(graph.pred_off), _p(graph.pred), C.byref(h)))
        self.handle = h

    def node_rows(self):
        r = np.zeros(self.graph.n, np.uint32)
        _lib.check(_lib.lib().poa_graph_node_rows(self.handle, _p(r)))
        return r

    def sweep_slots(self):
        """(slot, n_slots) of the score-only sweep: slot[row] (POA_NONE: never read back), rows alive at once."""
        slot = np.zeros(max(self.graph.n, 1), np.uint32)
        n = C.c_uint32(0)
        _lib.check(_lib.lib().poa_graph_sweep_slots(self.handle, _p(slot), C.byref(n)))
        return slot[:self.graph.n], int(n.value)

    def sweep_checks(self, stride=0):
        """check[row] of a capped score-set run (poa_graph_sweep_checks): 1 where a wave compares the row's smallest M value with
        its cap — the cut rows (no edge skips them) without the end row, at least `stride` rows apart (0: the engine's default)."""
        check = np.zeros(max(self.graph.n, 1), np.uint8)
        n = C.c_uint32(0)
        _lib.check(_lib.lib().poa_graph_sweep_checks(self.handle, int(stride), _p(check), C.byref(n)))
        assert int(check[:self.graph.n].sum()) == n.value
        return check[:self.graph.n]

    def checkpoint_plan(self, segment_rows=0, two_piece=False):
        """(boundary, rows_per_query) of the checkpointed mode: boundary[0] = 0 < ... < boundary[-1] = rows cut the rows into
        segments of segment_rows rows (0: the engine's choice); rows_per_query = plane rows of `pitch` cells a query holds.
        two_piece: the plan of mode "checkpoint2" (three kept planes, five window planes; its own default segment length)."""
        plan = _lib.lib().poa_graph_checkpoint_plan2 if two_piece else _lib.lib().poa_graph_checkpoint_plan
        n_seg, rpq = C.c_uint32(0), C.c_uint32(0)
        _lib.check(plan(self.handle, int(segment_rows), C.byref(n_seg), None, C.byref(rpq)))
        boundary = np.zeros(n_seg.value + 1, np.uint32)
        _lib.check(plan(self.handle, int(segment_rows), C.byref(n_seg), _p(boundary), C.byref(rpq)))
        return boundary, int(rpq.value)

    def __del__(self):
        try:
            if self.handle:
                _lib.lib().poa_graph_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def sweep_checks(graph, stride=0):
    """The check rows of `graph` in a capped score-set run, a u8 array by row (DeviceGraph.sweep_checks)."""
    return _device_graph(graph).sweep_checks(stride)


def _device_graph(graph):
    if isinstance(graph, DeviceGraph):
        return graph
    dg = getattr(graph, "_device_graph", None)
    if dg is None:
        dg = DeviceGraph(graph)
        try:
            graph._device_graph = dg
        except Exception:
            pass
    return dg


class ResidentBatch:
    """Queries + results resident in HBM (`poa_batch_*`): create once, run many times."""

    def __init__(self, graph, qseq, qoff, device=0, workspace_bytes=0, config=None):
        """config: the poa_config_t the batch will run with — needed for modes "score", "checkpoint" and "checkpoint2", whose
        batches hold slots (and snapshots and a segment window) instead of planes (poa_batch_create_ex) and run in no other mode."""
        self.dg = _device_graph(graph)
        self.qseq = np.ascontiguousarray(qseq, np.uint8)
        self.qoff = np.ascontiguousarray(qoff, np.uint64)
        self.n = len(self.qoff) - 1
        h = C.c_void_p()
        if config is None:
            _lib.check(_lib.lib().poa_batch_create(self.dg.handle, device, self.n, _p(self.qseq), _p(self.qoff),
                                                   int(workspace_bytes), C.byref(h)))
        else:
            _lib.check(_lib.lib().poa_batch_create_ex(self.dg.handle, device, self.n, _p(self.qseq), _p(self.qoff),
                                                      C.byref(config), int(workspace_bytes), C.byref(h)))
        self.handle = h
        self.pair_capacity = int(self.qoff[-1]) + self.n * self.dg.graph.n

    def run(self, costs, stream=None, config=None):
        """Launch on `stream` without synchronising.  costs: GapAffine (poa_batch_run_ex) or GapAffine2Piece
        (poa_batch_run_2piece: the dense two-piece pass, the score-only sweep on a batch created for mode "score", or the
        checkpointed two-piece passes on a batch created for mode "checkpoint2" — pass that config to the run as well)."""
        c = costs._c()
        if isinstance(costs, GapAffine2Piece):
            _lib.check(_lib.lib().poa_batch_run_2piece(self.handle, C.byref(c), C.byref(config) if config is not None else None,
                                                       C.c_void_p(stream or 0)))
            return
        if config is None:
            config = _lib.tune_from_env()   # (a dense-mode config carrying the overrides, if any are set)
        if config is None:
            _lib.check(_lib.lib().poa_batch_run(self.handle, C.byref(c), C.c_void_p(stream or 0)))
        else:
            _lib.check(_lib.lib().poa_batch_run_ex(self.handle, C.byref(c), C.byref(config), C.c_void_p(stream or 0)))

    def fetch(self, want_pairs=True, pinned=False, copy=False):
        """Synchronise and copy the results to the host.  pinned=True: the destination buffers are page-locked (allocated
        once per batch through torch, if importable), which lets the device->host copy run at PCIe speed instead of through
        the driver's staging of pageable memory.  NB the arrays of a pinned fetch ALIAS those per-batch buffers: the next
        pinned fetch of this batch overwrites them — pass copy=True (or copy what you keep) to get arrays of your own."""
        n = self.n
        bufs = self._host_buffers(want_pairs, pinned)
        score, flags, pair_off, pairs = bufs
        st = _lib.PoaStats()
        _lib.check(_lib.lib().poa_batch_fetch(self.handle, _p(score), _p(pairs), _p(pair_off), self.pair_capacity,
                                              _p(flags), C.byref(st)))
        if want_pairs:
            pairs = pairs[:int(pair_off[n])]
        if copy and pinned:
            score, pairs, pair_off, flags = score.copy(), pairs.copy(), pair_off.copy(), flags.copy()
        return BatchResult(score, pairs, pair_off, flags, st.as_dict())

    def _host_buffers(self, want_pairs, pinned):
        n = self.n
        if pinned:
            cached = getattr(self, "_pinned", None)
            if cached is None:
                try:
                    import torch
                    mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True).numpy()
                    cached = (mk((n,), torch.int32).view(np.uint32), mk((n,), torch.int32).view(np.uint32),
                              mk((n + 1,), torch.int64).view(np.uint64), mk((max(self.pair_capacity, 1), 2), torch.int32).view(np.uint32))
                except Exception:
                    cached = False
                self._pinned = cached
            if cached:
                return cached[0], cached[1], cached[2], (cached[3] if want_pairs else None)
        score, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        pair_off = np.zeros(n + 1, np.uint64)
        pairs = np.zeros((max(self.pair_capacity, 1), 2), np.uint32) if want_pairs else None
        return score, flags, pair_off, pairs

    def stats(self):
        """Synchronise and return HIP-event timings summed over the runs since the last call."""
        st = _lib.PoaStats()
        _lib.check(_lib.lib().poa_batch_stats(self.handle, C.byref(st)))
        return st.as_dict()

    def workspace_bytes(self):
        """Bytes of the plane workspace the batch holds."""
        v = C.c_uint64(0)
        _lib.check(_lib.lib().poa_batch_workspace_bytes(self.handle, C.byref(v)))
        return int(v.value)

    def search_counters(self):
        """AstarResult::{num_queued, num_visited, num_pruned} + wave-search steps, one row per query (exact / hybrid runs)."""
        out = np.zeros((self.n, 4), np.uint32)
        _lib.check(_lib.lib().poa_batch_fetch_search_counters(self.handle, _p(out)))
        return out

    def layout(self):
        """How the dense pass of the last run stored its planes: subset of {"u16", "compact", "relative", "derived_gaps"} (empty: u32 planes)."""
        v = C.c_uint32(0)
        _lib.check(_lib.lib().poa_batch_last_layout(self.handle, C.byref(v)))
        return {name for bit, name in ((1, "u16"), (2, "compact"), (4, "relative"), (8, "derived_gaps")) if v.value & bit}

    def band_info(self):
        """The banded forward pass of the last dense run: {"used", "banded", "fell_back", "min_d"} (poa_batch_band_info)."""
        out = (C.c_uint32 * 4)()
        _lib.check(_lib.lib().poa_batch_band_info(self.handle, out))
        return {"used": bool(out[0]), "banded": int(out[1]), "fell_back": int(out[2]), "min_d": int(out[3])}

    def band_pair_info(self):
        """The paired banded pass of the last dense run: {"paired", "single", "rule_count", "ran_paired"} (poa_batch_band_pair_info)."""
        out = (C.c_uint32 * 4)()
        _lib.check(_lib.lib().poa_batch_band_pair_info(self.handle, out))
        return {"paired": int(out[0]), "single": int(out[1]), "rule_count": int(out[2]), "ran_paired": bool(out[3])}

    def band_narrow_info(self):
        """The narrow tier of the paired banded pass in the last dense run: {"ran", "certified", "certified_512", "chosen_by"}
        (poa_batch_band_narrow_info): queries that ran the 384-column tier, those it certified, those the 512-column pass then
        certified (the rest went to the full pass), and None / "rule" / "override"."""
        out = (C.c_uint32 * 4)()
        _lib.check(_lib.lib().poa_batch_band_narrow_info(self.handle, out))
        return {"ran": int(out[0]), "certified": int(out[1]), "certified_512": int(out[2]), "chosen_by": (None, "rule", "override")[int(out[3])]}

    def tb_info(self):
        """The separate traceback launches of the last run's dense pass: {"kernel": None / "generic" / "lean", "lanes", "depth",
        "walks"} (poa_batch_tb_info)."""
        out = (C.c_uint32 * 4)()
        _lib.check(_lib.lib().poa_batch_tb_info(self.handle, out))
        return {"kernel": (None, "generic", "lean")[int(out[0])], "lanes": int(out[1]), "depth": int(out[2]), "walks": int(out[3])}

    def launches(self):
        """What the dense one-piece pass of the last run launched, one dict per chunk (poa_batch_last_launch): "kernel" in
        {"forward", "packed", "px", "pxmw", "band"}, "quads", "fuse", "mw", "waves", "code_fmt", "tb_lanes" (0: no separate
        traceback launch), "tb_depth", "queries"."""
        out = []
        while True:
            v = (C.c_uint32 * 8)()
            rc = _lib.lib().poa_batch_last_launch(self.handle, len(out), v)
            if rc == -1 and (out or self.n == 0):   # past the last chunk (a batch without queries launches nothing)
                return out
            _lib.check(rc)
            out.append({"kernel": LAUNCH_KERNELS[v[0]], "quads": int(v[1]), "fuse": bool(v[2] & 1), "mw": bool(v[2] & 2),
                        "waves": int(v[3]), "code_fmt": int(v[4]), "tb_lanes": int(v[5]), "tb_depth": int(v[6]), "queries": int(v[7])})

    def replay_info(self):
        """What the exact replay of the last run launched, one dict per chunk (poa_batch_replay_info): "kernel" in REPLAY_KERNELS,
        "win" (priorities in the descriptor ring), "lanes" per query, "waves" per block, "graph_lds", "rec_lds", "ring_global",
        "persistent", "resident" (blocks, 0: not computed), "blocks" launched, "lds_bytes"."""
        return _replay_records(_lib.lib().poa_batch_replay_info, self.handle, self.n)

    def device_results(self):
        ptrs = [C.c_void_p() for _ in range(4)]
        _lib.check(_lib.lib().poa_batch_device_results(self.handle, *[C.byref(p) for p in ptrs]))
        return dict(zip(("score", "flags", "pair_off", "pairs"), [p.value for p in ptrs]))

    def planes(self, query):
        rows = self.dg.graph.n
        cols = int(self.qoff[query + 1] - self.qoff[query]) + 1
        m, i, d = (np.zeros((rows, cols), np.uint32) for _ in range(3))
        _lib.check(_lib.lib().poa_batch_fetch_planes(self.handle, query, _p(m), _p(i), _p(d)))
        return m, i, d

    def compact_planes(self, query):
        """(m_raw, d, d_kept) of one query after a dense run in the compact derived-gaps layout (poa_batch_fetch_compact): the
        stored M words u16[rows, len + 1] (score in bits 0..13, bit 14: I == M, bit 15: D == M), the kept D rows u16[rows, len + 1]
        (0xFFFF where d_kept[row] is False) and d_kept bool[rows]; row = the engine's row (DeviceGraph.node_rows)."""
        rows = self.dg.graph.n
        cols = int(self.qoff[query + 1] - self.qoff[query]) + 1
        m_raw, d = np.zeros((rows, cols), np.uint16), np.zeros((rows, cols), np.uint16)
        kept = np.zeros(rows, np.uint8)
        _lib.check(_lib.lib().poa_batch_fetch_compact(self.handle, query, _p(m_raw), _p(d), _p(kept)))
        return m_raw, d, kept.astype(bool)

    def planes_2piece(self, query):
        """M, I1, D1, I2, D2 of one query after a dense two-piece run, rows = topological rank (its chunk must be the last one run)."""
        rows = self.dg.graph.n
        cols = int(self.qoff[query + 1] - self.qoff[query]) + 1
        out = [np.zeros((rows, cols), np.uint32) for _ in range(5)]
        _lib.check(_lib.lib().poa_batch_fetch_planes_2piece(self.handle, query, *[_p(a) for a in out]))
        return out

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().poa_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _MultiInput:
    """graphs + per-graph query lists (or graph_qoff + packed queries) as the arrays poa_multi_* take."""

    def __init__(self, graphs, seqs_per_graph=None, graph_qoff=None, qseq=None, qoff=None):
        self.dgs = [_device_graph(g) for g in graphs]
        if seqs_per_graph is not None:
            if len(seqs_per_graph) != len(self.dgs):
                raise ValueError("seqs_per_graph needs one list of queries per graph")
            graph_qoff = np.concatenate([[0], np.cumsum([len(s) for s in seqs_per_graph])])
            qseq, qoff = pack_queries([q for s in seqs_per_graph for q in s])
        self.graph_qoff = np.ascontiguousarray(graph_qoff, np.uint64)
        self.qseq = np.ascontiguousarray(qseq, np.uint8)
        self.qoff = np.ascontiguousarray(qoff, np.uint64)
        self.n = len(self.qoff) - 1
        if len(self.graph_qoff) != len(self.dgs) + 1:
            raise ValueError("graph_qoff needs n_graphs + 1 entries")
        # the C ABI takes the query count from graph_qoff[n_graphs]: check it here, where the count is known
        if int(self.graph_qoff[-1]) != self.n:
            raise ValueError("graph_qoff[n_graphs] = %d is not the query count %d" % (int(self.graph_qoff[-1]), self.n))
        self.handles = (C.c_void_p * max(len(self.dgs), 1))(*[dg.handle for dg in self.dgs])
        self.n_graphs = len(self.dgs)
        per_graph = np.diff(self.graph_qoff.astype(np.int64))
        self.pair_capacity = int(self.qoff[-1]) + int(sum(int(c) * dg.graph.n for c, dg in zip(per_graph, self.dgs) if c > 0))


MULTI_ONE_STRIP_MAX_LEN = 1023   # longest query of a dense or exact multi-graph batch without POA_CFG_WIDE_QUERIES


def _multi_wide_config(who, mi, config, dense, exact, wide):
    """(config, flag) for the footprint / create call of a multi-graph batch.  wide None: POA_CFG_WIDE_QUERIES is set iff the
    kind is dense or exact and a query is longer than 1023 symbols; True / False force it.  The caller's config is not modified:
    where the flag has to change, a copy carries it (mode "exact" / "dense" when there is no config, as the library reads NULL)."""
    if not (dense or exact):
        if wide:
            raise ValueError(who + ": wide=True is for the dense and exact kinds; a checkpointed batch takes queries of any length")
        return config, False
    if wide is None:
        wide = mi.n > 0 and int(np.diff(mi.qoff.astype(np.int64)).max()) > MULTI_ONE_STRIP_MAX_LEN
    has = config is not None and bool(config.flags & _lib.CFG_WIDE_QUERIES)
    if bool(wide) != has:
        src = config if config is not None else make_config("exact" if exact else "dense")
        config = type(src).from_buffer_copy(src)
        config.flags = (config.flags | _lib.CFG_WIDE_QUERIES) if wide else (config.flags & ~_lib.CFG_WIDE_QUERIES)
    return config, bool(wide)


def _multi_kind_check(who, two_piece, dense, exact, dense2, wide):
    """The kinds of a multi-graph batch exclude each other; dense2 is the dense batch of the two-piece model, a kind of its own."""
    if (dense or exact) and two_piece:
        raise ValueError(who + ": the dense and exact multi-graph batches are one-piece (the dense two-piece batch: dense2=True)")
    if dense and exact:
        raise ValueError(who + ": dense and exact are two kinds of batch")
    if dense2 and (dense or exact or two_piece):
        raise ValueError(who + ": dense2 is a kind of its own: not together with dense, exact or two_piece")
    if dense2 and wide:
        raise ValueError(who + ": wide=True is for the dense and exact kinds; the dense two-piece batch takes queries of any length")


def multi_footprint(graphs, seqs_per_graph=None, graph_qoff=None, qseq=None, qoff=None, config=None, two_piece=False, dense=False, exact=False,
                    wide=None, dense2=False):
    """(bytes, largest_query_bytes) of a multi-graph batch: the plane workspace of the whole batch as one chunk and of its
    largest query (poa_multi_footprint; host only).  config: make_config("checkpoint", ckpt_rows=k) to size another plan.
    two_piece: the batch of the two-piece model (poa_multi_footprint_2piece; config: None or mode "checkpoint2").
    dense: the dense batch (poa_multi_footprint_dense; config: None or mode "dense"): compact u16 planes per query.
    exact: the exact batch (poa_multi_footprint_exact; config: None or mode "exact" / "hybrid"): the dense region and the u32
    visited table per query, plus the replay workspace of every slot (queue_entries_per_cell from config).
    wide: POA_CFG_WIDE_QUERIES for the dense and exact kinds (None: set iff a query is longer than 1023 symbols; True / False
    force it; True with a checkpointed kind is a ValueError: that kind takes any length already).
    dense2: the dense two-piece batch (poa_multi_footprint_dense_2piece; config: None or mode "dense"): five u16 planes per
    query, any length; not together with dense, exact, two_piece or wide=True."""
    _multi_kind_check("multi_footprint", two_piece, dense, exact, dense2, wide)
    mi = _MultiInput(graphs, seqs_per_graph, graph_qoff, qseq, qoff)
    config, _ = _multi_wide_config("multi_footprint", mi, config, dense, exact, wide)
    total, largest = C.c_uint64(0), C.c_uint64(0)
    fn = _lib.lib().poa_multi_footprint_2piece if two_piece else (_lib.lib().poa_multi_footprint_dense if dense else _lib.lib().poa_multi_footprint)
    if exact:
        fn = _lib.lib().poa_multi_footprint_exact
    if dense2:
        fn = _lib.lib().poa_multi_footprint_dense_2piece
    _lib.check(fn(mi.handles, mi.n_graphs, _p(mi.graph_qoff), _p(mi.qoff), C.byref(config) if config is not None else None,
                  C.byref(total), C.byref(largest)))
    return int(total.value), int(largest.value)


class MultiGraphBatch:
    """The queries of many graphs resident in HBM (`poa_multi_*`): one checkpointed run covers all of them, one wavefront per
    query.  Queries are grouped by graph — seqs_per_graph[g] are graph g's, or graph_qoff + packed qseq / qoff; results come
    back in query order, rpos = node index in that query's own graph.  two_piece=True: the batch of the two-piece model
    (`poa_multi_create_2piece`; its footprint differs, so the model is chosen at creation), run with GapAffine2Piece costs.
    dense=True: the dense batch (`poa_multi_create_dense`): the packed forward pass over compact u16 planes and one walk launch
    per chunk instead of the two checkpointed passes; one-piece costs that allow u16 cells.  Queries of more than 1023 symbols
    need POA_CFG_WIDE_QUERIES at creation (`wide`: None sets it iff such a query is there, True / False force it; `self.wide`
    says what the batch was created with): a chunk with such a query runs the strip loop, every other chunk what it always ran.
    exact=True: the exact batch (`poa_multi_create_exact`): the dense batch with the replay of the reference's search behind it;
    run with make_config("exact" | "hybrid", heuristic, pruning, ...): per query what align_batch returns in that mode for the
    query's graph alone, and search_counters() the replay's counters.
    dense2=True: the dense two-piece batch (`poa_multi_create_dense_2piece`): five u16 planes per query, one forward and one
    walk launch per chunk instead of the two checkpointed passes; run with GapAffine2Piece costs that allow u16 cells (config:
    None or make_config("dense", ...)), queries of any length; planes_2piece(query) reads a query's planes back."""

    def __init__(self, graphs, seqs_per_graph=None, graph_qoff=None, qseq=None, qoff=None, device=0, workspace_bytes=0, config=None,
                 two_piece=False, dense=False, exact=False, wide=None, dense2=False):
        _multi_kind_check("MultiGraphBatch", two_piece, dense, exact, dense2, wide)
        mi = _MultiInput(graphs, seqs_per_graph, graph_qoff, qseq, qoff)
        self.input, self.n, self.pair_capacity = mi, mi.n, mi.pair_capacity
        self.graph_qoff, self.qseq, self.qoff = mi.graph_qoff, mi.qseq, mi.qoff
        self.two_piece = bool(two_piece)
        self.dense = bool(dense)
        self.exact = bool(exact)
        self.dense2 = bool(dense2)
        config, self.wide = _multi_wide_config("MultiGraphBatch", mi, config, self.dense, self.exact, wide)
        h = C.c_void_p()
        create = _lib.lib().poa_multi_create_2piece if self.two_piece else (_lib.lib().poa_multi_create_dense if self.dense else _lib.lib().poa_multi_create)
        if self.exact:
            create = _lib.lib().poa_multi_create_exact
        if self.dense2:
            create = _lib.lib().poa_multi_create_dense_2piece
        _lib.check(create(mi.handles, mi.n_graphs, _p(mi.graph_qoff), device, _p(mi.qseq), _p(mi.qoff),
                          C.byref(config) if config is not None else None, int(workspace_bytes), C.byref(h)))
        self.handle = h

    def run(self, costs, stream=None, config=None):
        """Launch on `stream` without synchronising (config: None or make_config("checkpoint", ...); for a two_piece batch
        make_config("checkpoint2", ...)).  GapAffine2Piece costs run through poa_multi_run_2piece, all others through
        poa_multi_run: costs of the other model than the batch's are refused by the library (POA_ERR_INVALID_ARG).  A dense
        batch runs one-piece costs through poa_multi_run_dense (config: None or make_config("dense", ...)), an exact batch
        through poa_multi_run_exact (config: None = make_config("exact"), or make_config("hybrid", ...)).  A dense2 batch runs
        GapAffine2Piece costs through poa_multi_run_dense_2piece (config: None or make_config("dense", ...))."""
        c = costs._c()
        if config is None:
            config = make_config("exact" if self.exact else ("dense" if (self.dense or self.dense2) else ("checkpoint2" if self.two_piece else "checkpoint")))   # (carries the POA_<NAME> overrides, if any are set)
        if self.dense2:
            if not isinstance(costs, GapAffine2Piece):
                raise ValueError("MultiGraphBatch.run: a dense2 batch runs GapAffine2Piece costs")
            run = _lib.lib().poa_multi_run_dense_2piece
        elif isinstance(costs, GapAffine2Piece):
            run = _lib.lib().poa_multi_run_2piece
        elif self.exact:
            run = _lib.lib().poa_multi_run_exact
        else:
            run = _lib.lib().poa_multi_run_dense if self.dense else _lib.lib().poa_multi_run
        _lib.check(run(self.handle, C.byref(c), C.byref(config), C.c_void_p(stream or 0)))

    def launches(self):
        """What the last run of a dense batch launched, one dict per chunk (poa_multi_last_launch), in the form of
        ResidentBatch.launches: "kernel" is "packed", "quads" 1 or 2, "tb_lanes" 64, "tb_depth" 32, "queries" the chunk's.
        A chunk that ran the strip loop (POA_LAUNCH_STRIPS: a query of more than 1023 symbols) has "strips": True, no other
        chunk has the key."""
        out = []
        while True:
            v = (C.c_uint32 * 8)()
            rc = _lib.lib().poa_multi_last_launch(self.handle, len(out), v)
            if rc == -1 and (out or (self.n == 0 and (self.dense or self.exact))):   # past the last chunk (a batch without queries launches nothing)
                return out
            _lib.check(rc)
            out.append({"kernel": LAUNCH_KERNELS[v[0]], "quads": int(v[1]), "fuse": bool(v[2] & 1), "mw": bool(v[2] & 2),
                        "waves": int(v[3]), "code_fmt": int(v[4]), "tb_lanes": int(v[5]), "tb_depth": int(v[6]), "queries": int(v[7])})
            if self.exact:   # the low launch bits of an exact batch name the replay kernel instead
                out[-1].update(fuse=False, mw=False, replay={1: "lds", 2: "generic"}[int(v[2]) & 3])
            if v[2] & _lib.LAUNCH_STRIPS:
                out[-1]["strips"] = True

    def planes_2piece(self, query):
        """M, I1, D1, I2, D2 of one query after a run of a dense2 batch (poa_multi_fetch_planes_2piece), rows = topological rank
        in the query's own graph (its chunk must be the last one run)."""
        g = int(np.searchsorted(self.graph_qoff, query, side="right")) - 1
        rows = self.input.dgs[g].graph.n
        cols = int(self.qoff[query + 1] - self.qoff[query]) + 1
        out = [np.zeros((rows, cols), np.uint32) for _ in range(5)]
        _lib.check(_lib.lib().poa_multi_fetch_planes_2piece(self.handle, query, *[_p(a) for a in out]))
        return out

    def replay_info(self):
        """What the replay of the last run of an exact batch launched, one dict per chunk (poa_multi_replay_info), in the form
        of ResidentBatch.replay_info."""
        return _replay_records(_lib.lib().poa_multi_replay_info, self.handle, self.n)

    def search_counters(self):
        """[n, 4] num_queued, num_visited, num_pruned, steps of the last run of an exact batch (poa_multi_fetch_search_counters);
        zeros for a query that was not replayed."""
        out = np.zeros((self.n, 4), np.uint32)
        _lib.check(_lib.lib().poa_multi_fetch_search_counters(self.handle, _p(out)))
        return out

    def fetch(self, want_pairs=True):
        n = self.n
        score, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        pair_off = np.zeros(n + 1, np.uint64)
        pairs = np.zeros((max(self.pair_capacity, 1), 2), np.uint32) if want_pairs else None
        st = _lib.PoaStats()
        _lib.check(_lib.lib().poa_multi_fetch(self.handle, _p(score), _p(pairs), _p(pair_off), self.pair_capacity, _p(flags), C.byref(st)))
        if want_pairs:
            pairs = pairs[:int(pair_off[n])]
        return BatchResult(score, pairs, pair_off, flags, st.as_dict())

    def stats(self):
        st = _lib.PoaStats()
        _lib.check(_lib.lib().poa_multi_stats(self.handle, C.byref(st)))
        return st.as_dict()

    def workspace_bytes(self):
        v = C.c_uint64(0)
        _lib.check(_lib.lib().poa_multi_workspace_bytes(self.handle, C.byref(v)))
        return int(v.value)

    def device_results(self):
        ptrs = [C.c_void_p() for _ in range(4)]
        _lib.check(_lib.lib().poa_multi_device_results(self.handle, *[C.byref(p) for p in ptrs]))
        return dict(zip(("score", "flags", "pair_off", "pairs"), [p.value for p in ptrs]))

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().poa_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ScoreSetInput:
    """graphs + a pool of queries + (query, graph) pairs as the arrays poa_scoreset_* take.  pairs None: the full matrix."""

    def __init__(self, graphs, seqs=None, qseq=None, qoff=None, pairs=None):
        self.dgs = [_device_graph(g) for g in graphs]
        if seqs is not None:
            qseq, qoff = pack_queries(seqs)
        self.qseq = np.ascontiguousarray(qseq, np.uint8)
        self.qoff = np.ascontiguousarray(qoff, np.uint64)
        self.n_queries = len(self.qoff) - 1
        self.n_graphs = len(self.dgs)
        self.handles = (C.c_void_p * max(self.n_graphs, 1))(*[dg.handle for dg in self.dgs])
        if pairs is None:
            self.pair_query = self.pair_graph = None
            self.n = self.n_queries * self.n_graphs
        else:
            pr = np.asarray(pairs, np.int64).reshape(-1, 2)
            # the C ABI checks these too; here the caller gets the offending pair named in Python terms
            bad = np.flatnonzero((pr[:, 0] < 0) | (pr[:, 0] >= self.n_queries) | (pr[:, 1] < 0) | (pr[:, 1] >= self.n_graphs))
            if len(bad):
                raise ValueError("pair %d = (query %d, graph %d) is out of range (%d queries, %d graphs)"
                                 % (int(bad[0]), int(pr[bad[0], 0]), int(pr[bad[0], 1]), self.n_queries, self.n_graphs))
            self.pair_query = np.ascontiguousarray(pr[:, 0], np.uint32)
            self.pair_graph = np.ascontiguousarray(pr[:, 1], np.uint32)
            self.n = len(pr)

    def pair_args(self):
        return self.n, _p(self.pair_query), _p(self.pair_graph)


def scoreset_footprint(graphs, seqs=None, qseq=None, qoff=None, pairs=None, config=None):
    """(bytes, largest_pair_bytes) of a score set: the slot workspace of the whole set as one chunk and of its largest pair
    (poa_scoreset_footprint; host only)."""
    si = _ScoreSetInput(graphs, seqs, qseq, qoff, pairs)
    total, largest = C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.lib().poa_scoreset_footprint(si.handles, si.n_graphs, si.n_queries, _p(si.qoff), *si.pair_args(),
                                                 C.byref(config) if config is not None else None, C.byref(total), C.byref(largest)))
    return int(total.value), int(largest.value)


class ScoreSet:
    """(query, graph) pairs resident in HBM (`poa_scoreset_*`): one score-only run covers all of them, one wavefront per pair.
    graphs: the graph list; seqs (or packed qseq / qoff): the pool of queries, uploaded once; pairs: an [n, 2] array of
    (query index, graph index) in any order, with repeats — None: the full queries x graphs matrix, pair p = (p // n_graphs,
    p % n_graphs).  Results come back in pair order."""

    def __init__(self, graphs, seqs=None, qseq=None, qoff=None, pairs=None, workspace_bytes=0, config=None, device=0):
        si = _ScoreSetInput(graphs, seqs, qseq, qoff, pairs)
        self.input, self.n, self.n_queries, self.n_graphs = si, si.n, si.n_queries, si.n_graphs
        h = C.c_void_p()
        _lib.check(_lib.lib().poa_scoreset_create(si.handles, si.n_graphs, device, si.n_queries, _p(si.qseq), _p(si.qoff), *si.pair_args(),
                                                  C.byref(config) if config is not None else None, int(workspace_bytes), C.byref(h)))
        self.handle = h

    def run(self, costs, stream=None, config=None, cap=None, best=False, slack=0, limit=None):
        """Launch on `stream` without synchronising.  costs: GapAffine (poa_scoreset_run) or GapAffine2Piece
        (poa_scoreset_run_2piece); config: None or make_config("score", ...).
        cap: None, or a score cap — a scalar, or one value per pair in pair order; POA_NONE: no cap for that pair — for
        poa_scoreset_run_capped / _run_2piece_capped: a pair whose score is above its cap comes back as POA_NONE with
        FLAG_CAPPED set, and its wave stops as soon as a row proves it.
        best=True: a best-of run (poa_scoreset_run_best / _run_2piece_best) — every pair is capped by the best score its query
        has reached so far plus `slack`, under `limit` (None, a scalar or one ceiling per query; POA_NONE: none); fetch_best
        returns the winning pair of every query.  cap and best exclude each other."""
        c = costs._c()
        if config is None:
            config = make_config("score")   # (carries the POA_<NAME> overrides, if any are set)
        two_piece = isinstance(costs, GapAffine2Piece)
        if best:
            if cap is not None:
                raise ValueError("run: cap and best=True exclude each other")
            if not 0 <= int(slack) <= _lib.POA_NONE:
                raise ValueError("slack: a u32")
            lim = None
            if limit is not None:
                lim = np.full(self.n_queries, limit, np.uint32) if np.ndim(limit) == 0 else np.ascontiguousarray(limit, np.uint32)
                if lim.shape != (self.n_queries,):
                    raise ValueError("limit: a scalar or one value per query (%d), got shape %s" % (self.n_queries, lim.shape))
                if self.n_queries == 0:
                    lim = None
            fn = _lib.lib().poa_scoreset_run_2piece_best if two_piece else _lib.lib().poa_scoreset_run_best
            _lib.check(fn(self.handle, C.byref(c), C.byref(config), int(slack), _p(lim), C.c_void_p(stream or 0)))
            return
        if cap is None:
            fn = _lib.lib().poa_scoreset_run_2piece if two_piece else _lib.lib().poa_scoreset_run
            _lib.check(fn(self.handle, C.byref(c), C.byref(config), C.c_void_p(stream or 0)))
            return
        caps = np.full(self.n, cap, np.uint32) if np.ndim(cap) == 0 else np.ascontiguousarray(cap, np.uint32)
        if caps.shape != (self.n,):
            raise ValueError("cap: a scalar or one value per pair (%d), got shape %s" % (self.n, caps.shape))
        if self.n == 0:
            caps = np.zeros(1, np.uint32)   # (a non-null pointer)
        fn = _lib.lib().poa_scoreset_run_2piece_capped if two_piece else _lib.lib().poa_scoreset_run_capped
        _lib.check(fn(self.handle, C.byref(c), C.byref(config), _p(caps), C.c_void_p(stream or 0)))

    def swept_rows(self):
        """Synchronise; the row bodies each pair's wave executed in the last run (poa_scoreset_fetch_swept), in pair order."""
        swept = np.zeros(max(self.n, 1), np.uint32)
        _lib.check(_lib.lib().poa_scoreset_fetch_swept(self.handle, _p(swept)))
        return swept[:self.n]

    def fetch_best(self):
        """Synchronise; the result of the last run, a best-of run (poa_scoreset_fetch_best): a dict of u32 arrays per query —
        pair (POA_NONE: no pair qualifies), score, flags, second_score, n_within."""
        rec = np.zeros((max(self.n_queries, 1), C.sizeof(_lib.PoaBest) // 4), np.uint32)
        _lib.check(_lib.lib().poa_scoreset_fetch_best(self.handle, _p(rec)))
        rec = rec[:self.n_queries]
        return {k: np.ascontiguousarray(rec[:, i]) for i, k in enumerate(("pair", "score", "flags", "second_score", "n_within"))}

    def fetch(self):
        """Synchronise; (score, flags, stats): u32 arrays in pair order and the poa_stats_t of the runs since the last call."""
        score, flags = np.zeros(self.n, np.uint32), np.zeros(self.n, np.uint32)
        st = _lib.PoaStats()
        _lib.check(_lib.lib().poa_scoreset_fetch(self.handle, _p(score), _p(flags), C.byref(st)))
        return score, flags, st.as_dict()

    def stats(self):
        st = _lib.PoaStats()
        _lib.check(_lib.lib().poa_scoreset_stats(self.handle, C.byref(st)))
        return st.as_dict()

    def workspace_bytes(self):
        v = C.c_uint64(0)
        _lib.check(_lib.lib().poa_scoreset_workspace_bytes(self.handle, C.byref(v)))
        return int(v.value)

    def device_results(self):
        ptrs = [C.c_void_p() for _ in range(2)]
        _lib.check(_lib.lib().poa_scoreset_device_results(self.handle, *[C.byref(p) for p in ptrs]))
        return dict(zip(("score", "flags"), [p.value for p in ptrs]))

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().poa_scoreset_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PoastaAligner:
    """`PoastaAligner::new(config, aln_type)` (mod.rs:53)."""

    def __init__(self, config, aln_type=AlignmentType.Global, device=0, mode="dense", queue_entries_per_cell=0.0):
        if aln_type != AlignmentType.Global and not isinstance(aln_type, EndsFree):
            raise ValueError("aln_type must be AlignmentType.Global or AlignmentType.EndsFree(...)")
        self.config, self.aln_type, self.device = config, aln_type, device
        self.mode, self.queue_entries_per_cell = mode, queue_entries_per_cell

    # -- the three reference entry points; all run the same dense pass ------------------------
    def align(self, ref_graph, seq, pruning=True):
        """mod.rs:114-145."""
        return self.align_batch(ref_graph, [seq], pruning=pruning).result(0)

    def align_with_existing_bubbles(self, ref_graph, seq, existing_bubbles=None):
        """mod.rs:69-79.  The bubble index only steers the reference's pruning; unused here."""
        return self.align(ref_graph, seq)

    def align_no_pruning(self, ref_graph, seq):
        """mod.rs:81-90 (matters only for the exact replay: no pruning changes which cells the reference visits)."""
        return self.align(ref_graph, seq, pruning=False)

    def planes_2piece(self, ref_graph, seq):
        """M, I1, D1, I2, D2 of one query under the two-piece model, rows = topological rank (parity tests)."""
        dg = _device_graph(ref_graph)
        s = np.ascontiguousarray(np.frombuffer(seq, np.uint8) if isinstance(seq, (bytes, bytearray)) else seq, np.uint8)
        shape = (dg.graph.n, len(s) + 1)
        out = [np.zeros(shape, np.uint32) for _ in range(5)]
        c = self.config.costs._c()
        _lib.check(_lib.lib().poa_planes_2piece(dg.handle, C.byref(c), _p(s), len(s), *[_p(a) for a in out], self.device))
        return out

    def score_batch(self, ref_graph, seqs=None, qseq=None, qoff=None):
        """Scores only (mode "score"): (score, flags) as numpy arrays — dense mode's scores, flags limited to what follows
        from the input alone (EMPTY_GRAPH, SHORT_QUERY).  No score planes are stored, no traceback runs."""
        dg = _device_graph(ref_graph)
        if seqs is not None:
            qseq, qoff = pack_queries(seqs)
        qseq = np.ascontiguousarray(qseq, np.uint8)
        qoff = np.ascontiguousarray(qoff, np.uint64)
        n = len(qoff) - 1
        score, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        pair_off = np.zeros(n + 1, np.uint64)
        st = _lib.PoaStats()
        c = self.config.costs._c()
        cfg = make_config("score", self.config.heuristic)
        if getattr(self.config, "two_piece", False):
            _lib.check(_lib.lib().poa_align_batch_2piece_ex(dg.handle, C.byref(c), C.byref(cfg), n, _p(qseq), _p(qoff), _p(score),
                                                            None, _p(pair_off), 0, _p(flags), C.byref(st), None, self.device))
        else:
            _lib.check(_lib.lib().poa_align_batch_ex(dg.handle, C.byref(c), C.byref(cfg), n, _p(qseq), _p(qoff), _p(score),
                                                     None, _p(pair_off), 0, _p(flags), C.byref(st), self.device))
        self.last_stats = st.as_dict()
        return score, flags

    # -- batch shape (lasagna.rs:246-268) ------------------------------------------------------
    def align_batch(self, ref_graph, seqs=None, qseq=None, qoff=None, want_pairs=True, pruning=True):
        dg = _device_graph(ref_graph)
        if seqs is not None:
            qseq, qoff = pack_queries(seqs)
        qseq = np.ascontiguousarray(qseq, np.uint8)
        qoff = np.ascontiguousarray(qoff, np.uint64)
        n = len(qoff) - 1
        score, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        pair_off = np.zeros(n + 1, np.uint64)
        cap = int(qoff[-1]) + n * dg.graph.n
        pairs = np.zeros((max(cap, 1), 2), np.uint32) if want_pairs else None
        st = _lib.PoaStats()
        c = self.config.costs._c()
        if getattr(self.config, "two_piece", False):
            if self.mode == "dense":
                if self.aln_type != AlignmentType.Global:
                    raise ValueError("two-piece model: ends-free alignment runs as the exact replay (mode='exact')")
                _lib.check(_lib.lib().poa_align_batch_2piece(dg.handle, C.byref(c), n, _p(qseq), _p(qoff), _p(score), _p(pairs),
                                                             _p(pair_off), cap, _p(flags), C.byref(st), self.device))
                counters = None
            else:
                # the reference's own search, five states (gap_affine_2piece.rs): scores and alignments are what it returns
                cfg = make_config(self.mode, self.config.heuristic, pruning, self.queue_entries_per_cell, aln_type=self.aln_type)
                counters = np.zeros((n, 4), np.uint32)
                _lib.check(_lib.lib().poa_align_batch_2piece_ex(dg.handle, C.byref(c), C.byref(cfg), n, _p(qseq), _p(qoff), _p(score),
                                                                _p(pairs), _p(pair_off), cap, _p(flags), C.byref(st), _p(counters),
                                                                self.device))
            if want_pairs:
                pairs = pairs[:int(pair_off[n])]
            res = BatchResult(score, pairs, pair_off, flags, st.as_dict())
            res.search_counters = counters   # num_queued, num_visited, num_pruned, live queue entries (exact mode)
            return res
        cfg = make_config(self.mode, self.config.heuristic, pruning, self.queue_entries_per_cell, aln_type=self.aln_type)
        _lib.check(_lib.lib().poa_align_batch_ex(dg.handle, C.byref(c), C.byref(cfg), n, _p(qseq), _p(qoff), _p(score),
                                                 _p(pairs), _p(pair_off), cap, _p(flags), C.byref(st), self.device))
        if want_pairs:
            pairs = pairs[:int(pair_off[n])]
        return BatchResult(score, pairs, pair_off, flags, st.as_dict())

    def align_multi(self, graphs, seqs_per_graph, want_pairs=True, mode="checkpoint", pruning=True):
        """Many graphs, a few reads each, in one checkpointed run (poa_align_multi): seqs_per_graph[g] are the queries of
        graphs[g].  Returns a BatchResult over all queries in that order: dense mode's score, alignment and flags of every
        query against its own graph.  Global.  A two-piece config (Affine2PieceDijkstra / Affine2PieceMinGapCost) runs
        poa_align_multi_2piece: the dense two-piece pass's results.
        mode="dense": the same results from the dense batch (poa_align_multi_dense): the packed forward pass over compact
        planes — more workspace, one-piece costs only (a two-piece config: ValueError).  Reads of more than 1023 symbols set
        POA_CFG_WIDE_QUERIES by themselves: their chunks run the forward pass strip by strip.
        mode="exact" | "hybrid": the replay of the reference's search behind the dense batch (poa_align_multi_exact): per query
        what align_batch returns on a PoastaAligner of that mode for the query's graph alone; heuristic and pruning come from
        the aligner's config as there, queue_entries_per_cell from the aligner.  One-piece, Global; long reads as under "dense".
        mode="dense2": the two-piece results from the dense two-piece batch (poa_align_multi_dense_2piece): five u16 planes per
        query, reads of any length — more workspace, a two-piece config only (a one-piece config: ValueError), costs that allow
        u16 cells."""
        if self.aln_type != AlignmentType.Global:
            raise ValueError("align_multi: AlignmentType.Global only")
        if mode not in ("checkpoint", "dense", "exact", "hybrid", "dense2"):
            raise ValueError("align_multi: mode is \"checkpoint\", \"dense\", \"exact\", \"hybrid\" or \"dense2\"")
        two_piece = getattr(self.config, "two_piece", False)
        if mode == "dense2" and not two_piece:
            raise ValueError("align_multi: mode=\"dense2\" is the dense batch of the two-piece model; a one-piece config runs mode=\"dense\"")
        if mode not in ("checkpoint", "dense2") and two_piece:
            raise ValueError("align_multi: mode=\"%s\" is one-piece; a two-piece config runs the checkpointed batch or mode=\"dense2\"" % mode)
        if mode in ("exact", "hybrid"):
            mi = _MultiInput(graphs, seqs_per_graph)
            n = mi.n
            score, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            pair_off = np.zeros(n + 1, np.uint64)
            pairs = np.zeros((max(mi.pair_capacity, 1), 2), np.uint32) if want_pairs else None
            st = _lib.PoaStats()
            c = self.config.costs._c()
            cfg = make_config(mode, self.config.heuristic, pruning, self.queue_entries_per_cell)
            cfg, _ = _multi_wide_config("align_multi", mi, cfg, False, True, None)
            _lib.check(_lib.lib().poa_align_multi_exact(mi.handles, mi.n_graphs, _p(mi.graph_qoff), C.byref(c), C.byref(cfg), _p(mi.qseq),
                                                        _p(mi.qoff), _p(score), _p(pairs), _p(pair_off), mi.pair_capacity, _p(flags),
                                                        C.byref(st), self.device))
            if want_pairs:
                pairs = pairs[:int(pair_off[n])]
            return BatchResult(score, pairs, pair_off, flags, st.as_dict())
        mi = _MultiInput(graphs, seqs_per_graph)
        n = mi.n
        score, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        pair_off = np.zeros(n + 1, np.uint64)
        pairs = np.zeros((max(mi.pair_capacity, 1), 2), np.uint32) if want_pairs else None
        st = _lib.PoaStats()
        c = self.config.costs._c()
        cfg = make_config("dense" if mode in ("dense", "dense2") else ("checkpoint2" if two_piece else "checkpoint"), self.config.heuristic)
        cfg, _ = _multi_wide_config("align_multi", mi, cfg, mode == "dense", False, None)
        fn = _lib.lib().poa_align_multi_2piece if two_piece else (_lib.lib().poa_align_multi_dense if mode == "dense" else _lib.lib().poa_align_multi)
        if mode == "dense2":
            fn = _lib.lib().poa_align_multi_dense_2piece
        _lib.check(fn(mi.handles, mi.n_graphs, _p(mi.graph_qoff), C.byref(c), C.byref(cfg), _p(mi.qseq), _p(mi.qoff), _p(score),
                      _p(pairs), _p(pair_off), mi.pair_capacity, _p(flags), C.byref(st), self.device))
        if want_pairs:
            pairs = pairs[:int(pair_off[n])]
        return BatchResult(score, pairs, pair_off, flags, st.as_dict())

    def score_pairs(self, graphs, seqs, pairs, max_score=None):
        """Scores of (query, graph) pairs over many graphs in one score-only run (poa_score_pairs): pairs is an [n, 2] array of
        (index into seqs, index into graphs), None for the full matrix.  Returns (score, flags) in pair order: what score_batch
        gives for that query against that graph alone.
        max_score: None, or a cap — a scalar or one value per pair: a pair that scores above it comes back as POA_NONE with
        FLAG_CAPPED set, without its sweep being finished (a ScoreSet run with cap=max_score)."""
        if self.aln_type != AlignmentType.Global:
            raise ValueError("score_pairs: AlignmentType.Global only")
        if max_score is not None:
            ss = ScoreSet(graphs, seqs, pairs=pairs, device=self.device)
            try:
                ss.run(self.config.costs, config=make_config("score", self.config.heuristic), cap=max_score)
                score, flags, st = ss.fetch()
            finally:
                ss.close()
            self.last_stats = st
            return score, flags
        si = _ScoreSetInput(graphs, seqs, pairs=pairs)
        score, flags = np.zeros(si.n, np.uint32), np.zeros(si.n, np.uint32)
        st = _lib.PoaStats()
        c = self.config.costs._c()
        cfg = make_config("score", self.config.heuristic)
        fn = _lib.lib().poa_score_pairs_2piece if getattr(self.config, "two_piece", False) else _lib.lib().poa_score_pairs
        _lib.check(fn(si.handles, si.n_graphs, C.byref(c), C.byref(cfg), si.n_queries, _p(si.qseq), _p(si.qoff), *si.pair_args(),
                      _p(score), _p(flags), C.byref(st), self.device))
        self.last_stats = st.as_dict()
        return score, flags

    def assign(self, graphs, seqs, pairs=None, slack=0, max_score=None):
        """Which graph does each query belong to: one best-of score-set run (ScoreSet.run(best=True)) over `pairs` ([n, 2]
        (query, graph) indices; None: every query against every graph).  A query's candidates are tried in the order they are
        listed, and the best score so far caps the rest: list the likeliest graph first.  max_score: None, a scalar or one
        ceiling per query.  Returns a dict of arrays per query: graph (int64, -1: no candidate within max_score), pair, score,
        flags, second_score (the runner-up if within `slack` of the winner, else POA_NONE), n_within."""
        if self.aln_type != AlignmentType.Global:
            raise ValueError("assign: AlignmentType.Global only")
        ss = ScoreSet(graphs, seqs, pairs=pairs, device=self.device)
        try:
            ss.run(self.config.costs, config=make_config("score", self.config.heuristic), best=True, slack=slack, limit=max_score)
            out = ss.fetch_best()
            self.last_stats = ss.stats()
        finally:
            ss.close()
        si = ss.input
        won = out["pair"] != _lib.POA_NONE
        pair = np.where(won, out["pair"], 0).astype(np.int64)
        if si.pair_graph is None:
            graph_of = pair % max(si.n_graphs, 1)
        else:
            graph_of = si.pair_graph[pair].astype(np.int64) if si.n else pair   # (no pairs: nobody won)
        out["graph"] = np.where(won, graph_of, -1).astype(np.int64)
        return out

    def assign_and_align(self, graphs, seqs, pairs=None, max_score=None, want_pairs=True, mode="checkpoint"):
        """assign, then the alignments of the assigned queries against their winning graphs in one align_multi run (the
        two-piece form for a two-piece config; mode: align_multi's).  Returns (assignment, BatchResult), the BatchResult in
        the order of seqs; a query without a graph has no pairs, score POA_NONE and flags 0."""
        if mode == "dense" and getattr(self.config, "two_piece", False):   # (before the assignment runs for nothing)
            raise ValueError("assign_and_align: mode=\"dense\" is one-piece; a two-piece config runs the checkpointed batch or mode=\"dense2\"")
        if mode == "dense2" and not getattr(self.config, "two_piece", False):
            raise ValueError("assign_and_align: mode=\"dense2\" is the dense batch of the two-piece model; a one-piece config runs mode=\"dense\"")
        a = self.assign(graphs, seqs, pairs=pairs, max_score=max_score)
        n = len(seqs)
        order = [np.flatnonzero(a["graph"] == g) for g in range(len(graphs))]
        res = self.align_multi(graphs, [[seqs[int(i)] for i in idx] for idx in order], want_pairs=want_pairs, mode=mode)
        score, flags = np.full(n, _lib.POA_NONE, np.uint32), np.zeros(n, np.uint32)
        counts = np.zeros(n, np.uint64)
        where = np.concatenate(order).astype(np.int64) if order else np.zeros(0, np.int64)   # where[k]: the query of res' k-th
        score[where], flags[where] = res.score, res.flags
        counts[where] = np.diff(res.pair_off.astype(np.int64)).astype(np.uint64)
        pair_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        out_pairs = None
        if want_pairs:
            out_pairs = np.zeros((int(pair_off[n]), 2), np.uint32)
            for k, qi in enumerate(where):
                out_pairs[int(pair_off[qi]):int(pair_off[qi + 1])] = res.pairs[int(res.pair_off[k]):int(res.pair_off[k + 1])]
        return a, BatchResult(score, out_pairs, pair_off, flags, res.stats)

    def score_matrix(self, graphs, seqs, max_score=None):
        """The full queries x graphs matrix of scores, a [n_queries, n_graphs] u32 array (score_pairs with pairs=None).
        max_score: None, or a cap — a scalar or one value per query; entries above it are POA_NONE."""
        if max_score is not None and np.ndim(max_score) != 0:
            max_score = np.asarray(max_score, np.uint32)
            if max_score.shape != (len(seqs),):
                raise ValueError("max_score: a scalar or one value per query (%d)" % len(seqs))
            max_score = np.repeat(max_score, len(graphs))
        score, _ = self.score_pairs(graphs, seqs, None, max_score=max_score)
        return score.reshape(len(seqs), len(graphs))
