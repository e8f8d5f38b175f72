#!/usr/bin/env python3
"""Many small graphs: one multi-graph batch against the per-graph loops, one process, one GPU, interleaved repetitions.

Workload: 256 graphs of about 200 rows (LinearishPOA at a backbone of 190), 32 reads of about 200 bp each, fixed seeds,
costs 4 / 6 / 2.  Per step, with the pairs fetched:
  (a)  poa_multi_run + poa_multi_fetch on a resident multi-graph batch; (a1) the one-shot poa_align_multi, which also creates
       and destroys the batch, as the loops below do per graph;
  (b)  the loop over the graphs of poa_align_batch_ex in POA_MODE_CHECKPOINT;
  (c)  the same loop in dense mode.
(b) and (c) are the paths a host had before.  The first --warmup steps are dropped; medians with min / max of the rest.  Kernel-only
times are the HIP-event sums of poa_stats_t (ms_forward, ms_traceback), summed over the calls of a step.  Writes
profiles/pr_multi_graph/timing.json.

--two-piece: the same shape and the same four paths under the two-piece model, costs 4 / 6,24 / 2,1: (a) poa_multi_run_2piece +
poa_multi_fetch on a batch of poa_multi_create_2piece, (a1) poa_align_multi_2piece, (b) the loop of poa_align_batch_2piece_ex in
POA_MODE_CHECKPOINT2, (c) the loop of the dense poa_align_batch_2piece.  Writes profiles/pr_multi_graph_2piece/timing.json.

--dense: the one-piece paths above and, in the same process on the same workload, the dense multi-graph batch: (d) poa_multi_run_dense
+ poa_multi_fetch on a resident batch of poa_multi_create_dense, (d1) the one-shot poa_align_multi_dense.  Writes
profiles/pr_multi_dense/timing.json, with both footprints.

--exact: the exact multi-graph batch in POA_MODE_HYBRID on the same graphs, in two shapes in one process: one read per graph (the
shape of a round of lock-step POA builds) and --reads reads per graph.  Per shape (e) poa_multi_run_exact + poa_multi_fetch on a
resident batch of poa_multi_create_exact, (e1) the one-shot poa_align_multi_exact, (f) the loop over the graphs of the one-shot
poa_align_batch_ex in POA_MODE_HYBRID; how many reads were replayed; the results of the three compared.  Writes
profiles/pr_multi_exact/timing.json.

--wide: dense and exact multi-graph batches with reads longer than one strip of the packed forward pass (POA_CFG_WIDE_QUERIES), on a
workload of its own: 64 graphs of about 1300 rows (LinearishPOA: a backbone of 1200 with 100 SNP bubbles), 8 reads of 1100 - 1300 bp
each (--graphs / --reads override the counts).  Per step, pairs fetched, in one process: (w) poa_multi_run_dense + poa_multi_fetch on
the wide dense batch; (a) poa_multi_run + poa_multi_fetch on the checkpointed batch of the same inputs; (c) the loop over the graphs
of the one-shot poa_align_batch_ex in POA_MODE_DENSE; (s) the wide dense batch built from the same reads cut to 1023 symbols, whose
chunks are one strip: against (w) per cell it shows what the strip loop itself costs.  With --exact also (e) poa_multi_run_exact +
poa_multi_fetch in POA_MODE_HYBRID on the wide exact batch of --exact-reads reads per graph against (f) the per-graph hybrid loop on
the same reads.  --dense is implied.  Writes profiles/pr_multi_wide/timing.json.

--dense2: the two resident two-piece batches on the --two-piece workload, costs 4 / 6,24 / 2,1, in one process, pairs fetched:
(a) poa_multi_run_2piece + poa_multi_fetch on the checkpointed batch of poa_multi_create_2piece; (d2) poa_multi_run_dense_2piece +
poa_multi_fetch on the batch of poa_multi_create_dense_2piece.  Each step split into its two launches (pass 1 and pass 2; forward
and walk) by the HIP-event sums of poa_stats_t, with both batches' plane bytes and workspaces and the results compared.  Writes
profiles/pr_multi_dense2/timing.json.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--reads", type=int, default=32)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--two-piece", action="store_true", help="the two-piece model, costs 4 / 6,24 / 2,1 (poa_multi_*_2piece)")
    ap.add_argument("--dense", action="store_true", help="add the dense multi-graph batch (poa_multi_*_dense) to the one-piece paths")
    ap.add_argument("--exact", action="store_true", help="the exact multi-graph batch in hybrid mode against the per-graph hybrid loop, 1 and --reads reads per graph")
    ap.add_argument("--wide", action="store_true", help="reads of 1100 - 1300 bp on graphs of about 1300 rows: the wide dense batch (with --exact: and the wide exact batch)")
    ap.add_argument("--dense2", action="store_true", help="the dense two-piece multi-graph batch (poa_multi_*_dense_2piece) against the checkpointed two-piece batch")
    ap.add_argument("--exact-reads", type=int, default=1, help="--wide --exact: reads per graph of the exact batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.dense2:
        if args.dense or args.exact or args.wide:
            ap.error("--dense2 stands alone (it implies the --two-piece workload)")
        return dense2_main(args)
    if args.wide:
        if args.two_piece:
            ap.error("--wide is one-piece")
        return wide_main(args, ap)
    if args.exact:
        if args.two_piece or args.dense:
            ap.error("--exact stands alone")
        return exact_main(args)
    two = args.two_piece
    if two and args.dense:
        ap.error("--dense is one-piece")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "pr_multi_dense" if args.dense else ("pr_multi_graph_2piece" if two else "pr_multi_graph"), "timing.json")
    import numpy as np
    from poasta_amd import _lib, aligner, workloads as W

    graphs, packed, seqs = [], [], []
    for k in range(args.graphs):
        g, (qseq, qoff) = W.scaled_linearish(190, 10, 5, args.reads, args.length, graph_seed=100 + k, query_seed=5000 + k)
        graphs.append(g)
        packed.append((qseq, qoff))
        seqs.append([qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(args.reads)])
    dgs = [aligner._device_graph(g) for g in graphs]
    costs = aligner.GapAffine2Piece(4, 2, 6, 1, 24) if two else aligner.GapAffine(4, 2, 6)
    c = costs._c()
    L = _lib.lib()
    n_total = args.graphs * args.reads
    cells = sum(g.n * (int(qoff[-1]) + args.reads) for g, (_, qoff) in zip(graphs, packed))

    mb = aligner.MultiGraphBatch(graphs, seqs, two_piece=two)
    al = aligner.PoastaAligner(aligner.Affine2PieceDijkstra(costs) if two else aligner.AffineMinGapCost(costs))

    last_multi_stats = {}

    def step_multi():
        mb.run(costs)
        r = mb.fetch()
        last_multi_stats.update(r.stats)
        return r, r.stats["ms_forward"], r.stats["ms_traceback"]

    def step_one_shot():
        r = al.align_multi(graphs, seqs)
        return r, r.stats["ms_forward"], r.stats["ms_traceback"]

    md = aligner.MultiGraphBatch(graphs, seqs, dense=True) if args.dense else None
    last_dense_stats = {}

    def step_dense():
        md.run(costs)
        r = md.fetch()
        last_dense_stats.update(r.stats)
        return r, r.stats["ms_forward"], r.stats["ms_traceback"]

    def step_dense_one_shot():
        r = al.align_multi(graphs, seqs, mode="dense")
        return r, r.stats["ms_forward"], r.stats["ms_traceback"]

    def loop(mode):
        if not two:
            cfg = aligner.make_config(mode)
        elif mode == "checkpoint":
            cfg = aligner.make_config("checkpoint2")   # (the dense two-piece call takes no config)

        def step():
            score, flags, pairs, counts = [], [], [], []
            fwd = tb = 0.0
            for dg, (qseq, qoff) in zip(dgs, packed):
                n = len(qoff) - 1
                cap = int(qoff[-1]) + n * dg.graph.n
                s, f, po = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
                pr = np.zeros((cap, 2), np.uint32)
                st = _lib.PoaStats()
                if not two:
                    _lib.check(L.poa_align_batch_ex(dg.handle, C.byref(c), C.byref(cfg), n, aligner._p(qseq), aligner._p(qoff), aligner._p(s),
                                                    aligner._p(pr), aligner._p(po), cap, aligner._p(f), C.byref(st), 0))
                elif mode == "dense":
                    _lib.check(L.poa_align_batch_2piece(dg.handle, C.byref(c), n, aligner._p(qseq), aligner._p(qoff), aligner._p(s),
                                                        aligner._p(pr), aligner._p(po), cap, aligner._p(f), C.byref(st), 0))
                else:
                    _lib.check(L.poa_align_batch_2piece_ex(dg.handle, C.byref(c), C.byref(cfg), n, aligner._p(qseq), aligner._p(qoff),
                                                           aligner._p(s), aligner._p(pr), aligner._p(po), cap, aligner._p(f), C.byref(st),
                                                           None, 0))
                fwd += st.ms_forward
                tb += st.ms_traceback
                score.append(s); flags.append(f); pairs.append(pr[:int(po[n])]); counts.append(np.diff(po.astype(np.int64)))
            off = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.uint64)
            return aligner.BatchResult(np.concatenate(score), np.concatenate(pairs), off, np.concatenate(flags), {}), fwd, tb
        return step

    paths = {"multi_run_fetch": step_multi, "multi_one_shot": step_one_shot, "loop_checkpoint": loop("checkpoint"), "loop_dense": loop("dense")}
    if args.dense:
        paths = dict([("dense_run_fetch", step_dense), ("dense_one_shot", step_dense_one_shot)] + list(paths.items()))
    rows = {k: [] for k in paths}
    sums = {}
    for rep in range(args.warmup + args.steps):
        for name, step in paths.items():
            t0 = time.perf_counter()
            res, fwd, tb = step()
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                rows[name].append((wall, fwd, tb))
            sums[name] = {"score_sum": int(res.score.astype(np.uint64).sum()), "flags_crc32": zlib.crc32(res.flags.tobytes()),
                          "n_pairs": int(res.pair_off[-1]), "pairs_crc32": zlib.crc32(np.ascontiguousarray(res.pairs).tobytes())}
            del res

    def med(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

    out = {"workload": "%d graphs x %d reads of %d bp, LinearishPOA backbone 190" % (args.graphs, args.reads, args.length),
           "costs": "4 / 6,24 / 2,1 (mismatch / open1,open2 / extend1,extend2)" if two else "4 / 6 / 2 (mismatch / open / extend)", "graphs": args.graphs, "queries": n_total,
           "rows_per_graph": {"min": min(g.n for g in graphs), "max": max(g.n for g in graphs)}, "cells": cells,
           "steps": args.steps, "warmup": args.warmup, "multi_workspace_bytes": mb.workspace_bytes(),
           "multi_footprint_bytes": aligner.multi_footprint(graphs, seqs, two_piece=two)[0],
           "results_equal": all(sums[k] == sums["loop_dense"] for k in sums)}
    for name in paths:
        out[name] = {"ms_step": med([r[0] for r in rows[name]]), "ms_forward_kernels": med([r[1] for r in rows[name]]),
                     "ms_traceback_kernels": med([r[2] for r in rows[name]])}
        out[name].update(sums[name])
    for name in ("multi_run_fetch", "multi_one_shot") + (("dense_run_fetch", "dense_one_shot") if args.dense else ()):
        for base in ("loop_checkpoint", "loop_dense") + (("multi_run_fetch", "multi_one_shot") if name.startswith("dense") else ()):
            out["ms_step_ratio_%s_over_%s" % (name, base)] = round(out[name]["ms_step"]["median"] / out[base]["ms_step"]["median"], 4)
    # the resident run's own record (poa_stats_t of the last step): cell bytes stored, chunks, the passes
    out["multi_run_stats"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in last_multi_stats.items()}
    if args.dense:
        out["dense_workspace_bytes"] = md.workspace_bytes()
        out["dense_footprint_bytes"] = aligner.multi_footprint(graphs, seqs, dense=True)[0]
        out["dense_launches"] = md.launches()
        out["dense_run_stats"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in last_dense_stats.items()}
        md.close()
    mb.close()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if out["results_equal"] else 1


def dense2_main(args):
    import numpy as np
    from poasta_amd import aligner, workloads as W

    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "pr_multi_dense2", "timing.json")
    graphs, seqs = [], []
    for k in range(args.graphs):
        g, (qseq, qoff) = W.scaled_linearish(190, 10, 5, args.reads, args.length, graph_seed=100 + k, query_seed=5000 + k)
        graphs.append(g)
        seqs.append([qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(args.reads)])
    costs = aligner.GapAffine2Piece(4, 2, 6, 1, 24)
    batches = {"checkpoint2_run_fetch": aligner.MultiGraphBatch(graphs, seqs, two_piece=True),
               "dense2_run_fetch": aligner.MultiGraphBatch(graphs, seqs, dense2=True)}
    rows = {k: [] for k in batches}
    sums, last = {}, {}
    for rep in range(args.warmup + args.steps):
        for name, mb in batches.items():
            t0 = time.perf_counter()
            mb.run(costs)
            res = mb.fetch()
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                rows[name].append((wall, res.stats["ms_forward"], res.stats["ms_traceback"]))
            last[name] = res.stats
            sums[name] = {"score_sum": int(res.score.astype(np.uint64).sum()), "flags_crc32": zlib.crc32(res.flags.tobytes()),
                          "n_pairs": int(res.pair_off[-1]), "pairs_crc32": zlib.crc32(np.ascontiguousarray(res.pairs).tobytes())}
            del res

    def med(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

    out = {"workload": "%d graphs x %d reads of %d bp, LinearishPOA backbone 190" % (args.graphs, args.reads, args.length),
           "costs": "4 / 6,24 / 2,1 (mismatch / open1,open2 / extend1,extend2)", "graphs": args.graphs, "queries": args.graphs * args.reads,
           "rows_per_graph": {"min": min(g.n for g in graphs), "max": max(g.n for g in graphs)},
           "cells": sum(g.n * (len(q) + 1) for g, qs in zip(graphs, seqs) for q in qs), "steps": args.steps, "warmup": args.warmup,
           "results_equal": sums["dense2_run_fetch"] == sums["checkpoint2_run_fetch"]}
    # ms_first_launch: pass 1 (the sweep with snapshots) / the forward launch; ms_second_launch: pass 2 (recompute and walk) / the
    # walk launch, each with the scan and compaction of the pairs behind it
    for name, mb in batches.items():
        out[name] = {"ms_step": med([r[0] for r in rows[name]]), "ms_first_launch": med([r[1] for r in rows[name]]),
                     "ms_second_launch": med([r[2] for r in rows[name]]), "plane_bytes": int(last[name]["plane_bytes"]),
                     "workspace_bytes": mb.workspace_bytes(), "n_chunks": int(last[name]["n_chunks"])}
        out[name].update(sums[name])
        mb.close()
    out["checkpoint2_footprint_bytes"] = aligner.multi_footprint(graphs, seqs, two_piece=True)[0]
    out["dense2_footprint_bytes"] = aligner.multi_footprint(graphs, seqs, dense2=True)[0]
    out["ms_step_ratio_dense2_over_checkpoint2"] = round(out["dense2_run_fetch"]["ms_step"]["median"] / out["checkpoint2_run_fetch"]["ms_step"]["median"], 4)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if out["results_equal"] else 1


def exact_main(args):
    import numpy as np
    from poasta_amd import _lib, aligner, workloads as W

    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "pr_multi_exact", "timing.json")
    costs = aligner.GapAffine(4, 2, 6)
    c = costs._c()
    L = _lib.lib()
    al = aligner.PoastaAligner(aligner.AffineMinGapCost(costs), mode="hybrid")

    def med(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

    out = {"costs": "4 / 6 / 2 (mismatch / open / extend)", "mode": "hybrid, min-gap heuristic, pruning", "graphs": args.graphs, "steps": args.steps,
           "warmup": args.warmup, "shapes": {}}
    ok = True
    for reads in sorted({1, args.reads}):
        graphs, packed, seqs = [], [], []
        for k in range(args.graphs):
            g, (qseq, qoff) = W.scaled_linearish(190, 10, 5, reads, args.length, graph_seed=100 + k, query_seed=5000 + k)
            graphs.append(g)
            packed.append((qseq, qoff))
            seqs.append([qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(reads)])
        dgs = [aligner._device_graph(g) for g in graphs]
        cfg = aligner.make_config("hybrid")
        mb = aligner.MultiGraphBatch(graphs, seqs, exact=True, config=cfg)
        last = {}

        def step_resident():
            mb.run(costs, config=cfg)
            r = mb.fetch()
            last.update(r.stats)
            return r, r.stats

        def step_one_shot():
            r = al.align_multi(graphs, seqs, mode="hybrid")
            return r, r.stats

        def step_loop():
            score, flags, pairs, counts = [], [], [], []
            tot = {"ms_forward": 0.0, "ms_traceback": 0.0, "ms_exact": 0.0, "n_exact": 0}
            for dg, (qseq, qoff) in zip(dgs, packed):
                n = len(qoff) - 1
                cap = int(qoff[-1]) + n * dg.graph.n
                s, f, po = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
                pr = np.zeros((cap, 2), np.uint32)
                st = _lib.PoaStats()
                _lib.check(L.poa_align_batch_ex(dg.handle, C.byref(c), C.byref(cfg), n, aligner._p(qseq), aligner._p(qoff), aligner._p(s),
                                                aligner._p(pr), aligner._p(po), cap, aligner._p(f), C.byref(st), 0))
                for k in tot:
                    tot[k] += getattr(st, k)
                score.append(s); flags.append(f); pairs.append(pr[:int(po[n])]); counts.append(np.diff(po.astype(np.int64)))
            off = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.uint64)
            return aligner.BatchResult(np.concatenate(score), np.concatenate(pairs), off, np.concatenate(flags), {}), tot

        paths = {"exact_run_fetch": step_resident, "exact_one_shot": step_one_shot, "loop_hybrid_one_shot": step_loop}
        rows = {k: [] for k in paths}
        sums = {}
        for rep in range(args.warmup + args.steps):
            for name, step in paths.items():
                t0 = time.perf_counter()
                res, st = step()
                wall = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    rows[name].append((wall, st["ms_forward"] + st["ms_traceback"], st["ms_exact"]))
                sums[name] = {"score_sum": int(res.score.astype(np.uint64).sum()), "flags_crc32": zlib.crc32(res.flags.tobytes()),
                              "n_pairs": int(res.pair_off[-1]), "pairs_crc32": zlib.crc32(np.ascontiguousarray(res.pairs).tobytes()),
                              "n_replayed": int(st["n_exact"])}
                del res
        shape = {"workload": "%d graphs x %d reads of %d bp, LinearishPOA backbone 190" % (args.graphs, reads, args.length), "queries": args.graphs * reads,
                 "rows_per_graph": {"min": min(g.n for g in graphs), "max": max(g.n for g in graphs)},
                 "results_equal": all(sums[k] == sums["loop_hybrid_one_shot"] for k in sums),
                 "footprint_bytes": aligner.multi_footprint(graphs, seqs, exact=True, config=cfg)[0], "plane_workspace_bytes": mb.workspace_bytes(),
                 "launches": mb.launches(), "run_stats": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in last.items()}}
        for name in paths:
            shape[name] = {"ms_step": med([r[0] for r in rows[name]]), "ms_dense_kernels": med([r[1] for r in rows[name]]),
                           "ms_replay_kernels": med([r[2] for r in rows[name]])}
            shape[name].update(sums[name])
        for name in ("exact_run_fetch", "exact_one_shot"):
            shape["ms_step_ratio_%s_over_loop" % name] = round(shape[name]["ms_step"]["median"] / shape["loop_hybrid_one_shot"]["ms_step"]["median"], 4)
        ok = ok and shape["results_equal"]
        out["shapes"]["%d_reads_per_graph" % reads] = shape
        mb.close()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


def wide_main(args, ap):
    import numpy as np
    from poasta_amd import _lib, aligner, workloads as W
    from poasta_amd.graph import pack_queries

    n_graphs = args.graphs if args.graphs != ap.get_default("graphs") else 64
    n_reads = args.reads if args.reads != ap.get_default("reads") else 8
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "pr_multi_wide", "timing.json")
    costs = aligner.GapAffine(4, 2, 6)
    c = costs._c()
    L = _lib.lib()
    graphs, seqs = [], []
    for k in range(n_graphs):
        poa = W.LinearishPOA(1200, 100, 0, seed=300 + k)
        rng = np.random.default_rng(7000 + k)
        graphs.append(poa.graph)
        seqs.append([poa.queries(1, length=int(rng.integers(1100, 1301)), seed=7000 + k, first=i)[0] for i in range(n_reads)])
    cut = [[q[:1023] for q in qs] for qs in seqs]
    dgs = [aligner._device_graph(g) for g in graphs]
    lens = [len(q) for qs in seqs for q in qs]
    cells_of = lambda ss: sum(g.n * (len(q) + 1) for g, qs in zip(graphs, ss) for q in qs)

    def resident(mb, cfg=None):
        last = {}

        def step():
            mb.run(costs, config=cfg)
            r = mb.fetch()
            last.update(r.stats)
            return r, r.stats
        return step, last

    def loop(ss, cfg):
        packed = [pack_queries(qs) for qs in ss]

        def step():
            score, flags, pairs, counts = [], [], [], []
            tot = {"ms_forward": 0.0, "ms_traceback": 0.0, "ms_exact": 0.0, "n_exact": 0}
            for dg, (qseq, qoff) in zip(dgs, packed):
                n = len(qoff) - 1
                cap = int(qoff[-1]) + n * dg.graph.n
                s, f, po = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
                pr = np.zeros((cap, 2), np.uint32)
                st = _lib.PoaStats()
                _lib.check(L.poa_align_batch_ex(dg.handle, C.byref(c), C.byref(cfg), n, aligner._p(qseq), aligner._p(qoff), aligner._p(s),
                                                aligner._p(pr), aligner._p(po), cap, aligner._p(f), C.byref(st), 0))
                for k in tot:
                    tot[k] += getattr(st, k)
                score.append(s); flags.append(f); pairs.append(pr[:int(po[n])]); counts.append(np.diff(po.astype(np.int64)))
            off = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.uint64)
            return aligner.BatchResult(np.concatenate(score), np.concatenate(pairs), off, np.concatenate(flags), {}), tot
        return step

    md = aligner.MultiGraphBatch(graphs, seqs, dense=True)
    mc = aligner.MultiGraphBatch(graphs, seqs)
    ms = aligner.MultiGraphBatch(graphs, cut, dense=True, wide=True)
    assert md.wide and ms.wide
    step_w, last_w = resident(md)
    step_a, last_a = resident(mc)
    step_s, last_s = resident(ms)
    paths = {"wide_dense_run_fetch": step_w, "checkpoint_run_fetch": step_a, "loop_dense_one_shot": loop(seqs, aligner.make_config("dense")),
             "cut_1023_dense_run_fetch": step_s}
    groups = {"full": ["wide_dense_run_fetch", "checkpoint_run_fetch", "loop_dense_one_shot"], "cut": ["cut_1023_dense_run_fetch"]}
    mx = None
    if args.exact:
        hyb = aligner.make_config("hybrid")
        xseqs = [qs[:args.exact_reads] for qs in seqs]
        mx = aligner.MultiGraphBatch(graphs, xseqs, exact=True, config=hyb)
        assert mx.wide
        step_e, last_e = resident(mx, hyb)
        paths.update({"wide_exact_run_fetch": step_e, "loop_hybrid_one_shot": loop(xseqs, hyb)})
        groups["exact"] = ["wide_exact_run_fetch", "loop_hybrid_one_shot"]
    rows = {k: [] for k in paths}
    sums = {}
    for rep in range(args.warmup + args.steps):
        for name, step in paths.items():
            t0 = time.perf_counter()
            res, st = step()
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                rows[name].append((wall, st["ms_forward"], st["ms_traceback"], st.get("ms_exact", 0.0)))
            sums[name] = {"score_sum": int(res.score.astype(np.uint64).sum()), "flags_crc32": zlib.crc32(res.flags.tobytes()),
                          "n_pairs": int(res.pair_off[-1]), "pairs_crc32": zlib.crc32(np.ascontiguousarray(res.pairs).tobytes())}
            del res

    def med(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

    out = {"workload": "%d graphs x %d reads of 1100 - 1300 bp, LinearishPOA backbone 1200 with 100 SNP bubbles" % (n_graphs, n_reads),
           "costs": "4 / 6 / 2 (mismatch / open / extend)", "graphs": n_graphs, "queries": n_graphs * n_reads,
           "rows_per_graph": {"min": min(g.n for g in graphs), "max": max(g.n for g in graphs)},
           "read_length": {"min": min(lens), "max": max(lens)}, "cells": cells_of(seqs), "cells_cut_1023": cells_of(cut),
           "steps": args.steps, "warmup": args.warmup,
           "results_equal": {g: all(sums[k] == sums[names[0]] for k in names) for g, names in groups.items() if len(names) > 1}}
    for name in paths:
        out[name] = {"ms_step": med([r[0] for r in rows[name]]), "ms_forward_kernels": med([r[1] for r in rows[name]]),
                     "ms_traceback_kernels": med([r[2] for r in rows[name]])}
        if name in groups.get("exact", ()):
            out[name]["ms_replay_kernels"] = med([r[3] for r in rows[name]])
        out[name].update(sums[name])
    w = out["wide_dense_run_fetch"]["ms_step"]["median"]
    for base in ("checkpoint_run_fetch", "loop_dense_one_shot"):
        out["ms_step_ratio_wide_dense_over_%s" % base] = round(w / out[base]["ms_step"]["median"], 4)
    # what the strip loop itself costs: forward-kernel time per cell, wide against the same reads cut to one strip
    per_cell = lambda name, cells: out[name]["ms_forward_kernels"]["median"] * 1e6 / cells
    out["forward_ns_per_cell"] = {"wide": round(per_cell("wide_dense_run_fetch", out["cells"]), 5),
                                  "cut_1023": round(per_cell("cut_1023_dense_run_fetch", out["cells_cut_1023"]), 5)}
    out["forward_ns_per_cell_ratio_wide_over_cut_1023"] = round(out["forward_ns_per_cell"]["wide"] / out["forward_ns_per_cell"]["cut_1023"], 4)
    if args.exact:
        out["exact_reads_per_graph"] = args.exact_reads
        out["ms_step_ratio_wide_exact_over_loop_hybrid"] = round(out["wide_exact_run_fetch"]["ms_step"]["median"] / out["loop_hybrid_one_shot"]["ms_step"]["median"], 4)
        out["wide_exact_launches"] = mx.launches()
        out["wide_exact_run_stats"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in last_e.items()}
        mx.close()
    out["wide_dense_workspace_bytes"] = md.workspace_bytes()
    out["wide_dense_footprint_bytes"] = aligner.multi_footprint(graphs, seqs, dense=True)[0]
    out["checkpoint_workspace_bytes"] = mc.workspace_bytes()
    out["wide_dense_launches"] = md.launches()
    out["cut_1023_launches"] = ms.launches()
    out["wide_dense_run_stats"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in last_w.items()}
    out["checkpoint_run_stats"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in last_a.items()}
    for mb in (md, mc, ms):
        mb.close()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if all(out["results_equal"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
