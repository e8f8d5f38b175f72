#!/usr/bin/env python3
"""Which graph does a read belong to: one score set against the per-graph score-mode loop, one process, one GPU, interleaved
repetitions.

Workload: the 256 graphs of scripts/multi_graph_timing.py (LinearishPOA at a backbone of 190, about 212 rows) and their 32 x 256
reads of about 200 bp, fixed seeds, costs 4 / 6 / 2.  Every read is scored against its own graph and 7 others: 65 536 pairs.
Per step:
  (a)  poa_scoreset_run + poa_scoreset_fetch on a resident score set;
  (a1) the one-shot poa_score_pairs, which also creates and destroys the set, as the loop below does per graph;
  (b)  the loop over the graphs of poa_align_batch_ex in POA_MODE_SCORE, each call with the 256 reads paired with that graph —
       the path a host had before.
The first --warmup steps are dropped; medians with min / max of the rest.  Kernel-only time is the HIP-event sum of poa_stats_t
(ms_forward), summed over the calls of a step.  The measurement runs in a child process under its own time limit; a non-zero
status ends the script.  Writes profiles/pr_scoreset/timing.json.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OTHERS = 7
STEP_LIMIT_S = 420


def measure(args):
    import numpy as np
    from poasta_amd import _lib, aligner, workloads as W
    from poasta_amd.graph import pack_queries

    graphs, seqs = [], []
    for k in range(args.graphs):
        g, (qseq, qoff) = W.scaled_linearish(190, 10, 5, args.reads, args.length, graph_seed=100 + k, query_seed=5000 + k)
        graphs.append(g)
        seqs += [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(args.reads)]
    # read i of graph k against graph k and the graphs k + 37 j (37 is odd: seven distinct others for up to 256 graphs)
    pairs = np.array([(k * args.reads + i, (k + 37 * j) % args.graphs) for k in range(args.graphs) for i in range(args.reads)
                      for j in range(OTHERS + 1)], np.int64)
    n = len(pairs)
    dgs = [aligner._device_graph(g) for g in graphs]
    costs = aligner.GapAffine(4, 2, 6)
    c = costs._c()
    cfg = aligner.make_config("score")
    L = _lib.lib()
    cells = int(sum(graphs[gi].n * (len(seqs[qi]) + 1) for qi, gi in pairs))

    ss = aligner.ScoreSet(graphs, seqs, pairs=pairs)
    al = aligner.PoastaAligner(aligner.AffineMinGapCost(costs))

    def step_set():
        ss.run(costs)
        score, flags, st = ss.fetch()
        return score, flags, st["ms_forward"]

    def step_one_shot():
        score, flags = al.score_pairs(graphs, seqs, pairs)
        return score, flags, al.last_stats["ms_forward"]

    by_graph = []   # per graph: the positions of its pairs and their packed queries
    for gi in range(args.graphs):
        pos = np.flatnonzero(pairs[:, 1] == gi)
        by_graph.append((pos,) + tuple(pack_queries([seqs[int(qi)] for qi in pairs[pos, 0]])))

    def step_loop():
        score, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        fwd = 0.0
        for dg, (pos, qseq, qoff) in zip(dgs, by_graph):
            m = len(pos)
            s, f, po = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m + 1, np.uint64)
            st = _lib.PoaStats()
            _lib.check(L.poa_align_batch_ex(dg.handle, C.byref(c), C.byref(cfg), m, aligner._p(qseq), aligner._p(qoff), aligner._p(s), None,
                                            aligner._p(po), 0, aligner._p(f), C.byref(st), 0))
            fwd += st.ms_forward
            score[pos], flags[pos] = s, f
        return score, flags, fwd

    paths = {"scoreset_run_fetch": step_set, "score_pairs_one_shot": step_one_shot, "loop_score_mode": step_loop}
    rows = {k: [] for k in paths}
    sums = {}
    for rep in range(args.warmup + args.steps):
        for name, step in paths.items():
            t0 = time.perf_counter()
            score, flags, fwd = step()
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                rows[name].append((wall, fwd))
            sums[name] = {"score_sum": int(score.astype(np.uint64).sum()), "score_crc32": zlib.crc32(score.tobytes()),
                          "flags_crc32": zlib.crc32(flags.tobytes())}

    def med(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

    own = pairs[:, 1] == pairs[:, 0] // args.reads
    out = {"workload": "%d graphs x %d reads of %d bp, LinearishPOA backbone 190; every read against its own graph and %d others"
                       % (args.graphs, args.reads, args.length, OTHERS),
           "costs": "4 / 6 / 2 (mismatch / open / extend)", "graphs": args.graphs, "queries": len(seqs), "pairs": n,
           "rows_per_graph": {"min": min(g.n for g in graphs), "max": max(g.n for g in graphs)}, "cells": cells,
           "steps": args.steps, "warmup": args.warmup, "scoreset_workspace_bytes": ss.workspace_bytes(),
           "scoreset_footprint_bytes": aligner.scoreset_footprint(graphs, seqs, pairs=pairs)[0],
           "own_graph_is_the_best_of_its_eight": int((score.reshape(-1, OTHERS + 1).argmin(axis=1) == 0).sum()) if own.reshape(-1, OTHERS + 1)[:, 0].all() else None,
           "results_equal": all(sums[k] == sums["loop_score_mode"] for k in sums)}
    for name in paths:
        out[name] = {"ms_step": med([r[0] for r in rows[name]]), "ms_forward_kernels": med([r[1] for r in rows[name]])}
        out[name].update(sums[name])
    for name in ("scoreset_run_fetch", "score_pairs_one_shot"):
        out["ms_step_ratio_%s_over_loop" % name] = round(out[name]["ms_step"]["median"] / out["loop_score_mode"]["ms_step"]["median"], 4)
    ss.close()
    print(json.dumps(out))
    return 0 if out["results_equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--reads", type=int, default=32)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--measure", action="store_true", help="measure in this process and print the JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_scoreset", "timing.json"))
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--measure"] + [a for k in ("graphs", "reads", "length", "steps", "warmup")
                                                                      for a in ("--" + k, str(getattr(args, k)))]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        print("the measurement exceeded its %d s: stopping" % STEP_LIMIT_S, file=sys.stderr)
        return 124
    lines = p.stdout.decode().strip().splitlines()
    if lines:
        print(lines[-1], flush=True)
    if p.returncode != 0 and not lines:
        print("the measurement failed with status %d: stopping" % p.returncode, file=sys.stderr)
        return p.returncode if p.returncode > 0 else 1
    if lines:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(json.loads(lines[-1]), f, indent=1)
            f.write("\n")
    return p.returncode if p.returncode >= 0 else 1


if __name__ == "__main__":
    sys.exit(main())
