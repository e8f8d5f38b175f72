#!/usr/bin/env python3
"""Capped score-set runs on the workload of scripts/scoreset_timing.py: what the checks cost, and what stopping early saves.

Workload: 256 graphs (LinearishPOA at a backbone of 190, about 212 rows) and their 32 x 256 reads of about 200 bp, fixed seeds,
costs 4 / 6 / 2; every read against its own graph and 7 others, 65 536 pairs on one resident score set.  Per step, interleaved in
one process:
  (a) poa_scoreset_run + poa_scoreset_fetch, uncapped;
  (b) poa_scoreset_run_capped with every cap POA_SCORE_UNVISITED: the pure cost of the checks — per stride;
  (c) poa_scoreset_run_capped with, per read, a cap of 1.5 times the read's score on its own graph, taken from (a) — per stride;
      also the share of pairs capped and the mean of swept / rows over the losing pairs (poa_scoreset_fetch_swept).
The strides are 1, the engine's default and one larger.  The first --warmup steps are dropped; medians with min / max of the
rest; the step time is the host clock around run + fetch (which synchronises), the kernel time the HIP-event sum of poa_stats_t.
Every measurement runs in a child process under its own time limit; a non-zero status ends the script.

--parent-lib names a build of the parent commit's library: (a) is then also measured on it (POA_LIB_PATH), before and after this
tree's measurement, and on this tree a second time, so that the difference between the two trees can be read against the spread
of each tree's own two runs.  Writes profiles/pr_scoreset_cap/timing.json.
"""
import argparse
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
NONE = 0xFFFFFFFF
LARGE_STRIDE = 32


def measure(args):
    import numpy as np
    from poasta_amd import aligner, workloads as W

    graphs, seqs = [], []
    for k in range(args.graphs):
        g, (qseq, qoff) = W.scaled_linearish(190, 10, 5, args.reads, args.length, graph_seed=100 + k, query_seed=5000 + k)
        graphs.append(g)
        seqs += [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(args.reads)]
    # read i of graph k against graph k and the graphs k + 37 j (scripts/scoreset_timing.py): the first of a read's eight is its own
    pairs = np.array([(k * args.reads + i, (k + 37 * j) % args.graphs) for k in range(args.graphs) for i in range(args.reads)
                      for j in range(OTHERS + 1)], np.int64)
    n = len(pairs)
    rows = np.array([graphs[gi].n for gi in pairs[:, 1]], np.float64)
    costs = aligner.GapAffine(4, 2, 6)
    ss = aligner.ScoreSet(graphs, seqs, pairs=pairs)

    def step(cap=None, stride=None):
        cfg = aligner.make_config("score", cap_stride=stride) if stride else None
        ss.run(costs, config=cfg, cap=cap)
        score, flags, st = ss.fetch()
        return score, flags, st["ms_forward"]

    score0, flags0, _ = step()
    own = score0.reshape(-1, OTHERS + 1)[:, 0].astype(np.uint64)
    cap15 = np.repeat((own * 3) // 2, OTHERS + 1).astype(np.uint32)
    none = np.full(n, NONE, np.uint32)
    want15 = np.where(score0 > cap15, NONE, score0).astype(np.uint32)

    variants = {"uncapped": (None, None)}
    if not args.uncapped_only:
        strides = [("stride_1", 1), ("stride_default", None), ("stride_%d" % LARGE_STRIDE, LARGE_STRIDE)]
        for name, stride in strides:
            variants["no_cap_" + name] = (none, stride)
        for name, stride in strides:
            variants["cap_1.5x_own_" + name] = (cap15, stride)
    times = {k: [] for k in variants}
    info = {}
    for rep in range(args.warmup + args.steps):
        for name, (cap, stride) in variants.items():
            t0 = time.perf_counter()
            score, flags, fwd = step(cap, stride)
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                times[name].append((wall, fwd))
            if rep == 0:
                want = want15 if cap is cap15 else score0
                d = {"results_as_expected": bool(np.array_equal(score, want)), "score_crc32": zlib.crc32(score.tobytes())}
                if cap is not None:
                    swept = ss.swept_rows().astype(np.float64)
                    capped = (flags & 0x80) != 0
                    d.update(pairs_capped=int(capped.sum()), share_capped=round(float(capped.mean()), 4),
                             mean_swept_over_rows_all_pairs=round(float((swept / rows).mean()), 4),
                             mean_swept_over_rows_capped_pairs=round(float((swept[capped] / rows[capped]).mean()), 4) if capped.any() else None,
                             pairs_stopped_early=int((swept < rows).sum()))
                info[name] = d

    def med(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

    out = {"library": "the parent commit's build (--parent-lib)" if os.environ.get("POA_LIB_PATH") else "this tree", "pairs": n, "graphs": args.graphs, "queries": len(seqs),
           "rows_per_graph": {"min": min(g.n for g in graphs), "max": max(g.n for g in graphs)}, "steps": args.steps, "warmup": args.warmup,
           "own_graph_is_the_best_of_its_eight": int((score0.reshape(-1, OTHERS + 1).argmin(axis=1) == 0).sum()),
           "own_graph_score_median": int(np.median(own)),
           "check_rows_of_graph_0": {"stride_1": int(aligner.sweep_checks(graphs[0], 1).sum()), "default": int(aligner.sweep_checks(graphs[0], 0).sum())}
                                    if not args.uncapped_only else None, "uncapped_score_crc32": zlib.crc32(score0.tobytes()), "variants": {}}
    for name in variants:
        out["variants"][name] = {"ms_step": med([r[0] for r in times[name]]), "ms_forward_kernels": med([r[1] for r in times[name]])}
        out["variants"][name].update(info[name])
    base = out["variants"]["uncapped"]
    for name in variants:
        v = out["variants"][name]
        v["ms_step_over_uncapped"] = round(v["ms_step"]["median"] / base["ms_step"]["median"], 4)
        v["ms_kernels_over_uncapped"] = round(v["ms_forward_kernels"]["median"] / base["ms_forward_kernels"]["median"], 4)
    ss.close()
    print(json.dumps(out))
    return 0 if all(v["results_as_expected"] for v in out["variants"].values()) else 1


def child(args, lib=None, uncapped_only=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--measure"] + [a for k in ("graphs", "reads", "length", "steps", "warmup")
                                                                      for a in ("--" + k, str(getattr(args, k)))]
    if uncapped_only:
        cmd.append("--uncapped-only")
    env = dict(os.environ)
    env.pop("POA_LIB_PATH", None)
    if lib:
        env["POA_LIB_PATH"] = os.path.abspath(lib)
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_LIMIT_S, env=env)
    except subprocess.TimeoutExpired:
        print("the measurement exceeded its %d s: stopping" % STEP_LIMIT_S, file=sys.stderr)
        sys.exit(124)
    lines = p.stdout.decode().strip().splitlines()
    if p.returncode != 0 or not lines:
        print("the measurement failed with status %d: stopping" % p.returncode, file=sys.stderr)
        if lines:
            print(lines[-1], flush=True)
        sys.exit(p.returncode if p.returncode > 0 else 1)
    print(lines[-1], flush=True)
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--reads", type=int, default=32)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--measure", action="store_true", help="measure in this process and print the JSON line")
    ap.add_argument("--uncapped-only", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libpoasta_amd.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_scoreset_cap", "timing.json"))
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    out = {"workload": "%d graphs x %d reads of %d bp, LinearishPOA backbone 190; every read against its own graph and %d others"
                       % (args.graphs, args.reads, args.length, OTHERS), "costs": "4 / 6 / 2 (mismatch / open / extend)"}
    if args.parent_lib:
        out["parent_uncapped_first"] = child(args, args.parent_lib, True)
    out["this_tree"] = child(args)
    if args.parent_lib:
        out["parent_uncapped_second"] = child(args, args.parent_lib, True)
        out["this_tree_uncapped_second"] = child(args, None, True)
        med = lambda d: d["variants"]["uncapped"]["ms_step"]["median"]
        kmed = lambda d: d["variants"]["uncapped"]["ms_forward_kernels"]["median"]
        p1, p2, t1, t2 = (out[k] for k in ("parent_uncapped_first", "parent_uncapped_second", "this_tree", "this_tree_uncapped_second"))
        out["uncapped_parent_vs_this_tree"] = {
            "ms_step_parent": [med(p1), med(p2)], "ms_step_this_tree": [med(t1), med(t2)],
            "ms_kernels_parent": [kmed(p1), kmed(p2)], "ms_kernels_this_tree": [kmed(t1), kmed(t2)],
            "parent_run_to_run_spread_kernels": round(abs(kmed(p1) - kmed(p2)) / min(kmed(p1), kmed(p2)), 4),
            "this_tree_over_parent_kernels": round((kmed(t1) + kmed(t2)) / (kmed(p1) + kmed(p2)), 4),
            "same_scores": p1["uncapped_score_crc32"] == t1["uncapped_score_crc32"]}
    else:
        out["parent_uncapped"] = "not measured (no --parent-lib)"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
