#!/usr/bin/env python3
"""Score-only mode against dense mode, same box, same process, interleaved repetitions (one GPU).

Workloads: configs[1] at full size, configs[3] and configs[4] at the sizes tests/test_gpu_full_size.py uses.  Each workload runs
in a child process of its own under its own time limit; the first failing step ends the run.  Per workload and mode:
ms_forward, whole-step ms (run + fetch of scores and flags, no pairs), workspace bytes, chunks, Gcells/s, the sum of scores.
Writes profiles/pr_score_only/timing.json.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {   # name: (constructor, repetitions, time limit of the step in seconds)
    "configs[1]": (lambda W: W.config2(n_queries=10000), 9, 240),
    "configs[3]": (lambda W: W.config4(n_queries=512), 3, 420),
    "configs[4]": (lambda W: W.config5(n_queries=2000), 3, 420),
}


def measure(name, reps_override=0):
    import numpy as np
    from poasta_amd import aligner, workloads as W
    make, reps, _ = WORKLOADS[name]
    reps = reps_override or reps
    g, (qseq, qoff) = make(W)
    costs = aligner.GapAffine(4, 2, 6)
    cfg = aligner.make_config("score")
    batches = {"score": aligner.ResidentBatch(g, qseq, qoff, config=cfg), "dense": aligner.ResidentBatch(g, qseq, qoff)}
    configs = {"score": cfg, "dense": None}
    rows = {m: [] for m in batches}
    sums = {}
    for rep in range(reps + 1):   # repetition 0 warms up both modes and is dropped
        for mode in ("dense", "score"):
            rb = batches[mode]
            t0 = time.perf_counter()
            rb.run(costs, None, configs[mode])
            res = rb.fetch(want_pairs=False)
            wall = (time.perf_counter() - t0) * 1e3
            sums[mode] = int(res.score.astype(np.uint64).sum())
            if rep:
                rows[mode].append((res.stats["ms_forward"], res.stats["ms_traceback"], wall, res.stats["n_chunks"], res.stats["cells"]))
    out = {"workload": name, "rows": int(g.n), "queries": len(qoff) - 1, "n_sweep_slots": aligner._device_graph(g).sweep_slots()[1],
           "scores_equal": sums["dense"] == sums["score"]}
    for mode, rb in batches.items():
        fwd = sorted(r[0] for r in rows[mode])
        wall = sorted(r[2] for r in rows[mode])
        med = fwd[len(fwd) // 2]
        out[mode] = {"ms_forward": round(med, 3), "ms_forward_min": round(fwd[0], 3), "ms_forward_max": round(fwd[-1], 3),
                     "ms_traceback": round(sorted(r[1] for r in rows[mode])[len(fwd) // 2], 3),
                     "ms_step": round(wall[len(wall) // 2], 3), "ms_step_min": round(wall[0], 3), "ms_step_max": round(wall[-1], 3),
                     "workspace_bytes": rb.workspace_bytes(), "chunks": rows[mode][0][3],
                     "gcells_per_s_forward": round(rows[mode][0][4] / (med * 1e-3) / 1e9, 1), "score_sum": sums[mode],
                     "layout": sorted(rb.layout()), "repetitions": len(fwd)}
        rb.close()
    out["ms_forward_ratio_score_over_dense"] = round(out["score"]["ms_forward"] / out["dense"]["ms_forward"], 3)
    out["ms_step_ratio_score_over_dense"] = round(out["score"]["ms_step"] / out["dense"]["ms_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), help="measure this one in this process and print its JSON line")
    ap.add_argument("--only", nargs="*", default=None, help="parent: the workloads to run (default: all)")
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_score_only", "timing.json"))
    args = ap.parse_args()
    if args.workload:
        print(json.dumps(measure(args.workload, args.reps)))
        return 0
    results = []
    for name in (args.only or list(WORKLOADS)):
        limit = WORKLOADS[name][2]
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", name, "--reps", str(args.reps)],
                               stdout=subprocess.PIPE, timeout=limit)
        except subprocess.TimeoutExpired:
            print("step %s exceeded its %d s: stopping" % (name, limit), file=sys.stderr)
            return 124
        if p.returncode != 0:
            print("step %s failed with status %d: stopping" % (name, p.returncode), file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        line = p.stdout.decode().strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"costs": "4 / 6 / 2 (mismatch / open / extend)", "workloads": results}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
