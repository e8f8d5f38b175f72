#!/usr/bin/env python3
"""Checkpointed mode against dense mode, same box, same process, interleaved repetitions (one GPU).

Workloads: configs[1] at full size, configs[3] at its full 5 000 queries, configs[4].  Each workload runs in a child process of
its own under its own time limit; the first failing step ends the run.  Per workload and mode: medians with min / max of
ms_forward (checkpointed: pass 1), ms_traceback (checkpointed: pass 2 + compaction) and the whole step (run + fetch of scores and
flags), workspace bytes, chunks, the plan, and a checksum of the scores and of the pairs (one extra run with the pairs fetched).
Writes profiles/pr_checkpoint/timing.json.
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
    "configs[1]": (lambda W, n: W.config2(n_queries=n or 10000), 9, 240),
    "configs[3]": (lambda W, n: W.config4(n_queries=n or 5000), 2, 900),
    "configs[4]": (lambda W, n: W.config5(n_queries=n or 2000), 3, 420),
}


CAP_BYTES = 100 << 30


def measure(name, reps_override=0, n_queries=0):
    import zlib
    import numpy as np
    from poasta_amd import aligner, workloads as W
    make, reps, _ = WORKLOADS[name]
    reps = reps_override or reps
    g, (qseq, qoff) = make(W, n_queries)   # n_queries: a smaller batch of the same workload (profiler runs)
    costs = aligner.GapAffine(4, 2, 6)
    cfg = aligner.make_config("checkpoint")
    # both batches are resident at once: each gets the same cap on its plane workspace (a batch takes no more than it needs)
    batches = {"dense": aligner.ResidentBatch(g, qseq, qoff, workspace_bytes=CAP_BYTES),
               "checkpoint": aligner.ResidentBatch(g, qseq, qoff, workspace_bytes=CAP_BYTES, config=cfg)}
    configs = {"checkpoint": cfg, "dense": None}
    rows = {m: [] for m in batches}
    sums = {}
    for rep in range(reps + 1):   # repetition 0 warms up both modes and is dropped
        for mode in ("dense", "checkpoint"):
            rb = batches[mode]
            t0 = time.perf_counter()
            rb.run(costs, None, configs[mode])
            res = rb.fetch(want_pairs=False)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                rows[mode].append((res.stats["ms_forward"], res.stats["ms_traceback"], wall, res.stats["n_chunks"], res.stats["cells"]))
    for mode in ("dense", "checkpoint"):   # the results themselves, once: scores, flags, pair offsets and pairs
        rb = batches[mode]
        rb.run(costs, None, configs[mode])
        res = rb.fetch()
        sums[mode] = {"score_sum": int(res.score.astype(np.uint64).sum()), "flagged": int((res.flags != 0).sum()),
                      "n_pairs": int(res.pair_off[-1]), "pairs_crc32": zlib.crc32(np.ascontiguousarray(res.pairs).tobytes()),
                      "flags_crc32": zlib.crc32(res.flags.tobytes())}
        del res
    dg = aligner._device_graph(g)
    boundary, rpq = dg.checkpoint_plan()
    out = {"workload": name, "rows": int(g.n), "queries": len(qoff) - 1, "n_sweep_slots": dg.sweep_slots()[1],
           "segments": len(boundary) - 1, "segment_rows": int(boundary[1]), "rows_per_query": rpq,
           "workspace_cap_bytes": CAP_BYTES, "results_equal": sums["dense"] == sums["checkpoint"]}

    def med(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

    for mode, rb in batches.items():
        out[mode] = {"ms_forward": med([r[0] for r in rows[mode]]), "ms_traceback": med([r[1] for r in rows[mode]]),
                     "ms_step": med([r[2] for r in rows[mode]]), "workspace_bytes": rb.workspace_bytes(), "chunks": rows[mode][0][3],
                     "gcells_per_s_step": round(rows[mode][0][4] / (med([r[2] for r in rows[mode]])["median"] * 1e-3) / 1e9, 1),
                     "layout": sorted(rb.layout()), "repetitions": len(rows[mode])}
        out[mode].update(sums[mode])
        rb.close()
    out["ms_step_ratio_checkpoint_over_dense"] = round(out["checkpoint"]["ms_step"]["median"] / out["dense"]["ms_step"]["median"], 3)
    out["workspace_ratio_checkpoint_over_dense"] = round(out["checkpoint"]["workspace_bytes"] / max(out["dense"]["workspace_bytes"], 1), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), help="measure this one in this process and print its JSON line")
    ap.add_argument("--only", nargs="*", default=None, help="parent: the workloads to run (default: all)")
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--queries", type=int, default=0, help="N queries per workload instead of its full size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_checkpoint", "timing.json"))
    args = ap.parse_args()
    if args.workload:
        print(json.dumps(measure(args.workload, args.reps, args.queries)))
        return 0
    results = []
    for name in (args.only or list(WORKLOADS)):
        limit = WORKLOADS[name][2]
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", name, "--reps", str(args.reps), "--queries", str(args.queries)],
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
