#!/usr/bin/env python3
"""Checkpointed two-piece mode (POA_MODE_CHECKPOINT2) against the dense two-piece resident run, same process, repetitions
interleaved (one GPU), mismatch 4, -g 6,24 -e 2,1.

Workloads: configs[1]'s shape (8 000 reads of 1 kbp), and a configs[3]-shaped sample (56 101 rows x 10 kbp, u32 cells) of as many
queries as the dense run's five planes still fit beside the checkpointed batch.  Each workload runs in a child process of its
own under its own time limit; the first failing step ends the run.  Per workload and mode: medians with min / max of ms_forward
(checkpointed: pass 1), ms_traceback (checkpointed: pass 2) and the whole step (run + fetch of scores and flags), chunks, bytes per
query, and a checksum of the results (one extra run with the pairs fetched).  Writes
profiles/pr_two_piece_checkpoint/timing.json.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {   # name: (constructor, default queries, repetitions, time limit of the step in seconds)
    "configs[1]": (lambda W, n: W.config2(n_queries=n), 8000, 5, 200),
    "configs[3]-sample": (lambda W, n: W.config4(n_queries=n), 12, 2, 400),
}
COSTS = (4, 2, 6, 1, 24)   # GapAffine2Piece(mismatch, extend1, open1, extend2, open2)


def measure(name, reps_override=0, n_queries=0):
    import zlib
    import numpy as np
    from poasta_amd import aligner, workloads as W
    make, n_default, reps, _ = WORKLOADS[name]
    reps = reps_override or reps
    g, (qseq, qoff) = make(W, n_queries or n_default)
    n = len(qoff) - 1
    costs = aligner.GapAffine2Piece(*COSTS)
    cfg = aligner.make_config("checkpoint2")
    batches = {"dense": aligner.ResidentBatch(g, qseq, qoff), "checkpoint2": aligner.ResidentBatch(g, qseq, qoff, config=cfg)}
    configs = {"dense": None, "checkpoint2": cfg}
    rows = {m: [] for m in batches}
    sums = {}
    for rep in range(reps + 1):   # repetition 0 warms up both modes and is dropped
        for mode in ("dense", "checkpoint2"):
            rb = batches[mode]
            t0 = time.perf_counter()
            rb.run(costs, None, configs[mode])
            res = rb.fetch(want_pairs=False)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                rows[mode].append((res.stats["ms_forward"], res.stats["ms_traceback"], wall, res.stats["n_chunks"], res.stats["plane_bytes"]))
    for mode in ("dense", "checkpoint2"):
        rb = batches[mode]
        rb.run(costs, None, configs[mode])
        res = rb.fetch()
        sums[mode] = {"score_sum": int(res.score.astype(np.uint64).sum()), "flagged": int((res.flags != 0).sum()),
                      "n_pairs": int(res.pair_off[-1]), "pairs_crc32": zlib.crc32(np.ascontiguousarray(res.pairs).tobytes()),
                      "flags_crc32": zlib.crc32(res.flags.tobytes())}
        del res
    dg = aligner._device_graph(g)
    boundary, rpq = dg.checkpoint_plan(two_piece=True)
    pitch_sum = sum((int(qoff[i + 1] - qoff[i]) + 1 + 63) // 64 * 64 for i in range(n))
    out = {"workload": name, "rows": int(g.n), "queries": n, "n_sweep_slots": dg.sweep_slots()[1], "segments": len(boundary) - 1,
           "segment_rows": int(boundary[1]), "rows_per_query2": rpq, "results_equal": sums["dense"] == sums["checkpoint2"]}

    def med(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

    for mode, rb in batches.items():
        layout = sorted(rb.layout())
        cell = 2 if "u16" in layout else 4
        held = (rpq if mode == "checkpoint2" else 5 * g.n) * pitch_sum * cell // n   # what a run of this width addresses per query
        out[mode] = {"ms_forward": med([r[0] for r in rows[mode]]), "ms_traceback": med([r[1] for r in rows[mode]]),
                     "ms_step": med([r[2] for r in rows[mode]]), "chunks": rows[mode][0][3], "workspace_bytes": rb.workspace_bytes(),
                     "bytes_per_query": held, "plane_bytes_written": rows[mode][0][4], "layout": layout, "repetitions": len(rows[mode])}
        out[mode].update(sums[mode])
        rb.close()
    out["ms_step_ratio"] = round(out["checkpoint2"]["ms_step"]["median"] / out["dense"]["ms_step"]["median"], 3)
    out["bytes_per_query_ratio"] = round(out["checkpoint2"]["bytes_per_query"] / out["dense"]["bytes_per_query"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), help="measure this one in this process and print its JSON line")
    ap.add_argument("--only", nargs="*", default=None, help="parent: the workloads to run (default: all)")
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--queries", type=int, default=0, help="N queries per workload instead of its default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_two_piece_checkpoint", "timing.json"))
    args = ap.parse_args()
    if args.workload:
        print(json.dumps(measure(args.workload, args.reps, args.queries)))
        return 0
    results = []
    for name in (args.only or list(WORKLOADS)):
        limit = WORKLOADS[name][3]
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
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"costs": "mismatch 4, -g 6,24 -e 2,1", "workloads": results}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
