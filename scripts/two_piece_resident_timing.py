#!/usr/bin/env python3
"""Two-piece model: the one-shot call (poa_align_batch_2piece) against the resident run (poa_batch_run_2piece), same box, same
process, alternating repetitions (one GPU).

configs[1] shape under `poasta align -g 6,24 -e 2,1` (mismatch 4).  Per path and repetition: kernel time (ms_forward +
ms_traceback, HIP events) and wall time of the whole step (one-shot: the call; resident: run + fetch of everything).  Then the
step time with two resident batches in flight on two streams, and the memory of a mixed-length batch (one 10 kbp read among
1 kbp reads): bytes of planes per query as the one-shot call sizes them (every query at the longest query's pitch) and as the
batch holds them (each at its own).  The results of both paths are compared once, bit for bit.
Writes profiles/pr_two_piece_resident/timing.json and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch   # (before the engine: streams for the two batches in flight)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from poasta_amd import aligner, workloads as W
from poasta_amd.graph import pack_queries

COSTS = aligner.GapAffine2Piece(4, 2, 6, 1, 24)


def same(a, b):
    n = len(a.score)
    return bool(np.array_equal(a.score, b.score) and np.array_equal(a.flags, b.flags) and np.array_equal(a.pair_off, b.pair_off)
                and np.array_equal(a.pairs[:int(a.pair_off[n])], b.pairs[:int(b.pair_off[n])]))


def spread(v):
    return {"values": [round(x, 3) for x in v], "median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8, help="steps of the two-in-flight loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_two_piece_resident", "timing.json"))
    args = ap.parse_args()
    g, (qseq, qoff) = W.config2(n_queries=args.queries)
    al = aligner.PoastaAligner(aligner.Affine2PieceDijkstra(COSTS))
    out = {"workload": "configs[1]", "queries": args.queries, "rows": int(g.n), "costs": "mismatch 4, -g 6,24 -e 2,1"}
    # a mixed-length batch: what one long read costs the short ones (first: before any larger workspace is parked for reuse)
    poa = W.LinearishPOA(seed=1)
    qs = poa.queries(63, length=1000) + poa.queries(1, length=10000, first=63)
    mq, mo = pack_queries(qs)
    pitch = [(len(q) + 64) // 64 * 64 for q in qs]
    m_one = al.align_batch(poa.graph, qseq=mq, qoff=mo)
    mb = aligner.ResidentBatch(poa.graph, mq, mo)
    mb.run(COSTS)
    m_res = mb.fetch()
    elem = 2 if "u16" in mb.layout() else 4
    rws = int(poa.graph.n)
    out["mixed_lengths"] = {"queries": "63 x 1 000 bases + 1 x 10 000 bases", "cell_bytes": elem, "results_equal": same(m_res, m_one),
                            "one_shot_plane_bytes_per_query": 5 * rws * max(pitch) * elem,
                            "resident_plane_bytes_of_a_1kbp_query": 5 * rws * pitch[0] * elem,
                            "resident_plane_bytes_of_the_10kbp_query": 5 * rws * pitch[-1] * elem,
                            "one_shot_plane_bytes_total": 5 * rws * max(pitch) * elem * len(qs),
                            "resident_plane_bytes_total": 5 * rws * sum(pitch) * elem,
                            "resident_workspace_bytes_held": mb.workspace_bytes()}
    mb.close()
    rb = aligner.ResidentBatch(g, qseq, qoff)
    one = al.align_batch(g, qseq=qseq, qoff=qoff)   # warm-up of both paths, and the comparison
    rb.run(COSTS)
    res = rb.fetch()
    out["results_equal"] = same(res, one)
    out["layout"] = sorted(rb.layout())
    rows = {"one_shot": [], "resident": []}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        one = al.align_batch(g, qseq=qseq, qoff=qoff)
        rows["one_shot"].append((one.stats["ms_forward"] + one.stats["ms_traceback"], (time.perf_counter() - t0) * 1e3, one.stats["n_chunks"]))
        t0 = time.perf_counter()
        rb.run(COSTS)
        res = rb.fetch()
        rows["resident"].append((res.stats["ms_forward"] + res.stats["ms_traceback"], (time.perf_counter() - t0) * 1e3, res.stats["n_chunks"]))
    for k, v in rows.items():
        out[k] = {"ms_kernels": spread([r[0] for r in v]), "ms_step_wall": spread([r[1] for r in v]), "chunks": v[0][2]}
    out["resident"]["workspace_bytes"] = rb.workspace_bytes()
    ks = out["one_shot"]["ms_kernels"]
    out["kernel_time"] = {"one_shot_spread_ms": round(ks["max"] - ks["min"], 3),
                          "resident_median_minus_one_shot_median_ms": round(out["resident"]["ms_kernels"]["median"] - ks["median"], 3)}
    out["kernel_time"]["within_one_shot_spread"] = out["kernel_time"]["resident_median_minus_one_shot_median_ms"] <= out["kernel_time"]["one_shot_spread_ms"]
    # two batches in flight: the walk and the fetch of one step under the forward pass of the next
    rb2 = aligner.ResidentBatch(g, qseq, qoff)
    batches, streams = [rb, rb2], [torch.cuda.Stream(), torch.cuda.Stream()]
    for k in range(2):
        batches[k].run(COSTS, streams[k].cuda_stream)
    for k in range(2):
        batches[k].fetch()
    t0 = time.perf_counter()
    for k in range(args.steps):
        b = batches[k % 2]
        if k >= 2:
            b.fetch()
        b.run(COSTS, streams[k % 2].cuda_stream)
    last = [batches[k].fetch() for k in range(2)]
    out["two_in_flight"] = {"steps": args.steps, "ms_per_step": round((time.perf_counter() - t0) * 1e3 / args.steps, 3),
                            "results_equal": all(same(r, one) for r in last)}
    rb.close()
    rb2.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if (out["results_equal"] and out["two_in_flight"]["results_equal"] and out["mixed_lengths"]["results_equal"]) else 1


if __name__ == "__main__":
    sys.exit(main())
