#!/usr/bin/env python3
"""Best-of score-set runs on the workload of scripts/scoreset_cap_timing.py: does a cap that tightens on the device pay?

Workload: 256 graphs (LinearishPOA at a backbone of 190, about 212 rows) and their 32 x 256 reads of about 200 bp, fixed seeds,
costs 4 / 6 / 2; every read against its own graph and 7 others, 65 536 pairs, the own graph listed first.  Per step, interleaved
in one process:
  (a) poa_scoreset_run + poa_scoreset_fetch + the arg-min over each read's eight scores on the host;
  (b) poa_scoreset_run_capped with, per read, a cap of 1.5 times the read's score on its own graph (taken from (a): a caller
      cannot know it) + poa_scoreset_fetch + the same arg-min;
  (c) poa_scoreset_run_best, slack 0 + poa_scoreset_fetch_best;
  (d) the same on a second set whose pair list names the own graph LAST: the worst order;
  (e) (c) launched from the pair-order class lists (POA_CFG_BEST_PAIR_ORDER): what the rank order buys;
  (f) (c) with slack 0xFFFFFFFF: the policy's overhead when nothing can stop.
The first --warmup steps are dropped; medians with min / max of the rest; the step time is the host clock around the calls named
above (the fetch synchronises), the kernel time the HIP-event sum of poa_stats_t.  Per variant also the mean of swept / rows over
the losing pairs (poa_scoreset_fetch_swept) and the number of reads whose winner is their own graph.
Every measurement runs in a child process under its own time limit; a non-zero status ends the script.

--parent-lib names a build of the parent commit's library (scripts/dev/variant.sh): (a) and (b) are then also measured on it
(POA_LIB_PATH), before and after this tree's measurement, and on this tree a second time, so that the difference between the two
trees can be read against the spread of each tree's own two runs.  Writes profiles/pr_scoreset_best/timing.json.
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


def measure(args):
    import numpy as np
    from poasta_amd import _lib, aligner, workloads as W

    graphs, seqs = [], []
    for k in range(args.graphs):
        g, (qseq, qoff) = W.scaled_linearish(190, 10, 5, args.reads, args.length, graph_seed=100 + k, query_seed=5000 + k)
        graphs.append(g)
        seqs += [qseq[int(qoff[i]):int(qoff[i + 1])] for i in range(args.reads)]
    nq = len(seqs)
    # read i of graph k against graph k and the graphs k + 37 j (scripts/scoreset_timing.py): the first of a read's eight is its own
    pairs = np.array([(k * args.reads + i, (k + 37 * j) % args.graphs) for k in range(args.graphs) for i in range(args.reads)
                      for j in range(OTHERS + 1)], np.int64)
    last = pairs.reshape(nq, OTHERS + 1, 2)[:, ::-1].reshape(-1, 2)   # the own graph last
    n = len(pairs)
    rows = np.array([graphs[gi].n for gi in pairs[:, 1]], np.float64)
    costs = aligner.GapAffine(4, 2, 6)
    ss = aligner.ScoreSet(graphs, seqs, pairs=pairs)
    plain = aligner.make_config("score")

    ss.run(costs)
    score0, _, _ = ss.fetch()
    m0 = score0.reshape(nq, OTHERS + 1)
    own = m0[:, 0].astype(np.uint64)
    cap15 = np.repeat((own * 3) // 2, OTHERS + 1).astype(np.uint32)
    best0, arg0 = m0.min(axis=1), m0.argmin(axis=1)

    def host_argmin(s, cap):
        s.run(costs, cap=cap)
        score, _, st = s.fetch()
        m = score.reshape(nq, OTHERS + 1)
        return m.min(axis=1), m.argmin(axis=1), st["ms_forward"]

    def best_of(s, slack=0, cfg=None):
        s.run(costs, config=cfg, best=True, slack=slack)
        b = s.fetch_best()
        return b["score"], b["pair"] % (OTHERS + 1), s.stats()["ms_forward"]

    variants = {"a_uncapped_host_argmin": lambda: host_argmin(ss, None), "b_capped_1.5x_own_host_argmin": lambda: host_argmin(ss, cap15)}
    winner_own = {"a_uncapped_host_argmin": 0, "b_capped_1.5x_own_host_argmin": 0}
    if not args.parent_variants_only:
        ss_last = aligner.ScoreSet(graphs, seqs, pairs=last)
        pair_order = aligner.make_config("score")
        pair_order.flags |= _lib.CFG_BEST_PAIR_ORDER
        variants.update({"c_best_slack_0": lambda: best_of(ss), "d_best_own_graph_last": lambda: best_of(ss_last),
                         "e_best_pair_order_lists": lambda: best_of(ss, cfg=pair_order), "f_best_slack_none": lambda: best_of(ss, NONE, plain)})
        winner_own.update({"c_best_slack_0": 0, "d_best_own_graph_last": OTHERS, "e_best_pair_order_lists": 0, "f_best_slack_none": 0})
    times = {k: [] for k in variants}
    info = {}
    for rep in range(args.warmup + args.steps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            best, arg, fwd = fn()
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                times[name].append((wall, fwd))
            if rep == 0:
                s = ss_last if name.startswith("d_") else ss
                rank_own = winner_own[name]
                swept = s.swept_rows().astype(np.float64).reshape(nq, OTHERS + 1)
                r = (rows.reshape(nq, OTHERS + 1)[:, ::-1] if name.startswith("d_") else rows.reshape(nq, OTHERS + 1))
                losing = np.ones((nq, OTHERS + 1), bool)
                losing[np.arange(nq), arg] = False
                want_arg = OTHERS - arg0 if name.startswith("d_") else arg0
                # ((d) reverses each read's list: among equal scores its lowest index is another pair, so only the score is compared
                # where a read's best score is attained twice)
                tied = (m0 == best0[:, None]).sum(axis=1) > 1
                info[name] = {"results_as_expected": bool(np.array_equal(best, best0) and np.array_equal(arg[~tied], want_arg[~tied])),
                              "best_score_crc32": zlib.crc32(np.ascontiguousarray(best).tobytes()),
                              "winner_is_own_graph": int((arg == rank_own).sum()),
                              "mean_swept_over_rows_losing_pairs": round(float((swept[losing] / r[losing]).mean()), 4),
                              "pairs_stopped_early": int((swept < r).sum())}

    def med(v):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

    out = {"library": "the parent commit's build (--parent-lib)" if os.environ.get("POA_LIB_PATH") else "this tree", "pairs": n, "graphs": args.graphs,
           "queries": nq, "steps": args.steps, "warmup": args.warmup, "uncapped_score_crc32": zlib.crc32(score0.tobytes()), "variants": {}}
    for name in variants:
        out["variants"][name] = {"ms_step": med([r[0] for r in times[name]]), "ms_forward_kernels": med([r[1] for r in times[name]]),
                                 "ms_step_all": [round(r[0], 3) for r in times[name]]}
        out["variants"][name].update(info[name])
    base = out["variants"]["a_uncapped_host_argmin"]
    for name in variants:
        v = out["variants"][name]
        v["ms_step_over_a"] = round(v["ms_step"]["median"] / base["ms_step"]["median"], 4)
        v["ms_kernels_over_a"] = round(v["ms_forward_kernels"]["median"] / base["ms_forward_kernels"]["median"], 4)
    ss.close()
    print(json.dumps(out))
    return 0 if all(v["results_as_expected"] for v in out["variants"].values()) else 1


def child(args, lib=None, parent_variants_only=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--measure"] + [a for k in ("graphs", "reads", "length", "steps", "warmup")
                                                                      for a in ("--" + k, str(getattr(args, k)))]
    if parent_variants_only:
        cmd.append("--parent-variants-only")
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
    ap.add_argument("--parent-variants-only", action="store_true", help="(a) and (b) only: what the parent commit's library has")
    ap.add_argument("--parent-lib", default=None, help="libpoasta_amd.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_scoreset_best", "timing.json"))
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    out = {"workload": "%d graphs x %d reads of %d bp, LinearishPOA backbone 190; every read against its own graph (listed first) and %d others"
                       % (args.graphs, args.reads, args.length, OTHERS), "costs": "4 / 6 / 2 (mismatch / open / extend)"}
    if args.parent_lib:
        out["parent_first"] = child(args, args.parent_lib, True)
    out["this_tree"] = child(args)
    if args.parent_lib:
        out["parent_second"] = child(args, args.parent_lib, True)
        out["this_tree_second"] = child(args, None, True)
        cmp = {}
        for name in ("a_uncapped_host_argmin", "b_capped_1.5x_own_host_argmin"):
            k = lambda d: d["variants"][name]["ms_forward_kernels"]["median"]
            w = lambda d: d["variants"][name]["ms_step"]["median"]
            p1, p2, t1, t2 = out["parent_first"], out["parent_second"], out["this_tree"], out["this_tree_second"]
            cmp[name] = {"ms_step_parent": [w(p1), w(p2)], "ms_step_this_tree": [w(t1), w(t2)], "ms_kernels_parent": [k(p1), k(p2)],
                         "ms_kernels_this_tree": [k(t1), k(t2)],
                         "parent_run_to_run_spread_kernels": round(abs(k(p1) - k(p2)) / min(k(p1), k(p2)), 4),
                         "this_tree_run_to_run_spread_kernels": round(abs(k(t1) - k(t2)) / min(k(t1), k(t2)), 4),
                         "this_tree_over_parent_kernels": round((k(t1) + k(t2)) / (k(p1) + k(p2)), 4),
                         "same_results": p1["variants"][name]["best_score_crc32"] == t1["variants"][name]["best_score_crc32"]}
        out["parent_vs_this_tree"] = cmp
    else:
        out["parent"] = "not measured (no --parent-lib)"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
