/* poasta_amd_scoreset_best.h — best-of score-set runs: the part of the C ABI of include/poasta_amd.h that lets a score set
 * (poa_scoreset_*) answer its own question, "which of these graphs does this query belong to", on the device.  poasta_amd.h
 * includes this file at its end, after poasta_amd_scoreset_cap.h, so a caller of that header has these declarations; including
 * this file alone gives the whole ABI as well.  Same library, same conventions. */
#ifndef POASTA_AMD_SCORESET_BEST_H
#define POASTA_AMD_SCORESET_BEST_H
#include "poasta_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One record per query of the set's pool, 32 bytes, in query order. */
typedef struct {
    uint32_t pair;          /* the winning pair's index in the set's pair list; POA_NONE: no pair qualifies */
    uint32_t score;         /* its score; POA_SCORE_UNVISITED: none */
    uint32_t flags;         /* its flags, as the uncapped run returns them; 0: none */
    uint32_t second_score;  /* the smallest score of another pair of the query within T (below), else POA_SCORE_UNVISITED */
    uint32_t n_within;      /* the query's pairs with a score <= T, the winner included */
    uint32_t reserved[3];   /* 0 */
} poa_best_t;

/* cfg->flags of a best-of run: launch from the pair-order class lists instead of the best-of order (measurement only; the
 * results are the same, the cap bites later) */
#define POA_CFG_BEST_PAIR_ORDER 2u

/* Best-of runs.  The cap of a pair is not given by the caller: it is the best score any pair of the SAME QUERY has finished
 * with so far in this run, plus `slack`, under the query's optional ceiling limit[q] (a host array [n_queries], copied before
 * the call returns; NULL, or POA_SCORE_UNVISITED for a query: none).  With s_p the score poa_scoreset_run (or _run_2piece: the
 * two-piece score) returns for pair p, and Q(q) the pairs of query q:
 *     E(q)            = { p in Q(q) : s_p != POA_SCORE_UNVISITED and s_p <= limit[q] }
 *     best.score      = min s_p over E(q); best.pair = the smallest pair index in E(q) that attains it; best.flags = its flags.
 *                       E(q) empty (a query without pairs included): POA_NONE, POA_SCORE_UNVISITED, 0
 *     T_q             = min(best.score + slack (saturating), limit[q]); E(q) empty: limit[q]
 *     n_within        = the number of p in Q(q) with s_p <= T_q
 *     second_score    = min s_p over p in Q(q) other than best.pair with s_p <= T_q, else POA_SCORE_UNVISITED: the exact
 *                       runner-up whenever it lies within the slack
 * and per pair (poa_scoreset_fetch after such a run):
 *     s_p <= T_q:  score[p] = s_p, flags[p] as uncapped — always
 *     s_p >  T_q:  either that, or (POA_SCORE_UNVISITED, flags | POA_FLAG_CAPPED): which one depends on when the pair's wave ran
 *                  and is unspecified; a pair reported as capped always has s_p > T_q.
 * Pairs against a graph without real nodes take part with s = 4 * len and POA_FLAG_EMPTY_GRAPH, as in capped runs; so do
 * queries of len <= 1.  Everything in poa_best_t is exact and independent of scheduling: a query's running best only
 * decreases, so the cap a wave reads at any time is >= T_q and a pair with s_p <= T_q is never stopped; tied winners all
 * finish, and a 64-bit atomic min over (score << 32 | pair index) keeps the lowest index; a stale read of the running best only
 * prunes less; no wave waits for another.  Waves test where capped runs test (check rows, strip ends, the final write).
 * Launch order: within a chunk and kernel class, pairs are dispatched by (rank, pair index), a pair's rank being its position
 * among its query's pairs in pair order: list a query's most likely graph FIRST and its cap is set before the others start.
 * Chunks are stream-ordered: a later chunk sees the final bests of the earlier ones.
 * Other arguments, errors and the launch on `stream` without synchronising are those of poa_scoreset_run_capped.  The set's
 * FIRST best-of run allocates what these runs need beyond the set — the best words, limits, poa_best_t records, the
 * query-to-pairs lists and launch orders, and the buffers of capped runs if no capped run made them — and the set keeps them;
 * every later run of any kind allocates nothing.  Best-of, capped and uncapped runs of either model may alternate on one set. */
int poa_scoreset_run_best(poa_scoreset_t* s, const poa_costs_t* costs, const poa_config_t* cfg, uint32_t slack,
                          const uint32_t* limit /* [n_queries] or NULL */, void* stream);
int poa_scoreset_run_2piece_best(poa_scoreset_t* s, const poa_costs2_t* costs, const poa_config_t* cfg, uint32_t slack,
                                 const uint32_t* limit /* [n_queries] or NULL */, void* stream);
/* synchronises; best[n_queries] of the last run.  POA_ERR_INVALID_ARG unless the last run was a best-of run.
 * poa_scoreset_fetch, _fetch_swept, _stats and _device_results serve a best-of run as they serve a capped one. */
int poa_scoreset_fetch_best(poa_scoreset_t* s, poa_best_t* best /* [n_queries] */);
/* the device array of poa_best_t [n_queries] (valid once the run's stream has finished); POA_ERR_INVALID_ARG before the set's
 * first best-of run */
int poa_scoreset_device_best(poa_scoreset_t* s, void** best);
/* one-shot: create, run, fetch best and (score / flags non-NULL) the per-pair results, destroy */
int poa_score_best(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs_t* costs, const poa_config_t* cfg,
                   uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs, const uint32_t* pair_query,
                   const uint32_t* pair_graph, uint32_t slack, const uint32_t* limit, poa_best_t* best, uint32_t* score,
                   uint32_t* flags, poa_stats_t* stats, int device);
int poa_score_best_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs2_t* costs, const poa_config_t* cfg,
                          uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs,
                          const uint32_t* pair_query, const uint32_t* pair_graph, uint32_t slack, const uint32_t* limit,
                          poa_best_t* best, uint32_t* score, uint32_t* flags, poa_stats_t* stats, int device);

#ifdef __cplusplus
}
#endif
#endif /* POASTA_AMD_SCORESET_BEST_H */
