/* poasta_amd_scoreset_cap.h — capped score-set runs: the part of the C ABI of include/poasta_amd.h that gives a score set
 * (poa_scoreset_*) a score cap per pair.  poasta_amd.h includes this file at its end, so a caller of that header has these
 * declarations; including this file alone gives the whole ABI as well.  Same library, same conventions. */
#ifndef POASTA_AMD_SCORESET_CAP_H
#define POASTA_AMD_SCORESET_CAP_H
#include "poasta_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Capped runs: "above this score I do not care".  cap[n_pairs] is a host array in pair order, copied before the call returns;
 * cap[p] == POA_SCORE_UNVISITED: no cap for that pair.  With s the score the uncapped run returns for pair p:
 *     s <= cap[p]:  score[p] = s, flags[p] as uncapped
 *     s >  cap[p]:  score[p] = POA_SCORE_UNVISITED, flags[p] as uncapped | POA_FLAG_CAPPED
 * for every pair alike: one against a graph without real nodes (s = 4 * len, POA_FLAG_EMPTY_GRAPH stays), len <= 1, and the
 * two-piece run, whose cap is compared with the two-piece score.  The result is exact and does not depend on where a wave
 * stops: scores never decrease along an alignment path, so at a row that every start-to-end path passes the smallest M value
 * of the row is a lower bound on the final score; a wave whose bound is above its cap stops there and hands its slot on the
 * chip to the next pair.  Pairs of at most 1024 columns test at the check rows of their graph (poa_graph_sweep_checks;
 * tune[POA_TUNE_CAP_STRIDE] overrides the stride), wider pairs at the end of every strip but the last, on M of the strip's
 * last column.  Other arguments, errors and the launch on `stream` without synchronising are those of poa_scoreset_run /
 * _run_2piece; cap == NULL: POA_ERR_INVALID_ARG.  The set's FIRST capped run allocates what capped runs need beyond the set —
 * the caps, the swept-row counts and the check rows on the device, a pinned staging area on the host — and the set keeps them;
 * every later run, capped or not, allocates nothing.  A capped run waits on the host for the previous capped run's copy of
 * its caps (not for its kernels).  Capped and uncapped runs of either model may alternate on one set; poa_scoreset_fetch,
 * _stats and _device_results serve all of them alike (plane_bytes counts the rows of an unstopped run). */
int poa_scoreset_run_capped(poa_scoreset_t* s, const poa_costs_t* costs, const poa_config_t* cfg, const uint32_t* cap, void* stream);
int poa_scoreset_run_2piece_capped(poa_scoreset_t* s, const poa_costs2_t* costs, const poa_config_t* cfg, const uint32_t* cap,
                                   void* stream);
/* synchronises; swept[n_pairs]: the row bodies the wave of each pair of the last run executed.  A pair of at most 1024 columns
 * that ran to the end: rows(graph); one that stopped after check row r: r + 1; a wider pair: the sum over its strips; a pair
 * against a graph without real nodes: 0.  After an uncapped run: the full counts.  Before any run: POA_ERR_INVALID_ARG. */
int poa_scoreset_fetch_swept(poa_scoreset_t* s, uint32_t* swept /* [n_pairs] */);

#ifdef __cplusplus
}
#endif
#endif /* POASTA_AMD_SCORESET_CAP_H */
