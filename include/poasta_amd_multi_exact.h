/* poasta_amd_multi_exact.h — exact multi-graph batches: the part of the C ABI of include/poasta_amd.h that replays the
 * reference's search for the queries of many graphs in one launch.  poasta_amd.h includes this file at its end, so a caller of
 * that header has these declarations; including this file alone gives the whole ABI as well.  Same library, same conventions. */
#ifndef POASTA_AMD_MULTI_EXACT_H
#define POASTA_AMD_MULTI_EXACT_H
#include "poasta_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A poa_multi_t of a fourth kind, beside the checkpointed batches and the dense one: the dense batch of poa_multi_create_dense
 * with the replay of the reference's best-first search behind every chunk's dense pass.  A run is per chunk the dense kind's
 * forward and walk launches unchanged, the INF-fill of the replayed queries' u32 visited tables (every query in
 * POA_MODE_EXACT, the queries with non-zero dense flags in POA_MODE_HYBRID), ONE replay launch (one wavefront per query, each
 * on the tables of its own graph), ONE u32 walk launch over the replayed tables, then the scan and compaction of the pairs.
 * One-piece model, Global.
 *
 * Contract.  Per query: score, pairs, pair_off, flags and the four search-counter words are those of poa_align_batch_ex for that
 * query's graph alone under the same cfg (mode EXACT or HYBRID, heuristic, pruning), bit for bit.  A NULL cfg is POA_MODE_EXACT
 * with the min-gap heuristic and pruning.  The one exception is POA_FLAG_EXACT_OVERFLOW: the replay workspace of a slot (reached
 * sets, DFA stack, queue pool, descriptor ring) has ONE size for the whole batch, the maxima over the graphs that have queries of
 * what the single-graph call sizes for its own graph — so a query may overflow its queue pool here at a smaller or larger
 * queue_entries_per_cell than in its single-graph call.  Results are identical wherever neither call overflows; a query that
 * overflows keeps its dense result and gets the flag, as there.  Queries of a graph without real nodes keep the dense result
 * (POA_FLAG_EMPTY_GRAPH) and counter words 0, as do the queries a hybrid run does not replay.
 *
 * The argument lists are those of the poa_multi_*_dense namesakes; poa_multi_fetch / _stats / _device_results /
 * _workspace_bytes / _destroy serve the batch unchanged (poa_stats_t: ms_exact is the fill, replay and u32 walk, n_exact the
 * queries whose replay succeeded).
 *
 * Footprint.  Per query poa_graph_compact_elems(graph, len) two-byte elements + 256 bytes (the dense region) and
 * 3 x rows(graph) x pitch four-byte cells + 256 bytes (the visited table), pitch = len + 1 rounded up to 64;
 * largest_query_bytes is the largest such sum.  Chunks are cut greedily in query order under workspace_bytes by that sum.
 * poa_multi_footprint_exact returns in `bytes` the sum over all queries PLUS the replay workspace of as many slots as the
 * largest chunk has queries (all of them without a cap), sized for cfg's queue_entries_per_cell and a descriptor ring of 64
 * priorities.  Per slot: n_exit x (wpn + swpn) x 8 bytes of reached sets (n_exit the largest exit count of a graph, wpn the
 * 64-bit words of the longest query, swpn = wpn / 64 rounded up; both products rounded up to even), stack_cap x 12 (largest
 * rows + longest query + 8), pool x 16 (max(256, queue_entries_per_cell x rows x (longest query + 1)) + 64 x (3 x win + 8)
 * entries, rounded up to 64) and 3 x win x 4 bytes of ring.  Costs under which the ring is wider (win = the power of two at or
 * above max(mismatch, open + extend) + open + (spread + 3) x extend + 8, spread = the largest dist_max - dist_min of a row) grow
 * the slot at the run that uses them.  Host only, no device needed.
 *
 * POA_ERR_UNSUPPORTED, each naming the single-graph call that takes the case: a mode other than EXACT / HYBRID,
 * POA_SPAN_ENDS_FREE, a query of more than 1023 symbols unless cfg->flags has POA_CFG_WIDE_QUERIES (read by the footprint,
 * create and one-shot calls as poasta_amd_multi_dense.h describes; the dense pass then walks such a query strip by strip, the
 * replay and the u32 walk are sized by the plan as before), the replay's own size limits checked per graph (priority range, visited
 * table, reached sets, queue pool); at poa_multi_run_exact costs under which some graph needs u32 dense cells or
 * tune[POA_TUNE_PLANES] = 32, tune[POA_TUNE_EXACT_IMPL] other than 0 / 2 (wave) and tune[POA_TUNE_WS_GROUP] other than 64.  The
 * two-piece model has no such batch.  POA_TUNE_EXACT_LDS = 0 and POA_TUNE_WS_RING_GLOBAL force the generic-pointer replay kernel;
 * POA_TUNE_WS_LANES, _ADAPT, _CHUNK_CAP and _REC apply as in the single-graph replay.
 * POA_ERR_INVALID_ARG: the argument errors of poa_multi_create; an unknown heuristic; the other kinds' run calls on this batch and
 * poa_multi_run_exact on a batch of another kind; a fetch before a run.
 * poa_multi_run_exact launches on `stream` without synchronising; it allocates only when the costs need a larger slot than any
 * run before (it then waits for the previous run).  It may be called again with other costs and with the other mode.
 * poa_multi_last_launch serves the batch: the dense kind's record with the replay kernel in out[2] (1: graph, records and ring
 * in LDS; 2: generic pointers) in its low two bits, POA_LAUNCH_STRIPS on top for a chunk that ran the strip loop. */
int poa_multi_footprint_exact(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                              const uint64_t* qoff, const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes);
int poa_multi_create_exact(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device,
                           const uint8_t* qseq, const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes,
                           poa_multi_t** out);
int poa_multi_run_exact(poa_multi_t* m, const poa_costs_t* costs, const poa_config_t* cfg, void* stream);
/* out[4 * n_queries]: num_queued, num_visited, num_pruned, steps of every query of the last run, in the format of
 * poa_batch_fetch_search_counters; zeros for a query that was not replayed.  Waits for the run. */
int poa_multi_fetch_search_counters(poa_multi_t* m, uint32_t* out);
/* what the replay launched for chunk `chunk` of the last poa_multi_run_exact, in the record format of poa_batch_replay_info
 * (poasta_amd.h): POA_REPLAY_WAVE_LDS or POA_REPLAY_WAVE_GENERIC, the slot's `win`, 64 lanes per query, one wave per block, the
 * POA_REPLAY_BIT_* bits, 0, the chunk's queries as blocks, the dynamic LDS bytes.  Host side only. */
int poa_multi_replay_info(poa_multi_t* m, uint32_t chunk, uint32_t out[8]);
/* one-shot: create, run, fetch, destroy */
int poa_align_multi_exact(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                          const poa_costs_t* costs, const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff,
                          uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity, uint32_t* flags,
                          poa_stats_t* stats, int device);

#ifdef __cplusplus
}
#endif
#endif /* POASTA_AMD_MULTI_EXACT_H */
