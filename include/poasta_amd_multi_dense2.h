/* poasta_amd_multi_dense2.h — dense two-piece multi-graph batches: the part of the C ABI of include/poasta_amd.h that runs the
 * queries of many graphs through the dense two-piece pass in one launch.  poasta_amd.h includes this file at its end, so a caller
 * of that header has these declarations; including this file alone gives the whole ABI as well.  Same library, same conventions. */
#ifndef POASTA_AMD_MULTI_DENSE2_H
#define POASTA_AMD_MULTI_DENSE2_H
#include "poasta_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A poa_multi_t of a fifth kind, beside the checkpointed batches, the dense one and the exact one: the workspace holds every
 * query's five u16 score planes (M, I1, D1, I2, D2: the layout of a single-graph dense two-piece run on u16 cells), and a run
 * is per chunk ONE forward launch over the queries of all graphs (one wavefront per query, the four waves of a workgroup free
 * to belong to four graphs), ONE walk launch over the stored planes (one lane per query, the 64 lanes of a wave free to belong
 * to 64 graphs), then the scan and compaction of the pairs.  No checkpoints, no second forward pass.
 * Two-piece model, Global, u16 cells only, queries of any length.
 *
 * Contract.  Per query: score, pairs, pair_off and flags are those of poa_align_batch_2piece for that query's graph alone — and
 * therefore those of poa_multi_run_2piece on the same inputs — bit for bit.  A query against a graph without real nodes gets
 * score 4 x len, POA_FLAG_EMPTY_GRAPH and no pairs.
 * The argument lists are those of the poa_multi_*_2piece namesakes (poa_costs2_t for the costs); poa_multi_fetch / _stats /
 * _device_results / _workspace_bytes / _destroy serve the batch unchanged.
 *
 * Footprint, per query: 5 x rows(graph) x pitch two-byte elements + 256 bytes of padding, pitch = len + 1 rounded up to 64: ten
 * bytes per cell of pitch.  poa_multi_footprint_dense_2piece returns the sum over all queries and its largest term, on the
 * host, without a device.  Chunks are cut greedily in query order under workspace_bytes exactly as poa_multi_create cuts them
 * (0: the whole batch, or what free memory allows; a cap below the largest query is raised to it).  There is no length limit
 * and there are no strip carries: a row of up to 1024 columns keeps its predecessor in registers, a wider one reads it back
 * from the planes.  POA_CFG_WIDE_QUERIES is not read.
 *
 * POA_ERR_UNSUPPORTED: cfg with a mode other than POA_MODE_DENSE (NULL is dense); POA_SPAN_ENDS_FREE; at
 * poa_multi_run_dense_2piece, costs under which some graph with queries needs u32 cells (gap_open1 x [len > 0] + gap_open1 x
 * [path > 0] + gap_extend1 x (longest query + shortest path) above 65534: the rule of poa_multi_run_2piece),
 * costs->wide_planes, or tune[POA_TUNE_PLANES] = 32 — the batch is sized for u16 cells only, and the message names
 * poa_multi_create_2piece, the batch that runs either width.  The batch stays usable after a refused run.
 * POA_ERR_INVALID_ARG: the argument errors of poa_multi_create; gap_extend1 < gap_extend2; a fetch before a run; poa_multi_run /
 * _run_2piece / _run_dense / _run_exact on this batch and poa_multi_run_dense_2piece on a batch of any other kind;
 * poa_multi_last_launch and poa_multi_replay_info on this batch.  poa_multi_create_dense and poa_multi_run_dense stay one-piece.
 *
 * poa_multi_run_dense_2piece launches on `stream` without synchronising, allocates nothing and may be called again with other
 * costs.  poa_stats_t: cells = sum rows(graph_i) x (len_i + 1), plane_bytes = sum 2 x 5 x rows(graph_i) x pitch_i, n_chunks,
 * ms_forward and ms_traceback as for every resident run.
 * Open: u32 cells; a group or speculative walk over five planes; the packed-u16 mapping of the two-piece rows. */
int poa_multi_footprint_dense_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                                     const uint64_t* qoff, const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes);
int poa_multi_create_dense_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device,
                                  const uint8_t* qseq, const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes,
                                  poa_multi_t** out);
int poa_multi_run_dense_2piece(poa_multi_t* m, const poa_costs2_t* costs, const poa_config_t* cfg, void* stream);
/* one-shot: create, run, fetch, destroy */
int poa_align_multi_dense_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                                 const poa_costs2_t* costs, const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff,
                                 uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                                 uint32_t* flags, poa_stats_t* stats, int device);
/* M, I1, D1, I2, D2 of one query after a run, as u32 (an unvisited u16 cell, 0xFFFF, reads 0xFFFFFFFF): rows(graph of the
 * query) x (len + 1) each, row = topological rank (poa_graph_node_rows).  Valid when the query's chunk was the last one run,
 * the rule of poa_batch_fetch_planes_2piece; POA_ERR_INVALID_ARG otherwise, before a run, and on a batch of another kind.
 * Synchronises the run's stream. */
int poa_multi_fetch_planes_2piece(poa_multi_t* m, uint32_t query, uint32_t* m_plane, uint32_t* i1, uint32_t* d1, uint32_t* i2,
                                  uint32_t* d2);

#ifdef __cplusplus
}
#endif
#endif /* POASTA_AMD_MULTI_DENSE2_H */
