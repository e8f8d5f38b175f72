/* poasta_amd_multi_dense.h — dense multi-graph batches: the part of the C ABI of include/poasta_amd.h that runs the queries of
 * many graphs through the packed dense forward pass in one launch.  poasta_amd.h includes this file at its end, so a caller of
 * that header has these declarations; including this file alone gives the whole ABI as well.  Same library, same conventions. */
#ifndef POASTA_AMD_MULTI_DENSE_H
#define POASTA_AMD_MULTI_DENSE_H
#include "poasta_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A poa_multi_t of a third kind, beside the batches of poa_multi_create and poa_multi_create_2piece: the workspace holds every
 * query's compact u16 planes (the layout of a single-graph POA_MODE_DENSE run), and a run is per chunk ONE forward launch over
 * the queries of all graphs (the packed-u16 kernel, one wavefront per query, the four waves of a workgroup free to belong to
 * four graphs), ONE traceback launch (64 lanes per walk, speculation depth 32), then the scan and compaction of the pairs.
 * One-piece model, Global.  Score, pairs, pair_off and flags are those of poa_align_batch_ex in POA_MODE_DENSE of every query
 * against its own graph — and therefore those of poa_multi_run on the same inputs — bit for bit.
 * The argument lists are those of the poa_multi_* namesakes; poa_multi_fetch / _stats / _device_results / _workspace_bytes /
 * _destroy serve the batch unchanged.
 *
 * Footprint, per query: poa_graph_compact_elems(graph, len) two-byte elements + 256 bytes of padding, where the elements are
 * rows x pitch (M) + rows x pitch / 4 (four flag bits per cell) + kept D rows x pitch, pitch = len + 1 rounded up to 64.
 * poa_multi_footprint_dense returns the sum over all queries and its largest term, on the host, without a device.  Chunks are
 * cut greedily in query order under workspace_bytes exactly as poa_multi_create cuts them (0: the whole batch, or what free
 * memory allows; a cap below the largest query is raised to it).  A chunk whose widest query has at most 512 columns runs the
 * one-quad kernel, any other the two-quad one.
 *
 * POA_ERR_UNSUPPORTED: cfg with a mode other than POA_MODE_DENSE (NULL is dense), POA_SPAN_ENDS_FREE; a query of more than
 * 1023 symbols (wider than one strip; poa_multi_create takes any length); at poa_multi_run_dense, costs under which some graph
 * with queries needs u32 cells (gap_open x [len > 0] + gap_open x [path > 0] + gap_extend x (longest query + shortest path)
 * above 65534: the rule of poa_multi_run) or tune[POA_TUNE_PLANES] = 32 — the batch is sized for u16 cells only; the
 * checkpointed batch runs either width.  The batch stays usable after a refused run.
 * POA_ERR_INVALID_ARG: the argument errors of poa_multi_create; poa_multi_run / poa_multi_run_2piece on a dense batch and
 * poa_multi_run_dense on a checkpointed one; a fetch before a run.  poa_multi_create, poa_multi_run and poa_align_multi keep
 * refusing POA_MODE_DENSE.
 *
 * POA_CFG_WIDE_QUERIES in cfg->flags of the footprint, create and one-shot calls lifts the 1023-symbol limit (any length up to
 * 0x7FFFFFF0 symbols).  The flag belongs to the batch: poa_multi_run_dense needs nothing in its cfg.  The footprint rule is
 * unchanged.  A chunk whose widest query has at most 1024 columns launches exactly what it launches without the flag; a chunk
 * with a wider query launches poa_forward_packed_multi_wide_kernel once for all its queries: one wavefront per query walks the
 * query's strips of 1024 columns in sequence and hands 2 x rows(graph) four-byte words per such query from strip to strip
 * (the insertion-scan carry and I of the strip's last column); queries of one strip in that chunk take no carry words.  The
 * carries of one chunk must stay below 2^32 words (POA_ERR_UNSUPPORTED otherwise: cap workspace_bytes).  Results are those of
 * poa_align_batch_ex in POA_MODE_DENSE bit for bit, as for every other query.  Without the flag nothing changes.
 * poa_multi_run_dense launches on `stream` without synchronising, allocates nothing and may be called again with other costs.
 * poa_stats_t: cells = sum rows(graph_i) x (len_i + 1), plane_bytes = sum 2 x poa_graph_compact_elems, n_chunks, ms_forward
 * and ms_traceback as for every resident run. */
int poa_multi_footprint_dense(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                              const uint64_t* qoff, const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes);
int poa_multi_create_dense(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device,
                           const uint8_t* qseq, const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes,
                           poa_multi_t** out);
int poa_multi_run_dense(poa_multi_t* m, const poa_costs_t* costs, const poa_config_t* cfg, void* stream);
/* one-shot: create, run, fetch, destroy */
int poa_align_multi_dense(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                          const poa_costs_t* costs, const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff,
                          uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity, uint32_t* flags,
                          poa_stats_t* stats, int device);

/* two-byte elements the compact planes of one query of `len` symbols hold on that graph (padding not included).  Host only. */
int poa_graph_compact_elems(const poa_graph_t* g, uint32_t len, uint64_t* elems);
/* what chunk `chunk` of the last poa_multi_run_dense launched, in the record format of poa_batch_last_launch:
 * POA_KERNEL_PACKED, quads (1 or 2), 0, 4 waves per workgroup, code_fmt 0, 64 lanes per walk, depth 32, queries of the chunk.
 * A chunk that ran the strip loop (POA_CFG_WIDE_QUERIES, a query wider than 1024 columns) reports quads 2 and POA_LAUNCH_STRIPS
 * in out[2].  POA_ERR_INVALID_ARG on a checkpointed batch, before a run, and past the last chunk.  Host side only. */
int poa_multi_last_launch(poa_multi_t* m, uint32_t chunk, uint32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* POASTA_AMD_MULTI_DENSE_H */
