/* poasta_amd — C ABI of the MI355X (gfx950) gap-affine POA alignment engine.
 *
 * Drop-in boundary: everything behind `poasta::aligner::PoastaAligner::{align,
 * align_with_existing_bubbles, align_no_pruning}` (/root/reference/src/aligner/mod.rs:69-145),
 * i.e. `astar_alignment` (src/aligner/astar.rs:108-226) + the score-based backtrace
 * (src/aligner/scoring/gap_affine.rs:550-657, :804-915), for the gap-affine cost model
 * (`GapAffine`, gap_affine.rs:20-30) in Global mode with query offsets of type u32
 * (the only instantiation the reference binaries use: src/bin/poasta.rs:214, src/bin/lasagna.rs:125).
 *
 * The host keeps the graph (`POAGraph`), builds it, mutates it and does all I/O.  It hands the
 * library a flattened view of the `AlignableRefGraph` trait (src/graphs/mod.rs:23-53) and a batch of
 * queries (the `lasagna align` shape, src/bin/lasagna.rs:184-276: N reads x 1 immutable graph).
 *
 * Plain C: pointers and sizes only.  All functions return POA_OK (0) or a negative POA_ERR_* code;
 * nothing aborts or throws across this boundary.  INTEGRATION.md shows the Rust `extern "C"` block
 * and the ~30-line shim inside `PoastaAligner::align_internal`.
 */
#ifndef POASTA_AMD_H
#define POASTA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POA_NONE 0xFFFFFFFFu /* AlignedPair{rpos|qpos: None} (src/aligner/alignment.rs:4-13) */
#define POA_SCORE_UNVISITED 0xFFFFFFFFu /* Score::Unvisited (src/aligner/scoring/mod.rs:64-70) */

/* return codes */
#define POA_OK 0
#define POA_ERR_INVALID_ARG (-1)
#define POA_ERR_NOT_A_DAG (-2)      /* cycle, unreachable node, start with predecessors, end with successors */
#define POA_ERR_NO_DEVICE (-3)      /* no usable gfx950 device: the HIP path never falls back to the CPU */
#define POA_ERR_HIP (-4)            /* a HIP runtime call failed; see poa_last_error() */
#define POA_ERR_CAPACITY (-5)       /* pair_capacity too small; pair_off[n] holds the needed total */
#define POA_ERR_OUT_OF_MEMORY (-6)
#define POA_ERR_UNSUPPORTED (-7)

/* per-query flags (poa_align_batch `flags`).
 * Scores are exact whenever START_QUIRK and SHORT_QUERY are clear.  The alignment is the
 * reference's, bit for bit, whenever the word is 0: the optimal alignment is then unique in the
 * reference's own alignment graph, so every search order yields it. */
#define POA_FLAG_AMBIGUOUS 0x01u    /* >1 co-optimal alignment: the reference's pick depends on its search order */
#define POA_FLAG_START_QUIRK 0x02u  /* path uses an edge the reference's offset-0 special case may hide (dfa.rs:146-167) */
#define POA_FLAG_REF_PANIC 0x04u    /* the reference would panic on this input (u32 wrap in mod.rs:144-152) */
#define POA_FLAG_SHORT_QUERY 0x08u  /* len <= 1: reference special cases (gap_affine.rs:808-824) */
#define POA_FLAG_TRUNCATED 0x10u    /* backtrace ended before the start node (as the reference's would) */
#define POA_FLAG_EMPTY_GRAPH 0x20u  /* no real nodes: PoastaAligner::align shortcut (mod.rs:124-142), score 4*len */
#define POA_FLAG_EXACT_OVERFLOW 0x40u /* exact replay ran out of workspace: the dense result (and its flags) was kept.  For a POA_SPAN_ENDS_FREE
                                       * run that result is the GLOBAL alignment of the dense pass, not an answer to the span asked for: treat the
                                       * query as not aligned and run it again with a larger queue_entries_per_cell.  The descriptor ring is sized
                                       * to hold every priority that is live at once (a free graph begin included), so only the queue pool sets it. */
#define POA_FLAG_CAPPED 0x80u       /* capped score-set run: the score is above the pair's cap and was not returned */

/* modes (poa_config_t.mode) */
#define POA_MODE_DENSE 0u   /* dense planes + traceback: scores exact, alignment certified-or-flagged */
#define POA_MODE_EXACT 1u   /* dense pass, then a replay of the reference's own A* search (same pop order, greedy
                               extension and pruning) for EVERY query: alignments bit-identical incl. tie-breaks */
#define POA_MODE_HYBRID 2u  /* dense pass, then the exact replay only for queries whose dense flags are non-zero */
#define POA_MODE_SCORE 3u   /* forward sweep only: score[] as in dense mode, no alignment.  Only the rows some later row still
                               reads are kept (poa_graph_sweep_slots), so a query needs n_slots x pitch cells of M and D instead
                               of rows x pitch.  pairs may be NULL and pair_capacity 0; pair_off[0..n] is all zero.  flags[i]
                               carries only the bits dense mode derives from the input alone, POA_FLAG_EMPTY_GRAPH and
                               POA_FLAG_SHORT_QUERY; the path-dependent bits (AMBIGUOUS, START_QUIRK, TRUNCATED, REF_PANIC)
                               are not evaluated and stay clear.  Global only: with POA_SPAN_ENDS_FREE every entry point
                               returns POA_ERR_UNSUPPORTED.  heuristic and pruning are ignored.  A resident batch must be
                               created for it (poa_batch_create_ex) and runs in no other mode. */
#define POA_MODE_CHECKPOINT 4u /* dense mode's results — score[], pairs, pair_off, flags, bit for bit — from a slot-sized workspace:
                               the rows are cut into segments (poa_graph_checkpoint_plan); a forward sweep keeps, besides its live
                               rows, a snapshot of the rows each later segment still reads, and a second pass recomputes one segment
                               at a time into a window and walks the traceback through it, last segment first.  A query holds
                               rows_per_query x pitch cells instead of 3 x rows x pitch, at the price of a second forward pass.
                               One-piece model, Global only: POA_SPAN_ENDS_FREE and poa_align_batch_2piece_ex return
                               POA_ERR_UNSUPPORTED, as does poa_batch_fetch_planes.  heuristic and pruning are ignored.  A resident
                               batch must be created for it (poa_batch_create_ex) and runs in no other mode. */
#define POA_MODE_CHECKPOINT2 5u /* the same for the two-piece model: poa_align_batch_2piece's score[], pairs, pair_off and flags, bit
                               for bit, from a slot-sized workspace (poa_graph_checkpoint_plan2: M, D1 and D2 in slots and snapshots,
                               five planes in the window).  A mode of its own because a batch's footprint is fixed when it is
                               created, before any costs are seen.  Two-piece entry points only (poa_align_batch_2piece_ex,
                               poa_batch_run_2piece on a batch created for it): the one-piece entry points return
                               POA_ERR_UNSUPPORTED.  Global only (POA_SPAN_ENDS_FREE: POA_ERR_UNSUPPORTED); heuristic and pruning
                               are ignored. */
#define POA_HEURISTIC_DIJKSTRA 0u /* AffineDijkstra   (src/aligner/config.rs:49)  */
#define POA_HEURISTIC_MINGAP 1u   /* AffineMinGapCost (src/aligner/config.rs:104), the default of both reference CLIs */

/* GapAffine (gap_affine.rs:20-24).  NB the Rust constructor order is (mismatch, extend, open). */
typedef struct poa_costs {
    uint8_t mismatch;
    uint8_t gap_open;
    uint8_t gap_extend;
    uint8_t reserved;
} poa_costs_t;

/* GapAffine2Piece (src/aligner/scoring/gap_affine_2piece.rs:19-33; the reference's constructor order is (mismatch, extend1,
 * open1, extend2, open2) and it asserts extend1 >= extend2).  A gap opens in the first piece (open1 + extend1) and may move to
 * the second at extend2 per step; open2 enters only the reference's heuristic / pruning arithmetic, never the DP
 * (gap_affine_2piece.rs:362-368, :402-408), so the dense pass does not read it. */
typedef struct poa_costs2 {
    uint8_t mismatch;
    uint8_t gap_open1;
    uint8_t gap_extend1;
    uint8_t gap_open2;
    uint8_t gap_extend2;
    uint8_t wide_planes;      /* 1: u32 planes whatever the bound on the score allows (A/B) */
    uint8_t reserved[2];
} poa_costs2_t;

/* Which reference configuration the exact replay emulates (only the replay depends on it: heuristic and pruning
 * fix the reference's search order, not its optimum).  Zero-initialised == dense mode. */
/* std::ops::Bound<usize> of AlignmentType::EndsFree (scoring/mod.rs:50-62) */
typedef struct poa_bound {
    uint32_t kind;            /* POA_BOUND_* */
    uint32_t value;
} poa_bound_t;
#define POA_BOUND_UNBOUNDED 0u
#define POA_BOUND_INCLUDED 1u
#define POA_BOUND_EXCLUDED 2u
#define POA_SPAN_GLOBAL 0u    /* AlignmentType::Global */
#define POA_SPAN_ENDS_FREE 1u /* AlignmentType::EndsFree{..}: what the reference returns is defined by its SEARCH
                                 (initial states gap_affine.rs:136-183, is_end :185-248: with unbounded ends the first
                                 popped Match state past offset 0 ends it), so the engine replays that search for every
                                 query whatever `mode` says; POA_FLAG_TRUNCATED then only says that the alignment does
                                 not begin at the start node */

/* Overrides of the choices the engine makes per call (plane layout, forward / traceback / replay kernel and their shapes) — for
 * A/B measurements and for the tests that run every parity case under every variant.  poa_config_t.tune[k] == 0: the engine
 * decides; else the entry holds (value + 1).  The library reads no environment variable: the Python binding fills this block from
 * POA_<NAME> variables (poasta_amd/_lib.py: tune_from_env), a host that wants a variant for one call sets it in that call's config. */
enum {
    POA_TUNE_PLANES = 0,      /* 32: u32 planes */
    POA_TUNE_COMPACT,         /* 0: three planes instead of the compact layout */
    POA_TUNE_PACKED,          /* 0: scalar-arithmetic forward kernel */
    POA_TUNE_RELATIVE,        /* 0 / 1: relative encoding off / on */
    POA_TUNE_PX,              /* 0: adjacent-pairs packed kernel instead of pairs-across-quads */
    POA_TUNE_MF,              /* 0 / 1 / 2: at most that many flag pairs beside the score; 3: one pair, the other derived */
    POA_TUNE_MW,              /* 0: no multi-wave pipeline */
    POA_TUNE_PXMW,            /* 0 / 1: 1024-column multi-wave kernel off / on */
    POA_TUNE_FWD_QUADS,
    POA_TUNE_FUSE_TB,
    POA_TUNE_TB_GROUP,        /* lanes per traceback walk: 8 / 16 / 32 / 64 */
    POA_TUNE_TB_DEPTH,        /* speculative steps per round trip */
    POA_TUNE_EXACT_IMPL,      /* replay kernel: 1 one search per lane, 2 wave per query (default), 3 flat parallel steps */
    POA_TUNE_EXACT_LANES,
    POA_TUNE_EXACT_LDS,       /* 0: graph tables read from global memory */
    POA_TUNE_WS_LANES,
    POA_TUNE_WS_GROUP,
    POA_TUNE_WS_WAVES,
    POA_TUNE_WS_RING_GLOBAL,
    POA_TUNE_WS_STATIC,
    POA_TUNE_WS_CHUNK_CAP,
    POA_TUNE_WS_PROF,         /* per-phase cycle counts of the replay kernel, printed by poa_batch_stats */
    POA_TUNE_PS_LANES,
    POA_TUNE_PS_LEAN,         /* 0: flat kernel with the generic code in log mode */
    POA_TUNE_TIMING,          /* poa_align_batch: host-side timing printed to stderr */
    POA_TUNE_WS_ADAPT,        /* wave replay: entries tested in the step after an expansion (0: always WS_LANES) */
    POA_TUNE_WS_REC,          /* 0: the wave replay's one-round-trip path reads the graph arrays instead of the per-row records */
    POA_TUNE_CKPT_ROWS,       /* checkpointed mode: rows per segment (read when the batch is created; 0 / unset: the engine's choice) */
    POA_TUNE_BAND,            /* 0: the one-strip dense kernel computes every cell instead of an exact band (poa_batch_band_info) */
    POA_TUNE_BAND_DELTA,      /* banded kernel: cap of the band distance D (tests: a small cap sends every query to the full kernel) */
    POA_TUNE_BAND_PAIR,       /* banded kernel, two queries of one length per wave: 0 never, 1 whatever the chunk's count (default: from a count on, poa_batch_band_pair_info);
                               * the table is full, so the value also carries the override of the narrow tier: see POA_BAND_NARROW_SHIFT */
    POA_TUNE_CAP_STRIDE,      /* capped score-set run: least distance in rows between two check rows (default: poa_graph_sweep_checks) */
    POA_TUNE_COUNT = 32
};

typedef struct poa_config {
    uint32_t mode;            /* POA_MODE_* */
    uint32_t heuristic;       /* POA_HEURISTIC_* (replay only) */
    uint32_t pruning;         /* 1: align / align_with_existing_bubbles; 0: align_no_pruning (mod.rs:81-90) */
    float queue_entries_per_cell; /* replay queue pool, entries per (row x column) cell; 0 = default 0.25 */
    uint32_t flags;           /* POA_CFG_* */
    uint32_t span;            /* POA_SPAN_* ; the four bounds are read only for POA_SPAN_ENDS_FREE */
    poa_bound_t qry_free_begin;   /* carried, never read by the reference's 1-piece path (gap_affine.rs:146) */
    poa_bound_t qry_free_end;
    poa_bound_t graph_free_begin;
    poa_bound_t graph_free_end;
    uint32_t tune[POA_TUNE_COUNT]; /* overrides of the engine's own choices, read once per call; see POA_TUNE_* */
} poa_config_t;
#define POA_CFG_FULL_PLANES 1u /* keep all three score planes in memory (needed by poa_batch_fetch_planes); the default
                                  u16 layout stores M, a 4-bit code per cell instead of I, and only the D rows read back */
#define POA_CFG_WIDE_QUERIES 2u /* a dense or exact multi-graph batch takes queries of more than 1023 symbols: the forward pass
                                  walks such a query strip by strip (poasta_amd_multi_dense.h).  Read by poa_multi_footprint_dense /
                                  _create_dense / poa_align_multi_dense and their _exact namesakes, by no other entry point
                                  (POA_CFG_BEST_PAIR_ORDER shares the value: the score-set calls that read it never read this one) */

/* AlignedPair (alignment.rs:4-13): rpos = node index of the host graph, qpos = 0-based query position */
typedef struct poa_aln_pair {
    uint32_t rpos;
    uint32_t qpos;
} poa_aln_pair_t;

/* Counters returned per call — the analogue of AstarResult::{num_queued,num_visited,num_pruned}
 * (astar.rs:86-89) for a dense pass, plus HIP-event timings taken on the launch stream. */
typedef struct poa_stats {
    uint64_t cells;            /* sum over queries of rows * (len + 1) */
    uint64_t bases;            /* sum of query lengths */
    uint64_t plane_bytes;      /* bytes of M/I/D score planes written */
    uint32_t n_queries;
    uint32_t n_chunks;         /* query chunks processed (workspace reuse) */
    uint32_t n_forward_launches;
    uint32_t n_flagged;        /* queries with flags != 0 */
    float ms_forward;          /* sum of forward-kernel durations (HIP events) */
    float ms_traceback;        /* sum of traceback + compaction kernel durations */
    float ms_h2d;              /* query upload (poa_align_batch only) */
    float ms_d2h;              /* result download (poa_align_batch / poa_batch_fetch) */
    float ms_exact;            /* exact-replay search kernels (+ their traceback), 0 in dense mode */
    uint32_t n_exact;          /* queries whose result came from the exact replay (last run) */
    float ms_total;            /* first launch -> last kernel end, summed over runs */
    uint32_t n_runs;           /* poa_batch_run calls covered by the ms_* sums */
} poa_stats_t;

typedef struct poa_graph poa_graph_t;
typedef struct poa_batch poa_batch_t;

/* Threading: a poa_graph_t is immutable after poa_graph_create and may be shared by batches on several threads (its bubble
 * index, needed by exact / hybrid runs only, is built once under a lock).  A poa_batch_t belongs to one thread at a time.
 * poa_align_batch* are re-entrant on distinct output buffers.  poa_last_error() is thread-local. */

/* ---- library --------------------------------------------------------------------------- */
const char* poa_version(void);
const char* poa_last_error(void);     /* thread-local description of the last failure */
int poa_device_count(void);           /* number of visible HIP devices (0 if none) */

/* ---- graph: the flattened AlignableRefGraph --------------------------------------------- */
/* Built once per graph by iterating the trait in the host (graphs/mod.rs:23-53):
 *   n          node_count_with_start_and_end()
 *   start,end  start_node(), end_node()
 *   symbol[n]  get_symbol_char() as u8 ('#' start, '$' end: graphs/poa.rs:102-103)
 *   succ_off[n+1], succ[]   successors(v) in ITERATION ORDER
 *   pred_off[n+1], pred[]   predecessors(v) in ITERATION ORDER (decides traceback ties,
 *                           gap_affine.rs:591,:617,:627)
 * The end node equals every query symbol (POAGraph::is_symbol_equal, graphs/poa.rs:463-465).
 * The library copies everything; the caller keeps ownership of its arrays. */
int poa_graph_create(uint32_t n, uint32_t start, uint32_t end, const uint8_t* symbol,
                     const uint32_t* succ_off, const uint32_t* succ,
                     const uint32_t* pred_off, const uint32_t* pred, poa_graph_t** out);
void poa_graph_destroy(poa_graph_t* g);
/* Refresh a graph handle after the host graph changed (POAGraph::add_alignment_with_weights + post_process,
 * src/graphs/poa.rs:171-363: nodes appended, edges added, start / end edges re-wired): same arguments as poa_graph_create, the
 * handle stays the same object.  The row tables are re-flattened in place (O(N + E) on the host — microseconds at the sizes of a
 * sequential POA build, under 1 % of a read's alignment call: scripts/sequential_poa_latency.sh); batches created from the
 * handle before the call keep the tables they copied and must not be run again. */
int poa_graph_update(poa_graph_t* g, uint32_t n_nodes_with_start_end, uint32_t start, uint32_t end, const uint8_t* symbol,
                     const uint32_t* succ_off, const uint32_t* succ, const uint32_t* pred_off, const uint32_t* pred);

uint32_t poa_graph_rows(const poa_graph_t* g);           /* == n */
/* slots of the score-only sweep: slot[n] by ROW (POA_NONE: the row is never read back); *n_slots = rows alive at once.
 * A row has a slot iff some successor is not the chain row directly below it; it is live from its own row to its last
 * reader.  Host-side table, recomputed by poa_graph_update; needs no device. */
int poa_graph_sweep_slots(const poa_graph_t* g, uint32_t* slot /* may be NULL */, uint32_t* n_slots);
/* check rows of a capped score-set run (poa_scoreset_run_capped): check[n] by ROW, 1 where a wave compares the row's smallest M
 * value with its cap; *n_checks = how many.  Row r is a CUT row if no edge (u, v) has row(u) < r < row(v): every start-to-end
 * path passes through it, and once it has run no earlier row is live in the sweep.  Row 0 and the end row are cut rows.  The
 * check rows are the cut rows without the end row (the result is written there anyway), thinned greedily in row order so that
 * two consecutive check rows are at least `stride` rows apart; stride 0: the engine's default, 8.  Host-side table, recomputed
 * by poa_graph_update; needs no device. */
int poa_graph_sweep_checks(const poa_graph_t* g, uint32_t stride, uint8_t* check /* [rows], may be NULL */, uint32_t* n_checks);
/* segment plan of the checkpointed mode (POA_MODE_CHECKPOINT): the rows are cut into *n_segments segments of segment_rows rows
 * (0: the engine's choice — the length that holds the fewest rows; a graph of a few rows is one segment), boundary[0] = 0 <
 * ... < boundary[*n_segments] = rows.  The snapshot of a boundary b > 0 holds every row < b that has a sweep slot and a reader
 * >= b, plus row b - 1 if row b takes it from registers in the sweep (its only predecessor).  *rows_per_query = plane rows (of
 * `pitch` cells) a query holds: 2 x n_slots (the sweep's live rows, M and D) + 2 x the snapshot rows of all boundaries + 3 x
 * the longest segment (the window: M, I, D).  Host-side table, recomputed by poa_graph_update; needs no device. */
int poa_graph_checkpoint_plan(const poa_graph_t* g, uint32_t segment_rows /* 0: engine's choice */, uint32_t* n_segments,
                              uint32_t* boundary /* may be NULL, [*n_segments + 1] */, uint32_t* rows_per_query);
/* the same plan for the two-piece model (POA_MODE_CHECKPOINT2): same contract, same boundaries rule and snapshot membership;
 * *rows_per_query = 3 x n_slots (M, D1, D2) + 3 x the snapshot rows of all boundaries + 5 x the longest segment (the window:
 * M, I1, D1, I2, D2).  segment_rows 0 is the length that minimises THIS sum (the window weighs 5 instead of 3, so it differs
 * from the one-piece choice), never more than one segment of all rows costs. */
int poa_graph_checkpoint_plan2(const poa_graph_t* g, uint32_t segment_rows /* 0: engine's choice */, uint32_t* n_segments,
                               uint32_t* boundary /* may be NULL, [*n_segments + 1] */, uint32_t* rows_per_query);
/* row (topological rank used for the score planes) of every node; rank[n] */
int poa_graph_node_rows(const poa_graph_t* g, uint32_t* rank);

/* ---- one-shot batch alignment (host buffers in, host buffers out) ------------------------ */
/* Replaces, for a batch of queries against one graph, what the reference does per query in
 * `align_sequence` (src/bin/lasagna.rs:112-138) / `perform_alignment` (src/bin/poasta.rs:214).
 *   qseq,qoff[n+1]  concatenated queries
 *   score[n]        AstarResult::score
 *   pairs, pair_off[n+1], pair_capacity   AstarResult::alignment of query i =
 *                   pairs[pair_off[i] .. pair_off[i+1]); capacity sum(len_i + n_nodes) always suffices
 *   flags[n]        POA_FLAG_* (may be NULL)
 *   stats           may be NULL
 *   device          HIP device ordinal */
int poa_align_batch(const poa_graph_t* g, const poa_costs_t* costs, uint32_t n_queries,
                    const uint8_t* qseq, const uint64_t* qoff, uint32_t* score,
                    poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                    uint32_t* flags, poa_stats_t* stats, int device);
/* same with a mode (cfg NULL == dense) */
int poa_align_batch_ex(const poa_graph_t* g, const poa_costs_t* costs, const poa_config_t* cfg, uint32_t n_queries,
                       const uint8_t* qseq, const uint64_t* qoff, uint32_t* score,
                       poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                       uint32_t* flags, poa_stats_t* stats, int device);
/* Two-piece affine model, Global, dense pass: replaces `PoastaAligner::new(Affine2PieceDijkstra(costs),
 * AlignmentType::Global).align_no_pruning(graph, seq)` per query — src/aligner/config.rs:160-213, the cost model of
 * `poasta align -g 6,24 -e 2,1` (src/bin/poasta.rs:319-445).  Same buffers as poa_align_batch.  Scores are the optimum of the
 * reference's two-piece alignment graph (what its search returns in Dijkstra order without pruning); flags == 0 certifies
 * the alignment as the one the reference's backtrace rule forces (gap_affine_2piece.rs:639-794).  Returns
 * POA_ERR_INVALID_ARG where the reference's constructor panics (extend1 < extend2).
 * Like poa_align_batch it is a resident batch created, run (poa_batch_run_2piece), fetched and destroyed inside the call.  The
 * batch is asked to hold min(60 % of the device's free memory, 64 GiB) of planes at most, and no more than the run needs: 20
 * bytes per cell of a query's pitch with u32 cells, 12 with u16 cells (the batch's three-plane 4-byte regions, of which five
 * u16 planes use 10); a larger batch runs in chunks.  The workspace is parked for the next call (poa_release_cache). */
int poa_align_batch_2piece(const poa_graph_t* g, const poa_costs2_t* costs, uint32_t n_queries,
                           const uint8_t* qseq, const uint64_t* qoff, uint32_t* score,
                           poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                           uint32_t* flags, poa_stats_t* stats, int device);
/* Two-piece model with a mode (cfg NULL or mode DENSE == poa_align_batch_2piece).  Mode EXACT (HYBRID is taken as EXACT: under
 * this model the dense certificate does not cover the cases where the reference's search is not optimal) replays the
 * reference's own search per query — replaces `PoastaAligner::new(Affine2PieceMinGapCost(costs) | Affine2PieceDijkstra(costs),
 * aln_type).align(graph, seq)` (src/aligner/config.rs:160-272, astar.rs:124-226 over scoring/gap_affine_2piece.rs: five
 * states, stacks popped M, D1, D2, I1, I2 (:1069-1097), gap_cost / heuristic (:99-127, heuristic.rs:70-102), pruning with the
 * second-piece branches of bubbles/reached.rs:84-124,:165-186, ends-free begin / end rules :179-290) — what
 * `poasta align -g 6,24 -e 2,1` runs (src/bin/poasta.rs:319-445).  cfg->heuristic / pruning / span / bounds as in
 * poa_align_batch_ex.  score[n] is the score the reference's search returns (which may exceed the dense optimum), pairs
 * its backtrace (gap_affine_2piece.rs:639-794, :944-1043); flags: POA_FLAG_REF_PANIC, POA_FLAG_TRUNCATED,
 * POA_FLAG_EXACT_OVERFLOW (queue pool: raise cfg->queue_entries_per_cell).  search_counters (may be NULL): 4 words per query —
 * num_queued, num_visited, num_pruned (AstarResult, astar.rs:228) and the queue entries that were live at once.
 * The replay runs on the same kind of batch: five u32 planes per query at the query's own pitch and, per query of a chunk, the
 * search's queue and reached sets; both together take 85 % of the device's free memory at most, a larger batch runs in chunks.
 * poa_stats_t: ms_exact is the search, ms_forward 0, n_exact the number of queries. */
/* Mode SCORE: the scores poa_align_batch_2piece returns, by the score-only sweep under the one-piece costs
 * open' = open1 + extend1 - extend2, extend' = extend2; no pairs, flags as under POA_MODE_SCORE.
 * Mode CHECKPOINT2: everything poa_align_batch_2piece returns, from a batch of the checkpointed footprint created, run,
 * fetched and destroyed inside the call. */
int poa_align_batch_2piece_ex(const poa_graph_t* g, const poa_costs2_t* costs, const poa_config_t* cfg, uint32_t n_queries,
                              const uint8_t* qseq, const uint64_t* qoff, uint32_t* score,
                              poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                              uint32_t* flags, poa_stats_t* stats, uint32_t* search_counters, int device);
/* debugging / parity: the five score planes M, I1, D1, I2, D2 of ONE query, rows x (len + 1) each, row = topological rank
 * (poa_graph_node_rows) */
int poa_planes_2piece(const poa_graph_t* g, const poa_costs2_t* costs, const uint8_t* seq, uint32_t len,
                      uint32_t* m, uint32_t* i1, uint32_t* d1, uint32_t* i2, uint32_t* d2, int device);

/* poa_align_batch and poa_align_batch_2piece (with _ex, and poa_planes_2piece) park their plane workspace (tens of GB;
 * hipMalloc/hipFree of it cost seconds) per device for the next call; this returns that memory to the driver.
 * (src/bin/lasagna.rs has no counterpart: its tables live on the heap.) */
void poa_release_cache(void);

/* ---- resident batch (queries and results stay in HBM; used by the multi-GPU driver) ------ */
/* poa_batch_create uploads graph + queries to `device` and sizes the score-plane workspace
 * (workspace_bytes = 0: pick from free memory).  poa_batch_run launches forward + traceback on
 * `stream` (a hipStream_t, NULL = default stream) and returns without synchronising.
 * poa_batch_fetch synchronises the stream and copies results to the host. */
int poa_batch_create(const poa_graph_t* g, int device, uint32_t n_queries, const uint8_t* qseq,
                     const uint64_t* qoff, uint64_t workspace_bytes, poa_batch_t** out);
/* same for a batch that will run in cfg->mode (cfg NULL or any mode but POA_MODE_SCORE == poa_batch_create).  A batch created
 * for POA_MODE_SCORE holds max(n_slots, 1) x pitch 4-byte cells of M and of D per query (+ 256 bytes of padding) instead of
 * full planes, is chunked by that footprint (a batch that fits runs as one chunk) and has no pair buffers.  Besides the slots
 * it holds, only when some query is longer than 1024 columns, the carries between strips: 16 bytes per graph row and query
 * in flight (not part of poa_batch_workspace_bytes).  The one-shot calls create and destroy such a batch per call.  Running it in
 * another mode, or a batch of poa_batch_create in POA_MODE_SCORE, returns POA_ERR_INVALID_ARG.
 * A batch created for POA_MODE_CHECKPOINT holds rows_per_query x pitch 4-byte cells per query (poa_graph_checkpoint_plan at
 * cfg->tune[POA_TUNE_CKPT_ROWS]; + 256 bytes of padding) and is chunked by that footprint; the cell width of a run follows
 * from its costs, after the batch exists, so it is sized for u32 cells and a u16 run packs twice the queries into a chunk when
 * the batch needs chunks at all.  Pair buffers as in dense mode, carries between strips as in score mode.  The same rule on
 * modes: it runs in POA_MODE_CHECKPOINT only, and no other batch runs in that mode (POA_ERR_INVALID_ARG).
 * A batch created for POA_MODE_CHECKPOINT2 is the same with the two-piece plan (poa_graph_checkpoint_plan2: three slotted and
 * snapshot planes, five window planes) and 24 bytes of carries per graph row and query in flight; it runs in that mode through
 * poa_batch_run_2piece only.  POA_SPAN_ENDS_FREE at creation: POA_ERR_UNSUPPORTED. */
int poa_batch_create_ex(const poa_graph_t* g, int device, uint32_t n_queries, const uint8_t* qseq,
                        const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes, poa_batch_t** out);
/* bytes of the plane workspace the batch holds */
int poa_batch_workspace_bytes(poa_batch_t* b, uint64_t* bytes);
int poa_batch_run(poa_batch_t* b, const poa_costs_t* costs, void* stream);
/* same with a mode: cfg NULL == dense */
int poa_batch_run_ex(poa_batch_t* b, const poa_costs_t* costs, const poa_config_t* cfg, void* stream);
/* Two-piece affine model on a resident batch: what poa_align_batch_2piece computes — the same scores, flags and pairs, bit for
 * bit — launched on `stream` without synchronising, results in the batch's own device buffers, so poa_batch_fetch,
 * poa_batch_stats and poa_batch_device_results serve it as they serve poa_batch_run_ex, and one batch may alternate the two.
 *   cfg NULL or POA_MODE_DENSE   the dense two-piece pass with its traceback and certificate; a batch of poa_batch_create.
 *                                Cells are u16 when [open1 + extend1 * longest query] + [open1 + extend1 * shortest path] <= 65534
 *                                and costs->wide_planes is 0, else u32.  Every query holds five planes of its OWN pitch; five u16
 *                                planes fit the region the batch planned for it, five u32 planes get a plan of their own on the
 *                                first such run (and, only if the longest query's do not fit, a larger workspace:
 *                                poa_batch_workspace_bytes then grows).  No allocation, copy or host synchronisation after the
 *                                first run of a width.
 *   POA_MODE_SCORE               the score-only sweep under open' = open1 + extend1 - extend2, extend' = extend2; a batch created
 *                                for POA_MODE_SCORE.
 *   POA_MODE_EXACT / HYBRID / CHECKPOINT, POA_SPAN_ENDS_FREE: POA_ERR_UNSUPPORTED (the replay runs through the one-shot call
 *                                alone: poa_align_batch_2piece_ex; checkpointed mode is one-piece only).
 *   POA_MODE_CHECKPOINT2         poa_align_batch_2piece's results from a slot-sized workspace: per chunk a two-piece sweep that
 *                                keeps slots and snapshots of M, D1 and D2 (pass 1), then, last segment first, the recompute of a
 *                                segment's five planes into the window and the walk through it (pass 2); a batch created for
 *                                POA_MODE_CHECKPOINT2.  Cell width by the rule above; the batch is sized for u32, so a u16 run
 *                                packs twice the queries per chunk.  poa_stats_t.plane_bytes = the bytes written when the walk enters
 *                                every segment (at most that: a segment an edge skips is not recomputed).
 *                                poa_batch_fetch_planes and poa_batch_fetch_planes_2piece return POA_ERR_UNSUPPORTED afterwards.
 *                                Such a batch in any other mode, or through poa_batch_run / poa_batch_run_ex, and any other
 *                                batch in this mode: POA_ERR_INVALID_ARG.
 * A batch created for another mode than the run's: POA_ERR_INVALID_ARG; extend1 < extend2: POA_ERR_INVALID_ARG.
 * poa_stats_t.plane_bytes = cells x 5 x cell bytes.  Afterwards poa_batch_last_layout reports POA_LAYOUT_U16 or 0,
 * poa_batch_fetch_planes returns POA_ERR_UNSUPPORTED and poa_batch_fetch_search_counters POA_ERR_INVALID_ARG. */
int poa_batch_run_2piece(poa_batch_t* b, const poa_costs2_t* costs, const poa_config_t* cfg, void* stream);
int poa_batch_fetch(poa_batch_t* b, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off,
                    uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats);
/* synchronise the stream and return the HIP-event timings accumulated over every poa_batch_run
 * since the last poa_batch_stats / poa_batch_fetch call (no device->host result copy) */
int poa_batch_stats(poa_batch_t* b, poa_stats_t* stats);
/* device pointers of the results of the last run (valid until the next run / destroy):
 * score u32[n], flags u32[n], pair_off u64[n+1], pairs poa_aln_pair_t[pair_off[n]] */
int poa_batch_device_results(poa_batch_t* b, void** score, void** flags, void** pair_off, void** pairs);
/* AstarResult::{num_queued, num_visited, num_pruned} (src/aligner/astar.rs:81-90) of the queries whose result came from the
 * replayed search in the last exact / hybrid run, plus the number of steps the wave search took: out[4 * n], one
 * {num_queued, num_visited, num_pruned, steps} per query (zeros for queries that were not replayed). */
int poa_batch_fetch_search_counters(poa_batch_t* b, uint32_t* out);
/* how the dense pass of the last run stored its score planes: POA_LAYOUT_* bits.  Chosen per run from a bound on the optimal
 * score (u32 Score values of the reference, src/aligner/scoring/mod.rs:64-70, are kept verbatim unless a narrower
 * encoding is provably exact for everything the result depends on). */
#define POA_LAYOUT_U16 1u       /* 2-byte cells (bound <= 65534) */
#define POA_LAYOUT_COMPACT 2u   /* M plane + 4 flag bits per cell + the D rows that are read back */
#define POA_LAYOUT_DERIVED_GAPS 8u /* compact cells keep the two Match-state flags only; the traceback derives the gap-state ones */
#define POA_LAYOUT_RELATIVE 4u  /* cells hold score - e * (shortest-path depth of the row - column): scores beyond u16 */
int poa_batch_last_layout(poa_batch_t* b, uint32_t* layout);
/* the banded forward pass of the last dense run (one-strip batches, 512 < widest plane row <= 1024): out[0] = 1 if it ran,
 * out[1] = queries whose banded result was certified exact and kept, out[2] = queries the full kernel recomputed, out[3] = the
 * smallest band distance D among the queries it ran on (a query is certified when its score is <= e * (D - 4)).
 * Synchronises with the run's stream. */
int poa_batch_band_info(poa_batch_t* b, uint32_t out[4]);
/* what the dense one-piece pass launched for chunk `chunk` of the last run (tests: did the kernel an override names really run?):
 *   out[0] forward kernel, POA_KERNEL_*      out[1] column groups per lane ("quads": 512 u16 / 256 u32 columns each)
 *   out[2] POA_LAUNCH_* bits                 out[3] waves per workgroup
 *   out[4] TbParams::code_fmt of the cells   out[5] lanes per walk of the separate traceback launch (0: none, the walk was fused)
 *   out[6] traceback speculation depth       out[7] queries in the chunk
 * The cell type and layout are the run's (poa_batch_last_layout).  POA_ERR_INVALID_ARG: no run yet, or no such chunk;
 * POA_ERR_UNSUPPORTED: the last run was not a dense one-piece run (another mode, or the two-piece model).  Host side only. */
enum {
    POA_KERNEL_NONE = 0,
    POA_KERNEL_FORWARD,   /* poa_forward_kernel<quads, u16 | u32, fuse, compact, MW> */
    POA_KERNEL_PACKED,    /* poa_forward_packed_kernel<quads, fuse, MW> */
    POA_KERNEL_PX,        /* poa_forward_px_kernel<0..3> (code_fmt 1..4) */
    POA_KERNEL_PXMW,      /* poa_forward_pxmw_kernel */
    POA_KERNEL_BAND       /* poa_forward_band_kernel<false> (and / or poa_forward_band2_kernel: poa_batch_band_pair_info), then <true> over the queries it could not certify */
};
#define POA_LAUNCH_FUSE 1u   /* the forward kernel walked the traceback of its queries in its epilogue */
#define POA_LAUNCH_MW 2u     /* one workgroup per query, its strips pipelined over the waves */
#define POA_LAUNCH_STRIPS 4u /* poa_multi_last_launch only: the chunk ran the strip loop of a POA_CFG_WIDE_QUERIES batch */
int poa_batch_last_launch(poa_batch_t* b, uint32_t chunk, uint32_t out[8]);
/* what the exact replay launched for chunk `chunk` of the last run (POA_MODE_EXACT, POA_MODE_HYBRID, every ends-free run):
 *   out[0] replay kernel, POA_REPLAY_*        out[1] priorities in the descriptor ring (`win`; the lane kernel has no ring)
 *   out[2] lanes per query                    out[3] waves per block
 *   out[4] POA_REPLAY_BIT_* bits              out[5] resident blocks as the launcher computed them (0: it did not ask)
 *   out[6] blocks launched                    out[7] dynamic LDS bytes of the launch
 * POA_ERR_INVALID_ARG: no run yet, or no such chunk; POA_ERR_UNSUPPORTED: the last run replayed nothing.  Host side only. */
enum {
    POA_REPLAY_NONE = 0,
    POA_REPLAY_LANE,          /* poa_exact_kernel: one sequential search per lane */
    POA_REPLAY_WAVE_LDS,      /* poa_wsearch_kernel: a wave per query, graph and ring in LDS */
    POA_REPLAY_WAVE_GROUPS,   /* poa_wsearch_groups_kernel: several queries per wave */
    POA_REPLAY_WAVE_GENERIC,  /* poa_wsearch_global_kernel: a wave per query, graph or ring read through generic pointers */
    POA_REPLAY_FLAT_GENERIC,  /* poa_fsearch_kernel: the parallel step over the generic code */
    POA_REPLAY_FLAT_LEAN      /* poa_fsearch_lean_kernel: the parallel step's lean code (Global runs with row records) */
};
#define POA_REPLAY_BIT_GRAPH_LDS 1u    /* the graph arrays (flat lean: the row records it reads) were staged into LDS */
#define POA_REPLAY_BIT_REC_LDS 2u      /* the per-row records were staged into LDS */
#define POA_REPLAY_BIT_RING_GLOBAL 4u  /* the descriptor ring lay in global memory */
#define POA_REPLAY_BIT_PERSISTENT 8u   /* persistent schedule: `resident` blocks took the queries from a work counter */
int poa_batch_replay_info(poa_batch_t* b, uint32_t chunk, uint32_t out[8]);
/* the paired banded pass of the last dense run (two queries of one length per wave, one per 16-bit half of every register):
 * out[0] = queries that ran paired, out[1] = queries of banded chunks that ran one per wave, out[2] = the default rule's
 * count (a chunk pairs from that many queries in pairs on; POA_TUNE_BAND_PAIR overrides), out[3] = 1 if the run paired.
 * poa_batch_band_info and poa_batch_last_launch say the same for both ways.  Host side only. */
int poa_batch_band_pair_info(poa_batch_t* b, uint32_t out[4]);
/* POA_TUNE_BAND_PAIR, in full: value & POA_BAND_PAIR_MASK is the pairing (0 never, 1 always, POA_BAND_PAIR_RULE: the default
 * rule, as if unset), (value >> POA_BAND_NARROW_SHIFT) & 3 the narrow tier of the paired pass (0: the default rule, 1: never,
 * 2: for every pair whose class has a narrow band, whatever the rule says). */
#define POA_BAND_PAIR_MASK 3
#define POA_BAND_PAIR_RULE 2
#define POA_BAND_NARROW_SHIFT 2
/* the narrow tier of the last dense run (paired banded pass over a window of 384 columns; a query it cannot certify runs the
 * 512-column pass, and the full pass after that): out[0] = queries that ran the narrow tier, out[1] = those it certified,
 * out[2] = those the 512 pass then certified (the rest were recomputed by the full pass), out[3] = 0 the tier did not run,
 * 1 the default rule chose it, 2 an override did.  poa_batch_band_info counts a query certified by either tier as banded. */
int poa_batch_band_narrow_info(poa_batch_t* b, uint32_t out[4]);
/* debugging / parity: copy the M, I, D score planes of query i (rows x (len+1), row = topological
 * rank, see poa_graph_node_rows) — only valid if the query's chunk was the last one run */
int poa_batch_fetch_planes(poa_batch_t* b, uint32_t query, uint32_t* m, uint32_t* i, uint32_t* d);
/* debugging / parity: the planes of query i as a dense one-piece run stored them in the compact derived-gaps layout (the last
 * run's layout has POA_LAYOUT_DERIVED_GAPS and not POA_LAYOUT_RELATIVE), rows x (len+1) each, row = the engine's row
 * (poa_graph_node_rows), the pitch padding stripped:
 *   m_raw   the stored M words as they lie in memory: the score in bits 0..13 (0x3FFF: INF), bit 14: I == M, bit 15: D == M
 *   d       the kept D rows (0xFFFF: INF); a row the layout does not keep is filled with 0xFFFF and has d_kept[row] = 0
 *   d_kept  [rows] 1 for the rows whose D the layout keeps
 * After the banded forward pass only the cells inside a certified query's windows were written by that run.  Valid under the rule
 * of poa_batch_fetch_planes (the query's chunk was the last one run); any other layout or mode: POA_ERR_UNSUPPORTED.  Synchronises
 * with the run's stream. */
int poa_batch_fetch_compact(poa_batch_t* b, uint32_t query, uint16_t* m_raw, uint16_t* d, uint8_t* d_kept);
/* the five planes M, I1, D1, I2, D2 of query i after a dense poa_batch_run_2piece, rows x (len + 1) each — valid under the rule
 * of poa_batch_fetch_planes: the query's chunk was the last one run, and the last run was a dense two-piece run */
int poa_batch_fetch_planes_2piece(poa_batch_t* b, uint32_t query, uint32_t* m, uint32_t* i1, uint32_t* d1, uint32_t* i2, uint32_t* d2);
void poa_batch_destroy(poa_batch_t* b);

/* ---- multi-graph batch: the queries of many graphs in one checkpointed run ---------------- */
/* For hosts that bring hundreds of small graphs with a few reads each (window consensus, amplicon families): one launch per
 * pass covers every query of every graph, one wavefront per query, each wave reading its own graph's tables.
 *   graphs[n_graphs]          graph handles; the same handle may be listed more than once (its tables are uploaded once)
 *   graph_qoff[n_graphs + 1]  queries are grouped by graph: graph g owns the queries [graph_qoff[g], graph_qoff[g + 1]), a range
 *                             may be empty.  graph_qoff[0] must be 0 and the array non-decreasing; graph_qoff[n_graphs] IS the
 *                             query count n of the batch, so qseq / qoff[n + 1] must hold that many queries (a caller that
 *                             knows its count another way checks the two against each other before the call, as the Python
 *                             binding does)
 *   cfg                       NULL or mode POA_MODE_CHECKPOINT, the only mode: the results are dense mode's score, pairs,
 *                             pair_off and flags of every query against its own graph, bit for bit (poa_align_batch_ex in that
 *                             mode, graph by graph).  Every other mode, and POA_SPAN_ENDS_FREE: POA_ERR_UNSUPPORTED.
 *                             tune[POA_TUNE_CKPT_ROWS] (read at creation / by poa_multi_footprint) applies to every graph,
 *                             tune[POA_TUNE_PLANES] to a run.
 * Results are in query order; pairs[].rpos is the node index in THAT query's graph; pair_off runs over all queries; capacity
 * sum(len_i + n_nodes(graph_i)) always suffices.  Queries against a graph without real nodes get POA_FLAG_EMPTY_GRAPH, score
 * 4 * len and no pairs, as poa_align_batch_ex gives them.  POA_ERR_INVALID_ARG: graph_qoff[0] != 0, graph_qoff not
 * non-decreasing, a NULL graph or array.
 * Memory: a query holds rows_per_query(its graph) x pitch 4-byte cells + 256 bytes (poa_graph_checkpoint_plan of its graph alone;
 * pitch = len + 1 rounded up to 64).  poa_multi_footprint returns the sum over all queries (the batch as one chunk) and its
 * largest term, on the host, without a device.  poa_multi_create takes workspace_bytes as a cap (0: the whole batch, or what
 * free device memory allows; a cap below the largest query is raised to it) and cuts the queries into chunks greedily in query
 * order — a chunk ends in front of the first query that no longer fits, inside a graph's range or between two graphs.  The
 * batch is sized for u32 cells; a u16 run uses the same chunks and half of every region.  The cell width of a run is u16 only
 * if EVERY graph that has queries allows it — [open + extend x its longest query] + [open + extend x its shortest path] <=
 * 65534 — and tune[POA_TUNE_PLANES] is not 32; else u32 for the whole run.  Both are exact: results do not depend on it.
 * Carries between strips (queries of more than 1024 columns only): 16 bytes per graph row of such a query in flight.
 * poa_multi_run launches on `stream` (a hipStream_t, NULL = default stream) without synchronising, and may be called again
 * with other costs; poa_multi_fetch / _stats / _device_results behave as their poa_batch_* namesakes, with poa_stats_t summed
 * over all graphs (cells = sum rows(graph_i) x (len_i + 1)).  poa_graph_update on a member graph after poa_multi_create: the
 * batch keeps the tables it copied and must not be run again.  A poa_multi_t belongs to one thread at a time. */
typedef struct poa_multi poa_multi_t;
/* host only, no device: bytes of plane workspace for the whole batch as one chunk, and of its largest query */
int poa_multi_footprint(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                        const uint64_t* qoff, const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes);
int poa_multi_create(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device,
                     const uint8_t* qseq, const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes,
                     poa_multi_t** out);
int poa_multi_run(poa_multi_t* m, const poa_costs_t* costs, const poa_config_t* cfg, void* stream);
int poa_multi_fetch(poa_multi_t* m, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                    uint32_t* flags, poa_stats_t* stats);
int poa_multi_stats(poa_multi_t* m, poa_stats_t* stats);
int poa_multi_device_results(poa_multi_t* m, void** score, void** flags, void** pair_off, void** pairs);
/* bytes of the plane workspace the batch holds: its largest chunk */
int poa_multi_workspace_bytes(poa_multi_t* m, uint64_t* bytes);
void poa_multi_destroy(poa_multi_t* m);
/* one-shot: create, run, fetch, destroy */
int poa_align_multi(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                    const poa_costs_t* costs, const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff,
                    uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity, uint32_t* flags,
                    poa_stats_t* stats, int device);

/* The same batch under the two-piece affine model: for every query what poa_align_batch_2piece returns for it against its own
 * graph alone — score, pairs, pair_off, flags, bit for bit (poa_align_batch_2piece_ex in POA_MODE_CHECKPOINT2, graph by
 * graph).  Global only.  The argument lists are those of the one-piece namesakes with poa_costs2_t for the costs; the object is
 * a poa_multi_t, and poa_multi_fetch / _stats / _device_results / _workspace_bytes / _destroy serve it unchanged.  Its
 * footprint is fixed at creation, before any costs are seen, and differs from the one-piece batch's: hence a create function
 * of its own, and poa_multi_create / _run / _footprint / poa_align_multi keep refusing POA_MODE_CHECKPOINT2.
 *   cfg      NULL or mode POA_MODE_CHECKPOINT2; every other mode, and POA_SPAN_ENDS_FREE: POA_ERR_UNSUPPORTED.
 *            tune[POA_TUNE_CKPT_ROWS] (read at creation / by the footprint) applies to every graph, tune[POA_TUNE_PLANES] to a run.
 * POA_ERR_INVALID_ARG: poa_multi_run on a batch of poa_multi_create_2piece, poa_multi_run_2piece on a batch of
 * poa_multi_create, gap_extend1 < gap_extend2, the argument errors of poa_multi_create, a fetch before a run.  The batch stays
 * usable after a refused call; the run may be repeated with other costs and on any stream, and allocates nothing on the device.
 * Memory: a query holds rows_per_query2(its graph) x pitch 4-byte cells + 256 bytes (poa_graph_checkpoint_plan2 of its graph
 * alone at the batch's segment length: three kept planes, five window planes; pitch = len + 1 rounded up to 64).
 * poa_multi_footprint_2piece returns the sum and the largest term; chunks are cut greedily in query order under
 * workspace_bytes exactly as poa_multi_create cuts them (0: the whole batch, or what free memory allows; a cap below the
 * largest query is raised to it).  The batch is sized for u32 cells; a u16 run uses the same chunks and half of every region.
 * The cell width of a run is u16 only if EVERY graph that has queries allows it — [open1 + extend1 x its longest query] +
 * [open1 + extend1 x its shortest path] <= 65534 — costs->wide_planes is 0 and tune[POA_TUNE_PLANES] is not 32; else u32 for
 * the whole run.  Both are exact: results do not depend on it.  Carries between strips (queries of more than 1024 columns
 * only): 24 bytes per graph row of such a query in flight; a query of pitch <= 1024 never touches a carry.
 * poa_stats_t is summed over graphs as for poa_multi_run: cells = sum rows(graph_i) x (len_i + 1), plane_bytes = sum over
 * queries of (3 x (slotted + snapshot rows) + 5 x rows) x pitch x cell bytes. */
int poa_multi_footprint_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                               const uint64_t* qoff, const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes);
int poa_multi_create_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device,
                            const uint8_t* qseq, const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes,
                            poa_multi_t** out);
int poa_multi_run_2piece(poa_multi_t* m, const poa_costs2_t* costs, const poa_config_t* cfg, void* stream);
/* one-shot: create, run, fetch, destroy */
int poa_align_multi_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff,
                           const poa_costs2_t* costs, const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff,
                           uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                           uint32_t* flags, poa_stats_t* stats, int device);

/* ---- score set: score-only runs over (query, graph) pairs of many graphs ------------------- */
/* For the question that comes before the alignment — which of these graphs does a read belong to (read-to-family assignment,
 * choosing the window or haplotype graph before a POA build, demultiplexing against amplicon graphs): one launch per kernel
 * class covers every pair, one wavefront per pair, each wave reading its own pair's graph's tables.  The winners then go to
 * poa_multi_* for their alignments.
 *   graphs[n_graphs]          graph handles; the same handle may be listed more than once (its tables are uploaded once)
 *   qseq / qoff[n_queries+1]  the pool of queries, uploaded once however many pairs name them
 *   pair_query[n_pairs],      u32 indices into the query pool and the graph list, in any order, with repeats; a graph or a
 *   pair_graph[n_pairs]       query may have no pair at all.  Both NULL and n_pairs == n_queries * n_graphs: the full matrix,
 *                             pair p = (query p / n_graphs, graph p % n_graphs).  n_pairs == 0 is valid and returns nothing.
 *   cfg                       NULL or mode POA_MODE_SCORE, the only mode.  Every other mode, and POA_SPAN_ENDS_FREE:
 *                             POA_ERR_UNSUPPORTED.  tune[POA_TUNE_PLANES] and tune[POA_TUNE_PX] apply to a run, as they do to
 *                             a score-mode poa_batch_run_ex.
 * Results are in pair order: score[p] and flags[p] are, bit for bit, what poa_align_batch_ex in POA_MODE_SCORE returns for that
 * query against that graph alone (poa_scoreset_run), or poa_align_batch_2piece_ex in that mode (poa_scoreset_run_2piece, through
 * the cost equivalence open' = open1 + extend1 - extend2, extend' = extend2 of DESIGN.md §6a): dense mode's score; flags carry
 * only POA_FLAG_EMPTY_GRAPH and POA_FLAG_SHORT_QUERY; a pair against a graph without real nodes gets score 4 * len and
 * POA_FLAG_EMPTY_GRAPH.  The two runs may alternate on one set, with other costs each time.
 * POA_ERR_INVALID_ARG: a pair index out of range, a NULL graph or array (other than the both-NULL matrix form), an n_pairs that
 * does not match the matrix form, poa_scoreset_fetch before a run, gap_extend1 < gap_extend2.
 * Memory: a pair holds max(n_slots(its graph), 1) x pitch 4-byte cells of M and of D + 256 bytes (poa_graph_sweep_slots; pitch =
 * len + 1 rounded up to 64) — the per-query rule of a score-mode batch with the pair's own graph's n_slots.
 * poa_scoreset_footprint returns the sum over all pairs (the set as one chunk) and its largest term, on the host, without a
 * device.  poa_scoreset_create takes workspace_bytes as a cap (0: the whole set, or what free device memory allows; a cap below
 * the largest pair is raised to it) and cuts the pairs into chunks greedily in pair order.  The set is sized for u32 cells.
 * The cell width of a run is u16 only if EVERY graph that appears in a pair allows it — [open + extend x the longest query
 * paired with it] + [open + extend x its shortest path] <= 65534, with the reduced costs for the two-piece run — and
 * tune[POA_TUNE_PLANES] is not 32; else u32 for the whole run.  Both are exact: results do not depend on it.
 * Carries between strips (pairs of more than 1024 columns only): 16 bytes per graph row of such a pair in flight.
 * poa_scoreset_run* launch on `stream` (a hipStream_t, NULL = default stream) without synchronising; after the set's creation
 * a run allocates nothing on the device.  poa_stats_t counts pairs: n_queries = n_pairs, cells = sum rows(graph) x (len + 1),
 * plane_bytes = the slot bytes the last run stored.  poa_graph_update on a member graph after poa_scoreset_create: the set
 * keeps the tables it copied and must not be run again.  A poa_scoreset_t belongs to one thread at a time. */
typedef struct poa_scoreset poa_scoreset_t;
/* host only, no device: bytes of slot workspace for the whole set as one chunk, and of its largest pair */
int poa_scoreset_footprint(const poa_graph_t* const* graphs, uint32_t n_graphs, uint32_t n_queries, const uint64_t* qoff,
                           uint64_t n_pairs, const uint32_t* pair_query, const uint32_t* pair_graph, const poa_config_t* cfg,
                           uint64_t* bytes, uint64_t* largest_pair_bytes);
int poa_scoreset_create(const poa_graph_t* const* graphs, uint32_t n_graphs, int device, uint32_t n_queries, const uint8_t* qseq,
                        const uint64_t* qoff, uint64_t n_pairs, const uint32_t* pair_query, const uint32_t* pair_graph,
                        const poa_config_t* cfg, uint64_t workspace_bytes, poa_scoreset_t** out);
int poa_scoreset_run(poa_scoreset_t* s, const poa_costs_t* costs, const poa_config_t* cfg, void* stream);
int poa_scoreset_run_2piece(poa_scoreset_t* s, const poa_costs2_t* costs, const poa_config_t* cfg, void* stream);
/* Capped runs — a score cap per pair and an exact early exit in the sweep (poa_scoreset_run_capped, poa_scoreset_run_2piece_capped,
 * poa_scoreset_fetch_swept) — are declared in poasta_amd_scoreset_cap.h, which this header includes at its end; best-of runs
 * — the cap is the query's best score so far, the run returns the winning pair per query (poa_scoreset_run_best,
 * poa_scoreset_fetch_best, poa_score_best) — in poasta_amd_scoreset_best.h, included after it. */
/* synchronises; score[n_pairs], flags[n_pairs] (may be NULL) in pair order */
int poa_scoreset_fetch(poa_scoreset_t* s, uint32_t* score, uint32_t* flags, poa_stats_t* stats);
int poa_scoreset_stats(poa_scoreset_t* s, poa_stats_t* stats);
int poa_scoreset_device_results(poa_scoreset_t* s, void** score, void** flags);
/* bytes of the slot workspace the set holds: its largest chunk */
int poa_scoreset_workspace_bytes(poa_scoreset_t* s, uint64_t* bytes);
void poa_scoreset_destroy(poa_scoreset_t* s);
/* one-shot: create, run, fetch, destroy */
int poa_score_pairs(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs_t* costs, const poa_config_t* cfg,
                    uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs, const uint32_t* pair_query,
                    const uint32_t* pair_graph, uint32_t* score, uint32_t* flags, poa_stats_t* stats, int device);
int poa_score_pairs_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs2_t* costs, const poa_config_t* cfg,
                           uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs,
                           const uint32_t* pair_query, const uint32_t* pair_graph, uint32_t* score, uint32_t* flags,
                           poa_stats_t* stats, int device);

#ifdef __cplusplus
}
#endif
#include "poasta_amd_scoreset_cap.h"
#include "poasta_amd_scoreset_best.h"
#include "poasta_amd_tb.h"
#include "poasta_amd_multi_dense.h"
#include "poasta_amd_multi_exact.h"
#include "poasta_amd_multi_dense2.h"
#endif /* POASTA_AMD_H */
