// Host-side plan of a score set (poa_scoreset_*, poa_scoreset.hpp).  Host code, no device needed.
//
// A score set runs the score-only sweep (poa_forward_sweep.hpp) over a list of (query, graph) PAIRS: a shared pool of queries,
// a list of graphs, and pairs in any order, with repeats; one wavefront per pair, each wave reading the tables of its own
// pair's graph.  The plan says where everything lies:
//
//   per graph    n_rows, n_slots, n_slotted and the bases of its tables in the CONCATENATED device tables.  Two index spaces:
//                rows (RowMeta, slot) and edges (pred_rows, pred_slot).  The values in the tables stay graph-local, a wave
//                addresses them from its graph's base pointers.  A handle listed more than once has one copy of its tables.
//                Also the longest query paired with it (the run's cell-width bound) and its number of pairs.
//   per pair     graph, query; pitch = len + 1 rounded up to 64; the offset of its slot region in the workspace, in 4-byte
//                cells and relative to its chunk: a pair holds max(n_slots(graph), 1) x pitch cells of M and of D + 256 bytes
//                — the per-query rule of a score-mode batch (poa_batch_create_ex) with the pair's own graph's n_slots; its
//                carry offset.
//   chunks       greedy in pair order by that footprint under `workspace_bytes`: a chunk is closed in front of the first pair
//                that no longer fits.  The offsets are in 4-byte cells whatever the run's cell type: a u16 run and the packed
//                kernel (2048 bytes per slot row, which a pair of pitch > 512 always has room for) use the front of a region.
//   strip carries  as MultiPlan::carry_off: only a pair wider than one strip of the widest kernel variant (pitch > 1024
//                columns) takes 4 x n_rows(graph) words in the chunk's carry buffer, at its own offset.
//   kernel classes  where a single-graph run picks ONE kernel variant per chunk from the chunk's largest pitch, a chunk here
//                mixes pitches, so every pair has a class of its own — the packed one-strip kernel, or the general kernel at
//                Q = 1, 2 or 4 — and the run launches each non-empty class of a chunk once over the list of its pairs.  The
//                class depends on the cell width of the run and on whether the packed path is on, so the plan holds three
//                VARIANTS (u16 with the packed path, u16 without, u32): per variant the pairs of every chunk sorted by class
//                (stable: pair order inside a class) and, per chunk and class, the range of that list.
//   best-of runs   (build_scoreset_best_order, made at the set's first best-of run) the pairs of every query as a CSR, and per
//                variant a second list over the same ranges, ordered by (rank, pair index) inside a range.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "poa_sweep_rows.hpp"

namespace poa_amd {

constexpr uint32_t SCORESET_STRIP_COLUMNS = 1024;   // widest strip of the sweep kernels, both cell types
constexpr uint64_t SCORESET_REGION_PAD_CELLS = 64;  // 256 bytes behind every pair's region

enum ScoreSetClass : uint32_t { SS_CLASS_PX = 0, SS_CLASS_Q1, SS_CLASS_Q2, SS_CLASS_Q4, SS_N_CLASSES };
enum ScoreSetVariant : uint32_t { SS_VAR_U16_PX = 0, SS_VAR_U16, SS_VAR_U32, SS_N_VARIANTS };

struct ScoreSetGraphIn {         // what the plan reads of a graph handle
    const FlatGraph* g;
    const SweepRows* sweep;
};

struct ScoreSetGraphPlan {
    uint32_t table_of = 0;       // first listing of the same handle: it owns the tables, this listing shares its bases
    uint32_t n_rows = 0, n_edges = 0, n_slots = 0, n_slotted = 0;
    uint64_t row_base = 0, edge_base = 0;
    uint64_t max_len = 0;        // longest query paired with this graph
    uint64_t n_pairs = 0;
    bool empty = false;          // no real nodes: its pairs get the shortcut result
};

// the kernel class of a pair of that pitch in a run of that variant (the rule of run_sweep, per pair instead of per chunk)
inline ScoreSetClass scoreset_class(uint32_t variant, uint32_t pitch) {
    if (variant == SS_VAR_U32) return pitch <= 256 ? SS_CLASS_Q1 : (pitch <= 512 ? SS_CLASS_Q2 : SS_CLASS_Q4);
    if (pitch <= 512) return SS_CLASS_Q1;
    if (variant == SS_VAR_U16_PX && pitch <= 1024) return SS_CLASS_PX;
    return SS_CLASS_Q2;
}

struct ScoreSetPlan {
    struct Chunk {
        uint32_t first, count;
        uint64_t cells, carry_words;
        uint32_t class_begin[SS_N_VARIANTS][SS_N_CLASSES + 1];   // ranges of class_list[variant], absolute pair positions
    };
    uint32_t n_queries = 0, n_pairs = 0;
    std::vector<ScoreSetGraphPlan> graphs;
    uint64_t n_rows_total = 0, n_edges_total = 0;
    std::vector<uint32_t> pair_graph, pair_query, pitch, carry_off;   // [n_pairs]
    std::vector<uint64_t> region_off;                                 // [n_pairs] 4-byte cells from the start of the pair's chunk
    std::vector<uint32_t> class_list[SS_N_VARIANTS];                  // [n_pairs] pair indices, chunk by chunk, class by class
    // best-of runs (poa_scoreset_run_best): the pairs of every query, and a second launch order
    std::vector<uint32_t> query_off;                                  // [n_queries + 1] CSR over query_pairs
    std::vector<uint32_t> query_pairs;                                // [n_pairs] a query's pairs, ascending pair index
    std::vector<uint32_t> best_list[SS_N_VARIANTS];                   // [n_pairs] the (chunk, class) ranges of class_list, each
                                                                      // ordered by (rank, pair index); see build_scoreset_best_order
    std::vector<Chunk> chunks;
    uint64_t bytes_total = 0;           // the whole set as one chunk
    uint64_t largest_pair_bytes = 0;
    uint64_t workspace_bytes = 0;       // the largest chunk: what the set holds
    uint64_t max_carry_words = 0;       // the largest chunk's carries
    uint64_t total_cells = 0, total_bases = 0;
    uint64_t slotted_pitch = 0;         // sum over the pairs outside the packed class (u16, packed path on) of n_slotted x pitch
    uint64_t slotted_pitch_all = 0;     // the same sum over all pairs
    uint64_t slotted_px = 0;            // sum of n_slotted over the pairs of the packed class
};

// 4-byte cells a pair holds: a query of `len` symbols on a graph of `n_slots` slots, padding included
inline uint64_t scoreset_pair_cells(uint32_t n_slots, uint64_t len) {
    return 2ull * (n_slots ? n_slots : 1u) * (((len + 1 + 63) / 64) * 64) + SCORESET_REGION_PAD_CELLS;
}

// pair_query / pair_graph both null: the full matrix, n_pairs == n_queries * n_graphs, pair p = (p / n_graphs, p % n_graphs)
// (n_pairs == 0 is a valid, empty set in either form).
// workspace_bytes 0: no cap (one chunk).  A cap below the largest pair's footprint is raised to it.
// Returns 0, or -1 (invalid argument) / -7 (unsupported) — the values of POA_ERR_INVALID_ARG / POA_ERR_UNSUPPORTED — with `err` set.
int build_scoreset_plan(const ScoreSetGraphIn* graphs, uint32_t n_graphs, uint32_t n_queries, const uint64_t* qoff, uint64_t n_pairs,
                        const uint32_t* pair_query, const uint32_t* pair_graph, uint64_t workspace_bytes, ScoreSetPlan& out,
                        std::string& err);

// What a best-of run adds to a built plan: the query-to-pairs CSR and, per variant, the best-of launch order.  A pair's RANK is
// its position among its query's pairs in pair order.  Every (chunk, class) range of class_list is reordered by (rank, pair
// index), so the k-th candidate of every query is dispatched before any (k + 1)-th: in pair order a query's candidates are
// neighbours and run side by side, none of them seeing a result of another; in rank order the caller's most likely graph,
// listed first, has set the query's cap by the time its later candidates start.  Idempotent.
void build_scoreset_best_order(ScoreSetPlan& plan);

}  // namespace poa_amd
