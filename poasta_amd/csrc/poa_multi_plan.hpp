// Host-side plan of a multi-graph checkpointed batch (poa_multi_*, poa_multi.hpp).  Host code, no device needed.
//
// A multi-graph batch runs the queries of MANY graphs in one launch of the checkpointed kernels (poa_checkpoint.hpp): one
// wavefront per query, each wave reading the tables of its own query's graph.  Queries are grouped by graph: graph g owns the
// queries [graph_qoff[g], graph_qoff[g + 1]).  The plan says where everything lies:
//
//   per graph    its CheckpointPlan — what poa_graph_checkpoint_plan gives for that graph alone at the batch's segment length —
//                and the bases of its tables in the CONCATENATED device tables.  Four index spaces: rows (RowMeta, slot; n_rows
//                entries per graph), edges (pred_rows, pred_slot, pred_src), snap_off (n_rows + 1 entries: a CSR of its own, which
//                indexes snap_dst from that graph's snap_dst base) and boundary (n_segments + 1).  The values in the tables stay
//                graph-local (row 0 is the graph's first row): a wave addresses them from its graph's base pointers, so the
//                kernels' bodies see exactly the tables a single-graph batch would hand them.  A handle listed more than once
//                has one copy of its tables.
//   per query    graph id; pitch = columns rounded up to 64 (the rule of a single-graph batch); the offset of its region in the
//                plane workspace, in 4-byte cells and relative to its chunk: a query holds rows_per_query(graph) x pitch cells
//                + 256 bytes of padding; the offset of its pair scratch, capacity len + n_rows(graph).
//   chunks       greedy in query order by that footprint under `workspace_bytes`: a chunk is closed in front of the first query
//                that no longer fits.  A boundary may fall inside a graph's range or between two graphs; a graph without queries
//                never shows.  The offsets are in cells of the run's cell type: a u16 run uses the same numbers, i.e. the
//                first half of every region's bytes.
//   strip carries  pass 1 hands the insertion value and the last column's M from strip to strip through two parities of
//                2 x n_rows words per query (ckpt_rows: carry + parity * 2 * n_rows + 2 * row).  With graphs of different n_rows
//                a common stride would have to be 4 x the LARGEST n_rows in the batch for every query; instead every query has
//                its own offset, carry_off[q], into the chunk's carry buffer, and only a query wider than one strip of the
//                widest kernel variant (pitch > 1024 columns: 64 lanes x 8 u16 cells x Q 2, or x 4 u32 cells x Q 4) takes
//                4 x n_rows(graph) words there.  Every variant the launch code selects for a chunk has strips of at least the
//                chunk's largest pitch when that pitch is <= 1024, so a query of pitch <= 1024 never touches a carry.
//
// The two-piece variant (poa_multi_*_2piece, poa_multi.hpp; `two_piece` below) is the same plan with the two-piece weights:
// per graph the two-piece CheckpointPlan (three kept planes, five window planes: what poa_graph_checkpoint_plan2 gives for
// that graph alone; MultiGraphIn::own is then the handle's two-piece plan), and 6 x n_rows carry words for a query wider than
// one strip (ckpt2_rows: two parities of three words per row).  Its strips are 1024 columns under both cell types too.
//
// The dense variant (poa_multi_*_dense, poa_multi_dense.hpp; build_multi_dense_plan below) lays out the compact u16 planes of
// the packed forward pass instead: per query compact_plane_elems(n_rows(graph), pitch, kept D rows of the graph) two-byte
// elements (poa_graph.hpp: the M plane, a quarter plane of flag codes, the kept D rows; a graph without a d_slot table keeps
// all n_rows of them) + 256 bytes of padding.  region_off and Chunk::cells are then in TWO-byte elements, relative to the
// query's chunk; chunks are cut by the same greedy rule; Chunk::max_pitch chooses the kernel's quads (1 up to 512 columns,
// 2 above).  Without `wide` every query is one strip: a query of more than 1023 symbols (pitch above 1024) is refused, and there
// are no carries.  With `wide` (POA_CFG_WIDE_QUERIES) any length passes and the carry rule above holds with the packed kernel's
// words: a query of pitch > MULTI_STRIP_COLUMNS takes 2 x n_rows(graph) words at carry_off[q], relative to its chunk
// (forward_packed_strips: carry[2r] the insertion-scan carry, carry[2r + 1] I of the strip's last column; one parity, the wave
// reads a row's words before it overwrites them), every other query 0; Chunk::carry_words and max_carry_words as in
// build_multi_plan.  The exact variant cuts its own chunks and lays the carries out by them.  The tables a dense graph needs are rows and d_slot by row (row_base), pred_rows and pred_dslot by edge
// (edge_base); the checkpoint fields of MultiGraphPlan stay empty.
//
// The dense two-piece variant (poa_multi_*_dense_2piece, poa_multi_dense2.hpp; build_multi_dense2_plan below) is the dense plan
// over five full u16 planes: per query 5 x n_rows(graph) x pitch two-byte elements (M, I1, D1, I2, D2) + 256 bytes of padding,
// region_off and Chunk::cells in two-byte elements relative to the query's chunk, the same greedy chunks.  Any query length and
// no carries: the forward body loops over passes of 512 columns, and a row wider than the passes it keeps in registers reads its
// predecessor back from the planes.  POA_CFG_WIDE_QUERIES is not read.  plane_bytes = sum of 2 x 5 x n_rows x pitch.  The
// tables such a graph needs are rows (row_base) and pred_rows (edge_base).
//
// The exact variant (poa_multi_*_exact, poa_multi_exact.hpp; build_multi_exact_plan below) is the dense plan plus what the
// replay of the reference's search needs (poa_wsearch.hpp):
//   per query    a second region behind the chunk's dense regions: the u32 visited table of the search, 3 x n_rows(graph) x
//                pitch four-byte cells + 256 bytes of padding.  table_off[q] is in FOUR-byte cells from the start of the
//                workspace (the chunk's dense regions end at Chunk::cells two-byte elements, a multiple of 16 bytes).
//   chunks       greedy by the sum of both footprints.
//   per graph    the bases of its ExactGraph arrays in the concatenated tables: sym (sym_base, padded to four bytes), the two
//                CSR offset arrays of n_rows + 1 entries (off_base), successors (succ_base), node-bubble entries (nbm_base);
//                dist_min / dist_max / exit_idx / the row records lie at row_base.  The values stay graph-local.
//   per slot     the replay workspace of one wave (MultiExactSlot): reached sets, their summaries, the DFA stack, the chunked
//                queue pool and a descriptor ring for launches that keep the ring in global memory.  ONE size for every slot:
//                the maxima over the graphs that have queries of what prepare_exact (poa_engine.hip) computes per graph.
//                THE STRIDE RULE: ws_search_query addresses a slot's reached sets as base + slot * n_exit(graph) * wpn, and
//                n_exit differs from graph to graph, so the slots of a multi-graph launch would overlap.  Every slot therefore
//                owns reached_stride = max n_exit x wpn words (rsum_stride likewise), and the kernel hands the search a base
//                biased by slot * (stride - n_exit(graph) * wpn) so that its expression lands on base + slot * stride.
//                Slots = the largest chunk's queries.  The sizes depend on the costs (ring width, queue pool): the plan holds
//                them for the costs it was given, and a run with other costs recomputes them (multi_exact_slot).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "poa_graph.hpp"
#include "poa_sweep_rows.hpp"

namespace poa_amd {

constexpr uint32_t MULTI_STRIP_COLUMNS = 1024;   // widest strip of the checkpointed kernels, both cell types
constexpr uint64_t MULTI_REGION_PAD_CELLS = 64;  // 256 bytes behind every query's region

struct MultiGraphIn {            // what the plan reads of a graph handle
    const FlatGraph* g;
    const SweepRows* sweep;
    const CheckpointPlan* own;   // the handle's plan at the engine's own segment length (two_piece: its two-piece plan)
};

struct MultiGraphPlan {
    CheckpointPlan ckpt;
    uint32_t table_of = 0;       // first listing of the same handle: it owns the tables, this listing shares its bases
    uint32_t n_rows = 0, n_edges = 0, n_slots = 0;
    uint64_t row_base = 0, edge_base = 0, snap_off_base = 0, snap_dst_base = 0, boundary_base = 0;
    uint64_t max_len = 0;        // longest query of this graph (0: none)
    uint32_t n_queries = 0;
    // exact variant: bases of the graph's ExactGraph arrays (see the head of this file) and their lengths
    uint64_t sym_base = 0, off_base = 0, succ_base = 0, nbm_base = 0;
    uint32_t n_succ = 0, n_nbm = 0, n_exit = 0;
    uint32_t skew = 0;           // max over rows of dist_max - dist_min (bounds the descriptor ring, prepare_exact)
};

// The replay workspace of one slot of an exact multi-graph batch, and where the five arrays of `slots` slots lie in one buffer.
struct MultiExactSlot {
    uint32_t n_exit = 0;          // largest over the graphs that have queries
    uint32_t wpn = 1, swpn = 1;   // words per exit row for the longest query of the batch, and of the summary
    uint32_t stack_cap = 0;       // DFA stack entries (12 bytes each)
    uint32_t skew = 0;            // max over those graphs' rows of dist_max - dist_min
    uint32_t win = 64;            // descriptor ring: priorities (power of two)
    uint32_t pool_cap = 0;        // queue pool entries (16 bytes each), a multiple of 64: chunk_cap = pool_cap / 64
    uint64_t reached_stride = 0, rsum_stride = 0;   // 8-byte words per slot: n_exit x wpn, n_exit x swpn
    uint64_t bytes = 0;           // of one slot, all five arrays
    // byte offsets of the arrays of `slots` slots in one buffer, each 16-byte aligned; the last returns the buffer's size
    uint64_t off_reached(uint64_t) const { return 0; }
    uint64_t off_rsum(uint64_t slots) const { return slots * reached_stride * 8; }
    uint64_t off_stack(uint64_t slots) const { return off_rsum(slots) + slots * rsum_stride * 8; }
    uint64_t off_pool(uint64_t slots) const { return (off_stack(slots) + slots * stack_cap * 12 + 15) & ~15ull; }
    uint64_t off_ring(uint64_t slots) const { return off_pool(slots) + slots * pool_cap * 16; }
    uint64_t buffer_bytes(uint64_t slots) const { return off_ring(slots) + slots * 3 * win * 4 + 16; }
};
struct MultiExactCosts { uint32_t x = 4, o = 6, e = 2; float queue_entries_per_cell = 0.f; };   // (0: the engine's 0.25)

struct MultiPlan {
    struct Chunk { uint32_t first, count; uint64_t cells; uint64_t carry_words; uint32_t max_pitch; uint64_t table_cells; };   // table_cells: exact variant, four-byte cells of the chunk's visited tables
    uint32_t n_queries = 0;
    std::vector<MultiGraphPlan> graphs;
    uint64_t n_rows_total = 0, n_edges_total = 0, n_snap_off_total = 0, n_snap_dst_total = 0, n_boundary_total = 0;
    std::vector<uint32_t> graph_of, pitch, carry_off;   // [n]
    std::vector<uint64_t> region_off;                   // [n] 4-byte cells from the start of the query's chunk
    std::vector<uint64_t> scratch_off;                  // [n + 1] pairs
    std::vector<Chunk> chunks;
    uint64_t bytes_total = 0;           // the whole batch as one chunk
    uint64_t largest_query_bytes = 0;
    uint64_t workspace_bytes = 0;       // the largest chunk: what the batch holds
    uint64_t max_carry_words = 0;       // the largest chunk's carries
    uint64_t total_cells = 0, total_bases = 0;
    uint64_t plane_bytes = 0;           // dense: sum of 2 x compact elems, the padding left out (poa_stats_t.plane_bytes)
    // exact variant
    std::vector<uint64_t> table_off;    // [n] four-byte cells from the start of the workspace
    uint64_t n_sym_total = 0, n_off_total = 0, n_succ_total = 0, n_nbm_total = 0;
    MultiExactSlot exact;               // one slot under the plan's costs
    uint32_t exact_slots = 0;           // the largest chunk's queries
    uint64_t exact_bytes = 0;           // exact.buffer_bytes(exact_slots): counted into the footprint beside bytes_total
};

// 4-byte cells a query of `len` symbols holds on a graph with that plan, padding included
inline uint64_t multi_query_cells(const CheckpointPlan& cp, uint64_t len) {
    return (uint64_t)cp.rows_per_query * (((len + 1 + 63) / 64) * 64) + MULTI_REGION_PAD_CELLS;
}

// workspace_bytes 0: no cap (one chunk).  A cap below the largest query's footprint is raised to it.
// Returns 0, or -1 (invalid argument) / -7 (unsupported) — the values of POA_ERR_INVALID_ARG / POA_ERR_UNSUPPORTED — with `err` set.
int build_multi_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                     uint32_t segment_rows, uint64_t workspace_bytes, MultiPlan& out, std::string& err, bool two_piece = false);

constexpr uint64_t MULTI_DENSE_PAD_ELEMS = 128;     // 256 bytes behind every query's region, in two-byte elements
constexpr uint64_t MULTI_DENSE_MAX_LEN = 1023;      // one strip of the packed kernel's widest variant: pitch <= 1024

// D rows a graph keeps in the compact layout: n_store_d with a d_slot table, every row without one
inline uint32_t multi_dense_d_rows(const FlatGraph& g) { return g.d_slot.empty() ? g.n : g.n_store_d; }
// two-byte elements a query of `len` symbols holds on that graph, padding NOT included
inline uint64_t multi_dense_query_elems(const FlatGraph& g, uint64_t len) {
    return compact_plane_elems(g.n, (uint32_t)(((len + 1 + 63) / 64) * 64), multi_dense_d_rows(g));
}

// The dense plan: reads MultiGraphIn::g alone (sweep and own may be null).  Same return values as build_multi_plan.
int build_multi_dense_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                           uint64_t workspace_bytes, MultiPlan& out, std::string& err, bool wide = false);

// two-byte elements a query of `len` symbols holds on that graph in a dense two-piece batch, padding NOT included: M, I1, D1, I2, D2
inline uint64_t multi_dense2_query_elems(const FlatGraph& g, uint64_t len) { return 5ull * g.n * (((len + 1 + 63) / 64) * 64); }

// The dense two-piece plan (see the head of this file): reads MultiGraphIn::g alone.  Same return values as build_multi_plan.
int build_multi_dense2_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                            uint64_t workspace_bytes, MultiPlan& out, std::string& err);

constexpr uint64_t MULTI_EXACT_PAD_CELLS = 64;     // 256 bytes behind every query's visited table, in four-byte cells
// four-byte cells of the visited table of a query of `len` symbols on that graph, padding NOT included
inline uint64_t multi_exact_table_cells(const FlatGraph& g, uint64_t len) { return 3ull * g.n * (((len + 1 + 63) / 64) * 64); }
// THE rule for the width of the replay's descriptor ring (`win` priorities, a power of two from 64): prepare_exact,
// multi_exact_slot and the CPU harness (tests/exact_host) all call it.  bq_push (poa_exact.hpp) refuses a push that would make
// the live priorities span `win` or more, so `win` must exceed highest live priority - lowest live priority at every push:
//   jump     a pop at priority f pushes at most max(x, o + e) + o + (skew + 3) * e above f: one edit, one state change, and
//            what the min-gap heuristic can grow along one edge and the greedy extension behind it, where skew = max over rows
//            of dist_max - dist_min (heuristic.rs:70-102).  With ONE initial state this is the whole live range.
//   spread   graph_free_begin = Unbounded queues EVERY real node at offset 0 with score 0 (push_initial_states,
//            gap_affine.rs:150-163), at priority h(row, 0): 0 for a row whose [dist_min - 1, dist_max - 1] holds the query's
//            length, else o + e * (distance of the length from that interval) <= o + e * max(max_len, dist_max).  Those
//            entries stay queued while the search pops from the lowest of them upwards, so the live range is
//            [f, max(highest initial priority, f + jump)] and the ring must cover the larger of the two.  Under Dijkstra
//            order h = 0 and the spread is 0; a graph of two rows or fewer has no real node and takes the one-state branch,
//            whose `win` the jump bounds as before.
// Global runs and every other kind of graph_free_begin keep the jump term alone.
struct ExactWinIn {
    uint32_t x = 4, o = 6, e = 2;   // mismatch, gap open, gap extend
    uint32_t skew = 0;              // max over rows of dist_max - dist_min
    bool mingap = true;             // the min-gap heuristic (false: Dijkstra order)
    bool free_begin = false;        // an ends-free run whose graph_free_begin is Unbounded
    uint64_t max_len = 0;           // longest query of the batch           (read with free_begin only)
    uint32_t dist_max = 0;          // largest dist_max over the graph's rows (read with free_begin only)
};
inline uint64_t exact_replay_win_need(const ExactWinIn& in) {
    const uint64_t maxc = in.x > in.o + in.e ? in.x : in.o + in.e;
    uint64_t span = maxc + in.o + ((uint64_t)in.skew + 3) * in.e;
    if (in.free_begin && in.mingap) {
        const uint64_t far = in.max_len > in.dist_max ? in.max_len : in.dist_max;
        const uint64_t spread = in.o + far * in.e;
        if (spread > span) span = spread;
    }
    return span + 8;
}
inline uint32_t exact_replay_win(const ExactWinIn& in) {
    const uint64_t need = exact_replay_win_need(in);
    uint32_t win = 64;
    while (win < need && win < (1u << 24)) win *= 2;
    return win;
}
// the ring's width of a Global run under those costs for a graph spread `skew`
inline uint32_t multi_exact_win(uint32_t x, uint32_t o, uint32_t e, uint32_t skew) {
    ExactWinIn in;
    in.x = x; in.o = o; in.e = e; in.skew = skew;
    return exact_replay_win(in);
}

// One slot's sizes under `costs`, from what an exact plan holds of its graphs (rows, exits, spread, longest query).  The
// replay's own size limits are checked per graph as prepare_exact checks them.  Returns 0 or -7 with `err` set.
int multi_exact_slot(const MultiPlan& plan, const MultiExactCosts& costs, MultiExactSlot& out, std::string& err);

// The exact plan: build_multi_dense_plan plus the table regions, the chunks by both footprints, the ExactGraph table bases and
// the slot workspace under `costs`.  Reads MultiGraphIn::g alone; every listed graph's bubble index must be built.
int build_multi_exact_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                           uint64_t workspace_bytes, const MultiExactCosts& costs, MultiPlan& out, std::string& err, bool wide = false);

}  // namespace poa_amd
