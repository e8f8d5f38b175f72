// Plan of a multi-graph checkpointed batch: see poa_multi_plan.hpp.
#include "poa_multi_plan.hpp"

#include <algorithm>

namespace poa_amd {

namespace {
constexpr int ERR_INVALID_ARG = -1, ERR_UNSUPPORTED = -7;   // POA_ERR_INVALID_ARG, POA_ERR_UNSUPPORTED (include/poasta_amd.h)
}

int build_multi_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                     uint32_t segment_rows, uint64_t workspace_bytes, MultiPlan& out, std::string& err, bool two_piece) {
    out = MultiPlan();
    if (!graph_qoff || !qoff || (n_graphs && !graphs)) { err = "multi-graph batch: null argument"; return ERR_INVALID_ARG; }
    if (graph_qoff[0] != 0) { err = "multi-graph batch: graph_qoff[0] is not 0"; return ERR_INVALID_ARG; }
    for (uint32_t g = 0; g < n_graphs; ++g) {
        if (!graphs[g].g || !graphs[g].sweep || !graphs[g].own) { err = "multi-graph batch: null graph"; return ERR_INVALID_ARG; }
        if (graph_qoff[g + 1] < graph_qoff[g]) { err = "multi-graph batch: graph_qoff is not non-decreasing"; return ERR_INVALID_ARG; }
    }
    if (graph_qoff[n_graphs] > 0xFFFFFFF0ull) { err = "multi-graph batch: graph_qoff[n_graphs] is not a query count a batch can hold"; return ERR_INVALID_ARG; }
    const uint32_t n = (uint32_t)graph_qoff[n_graphs];
    for (uint32_t i = 0; i < n; ++i) {
        if (qoff[i + 1] < qoff[i]) { err = "multi-graph batch: qoff not monotone"; return ERR_INVALID_ARG; }
        if (qoff[i + 1] - qoff[i] > 0x7FFFFFF0ull) { err = "query longer than 2^31"; return ERR_UNSUPPORTED; }
    }
    out.n_queries = n;
    out.graphs.resize(n_graphs);
    out.graph_of.resize(n); out.pitch.resize(n); out.carry_off.resize(n); out.region_off.resize(n);
    out.scratch_off.resize((size_t)n + 1);

    for (uint32_t g = 0; g < n_graphs; ++g) {
        MultiGraphPlan& gp = out.graphs[g];
        const MultiGraphIn& in = graphs[g];
        gp.table_of = g;
        for (uint32_t h = 0; h < g; ++h)
            if (graphs[h].g == in.g) { gp.table_of = h; break; }
        gp.n_rows = in.g->n; gp.n_edges = (uint32_t)in.g->pred_rows.size(); gp.n_slots = in.sweep->n_slots;
        gp.n_queries = (uint32_t)(graph_qoff[g + 1] - graph_qoff[g]);
        if (gp.table_of != g) {
            const MultiGraphPlan& first = out.graphs[gp.table_of];
            gp.ckpt = first.ckpt;
            gp.row_base = first.row_base; gp.edge_base = first.edge_base; gp.snap_off_base = first.snap_off_base;
            gp.snap_dst_base = first.snap_dst_base; gp.boundary_base = first.boundary_base;
        } else {
            if (segment_rows == 0 || segment_rows == in.own->segment_rows) gp.ckpt = *in.own;
            else build_checkpoint_plan(*in.g, *in.sweep, segment_rows, gp.ckpt, two_piece);
            gp.row_base = out.n_rows_total; gp.edge_base = out.n_edges_total; gp.snap_off_base = out.n_snap_off_total;
            gp.snap_dst_base = out.n_snap_dst_total; gp.boundary_base = out.n_boundary_total;
            out.n_rows_total += gp.n_rows; out.n_edges_total += gp.n_edges; out.n_snap_off_total += gp.ckpt.snap_off.size();
            out.n_snap_dst_total += gp.ckpt.snap_dst.size(); out.n_boundary_total += gp.ckpt.boundary.size();
        }
        for (uint64_t i = graph_qoff[g]; i < graph_qoff[g + 1]; ++i) {
            const uint64_t L = qoff[i + 1] - qoff[i];
            out.graph_of[i] = g;
            out.pitch[i] = (uint32_t)(((L + 1 + 63) / 64) * 64);
            gp.max_len = std::max(gp.max_len, L);
        }
    }

    uint64_t scratch = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const MultiGraphPlan& gp = out.graphs[out.graph_of[i]];
        const uint64_t L = qoff[i + 1] - qoff[i];
        const uint64_t bytes = multi_query_cells(gp.ckpt, L) * 4;
        out.bytes_total += bytes;
        out.largest_query_bytes = std::max(out.largest_query_bytes, bytes);
        out.scratch_off[i] = scratch;
        scratch += L + gp.n_rows;
        out.total_bases += L;
        out.total_cells += (uint64_t)gp.n_rows * (L + 1);
    }
    out.scratch_off[n] = scratch;

    // chunks: greedy in query order; the region and carry offsets restart with every chunk
    const uint64_t budget = workspace_bytes == 0 ? out.bytes_total : std::max(workspace_bytes, out.largest_query_bytes);
    MultiPlan::Chunk cur{0, 0, 0, 0, 0};
    auto close = [&]() {
        out.chunks.push_back(cur);
        out.workspace_bytes = std::max(out.workspace_bytes, cur.cells * 4);
        out.max_carry_words = std::max(out.max_carry_words, cur.carry_words);
    };
    for (uint32_t i = 0; i < n; ++i) {
        const MultiGraphPlan& gp = out.graphs[out.graph_of[i]];
        const uint64_t cells = multi_query_cells(gp.ckpt, qoff[i + 1] - qoff[i]);
        if (cur.count && (cur.cells + cells) * 4 > budget) {
            close();
            cur = MultiPlan::Chunk{i, 0, 0, 0, 0};
        }
        out.region_off[i] = cur.cells;
        cur.cells += cells;
        // two parities of two words per row (ckpt_rows), of three under the two-piece model (ckpt2_rows)
        const uint64_t cw = out.pitch[i] > MULTI_STRIP_COLUMNS ? (two_piece ? 6ull : 4ull) * gp.n_rows : 0ull;
        if (cur.carry_words + cw > 0xFFFFFFFFull) {
            err = "multi-graph batch: the strip carries of one chunk exceed 2^32 words; cap workspace_bytes";
            return ERR_UNSUPPORTED;
        }
        out.carry_off[i] = (uint32_t)cur.carry_words;
        cur.carry_words += cw;
        cur.max_pitch = std::max(cur.max_pitch, out.pitch[i]);
        cur.count++;
    }
    if (cur.count) close();
    return 0;
}

namespace {
// strip carries of a wide dense or exact query: two words per row (forward_packed_strips: the insertion-scan carry and I of the
// strip's last column), for a query wider than one strip only.  The checkpointed kinds' rule with the packed kernel's words.
inline uint64_t dense_carry_words(uint32_t pitch, uint32_t n_rows) { return pitch > MULTI_STRIP_COLUMNS ? 2ull * n_rows : 0ull; }
const char* const DENSE_CARRY_OVERFLOW = "multi-graph batch: the strip carries of one chunk exceed 2^32 words; cap workspace_bytes";

// build_multi_dense_plan; `carries` false: the chunks' carries are left to the caller (the exact plan cuts its own chunks).
// `five_planes`: build_multi_dense2_plan — the same plan over five full u16 planes per query; called with `wide` set (any
// length) and `carries` not (the two-piece pass hands nothing from strip to strip).
int dense_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
               uint64_t workspace_bytes, MultiPlan& out, std::string& err, bool wide, bool carries, bool five_planes = false) {
    out = MultiPlan();
    if (!graph_qoff || !qoff || (n_graphs && !graphs)) { err = "dense multi-graph batch: null argument"; return ERR_INVALID_ARG; }
    if (graph_qoff[0] != 0) { err = "dense multi-graph batch: graph_qoff[0] is not 0"; return ERR_INVALID_ARG; }
    for (uint32_t g = 0; g < n_graphs; ++g) {
        if (!graphs[g].g) { err = "dense multi-graph batch: null graph"; return ERR_INVALID_ARG; }
        if (graph_qoff[g + 1] < graph_qoff[g]) { err = "dense multi-graph batch: graph_qoff is not non-decreasing"; return ERR_INVALID_ARG; }
    }
    if (graph_qoff[n_graphs] > 0xFFFFFFF0ull) { err = "dense multi-graph batch: graph_qoff[n_graphs] is not a query count a batch can hold"; return ERR_INVALID_ARG; }
    const uint32_t n = (uint32_t)graph_qoff[n_graphs];
    for (uint32_t i = 0; i < n; ++i) {
        if (qoff[i + 1] < qoff[i]) { err = "dense multi-graph batch: qoff not monotone"; return ERR_INVALID_ARG; }
        if (wide && qoff[i + 1] - qoff[i] > 0x7FFFFFF0ull) { err = "query longer than 2^31"; return ERR_UNSUPPORTED; }
        if (!wide && qoff[i + 1] - qoff[i] > MULTI_DENSE_MAX_LEN) {
            err = "dense multi-graph batch: a query of more than 1023 symbols is wider than one strip of the packed forward pass; "
                  "the checkpointed batch (poa_multi_create) takes queries of any length";
            return ERR_UNSUPPORTED;
        }
    }
    out.n_queries = n;
    out.graphs.resize(n_graphs);
    out.graph_of.resize(n); out.pitch.resize(n); out.carry_off.assign(n, 0u); out.region_off.resize(n);
    out.scratch_off.resize((size_t)n + 1);

    for (uint32_t g = 0; g < n_graphs; ++g) {
        MultiGraphPlan& gp = out.graphs[g];
        const FlatGraph& fg = *graphs[g].g;
        gp.table_of = g;
        for (uint32_t h = 0; h < g; ++h)
            if (graphs[h].g == graphs[g].g) { gp.table_of = h; break; }
        gp.n_rows = fg.n; gp.n_edges = (uint32_t)fg.pred_rows.size();
        gp.n_queries = (uint32_t)(graph_qoff[g + 1] - graph_qoff[g]);
        if (gp.table_of != g) {
            gp.row_base = out.graphs[gp.table_of].row_base; gp.edge_base = out.graphs[gp.table_of].edge_base;
        } else {
            gp.row_base = out.n_rows_total; gp.edge_base = out.n_edges_total;
            out.n_rows_total += gp.n_rows; out.n_edges_total += gp.n_edges;
        }
        for (uint64_t i = graph_qoff[g]; i < graph_qoff[g + 1]; ++i) {
            const uint64_t L = qoff[i + 1] - qoff[i];
            out.graph_of[i] = g;
            out.pitch[i] = (uint32_t)(((L + 1 + 63) / 64) * 64);
            gp.max_len = std::max(gp.max_len, L);
        }
    }

    // per query: its compact planes and the padding, in two-byte elements
    auto elems_of = [&](uint32_t i) {
        const FlatGraph& fg = *graphs[out.graph_of[i]].g;
        const uint64_t L = qoff[i + 1] - qoff[i];
        return (five_planes ? multi_dense2_query_elems(fg, L) : multi_dense_query_elems(fg, L)) + MULTI_DENSE_PAD_ELEMS;
    };
    uint64_t scratch = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const MultiGraphPlan& gp = out.graphs[out.graph_of[i]];
        const uint64_t L = qoff[i + 1] - qoff[i];
        const uint64_t bytes = elems_of(i) * 2;
        out.bytes_total += bytes;
        out.plane_bytes += bytes - MULTI_DENSE_PAD_ELEMS * 2;
        out.largest_query_bytes = std::max(out.largest_query_bytes, bytes);
        out.scratch_off[i] = scratch;
        scratch += L + gp.n_rows;
        out.total_bases += L;
        out.total_cells += (uint64_t)gp.n_rows * (L + 1);
    }
    out.scratch_off[n] = scratch;

    // chunks: the greedy rule of build_multi_plan; the region and carry offsets restart with every chunk
    const uint64_t budget = workspace_bytes == 0 ? out.bytes_total : std::max(workspace_bytes, out.largest_query_bytes);
    MultiPlan::Chunk cur{0, 0, 0, 0, 0};
    auto close = [&]() {
        out.chunks.push_back(cur);
        out.workspace_bytes = std::max(out.workspace_bytes, cur.cells * 2);
        out.max_carry_words = std::max(out.max_carry_words, cur.carry_words);
    };
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t elems = elems_of(i);
        if (cur.count && (cur.cells + elems) * 2 > budget) {
            close();
            cur = MultiPlan::Chunk{i, 0, 0, 0, 0};
        }
        out.region_off[i] = cur.cells;
        cur.cells += elems;
        const uint64_t cw = carries ? dense_carry_words(out.pitch[i], out.graphs[out.graph_of[i]].n_rows) : 0ull;   // (0 without `wide`: every pitch <= 1024)
        if (cur.carry_words + cw > 0xFFFFFFFFull) { err = std::string("dense ") + DENSE_CARRY_OVERFLOW; return ERR_UNSUPPORTED; }
        out.carry_off[i] = (uint32_t)cur.carry_words;
        cur.carry_words += cw;
        cur.max_pitch = std::max(cur.max_pitch, out.pitch[i]);
        cur.count++;
    }
    if (cur.count) close();
    return 0;
}
}  // namespace

int build_multi_dense_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                           uint64_t workspace_bytes, MultiPlan& out, std::string& err, bool wide) {
    return dense_plan(graphs, n_graphs, graph_qoff, qoff, workspace_bytes, out, err, wide, true);
}

int build_multi_dense2_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                            uint64_t workspace_bytes, MultiPlan& out, std::string& err) {
    return dense_plan(graphs, n_graphs, graph_qoff, qoff, workspace_bytes, out, err, true, false, true);
}

int multi_exact_slot(const MultiPlan& plan, const MultiExactCosts& costs, MultiExactSlot& out, std::string& err) {
    out = MultiExactSlot();
    const uint64_t maxc = std::max<uint64_t>(costs.x, (uint64_t)costs.o + costs.e);
    const float f = costs.queue_entries_per_cell > 0.f ? costs.queue_entries_per_cell : 0.25f;
    uint64_t max_len = 0, pool64 = 256, stack = 8;
    for (size_t g = 0; g < plan.graphs.size(); ++g) {
        const MultiGraphPlan& gp = plan.graphs[g];
        if (!gp.n_queries) continue;
        const uint64_t n = gp.n_rows, len = gp.max_len;
        // the replay's own size limits, per graph (prepare_exact)
        const uint64_t n_prio = (n + len + 2) * maxc + costs.o + (n + len) * costs.e + 64;
        if (n_prio > (1ull << 26)) { err = "exact multi-graph batch: priority range too large for a graph / query size (poa_align_batch_ex refuses it too)"; return ERR_UNSUPPORTED; }
        if (3ull * n * ((len + 64) & ~63ull) >= (1ull << 32)) { err = "exact multi-graph batch: the visited table of one query exceeds 2^32 cells (poa_align_batch_ex refuses it too)"; return ERR_UNSUPPORTED; }
        if ((uint64_t)gp.n_exit * ((len + 64) / 64) >= (1ull << 32)) { err = "exact multi-graph batch: reached sets of one query exceed 2^32 words (poa_align_batch_ex refuses it too)"; return ERR_UNSUPPORTED; }
        out.skew = std::max(out.skew, gp.skew);
        out.n_exit = std::max(out.n_exit, gp.n_exit);
        max_len = std::max(max_len, len);
        stack = std::max(stack, n + len + 8);
        pool64 = std::max<uint64_t>(pool64, (uint64_t)(f * (double)n * (double)(len + 1)));
    }
    out.win = multi_exact_win(costs.x, costs.o, costs.e, out.skew);
    const uint64_t pool_ws = (pool64 + (uint64_t)64 * (3ull * out.win + 8) + 63) & ~63ull;   // BQ_CHUNK = 64 entries per chunk
    if (pool_ws > 0xFFFFFFF0ull) { err = "exact multi-graph batch: queue pool too large (lower queue_entries_per_cell, or poa_align_batch_ex per graph)"; return ERR_UNSUPPORTED; }
    out.pool_cap = (uint32_t)pool_ws;
    out.stack_cap = (uint32_t)stack;
    out.wpn = (uint32_t)((max_len + 1 + 63) / 64);
    out.swpn = (out.wpn + 63) / 64;
    out.reached_stride = ((uint64_t)out.n_exit * out.wpn + 1) & ~1ull;   // (an even count of 8-byte words: every slot 16-byte aligned)
    out.rsum_stride = ((uint64_t)out.n_exit * out.swpn + 1) & ~1ull;
    out.bytes = out.reached_stride * 8 + out.rsum_stride * 8 + (uint64_t)out.stack_cap * 12 + (uint64_t)out.pool_cap * 16 + 3ull * out.win * 4;
    return 0;
}

int build_multi_exact_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                           uint64_t workspace_bytes, const MultiExactCosts& costs, MultiPlan& out, std::string& err, bool wide) {
    // the dense plan as one chunk: the argument checks, the graphs' row and edge bases, pitches, pair scratch, the totals
    // (the carries belong to the chunks cut below)
    if (const int rc = dense_plan(graphs, n_graphs, graph_qoff, qoff, 0, out, err, wide, false)) {
        if (rc == ERR_UNSUPPORTED && !wide) err = "exact multi-graph batch: a query of more than 1023 symbols is wider than one strip of the packed forward pass; "
                                         "poa_align_batch_ex takes queries of any length, one graph at a time";
        return rc;
    }
    const uint32_t n = out.n_queries;
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const FlatGraph& fg = *graphs[g].g;
        if (!fg.bubbles_built) { err = "exact multi-graph batch: a graph's bubble index is not built"; return ERR_INVALID_ARG; }
        MultiGraphPlan& gp = out.graphs[g];
        gp.n_succ = (uint32_t)fg.succ_rows.size(); gp.n_nbm = (uint32_t)fg.nbm.size(); gp.n_exit = fg.n_exit;
        for (uint32_t r = 0; r < fg.n; ++r) gp.skew = std::max<uint32_t>(gp.skew, fg.dist_max[r] - std::min(fg.dist_min[r], fg.dist_max[r]));
        if (gp.table_of != g) {
            const MultiGraphPlan& first = out.graphs[gp.table_of];
            gp.sym_base = first.sym_base; gp.off_base = first.off_base; gp.succ_base = first.succ_base; gp.nbm_base = first.nbm_base;
        } else {
            gp.sym_base = out.n_sym_total; gp.off_base = out.n_off_total; gp.succ_base = out.n_succ_total; gp.nbm_base = out.n_nbm_total;
            out.n_sym_total += ((uint64_t)fg.n + 4 + 3) & ~3ull;   // the staging loop reads whole words
            out.n_off_total += (uint64_t)fg.n + 1; out.n_succ_total += gp.n_succ; out.n_nbm_total += gp.n_nbm;
        }
    }
    if (const int rc = multi_exact_slot(out, costs, out.exact, err)) return rc;

    auto dense_elems = [&](uint32_t i) { return multi_dense_query_elems(*graphs[out.graph_of[i]].g, qoff[i + 1] - qoff[i]) + MULTI_DENSE_PAD_ELEMS; };
    auto table_cells = [&](uint32_t i) { return multi_exact_table_cells(*graphs[out.graph_of[i]].g, qoff[i + 1] - qoff[i]) + MULTI_EXACT_PAD_CELLS; };
    out.bytes_total = 0; out.largest_query_bytes = 0; out.workspace_bytes = 0; out.max_carry_words = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t bytes = dense_elems(i) * 2 + table_cells(i) * 4;
        out.bytes_total += bytes;
        out.largest_query_bytes = std::max(out.largest_query_bytes, bytes);
    }
    // chunks: greedy by the sum of both footprints; the dense regions first, the tables behind them
    out.chunks.clear();
    out.table_off.assign(n, 0);
    const uint64_t budget = workspace_bytes == 0 ? out.bytes_total : std::max(workspace_bytes, out.largest_query_bytes);
    MultiPlan::Chunk cur{0, 0, 0, 0, 0, 0};
    auto close = [&]() {
        // (cells is a multiple of 16 two-byte elements: every part of a compact region is, and so is the padding)
        for (uint32_t i = cur.first; i < cur.first + cur.count; ++i) out.table_off[i] += cur.cells / 2;
        out.chunks.push_back(cur);
        out.workspace_bytes = std::max(out.workspace_bytes, cur.cells * 2 + cur.table_cells * 4);
        out.max_carry_words = std::max(out.max_carry_words, cur.carry_words);
        out.exact_slots = std::max(out.exact_slots, cur.count);
    };
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t elems = dense_elems(i), cells = table_cells(i);
        if (cur.count && (cur.cells + elems) * 2 + (cur.table_cells + cells) * 4 > budget) {
            close();
            cur = MultiPlan::Chunk{i, 0, 0, 0, 0, 0};
        }
        out.region_off[i] = cur.cells;
        out.table_off[i] = cur.table_cells;
        cur.cells += elems;
        cur.table_cells += cells;
        const uint64_t cw = dense_carry_words(out.pitch[i], out.graphs[out.graph_of[i]].n_rows);
        if (cur.carry_words + cw > 0xFFFFFFFFull) { err = std::string("exact ") + DENSE_CARRY_OVERFLOW; return ERR_UNSUPPORTED; }
        out.carry_off[i] = (uint32_t)cur.carry_words;
        cur.carry_words += cw;
        cur.max_pitch = std::max(cur.max_pitch, out.pitch[i]);
        cur.count++;
    }
    if (cur.count) close();
    out.exact_bytes = n ? out.exact.buffer_bytes(out.exact_slots) : 0;
    return 0;
}

}  // namespace poa_amd
