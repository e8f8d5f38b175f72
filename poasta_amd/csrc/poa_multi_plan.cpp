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

int build_multi_dense_plan(const MultiGraphIn* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                           uint64_t workspace_bytes, MultiPlan& out, std::string& err) {
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
        if (qoff[i + 1] - qoff[i] > MULTI_DENSE_MAX_LEN) {
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
    auto elems_of = [&](uint32_t i) { return multi_dense_query_elems(*graphs[out.graph_of[i]].g, qoff[i + 1] - qoff[i]) + MULTI_DENSE_PAD_ELEMS; };
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

    // chunks: the greedy rule of build_multi_plan; the region offsets restart with every chunk
    const uint64_t budget = workspace_bytes == 0 ? out.bytes_total : std::max(workspace_bytes, out.largest_query_bytes);
    MultiPlan::Chunk cur{0, 0, 0, 0, 0};
    auto close = [&]() {
        out.chunks.push_back(cur);
        out.workspace_bytes = std::max(out.workspace_bytes, cur.cells * 2);
    };
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t elems = elems_of(i);
        if (cur.count && (cur.cells + elems) * 2 > budget) {
            close();
            cur = MultiPlan::Chunk{i, 0, 0, 0, 0};
        }
        out.region_off[i] = cur.cells;
        cur.cells += elems;
        cur.max_pitch = std::max(cur.max_pitch, out.pitch[i]);
        cur.count++;
    }
    if (cur.count) close();
    return 0;
}

}  // namespace poa_amd
