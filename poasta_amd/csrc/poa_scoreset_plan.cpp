// Plan of a score set: see poa_scoreset_plan.hpp.
#include "poa_scoreset_plan.hpp"

#include <algorithm>

namespace poa_amd {

namespace {
constexpr int ERR_INVALID_ARG = -1, ERR_UNSUPPORTED = -7;   // POA_ERR_INVALID_ARG, POA_ERR_UNSUPPORTED (include/poasta_amd.h)
}

int build_scoreset_plan(const ScoreSetGraphIn* graphs, uint32_t n_graphs, uint32_t n_queries, const uint64_t* qoff, uint64_t n_pairs,
                        const uint32_t* pair_query, const uint32_t* pair_graph, uint64_t workspace_bytes, ScoreSetPlan& out,
                        std::string& err) {
    out = ScoreSetPlan();
    if (!qoff || (n_graphs && !graphs)) { err = "score set: null argument"; return ERR_INVALID_ARG; }
    const bool matrix = !pair_query && !pair_graph;
    if (!matrix && (!pair_query || !pair_graph)) { err = "score set: one of pair_query / pair_graph is null"; return ERR_INVALID_ARG; }
    if (matrix && n_pairs != 0 && n_pairs != (uint64_t)n_queries * n_graphs) {
        err = "score set: without pair arrays n_pairs must be n_queries * n_graphs (the full matrix)";
        return ERR_INVALID_ARG;
    }
    if (n_pairs > 0xFFFFFFF0ull) { err = "score set: n_pairs is not a pair count a set can hold"; return ERR_INVALID_ARG; }
    for (uint32_t g = 0; g < n_graphs; ++g)
        if (!graphs[g].g || !graphs[g].sweep) { err = "score set: null graph"; return ERR_INVALID_ARG; }
    for (uint32_t i = 0; i < n_queries; ++i) {
        if (qoff[i + 1] < qoff[i]) { err = "score set: qoff not monotone"; return ERR_INVALID_ARG; }
        if (qoff[i + 1] - qoff[i] > 0x7FFFFFF0ull) { err = "query longer than 2^31"; return ERR_UNSUPPORTED; }
    }
    const uint32_t n = (uint32_t)n_pairs;
    if (!matrix)
        for (uint32_t p = 0; p < n; ++p)
            if (pair_query[p] >= n_queries || pair_graph[p] >= n_graphs) {
                err = "score set: pair " + std::to_string(p) + " names a query or a graph out of range";
                return ERR_INVALID_ARG;
            }
    out.n_queries = n_queries; out.n_pairs = n;
    out.graphs.resize(n_graphs);
    out.pair_graph.resize(n); out.pair_query.resize(n); out.pitch.resize(n); out.carry_off.resize(n); out.region_off.resize(n);

    for (uint32_t g = 0; g < n_graphs; ++g) {
        ScoreSetGraphPlan& gp = out.graphs[g];
        const ScoreSetGraphIn& in = graphs[g];
        gp.table_of = g;
        for (uint32_t h = 0; h < g; ++h)
            if (graphs[h].g == in.g) { gp.table_of = h; break; }
        gp.n_rows = in.g->n; gp.n_edges = (uint32_t)in.g->pred_rows.size();
        gp.n_slots = in.sweep->n_slots; gp.n_slotted = in.sweep->n_slotted;
        gp.empty = in.g->n_real == 0;
        if (gp.table_of != g) {
            gp.row_base = out.graphs[gp.table_of].row_base; gp.edge_base = out.graphs[gp.table_of].edge_base;
        } else {
            gp.row_base = out.n_rows_total; gp.edge_base = out.n_edges_total;
            out.n_rows_total += gp.n_rows; out.n_edges_total += gp.n_edges;
        }
    }

    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t qi = matrix ? p / n_graphs : pair_query[p], gi = matrix ? p % n_graphs : pair_graph[p];
        ScoreSetGraphPlan& gp = out.graphs[gi];
        const uint64_t L = qoff[qi + 1] - qoff[qi];
        out.pair_query[p] = qi; out.pair_graph[p] = gi;
        out.pitch[p] = (uint32_t)(((L + 1 + 63) / 64) * 64);
        gp.max_len = std::max(gp.max_len, L);
        gp.n_pairs++;
        const uint64_t bytes = scoreset_pair_cells(gp.n_slots, L) * 4;
        out.bytes_total += bytes;
        out.largest_pair_bytes = std::max(out.largest_pair_bytes, bytes);
        out.total_bases += L;
        out.total_cells += (uint64_t)gp.n_rows * (L + 1);
        if (!gp.empty) {   // (a pair against a graph without real nodes stores nothing)
            const bool px = scoreset_class(SS_VAR_U16_PX, out.pitch[p]) == SS_CLASS_PX;
            out.slotted_pitch_all += (uint64_t)gp.n_slotted * out.pitch[p];
            if (px) out.slotted_px += gp.n_slotted;
            else out.slotted_pitch += (uint64_t)gp.n_slotted * out.pitch[p];
        }
    }

    // chunks: greedy in pair order; the region and carry offsets restart with every chunk
    const uint64_t budget = workspace_bytes == 0 ? out.bytes_total : std::max(workspace_bytes, out.largest_pair_bytes);
    ScoreSetPlan::Chunk cur{};
    auto close = [&]() {
        out.chunks.push_back(cur);
        out.workspace_bytes = std::max(out.workspace_bytes, cur.cells * 4);
        out.max_carry_words = std::max(out.max_carry_words, cur.carry_words);
    };
    for (uint32_t p = 0; p < n; ++p) {
        const ScoreSetGraphPlan& gp = out.graphs[out.pair_graph[p]];
        const uint32_t qi = out.pair_query[p];
        const uint64_t cells = scoreset_pair_cells(gp.n_slots, qoff[qi + 1] - qoff[qi]);
        if (cur.count && (cur.cells + cells) * 4 > budget) {
            close();
            cur = ScoreSetPlan::Chunk{};
            cur.first = p;
        }
        out.region_off[p] = cur.cells;
        cur.cells += cells;
        const uint64_t cw = out.pitch[p] > SCORESET_STRIP_COLUMNS ? 4ull * gp.n_rows : 0ull;
        if (cur.carry_words + cw > 0xFFFFFFFFull) {
            err = "score set: the strip carries of one chunk exceed 2^32 words; cap workspace_bytes";
            return ERR_UNSUPPORTED;
        }
        out.carry_off[p] = (uint32_t)cur.carry_words;
        cur.carry_words += cw;
        cur.count++;
    }
    if (cur.count) close();

    // kernel classes: per variant the pairs of every chunk, class by class, in pair order inside a class
    for (uint32_t v = 0; v < SS_N_VARIANTS; ++v) {
        std::vector<uint32_t>& list = out.class_list[v];
        list.resize(n);
        for (ScoreSetPlan::Chunk& ch : out.chunks) {
            uint32_t count[SS_N_CLASSES] = {};
            for (uint32_t p = ch.first; p < ch.first + ch.count; ++p) count[scoreset_class(v, out.pitch[p])]++;
            uint32_t at[SS_N_CLASSES];
            ch.class_begin[v][0] = ch.first;
            for (uint32_t c = 0; c < SS_N_CLASSES; ++c) {
                at[c] = ch.class_begin[v][c];
                ch.class_begin[v][c + 1] = ch.class_begin[v][c] + count[c];
            }
            for (uint32_t p = ch.first; p < ch.first + ch.count; ++p) list[at[scoreset_class(v, out.pitch[p])]++] = p;
        }
    }
    return 0;
}

void build_scoreset_best_order(ScoreSetPlan& plan) {
    const uint32_t n = plan.n_pairs, nq = plan.n_queries;
    plan.query_off.assign((size_t)nq + 1, 0);
    plan.query_pairs.resize(n);
    for (uint32_t p = 0; p < n; ++p) plan.query_off[plan.pair_query[p] + 1]++;
    for (uint32_t q = 0; q < nq; ++q) plan.query_off[q + 1] += plan.query_off[q];
    std::vector<uint32_t> rank(n), seen(nq, 0);
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t q = plan.pair_query[p];
        rank[p] = seen[q]++;
        plan.query_pairs[plan.query_off[q] + rank[p]] = p;
    }
    for (uint32_t v = 0; v < SS_N_VARIANTS; ++v) {
        std::vector<uint32_t>& list = plan.best_list[v];
        list = plan.class_list[v];
        for (const ScoreSetPlan::Chunk& ch : plan.chunks)
            for (uint32_t c = 0; c < SS_N_CLASSES; ++c)
                std::sort(list.begin() + ch.class_begin[v][c], list.begin() + ch.class_begin[v][c + 1],
                          [&](uint32_t a, uint32_t b) { return rank[a] != rank[b] ? rank[a] < rank[b] : a < b; });
    }
}

}  // namespace poa_amd
