// Stand-alone check of the multi-graph plan under the two-piece model (poasta_amd/csrc/poa_multi_plan.cpp, two_piece = true):
// built by tests/test_multi_plan_2piece.py together with the plan, the sweep rows and the graph flattening under
// -fsanitize=address,undefined, and run on the CPU.  It plans the shapes of tests/test_multi_graph_2piece.py (tests 1-3) and
// checks what the kernels of poa_multi.hpp rely on: every offset in bounds, the regions of a chunk disjoint, the chunks
// covering every query exactly once, six carry words per graph row for a query wider than one strip and none for the others.
// Exit code 0 and "multi_host2 ok" on success.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../poasta_amd/csrc/poa_multi_plan.hpp"

using namespace poa_amd;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "multi_host2: line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

struct Builder {   // node 0: start '#', node 1: end '$'; finish() wires nodes without predecessors / successors to them
    std::vector<uint8_t> sym{'#', '$'};
    std::vector<std::vector<uint32_t>> succ{{}, {}}, pred{{}, {}};
    uint32_t node(uint8_t s) { sym.push_back(s); succ.emplace_back(); pred.emplace_back(); return (uint32_t)sym.size() - 1; }
    void edge(uint32_t a, uint32_t b) { succ[a].push_back(b); pred[b].push_back(a); }
    std::vector<uint32_t> path(uint32_t n, uint32_t seed) {
        std::vector<uint32_t> ids;
        for (uint32_t i = 0; i < n; ++i) {
            ids.push_back(node("ACGT"[(seed + 3 * i + i / 5) & 3]));
            if (i) edge(ids[i - 1], ids[i]);
        }
        return ids;
    }
};

struct Graph {
    FlatGraph g;
    SweepRows sweep;
    CheckpointPlan own2;   // the handle's two-piece plan at the engine's own segment length
};

void finish(Builder& b, Graph& out) {
    const uint32_t n = (uint32_t)b.sym.size();
    for (uint32_t v = 2; v < n; ++v) if (b.pred[v].empty()) b.edge(0, v);
    for (uint32_t v = 2; v < n; ++v) if (b.succ[v].empty()) b.edge(v, 1);
    std::vector<uint32_t> so(n + 1, 0), po(n + 1, 0), s, p;
    for (uint32_t v = 0; v < n; ++v) {
        so[v + 1] = so[v] + (uint32_t)b.succ[v].size();
        po[v + 1] = po[v] + (uint32_t)b.pred[v].size();
        s.insert(s.end(), b.succ[v].begin(), b.succ[v].end());
        p.insert(p.end(), b.pred[v].begin(), b.pred[v].end());
    }
    std::string err;
    const int rc = build_flat_graph(n, 0, 1, b.sym.data(), so.data(), s.data(), po.data(), p.data(), out.g, err);
    if (rc != 0) { std::fprintf(stderr, "multi_host2: build_flat_graph: %s\n", err.c_str()); std::exit(1); }
    build_sweep_rows(out.g, out.sweep);
    build_checkpoint_plan(out.g, out.sweep, 0, out.own2, true);
}

void check_plan(const std::vector<MultiGraphIn>& in, const std::vector<uint64_t>& gq, const std::vector<uint64_t>& qoff, uint32_t seg_rows,
                uint64_t ws, const MultiPlan& pl) {
    const uint32_t n_graphs = (uint32_t)in.size(), n = (uint32_t)qoff.size() - 1;
    CHECK(pl.n_queries == n && pl.graphs.size() == n_graphs);
    // per graph: the two-piece plan of the graph alone, and table ranges in bounds; distinct handles do not overlap, equal ones share
    std::vector<std::pair<uint64_t, uint64_t>> row_ranges;
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const MultiGraphPlan& gp = pl.graphs[g];
        CheckpointPlan alone;
        build_checkpoint_plan(*in[g].g, *in[g].sweep, seg_rows, alone, true);
        CHECK(gp.ckpt.rows_per_query == alone.rows_per_query && gp.ckpt.boundary == alone.boundary && gp.ckpt.pred_src == alone.pred_src);
        CHECK(gp.ckpt.snap_off == alone.snap_off && gp.ckpt.snap_dst == alone.snap_dst);
        CHECK(gp.ckpt.rows_per_query == 3 * gp.n_slots + 3 * gp.ckpt.n_snap_rows + 5 * gp.ckpt.max_segment);
        CHECK(gp.n_rows == in[g].g->n && gp.n_edges == in[g].g->pred_rows.size());
        CHECK(gp.row_base + gp.n_rows <= pl.n_rows_total && gp.edge_base + gp.n_edges <= pl.n_edges_total);
        CHECK(gp.snap_off_base + gp.n_rows + 1 <= pl.n_snap_off_total && gp.snap_dst_base + gp.ckpt.snap_dst.size() <= pl.n_snap_dst_total);
        CHECK(gp.boundary_base + gp.ckpt.n_segments() + 1 <= pl.n_boundary_total);
        CHECK(gp.ckpt.snap_off.back() == gp.ckpt.snap_dst.size());
        for (uint32_t d : gp.ckpt.snap_dst) CHECK(d < std::max(gp.ckpt.n_snap_rows, 1u));
        for (size_t s = 0; s + 1 < gp.ckpt.boundary.size(); ++s) CHECK(gp.ckpt.boundary[s + 1] - gp.ckpt.boundary[s] <= gp.ckpt.max_segment);
        CHECK(gp.table_of <= g && in[gp.table_of].g == in[g].g);
        if (gp.table_of == g) row_ranges.push_back({gp.row_base, gp.row_base + gp.n_rows});
        else CHECK(gp.row_base == pl.graphs[gp.table_of].row_base && gp.edge_base == pl.graphs[gp.table_of].edge_base);
        CHECK(gp.n_queries == gq[g + 1] - gq[g]);
    }
    std::sort(row_ranges.begin(), row_ranges.end());
    for (size_t k = 1; k < row_ranges.size(); ++k) CHECK(row_ranges[k - 1].second <= row_ranges[k].first);
    CHECK(row_ranges.empty() || row_ranges.back().second == pl.n_rows_total);

    // per query
    uint64_t total = 0, largest = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t g = pl.graph_of[i];
        CHECK(g < n_graphs && i >= gq[g] && i < gq[g + 1]);
        const uint64_t L = qoff[i + 1] - qoff[i];
        CHECK(pl.pitch[i] % 64 == 0 && pl.pitch[i] >= L + 1 && pl.pitch[i] < L + 1 + 64);
        const uint64_t bytes = ((uint64_t)pl.graphs[g].ckpt.rows_per_query * pl.pitch[i]) * 4 + 256;
        CHECK(bytes == multi_query_cells(pl.graphs[g].ckpt, L) * 4);
        total += bytes; largest = std::max(largest, bytes);
        CHECK(pl.scratch_off[i + 1] - pl.scratch_off[i] == L + pl.graphs[g].n_rows);
    }
    CHECK(pl.scratch_off[0] == 0);
    CHECK(total == pl.bytes_total && largest == pl.largest_query_bytes);

    // chunks: exact coverage, everything inside the workspace and the carry buffer, nothing overlapping
    const uint64_t budget = ws == 0 ? total : std::max(ws, largest);
    uint32_t next = 0;
    uint64_t max_bytes = 0, max_carry = 0;
    for (size_t c = 0; c < pl.chunks.size(); ++c) {
        const MultiPlan::Chunk& ch = pl.chunks[c];
        CHECK(ch.first == next && ch.count > 0);
        next += ch.count;
        CHECK(ch.cells * 4 <= budget && ch.cells * 4 <= pl.workspace_bytes);
        uint64_t end = 0, carry_end = 0;
        uint32_t max_pitch = 0;
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
            const MultiGraphPlan& gp = pl.graphs[pl.graph_of[i]];
            CHECK(pl.region_off[i] == end && pl.region_off[i] % 64 == 0);   // back to back: disjoint; 256-byte aligned (128 for u16 cells)
            // the last cell the kernels address (Ckpt2Region): three slot planes, three snapshot planes, five window planes
            const uint64_t used = (3ull * gp.n_slots + 3ull * gp.ckpt.n_snap_rows + 5ull * gp.ckpt.max_segment) * pl.pitch[i];
            end += multi_query_cells(gp.ckpt, qoff[i + 1] - qoff[i]);
            CHECK(pl.region_off[i] + used <= end && end <= ch.cells);
            // carries: six words per graph row (two parities x three) for a query wider than a strip, nothing for the others
            CHECK(pl.carry_off[i] == carry_end);
            if (pl.pitch[i] > MULTI_STRIP_COLUMNS) carry_end += 6ull * gp.n_rows;
            CHECK(carry_end <= ch.carry_words);
            max_pitch = std::max(max_pitch, pl.pitch[i]);
        }
        CHECK(end == ch.cells && carry_end == ch.carry_words && max_pitch == ch.max_pitch);
        // greedy: the next query did not fit
        if (c + 1 < pl.chunks.size()) {
            const uint32_t j = ch.first + ch.count;
            CHECK((ch.cells + multi_query_cells(pl.graphs[pl.graph_of[j]].ckpt, qoff[j + 1] - qoff[j])) * 4 > budget);
        }
        max_bytes = std::max(max_bytes, ch.cells * 4);
        max_carry = std::max(max_carry, ch.carry_words);
    }
    CHECK(next == n && max_bytes == pl.workspace_bytes && max_carry == pl.max_carry_words);
    CHECK(n == 0 || !pl.chunks.empty());
}

}  // namespace

int main() {
    Graph chain, bubble, gfa, empty, idle;
    { Builder b; b.path(20, 1); finish(b, chain); }
    {
        Builder b;
        auto back = b.path(12, 2);
        for (uint32_t len : {1u, 2u, 4u}) { auto br = b.path(len, len); b.edge(back[2], br[0]); b.edge(br.back(), back[8]); }
        b.edge(back[1], back[10]);
        finish(b, bubble);
    }
    {   // the shape of tests/golden/test.gfa: s1 (20) -> s2 (8) -> s3 (4) -> s4 (3), and s2 -> s4
        Builder b;
        auto s1 = b.path(20, 0), s2 = b.path(8, 1), s3 = b.path(4, 2), s4 = b.path(3, 3);
        b.edge(s1.back(), s2[0]); b.edge(s2.back(), s3[0]); b.edge(s2.back(), s4[0]); b.edge(s3.back(), s4[0]);
        finish(b, gfa);
    }
    { Builder b; finish(b, empty); }
    { Builder b; b.path(9, 3); finish(b, idle); }
    CHECK(empty.g.n == 2 && empty.g.n_real == 0 && gfa.g.n == 37);

    const Graph* listed[] = {&chain, &bubble, &gfa, &empty, &idle, &bubble};
    std::vector<MultiGraphIn> in;
    for (const Graph* g : listed) in.push_back(MultiGraphIn{&g->g, &g->sweep, &g->own2});
    const std::vector<std::vector<uint64_t>> lens = {{0, 1, 2, 30, 1100}, {12, 11, 13, 9, 12, 40}, {35, 31, 36, 28, 33, 30, 48, 1}, {4, 0, 1}, {}, {12, 10, 11, 0}};
    std::vector<uint64_t> gq{0}, qoff{0};
    for (const auto& ls : lens) {
        for (uint64_t l : ls) qoff.push_back(qoff.back() + l);
        gq.push_back(qoff.size() - 1);
    }
    const uint32_t ng = (uint32_t)in.size();

    std::string err;
    MultiPlan whole, one, p;
    CHECK(build_multi_plan(in.data(), ng, gq.data(), qoff.data(), 0, 0, whole, err, true) == 0);
    check_plan(in, gq, qoff, 0, 0, whole);
    CHECK(whole.chunks.size() == 1 && whole.workspace_bytes == whole.bytes_total);
    CHECK(whole.max_carry_words == 6ull * chain.g.n);   // the one query wider than a strip
    // the weights differ from the one-piece plan's: more bytes for the same queries, the same pair scratch
    {
        const Graph* src[] = {&chain, &bubble, &gfa, &empty, &idle};
        std::vector<CheckpointPlan> own1(5);
        std::vector<MultiGraphIn> in1;
        for (int k = 0; k < 5; ++k) build_checkpoint_plan(src[k]->g, src[k]->sweep, 0, own1[k]);
        const int idx[] = {0, 1, 2, 3, 4, 1};
        for (int k : idx) in1.push_back(MultiGraphIn{&src[k]->g, &src[k]->sweep, &own1[k]});
        CHECK(build_multi_plan(in1.data(), ng, gq.data(), qoff.data(), 0, 0, one, err) == 0);
        CHECK(one.bytes_total < whole.bytes_total && one.scratch_off == whole.scratch_off && one.max_carry_words == 4ull * chain.g.n);
    }
    // test 2: several segments
    CHECK(build_multi_plan(in.data(), ng, gq.data(), qoff.data(), 7, 0, p, err, true) == 0);
    check_plan(in, gq, qoff, 7, 0, p);
    uint32_t many = 0;
    for (int g = 0; g < 3; ++g) many += p.graphs[g].ckpt.n_segments() >= 3 ? 1 : 0;
    CHECK(many >= 2 && p.graphs[3].ckpt.n_segments() == 1);
    // test 3: a cap just above the largest query, and caps below it
    for (uint64_t ws : {whole.largest_query_bytes + 256, (uint64_t)1, whole.largest_query_bytes, whole.bytes_total - 1, whole.bytes_total / 2}) {
        CHECK(build_multi_plan(in.data(), ng, gq.data(), qoff.data(), 0, ws, p, err, true) == 0);
        check_plan(in, gq, qoff, 0, ws, p);
        CHECK(p.chunks.size() >= 2);
        if (ws == whole.largest_query_bytes + 256) {
            bool inside = false, between = false;
            for (size_t c = 1; c < p.chunks.size(); ++c) {
                const uint32_t f = p.chunks[c].first;
                (p.graph_of[f] == p.graph_of[f - 1] ? inside : between) = true;
            }
            CHECK(p.chunks.size() >= 3 && inside && between);
        }
    }
    // no graphs, no queries; graphs without queries
    const uint64_t zero[2] = {0, 0};
    CHECK(build_multi_plan(nullptr, 0, zero, zero, 0, 0, p, err, true) == 0 && p.chunks.empty() && p.bytes_total == 0);
    const std::vector<uint64_t> gq0(in.size() + 1, 0);
    CHECK(build_multi_plan(in.data(), ng, gq0.data(), zero, 0, 0, p, err, true) == 0);
    check_plan(in, gq0, std::vector<uint64_t>{0}, 0, 0, p);
    CHECK(p.bytes_total == 0 && p.largest_query_bytes == 0 && p.max_carry_words == 0);
    // the argument errors
    std::vector<uint64_t> bad = gq;
    bad[0] = 1;
    CHECK(build_multi_plan(in.data(), ng, bad.data(), qoff.data(), 0, 0, p, err, true) == -1 && !err.empty());
    bad = gq; std::swap(bad[1], bad[2]);
    CHECK(build_multi_plan(in.data(), ng, bad.data(), qoff.data(), 0, 0, p, err, true) == -1);
    std::vector<MultiGraphIn> hole = in;
    hole[2].g = nullptr;
    CHECK(build_multi_plan(hole.data(), (uint32_t)hole.size(), gq.data(), qoff.data(), 0, 0, p, err, true) == -1);
    std::printf("multi_host2 ok\n");
    return 0;
}
