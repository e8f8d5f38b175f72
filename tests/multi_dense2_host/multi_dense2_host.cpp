// Stand-alone check of the dense two-piece multi-graph plan (poasta_amd/csrc/poa_multi_plan.cpp, build_multi_dense2_plan): built
// by tests/test_multi_dense2_plan.py together with the plan, the sweep rows and the graph flattening under
// -fsanitize=address,undefined, and run on the CPU.  It plans the shapes of tests/test_multi_dense2.py and checks what the
// kernels of poa_multi_dense2.hpp rely on: the footprint formula query by query, every one of a region's five planes 16-byte
// aligned and inside its chunk, the regions of a chunk disjoint, the chunks covering every query exactly once by the greedy rule,
// one copy of the tables per distinct handle, no carries, no length limit.
// Exit code 0 and "multi_dense2_host ok" on success.
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
        if (!(cond)) { std::fprintf(stderr, "multi_dense2_host: line %d: %s\n", __LINE__, #cond); std::exit(1); } \
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

void finish(Builder& b, FlatGraph& out) {
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
    const int rc = build_flat_graph(n, 0, 1, b.sym.data(), so.data(), s.data(), po.data(), p.data(), out, err);
    if (rc != 0) { std::fprintf(stderr, "multi_dense2_host: build_flat_graph: %s\n", err.c_str()); std::exit(1); }
}

uint32_t pitch_of(uint64_t L) { return (uint32_t)(((L + 1 + 63) / 64) * 64); }
// the two-byte elements of one query, written out: five planes of rows x pitch
uint64_t elems_by_hand(const FlatGraph& g, uint64_t L) { return 5ull * g.n * pitch_of(L); }

void check_plan(const std::vector<MultiGraphIn>& in, const std::vector<uint64_t>& gq, const std::vector<uint64_t>& qoff, uint64_t ws,
                const MultiPlan& pl) {
    const uint32_t n_graphs = (uint32_t)in.size(), n = (uint32_t)qoff.size() - 1;
    CHECK(pl.n_queries == n && pl.graphs.size() == n_graphs);
    // per graph: table ranges in bounds; distinct handles do not overlap, equal ones share one copy
    std::vector<std::pair<uint64_t, uint64_t>> row_ranges, edge_ranges;
    uint64_t rows_distinct = 0, edges_distinct = 0;
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const MultiGraphPlan& gp = pl.graphs[g];
        CHECK(gp.n_rows == in[g].g->n && gp.n_edges == in[g].g->pred_rows.size());
        CHECK(gp.row_base + gp.n_rows <= pl.n_rows_total && gp.edge_base + gp.n_edges <= pl.n_edges_total);
        CHECK(gp.table_of <= g && in[gp.table_of].g == in[g].g);
        bool first = true;
        for (uint32_t h = 0; h < g; ++h) first = first && in[h].g != in[g].g;
        CHECK(first == (gp.table_of == g));
        if (first) {
            row_ranges.push_back({gp.row_base, gp.row_base + gp.n_rows});
            edge_ranges.push_back({gp.edge_base, gp.edge_base + gp.n_edges});
            rows_distinct += gp.n_rows; edges_distinct += gp.n_edges;
        } else CHECK(gp.row_base == pl.graphs[gp.table_of].row_base && gp.edge_base == pl.graphs[gp.table_of].edge_base);
        CHECK(gp.n_queries == gq[g + 1] - gq[g]);
        // every predecessor row the kernels read lies inside the graph's own rows
        for (uint32_t p : in[g].g->pred_rows) CHECK(p < gp.n_rows);
    }
    CHECK(rows_distinct == pl.n_rows_total && edges_distinct == pl.n_edges_total);
    for (auto* ranges : {&row_ranges, &edge_ranges}) {
        std::sort(ranges->begin(), ranges->end());
        for (size_t k = 1; k < ranges->size(); ++k) CHECK((*ranges)[k - 1].second <= (*ranges)[k].first);
    }

    // per query: the footprint formula
    uint64_t total = 0, largest = 0, planes = 0, cells = 0, bases = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t g = pl.graph_of[i];
        CHECK(g < n_graphs && i >= gq[g] && i < gq[g + 1]);
        const uint64_t L = qoff[i + 1] - qoff[i];
        CHECK(pl.pitch[i] == pitch_of(L));
        CHECK(multi_dense2_query_elems(*in[g].g, L) == elems_by_hand(*in[g].g, L));
        const uint64_t bytes = 2 * elems_by_hand(*in[g].g, L) + 256;
        total += bytes; largest = std::max(largest, bytes); planes += bytes - 256;
        cells += (uint64_t)in[g].g->n * (L + 1); bases += L;
        CHECK(pl.scratch_off[i + 1] - pl.scratch_off[i] == L + pl.graphs[g].n_rows);
        CHECK(pl.carry_off[i] == 0);
    }
    CHECK(pl.scratch_off[0] == 0);
    CHECK(total == pl.bytes_total && largest == pl.largest_query_bytes && planes == pl.plane_bytes);
    CHECK(cells == pl.total_cells && bases == pl.total_bases);
    CHECK(pl.max_carry_words == 0);

    // chunks: exact coverage, everything inside the workspace, nothing overlapping, greedy
    const uint64_t budget = ws == 0 ? total : std::max(ws, largest);
    uint32_t next = 0;
    uint64_t max_bytes = 0;
    for (size_t c = 0; c < pl.chunks.size(); ++c) {
        const MultiPlan::Chunk& ch = pl.chunks[c];
        CHECK(ch.first == next && ch.count > 0 && ch.carry_words == 0);
        next += ch.count;
        CHECK(ch.cells * 2 <= budget && ch.cells * 2 <= pl.workspace_bytes);
        uint64_t end = 0;
        uint32_t max_pitch = 0;
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
            const FlatGraph& fg = *in[pl.graph_of[i]].g;
            const uint64_t L = qoff[i + 1] - qoff[i];
            CHECK(pl.region_off[i] == end);   // back to back: disjoint
            const uint64_t rp = (uint64_t)fg.n * pl.pitch[i];
            // every plane of the region starts 16-byte aligned (the kernels load and store 16 bytes at a time), and the last
            // 16-byte group a lane addresses — row n - 1, columns pitch - 8 .. pitch - 1 of the fifth plane — ends inside it
            for (uint64_t k = 0; k < 5; ++k) CHECK(((pl.region_off[i] + k * rp) * 2) % 16 == 0);
            CHECK(pl.pitch[i] % 64 == 0 && pl.pitch[i] >= L + 1);
            end += elems_by_hand(fg, L) + MULTI_DENSE_PAD_ELEMS;
            CHECK(pl.region_off[i] + 4 * rp + (uint64_t)(fg.n - 1) * pl.pitch[i] + pl.pitch[i] <= end - MULTI_DENSE_PAD_ELEMS);
            CHECK(end <= ch.cells);
            max_pitch = std::max(max_pitch, pl.pitch[i]);
        }
        CHECK(end == ch.cells && max_pitch == ch.max_pitch);
        if (c + 1 < pl.chunks.size()) {   // greedy: the next query did not fit
            const uint32_t j = ch.first + ch.count;
            CHECK((ch.cells + elems_by_hand(*in[pl.graph_of[j]].g, qoff[j + 1] - qoff[j]) + MULTI_DENSE_PAD_ELEMS) * 2 > budget);
        }
        max_bytes = std::max(max_bytes, ch.cells * 2);
    }
    CHECK(next == n && max_bytes == pl.workspace_bytes);
    CHECK(n == 0 || !pl.chunks.empty());
}

}  // namespace

// `multi_dense2_host chunks CAP SPEC...`: plans the listings the caller describes and prints the footprint and the first query of
// every chunk, for the Python restatement of the greedy rule to compare with.  SPEC is "ROWS:len,len,..." (a chain of ROWS rows,
// sentinels included) or "=K:len,len,..." (the handle of listing K again); the lengths may be empty.
int print_chunks(int argc, char** argv) {
    const uint64_t cap = std::strtoull(argv[2], nullptr, 10);
    std::vector<FlatGraph> own((size_t)argc);   // (never resized: the plan holds pointers into it)
    std::vector<MultiGraphIn> in;
    std::vector<uint64_t> gq{0}, qoff{0};
    for (int a = 3; a < argc; ++a) {
        std::string spec = argv[a];
        const size_t colon = spec.find(':');
        CHECK(colon != std::string::npos);
        if (spec[0] == '=') {
            const size_t k = std::strtoull(spec.c_str() + 1, nullptr, 10);
            CHECK(k < in.size());
            in.push_back(in[k]);
        } else {
            const uint32_t rows = (uint32_t)std::strtoul(spec.c_str(), nullptr, 10);
            CHECK(rows >= 2);
            Builder b;
            if (rows > 2) b.path(rows - 2, (uint32_t)a);
            finish(b, own[(size_t)a]);
            CHECK(own[(size_t)a].n == rows);
            in.push_back(MultiGraphIn{&own[(size_t)a], nullptr, nullptr});
        }
        const char* p = spec.c_str() + colon + 1;
        while (*p) {
            char* end = nullptr;
            qoff.push_back(qoff.back() + std::strtoull(p, &end, 10));
            p = *end == ',' ? end + 1 : end;
        }
        gq.push_back(qoff.size() - 1);
    }
    MultiPlan pl;
    std::string err;
    CHECK(build_multi_dense2_plan(in.data(), (uint32_t)in.size(), gq.data(), qoff.data(), cap, pl, err) == 0);
    check_plan(in, gq, qoff, cap, pl);
    std::printf("%llu %llu %llu", (unsigned long long)pl.bytes_total, (unsigned long long)pl.largest_query_bytes, (unsigned long long)pl.workspace_bytes);
    for (const auto& ch : pl.chunks) std::printf(" %u", ch.first);
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && std::string(argv[1]) == "chunks") return print_chunks(argc, argv);
    FlatGraph chain, bubble, empty, idle;
    { Builder b; b.path(6, 1); finish(b, chain); }
    {   // three branches between two backbone nodes, and an edge that skips rows: in-degree 4, predecessors that are not adjacent rows
        Builder b;
        auto back = b.path(24, 2);
        for (uint32_t len : {1u, 3u, 6u}) { auto br = b.path(len, len); b.edge(back[2], br[0]); b.edge(br.back(), back[12]); }
        b.edge(back[1], back[20]);
        finish(b, bubble);
    }
    { Builder b; finish(b, empty); }
    { Builder b; b.path(9, 3); finish(b, idle); }
    CHECK(empty.n == 2 && empty.n_real == 0);
    CHECK(bubble.n >= 30);

    const FlatGraph* listed[] = {&chain, &bubble, &empty, &bubble, &idle};
    std::vector<MultiGraphIn> in;
    for (const FlatGraph* g : listed) in.push_back(MultiGraphIn{g, nullptr, nullptr});
    const std::vector<std::vector<uint64_t>> lens = {{0, 1, 2, 63, 64}, {511, 512, 1023, 1024, 1100, 5000}, {4, 0}, {12, 10, 33}, {}};
    std::vector<uint64_t> gq{0}, qoff{0};
    for (const auto& ls : lens) {
        for (uint64_t l : ls) qoff.push_back(qoff.back() + l);
        gq.push_back(qoff.size() - 1);
    }
    const uint32_t ng = (uint32_t)in.size();

    std::string err;
    MultiPlan whole, p;
    CHECK(build_multi_dense2_plan(in.data(), ng, gq.data(), qoff.data(), 0, whole, err) == 0);   // (a query of 5 000 symbols is accepted)
    check_plan(in, gq, qoff, 0, whole);
    CHECK(whole.chunks.size() == 1 && whole.workspace_bytes == whole.bytes_total && whole.chunks[0].max_pitch == pitch_of(5000));
    CHECK(whole.n_rows_total == (uint64_t)chain.n + bubble.n + empty.n + idle.n);   // the bubble graph once
    CHECK(whole.largest_query_bytes == 2ull * 5 * bubble.n * pitch_of(5000) + 256);
    // caps: just above the largest query, below it (raised), equal to it, and in between
    for (uint64_t ws : {whole.largest_query_bytes + 256, (uint64_t)1, whole.largest_query_bytes, whole.bytes_total - 1, whole.bytes_total / 2}) {
        CHECK(build_multi_dense2_plan(in.data(), ng, gq.data(), qoff.data(), ws, p, err) == 0);
        check_plan(in, gq, qoff, ws, p);
        CHECK(p.chunks.size() >= 2);
        if (ws == 1) CHECK(p.workspace_bytes == whole.largest_query_bytes);
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
    CHECK(build_multi_dense2_plan(nullptr, 0, zero, zero, 0, p, err) == 0 && p.chunks.empty() && p.bytes_total == 0);
    const std::vector<uint64_t> gq0(in.size() + 1, 0);
    CHECK(build_multi_dense2_plan(in.data(), ng, gq0.data(), zero, 0, p, err) == 0);
    check_plan(in, gq0, std::vector<uint64_t>{0}, 0, p);
    CHECK(p.bytes_total == 0 && p.largest_query_bytes == 0);
    // the argument errors
    std::vector<uint64_t> bad = gq;
    bad[0] = 1;
    err.clear();
    CHECK(build_multi_dense2_plan(in.data(), ng, bad.data(), qoff.data(), 0, p, err) == -1 && !err.empty());
    bad = gq; std::swap(bad[1], bad[2]);
    CHECK(build_multi_dense2_plan(in.data(), ng, bad.data(), qoff.data(), 0, p, err) == -1);
    std::vector<MultiGraphIn> hole = in;
    hole[1].g = nullptr;
    CHECK(build_multi_dense2_plan(hole.data(), (uint32_t)hole.size(), gq.data(), qoff.data(), 0, p, err) == -1);
    CHECK(build_multi_dense2_plan(in.data(), ng, nullptr, qoff.data(), 0, p, err) == -1);
    std::printf("multi_dense2_host ok\n");
    return 0;
}
