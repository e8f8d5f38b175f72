// Stand-alone check of what a best-of score-set run adds to the plan (poasta_amd/csrc/poa_scoreset_plan.cpp:
// build_scoreset_best_order): built by tests/test_scoreset_best_plan.py with the plan, the sweep rows and the graph flattening
// under -fsanitize=address,undefined, and run on the CPU.  Mixed inputs — repeated pairs, queries without pairs, several chunks,
// all three variants — and the properties the run relies on: every best-of range is a permutation of the same range of
// class_list, ranks do not decrease along it, the pair index ascends within a rank, and the CSR lists each pair once, under its
// query, ascending.  Exit code 0 and "scoreset_best_host ok" on success.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../poasta_amd/csrc/poa_scoreset_plan.hpp"

using namespace poa_amd;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "scoreset_best_host: line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

struct Graph {
    FlatGraph g;
    SweepRows sweep;
};

// a chain of n nodes with a few skipping edges; n == 0: a graph without real nodes (start and end only)
void make_graph(uint32_t n, uint32_t seed, Graph& out) {
    const uint32_t total = n + 2;   // node 0: start, node 1: end
    std::vector<uint8_t> sym(total, 'A');
    sym[0] = '#'; sym[1] = '$';
    std::vector<std::vector<uint32_t>> succ(total), pred(total);
    auto edge = [&](uint32_t a, uint32_t b) { succ[a].push_back(b); pred[b].push_back(a); };
    for (uint32_t i = 0; i < n; ++i) {
        sym[2 + i] = (uint8_t)"ACGT"[(seed + 3 * i + i / 5) & 3];
        if (i) edge(2 + i - 1, 2 + i);
        if (i >= 3 && (i + seed) % 4 == 0) edge(2 + i - 3, 2 + i);
    }
    if (n) { edge(0, 2); edge(2 + n - 1, 1); } else edge(0, 1);
    std::vector<uint32_t> so(total + 1, 0), po(total + 1, 0), s, p;
    for (uint32_t v = 0; v < total; ++v) {
        so[v + 1] = so[v] + (uint32_t)succ[v].size();
        po[v + 1] = po[v] + (uint32_t)pred[v].size();
        s.insert(s.end(), succ[v].begin(), succ[v].end());
        p.insert(p.end(), pred[v].begin(), pred[v].end());
    }
    std::string err;
    const int rc = build_flat_graph(total, 0, 1, sym.data(), so.data(), s.data(), po.data(), p.data(), out.g, err);
    if (rc != 0) { std::fprintf(stderr, "scoreset_best_host: build_flat_graph: %s\n", err.c_str()); std::exit(1); }
    build_sweep_rows(out.g, out.sweep);
}

void check(const ScoreSetPlan& pl, size_t min_chunks) {
    const uint32_t n = pl.n_pairs, nq = pl.n_queries;
    CHECK(pl.chunks.size() >= min_chunks);
    // the CSR: each pair once, under its query, ascending
    CHECK(pl.query_off.size() == (size_t)nq + 1 && pl.query_pairs.size() == n);
    CHECK(pl.query_off[0] == 0 && pl.query_off[nq] == n);
    std::vector<uint32_t> listed(n, 0), rank(n, 0);
    for (uint32_t q = 0; q < nq; ++q) {
        CHECK(pl.query_off[q] <= pl.query_off[q + 1]);
        for (uint32_t k = pl.query_off[q]; k < pl.query_off[q + 1]; ++k) {
            const uint32_t p = pl.query_pairs[k];
            CHECK(p < n && pl.pair_query[p] == q);
            CHECK(k == pl.query_off[q] || pl.query_pairs[k - 1] < p);
            listed[p]++;
            rank[p] = k - pl.query_off[q];
        }
    }
    for (uint32_t p = 0; p < n; ++p) CHECK(listed[p] == 1);
    // the best-of order: per variant, chunk and class a permutation of class_list's range, sorted by (rank, pair index)
    for (uint32_t v = 0; v < SS_N_VARIANTS; ++v) {
        CHECK(pl.best_list[v].size() == n && pl.class_list[v].size() == n);
        for (const ScoreSetPlan::Chunk& ch : pl.chunks) {
            CHECK(ch.class_begin[v][0] == ch.first && ch.class_begin[v][SS_N_CLASSES] == ch.first + ch.count);
            for (uint32_t c = 0; c < SS_N_CLASSES; ++c) {
                const uint32_t b = ch.class_begin[v][c], e = ch.class_begin[v][c + 1];
                CHECK(b <= e && e <= n);
                std::vector<uint32_t> x(pl.class_list[v].begin() + b, pl.class_list[v].begin() + e);
                std::vector<uint32_t> y(pl.best_list[v].begin() + b, pl.best_list[v].begin() + e);
                for (size_t i = 1; i < y.size(); ++i) {
                    CHECK(rank[y[i - 1]] <= rank[y[i]]);
                    if (rank[y[i - 1]] == rank[y[i]]) CHECK(y[i - 1] < y[i]);
                }
                std::sort(x.begin(), x.end());
                std::sort(y.begin(), y.end());
                CHECK(x == y);
            }
        }
    }
}

}  // namespace

int main() {
    std::vector<Graph> graphs(5);
    const uint32_t sizes[5] = {12, 30, 0, 7, 21};
    for (uint32_t g = 0; g < 5; ++g) make_graph(sizes[g], g + 1, graphs[g]);
    std::vector<ScoreSetGraphIn> in;
    for (Graph& g : graphs) in.push_back(ScoreSetGraphIn{&g.g, &g.sweep});
    in.push_back(ScoreSetGraphIn{&graphs[1].g, &graphs[1].sweep});   // a handle listed twice
    const uint32_t n_graphs = (uint32_t)in.size();
    // queries of every kernel class of every variant: pitch 64, 256 / 320 (u32: Q1 / Q2), 512 / 576 / 1024 (packed), 1088 (two strips)
    const uint64_t lens[] = {0, 1, 40, 63, 255, 256, 300, 511, 512, 600, 1023, 1024, 1100, 5, 17};
    const uint32_t nq = sizeof(lens) / sizeof(lens[0]);
    std::vector<uint64_t> qoff(nq + 1, 0);
    for (uint32_t q = 0; q < nq; ++q) qoff[q + 1] = qoff[q] + lens[q];
    std::string err;

    // the full matrix, as one chunk and as many
    for (uint64_t ws : {0ull, 1ull, 300000ull}) {
        ScoreSetPlan pl;
        CHECK(build_scoreset_plan(in.data(), n_graphs, nq, qoff.data(), (uint64_t)nq * n_graphs, nullptr, nullptr, ws, pl, err) == 0);
        build_scoreset_best_order(pl);
        check(pl, ws ? 2 : 1);
        build_scoreset_best_order(pl);   // idempotent
        check(pl, ws ? 2 : 1);
    }
    // a pair list in no order: repeated pairs, queries 3 and 13 without a pair, a graph without a pair
    std::vector<uint32_t> pq, pg;
    uint32_t state = 12345;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return state >> 8; };
    for (uint32_t i = 0; i < 400; ++i) {
        uint32_t q = next() % nq;
        if (q == 3 || q == 13) q = 12;
        uint32_t g = next() % n_graphs;
        if (g == 3) g = 5;
        pq.push_back(q); pg.push_back(g);
        if (i % 7 == 0) { pq.push_back(q); pg.push_back(g); }   // the same pair again, next to the first
    }
    pq.push_back(pq[0]); pg.push_back(pg[0]);                    // and far from it
    for (uint64_t ws : {0ull, 1ull, 200000ull, 5000000ull}) {
        ScoreSetPlan pl;
        CHECK(build_scoreset_plan(in.data(), n_graphs, nq, qoff.data(), pq.size(), pq.data(), pg.data(), ws, pl, err) == 0);
        build_scoreset_best_order(pl);
        check(pl, ws == 1 || ws == 200000 ? 2 : 1);
        CHECK(pl.query_off[4] == pl.query_off[3] && pl.query_off[14] == pl.query_off[13]);
    }
    // no pairs; no queries
    {
        ScoreSetPlan pl;
        CHECK(build_scoreset_plan(in.data(), n_graphs, nq, qoff.data(), 0, pq.data(), pg.data(), 0, pl, err) == 0);
        build_scoreset_best_order(pl);
        check(pl, 0);
        const uint64_t none[1] = {0};
        CHECK(build_scoreset_plan(in.data(), n_graphs, 0, none, 0, nullptr, nullptr, 0, pl, err) == 0);
        build_scoreset_best_order(pl);
        check(pl, 0);
    }
    std::printf("scoreset_best_host ok\n");
    return 0;
}
