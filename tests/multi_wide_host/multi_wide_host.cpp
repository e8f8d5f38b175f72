// Stand-alone check of the dense and exact multi-graph plans with queries wider than one strip (poasta_amd/csrc/poa_multi_plan.cpp,
// build_multi_dense_plan / build_multi_exact_plan with `wide`): built by tests/test_multi_wide_plan.py together with the plan, the
// sweep rows and the graph flattening under -fsanitize=address,undefined, and run on the CPU.  It checks what
// poa_forward_packed_multi_wide_kernel relies on: the pitch rule, the carry words of a query (0 up to pitch 1024, 2 x rows
// above), carry regions disjoint inside a chunk and restarting with every chunk, max_carry_words the largest chunk's, plane
// regions disjoint and inside the workspace, complete chunk coverage under a cap, the carry-overflow refusal; and for the exact
// plan that the table regions and the slot follow the longest query.  Without `wide` the 1024-symbol refusal stands.
// Exit code 0 and "multi_wide_host ok" on success.
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
        if (!(cond)) { std::fprintf(stderr, "multi_wide_host: line %d: %s\n", __LINE__, #cond); std::exit(1); } \
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
    int rc = build_flat_graph(n, 0, 1, b.sym.data(), so.data(), s.data(), po.data(), p.data(), out, err);
    if (rc == 0) rc = build_bubble_index(out, err);
    if (rc != 0) { std::fprintf(stderr, "multi_wide_host: graph: %s\n", err.c_str()); std::exit(1); }
}

uint32_t pitch_of(uint64_t L) { return (uint32_t)(((L + 1 + 63) / 64) * 64); }
uint64_t elems_by_hand(const FlatGraph& g, uint64_t L) {
    const uint64_t rp = (uint64_t)g.n * pitch_of(L);
    return rp + rp / 4 + (uint64_t)(g.d_slot.empty() ? g.n : g.n_store_d) * pitch_of(L);
}
uint64_t table_by_hand(const FlatGraph& g, uint64_t L) { return 3ull * g.n * pitch_of(L); }

// what both kinds share: pitches, carries, chunk coverage, plane regions.  `exact`: the tables behind the dense regions.
void check_plan(const std::vector<MultiGraphIn>& in, const std::vector<uint64_t>& gq, const std::vector<uint64_t>& qoff, uint64_t ws,
                const MultiPlan& pl, bool exact) {
    const uint32_t n = (uint32_t)qoff.size() - 1;
    CHECK(pl.n_queries == n && pl.graphs.size() == in.size());
    CHECK(pl.graph_of.size() == n && pl.pitch.size() == n && pl.carry_off.size() == n && pl.region_off.size() == n);
    uint64_t total = 0, largest = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t g = pl.graph_of[i];
        CHECK(g < in.size() && i >= gq[g] && i < gq[g + 1]);
        const uint64_t L = qoff[i + 1] - qoff[i];
        CHECK(pl.pitch[i] == pitch_of(L) && pl.pitch[i] % 64 == 0 && pl.pitch[i] >= L + 1 && pl.pitch[i] < L + 1 + 64);
        CHECK(multi_dense_query_elems(*in[g].g, L) == elems_by_hand(*in[g].g, L));
        if (exact) CHECK(multi_exact_table_cells(*in[g].g, L) == table_by_hand(*in[g].g, L));
        const uint64_t bytes = 2 * elems_by_hand(*in[g].g, L) + 256 + (exact ? 4 * table_by_hand(*in[g].g, L) + 256 : 0);
        total += bytes; largest = std::max(largest, bytes);
        CHECK(pl.scratch_off[i + 1] - pl.scratch_off[i] == L + pl.graphs[g].n_rows);
    }
    CHECK(total == pl.bytes_total && largest == pl.largest_query_bytes);

    const uint64_t budget = ws == 0 ? total : std::max(ws, largest);
    uint32_t next = 0;
    uint64_t max_bytes = 0, max_carry = 0;
    for (size_t c = 0; c < pl.chunks.size(); ++c) {
        const MultiPlan::Chunk& ch = pl.chunks[c];
        CHECK(ch.first == next && ch.count > 0);
        next += ch.count;
        uint64_t end = 0, carry_end = 0, table_end = 0;
        uint32_t max_pitch = 0;
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
            const FlatGraph& fg = *in[pl.graph_of[i]].g;
            const uint64_t L = qoff[i + 1] - qoff[i];
            // plane regions back to back: disjoint, 16-byte aligned, inside the chunk
            CHECK(pl.region_off[i] == end && (pl.region_off[i] * 2) % 16 == 0);
            end += elems_by_hand(fg, L) + MULTI_DENSE_PAD_ELEMS;
            // carries back to back from 0 in every chunk: 2 x rows words for a query wider than one strip, none otherwise
            const uint64_t cw = pl.pitch[i] > 1024 ? 2ull * fg.n : 0ull;
            CHECK((pl.pitch[i] > 1024) == (L >= 1024));
            CHECK(pl.carry_off[i] == carry_end);
            carry_end += cw;
            // the last word the strip loop touches: carry[2 * (n_rows - 1) + 1]
            if (cw) CHECK(pl.carry_off[i] + 2ull * (fg.n - 1) + 1 < carry_end);
            if (exact) {
                CHECK(pl.table_off[i] == ch.cells / 2 + table_end);   // four-byte cells from the start of the workspace
                table_end += table_by_hand(fg, L) + MULTI_EXACT_PAD_CELLS;
            }
            max_pitch = std::max(max_pitch, pl.pitch[i]);
        }
        CHECK(end == ch.cells && carry_end == ch.carry_words && max_pitch == ch.max_pitch);
        if (exact) CHECK(table_end == ch.table_cells);
        const uint64_t bytes = ch.cells * 2 + (exact ? ch.table_cells * 4 : 0);
        CHECK(bytes <= budget && bytes <= pl.workspace_bytes);
        if (c + 1 < pl.chunks.size()) {   // greedy: the next query did not fit
            const uint32_t j = ch.first + ch.count;
            const FlatGraph& fg = *in[pl.graph_of[j]].g;
            const uint64_t L = qoff[j + 1] - qoff[j];
            CHECK(bytes + 2 * (elems_by_hand(fg, L) + MULTI_DENSE_PAD_ELEMS) + (exact ? 4 * (table_by_hand(fg, L) + MULTI_EXACT_PAD_CELLS) : 0) > budget);
        }
        max_bytes = std::max(max_bytes, bytes);
        max_carry = std::max(max_carry, ch.carry_words);
    }
    CHECK(next == n && max_bytes == pl.workspace_bytes && max_carry == pl.max_carry_words);
}

}  // namespace

int main() {
    FlatGraph chain, bubble, ladder, empty, idle;
    { Builder b; b.path(20, 1); finish(b, chain); }
    {
        Builder b;
        auto back = b.path(12, 2);
        for (uint32_t len : {1u, 2u, 4u}) { auto br = b.path(len, len); b.edge(back[2], br[0]); b.edge(br.back(), back[8]); }
        b.edge(back[1], back[10]);
        finish(b, bubble);
    }
    {   // two rails: most rows are read back from memory, D rows kept by row
        Builder b;
        uint32_t a = b.node('A'), c = b.node('C');
        for (uint32_t i = 1; i < 12; ++i) {
            const uint32_t a2 = b.node("ACGT"[i & 3]), c2 = b.node("ACGT"[(i + 1) & 3]);
            b.edge(a, a2); b.edge(c, a2); b.edge(a, c2); b.edge(c, c2);
            a = a2; c = c2;
        }
        finish(b, ladder);
    }
    { Builder b; finish(b, empty); }
    { Builder b; b.path(9, 3); finish(b, idle); }

    // one handle listed twice (bubble), one graph without queries (idle)
    const FlatGraph* listed[] = {&chain, &bubble, &ladder, &empty, &idle, &bubble};
    std::vector<MultiGraphIn> in;
    for (const FlatGraph* g : listed) in.push_back(MultiGraphIn{g, nullptr, nullptr});
    const std::vector<std::vector<uint64_t>> lens = {{0, 1, 1023, 1024, 1025}, {2047, 12, 2048, 3000, 40}, {1024, 63, 1023, 2048}, {4, 0, 1500}, {}, {3000, 10, 1025, 0, 1023}};
    std::vector<uint64_t> gq{0}, qoff{0};
    for (const auto& ls : lens) {
        for (uint64_t l : ls) qoff.push_back(qoff.back() + l);
        gq.push_back(qoff.size() - 1);
    }
    const uint32_t ng = (uint32_t)in.size();
    std::string err;
    MultiPlan whole, p;

    // without `wide` (the default argument and false): the refusal of today, with its message
    CHECK(build_multi_dense_plan(in.data(), ng, gq.data(), qoff.data(), 0, p, err) == -7 && err.find("poa_multi_create") != std::string::npos);
    CHECK(build_multi_dense_plan(in.data(), ng, gq.data(), qoff.data(), 0, p, err, false) == -7 && err.find("1023") != std::string::npos);
    {
        const std::vector<uint64_t> g1{0, 1}, a{0, 1024}, b{0, 1023};
        CHECK(build_multi_dense_plan(in.data(), 1, g1.data(), a.data(), 0, p, err, false) == -7);
        CHECK(build_multi_dense_plan(in.data(), 1, g1.data(), b.data(), 0, p, err, false) == 0 && p.max_carry_words == 0 && p.chunks[0].max_pitch == 1024);
        // the same one-strip query under `wide`: the same plan, no carry
        MultiPlan w;
        CHECK(build_multi_dense_plan(in.data(), 1, g1.data(), b.data(), 0, w, err, true) == 0);
        CHECK(w.max_carry_words == 0 && w.carry_off[0] == 0 && w.bytes_total == p.bytes_total && w.chunks[0].max_pitch == 1024);
        // the first query that takes carries
        CHECK(build_multi_dense_plan(in.data(), 1, g1.data(), a.data(), 0, w, err, true) == 0);
        CHECK(w.pitch[0] == 1088 && w.max_carry_words == 2ull * chain.n && w.chunks[0].carry_words == 2ull * chain.n);
        // the length limit of the other constructors stays
        const std::vector<uint64_t> huge{0, 0x7FFFFFF1ull};
        CHECK(build_multi_dense_plan(in.data(), 1, g1.data(), huge.data(), 0, w, err, true) == -7 && err.find("2^31") != std::string::npos);
    }

    // dense, wide
    CHECK(build_multi_dense_plan(in.data(), ng, gq.data(), qoff.data(), 0, whole, err, true) == 0);
    check_plan(in, gq, qoff, 0, whole, false);
    CHECK(whole.chunks.size() == 1 && whole.chunks[0].max_pitch == pitch_of(3000));
    CHECK(whole.n_rows_total == (uint64_t)chain.n + bubble.n + ladder.n + empty.n + idle.n);   // the bubble graph once
    {   // the carries of the whole batch, by hand: every query of 1024 symbols or more
        uint64_t words = 0;
        for (size_t g = 0; g < lens.size(); ++g)
            for (uint64_t l : lens[g]) if (l >= 1024) words += 2ull * listed[g]->n;
        CHECK(words == whole.max_carry_words && words > 0);
    }
    bool inside = false, between = false, narrow_chunk = false, wide_chunk = false;
    for (uint64_t ws : {whole.largest_query_bytes + 256, (uint64_t)1, whole.largest_query_bytes, whole.bytes_total - 1, whole.bytes_total / 2, whole.bytes_total / 5}) {
        CHECK(build_multi_dense_plan(in.data(), ng, gq.data(), qoff.data(), ws, p, err, true) == 0);
        check_plan(in, gq, qoff, ws, p, false);
        CHECK(p.chunks.size() >= 2 && p.max_carry_words <= whole.max_carry_words);
        for (size_t c = 1; c < p.chunks.size(); ++c) {
            const uint32_t f = p.chunks[c].first;
            (p.graph_of[f] == p.graph_of[f - 1] ? inside : between) = true;
        }
        for (const auto& ch : p.chunks) {
            (ch.max_pitch <= 1024 ? narrow_chunk : wide_chunk) = true;
            CHECK((ch.max_pitch <= 1024) == (ch.carry_words == 0));   // a chunk of one-strip queries holds no carry
        }
    }
    CHECK(inside && between && narrow_chunk && wide_chunk);

    // exact, wide: the same carries, the tables and the slot by the longest query
    const MultiExactCosts c0;
    CHECK(build_multi_exact_plan(in.data(), ng, gq.data(), qoff.data(), 0, c0, p, err) == -7 && err.find("poa_align_batch_ex") != std::string::npos);
    MultiPlan xwhole;
    CHECK(build_multi_exact_plan(in.data(), ng, gq.data(), qoff.data(), 0, c0, xwhole, err, true) == 0);
    check_plan(in, gq, qoff, 0, xwhole, true);
    CHECK(xwhole.chunks.size() == 1 && xwhole.max_carry_words == whole.max_carry_words);
    {
        uint64_t n_exit = 0, stack = 8;
        for (uint32_t g = 0; g < ng; ++g) {
            if (lens[g].empty()) continue;
            n_exit = std::max<uint64_t>(n_exit, listed[g]->n_exit);
            stack = std::max<uint64_t>(stack, listed[g]->n + *std::max_element(lens[g].begin(), lens[g].end()) + 8);
        }
        const MultiExactSlot& s = xwhole.exact;
        const uint64_t wpn = (3000 + 1 + 63) / 64, swpn = (wpn + 63) / 64;
        CHECK(s.wpn == wpn && s.swpn == swpn && s.n_exit == n_exit && s.stack_cap == stack);
        CHECK(s.reached_stride == ((n_exit * wpn + 1) & ~1ull) && s.rsum_stride == ((n_exit * swpn + 1) & ~1ull));
        CHECK(s.bytes == s.reached_stride * 8 + s.rsum_stride * 8 + (uint64_t)s.stack_cap * 12 + (uint64_t)s.pool_cap * 16 + 3ull * s.win * 4);
        CHECK(xwhole.exact_slots == xwhole.n_queries && xwhole.exact_bytes == s.buffer_bytes(xwhole.exact_slots));
        // the pool holds at least the cells of the largest (graph, longest query) at the default 0.25 entries per cell
        uint64_t pool = 256;
        for (uint32_t g = 0; g < ng; ++g)
            if (!lens[g].empty()) pool = std::max<uint64_t>(pool, (uint64_t)(0.25f * (double)listed[g]->n * (double)(*std::max_element(lens[g].begin(), lens[g].end()) + 1)));
        CHECK(s.pool_cap >= pool && s.pool_cap % 64 == 0);
    }
    wide_chunk = narrow_chunk = false;
    for (uint64_t ws : {xwhole.largest_query_bytes + 256, (uint64_t)1, xwhole.bytes_total / 2, xwhole.bytes_total / 5}) {
        CHECK(build_multi_exact_plan(in.data(), ng, gq.data(), qoff.data(), ws, c0, p, err, true) == 0);
        check_plan(in, gq, qoff, ws, p, true);
        CHECK(p.chunks.size() >= 2 && p.exact.wpn == xwhole.exact.wpn);
        uint32_t most = 0;
        for (const auto& ch : p.chunks) { most = std::max(most, ch.count); (ch.max_pitch <= 1024 ? narrow_chunk : wide_chunk) = true; }
        CHECK(p.exact_slots == most);
    }
    CHECK(narrow_chunk && wide_chunk);

    // the carry-overflow refusal, with synthetic row counts: three queries of 2^30 rows each hold 3 x 2^31 carry words in one
    // chunk; a cap that gives every query its own chunk passes
    {
        FlatGraph big;
        big.n = 1u << 30;
        big.n_store_d = 0;
        big.d_slot.assign(1, 0u);   // (a d_slot table: no D rows kept; the plan reads its emptiness alone)
        const MultiGraphIn bin{&big, nullptr, nullptr};
        const std::vector<uint64_t> g1{0, 3}, q3{0, 1024, 2048, 3072}, q2{0, 1024, 2048, 3071};
        err.clear();
        CHECK(build_multi_dense_plan(&bin, 1, g1.data(), q3.data(), 0, p, err, true) == -7 && err.find("strip carries") != std::string::npos);
        CHECK(build_multi_dense_plan(&bin, 1, g1.data(), q3.data(), 1, p, err, true) == 0 && p.chunks.size() == 3 && p.max_carry_words == 1ull << 31);
        for (uint32_t i = 0; i < 3; ++i) CHECK(p.carry_off[i] == 0);
        // two wide queries and a one-strip one fit: 2 x 2^31 words is the last count below the limit... and is refused (2^32
        // words do not fit a 4-byte offset's range), so the sum must stay below it
        CHECK(build_multi_dense_plan(&bin, 1, g1.data(), q2.data(), 0, p, err, true) == -7);
        const std::vector<uint64_t> g2{0, 2}, q1{0, 1024, 2047};
        CHECK(build_multi_dense_plan(&bin, 1, g2.data(), q1.data(), 0, p, err, true) == 0 && p.max_carry_words == 1ull << 31 && p.carry_off[1] == 1u << 31);
        // without `wide` nothing of this is reached: the length refusal comes first
        CHECK(build_multi_dense_plan(&bin, 1, g1.data(), q3.data(), 0, p, err) == -7 && err.find("1023") != std::string::npos);
    }
    std::printf("multi_wide_host ok\n");
    return 0;
}
