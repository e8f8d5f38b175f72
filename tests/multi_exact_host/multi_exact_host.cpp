// Stand-alone check of the exact multi-graph plan (poasta_amd/csrc/poa_multi_plan.cpp, build_multi_exact_plan) and of the slot
// strides the replay kernel of poa_multi_exact.hpp relies on: built by tests/test_multi_exact_plan.py together with the plan, the
// sweep rows and the graph flattening under -fsanitize=address,undefined, and run on the CPU.
//
//   plan      dense regions and visited tables of a chunk disjoint, 16-byte aligned and inside the chunk; the chunks covering every
//             query once, cut greedily by the sum of both footprints; one copy of the ExactGraph tables per distinct handle; the
//             slot workspace the documented sum, its five arrays disjoint and inside the buffer; the footprint the documented sum.
//   searches  the host build of the search (ExactSearchT::run_buckets, as tests/exact_host runs it) for an interleaved batch of
//             a bubble-rich graph and a chain, every query in its own slot of ONE plan-sized buffer, addressed by the kernel's own
//             arithmetic (the biased base plus the search's slot * n_exit * wpn).  The buffer is cleared once, as the run clears
//             it, and every word a slot does not own holds a canary.  Visited table, score, status and counters must equal the
//             same search run alone on a workspace of its own, and no canary may move.  With the graph's own stride instead of
//             the batch-wide one the slots overlap: the arithmetic of that is asserted too.
// Exit code 0 and "multi_exact_host ok" on success.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../poasta_amd/csrc/poa_exact.hpp"
#include "../../poasta_amd/csrc/poa_multi_plan.hpp"

using namespace poa_amd;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "multi_exact_host: line %d: %s\n", __LINE__, #cond); std::exit(1); } \
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

void finish(Builder& b, FlatGraph& out, bool bubbles = true) {
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
    if (rc == 0 && bubbles) rc = build_bubble_index(out, err);
    if (rc != 0) { std::fprintf(stderr, "multi_exact_host: graph: %s\n", err.c_str()); std::exit(1); }
}

// an SNP ladder: `bubbles` times two alternative nodes between two backbone nodes
void snp_ladder(uint32_t bubbles, FlatGraph& out, std::vector<uint8_t>& backbone) {
    Builder b;
    uint32_t prev = b.node('A');
    backbone.push_back('A');
    for (uint32_t i = 0; i < bubbles; ++i) {
        const uint8_t s0 = "ACGT"[i & 3], s1 = "ACGT"[(i + 2) & 3];
        const uint32_t a = b.node(s0), c = b.node(s1), join = b.node("ACGT"[(i + 1) & 3]);
        b.edge(prev, a); b.edge(prev, c); b.edge(a, join); b.edge(c, join);
        backbone.push_back(s0); backbone.push_back("ACGT"[(i + 1) & 3]);
        prev = join;
    }
    finish(b, out);
}

uint32_t pitch_of(uint64_t L) { return (uint32_t)(((L + 1 + 63) / 64) * 64); }
uint64_t dense_elems(const FlatGraph& g, uint64_t L) {
    const uint64_t rp = (uint64_t)g.n * pitch_of(L);
    return rp + rp / 4 + (uint64_t)(g.d_slot.empty() ? g.n : g.n_store_d) * pitch_of(L);
}

void check_plan(const std::vector<MultiGraphIn>& in, const std::vector<uint64_t>& gq, const std::vector<uint64_t>& qoff, uint64_t ws,
                const MultiExactCosts& costs, const MultiPlan& pl) {
    const uint32_t n_graphs = (uint32_t)in.size(), n = (uint32_t)qoff.size() - 1;
    CHECK(pl.n_queries == n && pl.graphs.size() == n_graphs && pl.table_off.size() == n);
    // the ExactGraph tables: in bounds, one copy per distinct handle
    uint64_t sym = 0, off = 0, succ = 0, nbm = 0;
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const MultiGraphPlan& gp = pl.graphs[g];
        const FlatGraph& fg = *in[g].g;
        CHECK(gp.n_succ == fg.succ_rows.size() && gp.n_nbm == fg.nbm.size() && gp.n_exit == fg.n_exit);
        CHECK(gp.sym_base % 4 == 0 && gp.sym_base + fg.n + 4 <= pl.n_sym_total);
        CHECK(gp.off_base + fg.n + 1 <= pl.n_off_total && gp.succ_base + gp.n_succ <= pl.n_succ_total && gp.nbm_base + gp.n_nbm <= pl.n_nbm_total);
        if (gp.table_of == g) {
            CHECK(gp.sym_base == sym && gp.off_base == off && gp.succ_base == succ && gp.nbm_base == nbm);   // back to back: disjoint
            sym += ((uint64_t)fg.n + 4 + 3) & ~3ull; off += fg.n + 1; succ += gp.n_succ; nbm += gp.n_nbm;
        } else {
            const MultiGraphPlan& first = pl.graphs[gp.table_of];
            CHECK(in[gp.table_of].g == in[g].g && first.sym_base == gp.sym_base && first.off_base == gp.off_base && first.succ_base == gp.succ_base &&
                  first.nbm_base == gp.nbm_base && first.row_base == gp.row_base);
        }
    }
    CHECK(sym == pl.n_sym_total && off == pl.n_off_total && succ == pl.n_succ_total && nbm == pl.n_nbm_total);

    // the footprint: per query the dense region and the visited table, each with 256 bytes of padding
    uint64_t total = 0, largest = 0;
    std::vector<uint64_t> qbytes(n);
    for (uint32_t i = 0; i < n; ++i) {
        const FlatGraph& fg = *in[pl.graph_of[i]].g;
        const uint64_t L = qoff[i + 1] - qoff[i];
        qbytes[i] = 2 * dense_elems(fg, L) + 256 + 4 * 3ull * fg.n * pitch_of(L) + 256;
        total += qbytes[i]; largest = std::max(largest, qbytes[i]);
    }
    CHECK(total == pl.bytes_total && largest == pl.largest_query_bytes);

    // chunks
    const uint64_t budget = ws == 0 ? total : std::max(ws, largest);
    uint32_t next = 0, slots = 0;
    uint64_t max_bytes = 0;
    for (size_t c = 0; c < pl.chunks.size(); ++c) {
        const MultiPlan::Chunk& ch = pl.chunks[c];
        CHECK(ch.first == next && ch.count > 0);
        next += ch.count; slots = std::max(slots, ch.count);
        const uint64_t bytes = ch.cells * 2 + ch.table_cells * 4;
        CHECK(bytes <= budget && bytes <= pl.workspace_bytes);
        CHECK((ch.cells * 2) % 16 == 0);
        uint64_t dense_end = 0, table_end = ch.cells / 2, sum = 0;   // tables start where the dense regions end, in four-byte cells
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
            const FlatGraph& fg = *in[pl.graph_of[i]].g;
            const uint64_t L = qoff[i + 1] - qoff[i];
            CHECK(pl.region_off[i] == dense_end && (pl.region_off[i] * 2) % 16 == 0);
            dense_end += dense_elems(fg, L) + MULTI_DENSE_PAD_ELEMS;
            CHECK(pl.table_off[i] == table_end && (pl.table_off[i] * 4) % 16 == 0);
            CHECK(multi_exact_table_cells(fg, L) == 3ull * fg.n * pitch_of(L));
            table_end += 3ull * fg.n * pitch_of(L) + MULTI_EXACT_PAD_CELLS;
            sum += qbytes[i];
        }
        CHECK(dense_end == ch.cells && table_end * 4 == bytes && sum == bytes);   // the dense regions, then the tables: disjoint, inside
        if (c + 1 < pl.chunks.size()) CHECK(bytes + qbytes[ch.first + ch.count] > budget);   // greedy: the next query did not fit
        max_bytes = std::max(max_bytes, bytes);
    }
    CHECK(next == n && max_bytes == pl.workspace_bytes && slots == pl.exact_slots);

    // the slot: the maxima over the graphs that have queries, and the sum the header documents
    uint64_t n_exit = 0, max_len = 0, stack = 8, pool = 256;
    uint32_t skew = 0;
    const double f = costs.queue_entries_per_cell > 0.f ? costs.queue_entries_per_cell : 0.25f;
    for (uint32_t g = 0; g < n_graphs; ++g) {
        if (gq[g + 1] == gq[g]) continue;
        const FlatGraph& fg = *in[g].g;
        uint64_t len = 0;
        for (uint64_t i = gq[g]; i < gq[g + 1]; ++i) len = std::max(len, qoff[i + 1] - qoff[i]);
        n_exit = std::max<uint64_t>(n_exit, fg.n_exit); max_len = std::max(max_len, len);
        stack = std::max<uint64_t>(stack, fg.n + len + 8);
        pool = std::max<uint64_t>(pool, (uint64_t)((float)f * (double)fg.n * (double)(len + 1)));
        for (uint32_t r = 0; r < fg.n; ++r) skew = std::max(skew, fg.dist_max[r] - std::min(fg.dist_min[r], fg.dist_max[r]));
    }
    const MultiExactSlot& s = pl.exact;
    uint32_t win = 64;
    while (win < std::max<uint64_t>(costs.x, costs.o + costs.e) + costs.o + ((uint64_t)skew + 3) * costs.e + 8) win *= 2;
    CHECK(s.win == win && s.win == multi_exact_win(costs.x, costs.o, costs.e, skew) && s.skew == skew);
    {
        // the one rule behind it (exact_replay_win): Global, a bounded graph begin and Dijkstra order are the jump term above,
        // whatever the frontier fields say; a free graph begin under the min-gap heuristic covers o + e * max(len, dist_max)
        ExactWinIn in;
        in.x = costs.x; in.o = costs.o; in.e = costs.e; in.skew = skew; in.max_len = 100000; in.dist_max = 100000;
        CHECK(exact_replay_win(in) == win);
        in.free_begin = true; in.mingap = false;
        CHECK(exact_replay_win(in) == win);
        in.mingap = true;
        CHECK(exact_replay_win_need(in) >= in.o + 100000ull * in.e + 8 && exact_replay_win(in) >= exact_replay_win_need(in) &&
              exact_replay_win(in) >= win && (exact_replay_win(in) & (exact_replay_win(in) - 1)) == 0);
        ExactWinIn c;   // costs 4 / 6 / 2, a chain: 32 nodes overflowed 64 priorities, 300 nodes put the ring in global memory
        c.free_begin = true; c.max_len = 32; c.dist_max = 33;
        CHECK(exact_replay_win(c) == 128);
        c.max_len = 300; c.dist_max = 301;
        CHECK(exact_replay_win(c) == 1024);
        c.free_begin = false;
        CHECK(exact_replay_win(c) == 64);
    }
    const uint64_t wpn = (max_len + 1 + 63) / 64, swpn = (wpn + 63) / 64;
    CHECK(s.n_exit == n_exit && s.wpn == wpn && s.swpn == swpn && s.stack_cap == stack);
    CHECK(s.pool_cap == ((pool + 64 * (3ull * win + 8) + 63) & ~63ull) && s.pool_cap % BQ_CHUNK == 0);
    CHECK(s.reached_stride == ((n_exit * wpn + 1) & ~1ull) && s.rsum_stride == ((n_exit * swpn + 1) & ~1ull));
    CHECK(s.bytes == s.reached_stride * 8 + s.rsum_stride * 8 + stack * 12 + (uint64_t)s.pool_cap * 16 + 3ull * win * 4);
    // the five arrays of `slots` slots: in this order, disjoint, aligned, inside the buffer
    const uint64_t S = pl.exact_slots;
    CHECK(s.off_reached(S) == 0 && s.off_rsum(S) == S * s.reached_stride * 8 && s.off_stack(S) == s.off_rsum(S) + S * s.rsum_stride * 8);
    CHECK(s.off_pool(S) >= s.off_stack(S) + S * s.stack_cap * 12 && s.off_pool(S) % 16 == 0 && s.off_rsum(S) % 16 == 0 && s.off_stack(S) % 16 == 0);
    CHECK(s.off_ring(S) == s.off_pool(S) + S * (uint64_t)s.pool_cap * 16 && s.off_ring(S) + S * 3 * win * 4 <= s.buffer_bytes(S));
    CHECK(s.buffer_bytes(S) >= S * s.bytes && s.buffer_bytes(S) <= S * s.bytes + 64);
    CHECK(pl.exact_bytes == (n ? s.buffer_bytes(S) : 0));
}

struct Outcome {
    ExactResult R;
    std::vector<uint32_t> T;
};

ExactGraph graph_of(const FlatGraph& g, const std::vector<uint8_t>& row_sym) {
    return ExactGraph{g.n, g.start_row, g.end_row, row_sym.data(), g.succ_row_off.data(), g.succ_rows.data(), g.dist_min.data(), g.dist_max.data(),
                      g.exit_idx.data(), g.n_exit, g.nbm_off.data(), g.nbm.data(), nullptr, nullptr, g.row_rec.empty() ? nullptr : g.row_rec.data()};
}

// one query's search on the workspace W points at (the instantiation of the wave kernel's default path)
Outcome search(const FlatGraph& g, const std::vector<uint8_t>& seq, ExactWork W, const MultiExactCosts& c, uint32_t prune) {
    std::vector<uint8_t> row_sym((size_t)g.n + 4, 0);
    for (uint32_t r = 0; r < g.n; ++r) row_sym[r] = g.rows[r].sym;
    const ExactGraph G = graph_of(g, row_sym);
    Outcome out;
    out.T.assign((size_t)3 * g.n * pitch_of(seq.size()), EX_INF);
    W.T = out.T.data(); W.n_rows = g.n; W.pitch = pitch_of(seq.size());
    for (uint32_t i = 0; i < 3 * W.bq_win; ++i) W.bq_desc[i] = BQ_EMPTY;   // the wave clears its ring
    ExactCosts EC{c.x, c.o, c.e, 1u /* min-gap */, prune, 0, 0, 0, 0, 0, 0};
    ExactSearchT<EX_AS_NO_SPEC | EX_AS_REC_LDS> S(G, W, seq.data(), (uint32_t)seq.size(), EC);
    out.R = S.run_buckets(32);
    return out;
}

}  // namespace

int main() {
    FlatGraph chain, ladder, bubble, tiny, empty;
    std::vector<uint8_t> ladder_seq;
    { Builder b; b.path(40, 1); finish(b, chain); }
    snp_ladder(12, ladder, ladder_seq);
    {
        Builder b;
        auto back = b.path(12, 2);
        for (uint32_t len : {1u, 2u, 4u}) { auto br = b.path(len, len); b.edge(back[2], br[0]); b.edge(br.back(), back[8]); }
        b.edge(back[1], back[10]);   // a bypass edge: a large dist_max - dist_min
        finish(b, bubble);
    }
    { Builder b; b.node('A'); finish(b, tiny); }
    { Builder b; finish(b, empty); }
    // (the reference's index makes every node of a chain the exit of a one-node bubble: a chain has MORE exits than the ladder)
    CHECK(chain.n_exit != ladder.n_exit && ladder.n_exit >= 12 && chain.n_exit >= 40);
    CHECK(tiny.n == 3 && empty.n_real == 0);

    // ---- the plan ------------------------------------------------------------------------------------------------------------
    const FlatGraph* listed[] = {&tiny, &chain, &ladder, &bubble, &empty, &ladder};
    std::vector<MultiGraphIn> in;
    for (const FlatGraph* g : listed) in.push_back(MultiGraphIn{g, nullptr, nullptr});
    const std::vector<std::vector<uint64_t>> lens = {{0, 1, 2}, {3, 63, 64, 200}, {30, 31, 200}, {12, 64}, {4, 0}, {25, 1023}};
    std::vector<uint64_t> gq{0}, qoff{0};
    for (const auto& ls : lens) {
        for (uint64_t l : ls) qoff.push_back(qoff.back() + l);
        gq.push_back(qoff.size() - 1);
    }
    const uint32_t ng = (uint32_t)in.size();
    std::string err;
    MultiPlan whole, p;
    const MultiExactCosts c0;                      // 4 / 6 / 2: a ring of 64 priorities
    MultiExactCosts c1; c1.x = 40; c1.o = 30; c1.e = 3; c1.queue_entries_per_cell = 1.5f;
    CHECK(build_multi_exact_plan(in.data(), ng, gq.data(), qoff.data(), 0, c0, whole, err) == 0);
    check_plan(in, gq, qoff, 0, c0, whole);
    CHECK(whole.chunks.size() == 1 && whole.workspace_bytes == whole.bytes_total && whole.exact_slots == whole.n_queries);
    CHECK(whole.exact.win == 64);
    CHECK(build_multi_exact_plan(in.data(), ng, gq.data(), qoff.data(), 0, c1, p, err) == 0);
    check_plan(in, gq, qoff, 0, c1, p);
    CHECK(p.exact.win > 64 && p.exact.pool_cap > whole.exact.pool_cap);   // costs 40 / 30 / 3: a ring wider than 64
    {   // a run with other costs recomputes the slot from what the plan holds
        MultiExactSlot s2;
        CHECK(multi_exact_slot(whole, c1, s2, err) == 0 && s2.win == p.exact.win && s2.bytes == p.exact.bytes);
    }
    for (uint64_t ws : {whole.largest_query_bytes + 256, (uint64_t)1, whole.largest_query_bytes, whole.bytes_total - 1, whole.bytes_total / 2, whole.bytes_total / 5}) {
        CHECK(build_multi_exact_plan(in.data(), ng, gq.data(), qoff.data(), ws, c0, p, err) == 0);
        check_plan(in, gq, qoff, ws, c0, p);
        CHECK(p.chunks.size() >= 2 && p.exact_slots < p.n_queries);
        if (ws == whole.bytes_total / 5) {
            bool inside = false;
            for (size_t c = 1; c < p.chunks.size(); ++c) inside = inside || p.graph_of[p.chunks[c].first] == p.graph_of[p.chunks[c].first - 1];
            CHECK(inside);   // a boundary inside a graph's range
        }
    }
    {   // refusals: 1024 symbols, an index that was not built, the argument errors of the dense plan
        const std::vector<uint64_t> g1{0, 1}, wide{0, 1024};
        CHECK(build_multi_exact_plan(in.data(), 1, g1.data(), wide.data(), 0, c0, p, err) == -7 && err.find("poa_align_batch_ex") != std::string::npos);
        FlatGraph raw;
        { Builder b; b.path(5, 0); finish(b, raw, false); }
        const MultiGraphIn raw_in{&raw, nullptr, nullptr};
        const std::vector<uint64_t> one{0, 3};
        CHECK(build_multi_exact_plan(&raw_in, 1, g1.data(), one.data(), 0, c0, p, err) == -1 && err.find("bubble index") != std::string::npos);
        std::vector<uint64_t> bad = gq;
        bad[0] = 1;
        CHECK(build_multi_exact_plan(in.data(), ng, bad.data(), qoff.data(), 0, c0, p, err) == -1);
        CHECK(build_multi_exact_plan(in.data(), ng, nullptr, qoff.data(), 0, c0, p, err) == -1);
        const uint64_t zero[2] = {0, 0};
        CHECK(build_multi_exact_plan(nullptr, 0, zero, zero, 0, c0, p, err) == 0 && p.chunks.empty() && p.bytes_total == 0 && p.exact_bytes == 0);
        MultiExactCosts huge = c0; huge.queue_entries_per_cell = 1e7f;
        CHECK(build_multi_exact_plan(in.data(), ng, gq.data(), qoff.data(), 0, huge, p, err) == -7 && err.find("queue pool") != std::string::npos);
    }

    // ---- interleaved searches at the plan's strides -----------------------------------------------------------------------------
    // ladder, chain, ladder, chain, ...: eight of each, reads of the ladder's backbone and of the chain with a few edits
    const uint32_t pairs_n = 8;
    std::vector<MultiGraphIn> in2;
    std::vector<std::vector<uint8_t>> seqs;
    std::vector<uint64_t> gq2{0}, qoff2{0};
    std::vector<uint8_t> chain_seq;
    for (uint32_t r = 0; r < chain.n; ++r) if (r != chain.start_row && r != chain.end_row) chain_seq.push_back(chain.rows[r].sym);
    for (uint32_t k = 0; k < pairs_n; ++k) {
        for (int which = 0; which < 2; ++which) {
            std::vector<uint8_t> s = which == 0 ? ladder_seq : chain_seq;
            s[(3 * k + 5) % s.size()] = "ACGT"[(k + which) & 3];           // a substitution
            s.erase(s.begin() + (long)((5 * k + 9) % s.size()));           // a deletion
            s.insert(s.begin() + (long)((7 * k + 2) % s.size()), "TGCA"[k & 3]);   // an insertion
            if (k == 7) s.resize(which == 0 ? 3 : 1);
            in2.push_back(MultiGraphIn{which == 0 ? &ladder : &chain, nullptr, nullptr});
            seqs.push_back(s);
            qoff2.push_back(qoff2.back() + s.size());
            gq2.push_back(qoff2.size() - 1);
        }
    }
    for (const MultiExactCosts& cc : {c0, c1}) {
        MultiPlan pl;
        CHECK(build_multi_exact_plan(in2.data(), (uint32_t)in2.size(), gq2.data(), qoff2.data(), 0, cc, pl, err) == 0);
        check_plan(in2, gq2, qoff2, 0, cc, pl);
        const MultiExactSlot& s = pl.exact;
        const uint64_t S = pl.exact_slots;
        CHECK(S == 2 * pairs_n && s.n_exit == std::max(ladder.n_exit, chain.n_exit) && pl.n_rows_total == (uint64_t)ladder.n + chain.n);
        {   // with the graph's own stride (slot * n_exit(graph) * wpn) two slots overlap: the bug the stride rule is for
            bool overlap = false;
            for (uint32_t a = 0; a < S; ++a)
                for (uint32_t b2 = a + 1; b2 < S; ++b2) {
                    const uint64_t ea = in2[a].g->n_exit, eb = in2[b2].g->n_exit;
                    const uint64_t a0 = a * ea * s.wpn, a1 = a0 + ea * s.wpn, b0 = b2 * eb * s.wpn, b1 = b0 + eb * s.wpn;
                    overlap = overlap || (a0 < b1 && b0 < a1);
                }
            CHECK(overlap);
        }
        // one buffer; canaries everywhere, then the clears of the run: the reached sets and summaries of every slot's OWN range
        std::vector<uint8_t> buf(s.buffer_bytes(S), 0xC5);
        uint64_t* reached = reinterpret_cast<uint64_t*>(buf.data() + s.off_reached(S));
        uint64_t* rsum = reinterpret_cast<uint64_t*>(buf.data() + s.off_rsum(S));
        ExStackEntry* stack = reinterpret_cast<ExStackEntry*>(buf.data() + s.off_stack(S));
        ExU4* chunks = reinterpret_cast<ExU4*>(buf.data() + s.off_pool(S));
        uint32_t* ring = reinterpret_cast<uint32_t*>(buf.data() + s.off_ring(S));
        const uint64_t canary = 0xC5C5C5C5C5C5C5C5ull;
        for (uint32_t slot = 0; slot < S; ++slot) {
            const FlatGraph& fg = *in2[pl.graph_of[slot]].g;
            std::memset(reached + slot * s.reached_stride, 0, (size_t)fg.n_exit * s.wpn * 8);
            std::memset(rsum + slot * s.rsum_stride, 0, (size_t)fg.n_exit * s.swpn * 8);
        }
        bool pruned_any = false;
        std::vector<Outcome> got(S);
        for (uint32_t slot = 0; slot < S; ++slot) {
            const FlatGraph& fg = *in2[pl.graph_of[slot]].g;
            ExactWork W{};
            // the kernel's arithmetic: the biased base, then the search's own slot * n_exit * wpn
            uint64_t* rb = reached + (uint64_t)slot * (s.reached_stride - (uint64_t)fg.n_exit * s.wpn);
            uint64_t* sb = rsum + (uint64_t)slot * (s.rsum_stride - (uint64_t)fg.n_exit * s.swpn);
            W.reached = rb + (uint64_t)slot * fg.n_exit * s.wpn;
            W.rsum = sb + (uint64_t)slot * fg.n_exit * s.swpn;
            CHECK(W.reached == reached + slot * s.reached_stride && W.rsum == rsum + slot * s.rsum_stride);
            W.wpn = s.wpn; W.swpn = s.swpn;
            W.head = nullptr; W.n_prio = 0xFFFFFFFFu; W.pool = nullptr; W.pool_cap = 0;
            W.stack = stack + (uint64_t)slot * s.stack_cap; W.stack_cap = s.stack_cap;
            W.bq_desc = ring + (uint64_t)slot * 3 * s.win; W.bq_win = s.win;
            W.bq_chunks = chunks + (uint64_t)slot * (s.pool_cap / BQ_CHUNK) * BQ_CHUNK; W.bq_chunk_cap = s.pool_cap / BQ_CHUNK;
            got[slot] = search(fg, seqs[slot], W, cc, 1);
        }
        for (uint32_t slot = 0; slot < S; ++slot) {
            const FlatGraph& fg = *in2[pl.graph_of[slot]].g;
            // the same search alone: a workspace of its own, sized as the single-graph call sizes it
            const uint64_t L = seqs[slot].size();
            const uint32_t wpn = (uint32_t)((L + 1 + 63) / 64), swpn = (wpn + 63) / 64;
            std::vector<uint64_t> r1((size_t)fg.n_exit * wpn + 1, 0), s1((size_t)fg.n_exit * swpn + 1, 0);
            std::vector<ExStackEntry> st1(fg.n + L + 8);
            std::vector<uint32_t> ring1((size_t)3 * s.win);
            std::vector<ExU4> ch1((size_t)s.pool_cap);
            ExactWork W{};
            W.reached = r1.data(); W.rsum = s1.data(); W.wpn = wpn; W.swpn = swpn;
            W.head = nullptr; W.n_prio = 0xFFFFFFFFu; W.pool = nullptr; W.pool_cap = 0;
            W.stack = st1.data(); W.stack_cap = (uint32_t)st1.size();
            W.bq_desc = ring1.data(); W.bq_win = s.win; W.bq_chunks = ch1.data(); W.bq_chunk_cap = s.pool_cap / BQ_CHUNK;
            const Outcome alone = search(fg, seqs[slot], W, cc, 1);
            CHECK(alone.R.status == EX_OK && got[slot].R.status == EX_OK);
            CHECK(alone.R.score == got[slot].R.score && alone.R.end_row == got[slot].R.end_row && alone.R.end_off == got[slot].R.end_off);
            CHECK(alone.R.num_queued == got[slot].R.num_queued && alone.R.num_visited == got[slot].R.num_visited && alone.R.num_pruned == got[slot].R.num_pruned);
            CHECK(alone.T == got[slot].T);
            pruned_any = pruned_any || alone.R.num_pruned > 0;
            // no canary moved: what lies between the slot's own reached rows and the next slot
            for (uint64_t w = (uint64_t)fg.n_exit * s.wpn; w < s.reached_stride; ++w) CHECK(reached[slot * s.reached_stride + w] == canary);
            for (uint64_t w = (uint64_t)fg.n_exit * s.swpn; w < s.rsum_stride; ++w) CHECK(rsum[slot * s.rsum_stride + w] == canary);
        }
        CHECK(pruned_any);   // reached marks were set and used
        // the gap between the stack array and the pool, and the buffer's tail
        for (uint64_t bb = s.off_stack(S) + S * s.stack_cap * 12; bb < s.off_pool(S); ++bb) CHECK(buf[bb] == 0xC5);
        for (uint64_t bb = s.off_ring(S) + S * 3 * s.win * 4; bb < buf.size(); ++bb) CHECK(buf[bb] == 0xC5);
    }
    std::printf("multi_exact_host ok\n");
    return 0;
}
