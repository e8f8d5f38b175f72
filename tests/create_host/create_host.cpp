// Stand-alone check of the two pure rules the batch constructors of poa_engine.hip share (poasta_amd/csrc/poa_dense_plan.hpp):
// choose_workspace and concat_tables, and of two_piece_workspace, the workspace a one-shot two-piece call asks for.  Built by tests/test_create_frame.py together with poa_dense_plan.cpp under
// -fsanitize=address,undefined, and run on the CPU.
//
// The workspace table below was written out by hand from the four constructors as they stood before they shared the rule:
//     ws = requested
//     requested == 0:  avail = free > fixed ? (uint64_t)((free - fixed) * 0.85) : 0;  ws = min(total, avail)
//     a score-only or checkpointed resident batch (own footprint):  ws = min(ws, total)
//     ws < largest:    largest + fixed > free is refused (out of memory), else ws = largest
// with free - fixed a multiple of 100 wherever the 85 % matters, so that the product is a whole number.
// Exit code 0 and "create_host ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../poasta_amd/csrc/poa_dense_plan.hpp"
#include "../../poasta_amd/csrc/poa_multi_plan.hpp"

using namespace poa_amd;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "create_host: line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {
constexpr uint64_t REFUSED = ~0ull;

struct WsCase {
    const char* what;
    uint64_t requested, free_bytes, fixed, total, largest;
    uint64_t want, want_own;   // a batch that may hold more than its footprint; one that holds its own footprint, never more
};

const WsCase WS_CASES[] = {
    // requested 0: 85 % of 9000 is 7650, more than the batch needs
    {"0, room for everything", 0, 10000, 1000, 4000, 1500, 4000, 4000},
    // 85 % of 2000 is 1700: a cap, above the largest item
    {"0, room for less than the total", 0, 3000, 1000, 4000, 1500, 1700, 1700},
    // 1700 is below the largest item, which still fits beside `fixed`: 1900 + 1000 <= 3000
    {"0, room for less than the largest item but it fits", 0, 3000, 1000, 4000, 1900, 1900, 1900},
    // nothing is available and 1500 + 1000 > 900
    {"0, free below fixed", 0, 900, 1000, 4000, 1500, REFUSED, REFUSED},
    {"1, raised to the largest item", 1, 10000, 1000, 4000, 1500, 1500, 1500},
    {"the largest item itself", 1500, 10000, 1000, 4000, 1500, 1500, 1500},
    {"between the largest item and the total", 2000, 10000, 1000, 4000, 1500, 2000, 2000},
    {"the total", 4000, 10000, 1000, 4000, 1500, 4000, 4000},
    // only the batch that holds its own footprint clamps a request above it
    {"above the total", 9000, 10000, 1000, 4000, 1500, 9000, 4000},
    // a request is not held against free memory unless it has to be raised: 9000 + 1000 > 3000 passes
    {"above the total and above free memory", 9000, 3000, 1000, 4000, 1500, 9000, 4000},
    // 1500 + 1000 > 2400, and at 2500 it fits exactly
    {"1, the largest item plus fixed exceeds free", 1, 2400, 1000, 4000, 1500, REFUSED, REFUSED},
    {"1, the largest item plus fixed equals free", 1, 2500, 1000, 4000, 1500, 1500, 1500},
    {"0, the largest item plus fixed exceeds free", 0, 2400, 1000, 4000, 1500, REFUSED, REFUSED},
    // one item: the total is the largest
    {"0, one item", 0, 10000, 1000, 1500, 1500, 1500, 1500},
    // an empty batch: nothing to raise to, nothing to refuse, even without free memory
    {"empty, 0", 0, 10000, 1000, 0, 0, 0, 0},
    {"empty, 0, free below fixed", 0, 900, 1000, 0, 0, 0, 0},
    {"empty, a request", 512, 10000, 1000, 0, 0, 512, 0},
};

void check_workspace() {
    for (const WsCase& c : WS_CASES) {
        const uint64_t got = choose_workspace(c.requested, c.free_bytes, c.fixed, c.total, c.largest, false);
        const uint64_t got_own = choose_workspace(c.requested, c.free_bytes, c.fixed, c.total, c.largest, true);
        if (got != c.want || got_own != c.want_own) {
            std::fprintf(stderr, "create_host: %s: got %llu / %llu, want %llu / %llu\n", c.what, (unsigned long long)got,
                         (unsigned long long)got_own, (unsigned long long)c.want, (unsigned long long)c.want_own);
            std::exit(1);
        }
    }
    CHECK(WORKSPACE_NO_FIT == REFUSED);
    // sizes of a real device: 85 % of (256 GiB - 1 GiB) is a cap of 216.75 GiB, a whole number of bytes
    const uint64_t GiB = 1ull << 30;
    CHECK(choose_workspace(0, 256 * GiB, GiB, 1000 * GiB, 2 * GiB, false) == 255 * GiB / 20 * 17);
    CHECK(choose_workspace(0, 256 * GiB, GiB, 100 * GiB, 2 * GiB, true) == 100 * GiB);
}

// The chunks of `sizes` over `ws` bytes with at most max_count items each: the greedy rule of build_chunk_plan (poa_engine.hip)
// restated; its evening-out keeps the number of chunks.  Returns the chunk count, the largest chunk in *max_chunk.
uint64_t greedy_chunks(const std::vector<uint64_t>& sizes, uint64_t ws, uint64_t max_count, uint64_t* max_chunk) {
    uint64_t chunks = 0, used = 0, count = 0;
    *max_chunk = 0;
    for (uint64_t need : sizes) {
        if ((used + need > ws || count >= max_count) && count > 0) { ++chunks; used = 0; count = 0; }
        used += need; ++count;
        *max_chunk = std::max(*max_chunk, count);
    }
    return chunks + (count ? 1 : 0);
}

// two_piece_workspace against the rule the one-shot two-piece call had when it kept a workspace of its own:
//     dense:   budget = min(0.6 x free, 64 GiB), floor(budget / per_query) queries per chunk, one at least
//     replay:  budget = 0.85 x free, floor(budget / (per_query + replay bytes + 1)) queries per chunk, one at least
// with per_query the planes of the longest query, which every query was given.
void check_two_piece_workspace() {
    const uint64_t GiB = 1ull << 30;
    // dense: the budget, never above the total, never below the largest query
    CHECK(two_piece_workspace(1000, 5000, 100, 0, false).bytes == 600);
    CHECK(two_piece_workspace(1000, 500, 100, 0, false).bytes == 500);
    CHECK(two_piece_workspace(100, 5000, 100, 0, false).bytes == 100);
    CHECK(two_piece_workspace(288 * GiB, 100 * GiB, GiB, 0, false).bytes == 64 * GiB);
    CHECK(two_piece_workspace(288 * GiB, 60 * GiB, GiB, 0, false).bytes == 60 * GiB);
    CHECK(two_piece_workspace(100 * GiB, 100 * GiB, GiB, 0, false).bytes == (uint64_t)(100 * GiB * 0.6));
    CHECK(two_piece_workspace(1000, 5000, 100, 0, false).max_slots == ~0u);
    // equal queries: ceil(n / floor(budget / per_query)) chunks at a budget just below, at and just above a multiple of the query
    const uint64_t q = 1000, n = 37;
    const std::vector<uint64_t> equal(n, q);
    for (uint64_t m : {1ull, 2ull, 5ull, 36ull, 37ull, 38ull})
        for (uint64_t budget : {m * q - 1, m * q, m * q + 1}) {
            uint64_t free_bytes = budget * 5 / 3 - 3;
            while ((uint64_t)(free_bytes * 0.6) < budget) ++free_bytes;
            CHECK((uint64_t)(free_bytes * 0.6) == budget);
            const TwoPieceWorkspace w = two_piece_workspace(free_bytes, n * q, q, 0, false);
            CHECK(w.bytes <= n * q && w.bytes >= q);
            const uint64_t per_chunk = std::max<uint64_t>(budget / q, 1);
            uint64_t max_chunk = 0;
            CHECK(greedy_chunks(equal, w.bytes, w.max_slots, &max_chunk) == (n + per_chunk - 1) / per_chunk);
        }
    // replay: planes and the search workspaces of the largest chunk stay within 85 % of free, a chunk holds a query at least,
    // and queries of mixed sizes never take more chunks than the uniform stride of the longest gave them
    const std::vector<std::vector<uint64_t>> batches = {
        std::vector<uint64_t>(50, 400),
        {400, 100, 100, 400, 100, 100, 100, 100, 400, 100, 100, 100, 100, 100, 100, 100, 100, 400, 100, 100},
        {400, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100},
        {100, 400},
        {400},
    };
    for (const auto& sizes : batches)
        for (uint64_t slot_bytes : {0ull, 1ull, 150ull, 400ull, 5000ull})
            for (uint64_t free_bytes = 100; free_bytes <= 40000; free_bytes += 37) {
                uint64_t total = 0, largest = 0;
                for (uint64_t s : sizes) { total += s; largest = std::max(largest, s); }
                const TwoPieceWorkspace w = two_piece_workspace(free_bytes, total, largest, slot_bytes, true);
                CHECK(w.bytes >= largest && w.bytes <= total && w.max_slots >= 1);
                uint64_t max_chunk = 0;
                const uint64_t chunks = greedy_chunks(sizes, w.bytes, w.max_slots, &max_chunk);
                const uint64_t budget = (uint64_t)(free_bytes * 0.85);
                if (largest + slot_bytes <= budget) CHECK(w.bytes + max_chunk * slot_bytes <= budget);
                else CHECK(max_chunk == 1);   // (not even one fits the budget: one query at a time, as before)
                const uint64_t before = std::max<uint64_t>(std::min<uint64_t>(sizes.size(), budget / (largest + slot_bytes + 1)), 1);
                CHECK(chunks <= (sizes.size() + before - 1) / before);
            }
}

// Three graphs of which the third repeats the first's handle, the second without rows in this table (a graph that has no
// d_slot table: its part of the concatenated table is what the caller filled it with).  The bases are the planner's: a distinct
// handle starts where the tables so far end, a repeated one shares the bases of its first listing.
void check_concat() {
    const std::vector<uint32_t> rows_a{10, 11, 12, 13, 14}, rows_b{20, 21, 22}, none;
    const std::vector<uint32_t> edges_a{100, 101, 102, 103, 104, 105, 106}, edges_b{200, 201};
    std::vector<MultiGraphPlan> graphs(3);
    graphs[0].table_of = 0; graphs[0].row_base = 0; graphs[0].edge_base = 0;
    graphs[1].table_of = 1; graphs[1].row_base = rows_a.size(); graphs[1].edge_base = edges_a.size();
    graphs[2].table_of = 0; graphs[2].row_base = 0; graphs[2].edge_base = 0;
    const size_t n_rows = rows_a.size() + rows_b.size(), n_edges = edges_a.size() + edges_b.size();

    std::vector<uint32_t> asked;
    std::vector<uint32_t> by_row(n_rows, 7u);
    concat_tables(by_row, graphs, &MultiGraphPlan::row_base, [&](uint32_t g) -> const std::vector<uint32_t>& {
        asked.push_back(g);
        return g == 1 ? rows_b : rows_a;
    });
    CHECK((asked == std::vector<uint32_t>{0, 1}));   // one copy per distinct handle: the repeat is never read
    CHECK((by_row == std::vector<uint32_t>{10, 11, 12, 13, 14, 20, 21, 22}));

    std::vector<uint32_t> by_edge(n_edges, 7u);
    concat_tables(by_edge, graphs, &MultiGraphPlan::edge_base, [&](uint32_t g) -> const std::vector<uint32_t>& { return g == 1 ? edges_b : edges_a; });
    CHECK((by_edge == std::vector<uint32_t>{100, 101, 102, 103, 104, 105, 106, 200, 201}));

    // an empty table for the second graph: its range keeps the fill, the first graph's lies where it lay
    std::vector<uint32_t> sparse(n_rows, 7u);
    concat_tables(sparse, graphs, &MultiGraphPlan::row_base, [&](uint32_t g) -> const std::vector<uint32_t>& { return g == 1 ? none : rows_a; });
    CHECK((sparse == std::vector<uint32_t>{10, 11, 12, 13, 14, 7, 7, 7}));

    // ... and for a graph that ends the table: nothing is written at its base, the end of the table
    graphs[1].row_base = n_rows;
    std::vector<uint32_t> tail(n_rows, 7u);
    concat_tables(tail, graphs, &MultiGraphPlan::row_base, [&](uint32_t g) -> const std::vector<uint32_t>& { return g == 1 ? none : rows_a; });
    CHECK((tail == std::vector<uint32_t>{10, 11, 12, 13, 14, 7, 7, 7}));

    // another element type and another plan type: anything with table_of and a base of its own
    struct Listing { uint32_t table_of; uint64_t at; };
    const std::vector<Listing> listings{{0, 2}, {0, 2}, {2, 0}};
    const std::vector<uint8_t> first{1, 2}, third{3, 4};
    std::vector<uint8_t> bytes(4, 0);
    concat_tables(bytes, listings, &Listing::at, [&](uint32_t g) -> const std::vector<uint8_t>& { return g == 2 ? third : first; });
    CHECK((bytes == std::vector<uint8_t>{3, 4, 1, 2}));

    // no graphs, no table
    std::vector<uint32_t> nothing;
    concat_tables(nothing, std::vector<MultiGraphPlan>{}, &MultiGraphPlan::row_base, [&](uint32_t) -> const std::vector<uint32_t>& { return none; });
    CHECK(nothing.empty());
}
}  // namespace

int main() {
    check_workspace();
    check_two_piece_workspace();
    check_concat();
    std::printf("create_host ok\n");
    return 0;
}
