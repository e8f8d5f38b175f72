// Test harness (CPU): compiles the PRODUCT's derivation of the two gap-state traceback flags
// (poasta_amd/csrc/poa_tb_derive.hpp) and its graph preprocessing (poa_graph.cpp) for the host, feeds it what the compact
// format of poa_forward_px_kernel<3> keeps of a query's planes — the M values, the flags I == M and D == M, the D rows
// flagged ROW_STORE_D — and compares the derived flags of EVERY cell with the ones the full I and D planes give.
// derive_host_check_clamped feeds the same planes as a format with a score limit stores them: an M value or a kept D value at
// or above the limit reads INF, and the two flags of such an M cell are whatever the caller says (they are undefined).
// Not shipped; built by tests/test_derived_gap_flags.py.
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/poasta_amd.h"
#include "../../poasta_amd/csrc/poa_graph.hpp"
#include "../../poasta_amd/csrc/poa_tb_derive.hpp"

using namespace poa_amd;

namespace {

constexpr uint32_t INF32 = 0xFFFFFFFFu;

struct HostCtx {
    const RowMeta* rows;
    const uint32_t* pred_rows;
    const uint8_t* q;
    uint32_t L, o, e;
    const FlatGraph* g;
    const uint32_t *M, *I, *D;   // [node][L + 1]
    mutable uint64_t bad_d_reads = 0;   // reads of a D row the compact layout does not keep
    uint32_t limit = INF32;             // values at or above it read INF (INF32: the planes as they are)
    uint32_t clamped_flags = 0;         // the flags A and C of a cell whose M is clamped
    uint64_t at(uint32_t row, uint32_t j) const { return (uint64_t)rows[row].node * (L + 1) + j; }
    void cell(uint32_t row, uint32_t j, uint32_t& v, uint32_t& a, uint32_t& c) const {
        v = M[at(row, j)]; a = I[at(row, j)] == v; c = D[at(row, j)] == v;
        if (limit != INF32 && v >= limit) { v = INF32; a = c = clamped_flags; }
    }
    uint32_t m(uint32_t row, uint32_t j) const { return M[at(row, j)] >= limit ? INF32 : M[at(row, j)]; }
    uint32_t d_kept(uint32_t row, uint32_t j) const {
        if (!(rows[row].flags & ROW_STORE_D)) bad_d_reads++;
        return D[at(row, j)] >= limit ? INF32 : D[at(row, j)];
    }
    uint32_t pred(uint32_t k) const { return pred_rows[k]; }
    uint32_t pred_d(uint32_t k, uint32_t j) const { return d_kept(pred_rows[k], j); }
};

}  // namespace

extern "C" {

// planes by NODE, [n][len + 1] u32 (INF = 0xFFFFFFFF).  out[0..1] = cells checked for B / D, out[2..3] = differences,
// out[4] = reads of a D row that is not kept, out[5..7] = (state, row, column) of the first difference.
// Returns 0, or a negative POA_ERR_* for graph errors.
//
// limit != 0xFFFFFFFF: the planes are read as a format with that score limit stores them (M and kept D at or above it are INF,
// the flags of such an M cell are clamped_flags, 0 or 1), and the cells checked are those whose carried value, the true I resp. D,
// is finite and BELOW the limit: the walks' targets are below it, so a clamped cell lies above every target.
static int check(uint32_t n, uint32_t start, uint32_t end, const uint8_t* symbol, const uint32_t* succ_off,
                 const uint32_t* succ, const uint32_t* pred_off, const uint32_t* pred, uint8_t o, uint8_t e,
                 const uint8_t* seq, uint32_t len, const uint32_t* pm, const uint32_t* pi, const uint32_t* pd, uint32_t limit,
                 uint32_t clamped_flags, uint64_t* out) {
    FlatGraph g;
    std::string err;
    const int rc = build_flat_graph(n, start, end, symbol, succ_off, succ, pred_off, pred, g, err);
    if (rc != POA_OK) return rc;
    HostCtx c{g.rows.data(), g.pred_rows.data(), seq, len, o, e, &g, pm, pi, pd};
    c.limit = limit;
    c.clamped_flags = clamped_flags ? 1u : 0u;
    for (int k = 0; k < 8; ++k) out[k] = 0;
    auto differ = [&](uint32_t st, uint32_t r, uint32_t j) {
        if (out[2] + out[3] == 0) { out[5] = st; out[6] = r; out[7] = j; }
        out[st == 2 ? 2 : 3]++;
    };
    for (uint32_t r = 0; r < g.n; ++r) {
        const RowMeta m = g.rows[r];
        for (uint32_t j = 0; j <= len; ++j) {
            const uint32_t iv = pi[c.at(r, j)], dv = pd[c.at(r, j)];
            if (iv != INF32 && iv < limit && j > 0) {
                const uint32_t il = pi[c.at(r, j - 1)];
                const bool want = il != INF32 && il + e == iv;
                out[0]++;
                if (tbd_i_extends(c, m, r, j, iv) != want) differ(2, r, j);
            }
            if (dv != INF32 && dv < limit && (m.flags & ROW_CHAIN)) {
                const uint32_t du = pd[c.at(r - 1, j)];
                const bool want = du != INF32 && du + e == dv;
                out[1]++;
                if (tbd_d_extends(c, r, j, dv) != want) differ(1, r, j);
            }
        }
    }
    out[4] = c.bad_d_reads;
    return 0;
}

int derive_host_check(uint32_t n, uint32_t start, uint32_t end, const uint8_t* symbol, const uint32_t* succ_off,
                      const uint32_t* succ, const uint32_t* pred_off, const uint32_t* pred, uint8_t o, uint8_t e,
                      const uint8_t* seq, uint32_t len, const uint32_t* pm, const uint32_t* pi, const uint32_t* pd, uint64_t* out) {
    return check(n, start, end, symbol, succ_off, succ, pred_off, pred, o, e, seq, len, pm, pi, pd, INF32, 0, out);
}

int derive_host_check_clamped(uint32_t n, uint32_t start, uint32_t end, const uint8_t* symbol, const uint32_t* succ_off,
                              const uint32_t* succ, const uint32_t* pred_off, const uint32_t* pred, uint8_t o, uint8_t e,
                              const uint8_t* seq, uint32_t len, const uint32_t* pm, const uint32_t* pi, const uint32_t* pd,
                              uint32_t limit, uint32_t clamped_flags, uint64_t* out) {
    return check(n, start, end, symbol, succ_off, succ, pred_off, pred, o, e, seq, len, pm, pi, pd, limit, clamped_flags, out);
}

// rows flagged ROW_CHAIN, as nodes (so that the test can count the cells itself)
int derive_host_chain_nodes(uint32_t n, uint32_t start, uint32_t end, const uint8_t* symbol, const uint32_t* succ_off,
                            const uint32_t* succ, const uint32_t* pred_off, const uint32_t* pred, uint8_t* is_chain) {
    FlatGraph g;
    std::string err;
    const int rc = build_flat_graph(n, start, end, symbol, succ_off, succ, pred_off, pred, g, err);
    if (rc != POA_OK) return rc;
    for (uint32_t r = 0; r < g.n; ++r) is_chain[g.rows[r].node] = (g.rows[r].flags & ROW_CHAIN) ? 1 : 0;
    return 0;
}

}  // extern "C"
