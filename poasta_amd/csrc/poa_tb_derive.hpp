// The two gap-state flags of a cell, derived where the traceback needs them instead of stored by the forward pass
// (TbParams::code_fmt 4: a cell keeps its score and the flags A: I == M, C: D == M only).  Host and device: the CPU test
// (tests/test_derived_gap_flags.py) runs these very functions over every cell of the oracle's planes.
//
//   B at (r, j), carried cs = I[r][j]:        is I[r][j-1] == cs - e ?
//   D at (r, j), r a chain row, cs = D[r][j]: is D[r-1][j] == cs - e ?
//
// Both walk back along the gap (B: to the left in the row, D: up the chain) asking at each cell c "is G[c] == tt ?" for the
// gap plane G and a target tt that shrinks by e per cell, and both know G[c] >= tt throughout (G[next] <= G[c] + e and
// G[first] >= tt because the cell the walk stands in is a minimum over it).  At a cell:
//   * M[c] > tt (INF included): M <= G, so G[c] != tt                                                          -> false
//   * the cell's flag says G[c] == M[c] (A resp. C), or G[c] is stored (a kept D row), or the row has other predecessors
//     than the one above (their D rows are kept: one exact evaluation)                                          -> G[c] == tt
//   * a gap may open into c from the cell before it, c', and M[c'] + o + e == tt: G[c] <= that and G[c] >= tt  -> true
//     (M stands in for H of the insertion recurrence: where M[c'] = I[c'] < H[c'] the sum is >= I[c'] + e >= I[c], o >= 0)
//   * otherwise G[c] == tt exactly if its extension G[c'] + e == tt: go on at c' with tt - e.
// Stored scores of cells that no optimal path can use may be clamped to INF (the 14-bit format): such a value only ever
// stands where the true one also exceeds every target of a walk (targets are <= the final score).
//
// Ctx provides:  rows (const RowMeta*), q, L, o, e;
//   cell(row, j, v, a, c)   score of the cell (INF = 0xFFFFFFFF) and its flags A, C — one load
//   m(row, j)               score of the cell
//   d_kept(row, j)          D[row][j] of a ROW_STORE_D row
//   pred(k), pred_d(k, j)   row of entry k of pred_rows, and D of that (kept) row at column j
#pragma once
#include <stdint.h>

#include "poa_graph.hpp"

#if defined(__HIPCC__)
#define TBD_HD __host__ __device__
#else
#define TBD_HD
#endif

namespace poa_amd {

constexpr uint32_t TBD_INF = 0xFFFFFFFFu;

template <typename Ctx>
TBD_HD inline bool tbd_open_i(const Ctx& c, const RowMeta& m, uint32_t j) {
    if (j >= c.L) return false;
    if (m.flags & ROW_OPENI_ALWAYS) return true;
    if (m.flags & ROW_OPENI_NEVER) return false;
    return (uint32_t)m.child_sym != (uint32_t)c.q[j];
}

// flag B of cell (row, j), j > 0, cs = I[row][j] finite: I[row][j] == I[row][j-1] + e.  `m` = rows[row] (not the end row: it has
// no insertion state)
template <typename Ctx>
TBD_HD inline bool tbd_i_extends(const Ctx& c, const RowMeta& m, uint32_t row, uint32_t j, uint32_t cs) {
    if (cs < c.e) return false;
    uint32_t tt = cs - c.e;
    uint32_t v, a, cf;
    c.cell(row, j - 1, v, a, cf);
    for (uint32_t col = j - 1; col > 0; --col) {   // I[row][0] = INF
        if (v > tt) return false;
        if (a) return v == tt;
        c.cell(row, col - 1, v, a, cf);
        if (v != TBD_INF && tbd_open_i(c, m, col - 1) && v + c.o + c.e == tt) return true;
        if (tt < c.e) return false;
        tt -= c.e;
    }
    return false;
}

// flag D of cell (row, j), row a chain row (the end row included), cs = D[row][j] finite: D[row][j] == D[row-1][j] + e
template <typename Ctx>
TBD_HD inline bool tbd_d_extends(const Ctx& c, uint32_t row, uint32_t j, uint32_t cs) {
    if (cs < c.e) return false;
    uint32_t tt = cs - c.e;
    uint32_t v, a, cf;
    c.cell(row - 1, j, v, a, cf);
    for (uint32_t r = row - 1;; --r) {
        const RowMeta m = c.rows[r];
        if (v > tt) return false;
        if (m.flags & ROW_STORE_D) return c.d_kept(r, j) == tt;
        if (cf) return v == tt;
        const bool open = j >= c.L || (uint32_t)m.sym != (uint32_t)c.q[j];
        if (!(m.flags & ROW_CHAIN)) {
            // the start row (no predecessor: D = INF) or a row whose predecessors all keep their D rows
            uint32_t d = TBD_INF;
            for (uint32_t k = 0; k < m.pred_count; ++k) {
                const uint32_t pd = c.pred_d(m.pred_begin + k, j);
                if (pd != TBD_INF && pd + c.e < d) d = pd + c.e;
                const uint32_t pm = open ? c.m(c.pred(m.pred_begin + k), j) : TBD_INF;
                if (pm != TBD_INF && pm + c.o + c.e < d) d = pm + c.o + c.e;
            }
            return d == tt;
        }
        c.cell(r - 1, j, v, a, cf);   // a chain row has the row above as its only predecessor
        if (open && v != TBD_INF && v + c.o + c.e == tt) return true;
        if (tt < c.e) return false;
        tt -= c.e;
    }
}

}  // namespace poa_amd
