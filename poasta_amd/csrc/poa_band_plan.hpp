// Band plan of the one-strip dense forward pass (poa_forward_band.hpp): for a graph and a query length, the widest exact band
// whose rows fit a fixed window of columns that is re-based once per segment of rows.  Host code, no device dependency: the
// CPU test (tests/test_band_plan.py) runs it against the oracle's planes.
//
// Real nodes only are counted (the start and end rows consume nothing).  For a row r and a query of length L:
//   a_min[r], a_max[r]   fewest / most real nodes on a start -> r path, r itself included (the end row: its predecessors' value)
//   c_min[r], c_max[r]   fewest / most real nodes on a path after r to the end
//   ds(r, j) = dist(j, [a_min, a_max])     de(r, j) = dist(L - j, [c_min, c_max])     dist(v, [lo, hi]) = max(0, lo - v, v - hi)
// Every move changes ds and de by at most one and costs at least e whenever it does, so every state value of cell (r, j) is
// >= e * ds and every path from it to the end costs >= e * de.  band(D) = { (r, j) : ds + de <= D }; DESIGN.md §6, "Banded one-strip kernel" shows that a
// pass which reads every cell outside a superset of band(D) as INF gives the full pass's result for every query whose score
// is <= e * (D - 4) (two of the four for the neighbours the traceback reads, two for the window's left edge).  The plan depends on the graph and the length alone, not on the costs.
#pragma once
#include <cstdint>
#include <vector>

#include "poa_graph.hpp"

namespace poa_amd {

constexpr uint32_t BAND_SEG_ROWS = 64;     // rows per segment: the window moves only at multiples of it
constexpr uint32_t BAND_WINDOW = 512;      // columns per window
constexpr uint32_t BAND_WINDOW_NARROW = 384;   // columns per window of the narrow tier: a second plan per class, same segments and alignment
constexpr uint32_t BAND_BASE_ALIGN = 8;    // a window starts at a multiple of it
constexpr uint32_t BAND_NONE = 0xFFFFFFFFu;
constexpr uint32_t BAND_D_MAX = 65535;     // no score of a 14-bit plane needs a wider band

struct BandTables {
    std::vector<uint32_t> a_min, a_max, c_min, c_max;   // by row; BAND_NONE: not on any start -> end path
};

// the four distance tables of a flattened graph (one forward and one backward pass over the rows)
void build_band_tables(const FlatGraph& g, BandTables& out);

// the columns j in [0, L] of row r with ds + de <= D: false if there are none
bool band_row_interval(const BandTables& t, uint32_t r, uint32_t L, uint32_t D, uint32_t& lo, uint32_t& hi);

inline uint32_t band_segments(uint32_t n_rows, uint32_t seg_rows = BAND_SEG_ROWS) { return (n_rows + seg_rows - 1) / seg_rows; }

// The largest D <= BAND_D_MAX for which, in every segment of seg_rows rows, the rows' bands fit [base, base + window) with base a
// multiple of BAND_BASE_ALIGN; bases[band_segments(n, seg_rows)] receives the bases for that D (a segment without band cells takes
// the base of the segment before it).  Returns 0 (and bases of band(0), which may not fit) if not even band(0) fits: a class whose
// D < 4 is "no band".
uint32_t plan_band(const FlatGraph& g, const BandTables& t, uint32_t L, uint32_t seg_rows, uint32_t window, uint32_t* bases);

}  // namespace poa_amd
