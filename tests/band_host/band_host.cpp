// Test harness (CPU): compiles the PRODUCT's band plan (poasta_amd/csrc/poa_band_plan.cpp) and its graph preprocessing
// (poa_graph.cpp) for the host and hands the plan of one (graph, query length) to tests/test_band_plan.py, which checks it
// against the oracle's dense planes.  Not shipped; built by that test.
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/poasta_amd.h"
#include "../../poasta_amd/csrc/poa_band_plan.hpp"
#include "../../poasta_amd/csrc/poa_graph.hpp"

using namespace poa_amd;

extern "C" {

// hdr[0] = D, hdr[1] = segments; bases[segments]; node_row[n]; tabs[4][n] by ROW: a_min, a_max, c_min, c_max (0xFFFFFFFF: the
// row lies on no start -> end path).  Returns 0, or a negative POA_ERR_* for graph errors.
int band_host_plan(uint32_t n, uint32_t start, uint32_t end, const uint8_t* symbol, const uint32_t* succ_off, const uint32_t* succ,
                   const uint32_t* pred_off, const uint32_t* pred, uint32_t len, uint32_t seg_rows, uint32_t window, uint32_t* hdr,
                   uint32_t* bases, uint32_t* node_row, uint32_t* tabs) {
    FlatGraph g;
    std::string err;
    const int rc = build_flat_graph(n, start, end, symbol, succ_off, succ, pred_off, pred, g, err);
    if (rc != POA_OK) return rc;
    BandTables t;
    build_band_tables(g, t);
    hdr[1] = band_segments(g.n, seg_rows);
    hdr[0] = plan_band(g, t, len, seg_rows, window, bases);
    for (uint32_t v = 0; v < g.n; ++v) node_row[v] = g.node_row[v];
    for (uint32_t r = 0; r < g.n; ++r) {
        tabs[r] = t.a_min[r]; tabs[g.n + r] = t.a_max[r]; tabs[2 * g.n + r] = t.c_min[r]; tabs[3 * g.n + r] = t.c_max[r];
    }
    return 0;
}

// the columns of every row with ds + de <= D, as the plan computes them: lo[r] .. hi[r] (lo > hi: none)
int band_host_intervals(uint32_t n, uint32_t start, uint32_t end, const uint8_t* symbol, const uint32_t* succ_off, const uint32_t* succ,
                        const uint32_t* pred_off, const uint32_t* pred, uint32_t len, uint32_t D, uint32_t* lo, uint32_t* hi) {
    FlatGraph g;
    std::string err;
    const int rc = build_flat_graph(n, start, end, symbol, succ_off, succ, pred_off, pred, g, err);
    if (rc != POA_OK) return rc;
    BandTables t;
    build_band_tables(g, t);
    for (uint32_t r = 0; r < g.n; ++r)
        if (!band_row_interval(t, r, len, D, lo[r], hi[r])) { lo[r] = 1; hi[r] = 0; }
    return 0;
}

}  // extern "C"
