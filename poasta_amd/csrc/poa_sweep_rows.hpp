// Row liveness of the score-only sweep (POA_MODE_SCORE, poa_forward_sweep.hpp).  Host code, no device needed.
//
// The sweep keeps a row's M and D values in memory only while some later row still reads them.  In the engine's row order
// (FlatGraph::rows / pred_rows) a ROW_CHAIN row takes its only predecessor from registers, so a row has to outlive itself
// only if some successor is NOT the chain row directly below it (the criterion of ROW_STORE_D, applied to M as well, and
// without the end row, which nothing reads).  Such a row is live from its own index to the largest row index among its
// successors, both included: the successor reads it before it stores anything of its own.
//
// Slots are handed out by one sweep in row order: a row takes the lowest free slot, the slot returns to the pool after the
// row's last reader.  For intervals this greedy uses exactly as many slots as rows are live at once, which is the
// memory a query needs per plane: n_slots x pitch cells instead of rows x pitch.
#pragma once
#include <cstdint>
#include <vector>

#include "poa_graph.hpp"

namespace poa_amd {

constexpr uint32_t SWEEP_NO_SLOT = 0xFFFFFFFFu;

struct SweepRows {
    std::vector<uint32_t> slot;        // [n] by row; SWEEP_NO_SLOT: the row is never read back from memory
    std::vector<uint32_t> pred_slot;   // [pred_rows.size()] slot[pred_rows[k]] (saves the dependent lookup, like pred_dslot)
    std::vector<uint32_t> last_reader; // [n] largest row that reads the row (rows with a slot only; else the row itself)
    uint32_t n_slots = 0;              // rows live at once
    uint32_t n_slotted = 0;            // rows that have a slot (what a sweep stores per query and plane)
};

void build_sweep_rows(const FlatGraph& g, SweepRows& out);

}  // namespace poa_amd
