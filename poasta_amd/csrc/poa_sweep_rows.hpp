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
    std::vector<uint8_t> cut;          // [n] 1: a cut row (see build_sweep_checks)
};

void build_sweep_rows(const FlatGraph& g, SweepRows& out);

// Check rows of a capped sweep (poa_scoreset_run_capped).  Row r is a CUT row if no edge (u, v) has row(u) < r < row(v): every
// start-to-end path of the graph then passes through row r, and once row r has run no row before it is still live — neither in
// the slot table nor as the chain row handed over in registers, which is row r itself.  Costs are non-negative, so the score
// of a path never decreases along it: the smallest M value of a cut row is a lower bound on M[end row][len].  Row 0 and the
// end row are cut rows.  The CHECK rows are the cut rows without the end row (the result is written there anyway), thinned
// greedily in row order so that two consecutive check rows lie at least `stride` rows apart (0: SWEEP_CHECK_STRIDE).
constexpr uint32_t SWEEP_CHECK_STRIDE = 8;
void build_sweep_checks(const uint8_t* cut, uint32_t n_rows, uint32_t stride, std::vector<uint32_t>& check_rows);

// Segment plan of the checkpointed mode (POA_MODE_CHECKPOINT, poa_checkpoint.hpp).  Host code, no device needed.
//
// The row order is cut into segments [boundary[s], boundary[s + 1]) of segment_rows rows (the last one may be shorter).  The
// SNAPSHOT of a boundary b > 0 is what rows >= b may still read of rows < b: every row p < b that has a sweep slot and
// last_reader[p] >= b, plus row b - 1 if row b is a ROW_CHAIN row (the sweep hands it its predecessor in registers, so the
// slot table does not know that reader).  Only M and D are saved: I never leaves its row.  Snapshot rows are numbered through
// all boundaries, in boundary order; a query holds n_snap_rows rows of M and of D for them.
//
// Pass 1 (the sweep) stores a row into every snapshot it belongs to as it computes it: snap_off / snap_dst list those
// snapshot rows per graph row.  Pass 2 recomputes one segment at a time into a window of max_segment rows of M, I and D and
// reads a predecessor either from the window or from the snapshot of the segment's first boundary: pred_src says which, per
// predecessor edge (the walk goes through the same table, so it never needs a row -> location lookup).
constexpr uint32_t CKPT_SNAP = 0x80000000u;   // pred_src: the low bits are a snapshot row; else a row of the window

struct CheckpointPlan {
    uint32_t segment_rows = 0;         // rows per segment (the last may hold fewer)
    uint32_t max_segment = 0;          // rows of the longest segment: the window
    uint32_t n_snap_rows = 0;          // snapshot rows, all boundaries together
    uint32_t rows_per_query = 0;       // 2 * n_slots + 2 * n_snap_rows + 3 * max_segment plane rows of `pitch` cells (two-piece: 3, 3 and 5)
    std::vector<uint32_t> boundary;    // [n_segments + 1]: 0 ... rows
    std::vector<uint32_t> snap_off;    // [n + 1] CSR by row into snap_dst
    std::vector<uint32_t> snap_dst;    // snapshot rows a row is stored to in pass 1
    std::vector<uint32_t> pred_src;    // [pred_rows.size()] pass 2: window row (pred - segment start), or CKPT_SNAP | snapshot row
    uint32_t n_segments() const { return boundary.empty() ? 0u : (uint32_t)boundary.size() - 1u; }
};

// Planes a query holds per kept row (slot or snapshot) and per window row.  One-piece model: M and D are kept, the window
// holds M, I and D.  Two-piece model (POA_MODE_CHECKPOINT2, poa_checkpoint2.hpp): M, D1 and D2 are kept (D2 leaves its row as
// D1 does, I1 and I2 never do), the window holds all five.  Boundaries and snapshot membership are the same for both; the
// default segment length differs because the window weighs more.
struct CheckpointWeights { uint32_t kept, window; };
inline CheckpointWeights checkpoint_weights(bool two_piece) { return two_piece ? CheckpointWeights{3, 5} : CheckpointWeights{2, 3}; }

// plane rows a query holds with segments of k rows (what the default plan minimises)
uint64_t checkpoint_rows_per_query(const FlatGraph& g, const SweepRows& sw, uint32_t k, bool two_piece = false);
// segment_rows 0: the engine's choice — about sqrt(window * rows / (kept * (n_slots + 1))) segments, the candidate around it
// that holds the fewest rows, and never more than one segment of all rows would
void build_checkpoint_plan(const FlatGraph& g, const SweepRows& sw, uint32_t segment_rows, CheckpointPlan& out, bool two_piece = false);

}  // namespace poa_amd
