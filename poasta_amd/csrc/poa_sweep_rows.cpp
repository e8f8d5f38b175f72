// Row liveness table and slot assignment of the score-only sweep: see poa_sweep_rows.hpp.
#include "poa_sweep_rows.hpp"

#include <algorithm>
#include <functional>
#include <queue>

namespace poa_amd {

void build_sweep_rows(const FlatGraph& g, SweepRows& out) {
    const uint32_t n = (uint32_t)g.rows.size();
    out.slot.assign(n, SWEEP_NO_SLOT);
    out.last_reader.resize(n);
    out.pred_slot.assign(g.pred_rows.size(), SWEEP_NO_SLOT);
    out.n_slots = 0;
    out.n_slotted = 0;
    std::vector<uint8_t> kept(n, 0);
    for (uint32_t r = 0; r < n; ++r) out.last_reader[r] = r;
    for (uint32_t r = 0; r < n; ++r) {
        const RowMeta& m = g.rows[r];
        if (m.flags & ROW_CHAIN) continue;   // reads row r - 1 from registers
        for (uint32_t pe = 0; pe < m.pred_count; ++pe) {
            const uint32_t p = g.pred_rows[m.pred_begin + pe];
            kept[p] = 1;
            out.last_reader[p] = std::max(out.last_reader[p], r);
        }
    }
    // greedy interval colouring in row order: lowest free slot first, a slot is free again from the row after its last reader
    std::priority_queue<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> free_slots;
    typedef std::pair<uint32_t, uint32_t> Busy;   // (last reader, slot)
    std::priority_queue<Busy, std::vector<Busy>, std::greater<Busy>> busy;
    for (uint32_t r = 0; r < n; ++r) {
        while (!busy.empty() && busy.top().first < r) {
            free_slots.push(busy.top().second);
            busy.pop();
        }
        if (!kept[r]) continue;
        uint32_t s;
        if (free_slots.empty()) s = out.n_slots++;
        else { s = free_slots.top(); free_slots.pop(); }
        out.slot[r] = s;
        out.n_slotted++;
        busy.push(Busy(out.last_reader[r], s));
    }
    for (size_t k = 0; k < g.pred_rows.size(); ++k) out.pred_slot[k] = out.slot[g.pred_rows[k]];
    // cut rows: an edge (p, r) covers the rows strictly between its ends (every edge counts, the chain rows' too)
    std::vector<int32_t> cover((size_t)n + 1, 0);
    for (uint32_t r = 0; r < n; ++r) {
        const RowMeta& m = g.rows[r];
        for (uint32_t pe = 0; pe < m.pred_count; ++pe) {
            const uint32_t p = g.pred_rows[m.pred_begin + pe];
            if (p + 1 < r) { cover[p + 1]++; cover[r]--; }
        }
    }
    out.cut.assign(n, 0);
    int32_t depth = 0;
    for (uint32_t r = 0; r < n; ++r) {
        depth += cover[r];
        out.cut[r] = depth == 0;
    }
}

void build_sweep_checks(const uint8_t* cut, uint32_t n_rows, uint32_t stride, std::vector<uint32_t>& check_rows) {
    check_rows.clear();
    if (stride == 0) stride = SWEEP_CHECK_STRIDE;
    for (uint32_t r = 0; r + 1 < n_rows; ++r)
        if (cut[r] && (check_rows.empty() || r - check_rows.back() >= stride)) check_rows.push_back(r);
}

// rows p < b of boundary b's snapshot that the slot table knows: slotted, read by some row >= b
static inline bool snap_by_slot(const SweepRows& sw, uint32_t p, uint32_t b) {
    return sw.slot[p] != SWEEP_NO_SLOT && sw.last_reader[p] >= b;
}

uint64_t checkpoint_rows_per_query(const FlatGraph& g, const SweepRows& sw, uint32_t k, bool two_piece) {
    const uint32_t n = (uint32_t)g.rows.size();
    if (n == 0) return 0;
    if (k == 0 || k > n) k = n;
    uint64_t snap = 0;
    // a slotted row p lies in the snapshots of the boundaries b = i * k with p < b <= last_reader[p]
    for (uint32_t p = 0; p < n; ++p)
        if (sw.slot[p] != SWEEP_NO_SLOT) snap += sw.last_reader[p] / k - p / k;
    for (uint32_t b = k; b < n; b += k)
        if ((g.rows[b].flags & ROW_CHAIN) && !snap_by_slot(sw, b - 1, b)) snap++;
    const CheckpointWeights w = checkpoint_weights(two_piece);
    return (uint64_t)w.kept * sw.n_slots + (uint64_t)w.kept * snap + (uint64_t)w.window * k;
}

void build_checkpoint_plan(const FlatGraph& g, const SweepRows& sw, uint32_t segment_rows, CheckpointPlan& out, bool two_piece) {
    const CheckpointWeights wt = checkpoint_weights(two_piece);
    const uint32_t n = (uint32_t)g.rows.size();
    out = CheckpointPlan();
    out.snap_off.assign((size_t)n + 1, 0);
    out.pred_src.assign(g.pred_rows.size(), 0);
    out.boundary.assign(1, 0);
    if (n == 0) return;
    uint32_t k = segment_rows;
    if (k == 0) {
        // the sum kept * (n_slots + 1) * S + window * rows / S (2 and 3 planes in the one-piece model, 3 and 5 in the two-piece
        // one) is least at S = sqrt(window * rows / (kept * (n_slots + 1))); the real snapshots are smaller than n_slots + 1
        // rows, so the neighbourhood of that S is searched with the real count
        uint32_t s0 = 1;
        while ((uint64_t)(s0 + 1) * (s0 + 1) * wt.kept * (sw.n_slots + 1) <= (uint64_t)wt.window * n) ++s0;
        k = n;
        uint64_t best = checkpoint_rows_per_query(g, sw, n, two_piece);   // one segment: full planes, the most the mode may ever hold
        for (uint32_t s : {s0 / 2, (2 * s0) / 3, s0, s0 + s0 / 2, 2 * s0, 3 * s0}) {
            if (s < 2 || s > n) continue;
            const uint32_t kk = (n + s - 1) / s;
            const uint64_t c = checkpoint_rows_per_query(g, sw, kk, two_piece);
            if (c < best) { best = c; k = kk; }
        }
    }
    if (k > n) k = n;
    out.segment_rows = k;
    for (uint32_t b = k; b < n; b += k) out.boundary.push_back(b);
    out.boundary.push_back(n);
    out.max_segment = k;
    // snapshots, boundary by boundary: position of every saved row, and per row the list of its copies
    std::vector<std::vector<uint32_t>> dst(n);
    std::vector<uint32_t> live;   // slotted rows < b that some row >= b may read
    std::vector<uint32_t> pos(n, SWEEP_NO_SLOT);   // row -> snapshot row of the boundary being built
    uint32_t next = 0, p_scan = 0;
    for (size_t s = 1; s + 1 < out.boundary.size(); ++s) {
        const uint32_t b = out.boundary[s], b_end = out.boundary[s + 1];
        for (; p_scan < b; ++p_scan)
            if (sw.slot[p_scan] != SWEEP_NO_SLOT) live.push_back(p_scan);
        size_t w = 0;
        for (size_t i = 0; i < live.size(); ++i)
            if (sw.last_reader[live[i]] >= b) live[w++] = live[i];
        live.resize(w);
        std::vector<uint32_t> members(live);
        if ((g.rows[b].flags & ROW_CHAIN) && !snap_by_slot(sw, b - 1, b)) members.push_back(b - 1);
        for (uint32_t p : members) { pos[p] = next; dst[p].push_back(next); next++; }
        for (uint32_t r = b; r < b_end; ++r) {
            const RowMeta& m = g.rows[r];
            for (uint32_t pe = 0; pe < m.pred_count; ++pe) {
                const uint32_t p = g.pred_rows[m.pred_begin + pe];
                out.pred_src[m.pred_begin + pe] = p >= b ? p - b : (CKPT_SNAP | pos[p]);
            }
        }
        for (uint32_t p : members) pos[p] = SWEEP_NO_SLOT;
    }
    // first segment: every predecessor is in the window
    for (uint32_t r = 0; r < out.boundary[1]; ++r) {
        const RowMeta& m = g.rows[r];
        for (uint32_t pe = 0; pe < m.pred_count; ++pe) out.pred_src[m.pred_begin + pe] = g.pred_rows[m.pred_begin + pe];
    }
    out.n_snap_rows = next;
    for (uint32_t r = 0; r < n; ++r) out.snap_off[r + 1] = out.snap_off[r] + (uint32_t)dst[r].size();
    out.snap_dst.reserve(next);
    for (uint32_t r = 0; r < n; ++r) out.snap_dst.insert(out.snap_dst.end(), dst[r].begin(), dst[r].end());
    out.rows_per_query = (uint32_t)((uint64_t)wt.kept * sw.n_slots + (uint64_t)wt.kept * next + (uint64_t)wt.window * k);
}

}  // namespace poa_amd
