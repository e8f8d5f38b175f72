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
}

}  // namespace poa_amd
