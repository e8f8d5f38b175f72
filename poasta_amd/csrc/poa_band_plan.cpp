// Band plan of the one-strip dense forward pass: see poa_band_plan.hpp.
#include "poa_band_plan.hpp"

#include <algorithm>

namespace poa_amd {

namespace {
inline int64_t floor_div2(int64_t v) { return v >= 0 ? v / 2 : -((-v + 1) / 2); }
inline int64_t ceil_div2(int64_t v) { return -floor_div2(-v); }
}  // namespace

void build_band_tables(const FlatGraph& g, BandTables& out) {
    const uint32_t n = g.n;
    out.a_min.assign(n, BAND_NONE); out.a_max.assign(n, BAND_NONE);
    out.c_min.assign(n, BAND_NONE); out.c_max.assign(n, BAND_NONE);
    auto real = [&](uint32_t r) { return (g.rows[r].flags & (ROW_START | ROW_END)) ? 0u : 1u; };
    // rows are in topological order: every predecessor of a row lies before it
    for (uint32_t r = 0; r < n; ++r) {
        const RowMeta& m = g.rows[r];
        if (m.flags & ROW_START) { out.a_min[r] = 0; out.a_max[r] = 0; continue; }
        uint32_t lo = BAND_NONE, hi = BAND_NONE;
        for (uint32_t k = 0; k < m.pred_count; ++k) {
            const uint32_t p = g.pred_rows[m.pred_begin + k];
            if (out.a_min[p] == BAND_NONE) continue;
            lo = lo == BAND_NONE ? out.a_min[p] : std::min(lo, out.a_min[p]);
            hi = hi == BAND_NONE ? out.a_max[p] : std::max(hi, out.a_max[p]);
        }
        if (lo != BAND_NONE) { out.a_min[r] = lo + real(r); out.a_max[r] = hi + real(r); }
    }
    for (uint32_t r = n; r-- > 0;) {
        const RowMeta& m = g.rows[r];
        if (m.flags & ROW_END) { out.c_min[r] = 0; out.c_max[r] = 0; }
        if (out.c_min[r] == BAND_NONE) continue;   // no way to the end: nothing to hand to the predecessors
        const uint32_t lo = out.c_min[r] + real(r), hi = out.c_max[r] + real(r);
        for (uint32_t k = 0; k < m.pred_count; ++k) {
            const uint32_t p = g.pred_rows[m.pred_begin + k];
            out.c_min[p] = out.c_min[p] == BAND_NONE ? lo : std::min(out.c_min[p], lo);
            out.c_max[p] = out.c_max[p] == BAND_NONE ? hi : std::max(out.c_max[p], hi);
        }
    }
    for (uint32_t r = 0; r < n; ++r)
        if (out.a_min[r] == BAND_NONE || out.c_min[r] == BAND_NONE) out.a_min[r] = out.a_max[r] = out.c_min[r] = out.c_max[r] = BAND_NONE;
}

bool band_row_interval(const BandTables& t, uint32_t r, uint32_t L, uint32_t D, uint32_t& lo, uint32_t& hi) {
    if (t.a_min[r] == BAND_NONE) return false;
    // ds + de = dist(j, [p1, p2]) + dist(j, [q1, q2]): convex, piecewise linear with integer breakpoints
    const int64_t p1 = t.a_min[r], p2 = t.a_max[r], q1 = (int64_t)L - t.c_max[r], q2 = (int64_t)L - t.c_min[r];
    const int64_t l1 = std::min(p1, q1), l2 = std::max(p1, q1), u1 = std::min(p2, q2), u2 = std::max(p2, q2);
    const int64_t d = D;
    if (l2 - u1 > d) return false;   // the two intervals lie further apart than D
    // left of both minima regions the sum is (l2 - j) + max(0, l1 - j), right of them (j - u1) + max(0, j - u2)
    int64_t a = l2 - d >= l1 ? l2 - d : ceil_div2(l1 + l2 - d);
    int64_t b = u1 + d <= u2 ? u1 + d : floor_div2(u1 + u2 + d);
    a = std::max<int64_t>(a, 0); b = std::min<int64_t>(b, L);
    if (a > b) return false;
    lo = (uint32_t)a; hi = (uint32_t)b;
    return true;
}

uint32_t plan_band(const FlatGraph& g, const BandTables& t, uint32_t L, uint32_t seg_rows, uint32_t window, uint32_t* bases) {
    const uint32_t n_seg = band_segments(g.n, seg_rows);
    auto fit = [&](uint32_t D, uint32_t* out) {
        bool ok = true;
        uint32_t prev = 0;
        for (uint32_t s = 0; s < n_seg; ++s) {
            uint32_t slo = BAND_NONE, shi = 0;
            const uint32_t r1 = std::min(g.n, (s + 1) * seg_rows);
            for (uint32_t r = s * seg_rows; r < r1; ++r) {
                uint32_t lo, hi;
                if (!band_row_interval(t, r, L, D, lo, hi)) continue;
                slo = std::min(slo, lo); shi = std::max(shi, hi);
            }
            uint32_t base = prev;
            if (slo != BAND_NONE) {
                base = slo & ~(BAND_BASE_ALIGN - 1);
                if (shi - base >= window) ok = false;
            }
            if (out) out[s] = base;
            prev = base;
        }
        return ok;
    };
    if (!fit(0, nullptr)) { fit(0, bases); return 0; }
    uint32_t lo = 0, hi = BAND_D_MAX;   // fit(lo) holds; the fit is monotone in D (the bands only grow)
    if (fit(hi, nullptr)) lo = hi;
    while (lo + 1 < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (fit(mid, nullptr)) lo = mid; else hi = mid;
    }
    fit(lo, bases);
    return lo;
}

}  // namespace poa_amd
