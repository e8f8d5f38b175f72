// The selection rule of the dense one-piece pass (poa_dense_plan.hpp).  Host code only.
#include "poa_dense_plan.hpp"

#include <algorithm>

namespace poa_amd {

// u16 cells whenever every value that can matter fits.  u16 arithmetic saturates at 0xFFFF = INF, so every stored value is
// min(true value, 0xFFFF); costs are non-negative, hence every cell on an optimal path — and every predecessor candidate the
// traceback can accept — has a value <= the final score, and the final score is at most
//     ub = [o + e*L] + [o + e*(nodes on the shortest start->end path)]      (insert the query, delete that path),
// each bracket counted only if its length is not zero: ub = o * n_open + e * n_extend.  ub <= 0xFFFE  =>  everything the result
// depends on is exact in u16.  (The cruder bound (rows + L + 2) * max(x, o+e) on ANY finite value is always >= ub.)  The
// two-piece model takes the first piece's costs: a gap never costs more than its first-piece price.
uint64_t score_bound(uint64_t open, uint64_t extend, uint64_t n_open, uint64_t n_extend) { return open * n_open + extend * n_extend; }
bool u16_cells_suffice(uint64_t open, uint64_t extend, uint64_t n_open, uint64_t n_extend) {
    return score_bound(open, extend, n_open, n_extend) <= 65534;
}
// The workspace a batch constructor settles on.  requested 0: what the batch needs as one chunk, or 85 % of what the device has
// free beyond the batch's other buffers (`fixed`) if that is less.  own_footprint: the batch holds its own footprint and never
// more, so a larger request is a cap only.  Whatever came out is raised to the largest item, which must fit beside `fixed`.
uint64_t choose_workspace(uint64_t requested, uint64_t free_bytes, uint64_t fixed, uint64_t bytes_total, uint64_t largest, bool own_footprint) {
    uint64_t ws = requested;
    if (ws == 0) {
        const uint64_t avail = free_bytes > fixed ? (uint64_t)((free_bytes - fixed) * 0.85) : 0;
        ws = std::min<uint64_t>(bytes_total, avail);
    }
    if (own_footprint) ws = std::min<uint64_t>(ws, bytes_total);
    if (ws < largest) {
        if (largest + fixed > free_bytes) return WORKSPACE_NO_FIT;
        ws = largest;
    }
    return ws;
}

TwoPieceWorkspace two_piece_workspace(uint64_t free_bytes, uint64_t bytes_total, uint64_t largest, uint64_t replay_slot_bytes, bool replay) {
    uint64_t budget = std::min<uint64_t>((uint64_t)(free_bytes * 0.6), 64ull << 30);
    uint32_t max_slots = ~0u;
    if (replay) {
        // (the replay is bound by the latency of its dependent loads: as many searches in flight as the memory holds)
        const uint64_t per_slot = std::max<uint64_t>(largest + replay_slot_bytes, 1);
        max_slots = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((uint64_t)(free_bytes * 0.85) / per_slot, 1), ~0u);
        budget = max_slots * largest;
    }
    return {std::max(std::min(budget, bytes_total), largest), max_slots};
}

// POA_PLANES=32 forces u32 cells (debug / A-B)
bool planes32(const TuneView& T) { const int* pv = T.ptr(POA_TUNE_PLANES); return pv && *pv == 32; }

// waves per workgroup of a multi-wave launch: all strips at once when they fit, else the strips spread evenly over the
// groups that run one after the other (16 + 4 strips would leave twelve waves idle in the second group)
uint32_t mw_waves(uint32_t strips) {
    const uint32_t groups = (strips + DENSE_MW_MAX_WAVES - 1) / DENSE_MW_MAX_WAVES;
    return (strips + groups - 1) / groups;
}

// the 1024-column multi-wave kernel when the chunk fills the chip with one wave per 1024 columns (else 512-column strips of
// the adjacent-pairs kernel give twice the waves)
bool pxmw_ok(const TuneView& T, uint32_t count, uint32_t max_pitch) {
    if (const int* v = T.ptr(POA_TUNE_PXMW)) return (*v) != 0;
    return (uint64_t)count * ((max_pitch + 1023) / 1024) >= 1024;
}

DenseRunPlan plan_dense_run(uint32_t gap_open, uint32_t gap_extend, uint64_t max_len, uint64_t min_path_nodes, uint32_t mode, bool want_full,
                            bool plan16_same, const TuneView& T) {
    DenseRunPlan R;
    // u16 planes under the bound of u16_cells_suffice, for one graph and the longest query that meets it; the flag variants of
    // the px kernel below take the bound itself
    R.ub = score_bound(gap_open, gap_extend, (max_len ? 1 : 0) + (min_path_nodes ? 1 : 0), max_len + min_path_nodes);
    R.narrow = R.ub <= 65534 && !planes32(T);
    // compact layout (u16 only): 4-bit codes instead of the I plane, D rows only where they are read back.
    // POA_CFG_FULL_PLANES (or POA_COMPACT=0) keeps all three planes, e.g. for poa_batch_fetch_planes.
    R.compact = R.narrow && !want_full;
    if (const int* cv = T.ptr(POA_TUNE_COMPACT)) { if ((*cv) == 0) R.compact = false; }
    R.packed = true;  // packed-u16 arithmetic kernel for the compact layout (POA_PACKED=0: scalar u32 arithmetic)
    if (const int* pv2 = T.ptr(POA_TUNE_PACKED)) R.packed = (*pv2) != 0;
    // Scores beyond u16 (a read against a much longer graph, Global): store every cell relative to the depth potential
    // e * (row_depth - column) (FlatGraph::row_depth).  All moves keep non-negative costs there, so the saturation argument
    // of u16_cells_suffice holds for the relative values, and the largest one on an optimal path is the end cell's:
    //     S* - e * (shortest path nodes - L)  <=  ub - e * min_path_nodes + e * L  =  2 * (o + e * L).
    // Only the pairs-across-quads kernels (compact layout) implement it; POA_RELATIVE=0 keeps u32 planes, =1 forces it
    // wherever the bound allows (A-B against the absolute encodings).
    const uint64_t rel_ub = 2 * ((uint64_t)gap_open + (uint64_t)gap_extend * max_len);
    R.relative = !R.narrow && rel_ub <= 65534 && !want_full && R.packed && !T.ptr(POA_TUNE_PLANES) && !T.ptr(POA_TUNE_COMPACT);
    if (const int* rv = T.ptr(POA_TUNE_RELATIVE)) {
        if ((*rv) == 0) R.relative = false;
        else R.relative = rel_ub <= 65534 && !want_full && R.packed;
    }
    if (R.relative) { R.narrow = true; R.compact = true; }
    // 2-byte elements let twice the queries share the workspace; the exact replay needs the u32 plan
    R.plan = (R.narrow && mode == POA_MODE_DENSE && !plan16_same) ? (R.compact ? 2 : 1) : 0;
    R.spec_depth = 12;  // traceback speculation depth (lanes per round) of the full-plane layouts; the compact one: see the chunk's record
    if (const int* sv = T.ptr(POA_TUNE_TB_DEPTH)) { const int v = (*sv); if (v >= 1 && v <= 64) R.spec_depth = (uint32_t)v; }
    R.tb_group = 0;   // POA_TB_GROUP override (lanes per walk); default: chosen per chunk
    if (const int* gv = T.ptr(POA_TUNE_TB_GROUP)) { const int v = (*gv); if (v == 8 || v == 16 || v == 32 || v == 64) R.tb_group = v; }
    R.fuse_tb = false;  // measured slower (16.0 vs 13.4 ms): tracing waves hold slots without HBM traffic. trace each query in the epilogue of its forward wave (POA_FUSE_TB=0: separate launch)
    if (const int* fv = T.ptr(POA_TUNE_FUSE_TB)) R.fuse_tb = (*fv) != 0;
    R.quads_override = 0;
    if (const int* ov = T.ptr(POA_TUNE_FWD_QUADS)) R.quads_override = (*ov);  // tuning override
    // the banded one-strip kernel (poa_forward_band.hpp) wherever poa_forward_px_kernel<3> would run in a dense run; its bound
    // needs e > 0.  POA_BAND=0 switches it off, POA_BAND_DELTA caps the band distance (tests)
    R.want_band = mode == POA_MODE_DENSE && gap_extend > 0;
    if (const int* bv = T.ptr(POA_TUNE_BAND)) R.want_band = R.want_band && (*bv) != 0;
    R.band_cap = 0xFFFFFFFFu;
    if (const int* dv = T.ptr(POA_TUNE_BAND_DELTA)) R.band_cap = (*dv) > 0 ? (uint32_t)(*dv) : 0u;
    // two queries of one length per wave (poa_forward_band2_kernel): POA_BAND_PAIR=0 never, 1 whatever the count, else the rule
    // The tune table is full, so the same entry carries the override of the narrow tier (poasta_amd.h: POA_TUNE_BAND_PAIR):
    // bits 0..1 the pairing (0 never, 1 always, 2 by the rule), bits 2..3 the narrow tier (0 by the rule, 1 never, 2 whenever paired)
    // ... and bits 4..5 the lean walk kernel (poasta_amd_tb.h: POA_TB_LEAN_SHIFT; 0 by the rule, 1 never, 2 wherever eligible)
    R.band_pair = -1;
    R.band_narrow = -1;
    R.tb_lean = -1;
    if (const int* pv = T.ptr(POA_TUNE_BAND_PAIR)) {
        const int p = (*pv) & POA_BAND_PAIR_MASK, n = ((*pv) >> POA_BAND_NARROW_SHIFT) & 3, l = ((*pv) >> POA_TB_LEAN_SHIFT) & 3;
        if (p != POA_BAND_PAIR_RULE) R.band_pair = p != 0 ? 1 : 0;
        if (n) R.band_narrow = n - 1;
        if (l == 1 || l == 2) R.tb_lean = l - 1;
    }
    // hybrid and exact runs keep one walk kernel, the generic one, for their dense pass and for the walk after the replay
    R.tb_lean_mode = mode == POA_MODE_DENSE;
    return R;
}

// The lean walk kernel wherever it is eligible: it is the same walk in fewer instructions, so the rule has no threshold.
bool tb_lean_eligible(const DenseRunPlan& R, uint32_t tb_lanes, uint32_t code_fmt, uint64_t plane_elems) {
    return R.tb_lean_mode && tb_lanes != 0 && R.compact && code_fmt == 4 && !R.relative && plane_elems < (1ull << 32);
}

// The narrow tier (poa_forward_band2_kernel<6>, a window of 384 columns) for a band class of query length L whose narrow plan has
// band distance d_n: 0 the rule takes it, 1 only the override does (the plan has a band), 2 never (no band: D_n < 4).
// BAND_NARROW_MIN_SHARE is a policy, not a measurement: a query the tier cannot certify costs a second banded pass, so the rule
// keeps the tier to classes where it certifies every score up to e * L / 4 - half a unit of gap extension per base under the
// default costs, far above what reads that align at all score (profiles/pr_band_narrow/README.md has the price of a miss).
constexpr uint32_t BAND_NARROW_MIN_SHARE = 4;   // D_n - 4 >= L / 4
uint32_t band_narrow_class(uint32_t d_n, uint32_t L) {
    if (d_n < 4) return 2;
    return (uint64_t)BAND_NARROW_MIN_SHARE * (d_n - 4) >= L ? 0 : 1;
}
// how many of a paired chunk's leading pairs run the narrow tier: n_rule of them belong to classes the rule takes, n_any to
// classes with a narrow band at all.  The rule asks that the chunk pairs by band_pair_rule itself (pair_by_rule), not only
// under a forced POA_BAND_PAIR=1: the tier exists in the paired form alone and pays where pairing does.
uint32_t band_narrow_pairs(const DenseRunPlan& R, bool pair_by_rule, uint32_t n_rule, uint32_t n_any) {
    if (R.band_narrow == 0) return 0;
    if (R.band_narrow > 0) return n_any;
    return pair_by_rule ? n_rule : 0;
}

DenseChunkPlan plan_dense_chunk(const DenseRunPlan& R, uint32_t count, uint32_t max_pitch, const TuneView& T, uint64_t plane_elems) {
    // the launch record of this chunk (poa_batch_last_launch): kernel family, quads, fused walk, multi-wave, waves per workgroup
    uint32_t lk = POA_KERNEL_NONE, lq = 0, lwaves = 4, code_fmt = 0;
    bool lfuse = false, lmw = false;
    int mf = -1;
    const int quads_override = R.quads_override;
    // strip width: as narrow as the widest plane row of the chunk allows, at most 1024 columns
    if (R.narrow) {
        uint32_t quads = max_pitch <= 512 ? 1 : 2;  // 512 columns per quad (8 x u16 per lane)
        if (quads_override == 1 || quads_override == 2) quads = (uint32_t)quads_override;
        if (R.relative) quads = 2;  // the relative encoding lives in the pairs-across-quads kernels only
        lk = R.compact && R.packed ? POA_KERNEL_PACKED : POA_KERNEL_FORWARD; lq = quads;
        if (R.compact && R.packed) {
            // queries longer than one strip: one workgroup per query, its strips pipelined over the waves (MW)
            bool mw = max_pitch > 512 * quads;
            if (const int* mv = T.ptr(POA_TUNE_MW)) mw = mw && ((*mv) != 0 || R.relative);
            bool px = max_pitch <= 1024 && quads == 2 && (!R.fuse_tb || R.relative);  // one strip of up to 1024 columns: the pairs-across-quads kernel
            if (const int* xv = T.ptr(POA_TUNE_PX)) px = (px && (*xv) != 0) || (px && R.relative);
            if (px) {
                // scores below 0x3FFF (same bound as for u16, one power lower): two flags ride in the stored M value
                // (below 0x0FFF: all four; POA_MF = 0 / 1 / 2 caps the variant for A-B runs).  Wherever flags fit beside the
                // score the engine takes variant 3: the two Match-state flags in the score and no gap-state flags at all (the
                // traceback derives them, poa_tb_derive.hpp) - the forward pass is instruction-issue bound and they are a
                // fifth of its instructions
                mf = R.relative ? 0 : (R.ub <= 4094 ? 2 : (R.ub <= 16382 ? 1 : 0));
                if (const int* fv2 = T.ptr(POA_TUNE_MF)) mf = (*fv2) == 3 ? (mf >= 1 ? 3 : 0) : std::min(mf, std::max(0, (*fv2)));
                else if (mf >= 1) mf = 3;
                code_fmt = mf == 3 ? 4u : (mf == 2 ? 3u : (mf == 1 ? 2u : 1u));
                // the banded pass, then the full pass over the queries it could not certify (launch_band in poa_engine.hip)
                lk = (mf == 3 && R.want_band && max_pitch > 512) ? POA_KERNEL_BAND : POA_KERNEL_PX;
            } else if (mw && (R.relative || pxmw_ok(T, count, max_pitch))) {
                // pairs-across-quads mapping, 1024-column strips pipelined over the waves of a workgroup
                code_fmt = 1;
                lk = POA_KERNEL_PXMW; lq = 2; lmw = true; lwaves = mw_waves((max_pitch + 1023) / 1024);
            } else if (mw) {
                // narrow strips (more waves) until the chunk alone fills the chip
                if (!quads_override) quads = ((uint64_t)count * ((max_pitch + 1023) / 1024) >= 8192) ? 2 : 1;
                lq = quads; lmw = true; lwaves = mw_waves((max_pitch + 512 * quads - 1) / (512 * quads));
            } else lfuse = R.fuse_tb;
        } else if (!R.compact) lfuse = R.fuse_tb;
    } else {
        uint32_t quads = max_pitch <= 256 ? 1 : (max_pitch <= 512 ? 2 : 4);  // 256 columns per quad (4 x u32 per lane)
        if (quads_override == 1 || quads_override == 2 || quads_override == 4) quads = (uint32_t)quads_override;
        bool mw = max_pitch > 1024;  // longer than the widest strip: pipeline the strips over the waves of a workgroup
        if (const int* mv = T.ptr(POA_TUNE_MW)) mw = mw && (*mv) != 0;
        lk = POA_KERNEL_FORWARD; lq = quads;
        if (mw) {
            // 512-column strips (up to 16 waves per query) or 1024-column ones (up to 10): a query whose strips do not all
            // fit one workgroup runs as several groups one after the other, and few long queries are latency bound per
            // row (a 1024-column row costs ~1.4x a 512-column one), so take the variant with the least groups x row cost;
            // the waves per workgroup are balanced over the groups
            const uint32_t s2 = (max_pitch + 511) / 512, s4 = (max_pitch + 1023) / 1024;
            const uint32_t g2 = (s2 + DENSE_MW_MAX_WAVES - 1) / DENSE_MW_MAX_WAVES, g4 = (s4 + 9) / 10;
            bool wide = 14 * g4 < 10 * g2 || (uint64_t)count * s4 >= 8192;
            if (quads_override == 4) wide = true;
            if (quads_override == 2) wide = false;
            lq = wide ? 4 : 2; lmw = true; lwaves = wide ? (s4 + g4 - 1) / g4 : (s2 + g2 - 1) / g2;
        } else lfuse = R.fuse_tb;
    }
    uint32_t ltb = 0, ldepth = R.spec_depth;   // lanes per walk of the separate traceback launch (0: none), speculation depth
    if (!(R.fuse_tb && !R.relative && max_pitch <= 1024 && (!R.compact || R.packed))) {
        // Lanes per walk: as many as keep the launch within ~6 000 waves (what the chip holds at this kernel's occupancy
        // with room to spare), and a speculation depth to match.  Measured on config 2 after the insertion-run speculation
        // (ms per batch; 64 lanes x depth 32 / 32 x 32 / 16 x 16): 1 024 walks 0.44 / 0.57 / 0.74, 4 096 walks 0.68 / 0.77 /
        // 0.84, 10 000 walks 1.22 / 0.97 / 1.05, 20 000 walks 2.22 / 1.79 / 1.35.
        const int tbg = R.tb_group ? R.tb_group : (count <= 6144 ? 64 : (count <= 12288 ? 32 : 16));
        ltb = R.compact ? (uint32_t)tbg : 64u;
        if (R.compact && !T.ptr(POA_TUNE_TB_DEPTH)) ldepth = tbg == 16 ? 16u : 32u;
    }
    const bool lean = R.tb_lean != 0 && tb_lean_eligible(R, ltb, code_fmt, plane_elems);   // POA_TB_LEAN=0: never; 1 and the rule: wherever eligible
    return {{lk, lq, (lfuse ? POA_LAUNCH_FUSE : 0u) | (lmw ? POA_LAUNCH_MW : 0u), lwaves, code_fmt, ltb, ldepth, count}, mf, lk == POA_KERNEL_BAND, ltb != 0, lean};
}

}  // namespace poa_amd
