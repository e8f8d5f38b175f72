// Banded variant of poa_forward_px_kernel<3> (gfx950): the same recurrences, register mapping and store format (M plane with
// the two Match-state flags in bits 14 and 15, kept D rows, TbParams::code_fmt 4), but over a WINDOW of 512 columns per row
// instead of the whole strip of 1024 — four packed registers per row array instead of eight.  The window is placed at
// base[segment] (poa_band_plan.hpp: one base per 64 rows, a multiple of 8) and every cell outside the window of its row's
// segment reads as INF.  DESIGN.md §6, "Banded one-strip kernel": such a pass computes values >= the true ones, and for a query whose computed end score
// is <= T = e * (D - 4), D the plan's band distance, the score, every cell the traceback's decisions read and therefore the
// alignment and the flags are those of the full pass.  The wave checks that after its last row; a query that fails the test
// (or whose class has no band) is appended to a device list, which the FULL instantiation of this same kernel then works off:
// eight registers per row array, one window of 1024 columns at base 0 - the arithmetic of poa_forward_px_kernel<3> - rewriting
// the whole planes of those queries.  (poa_forward_px_kernel itself stays as it is: it takes its queries by position.)
//
// Lane l owns window columns 4l..4l+3 (low halves) and 256+4l..256+4l+3 (high halves); register k holds
//      lo half = column base + 4l + k,   hi half = column base + 256 + 4l + k.
// Only window cells are written: nothing else of the planes is touched, and what lies outside the windows is stale memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_band_plan.hpp"
#include "poa_forward_px.hpp"

namespace poa_amd {

struct BandParams {
    const uint32_t* cls;       // [total] band class of every query (one class per distinct query length)
    const uint32_t* cls_d;     // [n_classes] band distance D of the class (< 4: no band)
    const uint32_t* cls_base;  // [n_classes * n_seg] window base per segment of BAND_ROWS rows
    uint32_t n_seg;
    uint32_t d_cap;            // D is capped by it (POA_TUNE_BAND_DELTA; 0xFFFFFFFF: no cap)
    uint32_t* list;            // queries the full kernel has to redo, appended at list[first_query + k]
    uint32_t* count;           // their number (cleared per run)
    const uint32_t* order;     // paired runs: the launch's queries - the chunk's pairs (A, B, A, B, ...) or its singles; else unused
    // the 512 pass over the narrow tier's misses (LIST): order is that tier's list and *n_order its length, known on the device
    // alone (the grid is sized for every query of the tier); a query this pass cannot certify either is counted in *count_nf
    const uint32_t* n_order;   // nullptr: order holds P.n_queries entries
    uint32_t* count_nf;
};

constexpr uint32_t BAND_ROWS = BAND_SEG_ROWS;
// Pairing (poa_forward_band2_kernel) halves the waves of a launch: it pays only where the chunk's pairs alone still fill the
// chip.  The default pairs a chunk from this many queries in pairs on (measured: profiles/pr_band_pairs/README.md).
constexpr uint32_t BAND_PAIR_MIN_QUERIES = 4096;
constexpr bool band_pair_rule(uint32_t paired_queries) { return paired_queries >= BAND_PAIR_MIN_QUERIES; }
static_assert(BAND_WINDOW == 512 && BAND_BASE_ALIGN % 4 == 0 && BAND_SEG_ROWS % 2 == 0,
              "the banded kernel: 2 x 64 lanes x 4 columns per window, a lane's four columns move together, segments start at even rows");

// LIST (banded pass only): wave w of the launch takes query B.order[w], P.n_queries counting the launch's queries - the
// singles of a paired run; the positional instantiation is untouched by it
template <bool FULL, bool LIST = false>
__global__ __launch_bounds__(256) void poa_forward_band_kernel(FwdParams P, BandParams B) {
    static_assert(!(FULL && LIST), "the full pass takes its queries from the fallback list");
    constexpr int K = FULL ? 8 : 4;      // columns per lane and half == packed registers per row array
    constexpr int KH = K / 4;            // 8-byte pieces (four u16 columns) per lane and half
    constexpr uint32_t QW = 64 * K;      // 256 (FULL: 512) columns per half
    constexpr uint32_t WIN = 2 * QW;     // 512 (FULL: 1024) columns per window
    constexpr uint32_t I16 = 0xFFFFu, INF2 = 0xFFFFFFFFu;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wq = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave-uniform
    if (wq >= P.n_queries) return;
    if (FULL && wq >= *B.count) return;   // the list of the banded pass: usually empty (the grid is sized for the chunk)
    if (LIST && B.n_order && wq >= *B.n_order) return;   // the list of the narrow tier, likewise
    const uint32_t qi = FULL ? B.list[P.first_query + wq] : (LIST ? B.order[wq] : P.first_query + wq);
    const uint32_t cl = (uint32_t)__builtin_amdgcn_readfirstlane((int)B.cls[qi]);   // uniform: the bases come in over the scalar cache
    const uint32_t band_d = ((const CU32*)B.cls_d)[cl] < B.d_cap ? ((const CU32*)B.cls_d)[cl] : B.d_cap;
    if (!FULL && band_d < 4) {   // no band for this length (T = e * (D - 4) needs D >= 4): the full pass computes the query
        if (lane == 0) {
            B.list[P.first_query + atomicAdd(B.count, 1u)] = qi;
            if (LIST && B.n_order) atomicAdd(B.count_nf, 1u);
        }
        return;
    }
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(P.qoff[qi + 1] - qbeg));
    const uint8_t* __restrict__ q = P.qseq + qbeg;
    const uint32_t pitch = P.pitch[qi];  // <= 1024 (launcher: one strip)
    const uint64_t RP = (uint64_t)P.n_rows * pitch;
    uint16_t* __restrict__ Mp = reinterpret_cast<uint16_t*>(P.planes) + P.plane_off[qi];
    uint16_t* __restrict__ Dp = Mp + RP + RP / 4;  // the kept D rows, row r at slot d_slot[r] (compact_plane_elems)
    const uint32_t e = P.cost_e, x = P.cost_x;     // absolute encoding only: one e, one o + e
    const uint32_t e2 = e | (e << 16), oe2 = P.cost_oe | (P.cost_oe << 16), x2 = x | (x << 16);
    auto pack16 = [](uint32_t v) { v = v < I16 ? v : I16; return v | (v << 16); };
    const uint32_t step = K * e;
    const uint32_t step2 = pack16(step);
    const uint32_t w15_2 = pack16(((lane & 15u) + 1u) * step);
    const uint32_t w31_2 = pack16(lane >= 32u ? (lane - 31u) * step : 0xFFFFu);  // see poa_forward_px_kernel
    const uint32_t lane_off2 = pack16(K * lane * e);

    const CRowWords* crows = (const CRowWords*)P.rows;
    const CU32* cpred = (const CU32*)P.pred_rows;
    const CU32* cslot = (const CU32*)P.d_slot;
    const CU32* cpslot = (const CU32*)P.pred_dslot;
    const CU32* cbase = (const CU32*)(B.cls_base + (uint64_t)cl * B.n_seg);

    // Per wave in LDS: the five symbol-mask tables of poa_forward_px_kernel (KH uint4 per lane and table: 5 KB, FULL: 10 KB) and
    // the hand-over buffer of a window move (the previous row's M and D, 512 u16 each: 2 KB; FULL: no moves)
    __shared__ uint4 sym_tab[4 * 5 * KH * 64];
    __shared__ uint2 move_buf[FULL ? 1 : 4 * 2 * 128];
    uint4* my_tab = sym_tab + (threadIdx.x >> 6) * (5 * KH * 64) + lane;
    uint2* my_move = move_buf + (FULL ? 0u : (threadIdx.x >> 6) * (2 * 128));

    uint32_t base = 0, c_lo = 0, c_hi = 0;
    bool act_lo = false, act_hi = false;
    uint32_t qP[K], qlE = 0;
    // place the window at column nb: my columns, my query symbols and the symbol masks
    auto place = [&](const uint32_t nb) {
        base = nb;
        c_lo = nb + K * lane; c_hi = nb + QW + K * lane;
        act_lo = c_lo < pitch; act_hi = c_hi < pitch;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t a = (c_lo + k < L) ? (uint32_t)q[c_lo + k] : 0u, b = (c_hi + k < L) ? (uint32_t)q[c_hi + k] : 0u;
            qP[k] = a | (b << 16);
        }
        qlE = ((c_lo > 0 && c_lo - 1 < L) ? (uint32_t)q[c_lo - 1] : 0u) | (((c_hi - 1 < L) ? (uint32_t)q[c_hi - 1] : 0u) << 16);
        const uint32_t letters[4] = {'A', 'C', 'G', 'T'};
#pragma unroll
        for (int si = 0; si < 4; ++si) {
            const uint32_t s2 = letters[si] | (letters[si] << 16);
            uint32_t m[K];
#pragma unroll
            for (int k = 0; k < K; ++k) m[k] = pku(pkv(0u) - pkv(pk_is_zero(qP[k] ^ s2)));
#pragma unroll
            for (int h = 0; h < KH; ++h) my_tab[(si * KH + h) * 64] = make_uint4(m[4 * h], m[4 * h + 1], m[4 * h + 2], m[4 * h + 3]);
        }
#pragma unroll
        for (int h = 0; h < KH; ++h) my_tab[(4 * KH + h) * 64] = make_uint4(0u, 0u, 0u, 0u);
        // each lane reads back only what it wrote itself: no barrier needed
    };

    // predecessor minima of the last multi-predecessor row: sibling rows (ROW_SAME_PREDS) reuse them
    uint32_t PMc[K], PDc[K], PMlc = INF2;
#pragma unroll
    for (int k = 0; k < K; ++k) { PMc[k] = INF2; PDc[k] = INF2; }

    // lane l <- v of lane l-1; lane 0: lo half <- INF (left of the window, even where the predecessor's own window reaches further
    // left: that edge is dropped, which the margin of T covers - DESIGN.md), hi half <- lane 63's lo half
    auto shr_lane = [&](uint32_t v) {
        const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
        return pk_wave_shr1(v, I16 | (last << 16));
    };

    uint32_t end_score = I16;   // M[end row][L] as computed (INF: outside the window)
    poa_u32x4 mw_ahead = crows[0];
    auto do_row = [&](const uint32_t r, const uint32_t (&Mprev)[K], const uint32_t (&Dprev)[K], uint32_t (&Mout)[K], uint32_t (&Dout)[K]) {
        const poa_u32x4 mw = mw_ahead;  // {node, pred_begin, pred_count, sym | child_sym << 8 | flags << 16 | sym_idx << 24}
        mw_ahead = crows[r + 1 < P.n_rows ? r + 1 : r];
        struct { uint32_t pred_begin, pred_count, sym, child_sym, flags, sym_idx; } meta{mw.y, mw.z, mw.w & 0xFFu, (mw.w >> 8) & 0xFFu, (mw.w >> 16) & 0xFFu, mw.w >> 24};
        const uint32_t sym = meta.sym;
        const uint32_t sym2 = sym | (sym << 16);
        uint32_t PMl = INF2;  // min over predecessors of M[p][my first column - 1], both halves

        auto row_body = [&](const uint32_t (&PM)[K], const uint32_t (&PD)[K]) {
            uint32_t (&Mc)[K] = Mout;
            uint32_t (&Dc)[K] = Dout;
            uint32_t Ic[K], PDe[K];
#pragma unroll
            for (int k = 0; k < K; ++k) PDe[k] = pk_add_sat(PD[k], e2);
            if (meta.flags & ROW_END) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    Dc[k] = PDe[k];
                    Mc[k] = pk_min(PM[k], Dc[k]);
                    Ic[k] = INF2;
                }
            } else {
                const uint32_t cs1 = (meta.flags & ROW_OPENI_ALWAYS) ? 0u : (uint32_t)meta.child_sym;
                const uint32_t start_keep = ((meta.flags & ROW_START) && lane == 0 && base == 0) ? 0xFFFF0000u : 0xFFFFFFFFu;
                uint32_t mD[K], mI[K];
                const uint32_t si = meta.sym_idx & 15u, ci = meta.sym_idx >> 4;  // set by build_flat_graph
                if ((meta.sym_idx & 0x88u) == 0) {   // both symbols among ACGT (or no child symbol, table 4): the common row
#pragma unroll
                    for (int h = 0; h < KH; ++h) {
                        const uint4 a = my_tab[(si * KH + h) * 64], c = my_tab[(ci * KH + h) * 64];
                        mD[4 * h] = a.x; mD[4 * h + 1] = a.y; mD[4 * h + 2] = a.z; mD[4 * h + 3] = a.w;
                        mI[4 * h] = c.x; mI[4 * h + 1] = c.y; mI[4 * h + 2] = c.z; mI[4 * h + 3] = c.w;
                    }
                } else {
                    const uint32_t csym2 = cs1 | (cs1 << 16);
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        mD[k] = pku(pkv(0u) - pkv(pk_is_zero(qP[k] ^ sym2)));
                        mI[k] = pku(pkv(0u) - pkv(pk_is_zero(qP[k] ^ csym2)));
                    }
                }
                // one OPERATION at a time over the lane's columns, as in poa_forward_px_kernel
                uint32_t Hc[K], u[K], h1[K];
                const uint32_t cost_left0 = pk_sub_sat(x2, pku(pkv(0u) - pkv(pk_is_zero(qlE ^ sym2))));
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = pk_add_sat(PM[k], oe2);
                h1[0] = cost_left0;
#pragma unroll
                for (int k = 1; k < K; ++k) h1[k] = pk_sub_sat(x2, mD[k - 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = pk_max(u[k], mD[k]);   // D: open a deletion only where the symbols differ (or past the query end, where q is 0)
                h1[0] = pk_add_sat(PMl, h1[0]);
#pragma unroll
                for (int k = 1; k < K; ++k) h1[k] = pk_add_sat(PM[k - 1], h1[k]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) Dc[k] = pk_min(PDe[k], u[k]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) Hc[k] = pk_min(h1[k], Dc[k]);
                Hc[0] &= start_keep;  // H[start][0] = 0
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = pk_add_sat(Hc[k], oe2);
                __builtin_amdgcn_sched_barrier(0);
                // insertion open: A = (q != child symbol) ? H + oe : INF; the open of column k + 1 is issued inside the chain's step k
                u[0] = pk_max(u[0], mI[0]);
                __builtin_amdgcn_sched_barrier(0);
                uint32_t t = INF2;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const uint32_t te = pk_add_sat(t, e2);
                    if (k + 1 < K) u[k + 1] = pk_max(u[k + 1], mI[k + 1]);
                    Ic[k] = t;
                    t = pk_min(te, u[k]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const uint32_t Pm = ~wave_scan_max_minus_pk(~t, step2, w15_2, w31_2);
                const uint32_t excl = pk_wave_shr1(Pm, INF2);
                // carry entering the high half = everything that leaves the low half (nothing enters the window from the left)
                const uint32_t total_lo = (uint32_t)__builtin_amdgcn_readlane((int)Pm, 63) & 0xFFFFu;
                const uint32_t cin = pk_min(excl, pk_add_sat(I16 | (total_lo << 16), lane_off2));
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    Ic[k] = pk_min(Ic[k], pk_add_sat(cin, (uint32_t)k * e2));
                    Mc[k] = pk_min(Hc[k], Ic[k]);
                }
            }

            // stored M value: flags A: I == M (bit 14), C: D == M (bit 15) over the 14-bit score (0x3FFF = INF)
            uint32_t Ms[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t fA = pk_eq_ge(Ic[k], Mc[k]), fC = pk_eq_ge(Dc[k], Mc[k]);
                Ms[k] = (fC << 15) | ((fA << 14) | pk_min(Mc[k], 0x3FFF3FFFu));
            }
            const bool keep_d = (meta.flags & ROW_STORE_D) != 0;
            const uint64_t rbase = (uint64_t)r * pitch;
            const uint64_t dbase = keep_d ? (uint64_t)(cslot ? cslot[r] : r) * pitch : 0;
            if constexpr (K == 8) {   // 16-byte stores, as poa_forward_px_kernel
            if (act_lo) {
                *reinterpret_cast<uint4*>(Mp + rbase + c_lo) = make_uint4(pk_lo_lo(Ms[0], Ms[1]), pk_lo_lo(Ms[2], Ms[3]), pk_lo_lo(Ms[4], Ms[5]), pk_lo_lo(Ms[6], Ms[7]));
                if (keep_d) *reinterpret_cast<uint4*>(Dp + dbase + c_lo) = make_uint4(pk_lo_lo(Dc[0], Dc[1]), pk_lo_lo(Dc[2], Dc[3]), pk_lo_lo(Dc[4], Dc[5]), pk_lo_lo(Dc[6], Dc[7]));
            }
            if (act_hi) {
                *reinterpret_cast<uint4*>(Mp + rbase + c_hi) = make_uint4(pk_hi_hi(Ms[0], Ms[1]), pk_hi_hi(Ms[2], Ms[3]), pk_hi_hi(Ms[4], Ms[5]), pk_hi_hi(Ms[6], Ms[7]));
                if (keep_d) *reinterpret_cast<uint4*>(Dp + dbase + c_hi) = make_uint4(pk_hi_hi(Dc[0], Dc[1]), pk_hi_hi(Dc[2], Dc[3]), pk_hi_hi(Dc[4], Dc[5]), pk_hi_hi(Dc[6], Dc[7]));
            }
            } else {
                if (act_lo) {
                    *reinterpret_cast<uint2*>(Mp + rbase + c_lo) = make_uint2(pk_lo_lo(Ms[0], Ms[1]), pk_lo_lo(Ms[2], Ms[3]));
                    if (keep_d) *reinterpret_cast<uint2*>(Dp + dbase + c_lo) = make_uint2(pk_lo_lo(Dc[0], Dc[1]), pk_lo_lo(Dc[2], Dc[3]));
                }
                if (act_hi) {
                    *reinterpret_cast<uint2*>(Mp + rbase + c_hi) = make_uint2(pk_hi_hi(Ms[0], Ms[1]), pk_hi_hi(Ms[2], Ms[3]));
                    if (keep_d) *reinterpret_cast<uint2*>(Dp + dbase + c_hi) = make_uint2(pk_hi_hi(Dc[0], Dc[1]), pk_hi_hi(Dc[2], Dc[3]));
                }
            }
            if (!FULL && (meta.flags & ROW_END)) {
                // the end cell (end row, L), if the window holds it: window column wc sits in lane (wc & 255) / 4, register wc & 3
                const uint32_t wc = L - base;
                if (L >= base && wc < WIN) {
                    const uint32_t kk = wc & 3u;
                    const uint32_t v = kk == 0 ? Mc[0] : (kk == 1 ? Mc[1] : (kk == 2 ? Mc[2] : Mc[K > 3 ? 3 : 0]));
                    const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane((int)((wc & (QW - 1)) >> 2)));
                    end_score = wc < QW ? (w & 0xFFFFu) : (w >> 16);
                }
            }
        };

        if (meta.flags & ROW_CHAIN) {
            PMl = shr_lane(Mprev[K - 1]);
            row_body(Mprev, Dprev);
        } else if ((meta.flags & ROW_SAME_PREDS) && (FULL || (r & (BAND_ROWS - 1)) != 0)) {
            // (a sibling row that opens a segment recomputes the minima: the cached ones are those of the old window)
            PMl = PMlc;
            row_body(PMc, PDc);
        } else {
            uint32_t (&PM)[K] = PMc;
            uint32_t (&PD)[K] = PDc;
#pragma unroll
            for (int k = 0; k < K; ++k) { PM[k] = INF2; PD[k] = INF2; }
            if (meta.pred_count > 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // I read back rows this wave stored
            for (uint32_t pe = 0; pe < meta.pred_count; ++pe) {
                const uint32_t pr = cpred[meta.pred_begin + pe];
                uint32_t tm[K], td[K];
                if (pr + 1 == r) {
#pragma unroll
                    for (int k = 0; k < K; ++k) { tm[k] = Mprev[k]; td[k] = Dprev[k]; }
                } else {
                    // a row read from memory counts as INF outside the window of ITS segment (stale memory lies there)
                    const uint32_t pb = FULL ? 0u : cbase[pr / BAND_ROWS];
                    const uint64_t pbase = (uint64_t)pr * pitch;
                    const uint64_t pbase_d = cpslot ? (uint64_t)cpslot[meta.pred_begin + pe] * pitch : pbase;
                    const bool in_lo = act_lo && (FULL || c_lo - pb < WIN);   // (unsigned: also false left of that window)
                    const bool in_hi = act_hi && (FULL || c_hi - pb < WIN);
                    if constexpr (K == 8) {   // 16-byte accesses, as poa_forward_px_kernel: two 8-byte ones per array cost it registers
                        uint4 m0 = make_uint4(INF2, INF2, INF2, INF2), d0 = m0, m1 = m0, d1 = m0;
                        if (in_lo) {
                            m0 = *reinterpret_cast<const uint4*>(Mp + pbase + c_lo);
                            d0 = *reinterpret_cast<const uint4*>(Dp + pbase_d + c_lo);
                        }
                        if (in_hi) {
                            m1 = *reinterpret_cast<const uint4*>(Mp + pbase + c_hi);
                            d1 = *reinterpret_cast<const uint4*>(Dp + pbase_d + c_hi);
                        }
                        const uint32_t a0[4] = {m0.x, m0.y, m0.z, m0.w}, a1[4] = {m1.x, m1.y, m1.z, m1.w};
                        const uint32_t b0[4] = {d0.x, d0.y, d0.z, d0.w}, b1[4] = {d1.x, d1.y, d1.z, d1.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            tm[2 * i] = pk_lo_lo(a0[i], a1[i]); tm[2 * i + 1] = pk_hi_hi(a0[i], a1[i]);
                            td[2 * i] = pk_lo_lo(b0[i], b1[i]); td[2 * i + 1] = pk_hi_hi(b0[i], b1[i]);
                        }
                    } else {
                        uint2 m0 = make_uint2(INF2, INF2), d0 = m0, m1 = m0, d1 = m0;
                        if (in_lo) {
                            m0 = *reinterpret_cast<const uint2*>(Mp + pbase + c_lo);
                            d0 = *reinterpret_cast<const uint2*>(Dp + pbase_d + c_lo);
                        }
                        if (in_hi) {
                            m1 = *reinterpret_cast<const uint2*>(Mp + pbase + c_hi);
                            d1 = *reinterpret_cast<const uint2*>(Dp + pbase_d + c_hi);
                        }
                        tm[0] = pk_lo_lo(m0.x, m1.x); tm[1] = pk_hi_hi(m0.x, m1.x); tm[2] = pk_lo_lo(m0.y, m1.y); tm[3] = pk_hi_hi(m0.y, m1.y);
                        td[0] = pk_lo_lo(d0.x, d1.x); td[1] = pk_hi_hi(d0.x, d1.x); td[2] = pk_lo_lo(d0.y, d1.y); td[3] = pk_hi_hi(d0.y, d1.y);
                    }
                    // strip the flags; the 14-bit INF becomes the 16-bit one again
                    constexpr uint32_t VM = 0x3FFF3FFFu;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const uint32_t v = tm[k] & VM;
                        const uint32_t is_inf = pku(pkv(0u) - pkv(pk_is_zero(v ^ VM)));  // 0xFFFF per half
                        tm[k] = v | (is_inf & ~VM);
                    }
                }
                PMl = pk_min(PMl, shr_lane(tm[K - 1]));
#pragma unroll
                for (int k = 0; k < K; ++k) { PM[k] = pk_min(PM[k], tm[k]); PD[k] = pk_min(PD[k], td[k]); }
            }
            PMlc = PMl;
            row_body(PM, PD);
        }
    };

    // A window move: a row array goes through LDS and comes back at the new columns; what the old window did not hold is INF.
    // Bases are multiples of 8, so a lane's four columns lie inside the old window together or not at all.
    auto move_put = [&](int slot, const uint32_t (&a)[K]) {
        my_move[slot * 128 + lane] = make_uint2(pk_lo_lo(a[0], a[1]), pk_lo_lo(a[2], a[3]));
        my_move[slot * 128 + 64 + lane] = make_uint2(pk_hi_hi(a[0], a[1]), pk_hi_hi(a[2], a[3]));
    };
    auto move_get = [&](int slot, const uint32_t shift, uint32_t (&a)[K]) {
        const uint32_t o_lo = shift + K * lane, o_hi = shift + QW + K * lane;   // my new columns as columns of the old window
        uint2 v0 = make_uint2(INF2, INF2), v1 = v0;
        if (o_lo < WIN) v0 = my_move[slot * 128 + (o_lo >> 2)];
        if (o_hi < WIN) v1 = my_move[slot * 128 + (o_hi >> 2)];
        a[0] = pk_lo_lo(v0.x, v1.x); a[1] = pk_hi_hi(v0.x, v1.x); a[2] = pk_lo_lo(v0.y, v1.y); a[3] = pk_hi_hi(v0.y, v1.y);
    };

    uint32_t MA[K], DA[K], MB[K], DB[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { MA[k] = INF2; DA[k] = INF2; }
    place(FULL ? 0u : cbase[0]);
    uint32_t r = 0;
    for (; r < P.n_rows; r += 2) {
        if (!FULL && r && (r & (BAND_ROWS - 1)) == 0) {
            const uint32_t nb = cbase[r / BAND_ROWS];
            if (nb != base) {
                const uint32_t shift = nb - base;   // (wraps for a move to the left: such columns test as outside, then wrap back inside)
                move_put(0, MA); move_put(1, DA);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                move_get(0, shift, MA); move_get(1, shift, DA);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                place(nb);
            }
        }
        do_row(r, MA, DA, MB, DB);
        if (r + 1 < P.n_rows) do_row(r + 1, MB, DB, MA, DA);
    }

    if (FULL) return;
    // certified: the computed end score is finite and <= T = e * (D - 4)
    const uint32_t T = e * (band_d - 4u) < 0x3FFEu ? e * (band_d - 4u) : 0x3FFEu;
    if (!(end_score <= T)) {
        if (lane == 0) {
            B.list[P.first_query + atomicAdd(B.count, 1u)] = qi;
            if (LIST && B.n_order) atomicAdd(B.count_nf, 1u);
        }
    }
}

// Two queries of one band class per wave: the row body of poa_forward_band_kernel<true> (eight registers per row array, 16-byte
// plane accesses, one scan over the 64 lanes) over the WINDOW of poa_forward_band_kernel<false>.  Lane l owns window columns
// base + 8l .. base + 8l + 7 and in every register
//      lo half = that column of query A,   hi half = the same column of query B,
// A = B.order[2w], B = B.order[2w + 1] for wave w: two queries of the same length, hence the same pitch, D and window bases
// (the host pairs them, poa_engine.hip).  The wave runs the scalar part of a row - row words, flags, branches, addresses -
// once for both.  Window, left-edge rule, recurrences and the certificate are those of <false>, so every stored word and the
// set of cells written are the same; a query that fails the certificate is appended to the fallback list on
// its own, its partner stays certified.
// LDS: the four ACGT mask tables, 8 KB per wave (the table "no child symbol" of the other instantiations is all zeros and is
// not kept); the hand-over buffer of a window move (2 arrays x 2 queries x 512 u16 = 4 KB) lies over them, since place()
// rebuilds the tables right after every move.  32 KB per workgroup, and at most 96 VGPRs: five workgroups per CU.
//
// K = 6 is the NARROW tier: the same pass over a window of 384 columns (BAND_WINDOW_NARROW), six registers per row array, under
// the class's narrow plan (its own D and bases; the launcher hands them in as B.cls_d and B.cls_base, and the list of the 512
// pass as B.list).  A lane's six columns are three dwords of a plane row, and bases stay multiples of 8, so whatever K = 8
// decides per lane is decided per DWORD here: a lane may straddle the end of the plane row (the pitch is a multiple of 8, 6 *
// lane is not) or the edge of a predecessor's window, and a window moves by a number of columns that is no multiple of 6.
// LDS: four tables of six registers (a 16-byte and an 8-byte piece per lane), 6 KB per wave; the hand-over buffer (3 KB) over them.
template <int K>
__global__ __launch_bounds__(256) void poa_forward_band2_kernel(FwdParams P, BandParams B) {
    static_assert(K == 8 || K == 6, "the 512-column window or the narrow one");
    constexpr uint32_t WIN = 64 * K;
    static_assert(WIN == (K == 8 ? BAND_WINDOW : BAND_WINDOW_NARROW) && BAND_BASE_ALIGN % 8 == 0,
                  "K = 8: a lane's eight columns move together; K = 6: a lane's dwords do");
    constexpr uint32_t I16 = 0xFFFFu, INF2 = 0xFFFFFFFFu;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wp = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wp >= P.n_queries) return;   // (the launch's pairs)
    const uint32_t qa = ((const CU32*)B.order)[2 * wp], qb = ((const CU32*)B.order)[2 * wp + 1];
    const uint32_t cl = ((const CU32*)B.cls)[qa];
    const uint32_t band_d = ((const CU32*)B.cls_d)[cl] < B.d_cap ? ((const CU32*)B.cls_d)[cl] : B.d_cap;
    if (band_d < 4) {   // (the cap of a test took the band away)
        if (lane == 0) {
            B.list[P.first_query + atomicAdd(B.count, 1u)] = qa;
            B.list[P.first_query + atomicAdd(B.count, 1u)] = qb;
        }
        return;
    }
    const uint64_t qbeg_a = P.qoff[qa], qbeg_b = P.qoff[qb];
    const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(P.qoff[qa + 1] - qbeg_a));
    const uint8_t* __restrict__ q_a = P.qseq + qbeg_a;
    const uint8_t* __restrict__ q_b = P.qseq + qbeg_b;
    const uint32_t pitch = (uint32_t)__builtin_amdgcn_readfirstlane((int)P.pitch[qa]);
    const uint64_t RP = (uint64_t)P.n_rows * pitch;
    uint16_t* __restrict__ Mp_a = reinterpret_cast<uint16_t*>(P.planes) + P.plane_off[qa];
    uint16_t* __restrict__ Mp_b = reinterpret_cast<uint16_t*>(P.planes) + P.plane_off[qb];
    const uint64_t d_off = RP + RP / 4;   // the kept D rows behind the M plane, as in <false>
    const uint32_t e = P.cost_e, x = P.cost_x;
    const uint32_t e2 = e | (e << 16), oe2 = P.cost_oe | (P.cost_oe << 16), x2 = x | (x << 16);
    auto pack16 = [](uint32_t v) { v = v < I16 ? v : I16; return v | (v << 16); };
    const uint32_t step = K * e;
    const uint32_t step2 = pack16(step);
    const uint32_t w15_2 = pack16(((lane & 15u) + 1u) * step);
    const uint32_t w31_2 = pack16(lane >= 32u ? (lane - 31u) * step : 0xFFFFu);

    const CRowWords* crows = (const CRowWords*)P.rows;
    const CU32* cpred = (const CU32*)P.pred_rows;
    const CU32* cslot = (const CU32*)P.d_slot;
    const CU32* cpslot = (const CU32*)P.pred_dslot;
    const CU32* cbase = (const CU32*)(B.cls_base + (uint64_t)cl * B.n_seg);

    constexpr uint32_t TAB_WAVE = K == 8 ? 4 * 2 * 64 : 4 * 64 + 2 * 64;   // uint4 per wave (K = 6: 4 x 64 uint4, then 4 x 64 uint2)
    __shared__ uint4 sym_tab[4 * TAB_WAVE];
    uint4* my_tab = sym_tab + (threadIdx.x >> 6) * TAB_WAVE + lane;
    uint4* my_move = sym_tab + (threadIdx.x >> 6) * TAB_WAVE;   // [array][query][lane] (K = 6: [array][query][dword of the window])
    uint2* my_tab2 = reinterpret_cast<uint2*>(my_move + 4 * 64) + lane;   // (K = 6) registers 4 and 5 of the tables

    uint32_t base = 0, c0 = 0;
    bool act = false;
    uint32_t nd = 0;   // (K = 6) my dwords inside the plane row: 0..3; act = all three
    uint32_t qP[K], qlE = 0;
    auto place = [&](const uint32_t nb) {
        base = nb;
        c0 = nb + K * lane;
        if constexpr (K == 8) act = c0 < pitch;
        else {
            nd = c0 < pitch ? ((pitch - c0) >> 1 < 3u ? (pitch - c0) >> 1 : 3u) : 0u;   // (c0 and the pitch are even)
            act = nd == 3u;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool in = c0 + k < L;
            qP[k] = (in ? (uint32_t)q_a[c0 + k] : 0u) | ((in ? (uint32_t)q_b[c0 + k] : 0u) << 16);
        }
        const bool in_l = c0 > 0 && c0 - 1 < L;
        qlE = (in_l ? (uint32_t)q_a[c0 - 1] : 0u) | ((in_l ? (uint32_t)q_b[c0 - 1] : 0u) << 16);
        const uint32_t letters[4] = {'A', 'C', 'G', 'T'};
#pragma unroll
        for (int si = 0; si < 4; ++si) {
            const uint32_t s2 = letters[si] | (letters[si] << 16);
            uint32_t m[K];
#pragma unroll
            for (int k = 0; k < K; ++k) m[k] = pku(pkv(0u) - pkv(pk_is_zero(qP[k] ^ s2)));
            if constexpr (K == 8) {
                my_tab[(si * 2) * 64] = make_uint4(m[0], m[1], m[2], m[3]);
                my_tab[(si * 2 + 1) * 64] = make_uint4(m[4], m[5], m[6], m[7]);
            } else {
                my_tab[si * 64] = make_uint4(m[0], m[1], m[2], m[3]);
                my_tab2[si * 64] = make_uint2(m[4], m[5]);
            }
        }
        // each lane reads back only what it wrote itself: no barrier needed
    };

    uint32_t PMc[K], PDc[K], PMlc = INF2;
#pragma unroll
    for (int k = 0; k < K; ++k) { PMc[k] = INF2; PDc[k] = INF2; }

    // lane l <- v of lane l-1; lane 0: INF in both halves (left of the window, as the lo half of <false>)
    auto shr_lane = [&](uint32_t v) { return pk_wave_shr1(v, INF2); };

    uint32_t end_a = I16, end_b = I16;   // M[end row][L] of A and of B as computed (INF: outside the window)
    poa_u32x4 mw_ahead = crows[0];
    auto do_row = [&](const uint32_t r, const uint32_t (&Mprev)[K], const uint32_t (&Dprev)[K], uint32_t (&Mout)[K], uint32_t (&Dout)[K]) {
        const poa_u32x4 mw = mw_ahead;
        mw_ahead = crows[r + 1 < P.n_rows ? r + 1 : r];
        struct { uint32_t pred_begin, pred_count, sym, child_sym, flags, sym_idx; } meta{mw.y, mw.z, mw.w & 0xFFu, (mw.w >> 8) & 0xFFu, (mw.w >> 16) & 0xFFu, mw.w >> 24};
        const uint32_t sym = meta.sym;
        const uint32_t sym2 = sym | (sym << 16);
        uint32_t PMl = INF2;

        auto row_body = [&](const uint32_t (&PM)[K], const uint32_t (&PD)[K]) {
            uint32_t (&Mc)[K] = Mout;
            uint32_t (&Dc)[K] = Dout;
            uint32_t Ic[K], PDe[K];
#pragma unroll
            for (int k = 0; k < K; ++k) PDe[k] = pk_add_sat(PD[k], e2);
            if (meta.flags & ROW_END) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    Dc[k] = PDe[k];
                    Mc[k] = pk_min(PM[k], Dc[k]);
                    Ic[k] = INF2;
                }
            } else {
                const uint32_t cs1 = (meta.flags & ROW_OPENI_ALWAYS) ? 0u : (uint32_t)meta.child_sym;
                const uint32_t start_keep = ((meta.flags & ROW_START) && lane == 0 && base == 0) ? 0u : 0xFFFFFFFFu;
                uint32_t mD[K], mI[K];
                const uint32_t si = meta.sym_idx & 15u, ci = meta.sym_idx >> 4;
                if ((meta.sym_idx & 0x88u) == 0) {   // both symbols among ACGT, or no child symbol (ci == 4: no mask)
                    if constexpr (K == 8) {
                    const uint4 a0 = my_tab[(si * 2) * 64], a1 = my_tab[(si * 2 + 1) * 64];
                    mD[0] = a0.x; mD[1] = a0.y; mD[2] = a0.z; mD[3] = a0.w; mD[4] = a1.x; mD[5] = a1.y; mD[6] = a1.z; mD[7] = a1.w;
                    if (ci < 4u) {
                        const uint4 c0_ = my_tab[(ci * 2) * 64], c1_ = my_tab[(ci * 2 + 1) * 64];
                        mI[0] = c0_.x; mI[1] = c0_.y; mI[2] = c0_.z; mI[3] = c0_.w; mI[4] = c1_.x; mI[5] = c1_.y; mI[6] = c1_.z; mI[7] = c1_.w;
                    } else {
#pragma unroll
                        for (int k = 0; k < K; ++k) mI[k] = 0u;
                    }
                    } else {
                        const uint4 a0 = my_tab[si * 64];
                        const uint2 a1 = my_tab2[si * 64];
                        mD[0] = a0.x; mD[1] = a0.y; mD[2] = a0.z; mD[3] = a0.w; mD[4] = a1.x; mD[5] = a1.y;
                        if (ci < 4u) {
                            const uint4 c0_ = my_tab[ci * 64];
                            const uint2 c1_ = my_tab2[ci * 64];
                            mI[0] = c0_.x; mI[1] = c0_.y; mI[2] = c0_.z; mI[3] = c0_.w; mI[4] = c1_.x; mI[5] = c1_.y;
                        } else {
#pragma unroll
                            for (int k = 0; k < K; ++k) mI[k] = 0u;
                        }
                    }
                } else {
                    const uint32_t csym2 = cs1 | (cs1 << 16);
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        mD[k] = pku(pkv(0u) - pkv(pk_is_zero(qP[k] ^ sym2)));
                        mI[k] = pku(pkv(0u) - pkv(pk_is_zero(qP[k] ^ csym2)));
                    }
                }
                uint32_t Hc[K], u[K], h1[K];
                const uint32_t cost_left0 = pk_sub_sat(x2, pku(pkv(0u) - pkv(pk_is_zero(qlE ^ sym2))));
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = pk_add_sat(PM[k], oe2);
                h1[0] = cost_left0;
#pragma unroll
                for (int k = 1; k < K; ++k) h1[k] = pk_sub_sat(x2, mD[k - 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = pk_max(u[k], mD[k]);
                h1[0] = pk_add_sat(PMl, h1[0]);
#pragma unroll
                for (int k = 1; k < K; ++k) h1[k] = pk_add_sat(PM[k - 1], h1[k]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) Dc[k] = pk_min(PDe[k], u[k]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) Hc[k] = pk_min(h1[k], Dc[k]);
                Hc[0] &= start_keep;  // H[start][0] = 0 for both queries
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = pk_add_sat(Hc[k], oe2);
                __builtin_amdgcn_sched_barrier(0);
                u[0] = pk_max(u[0], mI[0]);
                __builtin_amdgcn_sched_barrier(0);
                uint32_t t = INF2;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const uint32_t te = pk_add_sat(t, e2);
                    if (k + 1 < K) u[k + 1] = pk_max(u[k + 1], mI[k + 1]);
                    Ic[k] = t;
                    t = pk_min(te, u[k]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // one scan over the 64 lanes serves both queries; nothing enters the window from the left
                const uint32_t Pm = ~wave_scan_max_minus_pk(~t, step2, w15_2, w31_2);
                const uint32_t cin = pk_wave_shr1(Pm, INF2);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    Ic[k] = pk_min(Ic[k], pk_add_sat(cin, (uint32_t)k * e2));
                    Mc[k] = pk_min(Hc[k], Ic[k]);
                }
            }

            uint32_t Ms[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t fA = pk_eq_ge(Ic[k], Mc[k]), fC = pk_eq_ge(Dc[k], Mc[k]);
                Ms[k] = (fC << 15) | ((fA << 14) | pk_min(Mc[k], 0x3FFF3FFFu));
            }
            const bool keep_d = (meta.flags & ROW_STORE_D) != 0;
            const uint64_t rbase = (uint64_t)r * pitch;
            const uint64_t dbase = d_off + (keep_d ? (uint64_t)(cslot ? cslot[r] : r) * pitch : 0);
            if constexpr (K == 8) {
            if (act) {
                *reinterpret_cast<uint4*>(Mp_a + rbase + c0) = make_uint4(pk_lo_lo(Ms[0], Ms[1]), pk_lo_lo(Ms[2], Ms[3]), pk_lo_lo(Ms[4], Ms[5]), pk_lo_lo(Ms[6], Ms[7]));
                *reinterpret_cast<uint4*>(Mp_b + rbase + c0) = make_uint4(pk_hi_hi(Ms[0], Ms[1]), pk_hi_hi(Ms[2], Ms[3]), pk_hi_hi(Ms[4], Ms[5]), pk_hi_hi(Ms[6], Ms[7]));
                if (keep_d) {
                    *reinterpret_cast<uint4*>(Mp_a + dbase + c0) = make_uint4(pk_lo_lo(Dc[0], Dc[1]), pk_lo_lo(Dc[2], Dc[3]), pk_lo_lo(Dc[4], Dc[5]), pk_lo_lo(Dc[6], Dc[7]));
                    *reinterpret_cast<uint4*>(Mp_b + dbase + c0) = make_uint4(pk_hi_hi(Dc[0], Dc[1]), pk_hi_hi(Dc[2], Dc[3]), pk_hi_hi(Dc[4], Dc[5]), pk_hi_hi(Dc[6], Dc[7]));
                }
            }
            } else {
                // twelve bytes per query and array at 4-byte alignment; the lane that straddles the end of the plane row stores
                // only its dwords inside it (the next one would land in the next row, after the last row outside the plane)
                if (act) {
                    *reinterpret_cast<uint3*>(Mp_a + rbase + c0) = make_uint3(pk_lo_lo(Ms[0], Ms[1]), pk_lo_lo(Ms[2], Ms[3]), pk_lo_lo(Ms[4], Ms[5]));
                    *reinterpret_cast<uint3*>(Mp_b + rbase + c0) = make_uint3(pk_hi_hi(Ms[0], Ms[1]), pk_hi_hi(Ms[2], Ms[3]), pk_hi_hi(Ms[4], Ms[5]));
                    if (keep_d) {
                        *reinterpret_cast<uint3*>(Mp_a + dbase + c0) = make_uint3(pk_lo_lo(Dc[0], Dc[1]), pk_lo_lo(Dc[2], Dc[3]), pk_lo_lo(Dc[4], Dc[5]));
                        *reinterpret_cast<uint3*>(Mp_b + dbase + c0) = make_uint3(pk_hi_hi(Dc[0], Dc[1]), pk_hi_hi(Dc[2], Dc[3]), pk_hi_hi(Dc[4], Dc[5]));
                    }
                } else if (nd) {
                    *reinterpret_cast<uint32_t*>(Mp_a + rbase + c0) = pk_lo_lo(Ms[0], Ms[1]);
                    *reinterpret_cast<uint32_t*>(Mp_b + rbase + c0) = pk_hi_hi(Ms[0], Ms[1]);
                    if (nd == 2u) {
                        *reinterpret_cast<uint32_t*>(Mp_a + rbase + c0 + 2) = pk_lo_lo(Ms[2], Ms[3]);
                        *reinterpret_cast<uint32_t*>(Mp_b + rbase + c0 + 2) = pk_hi_hi(Ms[2], Ms[3]);
                    }
                    if (keep_d) {
                        *reinterpret_cast<uint32_t*>(Mp_a + dbase + c0) = pk_lo_lo(Dc[0], Dc[1]);
                        *reinterpret_cast<uint32_t*>(Mp_b + dbase + c0) = pk_hi_hi(Dc[0], Dc[1]);
                        if (nd == 2u) {
                            *reinterpret_cast<uint32_t*>(Mp_a + dbase + c0 + 2) = pk_lo_lo(Dc[2], Dc[3]);
                            *reinterpret_cast<uint32_t*>(Mp_b + dbase + c0 + 2) = pk_hi_hi(Dc[2], Dc[3]);
                        }
                    }
                }
            }
            if (meta.flags & ROW_END) {
                // the end cell (end row, L), if the window holds it: window column wc sits in lane wc / K, register wc % K
                const uint32_t wc = L - base;
                if (L >= base && wc < WIN) {
                    const uint32_t kk = wc % (uint32_t)K;
                    // (every register is read out and the choice made among scalars: a choice among the registers themselves
                    // becomes an indexed access that puts the row arrays into scratch)
                    const int src = __builtin_amdgcn_readfirstlane((int)(wc / (uint32_t)K));
                    uint32_t w = 0;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const uint32_t wk = (uint32_t)__builtin_amdgcn_readlane((int)Mc[k], src);
                        w = kk == (uint32_t)k ? wk : w;
                    }
                    end_a = w & 0xFFFFu;
                    end_b = w >> 16;
                }
            }
        };

        if (meta.flags & ROW_CHAIN) {
            PMl = shr_lane(Mprev[K - 1]);
            row_body(Mprev, Dprev);
        } else if ((meta.flags & ROW_SAME_PREDS) && (r & (BAND_ROWS - 1)) != 0) {
            // (a sibling row that opens a segment recomputes the minima: the cached ones are those of the old window)
            PMl = PMlc;
            row_body(PMc, PDc);
        } else {
            uint32_t (&PM)[K] = PMc;
            uint32_t (&PD)[K] = PDc;
#pragma unroll
            for (int k = 0; k < K; ++k) { PM[k] = INF2; PD[k] = INF2; }
            if (meta.pred_count > 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // I read back rows this wave stored
            for (uint32_t pe = 0; pe < meta.pred_count; ++pe) {
                const uint32_t pr = cpred[meta.pred_begin + pe];
                uint32_t tm[K], td[K];
                if (pr + 1 == r) {
#pragma unroll
                    for (int k = 0; k < K; ++k) { tm[k] = Mprev[k]; td[k] = Dprev[k]; }
                } else {
                    // a row read from memory counts as INF outside the window of ITS segment (stale memory lies there)
                    const uint32_t pb = cbase[pr / BAND_ROWS];
                    const uint64_t pbase = (uint64_t)pr * pitch;
                    const uint64_t pbase_d = d_off + (cpslot ? (uint64_t)cpslot[meta.pred_begin + pe] * pitch : pbase);
                    if constexpr (K == 8) {
                    const bool in = act && c0 - pb < WIN;   // (unsigned: also false left of that window)
                    uint4 m0 = make_uint4(INF2, INF2, INF2, INF2), d0 = m0, m1 = m0, d1 = m0;
                    if (in) {
                        m0 = *reinterpret_cast<const uint4*>(Mp_a + pbase + c0);
                        d0 = *reinterpret_cast<const uint4*>(Mp_a + pbase_d + c0);
                        m1 = *reinterpret_cast<const uint4*>(Mp_b + pbase + c0);
                        d1 = *reinterpret_cast<const uint4*>(Mp_b + pbase_d + c0);
                    }
                    const uint32_t a0[4] = {m0.x, m0.y, m0.z, m0.w}, a1[4] = {m1.x, m1.y, m1.z, m1.w};
                    const uint32_t b0[4] = {d0.x, d0.y, d0.z, d0.w}, b1[4] = {d1.x, d1.y, d1.z, d1.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        tm[2 * i] = pk_lo_lo(a0[i], a1[i]); tm[2 * i + 1] = pk_hi_hi(a0[i], a1[i]);
                        td[2 * i] = pk_lo_lo(b0[i], b1[i]); td[2 * i + 1] = pk_hi_hi(b0[i], b1[i]);
                    }
                    } else {
                        // per dword: inside the plane row and inside the predecessor's window (both edges are even columns, so a
                        // dword's two columns lie on one side; unsigned: also false left of that window)
                        const uint32_t off = c0 - pb;
                        const bool in0 = nd > 0u && off < WIN, in1 = nd > 1u && off + 2u < WIN, in2 = nd > 2u && off + 4u < WIN;
                        uint32_t a0[3] = {INF2, INF2, INF2}, a1[3] = {INF2, INF2, INF2}, b0[3] = {INF2, INF2, INF2}, b1[3] = {INF2, INF2, INF2};
                        if (in0 && in2) {   // (then in1 as well) the whole lane
                            const uint3 m0 = *reinterpret_cast<const uint3*>(Mp_a + pbase + c0), d0 = *reinterpret_cast<const uint3*>(Mp_a + pbase_d + c0);
                            const uint3 m1 = *reinterpret_cast<const uint3*>(Mp_b + pbase + c0), d1 = *reinterpret_cast<const uint3*>(Mp_b + pbase_d + c0);
                            a0[0] = m0.x; a0[1] = m0.y; a0[2] = m0.z; a1[0] = m1.x; a1[1] = m1.y; a1[2] = m1.z;
                            b0[0] = d0.x; b0[1] = d0.y; b0[2] = d0.z; b1[0] = d1.x; b1[1] = d1.y; b1[2] = d1.z;
                        } else {
                            const bool ins[3] = {in0, in1, in2};
#pragma unroll
                            for (int i = 0; i < 3; ++i) {
                                if (ins[i]) {
                                    a0[i] = *reinterpret_cast<const uint32_t*>(Mp_a + pbase + c0 + 2 * i);
                                    b0[i] = *reinterpret_cast<const uint32_t*>(Mp_a + pbase_d + c0 + 2 * i);
                                    a1[i] = *reinterpret_cast<const uint32_t*>(Mp_b + pbase + c0 + 2 * i);
                                    b1[i] = *reinterpret_cast<const uint32_t*>(Mp_b + pbase_d + c0 + 2 * i);
                                }
                            }
                        }
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            tm[2 * i] = pk_lo_lo(a0[i], a1[i]); tm[2 * i + 1] = pk_hi_hi(a0[i], a1[i]);
                            td[2 * i] = pk_lo_lo(b0[i], b1[i]); td[2 * i + 1] = pk_hi_hi(b0[i], b1[i]);
                        }
                    }
                    // strip the flags; the 14-bit INF becomes the 16-bit one again
                    constexpr uint32_t VM = 0x3FFF3FFFu;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const uint32_t v = tm[k] & VM;
                        const uint32_t is_inf = pku(pkv(0u) - pkv(pk_is_zero(v ^ VM)));
                        tm[k] = v | (is_inf & ~VM);
                    }
                }
                PMl = pk_min(PMl, shr_lane(tm[K - 1]));
#pragma unroll
                for (int k = 0; k < K; ++k) { PM[k] = pk_min(PM[k], tm[k]); PD[k] = pk_min(PD[k], td[k]); }
            }
            PMlc = PMl;
            row_body(PM, PD);
        }
    };

    // A window move, as in <false>: a row array of both queries goes through LDS and comes back at the new columns; what the
    // old window did not hold is INF.  Bases are multiples of 8: a lane's eight columns lie inside the old window or outside.
    // K = 6: the buffer holds the old window dword by dword ([array][query][WIN / 2]); a shift is a multiple of 8 columns, so my
    // three dwords are three dwords of the old window, each of them inside it or not on its own.
    uint32_t* my_move1 = reinterpret_cast<uint32_t*>(my_move);
    auto move_put = [&](int slot, const uint32_t (&a)[K]) {
        if constexpr (K == 8) {
        my_move[(slot * 2) * 64 + lane] = make_uint4(pk_lo_lo(a[0], a[1]), pk_lo_lo(a[2], a[3]), pk_lo_lo(a[4], a[5]), pk_lo_lo(a[6], a[7]));
        my_move[(slot * 2 + 1) * 64 + lane] = make_uint4(pk_hi_hi(a[0], a[1]), pk_hi_hi(a[2], a[3]), pk_hi_hi(a[4], a[5]), pk_hi_hi(a[6], a[7]));
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                my_move1[(slot * 2) * (WIN / 2) + 3 * lane + i] = pk_lo_lo(a[2 * i], a[2 * i + 1]);
                my_move1[(slot * 2 + 1) * (WIN / 2) + 3 * lane + i] = pk_hi_hi(a[2 * i], a[2 * i + 1]);
            }
        }
    };
    auto move_get = [&](int slot, const uint32_t shift, uint32_t (&a)[K]) {
        const uint32_t o = shift + K * lane;   // my new columns as columns of the old window
        if constexpr (K == 8) {
        uint4 v0 = make_uint4(INF2, INF2, INF2, INF2), v1 = v0;
        if (o < WIN) {
            v0 = my_move[(slot * 2) * 64 + (o >> 3)];
            v1 = my_move[(slot * 2 + 1) * 64 + (o >> 3)];
        }
        a[0] = pk_lo_lo(v0.x, v1.x); a[1] = pk_hi_hi(v0.x, v1.x); a[2] = pk_lo_lo(v0.y, v1.y); a[3] = pk_hi_hi(v0.y, v1.y);
        a[4] = pk_lo_lo(v0.z, v1.z); a[5] = pk_hi_hi(v0.z, v1.z); a[6] = pk_lo_lo(v0.w, v1.w); a[7] = pk_hi_hi(v0.w, v1.w);
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint32_t oc = o + 2u * i;   // (unsigned: a column left of the old window tests as outside)
                uint32_t v0 = INF2, v1 = INF2;
                if (oc < WIN) {
                    v0 = my_move1[(slot * 2) * (WIN / 2) + (oc >> 1)];
                    v1 = my_move1[(slot * 2 + 1) * (WIN / 2) + (oc >> 1)];
                }
                a[2 * i] = pk_lo_lo(v0, v1); a[2 * i + 1] = pk_hi_hi(v0, v1);
            }
        }
    };

    uint32_t MA[K], DA[K], MB[K], DB[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { MA[k] = INF2; DA[k] = INF2; }
    place(cbase[0]);
    for (uint32_t r = 0; r < P.n_rows; r += 2) {
        if (r && (r & (BAND_ROWS - 1)) == 0) {
            const uint32_t nb = cbase[r / BAND_ROWS];
            if (nb != base) {
                const uint32_t shift = nb - base;   // (wraps for a move to the left: such columns test as outside, then wrap back inside)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the buffer lies over the tables: their reads are done
                __builtin_amdgcn_wave_barrier();
                move_put(0, MA); move_put(1, DA);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                move_get(0, shift, MA); move_get(1, shift, DA);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                place(nb);
            }
        }
        do_row(r, MA, DA, MB, DB);
        if (r + 1 < P.n_rows) do_row(r + 1, MB, DB, MA, DA);
    }

    // certified, each query on its own: the computed end score is finite and <= T = e * (D - 4)
    const uint32_t T = e * (band_d - 4u) < 0x3FFEu ? e * (band_d - 4u) : 0x3FFEu;
    if (lane == 0) {
        if (!(end_a <= T)) B.list[P.first_query + atomicAdd(B.count, 1u)] = qa;
        if (!(end_b <= T)) B.list[P.first_query + atomicAdd(B.count, 1u)] = qb;
    }
}

}  // namespace poa_amd
