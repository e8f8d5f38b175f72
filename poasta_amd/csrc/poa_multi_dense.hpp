// Dense multi-graph batches (poa_multi_*_dense) for gfx950: the packed-u16 forward pass of poa_forward_packed.hpp and the walk of
// poa_kernels.hpp over the queries of many graphs in one launch each.  One wavefront per query in both
// launches, four waves per block; nothing is ordered between waves, so the four waves of a block may belong to four graphs.
//
// What a single-graph dense launch passes as its kernel arguments, FwdParams and TbParams, lies here once per listed graph in
// a device array (MultiDenseBlock).  A wave reads its query's graph id, copies that graph's FwdParams (forward launch) or
// TbParams (traceback launch) and patches what belongs to the launch: the chunk, the costs, the speculation depth.  The
// wave's query index and the graph id go through readfirstlane (wave_uni), as in multi_load (poa_multi.hpp): the block's
// address is then a scalar, the copy a run of scalar loads into SGPRs, and every table pointer and row count stays as uniform
// as a kernel argument is.  The walk IS the single-graph one: traceback_wave<uint16_t, true, 64> takes `const TbParams&`.
//
// The forward rows are forward_packed_strip<Q> below: the row loop of poa_forward_packed_kernel<Q, false, false> for a query
// that is ONE strip (pitch <= 512 Q columns; the plan refuses longer queries), written against `const FwdParams&`.  It is that
// kernel's code with everything a second strip or a second wave needs taken out (strip carries, the LDS hand-over ring, the
// fused walk) and nothing else changed: the same packed primitives (pk_*, wave_scan_min_plus16 of poa_forward_packed.hpp), the
// same statements in the same order, the same plane layout and codes — the single-graph kernel's file itself stays as it is,
// because bench.py ties the committed PMC counters to its hash (forward_kernel_source_hash).  Of its graph the body reads
// rows, pred_rows, n_rows, d_slot and pred_dslot.  tests/test_multi_dense.py compares every result with the single-graph pass.
//
// A batch created with POA_CFG_WIDE_QUERIES also holds queries wider than one strip.  A chunk with such a query runs
// poa_forward_packed_multi_wide_kernel over forward_packed_strips<2>: that kernel's strip loop for one wave (S == 1), the carries
// of a query at its own offset into the chunk's carry buffer (MultiPlan::carry_off).  Every other chunk launches what it
// launches without the flag.  The walk is unchanged: traceback_wave walks planes of any pitch.
//
// One walk per wave.  The single-graph launcher also runs 32 or 16 lanes per walk (plan_dense_chunk); here a narrower group
// would put queries of different graphs into one wave and make the block's pointers divergent.  Out of scope.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_forward_packed.hpp"
#include "poa_forward_sweep.hpp"

namespace poa_amd {

struct MultiDenseBlock {
    FwdParams F;           // first_query, n_queries and the costs are patched per wave
    TbParams T;            // the same, and spec_depth / code_fmt
    uint32_t empty;        // the graph has no real nodes: score 4 * len, POA_FLAG_EMPTY_GRAPH, no pairs (PoastaAligner::align, mod.rs:124-142)
    uint32_t pad;
};
static_assert(sizeof(MultiDenseBlock) == sizeof(FwdParams) + sizeof(TbParams) + 8, "a block is F, T, then empty and pad: what the host fills and uploads");

struct MultiDenseLaunch {
    const MultiDenseBlock* graphs;    // [n_graphs]
    const uint32_t* graph_of;         // [total] graph of a query
    uint32_t first_query, n_queries;  // the chunk
    uint32_t cost_x, cost_o, cost_e;
    uint32_t spec_depth, code_fmt;    // of the walk; code_fmt 0: one nibble per cell, what the packed kernel stores
    // read by poa_forward_packed_multi_wide_kernel alone
    uint32_t* carry;                  // the chunk's strip carries
    const uint32_t* carry_off;        // [total] words from `carry`, relative to the query's chunk (MultiPlan::carry_off)
};

// the wave's query and its graph's block; nullptr: no query for this wave
__device__ __forceinline__ const MultiDenseBlock* multi_dense_block(const MultiDenseLaunch& A, uint32_t& wq) {
    wq = wave_uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wq >= A.n_queries) return nullptr;
    const uint32_t gid = wave_uni(A.graph_of[A.first_query + wq]);
    return A.graphs + gid;
}

// All rows of query qi, a query of one strip (P.pitch[qi] <= 512 * Q): see the head of this file.  The comments of
// poa_forward_packed_kernel apply; the row's names are its names.
template <int Q>
__device__ __forceinline__ void forward_packed_strip(const FwdParams& P, const uint32_t qi, const uint32_t lane) {
    constexpr int K = 8;                 // columns per lane and quad
    constexpr int NP = 4 * Q;            // packed registers per row array (2 columns each)
    constexpr uint32_t QW = 64 * K;      // 512 columns per quad
    constexpr uint32_t I16 = 0xFFFFu, INF2 = 0xFFFFFFFFu;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    const uint8_t* __restrict__ q = P.qseq + qbeg;
    const uint32_t pitch = P.pitch[qi];
    const uint64_t RP = (uint64_t)P.n_rows * pitch;
    uint16_t* __restrict__ Mp = reinterpret_cast<uint16_t*>(P.planes) + P.plane_off[qi];
    uint16_t* __restrict__ Ip = Mp + RP;  // holds the 4-bit codes (a quarter plane)
    uint16_t* __restrict__ Dp = Ip + RP / 4;  // the kept D rows, row r at slot d_slot[r] (compact_plane_elems)
    const uint32_t e = P.cost_e, oe = P.cost_oe, x = P.cost_x;
    const uint32_t e2 = e | (e << 16), oe2 = oe | (oe << 16), x2 = x | (x << 16);
    const uint32_t step = K * e;
    const uint32_t w15 = ((lane & 15u) + 1u) * step;
    const uint32_t w31 = (lane - 31u) * step;
    const uint32_t lane_off = K * lane * e;
    uint32_t off2[4];  // cost of extending an insertion from my first column of a quad to columns 2i, 2i+1
#pragma unroll
    for (int i = 0; i < 4; ++i) off2[i] = (2 * i * e) | ((2 * i + 1) * e << 16);
    const uint32_t inf2 = INF2;

    bool act[Q];
    uint32_t qP[NP];   // my query symbols, 16 bits each (0 past the end: never a symbol)
    uint32_t qlE[Q];   // symbol left of my first column of quad m, in the HIGH half
#pragma unroll
    for (int m = 0; m < Q; ++m) {
        const uint32_t c0 = m * QW + K * lane;
        act[m] = c0 < pitch;
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {
            const uint32_t c = c0 + 2 * pp;
            const uint32_t lo = (c < L) ? (uint32_t)q[c] : 0u, hi = (c + 1 < L) ? (uint32_t)q[c + 1] : 0u;
            qP[4 * m + pp] = lo | (hi << 16);
        }
        qlE[m] = ((c0 > 0 && c0 - 1 < L) ? (uint32_t)q[c0 - 1] : 0u) << 16;
    }
    uint32_t Mprev[NP], Dprev[NP];
    uint32_t PMc[NP], PDc[NP], PMlc[Q];  // predecessor minima of the last multi-predecessor row (ROW_SAME_PREDS reuses them)
#pragma unroll
    for (int p = 0; p < NP; ++p) { Mprev[p] = inf2; Dprev[p] = inf2; PMc[p] = inf2; PDc[p] = inf2; }
#pragma unroll
    for (int m = 0; m < Q; ++m) PMlc[m] = inf2;

    for (uint32_t r = 0; r < P.n_rows; ++r) {
        const RowMeta meta = P.rows[r];
        const uint32_t sym = meta.sym;
        const uint32_t sym2 = sym | (sym << 16);
        const uint64_t rbase = (uint64_t)r * pitch + K * lane;
        uint32_t PMl[Q];  // hi half = min over predecessors of M[p][my first column - 1]
        // the row itself, given the predecessor minima PM / PD; the chain path passes the previous row's registers themselves
        auto row_body = [&](const uint32_t (&PM)[NP], const uint32_t (&PD)[NP]) {
            uint32_t Mc[NP], Ic[NP], Dc[NP], Hc[NP], PDe[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) PDe[p] = pk_add_sat(PD[p], e2);
            if (meta.flags & ROW_END) {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    Dc[p] = PDe[p];
                    Mc[p] = pk_min(PM[p], Dc[p]);
                    Ic[p] = inf2;
                    Hc[p] = Mc[p];
                }
            } else {
                // insertion-open rule, branch-free: "always" == the child symbol 0, which no query symbol equals
                const uint32_t cs1 = (meta.flags & ROW_OPENI_ALWAYS) ? 0u : (uint32_t)meta.child_sym;
                const uint32_t csym2 = cs1 | (cs1 << 16);
                const uint32_t start_keep = ((meta.flags & ROW_START) && lane == 0) ? 0xFFFF0000u : 0xFFFFFFFFu;
                uint32_t Tq[Q];
#pragma unroll
                for (int m = 0; m < Q; ++m) {
                    uint32_t eq_prev = ((qlE[m] >> 16) == sym) ? 0x00010000u : 0u;  // does the column left of the quad match? (hi half)
                    uint32_t pm_prev = PMl[m];
                    uint32_t t = I16;  // in-lane insertion chain (32-bit scalar in the 16-bit domain)
                    uint32_t iloc[4];
#pragma unroll
                    for (int pp = 0; pp < 4; ++pp) {
                        const int p = 4 * m + pp;
                        const uint32_t eq1 = pk_is_zero(qP[p] ^ sym2);  // 1 where the query symbol equals the row's symbol
                        // D: open a deletion only where the symbols differ (or past the query end, where q is 0)
                        Dc[p] = pk_min(PDe[p], pk_inf_where(pk_add_sat(PM[p], oe2), eq1));
                        const uint32_t pm_s = shr_col(PM[p], pm_prev);  // M of the predecessor(s), one column to the left
                        const uint32_t eq_s = shr_col(eq1, eq_prev);
                        // (mis)match from the left column: + x where the symbols differ (x - (eq << 8) saturates to 0 on a match)
                        Hc[p] = pk_min(pk_add_sat(pm_s, pk_sub_sat(x2, pk_shl<8>(eq_s))), Dc[p]);
                        pm_prev = PM[p]; eq_prev = eq1;
                        if (m == 0 && pp == 0) Hc[p] &= start_keep;  // H[start][0] = 0
                        // insertion open: A = (q != child symbol) ? H + oe : INF
                        const uint32_t a = pk_inf_where(pk_add_sat(Hc[p], oe2), pk_is_zero(qP[p] ^ csym2));
                        const uint32_t a_lo = a & 0xFFFFu, a_hi = a >> 16;
                        const uint32_t i_lo = t;
                        t = umin3(t + e, a_lo, I16);
                        iloc[pp] = i_lo | (t << 16);
                        t = umin3(t + e, a_hi, I16);
                    }
                    Tq[m] = t;
#pragma unroll
                    for (int pp = 0; pp < 4; ++pp) Ic[4 * m + pp] = iloc[pp];
                }
                uint32_t cq = I16;   // nothing enters the one strip from the left
#pragma unroll
                for (int m = 0; m < Q; ++m) {
                    const uint32_t Pm = wave_scan_min_plus16(Tq[m], step, w15, w31);
                    const uint32_t excl = wave_shr1(Pm, I16);
                    const uint32_t cin = umin3(excl, cq + lane_off, I16);
                    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)Pm, 63);
                    cq = umin3(cq + QW * e, total, I16);
                    const uint32_t cin2 = cin | (cin << 16);
#pragma unroll
                    for (int pp = 0; pp < 4; ++pp) Ic[4 * m + pp] = pk_min(Ic[4 * m + pp], pk_add_sat(cin2, off2[pp]));
                }
#pragma unroll
                for (int p = 0; p < NP; ++p) Mc[p] = pk_min(Hc[p], Ic[p]);
            }

            // 4-bit codes (bit set == predicate holds): I==M, I[j]==I[j-1]+e, D==M, D==PD+e; 8 cells per dword, the
            // nibble of my column k at position (k >> 1) + 4 * (k & 1)  (decoder: tb_code)
            uint32_t* __restrict__ codes = reinterpret_cast<uint32_t*>(Ip) + (uint64_t)r * (pitch / 8) + lane;
            const bool keep_d = (meta.flags & ROW_STORE_D) != 0;
            uint32_t edge_i = inf2;
#pragma unroll
            for (int m = 0; m < Q; ++m) {
                uint32_t i_prev = pk_wave_shr1(Ic[4 * m + 3], edge_i);
                edge_i = (uint32_t)__builtin_amdgcn_readlane((int)Ic[4 * m + 3], 63);
                uint32_t fA = 0, fB = 0, fC = 0, fD = 0;  // flag of pair pp at bit 4*pp (even column) and 16 + 4*pp (odd column)
#pragma unroll
                for (int pp = 0; pp < 4; ++pp) {
                    const int p = 4 * m + pp;
                    const uint32_t i_left = shr_col(Ic[p], i_prev);
                    i_prev = Ic[p];
                    // equality flags (0/1 per half); in every pair below lhs >= rhs holds by construction
                    fA |= pk_eq_ge(Ic[p], Mc[p]) << (4 * pp);                           // I == M   (M = min(H, I) <= I)
                    fB |= pk_eq_ge(pk_add_sat(i_left, e2), Ic[p]) << (4 * pp);          // I[j] == I[j-1] + e
                    fC |= pk_eq_ge(Dc[p], Mc[p]) << (4 * pp);                           // D == M   (M <= H <= D)
                    fD |= pk_eq_ge(PDe[p], Dc[p]) << (4 * pp);                          // D == PD + e
                }
                const uint32_t word = fA | (fB << 1) | (fC << 2) | (fD << 3);
                if (act[m]) {
                    *reinterpret_cast<uint4*>(Mp + rbase + m * QW) = make_uint4(Mc[4 * m], Mc[4 * m + 1], Mc[4 * m + 2], Mc[4 * m + 3]);
                    if (keep_d)
                        *reinterpret_cast<uint4*>(Dp + (uint64_t)(P.d_slot ? P.d_slot[r] : r) * pitch + K * lane + m * QW) = make_uint4(Dc[4 * m], Dc[4 * m + 1], Dc[4 * m + 2], Dc[4 * m + 3]);
                    codes[m * (QW / 8)] = word;
                }
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) { Mprev[p] = Mc[p]; Dprev[p] = Dc[p]; }
        };

        if (meta.flags & ROW_CHAIN) {
            uint32_t edge = inf2;
#pragma unroll
            for (int m = 0; m < Q; ++m) {
                PMl[m] = pk_wave_shr1(Mprev[4 * m + 3], edge);
                edge = (uint32_t)__builtin_amdgcn_readlane((int)Mprev[4 * m + 3], 63);
            }
            row_body(Mprev, Dprev);
        } else if (meta.flags & ROW_SAME_PREDS) {
            // a sibling of the previous row (same predecessor set): its predecessor minima are still in registers
#pragma unroll
            for (int m = 0; m < Q; ++m) PMl[m] = PMlc[m];
            row_body(PMc, PDc);
        } else {
            uint32_t (&PM)[NP] = PMc;
            uint32_t (&PD)[NP] = PDc;
#pragma unroll
            for (int p = 0; p < NP; ++p) { PM[p] = inf2; PD[p] = inf2; }
#pragma unroll
            for (int m = 0; m < Q; ++m) PMl[m] = inf2;
            // I read back rows this wave stored itself: wavefront scope orders that
            if (meta.pred_count > 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            // Predecessors in batches of PB: all row indices first (scalar loads), then every plane load of the batch, then the
            // reduction — one memory round-trip per batch instead of two per predecessor
            constexpr int PB = Q == 1 ? 4 : 2;
            const CPredRows* cpred = (const CPredRows*)P.pred_rows + meta.pred_begin;
            const CPredRows* cpslot = (const CPredRows*)P.pred_dslot + meta.pred_begin;
            for (uint32_t pe0 = 0; pe0 < meta.pred_count; pe0 += PB) {
                uint32_t prs[PB];
                bool valid[PB], in_regs[PB];
#pragma unroll
                for (int b = 0; b < PB; ++b) {
                    valid[b] = pe0 + b < meta.pred_count;
                    prs[b] = valid[b] ? cpred[pe0 + b] : 0u;
                    in_regs[b] = prs[b] + 1 == r;  // the previous row is still in registers
                }
                uint4 la[PB][Q], lb[PB][Q];
#pragma unroll
                for (int b = 0; b < PB; ++b) {
                    const uint64_t pbase = (uint64_t)prs[b] * pitch + K * lane;
                    const uint64_t pbase_d = P.pred_dslot ? (uint64_t)(valid[b] ? cpslot[pe0 + b] : 0u) * pitch + K * lane : pbase;
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        la[b][m] = make_uint4(inf2, inf2, inf2, inf2); lb[b][m] = la[b][m];
                        if (valid[b] && !in_regs[b] && act[m]) {
                            la[b][m] = *reinterpret_cast<const uint4*>(Mp + pbase + m * QW);
                            lb[b][m] = *reinterpret_cast<const uint4*>(Dp + pbase_d + m * QW);
                        }
                    }
                }
#pragma unroll
                for (int b = 0; b < PB; ++b) {
                    if (!valid[b]) continue;
                    uint32_t tm[NP], td[NP];
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        tm[4 * m] = la[b][m].x; tm[4 * m + 1] = la[b][m].y; tm[4 * m + 2] = la[b][m].z; tm[4 * m + 3] = la[b][m].w;
                        td[4 * m] = lb[b][m].x; td[4 * m + 1] = lb[b][m].y; td[4 * m + 2] = lb[b][m].z; td[4 * m + 3] = lb[b][m].w;
                    }
                    if (in_regs[b]) {
#pragma unroll
                        for (int p = 0; p < NP; ++p) { tm[p] = Mprev[p]; td[p] = Dprev[p]; }
                    }
                    uint32_t edge = inf2;   // the column left of the one strip does not exist
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        PMl[m] = pk_min(PMl[m], pk_wave_shr1(tm[4 * m + 3], edge));
                        edge = (uint32_t)__builtin_amdgcn_readlane((int)tm[4 * m + 3], 63);
                    }
#pragma unroll
                    for (int p = 0; p < NP; ++p) { PM[p] = pk_min(PM[p], tm[p]); PD[p] = pk_min(PD[p], td[p]); }
                }
            }
#pragma unroll
            for (int m = 0; m < Q; ++m) PMlc[m] = PMl[m];
            row_body(PM, PD);
        }
    }
}

// All rows of query qi, strip by strip: a query of any pitch (POA_CFG_WIDE_QUERIES).  The strip loop of
// poa_forward_packed_kernel<Q, false, false> with S == 1 (one wave per query, its strips in sequence), written against
// `const FwdParams&`: that kernel's from_global / to_global paths with the MW ring, the progress counters and the fused walk
// taken out, the same statements in the same order.  What strip s needs from strip s - 1 for row r:
//   carry[2r]      the insertion-scan carry leaving strip s - 1 (lane 0 stores it)
//   carry[2r + 1]  I of its last column, for code bit B of my first column (lane 63 stores it)
//   M of its last column (the diagonal edge): read back from the stored plane, column sbase - 1 of the predecessor rows, of the
//                  previous row on a chain row
// `carry` is the query's own 2 x n_rows words (the caller's scalar pointer); one parity is enough, the wave reads a row's words
// before it overwrites them.  A query of one strip runs n_strips == 1 and touches no carry word.  The fences are that kernel's:
// a strip reads what the same wave stored in the strip before (carry words, the M edge column, the kept D rows).
template <int Q>
__device__ __forceinline__ void forward_packed_strips(const FwdParams& P, const uint32_t qi, const uint32_t lane) {
    constexpr int K = 8;                 // columns per lane and quad
    constexpr int NP = 4 * Q;            // packed registers per row array (2 columns each)
    constexpr uint32_t QW = 64 * K;      // 512 columns per quad
    constexpr uint32_t W = QW * Q;
    constexpr uint32_t I16 = 0xFFFFu, INF2 = 0xFFFFFFFFu;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    const uint8_t* __restrict__ q = P.qseq + qbeg;
    const uint32_t pitch = P.pitch[qi];
    const uint64_t RP = (uint64_t)P.n_rows * pitch;
    uint16_t* __restrict__ Mp = reinterpret_cast<uint16_t*>(P.planes) + P.plane_off[qi];
    uint16_t* __restrict__ Ip = Mp + RP;  // holds the 4-bit codes (a quarter plane)
    uint16_t* __restrict__ Dp = Ip + RP / 4;  // the kept D rows, row r at slot d_slot[r] (compact_plane_elems)
    uint32_t* __restrict__ carry = P.strip_carry;
    const uint32_t e = P.cost_e, oe = P.cost_oe, x = P.cost_x;
    const uint32_t e2 = e | (e << 16), oe2 = oe | (oe << 16), x2 = x | (x << 16);
    const uint32_t n_strips = wave_uni((pitch + W - 1) / W);
    const uint32_t step = K * e;
    const uint32_t w15 = ((lane & 15u) + 1u) * step;
    const uint32_t w31 = (lane - 31u) * step;
    const uint32_t lane_off = K * lane * e;
    uint32_t off2[4];  // cost of extending an insertion from my first column of a quad to columns 2i, 2i+1
#pragma unroll
    for (int i = 0; i < 4; ++i) off2[i] = (2 * i * e) | ((2 * i + 1) * e << 16);
    const uint32_t inf2 = INF2;

    for (uint32_t s = 0; s < n_strips; ++s) {
        const bool from_global = s > 0;                 // strip s - 1 was finished earlier (carry array + planes)
        const bool to_global = s + 1 < n_strips;
        const uint32_t sbase = s * W;
        bool act[Q];
        uint32_t qP[NP];   // my query symbols, 16 bits each (0 past the end: never a symbol)
        uint32_t qlE[Q];   // symbol left of my first column of quad m, in the HIGH half
#pragma unroll
        for (int m = 0; m < Q; ++m) {
            const uint32_t c0 = sbase + m * QW + K * lane;
            act[m] = c0 < pitch;
#pragma unroll
            for (int pp = 0; pp < 4; ++pp) {
                const uint32_t c = c0 + 2 * pp;
                const uint32_t lo = (c < L) ? (uint32_t)q[c] : 0u, hi = (c + 1 < L) ? (uint32_t)q[c + 1] : 0u;
                qP[4 * m + pp] = lo | (hi << 16);
            }
            qlE[m] = ((c0 > 0 && c0 - 1 < L) ? (uint32_t)q[c0 - 1] : 0u) << 16;
        }
        uint32_t Mprev[NP], Dprev[NP];
        uint32_t PMc[NP], PDc[NP], PMlc[Q];  // predecessor minima of the last multi-predecessor row (ROW_SAME_PREDS reuses them)
#pragma unroll
        for (int p = 0; p < NP; ++p) { Mprev[p] = inf2; Dprev[p] = inf2; PMc[p] = inf2; PDc[p] = inf2; }
#pragma unroll
        for (int m = 0; m < Q; ++m) PMlc[m] = inf2;

        for (uint32_t r = 0; r < P.n_rows; ++r) {
            const RowMeta meta = P.rows[r];
            const uint32_t sym = meta.sym;
            const uint32_t sym2 = sym | (sym << 16);
            const uint64_t rbase = (uint64_t)r * pitch + sbase + K * lane;
            uint32_t PMl[Q];  // hi half = min over predecessors of M[p][my first column - 1]
            // the row itself, given the predecessor minima PM / PD; the chain path passes the previous row's registers themselves
            auto row_body = [&](const uint32_t (&PM)[NP], const uint32_t (&PD)[NP]) {
                uint32_t Mc[NP], Ic[NP], Dc[NP], Hc[NP], PDe[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) PDe[p] = pk_add_sat(PD[p], e2);
                if (meta.flags & ROW_END) {
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        Dc[p] = PDe[p];
                        Mc[p] = pk_min(PM[p], Dc[p]);
                        Ic[p] = inf2;
                        Hc[p] = Mc[p];
                    }
                } else {
                    // insertion-open rule, branch-free: "always" == the child symbol 0, which no query symbol equals
                    const uint32_t cs1 = (meta.flags & ROW_OPENI_ALWAYS) ? 0u : (uint32_t)meta.child_sym;
                    const uint32_t csym2 = cs1 | (cs1 << 16);
                    const uint32_t start_keep = ((meta.flags & ROW_START) && sbase == 0 && lane == 0) ? 0xFFFF0000u : 0xFFFFFFFFu;
                    uint32_t Tq[Q];
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        uint32_t eq_prev = ((qlE[m] >> 16) == sym) ? 0x00010000u : 0u;  // does the column left of the quad match? (hi half)
                        uint32_t pm_prev = PMl[m];
                        uint32_t t = I16;  // in-lane insertion chain (32-bit scalar in the 16-bit domain)
                        uint32_t iloc[4];
#pragma unroll
                        for (int pp = 0; pp < 4; ++pp) {
                            const int p = 4 * m + pp;
                            const uint32_t eq1 = pk_is_zero(qP[p] ^ sym2);  // 1 where the query symbol equals the row's symbol
                            // D: open a deletion only where the symbols differ (or past the query end, where q is 0)
                            Dc[p] = pk_min(PDe[p], pk_inf_where(pk_add_sat(PM[p], oe2), eq1));
                            const uint32_t pm_s = shr_col(PM[p], pm_prev);  // M of the predecessor(s), one column to the left
                            const uint32_t eq_s = shr_col(eq1, eq_prev);
                            // (mis)match from the left column: + x where the symbols differ (x - (eq << 8) saturates to 0 on a match)
                            Hc[p] = pk_min(pk_add_sat(pm_s, pk_sub_sat(x2, pk_shl<8>(eq_s))), Dc[p]);
                            pm_prev = PM[p]; eq_prev = eq1;
                            if (m == 0 && pp == 0) Hc[p] &= start_keep;  // H[start][0] = 0
                            // insertion open: A = (q != child symbol) ? H + oe : INF
                            const uint32_t a = pk_inf_where(pk_add_sat(Hc[p], oe2), pk_is_zero(qP[p] ^ csym2));
                            const uint32_t a_lo = a & 0xFFFFu, a_hi = a >> 16;
                            const uint32_t i_lo = t;
                            t = umin3(t + e, a_lo, I16);
                            iloc[pp] = i_lo | (t << 16);
                            t = umin3(t + e, a_hi, I16);
                        }
                        Tq[m] = t;
#pragma unroll
                        for (int pp = 0; pp < 4; ++pp) Ic[4 * m + pp] = iloc[pp];
                    }
                    uint32_t cq = from_global ? carry[2 * r] : I16;
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        const uint32_t Pm = wave_scan_min_plus16(Tq[m], step, w15, w31);
                        const uint32_t excl = wave_shr1(Pm, I16);
                        const uint32_t cin = umin3(excl, cq + lane_off, I16);
                        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)Pm, 63);
                        cq = umin3(cq + QW * e, total, I16);
                        const uint32_t cin2 = cin | (cin << 16);
#pragma unroll
                        for (int pp = 0; pp < 4; ++pp) Ic[4 * m + pp] = pk_min(Ic[4 * m + pp], pk_add_sat(cin2, off2[pp]));
                    }
                    if (to_global && lane == 0) carry[2 * r] = cq;
#pragma unroll
                    for (int p = 0; p < NP; ++p) Mc[p] = pk_min(Hc[p], Ic[p]);
                }

                // 4-bit codes (bit set == predicate holds): I==M, I[j]==I[j-1]+e, D==M, D==PD+e; 8 cells per dword, the
                // nibble of my column k at position (k >> 1) + 4 * (k & 1)  (decoder: tb_code)
                uint32_t* __restrict__ codes = reinterpret_cast<uint32_t*>(Ip) + (uint64_t)r * (pitch / 8) + sbase / 8 + lane;
                const bool keep_d = (meta.flags & ROW_STORE_D) != 0;
                uint32_t edge_i = inf2;
                if (from_global) edge_i = carry[2 * r + 1] << 16;
#pragma unroll
                for (int m = 0; m < Q; ++m) {
                    uint32_t i_prev = pk_wave_shr1(Ic[4 * m + 3], edge_i);
                    edge_i = (uint32_t)__builtin_amdgcn_readlane((int)Ic[4 * m + 3], 63);
                    uint32_t fA = 0, fB = 0, fC = 0, fD = 0;  // flag of pair pp at bit 4*pp (even column) and 16 + 4*pp (odd column)
#pragma unroll
                    for (int pp = 0; pp < 4; ++pp) {
                        const int p = 4 * m + pp;
                        const uint32_t i_left = shr_col(Ic[p], i_prev);
                        i_prev = Ic[p];
                        // equality flags (0/1 per half); in every pair below lhs >= rhs holds by construction
                        fA |= pk_eq_ge(Ic[p], Mc[p]) << (4 * pp);                           // I == M   (M = min(H, I) <= I)
                        fB |= pk_eq_ge(pk_add_sat(i_left, e2), Ic[p]) << (4 * pp);          // I[j] == I[j-1] + e
                        fC |= pk_eq_ge(Dc[p], Mc[p]) << (4 * pp);                           // D == M   (M <= H <= D)
                        fD |= pk_eq_ge(PDe[p], Dc[p]) << (4 * pp);                          // D == PD + e
                    }
                    const uint32_t word = fA | (fB << 1) | (fC << 2) | (fD << 3);
                    if (act[m]) {
                        *reinterpret_cast<uint4*>(Mp + rbase + m * QW) = make_uint4(Mc[4 * m], Mc[4 * m + 1], Mc[4 * m + 2], Mc[4 * m + 3]);
                        if (keep_d)
                            *reinterpret_cast<uint4*>(Dp + (uint64_t)(P.d_slot ? P.d_slot[r] : r) * pitch + sbase + K * lane + m * QW) = make_uint4(Dc[4 * m], Dc[4 * m + 1], Dc[4 * m + 2], Dc[4 * m + 3]);
                        codes[m * (QW / 8)] = word;
                    }
                }
                if (to_global && lane == 63) carry[2 * r + 1] = Ic[NP - 1] >> 16;
#pragma unroll
                for (int p = 0; p < NP; ++p) { Mprev[p] = Mc[p]; Dprev[p] = Dc[p]; }
            };

            if (meta.flags & ROW_CHAIN) {
                uint32_t edge = inf2;
                if (from_global) edge = (uint32_t)Mp[(uint64_t)(r - 1) * pitch + sbase - 1] << 16;
#pragma unroll
                for (int m = 0; m < Q; ++m) {
                    PMl[m] = pk_wave_shr1(Mprev[4 * m + 3], edge);
                    edge = (uint32_t)__builtin_amdgcn_readlane((int)Mprev[4 * m + 3], 63);
                }
                row_body(Mprev, Dprev);
            } else if (meta.flags & ROW_SAME_PREDS) {
                // a sibling of the previous row (same predecessor set): its predecessor minima are still in registers
#pragma unroll
                for (int m = 0; m < Q; ++m) PMl[m] = PMlc[m];
                row_body(PMc, PDc);
            } else {
                uint32_t (&PM)[NP] = PMc;
                uint32_t (&PD)[NP] = PDc;
#pragma unroll
                for (int p = 0; p < NP; ++p) { PM[p] = inf2; PD[p] = inf2; }
#pragma unroll
                for (int m = 0; m < Q; ++m) PMl[m] = inf2;
                // I read back rows this wave stored itself: wavefront scope orders that
                if (meta.pred_count > 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                // Predecessors in batches of PB: all row indices first (scalar loads), then every plane load of the batch, then the
                // reduction — one memory round-trip per batch instead of two per predecessor
                constexpr int PB = Q == 1 ? 4 : 2;
                const CPredRows* cpred = (const CPredRows*)P.pred_rows + meta.pred_begin;
                const CPredRows* cpslot = (const CPredRows*)P.pred_dslot + meta.pred_begin;
                for (uint32_t pe0 = 0; pe0 < meta.pred_count; pe0 += PB) {
                    uint32_t prs[PB];
                    bool valid[PB], in_regs[PB];
#pragma unroll
                    for (int b = 0; b < PB; ++b) {
                        valid[b] = pe0 + b < meta.pred_count;
                        prs[b] = valid[b] ? cpred[pe0 + b] : 0u;
                        in_regs[b] = prs[b] + 1 == r;  // the previous row is still in registers
                    }
                    uint4 la[PB][Q], lb[PB][Q];
                    uint32_t edges[PB];
#pragma unroll
                    for (int b = 0; b < PB; ++b) {
                        const uint64_t pbase = (uint64_t)prs[b] * pitch + sbase + K * lane;
                        const uint64_t pbase_d = P.pred_dslot ? (uint64_t)(valid[b] ? cpslot[pe0 + b] : 0u) * pitch + sbase + K * lane : pbase;
#pragma unroll
                        for (int m = 0; m < Q; ++m) {
                            la[b][m] = make_uint4(inf2, inf2, inf2, inf2); lb[b][m] = la[b][m];
                            if (valid[b] && !in_regs[b] && act[m]) {
                                la[b][m] = *reinterpret_cast<const uint4*>(Mp + pbase + m * QW);
                                lb[b][m] = *reinterpret_cast<const uint4*>(Dp + pbase_d + m * QW);
                            }
                        }
                        edges[b] = inf2;
                        if (valid[b] && s > 0) edges[b] = (uint32_t)Mp[(uint64_t)prs[b] * pitch + sbase - 1] << 16;
                    }
#pragma unroll
                    for (int b = 0; b < PB; ++b) {
                        if (!valid[b]) continue;
                        uint32_t tm[NP], td[NP];
#pragma unroll
                        for (int m = 0; m < Q; ++m) {
                            tm[4 * m] = la[b][m].x; tm[4 * m + 1] = la[b][m].y; tm[4 * m + 2] = la[b][m].z; tm[4 * m + 3] = la[b][m].w;
                            td[4 * m] = lb[b][m].x; td[4 * m + 1] = lb[b][m].y; td[4 * m + 2] = lb[b][m].z; td[4 * m + 3] = lb[b][m].w;
                        }
                        if (in_regs[b]) {
#pragma unroll
                            for (int p = 0; p < NP; ++p) { tm[p] = Mprev[p]; td[p] = Dprev[p]; }
                        }
                        uint32_t edge = edges[b];
#pragma unroll
                        for (int m = 0; m < Q; ++m) {
                            PMl[m] = pk_min(PMl[m], pk_wave_shr1(tm[4 * m + 3], edge));
                            edge = (uint32_t)__builtin_amdgcn_readlane((int)tm[4 * m + 3], 63);
                        }
#pragma unroll
                        for (int p = 0; p < NP; ++p) { PM[p] = pk_min(PM[p], tm[p]); PD[p] = pk_min(PD[p], td[p]); }
                    }
                }
#pragma unroll
                for (int m = 0; m < Q; ++m) PMlc[m] = PMl[m];
                row_body(PM, PD);
            }
        }
        // the next strip reads what I stored in this one: its carry words, the M edge column, the kept D rows
        if (n_strips > 1) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
}

template <int Q>
__global__ __launch_bounds__(256) void poa_forward_packed_multi_kernel(MultiDenseLaunch A) {
    uint32_t wq;
    const MultiDenseBlock* __restrict__ gp = multi_dense_block(A, wq);
    if (!gp) return;
    if (gp->empty) {
        const uint32_t qi = A.first_query + wq;
        const TbParams& T = gp->T;
        const uint32_t L = (uint32_t)(T.qoff[qi + 1] - T.qoff[qi]);
        if ((threadIdx.x & 63u) == 0) { T.score[qi] = L * 4u; T.flags[qi] = POA_FLAG_EMPTY_GRAPH; T.n_pairs[qi] = 0; }
        return;
    }
    FwdParams P = gp->F;
    P.first_query = A.first_query; P.n_queries = A.n_queries;
    P.cost_x = A.cost_x; P.cost_oe = A.cost_o + A.cost_e; P.cost_e = A.cost_e;
    P.cost_de = P.cost_ie = P.cost_e; P.cost_doe = P.cost_ioe = P.cost_oe;   // absolute encoding
    forward_packed_strip<Q>(P, A.first_query + wq, threadIdx.x & 63u);
}

// A chunk with a query wider than one strip (POA_CFG_WIDE_QUERIES): every wave runs the strip loop, a query of one strip as
// n_strips == 1.  The wave's carry words lie at A.carry + A.carry_off[qi] (relative to the chunk: the buffer holds the largest
// chunk's), and the body sees them as the carry of query index 0, the way poa_multi.hpp treats P.carry with wq = 0.
__global__ __launch_bounds__(256) void poa_forward_packed_multi_wide_kernel(MultiDenseLaunch A) {
    uint32_t wq;
    const MultiDenseBlock* __restrict__ gp = multi_dense_block(A, wq);
    if (!gp) return;
    const uint32_t qi = A.first_query + wq;
    if (gp->empty) {
        const TbParams& T = gp->T;
        const uint32_t L = (uint32_t)(T.qoff[qi + 1] - T.qoff[qi]);
        if ((threadIdx.x & 63u) == 0) { T.score[qi] = L * 4u; T.flags[qi] = POA_FLAG_EMPTY_GRAPH; T.n_pairs[qi] = 0; }
        return;
    }
    FwdParams P = gp->F;
    P.first_query = A.first_query; P.n_queries = A.n_queries;
    P.cost_x = A.cost_x; P.cost_oe = A.cost_o + A.cost_e; P.cost_e = A.cost_e;
    P.cost_de = P.cost_ie = P.cost_e; P.cost_doe = P.cost_ioe = P.cost_oe;   // absolute encoding
    P.strip_carry = A.carry + wave_uni(A.carry_off[qi]);
    forward_packed_strips<2>(P, qi, threadIdx.x & 63u);
}

__global__ __launch_bounds__(256) void poa_traceback_multi_kernel(MultiDenseLaunch A) {
    uint32_t wq;
    const MultiDenseBlock* __restrict__ gp = multi_dense_block(A, wq);
    if (!gp) return;
    if (gp->empty) return;   // the forward pass wrote the result
    TbParams P = gp->T;
    P.first_query = A.first_query; P.n_queries = A.n_queries;
    P.cost_x = A.cost_x; P.cost_o = A.cost_o; P.cost_e = A.cost_e;
    P.spec_depth = A.spec_depth; P.code_fmt = A.code_fmt;
    traceback_wave<uint16_t, true, 64>(P, A.first_query + wq, threadIdx.x & 63u);
}

}  // namespace poa_amd
