// Score-only forward sweep (POA_MODE_SCORE) for gfx950: the recurrences of the dense forward pass (poa_kernels.hpp, DESIGN.md
// §2) with nothing kept but the rows some later row still reads, and one output per query: M[end row][len].
//
// Memory of a query: n_slots x pitch cells of M and of D, addressed by SLOT (poa_sweep_rows.hpp), not by row.  A row without a
// slot stores nothing — in a chain-like graph that is almost every row — and the I values never leave the row.  No traceback
// flag of any kind is computed.  One wavefront per query.
//
// Slot reuse, and why it needs no ordering between waves.  A slot is written by a row and overwritten by a later row once
// the first one's last reader has run.  Both kernels here keep a query inside ONE wave from its first row to its last:
//   * poa_sweep_px_kernel handles queries of one strip (pitch <= 1024);
//   * poa_sweep_kernel walks the strips of a longer query one after the other in the same wave.  A strip reads and writes only
//     its own column range of a slot, so the reuse of a slot by strip s never meets what strip s + 1 will read there: what
//     crosses a strip boundary — the insertion value entering the next strip and the M value of the strip's last column —
//     goes through a per-row carry array, as in the dense kernels, double-buffered by strip parity because the carries of
//     strip s are read during the whole of strip s + 1, which writes its own.
// Within a wave every lane re-reads from a slot only the cells it stored itself (the cross-lane edge column travels by DPP /
// readlane or through the carries), loads are consumed before the row that issued them stores, and a store is made
// visible to the wave's later loads by the wavefront-scope fence the dense kernels use for the same purpose.
// To whoever builds the multi-wave form on this: "no ordering needed" holds here only because the multi-wave pipeline was
// LEFT OUT — no later strip runs rows behind an earlier one — not because the per-strip column ranges are exploited.  They
// are what makes that form possible (each strip reuses its own columns of a slot at its own pace), but the carries then
// have to become a hand-over ring with back-pressure as in poa_forward_pxmw_kernel; the parity double-buffer is only
// correct for strips that run strictly one after the other.  The price of leaving it out is measured: one wave per query
// is 1.8x / 2.6x slower than the dense pipeline on few long queries (profiles/pr_score_only/).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_forward_px.hpp"

namespace poa_amd {

struct SweepParams {
    const RowMeta* rows;        // [n_rows]
    const uint32_t* pred_rows;  // [n_edges]
    const uint32_t* slot;       // [n_rows] SweepRows::slot
    const uint32_t* pred_slot;  // [n_edges] SweepRows::pred_slot
    uint32_t n_rows, n_slots;   // n_slots >= 1 (sizes the per-query region)
    uint32_t first_query, n_queries;
    const uint8_t* qseq;
    const uint64_t* qoff;       // [total + 1]
    const uint32_t* pitch;      // [total]
    const uint64_t* plane_off;  // [total] element offset of the query's slots (poa_sweep_kernel; the one-strip kernel derives it)
    uint32_t* planes;           // per query [M: n_slots x stride | D: n_slots x stride]
    uint32_t* carry;            // [n_queries_in_chunk][2 parities][n_rows][2]: I entering the next strip, M of the strip's last column
    uint32_t cost_x, cost_oe, cost_e;   // 32-bit: the two-piece reduction opens a gap at open1 + extend1 - extend2 (beyond u8)
    uint32_t* score;            // [total]
    uint32_t* flags;            // [total] POA_FLAG_SHORT_QUERY where the dense pass sets it from the input alone, else 0
};

// ---------------------------------------------------------------------------------------------------------------------
// Capped form of the row bodies (score sets: poa_scoreset_run_capped, poa_scoreset.hpp).  The caller is interested in the score
// only if it is at most `cap`.  At a CHECK row (poa_sweep_rows.hpp: a row every start-to-end path passes, after which no
// earlier row is live) the wave reduces the row's M cells of columns 0..L to one minimum; scores never decrease along a
// path, so that minimum is a lower bound on M[end row][L], and a wave whose minimum is above the cap writes its result and
// returns.  The result does not depend on where a wave stops: the final write applies the same rule to the score itself.
// Everything in here is wave-uniform (the callers pass it through readfirstlane): the test is a scalar compare and branch.
struct SweepCap {
    static constexpr bool on = true, best = false;
    uint32_t cap;            // POA_SCORE_UNVISITED: no cap (no check can fire, the final write changes nothing)
    const uint32_t* check;   // the graph's check rows, ascending, 0xFFFFFFFF behind the last one
    uint32_t* swept;         // [n_pairs] row bodies the pair's wave executed
    // the cap as the row bodies ask for it: by the whole wave at a check row or a strip end, by the one lane of the final write
    __device__ __forceinline__ uint32_t now_wave(uint32_t) const { return cap; }
    __device__ __forceinline__ uint32_t now_lane() const { return cap; }
    __device__ __forceinline__ void publish(uint32_t, uint32_t) const {}
};
struct SweepNoCap { static constexpr bool on = false; };   // the uncapped form: nothing is passed, nothing is compiled in

// Best-of form (score sets: poa_scoreset_run_best): the cap is not a number the caller gave but the best score any pair of the
// SAME QUERY has finished with so far, plus a slack, under an optional ceiling of the query.  The query's best lives in one
// 64-bit word, score << 32 | pair index, all ones before the first result; it only ever decreases (atomic min), so a cap read
// from it is never below the final one: a stale value prunes less, never wrongly, and no wave waits for another.  The word is
// read where SweepCap's number is used — at every check row, strip end and final write — with a relaxed agent-scope atomic
// VECTOR load (one lane, then readfirstlane): the scalar cache is not coherent with the atomics of other waves.  The final
// write publishes a finite score that is within the cap it has just read; ties go to the lowest pair index by the key's low half.
struct SweepBest {
    static constexpr bool on = true, best = true;
    unsigned long long* word;   // the query's best word
    uint32_t slack, limit;      // cap = min(best score + slack (saturating), limit); limit POA_SCORE_UNVISITED: none
    const uint32_t* check;      // as SweepCap
    uint32_t* swept;
    __device__ __forceinline__ uint32_t now_lane() const {
        const uint32_t s = (uint32_t)(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32);
        const uint32_t t = s + slack;
        return umin(t < s ? 0xFFFFFFFFu : t, limit);
    }
    __device__ __forceinline__ uint32_t now_wave(uint32_t lane) const {
        uint32_t c = 0;
        if (lane == 0) c = now_lane();
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
    }
    __device__ __forceinline__ void publish(uint32_t score, uint32_t pair) const {
        (void)__hip_atomic_fetch_min(word, ((unsigned long long)score << 32) | pair, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// a wave-uniform value as the compiler sees one: the first active lane's, in an SGPR
__device__ __forceinline__ uint32_t wave_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// minimum over the 64 lanes, uniform: the DPP steps of wave_scan_min_plus without the weights, lane 63 ends with the total
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    v = umin(v, dpp_or_inf<0x111, 0xF>(v));
    v = umin(v, dpp_or_inf<0x112, 0xF>(v));
    v = umin(v, dpp_or_inf<0x114, 0xF>(v));
    v = umin(v, dpp_or_inf<0x118, 0xF>(v));
    v = umin(v, dpp_or_inf<0x142, 0xA>(v));
    v = umin(v, dpp_or_inf<0x143, 0xC>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// the same on both 16-bit halves at once, then the smaller half
__device__ __forceinline__ uint32_t wave_min_pk(uint32_t v) {
    v = pk_min(v, dpp_or_inf<0x111, 0xF>(v));
    v = pk_min(v, dpp_or_inf<0x112, 0xF>(v));
    v = pk_min(v, dpp_or_inf<0x114, 0xF>(v));
    v = pk_min(v, dpp_or_inf<0x118, 0xF>(v));
    v = pk_min(v, dpp_or_inf<0x142, 0xA>(v));
    v = pk_min(v, dpp_or_inf<0x143, 0xC>(v));
    const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    return umin(t & 0xFFFFu, t >> 16);
}

// ---------------------------------------------------------------------------------------------------------------------
// General path: any pitch (strips of W = Q * 64 * K columns, one after the other), u16 cells where the engine's bound on
// the optimal score allows them (arithmetic in 32-bit registers, as in poa_forward_kernel), else u32.
//
// The rows of one query, all strips: the body of poa_sweep_kernel, shared with the score-set kernels (poa_scoreset.hpp), which
// hand it the tables of the pair's own graph in P.  Of P it reads the graph tables, n_rows, n_slots, the costs and score /
// flags; the query (L symbols at q, `pitch` columns), its slot region (M at Mp, D behind it), its carries (4 x n_rows words,
// touched only by a query wider than one strip) and the index `out` of its result come from the caller.
//
// CapT = SweepCap or SweepBest: the capped form (CAP).  A query of one strip tests at its graph's check rows.  A row of one strip of a wider query
// is not a cut of the cell grid, so such a query tests at the end of every strip but the last instead: the query extends
// beyond the strip, every path to column L crosses from the strip's last column to the next one, and the minimum over all
// rows of M in that column — the carry word, which also bounds the insertion carry from below — is a lower bound again.
template <int Q, typename T, typename CapT = SweepNoCap>
__device__ __forceinline__ void sweep_rows(const SweepParams& P, const uint32_t out, const uint32_t lane, const uint32_t L,
                                           const uint8_t* __restrict__ q, const uint32_t pitch, T* __restrict__ Mp,
                                           uint32_t* __restrict__ carry, const CapT cap = CapT{}) {
    constexpr bool CAP = CapT::on;
    using IO = PlaneIO<T>;
    constexpr int K = IO::K;
    constexpr int C = K * Q;
    constexpr uint32_t QW = 64 * K;
    constexpr uint32_t W = QW * Q;
    T* __restrict__ Dp = Mp + (uint64_t)P.n_slots * pitch;
    const uint32_t x = P.cost_x, oe = P.cost_oe, e = P.cost_e;
    const uint32_t n_strips = (pitch + W - 1) / W;
    const uint32_t step = K * e;
    const uint32_t w15 = ((lane & 15u) + 1u) * step;
    const uint32_t w31 = (lane - 31u) * step;
    const uint32_t lane_off = K * lane * e;

    for (uint32_t s = 0; s < n_strips; ++s) {
        const uint32_t sbase = s * W;
        const uint32_t* __restrict__ cin_row = carry + (uint64_t)((s + 1u) & 1u) * 2u * P.n_rows;   // written by strip s - 1
        uint32_t* __restrict__ cout_row = carry + (uint64_t)(s & 1u) * 2u * P.n_rows;
        const bool from_prev = s > 0, to_next = s + 1 < n_strips;
        const CU32* check = nullptr;   // (CAP only, like the next two) the next entry of the graph's check rows
        uint32_t next_check = 0xFFFFFFFFu, last_col_min = INF;
        if constexpr (CAP) {
            check = (const CU32*)cap.check;
            if (n_strips == 1) next_check = *check++;
        } else {
            (void)check; (void)next_check; (void)last_col_min;
        }
        bool act[Q];
        uint32_t qcp[C / 4], ql[Q];
#pragma unroll
        for (int m = 0; m < Q; ++m) {
            const uint32_t c0 = sbase + m * QW + K * lane;
            act[m] = c0 < pitch;
#pragma unroll
            for (int w = 0; w < K / 4; ++w) {
                uint32_t pk = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t c = c0 + 4 * w + k;
                    pk |= ((c < L) ? (uint32_t)q[c] : 0u) << (8 * k);
                }
                qcp[m * (K / 4) + w] = pk;
            }
            ql[m] = (c0 > 0 && c0 - 1 < L) ? (uint32_t)q[c0 - 1] : 0u;
        }
        auto qsym = [&](int i) -> uint32_t { return qbyte(qcp[i >> 2], i & 3); };

        uint32_t Mprev[C], Dprev[C];
#pragma unroll
        for (int k = 0; k < C; ++k) { Mprev[k] = INF; Dprev[k] = INF; }

        for (uint32_t r = 0; r < P.n_rows; ++r) {
            const RowMeta meta = P.rows[r];
            const uint32_t sym = meta.sym;
            const uint32_t my_slot = P.slot[r];
            uint32_t PM[C], PD[C], PMl[Q];
            if (meta.flags & ROW_CHAIN) {
                uint32_t edge = from_prev ? cin_row[2 * (r - 1) + 1] : INF;
#pragma unroll
                for (int m = 0; m < Q; ++m) {
                    PMl[m] = wave_shr1(Mprev[K * m + K - 1], edge);
                    edge = (uint32_t)__builtin_amdgcn_readlane((int)Mprev[K * m + K - 1], 63);
                }
#pragma unroll
                for (int k = 0; k < C; ++k) { PM[k] = Mprev[k]; PD[k] = Dprev[k]; }
            } else {
#pragma unroll
                for (int k = 0; k < C; ++k) { PM[k] = INF; PD[k] = INF; }
#pragma unroll
                for (int m = 0; m < Q; ++m) PMl[m] = INF;
                if (meta.pred_count > 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // I read back what this wave stored
                for (uint32_t pe = 0; pe < meta.pred_count; ++pe) {
                    const uint32_t pr = P.pred_rows[meta.pred_begin + pe];
                    uint32_t tm[C], td[C];
                    if (pr + 1 == r) {
#pragma unroll
                        for (int k = 0; k < C; ++k) { tm[k] = Mprev[k]; td[k] = Dprev[k]; }
                    } else {
                        const uint64_t pbase = (uint64_t)P.pred_slot[meta.pred_begin + pe] * pitch + sbase + K * lane;
#pragma unroll
                        for (int m = 0; m < Q; ++m) {
                            uint32_t a[K], b[K];
#pragma unroll
                            for (int k = 0; k < K; ++k) { a[k] = INF; b[k] = INF; }
                            if (act[m]) {
                                IO::load(Mp + pbase + m * QW, a);
                                IO::load(Dp + pbase + m * QW, b);
                            }
#pragma unroll
                            for (int k = 0; k < K; ++k) { tm[K * m + k] = a[k]; td[K * m + k] = b[k]; }
                        }
                    }
                    uint32_t edge = from_prev ? cin_row[2 * pr + 1] : INF;
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        PMl[m] = umin(PMl[m], wave_shr1(tm[K * m + K - 1], edge));
                        edge = (uint32_t)__builtin_amdgcn_readlane((int)tm[K * m + K - 1], 63);
                    }
#pragma unroll
                    for (int k = 0; k < C; ++k) { PM[k] = umin(PM[k], tm[k]); PD[k] = umin(PD[k], td[k]); }
                }
            }

            uint32_t Mc[C], Dc[C];
            if (meta.flags & ROW_END) {
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    Dc[k] = sat_add(PD[k], e);
                    Mc[k] = umin(PM[k], Dc[k]);
                }
            } else {
                const bool open_always = (meta.flags & ROW_OPENI_ALWAYS) != 0;
                const bool open_never = (meta.flags & ROW_OPENI_NEVER) != 0;
                const uint32_t csym = meta.child_sym;
                uint32_t H[C], Ic[C], Tq[Q];
#pragma unroll
                for (int m = 0; m < Q; ++m) {
                    uint32_t t = INF;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const int i = K * m + k;
                        const uint32_t qk = qsym(i);
                        const uint32_t open = (qk != sym) ? sat_add(PM[i], oe) : INF;
                        Dc[i] = umin(sat_add(PD[i], e), open);
                        const uint32_t pm_left = (k == 0) ? PMl[m] : PM[i - 1];
                        const uint32_t q_left = (k == 0) ? ql[m] : qsym(i - 1);
                        H[i] = umin(sat_add(pm_left, (q_left != sym) ? x : 0u), Dc[i]);
                        if (m == 0 && k == 0 && (meta.flags & ROW_START) && sbase == 0 && lane == 0) H[i] = 0;
                        Ic[i] = t;
                        const bool op = !open_never && (open_always || qk != csym);
                        t = umin(sat_add(t, e), op ? sat_add(H[i], oe) : INF);
                    }
                    Tq[m] = t;
                }
                uint32_t cq = from_prev ? cin_row[2 * r] : INF;  // insertion value entering column sbase
#pragma unroll
                for (int m = 0; m < Q; ++m) {
                    const uint32_t Pm = wave_scan_min_plus(Tq[m], step, w15, w31);
                    const uint32_t excl = wave_shr1(Pm, INF);
                    const uint32_t cin = umin(excl, sat_add(cq, lane_off));
                    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)Pm, 63);
                    cq = umin(sat_add(cq, QW * e), total);
                    Ic[K * m] = cin;
#pragma unroll
                    for (int k = 1; k < K; ++k) Ic[K * m + k] = umin(Ic[K * m + k], sat_add(cin, (uint32_t)k * e));
                }
                if (to_next && lane == 0) cout_row[2 * r] = cq;  // I[r][(s + 1) * W]
#pragma unroll
                for (int k = 0; k < C; ++k) Mc[k] = umin(H[k], Ic[k]);
            }
            if (to_next && lane == 63) cout_row[2 * r + 1] = Mc[C - 1];  // M[r][(s + 1) * W - 1]
            if constexpr (CAP) {
                if (to_next) last_col_min = umin(last_col_min, Mc[C - 1]);
                if (r == next_check) {
                    // columns beyond L are left out: they hold real values of cells no path to column L uses, which could
                    // only weaken the bound.  The lane's last valid column is worked out here, at the check row, and hidden
                    // from the optimiser: as a loop invariant the C column tests would be hoisted into C scalar register
                    // pairs, which the row loop does not have to spare (it would pay for them with spills on every row).
                    uint32_t mn = INF;
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        int32_t last = (int32_t)(L - (sbase + m * QW + K * lane));   // columns k <= last of this lane's K are real
                        asm volatile("" : "+v"(last));
#pragma unroll
                        for (int k = 0; k < K; ++k) mn = umin(mn, k <= last ? Mc[K * m + k] : INF);
                    }
                    if (wave_min(mn) > cap.now_wave(lane)) {
                        if (lane == 0) {
                            P.score[out] = INF;
                            P.flags[out] = (L == 1 ? POA_FLAG_SHORT_QUERY : 0u) | POA_FLAG_CAPPED;
                            cap.swept[out] = r + 1;
                        }
                        return;
                    }
                    next_check = *check++;
                }
            }
            if (my_slot != 0xFFFFFFFFu) {
                const uint64_t sb = (uint64_t)my_slot * pitch + sbase + K * lane;
#pragma unroll
                for (int m = 0; m < Q; ++m) {
                    if (act[m]) {
                        IO::store(Mp + sb + m * QW, &Mc[K * m]);
                        IO::store(Dp + sb + m * QW, &Dc[K * m]);
                    }
                }
            }
            if (r + 1 == P.n_rows && L >= sbase && L < sbase + W) {
                // the only output: M[end row][L], held by one lane of this strip
                uint32_t v = INF;
#pragma unroll
                for (int m = 0; m < Q; ++m)
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if (sbase + m * QW + K * lane + k == L) v = Mc[K * m + k];
                const uint32_t owner = ((L - sbase) % QW) / K;
                if (lane == owner) {
                    if constexpr (CAP) {
                        const uint32_t sc = (sizeof(T) == 2 && v >= 0xFFFFu) ? INF : v;
                        const bool over = sc > cap.now_lane();
                        P.score[out] = over ? INF : sc;
                        P.flags[out] = (L == 1 ? POA_FLAG_SHORT_QUERY : 0u) | (over ? POA_FLAG_CAPPED : 0u);
                        cap.swept[out] = n_strips * P.n_rows;
                        if constexpr (CapT::best) { if (!over && sc != INF) cap.publish(sc, out); }
                    } else {
                        P.score[out] = (sizeof(T) == 2 && v >= 0xFFFFu) ? INF : v;
                        P.flags[out] = L == 1 ? POA_FLAG_SHORT_QUERY : 0u;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < C; ++k) { Mprev[k] = Mc[k]; Dprev[k] = Dc[k]; }
        }
        if constexpr (CAP) {
            if (to_next && (uint32_t)__builtin_amdgcn_readlane((int)last_col_min, 63) > cap.now_wave(lane)) {
                if (lane == 0) {
                    P.score[out] = INF;
                    P.flags[out] = (L == 1 ? POA_FLAG_SHORT_QUERY : 0u) | POA_FLAG_CAPPED;
                    cap.swept[out] = (s + 1u) * P.n_rows;
                }
                return;
            }
        }
        if (n_strips > 1) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the carries of this strip, read by the next
    }
}

template <int Q, typename T>
__global__ __launch_bounds__(256) void poa_sweep_kernel(SweepParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wq = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave-uniform
    if (wq >= P.n_queries) return;
    const uint32_t qi = P.first_query + wq;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    sweep_rows<Q, T>(P, qi, lane, L, P.qseq + qbeg, P.pitch[qi], reinterpret_cast<T*>(P.planes) + P.plane_off[qi],
                     P.carry + 4ull * wq * P.n_rows);
}

// ---------------------------------------------------------------------------------------------------------------------
// Headline path: packed u16, one strip (pitch <= 1024), the pairs-across-quads register mapping of poa_forward_px_kernel
// (register k of a lane: lo half = column 8l + k, hi half = column 512 + 8l + k) and its row step in the MF = 3 shape, without
// the two remaining flag tests.  A slot row is stored in that REGISTER layout — 1024 cells, lane l's eight registers as two
// 16-byte words at [h * 64 + l] — since nothing but this kernel reads it: no v_perm_b32 repack on the way out or back in,
// and no store at all for a row without a slot.  Columns at and beyond the pitch hold ordinary "past the end of the query"
// values that only ever flow to the right, away from column L.
//
// The rows of one query: the body of poa_sweep_px_kernel, shared with the score-set kernels (poa_scoreset.hpp) as sweep_rows
// is.  L <= 1023 symbols at q; Mp is the calling lane's place in the query's region, [M: n_slots x 128 uint4 | D: n_slots x
// 128 uint4] + lane; the result goes to index `out`.  CapT = SweepCap or SweepBest: the capped form (CAP), tested at the graph's
// check rows.
template <typename CapT = SweepNoCap>
__device__ __forceinline__ void sweep_px_rows(const SweepParams& P, const uint32_t out, const uint32_t lane, const uint32_t L,
                                              const uint8_t* __restrict__ q, uint4* __restrict__ Mp, const CapT cap = CapT{}) {
    constexpr bool CAP = CapT::on;
    constexpr int K = 8;
    constexpr uint32_t QW = 64 * K;
    constexpr uint32_t I16 = 0xFFFFu, INF2 = 0xFFFFFFFFu;
    uint4* __restrict__ Dp = Mp + (uint64_t)P.n_slots * 128u;
    const uint32_t e = P.cost_e, x = P.cost_x;
    auto pack16 = [](uint32_t v) { v = v < I16 ? v : I16; return v | (v << 16); };
    const uint32_t e2 = pack16(e), oe2 = pack16(P.cost_oe), x2 = pack16(x);
    const uint32_t step = K * e;
    const uint32_t step2 = pack16(step);
    const uint32_t w15_2 = pack16(((lane & 15u) + 1u) * step);
    const uint32_t w31_2 = pack16(lane >= 32u ? (lane - 31u) * step : 0xFFFFu);
    const uint32_t lane_off2 = pack16(K * lane * e);
    const uint32_t c_lo = K * lane, c_hi = QW + K * lane;
    uint32_t qP[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t a = (c_lo + k < L) ? (uint32_t)q[c_lo + k] : 0u, b = (c_hi + k < L) ? (uint32_t)q[c_hi + k] : 0u;
        qP[k] = a | (b << 16);
    }
    const uint32_t qlE = ((c_lo > 0 && c_lo - 1 < L) ? (uint32_t)q[c_lo - 1] : 0u) | (((c_hi - 1 < L) ? (uint32_t)q[c_hi - 1] : 0u) << 16);

    // symbol masks per lane, staged once in LDS (as poa_forward_px_kernel does): mask[s][k] = 0xFFFF per half where my query
    // symbol equals "ACGT"[s]; a fifth, all-zero table stands for "an insertion opens everywhere"
    __shared__ uint4 sym_tab[4 * 5 * 2 * 64];
    uint4* my_tab = sym_tab + (threadIdx.x >> 6) * (5 * 2 * 64) + lane;
    {
        const uint32_t letters[4] = {'A', 'C', 'G', 'T'};
#pragma unroll
        for (int si = 0; si < 4; ++si) {
            const uint32_t s2 = letters[si] | (letters[si] << 16);
            uint32_t m[K];
#pragma unroll
            for (int k = 0; k < K; ++k) m[k] = pku(pkv(0u) - pkv(pk_is_zero(qP[k] ^ s2)));
            my_tab[(si * 2 + 0) * 64] = make_uint4(m[0], m[1], m[2], m[3]);
            my_tab[(si * 2 + 1) * 64] = make_uint4(m[4], m[5], m[6], m[7]);
        }
        my_tab[(4 * 2 + 0) * 64] = make_uint4(0u, 0u, 0u, 0u);
        my_tab[(4 * 2 + 1) * 64] = make_uint4(0u, 0u, 0u, 0u);
        // each lane reads back only what it wrote itself: no barrier needed
    }

    // read-only graph tables through the constant address space (scalar loads, not waited for with the plane accesses)
    const CRowWords* crows = (const CRowWords*)P.rows;
    const CU32* cpred = (const CU32*)P.pred_rows;
    const CU32* cslot = (const CU32*)P.slot;
    const CU32* cpslot = (const CU32*)P.pred_slot;

    uint32_t PMc[K], PDc[K], PMlc = INF2;   // predecessor minima of the last multi-predecessor row (ROW_SAME_PREDS reuses them)
#pragma unroll
    for (int k = 0; k < K; ++k) { PMc[k] = INF2; PDc[k] = INF2; }

    // (CAP) 0xFFFF in every half whose column lies beyond L: those cells stay out of a check row's minimum
    uint32_t pad[K];
    uint32_t ci = 0, next_check = 0xFFFFFFFFu;
    if constexpr (CAP) {
#pragma unroll
        for (int k = 0; k < K; ++k) pad[k] = (c_lo + k <= L ? 0u : I16) | (c_hi + k <= L ? 0u : 0xFFFF0000u);
        next_check = ((const CU32*)cap.check)[0];
    }

    poa_u32x4 mw_ahead = crows[0];   // row record and slot, read one row ahead
    uint32_t slot_ahead = cslot[0];
    // the previous row, by value: one loop body, one pair of arrays (alternating two register sets through references, as
    // the dense kernel does, ends with the arrays in scratch memory here)
    uint32_t Mprev[K], Dprev[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { Mprev[k] = INF2; Dprev[k] = INF2; }
    for (uint32_t r = 0; r < P.n_rows; ++r) {
        const poa_u32x4 mw = mw_ahead;
        const uint32_t my_slot = slot_ahead;
        const uint32_t rn = r + 1 < P.n_rows ? r + 1 : r;
        mw_ahead = crows[rn];
        slot_ahead = cslot[rn];
        struct { uint32_t pred_begin, pred_count, sym, child_sym, flags, sym_idx; } meta{mw.y, mw.z, mw.w & 0xFFu, (mw.w >> 8) & 0xFFu, (mw.w >> 16) & 0xFFu, mw.w >> 24};
        const uint32_t sym = meta.sym;
        const uint32_t sym2 = sym | (sym << 16);
        uint32_t PMl = INF2;

        // lane l <- v of lane l - 1; lane 0: lo half <- INF (no column -1), hi half <- lane 63's lo half (column 511)
        auto shr_lane = [&](uint32_t v) {
            const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
            return pk_wave_shr1(v, I16 | (last << 16));
        };

        uint32_t Mc[K], Dc[K];
        auto row_body = [&](const uint32_t (&PM)[K], const uint32_t (&PD)[K]) {
            uint32_t PDe[K];
#pragma unroll
            for (int k = 0; k < K; ++k) PDe[k] = pk_add_sat(PD[k], e2);
            if (meta.flags & ROW_END) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    Dc[k] = PDe[k];
                    Mc[k] = pk_min(PM[k], Dc[k]);
                }
            } else {
                const uint32_t cs1 = (meta.flags & ROW_OPENI_ALWAYS) ? 0u : (uint32_t)meta.child_sym;
                const uint32_t start_keep = ((meta.flags & ROW_START) && lane == 0) ? 0xFFFF0000u : 0xFFFFFFFFu;
                uint32_t mD[K], mI[K];
                const uint32_t si = meta.sym_idx & 15u, ci = meta.sym_idx >> 4;
                if ((meta.sym_idx & 0x88u) == 0) {
                    const uint4 a = my_tab[(si * 2 + 0) * 64], b = my_tab[(si * 2 + 1) * 64];
                    const uint4 c = my_tab[(ci * 2 + 0) * 64], d = my_tab[(ci * 2 + 1) * 64];
                    mD[0] = a.x; mD[1] = a.y; mD[2] = a.z; mD[3] = a.w; mD[4] = b.x; mD[5] = b.y; mD[6] = b.z; mD[7] = b.w;
                    mI[0] = c.x; mI[1] = c.y; mI[2] = c.z; mI[3] = c.w; mI[4] = d.x; mI[5] = d.y; mI[6] = d.z; mI[7] = d.w;
                } else {
                    const uint32_t csym2 = cs1 | (cs1 << 16);
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        mD[k] = pku(pkv(0u) - pkv(pk_is_zero(qP[k] ^ sym2)));
                        mI[k] = pku(pkv(0u) - pkv(pk_is_zero(qP[k] ^ csym2)));
                    }
                }
                // one OPERATION at a time over the eight columns, as in poa_forward_px_kernel: gfx950 wants a wait state between a
                // packed-math result and its packed-math use
                uint32_t Hc[K], Ic[K], u[K], h1[K];
                const uint32_t cost_left0 = pk_sub_sat(x2, pku(pkv(0u) - pkv(pk_is_zero(qlE ^ sym2))));
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = pk_add_sat(PM[k], oe2);
                h1[0] = cost_left0;
#pragma unroll
                for (int k = 1; k < K; ++k) h1[k] = pk_sub_sat(x2, mD[k - 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = pk_max(u[k], mD[k]);   // a deletion opens only where the symbols differ
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
                u[0] = pk_max(u[0], mI[0]);   // insertion open: (q != child symbol) ? H + oe : INF; column k + 1 inside the chain's step k
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
                const uint32_t total_lo = (uint32_t)__builtin_amdgcn_readlane((int)Pm, 63) & 0xFFFFu;
                const uint32_t cin = pk_min(excl, pk_add_sat(I16 | (total_lo << 16), lane_off2));
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    Ic[k] = pk_min(Ic[k], pk_add_sat(cin, (uint32_t)k * e2));
                    Mc[k] = pk_min(Hc[k], Ic[k]);
                }
            }
            if (my_slot != 0xFFFFFFFFu) {
                uint4* m = Mp + (uint64_t)my_slot * 128u;
                uint4* d = Dp + (uint64_t)my_slot * 128u;
                m[0] = make_uint4(Mc[0], Mc[1], Mc[2], Mc[3]);
                m[64] = make_uint4(Mc[4], Mc[5], Mc[6], Mc[7]);
                d[0] = make_uint4(Dc[0], Dc[1], Dc[2], Dc[3]);
                d[64] = make_uint4(Dc[4], Dc[5], Dc[6], Dc[7]);
            }
        };

        // The predecessor values are gathered into one pair of arrays and the row body has ONE call site: three call sites on
        // three different array pairs get merged by the compiler into one body fed by a pointer, and the arrays then live
        // in scratch memory.
        uint32_t PM[K], PD[K];
        if (meta.flags & ROW_CHAIN) {
            PMl = shr_lane(Mprev[K - 1]);
#pragma unroll
            for (int k = 0; k < K; ++k) { PM[k] = Mprev[k]; PD[k] = Dprev[k]; }
        } else if (meta.flags & ROW_SAME_PREDS) {
            PMl = PMlc;
#pragma unroll
            for (int k = 0; k < K; ++k) { PM[k] = PMc[k]; PD[k] = PDc[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) { PM[k] = INF2; PD[k] = INF2; }
            if (meta.pred_count > 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // I read back what this wave stored
            for (uint32_t pe = 0; pe < meta.pred_count; ++pe) {
                const uint32_t pr = cpred[meta.pred_begin + pe];
                uint32_t tm[K], td[K];
                if (pr + 1 == r) {
#pragma unroll
                    for (int k = 0; k < K; ++k) { tm[k] = Mprev[k]; td[k] = Dprev[k]; }
                } else {
                    const uint64_t pb = (uint64_t)cpslot[meta.pred_begin + pe] * 128u;
                    const uint4 m0 = Mp[pb], m1 = Mp[pb + 64], d0 = Dp[pb], d1 = Dp[pb + 64];
                    tm[0] = m0.x; tm[1] = m0.y; tm[2] = m0.z; tm[3] = m0.w; tm[4] = m1.x; tm[5] = m1.y; tm[6] = m1.z; tm[7] = m1.w;
                    td[0] = d0.x; td[1] = d0.y; td[2] = d0.z; td[3] = d0.w; td[4] = d1.x; td[5] = d1.y; td[6] = d1.z; td[7] = d1.w;
                }
                PMl = pk_min(PMl, shr_lane(tm[K - 1]));
#pragma unroll
                for (int k = 0; k < K; ++k) { PM[k] = pk_min(PM[k], tm[k]); PD[k] = pk_min(PD[k], td[k]); }
            }
            PMlc = PMl;
#pragma unroll
            for (int k = 0; k < K; ++k) { PMc[k] = PM[k]; PDc[k] = PD[k]; }
        }
        row_body(PM, PD);
        if constexpr (CAP) {
            if (r == next_check) {
                // register min tree over the lane's eight packed cells, both halves being columns, then across the lanes
                const uint32_t a = pk_min(pk_min(Mc[0] | pad[0], Mc[1] | pad[1]), pk_min(Mc[2] | pad[2], Mc[3] | pad[3]));
                const uint32_t b = pk_min(pk_min(Mc[4] | pad[4], Mc[5] | pad[5]), pk_min(Mc[6] | pad[6], Mc[7] | pad[7]));
                if (wave_min_pk(pk_min(a, b)) > cap.now_wave(lane)) {   // (0xFFFF is INF: a cap of 0xFFFF or more never fires)
                    if (lane == 0) {
                        P.score[out] = INF;
                        P.flags[out] = (L == 1 ? POA_FLAG_SHORT_QUERY : 0u) | POA_FLAG_CAPPED;
                        cap.swept[out] = r + 1;
                    }
                    return;
                }
                next_check = ((const CU32*)cap.check)[++ci];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) { Mprev[k] = Mc[k]; Dprev[k] = Dc[k]; }
    }

    // The only output: M[end row][L].  The register that holds it depends on L; the lane's slice of the symbol tables is
    // free now, so the row goes there and the one cell is read back with a dynamic LDS address (a register array indexed
    // by a run-time value would put the row arrays of the whole loop into scratch memory).
    my_tab[0] = make_uint4(Mprev[0], Mprev[1], Mprev[2], Mprev[3]);
    my_tab[64] = make_uint4(Mprev[4], Mprev[5], Mprev[6], Mprev[7]);
    const uint32_t col = L & (QW - 1u);
    if (lane == (col >> 3)) {
        const uint32_t kk = col & 7u;
        uint32_t v = reinterpret_cast<const uint32_t*>(&my_tab[(kk >> 2) * 64])[kk & 3u];
        v = L >= QW ? v >> 16 : v & 0xFFFFu;
        if constexpr (CAP) {
            const uint32_t sc = v == I16 ? INF : v;
            const bool over = sc > cap.now_lane();
            P.score[out] = over ? INF : sc;
            P.flags[out] = (L == 1 ? POA_FLAG_SHORT_QUERY : 0u) | (over ? POA_FLAG_CAPPED : 0u);
            cap.swept[out] = P.n_rows;
            if constexpr (CapT::best) { if (!over && sc != INF) cap.publish(sc, out); }
        } else {
            P.score[out] = v == I16 ? INF : v;
            P.flags[out] = L == 1 ? POA_FLAG_SHORT_QUERY : 0u;
        }
    }
}

__global__ __launch_bounds__(256) void poa_sweep_px_kernel(SweepParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wq = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave-uniform
    if (wq >= P.n_queries) return;
    const uint32_t qi = P.first_query + wq;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);  // <= 1023 (launcher: one strip)
    // per query: [M: n_slots x 128 uint4 | D: n_slots x 128 uint4]
    sweep_px_rows(P, qi, lane, L, P.qseq + qbeg, reinterpret_cast<uint4*>(P.planes) + (uint64_t)wq * P.n_slots * 256u + lane);
}

}  // namespace poa_amd
