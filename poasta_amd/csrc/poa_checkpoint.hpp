// Checkpointed alignment (POA_MODE_CHECKPOINT) for gfx950: dense mode's results — score, pairs, certificate flags — from a
// workspace of O(segments x live rows + segment length) plane rows per query instead of all rows.
//
// The graph's rows are cut into segments (CheckpointPlan, poa_sweep_rows.hpp).  Two kernels, one wavefront per query in both:
//
//   pass 1, poa_ckpt_sweep_kernel: the score-only sweep (poa_forward_sweep.hpp: same recurrences, same slot addressing, same
//     strip carries), which besides its slots stores every row that a later segment may read into the SNAPSHOT of that
//     segment's first boundary — M and D only, I never leaves its row.  A row is stored as it is computed, into every snapshot
//     it belongs to (snap_off / snap_dst), each strip writing its own column range.  It also yields the score.
//   pass 2, poa_ckpt_trace_kernel: from the last segment to the first, recompute the segment's M, I and D rows in full into
//     a window of max_segment rows — predecessors inside the segment from the window (or from registers: the previous row),
//     predecessors before it from the snapshot — then walk the traceback inside the window until it steps to a row before
//     the segment.  The walk's state survives in registers to the segment that holds that row; segments the walk jumps
//     over are not recomputed.  What crosses a strip boundary is read back from the window: full rows of M and I are there.
//
// The walk is the rule of tb_step (poa_kernels.hpp) in its full-plane form — stored M, I and D compared, predecessors in
// trait order, first candidate taken, the same certificate — taken one step at a time by lane 0.  traceback_wave speculates
// on runs of steps but emits, by construction, what the step-by-step walk emits, so both agree bit for bit.  TbCtx addresses a
// cell as row * pitch; here a predecessor is found through its EDGE (pred_src: window row or snapshot row), the only way
// the walk ever reaches another row.
//
// Memory of a query, in cells of T (u16 under the bound dense mode uses, else u32), rows of `pitch` cells:
//   [slot M: n_slots][slot D: n_slots][snapshot M: n_snap][snapshot D: n_snap][window M: seg][window I: seg][window D: seg]
// One wave owns all of it from its first row to its last, in both passes, so nothing is ordered between waves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_forward_px.hpp"
#include "poa_forward_sweep.hpp"
#include "poa_sweep_rows.hpp"

namespace poa_amd {

struct CkptParams {
    const RowMeta* rows;        // [n_rows]
    const uint32_t* pred_rows;  // [n_edges]
    const uint32_t* slot;       // [n_rows] SweepRows::slot
    const uint32_t* pred_slot;  // [n_edges] SweepRows::pred_slot
    const uint32_t* snap_off;   // [n_rows + 1] CheckpointPlan::snap_off
    const uint32_t* snap_dst;   // CheckpointPlan::snap_dst
    const uint32_t* pred_src;   // [n_edges] CheckpointPlan::pred_src
    const uint32_t* boundary;   // [n_segments + 1]
    uint32_t n_rows, n_slots, n_snap, seg_rows, n_segments;
    uint32_t start_row, end_row;
    uint32_t first_query, n_queries;
    const uint8_t* qseq;
    const uint64_t* qoff;       // [total + 1]
    const uint32_t* pitch;      // [total]
    const uint64_t* plane_off;  // [total] offset of the query's region, in cells
    uint32_t* planes;
    uint32_t* carry;            // pass 1: [n_queries_in_chunk][2 parities][n_rows][2], as in SweepParams
    uint32_t cost_x, cost_o, cost_e;
    const uint64_t* scratch_off;  // [total + 1] per-query region in `scratch` (capacity len + n_rows)
    uint2* scratch;               // pairs written from the BACK of each region, as poa_traceback_kernel does
    uint32_t* score;              // [total]
    uint32_t* flags;              // [total]
    uint32_t* n_pairs;            // [total]
};

template <typename T>
struct CkptRegion {
    T *slot_m, *slot_d, *snap_m, *snap_d, *win_m, *win_i, *win_d;
    __device__ __forceinline__ CkptRegion(const CkptParams& P, uint32_t qi, uint32_t pitch) {
        slot_m = reinterpret_cast<T*>(P.planes) + P.plane_off[qi];
        slot_d = slot_m + (uint64_t)P.n_slots * pitch;
        snap_m = slot_d + (uint64_t)P.n_slots * pitch;
        snap_d = snap_m + (uint64_t)P.n_snap * pitch;
        win_m = snap_d + (uint64_t)P.n_snap * pitch;
        win_i = win_m + (uint64_t)P.seg_rows * pitch;
        win_d = win_i + (uint64_t)P.seg_rows * pitch;
    }
};

// Rows [r0, r1) of one query, strip after strip.  PASS 1: the whole graph, slots + snapshots.  PASS 2: one segment, window.
template <int Q, typename T, int PASS>
__device__ __forceinline__ void ckpt_rows(const CkptParams& P, const CkptRegion<T>& R, const uint32_t qi, const uint32_t wq,
                                          const uint32_t lane, const uint32_t r0, const uint32_t r1, const uint32_t pitch,
                                          const uint32_t L, const uint8_t* __restrict__ q) {
    using IO = PlaneIO<T>;
    constexpr int K = IO::K;
    constexpr int C = K * Q;
    constexpr uint32_t QW = 64 * K;
    constexpr uint32_t W = QW * Q;
    uint32_t* __restrict__ carry = P.carry + 4ull * wq * P.n_rows;
    const uint32_t x = P.cost_x, oe = P.cost_o + P.cost_e, e = P.cost_e;
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
        // PASS 2: the query symbol left of the strip (wave-uniform), for the insertion value that enters the strip
        const uint32_t q_edge = (from_prev && sbase - 1 < L) ? (uint32_t)q[sbase - 1] : 0u;

        uint32_t Mprev[C], Dprev[C];
#pragma unroll
        for (int k = 0; k < C; ++k) { Mprev[k] = INF; Dprev[k] = INF; }

        for (uint32_t r = r0; r < r1; ++r) {
            const RowMeta meta = P.rows[r];
            const uint32_t sym = meta.sym;
            const uint32_t lr = r - r0;   // PASS 2: the row's place in the window
            uint32_t PM[C], PD[C], PMl[Q];
            if ((meta.flags & ROW_CHAIN) && r > r0) {
                uint32_t edge = INF;
                if (from_prev) edge = PASS == 1 ? cin_row[2 * (r - 1) + 1] : IO::get(R.win_m + (uint64_t)(lr - 1) * pitch + sbase - 1);
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
                    uint32_t edge = INF;
                    if (pr + 1 == r && r > r0) {
#pragma unroll
                        for (int k = 0; k < C; ++k) { tm[k] = Mprev[k]; td[k] = Dprev[k]; }
                        if (from_prev) edge = PASS == 1 ? cin_row[2 * pr + 1] : IO::get(R.win_m + (uint64_t)(lr - 1) * pitch + sbase - 1);
                    } else {
                        const T *pm, *pd;
                        if (PASS == 1) {
                            const uint64_t ps = (uint64_t)P.pred_slot[meta.pred_begin + pe] * pitch;
                            pm = R.slot_m + ps; pd = R.slot_d + ps;
                            if (from_prev) edge = cin_row[2 * pr + 1];
                        } else {
                            const uint32_t loc = P.pred_src[meta.pred_begin + pe];
                            const uint64_t ps = (uint64_t)(loc & ~CKPT_SNAP) * pitch;
                            pm = ((loc & CKPT_SNAP) ? R.snap_m : R.win_m) + ps;
                            pd = ((loc & CKPT_SNAP) ? R.snap_d : R.win_d) + ps;
                            if (from_prev) edge = IO::get(pm + sbase - 1);
                        }
                        const uint32_t cb = sbase + K * lane;
#pragma unroll
                        for (int m = 0; m < Q; ++m) {
                            uint32_t a[K], b[K];
#pragma unroll
                            for (int k = 0; k < K; ++k) { a[k] = INF; b[k] = INF; }
                            if (act[m]) {
                                IO::load(pm + cb + m * QW, a);
                                IO::load(pd + cb + m * QW, b);
                            }
#pragma unroll
                            for (int k = 0; k < K; ++k) { tm[K * m + k] = a[k]; td[K * m + k] = b[k]; }
                        }
                    }
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        PMl[m] = umin(PMl[m], wave_shr1(tm[K * m + K - 1], edge));
                        edge = (uint32_t)__builtin_amdgcn_readlane((int)tm[K * m + K - 1], 63);
                    }
#pragma unroll
                    for (int k = 0; k < C; ++k) { PM[k] = umin(PM[k], tm[k]); PD[k] = umin(PD[k], td[k]); }
                }
            }

            uint32_t Mc[C], Ic[C], Dc[C];
            if (meta.flags & ROW_END) {
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    Dc[k] = sat_add(PD[k], e);
                    Mc[k] = umin(PM[k], Dc[k]);
                    Ic[k] = INF;
                }
            } else {
                const bool open_always = (meta.flags & ROW_OPENI_ALWAYS) != 0;
                const bool open_never = (meta.flags & ROW_OPENI_NEVER) != 0;
                const uint32_t csym = meta.child_sym;
                uint32_t H[C], Tq[Q];
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
                // the insertion value entering column sbase.  Pass 1 carries it between the strips.  Pass 2 has the previous
                // strip's cells of this row in the window: I[sbase] = min(I[sbase - 1] + e, open ? H[sbase - 1] + oe : INF), and
                // M = min(H, I) may stand for H there because I + oe >= I + e
                uint32_t cq = INF;
                if (from_prev) {
                    if (PASS == 1) cq = cin_row[2 * r];
                    else {
                        const uint32_t il = IO::get(R.win_i + (uint64_t)lr * pitch + sbase - 1);
                        const uint32_t ml = IO::get(R.win_m + (uint64_t)lr * pitch + sbase - 1);
                        const bool op = !open_never && (open_always || q_edge != csym);
                        cq = umin(sat_add(il, e), op ? sat_add(ml, oe) : INF);
                    }
                }
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
                if (PASS == 1 && to_next && lane == 0) cout_row[2 * r] = cq;  // I[r][(s + 1) * W]
#pragma unroll
                for (int k = 0; k < C; ++k) Mc[k] = umin(H[k], Ic[k]);
            }
            const uint32_t cb = sbase + K * lane;
            if (PASS == 1) {
                if (to_next && lane == 63) cout_row[2 * r + 1] = Mc[C - 1];  // M[r][(s + 1) * W - 1]
                const uint32_t my_slot = P.slot[r];
                if (my_slot != SWEEP_NO_SLOT) {
                    const uint64_t sb = (uint64_t)my_slot * pitch + cb;
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        if (act[m]) {
                            IO::store(R.slot_m + sb + m * QW, &Mc[K * m]);
                            IO::store(R.slot_d + sb + m * QW, &Dc[K * m]);
                        }
                    }
                }
                // the snapshots this row belongs to (none for almost every row of a chain-like graph)
                const uint32_t se = P.snap_off[r + 1];
                for (uint32_t si = P.snap_off[r]; si < se; ++si) {
                    const uint64_t sb = (uint64_t)P.snap_dst[si] * pitch + cb;
#pragma unroll
                    for (int m = 0; m < Q; ++m) {
                        if (act[m]) {
                            IO::store(R.snap_m + sb + m * QW, &Mc[K * m]);
                            IO::store(R.snap_d + sb + m * QW, &Dc[K * m]);
                        }
                    }
                }
                if (r + 1 == P.n_rows && L >= sbase && L < sbase + W) {
                    uint32_t v = INF;
#pragma unroll
                    for (int m = 0; m < Q; ++m)
#pragma unroll
                        for (int k = 0; k < K; ++k)
                            if (sbase + m * QW + K * lane + k == L) v = Mc[K * m + k];
                    const uint32_t owner = ((L - sbase) % QW) / K;
                    if (lane == owner) P.score[qi] = (sizeof(T) == 2 && v >= 0xFFFFu) ? INF : v;
                }
            } else {
                const uint64_t wb = (uint64_t)lr * pitch + cb;
#pragma unroll
                for (int m = 0; m < Q; ++m) {
                    if (act[m]) {
                        IO::store(R.win_m + wb + m * QW, &Mc[K * m]);
                        IO::store(R.win_i + wb + m * QW, &Ic[K * m]);
                        IO::store(R.win_d + wb + m * QW, &Dc[K * m]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < C; ++k) { Mprev[k] = Mc[k]; Dprev[k] = Dc[k]; }
        }
        // pass 1: the carries of this strip; pass 2: the window cells of this strip, read by the next through other lanes
        if (n_strips > 1) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
}

template <int Q, typename T>
__global__ __launch_bounds__(256) void poa_ckpt_sweep_kernel(CkptParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wq = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave-uniform
    if (wq >= P.n_queries) return;
    const uint32_t qi = P.first_query + wq;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    const uint32_t pitch = P.pitch[qi];
    const CkptRegion<T> R(P, qi, pitch);
    ckpt_rows<Q, T, 1>(P, R, qi, wq, lane, 0u, P.n_rows, pitch, L, P.qseq + qbeg);
}

// ---------------------------------------------------------------------------------------------------------------------
// The walk: tb_step of poa_kernels.hpp, full-plane form, over a window and a snapshot.
template <typename T>
struct CkptCells {
    using IO = PlaneIO<T>;
    const RowMeta* rows;
    const uint32_t* pred_rows;
    const uint32_t* pred_src;
    const T *win_m, *win_i, *win_d, *snap_m, *snap_d;
    const uint8_t* q;
    uint32_t b0, pitch, L, x, o, e;
    __device__ __forceinline__ uint32_t m(uint32_t row, uint32_t j) const { return IO::get(win_m + (uint64_t)(row - b0) * pitch + j); }
    __device__ __forceinline__ uint32_t i(uint32_t row, uint32_t j) const { return IO::get(win_i + (uint64_t)(row - b0) * pitch + j); }
    __device__ __forceinline__ uint32_t d(uint32_t row, uint32_t j) const { return IO::get(win_d + (uint64_t)(row - b0) * pitch + j); }
    // M / D of a predecessor, by the place pred_src gives for its edge
    __device__ __forceinline__ uint32_t pm(uint32_t loc, uint32_t j) const {
        return IO::get(((loc & CKPT_SNAP) ? snap_m : win_m) + (uint64_t)(loc & ~CKPT_SNAP) * pitch + j);
    }
    __device__ __forceinline__ uint32_t pd(uint32_t loc, uint32_t j) const {
        return IO::get(((loc & CKPT_SNAP) ? snap_d : win_d) + (uint64_t)(loc & ~CKPT_SNAP) * pitch + j);
    }
};

template <typename T>
__device__ inline TbStep ckpt_step(const CkptCells<T>& c, uint32_t row, uint32_t j, uint32_t st, uint32_t& n_cand, bool& bad, bool& panic) {
    TbStep first{0, 0, 0, false, 0, 0};
    n_cand = 0;
    const RowMeta m = c.rows[row];
    first.node = m.node;
    const bool is_end = (m.flags & ROW_END) != 0;
    auto sub = [&](uint32_t a, uint32_t b) { uint32_t r = a - b; if (r == INF) panic = true; return r; };
    auto cand = [&](uint32_t r2, uint32_t j2, uint32_t s2) {
        if (!first.found) { first.row = r2; first.j = j2; first.st = s2; first.found = true; }
        n_cand++;
    };
    if (st == 0) {
        const uint32_t cs = c.m(row, j), dv = c.d(row, j), iv = c.i(row, j);
        first.cs = cs;
        if (cs == INF) return first;
        if (j > 0) {
            const bool moe = is_end || ((uint32_t)m.sym == (uint32_t)c.q[j - 1]);
            const uint32_t pj = is_end ? j : j - 1;   // the end row reads its predecessor at the SAME column
            // the reference evaluates `curr_score - mismatch` per predecessor: never for a row without predecessors
            const uint32_t target = (moe || m.pred_count == 0) ? cs : sub(cs, c.x);
            for (uint32_t pe0 = 0; pe0 < m.pred_count; pe0 += 4) {
                uint32_t prs[4], loc[4], vals[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    prs[b] = (pe0 + b < m.pred_count) ? c.pred_rows[m.pred_begin + pe0 + b] : 0u;
                    loc[b] = (pe0 + b < m.pred_count) ? c.pred_src[m.pred_begin + pe0 + b] : 0u;
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) vals[b] = (pe0 + b < m.pred_count) ? c.pm(loc[b], pj) : INF;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (pe0 + b < m.pred_count && vals[b] == target) cand(prs[b], pj, 0);
            }
        }
        if (dv == cs) cand(row, j, 1);
        if (iv == cs) cand(row, j, 2);
    } else if (st == 1) {
        const uint32_t cs = c.d(row, j);
        first.cs = cs;
        if (cs == INF) return first;
        if (m.pred_count == 0) return first;
        const uint32_t t_open = sub(sub(cs, c.o), c.e), t_ext = sub(cs, c.e);
        const bool real_open = !is_end && (j >= c.L || (uint32_t)m.sym != (uint32_t)c.q[j]);
        for (uint32_t pe0 = 0; pe0 < m.pred_count; pe0 += 4) {
            uint32_t prs[4], loc[4], vals[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                prs[b] = (pe0 + b < m.pred_count) ? c.pred_rows[m.pred_begin + pe0 + b] : 0u;
                loc[b] = (pe0 + b < m.pred_count) ? c.pred_src[m.pred_begin + pe0 + b] : 0u;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) vals[b] = (pe0 + b < m.pred_count) ? c.pm(loc[b], j) : INF;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (pe0 + b >= m.pred_count) continue;
                if (vals[b] == t_open) cand(prs[b], j, 0);
                else if (!real_open && vals[b] < t_open) bad = true;  // phantom edge the reference does not re-check
            }
        }
        for (uint32_t pe0 = 0; pe0 < m.pred_count; pe0 += 4) {
            uint32_t prs[4], loc[4], vals[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                prs[b] = (pe0 + b < m.pred_count) ? c.pred_rows[m.pred_begin + pe0 + b] : 0u;
                loc[b] = (pe0 + b < m.pred_count) ? c.pred_src[m.pred_begin + pe0 + b] : 0u;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) vals[b] = (pe0 + b < m.pred_count) ? c.pd(loc[b], j) : INF;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (pe0 + b < m.pred_count && vals[b] == t_ext) cand(prs[b], j, 1);
        }
    } else {
        const uint32_t cs = c.i(row, j);
        first.cs = cs;
        if (cs == INF) return first;
        if (j > 0) {
            const uint32_t t_open = sub(sub(cs, c.o), c.e), t_ext = sub(cs, c.e);
            const uint32_t pm = c.m(row, j - 1), pi = c.i(row, j - 1);
            bool open_i = j - 1 < c.L;   // tb_open_i
            if (open_i && !(m.flags & ROW_OPENI_ALWAYS)) open_i = !(m.flags & ROW_OPENI_NEVER) && (uint32_t)m.child_sym != (uint32_t)c.q[j - 1];
            if (pm == t_open) cand(row, j - 1, 0);
            else if (!open_i && pm < t_open) bad = true;
            if (pi == t_ext) {
                const bool only = (n_cand == 0);
                cand(row, j - 1, 0);  // sic: the reference returns Match here (gap_affine.rs:649)
                if (only && pm != t_ext) bad = true;  // the hop lands on M[row][j-1] which is not that I value
            }
        }
    }
    return first;
}

// Pass 2 of one query, by its wave: the driver of the walk, shared by poa_ckpt_trace_kernel and poa_ckpt_trace_multi_kernel
// (poa_multi.hpp).  `wq` places the query's strip carries (ckpt_rows).
template <int Q, typename T>
__device__ __forceinline__ void ckpt_trace_query(const CkptParams& P, const uint32_t qi, const uint32_t wq, const uint32_t lane) {
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    const uint8_t* __restrict__ q = P.qseq + qbeg;
    const uint32_t pitch = P.pitch[qi];
    const CkptRegion<T> R(P, qi, pitch);
    uint2* out = P.scratch + P.scratch_off[qi];
    const uint32_t cap = (uint32_t)(P.scratch_off[qi + 1] - P.scratch_off[qi]);
    auto emit_at = [&](uint32_t pos, uint32_t rpos, uint32_t qpos) {
        if (pos < cap) out[cap - 1 - pos] = make_uint2(rpos, qpos);
    };
    const uint32_t end_node = P.rows[P.end_row].node;

    // the walk's state, wave-uniform between the segments
    uint32_t crow = P.end_row, cj = L, cst = 0, cnt = 0, flags = 0;
    uint32_t done = 0, reached_start = 0, first_hop = 1;
    if (L == 0) { done = 1; reached_start = 1; }
    else if (L == 1) {
        // gap_affine.rs:812-824: "single nucleotide perfect match"; the end node equals every symbol: [(end, 0)]
        flags |= POA_FLAG_SHORT_QUERY;
        if (lane == 0) emit_at(0, end_node, 0);
        cnt = 1; done = 1; reached_start = 1;
    }
    uint32_t seg = P.n_segments - 1;
    while (!done) {
        while (crow < P.boundary[seg]) --seg;   // (segments the walk jumped over are not recomputed)
        const uint32_t b0 = P.boundary[seg], b1 = P.boundary[seg + 1];
        ckpt_rows<Q, T, 2>(P, R, qi, wq, lane, b0, b1, pitch, L, q);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");   // lane 0 reads what all lanes stored
        uint32_t w_row = crow, w_j = cj, w_st = cst, w_cnt = cnt, w_flags = flags, w_done = 0, w_reached = 0;
        if (lane == 0) {
            CkptCells<T> c;
            c.rows = P.rows; c.pred_rows = P.pred_rows; c.pred_src = P.pred_src;
            c.win_m = R.win_m; c.win_i = R.win_i; c.win_d = R.win_d; c.snap_m = R.snap_m; c.snap_d = R.snap_d;
            c.q = q; c.b0 = b0; c.pitch = pitch; c.L = L; c.x = P.cost_x; c.o = P.cost_o; c.e = P.cost_e;
            if (first_hop) {
                // first hop from the end cell: Match, .or_else(Insertion), .or_else(Deletion) (gap_affine.rs:832-835)
                uint32_t nc, fallback = 0;
                bool bad = false, pn = false;
                TbStep cur = ckpt_step<T>(c, w_row, w_j, 0, nc, bad, pn);
                if (cur.found && !pn && (nc != 1 || bad)) w_flags |= POA_FLAG_AMBIGUOUS;
                if (!cur.found && !pn) {
                    cur = ckpt_step<T>(c, w_row, w_j, 2, nc, bad, pn);
                    if (!cur.found && !pn) cur = ckpt_step<T>(c, w_row, w_j, 1, nc, bad, pn);
                    // no backtrace from the end cell: the reference builds a 'simple alignment' for len <= 3 and panics otherwise
                    if (!pn) {
                        if (!cur.found) { w_flags |= POA_FLAG_REF_PANIC; fallback = 1; }
                        else w_flags |= POA_FLAG_AMBIGUOUS;
                    }
                }
                // a Score subtraction wrapped onto u32::MAX: the reference dies here, nothing is emitted
                if (pn) { w_flags |= POA_FLAG_REF_PANIC; fallback = 2; }
                if (fallback) {
                    if (fallback == 2) w_flags |= POA_FLAG_TRUNCATED;
                    if (fallback == 1 && L <= 3) {
                        for (uint32_t k = 0; k < L; ++k) emit_at(k, end_node, L - 1 - k);
                        w_cnt = L;
                    }
                    w_done = 1; w_reached = 1;   // (nothing more to truncate)
                } else {
                    w_row = cur.row; w_j = cur.j; w_st = cur.st;
                }
            }
            while (!w_done && w_row >= b0) {
                uint32_t nc;
                bool bad = false, pn = false;
                const TbStep bt = ckpt_step<T>(c, w_row, w_j, w_st, nc, bad, pn);
                // a Score subtraction that wraps onto u32::MAX kills the reference at that step
                if (pn) { w_flags |= POA_FLAG_REF_PANIC; w_done = 1; break; }
                if (!bt.found) { w_done = 1; break; }
                if (nc != 1 || bad) w_flags |= POA_FLAG_AMBIGUOUS;
                if (w_st == 0 && bt.st != 0) {  // zero-cost gap close: no pair (gap_affine.rs:871-875)
                    w_row = bt.row; w_j = bt.j; w_st = bt.st;
                    continue;
                }
                if (w_st == 0) emit_at(w_cnt, bt.node, w_j - 1);
                else if (w_st == 2) emit_at(w_cnt, POA_NONE, w_j - 1);
                else emit_at(w_cnt, bt.node, POA_NONE);
                w_cnt += 1;
                if (bt.st == 0 && bt.j == 0 && bt.row != P.start_row && w_st != 1 && (uint32_t)P.rows[bt.row].sym == (uint32_t)q[0])
                    w_flags |= POA_FLAG_START_QUIRK;
                if (bt.row == P.start_row) { w_reached = 1; w_done = 1; break; }
                w_row = bt.row; w_j = bt.j; w_st = bt.st;
            }
        }
        crow = wave_uni(w_row); cj = wave_uni(w_j); cst = wave_uni(w_st); cnt = wave_uni(w_cnt); flags = wave_uni(w_flags);
        done = wave_uni(w_done); reached_start = wave_uni(w_reached);
        first_hop = 0;
    }
    if (!reached_start) flags |= POA_FLAG_TRUNCATED;
    if (lane == 0) {
        P.flags[qi] = flags;
        P.n_pairs[qi] = cnt < cap ? cnt : cap;
    }
}

// At least three waves per SIMD: every instantiation meets that, <4, uint32_t> with exactly the 168 VGPRs it allows, and without
// the floor the register allocator settles it at 184 or at 168 by the order of unrelated statements (profiles/pr_ckpt_walk/).
// The floor binds all five: a change that pushes <2, uint16_t> (166 VGPRs) or <4, uint32_t> past 168 no longer drops a wave, it
// spills to scratch without a word.  `make resources` (csrc/Makefile) shows it: ScratchSize must stay 0 for these kernels.
template <int Q, typename T>
__global__ __launch_bounds__(256, 3) void poa_ckpt_trace_kernel(CkptParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wq = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave-uniform
    if (wq >= P.n_queries) return;
    ckpt_trace_query<Q, T>(P, P.first_query + wq, wq, lane);
}

}  // namespace poa_amd
