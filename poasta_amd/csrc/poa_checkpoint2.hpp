// Checkpointed alignment under the two-piece affine model (POA_MODE_CHECKPOINT2) for gfx950: what the dense two-piece pass
// returns — score, pairs, certificate flags — from a workspace of O(segments x live rows + segment length) plane rows per
// query instead of five planes of all rows.  Included by poa_engine.hip after poa_twopiece.hpp.
//
// The segment plan is the one-piece mode's (CheckpointPlan, poa_sweep_rows.hpp) with the two-piece weights.  Two kernels, one
// wavefront per query in both, no communication between waves:
//
//   pass 1, poa2_ckpt_sweep_kernel: the recurrences of poa2_forward_kernel (tp_row_pass of poa_twopiece.hpp: one body for
//     both) over all rows with its column mapping — K columns per lane, 64 K per pass, I1 and I2 as the in-lane chain plus one wave scan per pass, carries between
//     passes in registers, the previous row in registers for chain rows.  M, D1 and D2 of a slotted row go to its slot, every
//     row listed in snap_off / snap_dst to its snapshot rows; I1 and I2 never leave their row.  It yields the score.
//   pass 2, poa2_ckpt_trace_kernel: from the last segment to the first, recompute the segment's five planes into a window of
//     max_segment rows — predecessors from registers, the window or the snapshot, by pred_src per edge — then walk inside the
//     window until the walk steps to a row before the segment.  The walk's state survives in registers to the segment that
//     holds that row; segments the walk jumps over are not recomputed.
//
// A query wider than one strip (NP passes: 1024 columns) is swept strip after strip, as the one-piece sweep does it: what a
// row hands to the next strip — I1 and I2 entering its first column, M of its last column — goes through `carry`, two
// parities of three words per row.  (Unlike the one-piece window, M of the window cannot stand for H when I1 is rebuilt at a
// strip's edge: M may be an I2 value, and I2 + open is not bounded below by I1 + extend1.)
//
// The walk is tp_step / tp_walk_begin / tp_walk_run of poa_twopiece.hpp, the code poa2_traceback_kernel runs, behind an
// addressing policy that finds a predecessor through its EDGE (pred_src: window row or snapshot row).
//
// Memory of a query, in cells of T (u16 under the bound the dense two-piece run uses, else u32), rows of `pitch` cells:
//   [slot M | D1 | D2 : n_slots each][snapshot M | D1 | D2 : n_snap each][window M | I1 | D1 | I2 | D2 : seg each]
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_forward_sweep.hpp"
#include "poa_sweep_rows.hpp"

namespace poa_amd {

struct Ckpt2Params {
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
    uint32_t* carry;            // [n_queries_in_chunk][2 parities][n_rows][3]; read only by a query wider than one strip
    uint32_t x, oe, o1, e1, e2;
    const uint64_t* scratch_off;  // [total + 1] per-query region in `scratch` (capacity len + n_rows)
    poa_aln_pair_t* scratch;      // pairs written from the BACK of each region
    uint32_t* score;              // [total]
    uint32_t* flags;              // [total]
    uint32_t* n_pairs;            // [total]
};

template <typename T>
struct Ckpt2Region {
    T *slot[3], *snap[3];   // M, D1, D2
    T* win[5];              // M, I1, D1, I2, D2: the plane order of the walk's states
    __device__ __forceinline__ Ckpt2Region(const Ckpt2Params& P, uint32_t qi, uint32_t pitch) {
        T* p = reinterpret_cast<T*>(P.planes) + P.plane_off[qi];
        for (int k = 0; k < 3; ++k) { slot[k] = p; p += (uint64_t)P.n_slots * pitch; }
        for (int k = 0; k < 3; ++k) { snap[k] = p; p += (uint64_t)P.n_snap * pitch; }
        for (int k = 0; k < 5; ++k) { win[k] = p; p += (uint64_t)P.seg_rows * pitch; }
    }
};

// Rows [r0, r1) of one query, strip after strip.  PASS 1: the whole graph, slots + snapshots.  PASS 2: one segment, window.
template <typename T, int NP, int PASS>
__device__ __forceinline__ void ckpt2_rows(const Ckpt2Params& P, const Ckpt2Region<T>& R, const uint32_t qi, const uint32_t wq,
                                           const uint32_t lane, const uint32_t r0, const uint32_t r1, const uint32_t pitch,
                                           const uint32_t L, const uint8_t* q) {
    using IO = PlaneIO<T>;
    constexpr int K = IO::K;
    constexpr uint32_t PW = 64 * K;    // columns per pass
    constexpr uint32_t W = PW * NP;    // columns per strip
    constexpr uint32_t INF = 0xFFFFFFFFu;
    const uint32_t n_pass = (L + 1 + PW - 1) / PW;   // pitch is a multiple of 64: a pass may end inside the row's padding
    const uint32_t n_strips = (n_pass + NP - 1) / NP;
    uint32_t* carry = P.carry + 6ull * wq * P.n_rows;
    const TpPassCosts PC{P.x, P.oe, P.e1, P.e2};

    for (uint32_t s = 0; s < n_strips; ++s) {
        const uint32_t sbase = s * W;
        const uint32_t* cin = carry + (uint64_t)((s + 1u) & 1u) * 3u * P.n_rows;   // written by strip s - 1
        uint32_t* cout = carry + (uint64_t)(s & 1u) * 3u * P.n_rows;
        const bool from_prev = s > 0, to_next = s + 1 < n_strips;
        uint32_t keepM[NP][K], keepD1[NP][K], keepD2[NP][K];   // M, D1, D2 of the previous row, my columns of every pass
#pragma unroll
        for (int ps = 0; ps < NP; ++ps)
#pragma unroll
            for (int k = 0; k < K; ++k) { keepM[ps][k] = INF; keepD1[ps][k] = INF; keepD2[ps][k] = INF; }

        for (uint32_t r = r0; r < r1; ++r) {
            const RowMeta rm = P.rows[r];
            const bool is_end = r == P.end_row, is_start = r == P.start_row;
            const uint32_t lr = r - r0;   // PASS 2: the row's place in the window
            const bool from_regs = (rm.flags & ROW_CHAIN) && r > r0;
            uint32_t c1 = INF, c2 = INF;   // I1 / I2 entering the first column of the pass
            uint32_t cpm = INF;            // min over predecessors of M[p][first column of the pass - 1]
            if (from_prev) {
                c1 = cin[3 * r]; c2 = cin[3 * r + 1];
                if (from_regs) cpm = PASS == 1 ? cin[3 * (r - 1) + 2] : IO::get(R.win[0] + (uint64_t)(lr - 1) * pitch + sbase - 1);
                else
                    for (uint32_t e = 0; e < rm.pred_count; ++e) {
                        uint32_t v;
                        if (PASS == 1) v = cin[3 * P.pred_rows[rm.pred_begin + e] + 2];
                        else {
                            const uint32_t loc = P.pred_src[rm.pred_begin + e];
                            v = IO::get(((loc & CKPT_SNAP) ? R.snap[0] : R.win[0]) + (uint64_t)(loc & ~CKPT_SNAP) * pitch + sbase - 1);
                        }
                        cpm = min(cpm, v);
                    }
            }
            uint32_t edge_m = INF;   // lane 63: M of the strip's last column
            const uint32_t my_slot = PASS == 1 ? P.slot[r] : SWEEP_NO_SLOT;
            const uint32_t sn0 = PASS == 1 ? P.snap_off[r] : 0u, sn1 = PASS == 1 ? P.snap_off[r + 1] : 0u;
            auto do_pass = [&](const uint32_t ps, uint32_t (&kM)[K], uint32_t (&kD1)[K], uint32_t (&kD2)[K]) {
                const uint32_t j = sbase + ps * PW + K * lane;   // my first column
                const bool in = j < pitch;                       // (whole 16-byte groups lie inside or outside the plane row)
                const bool first = sbase == 0 && ps == 0;
                uint32_t pm[K], pd[K], pd2[K];
#pragma unroll
                for (int k = 0; k < K; ++k) { pm[k] = INF; pd[k] = INF; pd2[k] = INF; }
                if (from_regs) {
#pragma unroll
                    for (int k = 0; k < K; ++k) { pm[k] = kM[k]; pd[k] = kD1[k]; pd2[k] = kD2[k]; }
                } else if (in)
                    for (uint32_t e = 0; e < rm.pred_count; ++e) {
                        const T *bm, *bd1, *bd2;
                        if (PASS == 1) {
                            const uint64_t po = (uint64_t)P.pred_slot[rm.pred_begin + e] * pitch + j;
                            bm = R.slot[0] + po; bd1 = R.slot[1] + po; bd2 = R.slot[2] + po;
                        } else {
                            const uint32_t loc = P.pred_src[rm.pred_begin + e];
                            const uint64_t po = (uint64_t)(loc & ~CKPT_SNAP) * pitch + j;
                            if (loc & CKPT_SNAP) { bm = R.snap[0] + po; bd1 = R.snap[1] + po; bd2 = R.snap[2] + po; }
                            else { bm = R.win[TP_SM] + po; bd1 = R.win[TP_SD] + po; bd2 = R.win[TP_SD2] + po; }
                        }
                        uint32_t a[K], b[K], c[K];
                        IO::load(bm, a); IO::load(bd1, b); IO::load(bd2, c);
#pragma unroll
                        for (int k = 0; k < K; ++k) { pm[k] = min(pm[k], a[k]); pd[k] = min(pd[k], b[k]); pd2[k] = min(pd2[k], c[k]); }
                    }
                uint32_t m[K], v1[K], d1[K], v2[K], d2[K];
                tp_row_pass<K>(PC, rm, is_end, is_start, first, j, L, lane, q, pm, pd, pd2, cpm, c1, c2, m, v1, d1, v2, d2);
                if (in) {
                    if (PASS == 1) {
                        if (my_slot != SWEEP_NO_SLOT) {
                            const uint64_t so = (uint64_t)my_slot * pitch + j;
                            IO::store(R.slot[0] + so, m); IO::store(R.slot[1] + so, d1); IO::store(R.slot[2] + so, d2);
                        }
                        // the snapshots this row belongs to (none for almost every row of a chain-like graph)
                        for (uint32_t si = sn0; si < sn1; ++si) {
                            const uint64_t so = (uint64_t)P.snap_dst[si] * pitch + j;
                            IO::store(R.snap[0] + so, m); IO::store(R.snap[1] + so, d1); IO::store(R.snap[2] + so, d2);
                        }
                        if (is_end && L >= j && L < j + K) {
                            uint32_t v = INF;
#pragma unroll
                            for (int k = 0; k < K; ++k)
                                if (j + k == L) v = m[k];
                            P.score[qi] = (sizeof(T) == 2 && v >= 0xFFFFu) ? INF : v;   // what a stored cell reads back as
                        }
                    } else {
                        const uint64_t wo = (uint64_t)lr * pitch + j;
                        IO::store(R.win[TP_SM] + wo, m); IO::store(R.win[TP_SI] + wo, v1); IO::store(R.win[TP_SD] + wo, d1);
                        IO::store(R.win[TP_SI2] + wo, v2); IO::store(R.win[TP_SD2] + wo, d2);
                    }
#pragma unroll
                    for (int k = 0; k < K; ++k) { kM[k] = m[k]; kD1[k] = d1[k]; kD2[k] = d2[k]; }
                    edge_m = m[K - 1];
                } else {
#pragma unroll
                    for (int k = 0; k < K; ++k) { kM[k] = INF; kD1[k] = INF; kD2[k] = INF; }
                    edge_m = INF;
                }
            };
#pragma unroll
            for (int ps = 0; ps < NP; ++ps)
                if (s * NP + (uint32_t)ps < n_pass) do_pass((uint32_t)ps, keepM[ps], keepD1[ps], keepD2[ps]);
            if (to_next) {   // (every pass of such a strip ran: edge_m is M[r][sbase + W - 1] in lane 63)
                if (lane == 0) { cout[3 * r] = c1; cout[3 * r + 1] = c2; }
                if (lane == 63) cout[3 * r + 2] = edge_m;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the next rows read this one back (same wave)
        }
        // the carries of this strip and its window cells, read by the next strip through other lanes
        if (n_strips > 1) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
}

template <typename T, int NP>
__global__ __launch_bounds__(64) void poa2_ckpt_sweep_kernel(Ckpt2Params P) {
    const uint32_t lane = threadIdx.x, wq = blockIdx.x;
    const uint32_t qi = P.first_query + wq;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    const uint32_t pitch = P.pitch[qi];
    const Ckpt2Region<T> R(P, qi, pitch);
    ckpt2_rows<T, NP, 1>(P, R, qi, wq, lane, 0u, P.n_rows, pitch, L, P.qseq + qbeg);
}

// The walk's addressing policy (poa_twopiece.hpp) over a window and a snapshot.
template <typename T>
struct Ckpt2Cells {
    using IO = PlaneIO<T>;
    const T* win;            // window planes M, I1, D1, I2, D2: the walk's state is the plane index
    const T* snap;           // snapshot planes M, D1, D2
    uint64_t win_plane, snap_plane;   // cells per plane
    const uint32_t* pred_src;
    uint32_t b0, pitch;
    __device__ __forceinline__ uint32_t at(uint32_t row, uint32_t j, uint32_t st) const { return IO::get(win + st * win_plane + (uint64_t)(row - b0) * pitch + j); }
    // M / D1 / D2 of a predecessor, by the place pred_src gives for its edge
    __device__ __forceinline__ uint32_t pred(uint32_t e, uint32_t, uint32_t j, uint32_t st) const {
        const uint32_t loc = pred_src[e];
        const T* base = (loc & CKPT_SNAP) ? snap + (st == TP_SM ? 0u : (st == TP_SD ? 1u : 2u)) * snap_plane : win + st * win_plane;
        return IO::get(base + (uint64_t)(loc & ~CKPT_SNAP) * pitch + j);
    }
    __device__ __forceinline__ uint32_t up(const RowMeta& rm, uint32_t v, uint32_t j) const {
        return ((rm.flags & ROW_CHAIN) && rm.pred_count > 0 && j > 0) ? pred(rm.pred_begin, v - 1, j - 1, TP_SM) : 0xFFFFFFFFu;
    }
};

// Pass 2 of one query, by its wave: the driver of the walk, shared by poa2_ckpt_trace_kernel and poa2_ckpt_trace_multi_kernel
// (poa_multi.hpp).  `wq` places the query's strip carries (ckpt2_rows).
template <typename T, int NP>
__device__ __forceinline__ void ckpt2_trace_query(const Ckpt2Params& P, const uint32_t qi, const uint32_t wq, const uint32_t lane) {
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    const uint8_t* q = P.qseq + qbeg;
    const uint32_t pitch = P.pitch[qi];
    const Ckpt2Region<T> R(P, qi, pitch);
    TpWalkCtx W;
    W.rows = P.rows; W.pred_rows = P.pred_rows; W.q = q; W.L = L; W.start_row = P.start_row; W.end_row = P.end_row;
    W.x = P.x; W.o1 = P.o1; W.e1 = P.e1; W.e2 = P.e2;
    W.out = P.scratch + P.scratch_off[qi];
    W.cap = (uint32_t)(P.scratch_off[qi + 1] - P.scratch_off[qi]);

    // the walk's state, wave-uniform between the segments
    TpWalk S{P.end_row, L, TP_SM, 0, 0, false, false};
    bool first_hop = true;
    uint32_t seg = P.n_segments - 1;
    while (!S.done) {
        while (S.row < P.boundary[seg]) --seg;   // (segments the walk jumped over are not recomputed)
        const uint32_t b0 = P.boundary[seg], b1 = P.boundary[seg + 1];
        if (L > 1) {   // (a query of at most one symbol is answered from the row records alone)
            ckpt2_rows<T, NP, 2>(P, R, qi, wq, lane, b0, b1, pitch, L, q);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");   // lane 0 reads what all lanes stored
        }
        TpWalk Wk = S;
        if (lane == 0) {
            Ckpt2Cells<T> C;
            C.win = R.win[0]; C.snap = R.snap[0];
            C.win_plane = (uint64_t)P.seg_rows * pitch; C.snap_plane = (uint64_t)P.n_snap * pitch;
            C.pred_src = P.pred_src; C.b0 = b0; C.pitch = pitch;
            if (first_hop) tp_walk_begin(W, C, Wk, P.end_row, L, POA_FLAG_SHORT_QUERY);
            tp_walk_run(W, C, Wk, b0);
        }
        S.row = wave_uni(Wk.row); S.j = wave_uni(Wk.j); S.st = wave_uni(Wk.st); S.n_out = wave_uni(Wk.n_out); S.fl = wave_uni(Wk.fl);
        S.done = wave_uni(Wk.done ? 1u : 0u) != 0; S.reached_start = wave_uni(Wk.reached_start ? 1u : 0u) != 0;
        first_hop = false;
    }
    if (lane == 0) {
        P.flags[qi] = tp_walk_flags(S);
        P.n_pairs[qi] = S.n_out < W.cap ? S.n_out : W.cap;
    }
}

template <typename T, int NP>
__global__ __launch_bounds__(64) void poa2_ckpt_trace_kernel(Ckpt2Params P) {
    const uint32_t lane = threadIdx.x, wq = blockIdx.x;
    ckpt2_trace_query<T, NP>(P, P.first_query + wq, wq, lane);
}

}  // namespace poa_amd
