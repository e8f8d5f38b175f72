// Two-piece affine model (/root/reference/src/aligner/scoring/gap_affine_2piece.rs): the dense pass.
// Included by poa_engine.hip (uses its poa_graph, DevBuf, HIP_TRY, fail).
//
// Edge set (gap_affine_2piece.rs:292-516; the tests hold a CPU restatement as the executable specification): a gap opens in the
// first piece exactly as in the one-piece model (open1 + extend1, greedy-match rule), every further step stays in its
// piece or moves from the first to the second at extend2; open2 is never charged.  Five planes per query:
//
//   D1[v][j] = min( PD1[j] + e1 , openD(v,j) ? PM[j] + o1 + e1 : INF )        PM / PD1 / PD2 = min over predecessors
//   D2[v][j] = min( PD1[j], PD2[j] ) + e2
//   H [v][j] = min( PM[j-1] + (mismatch ? x : 0) , D1, D2 )                    H[start][0] = 0
//   I1[v][j+1] = min( I1[v][j] + e1 , openI(v,j) ? H[v][j] + o1 + e1 : INF )   min-plus prefix scan, decay e1
//   I2[v][j+1] = min( I1[v][j], I2[v][j] ) + e2                                min-plus prefix scan over I1, decay e2
//   M [v][j] = min( H, I1, I2 )                                                end row: no I, D1 only by extension
//
// One wavefront per query, rows in topological order, four columns per lane and 256 per pass with the scan carries kept in
// registers; predecessor rows are re-read from the planes (just written by this wave: L2).  u32 arithmetic, INF absorbing.
// This is the u32 kernel of the model (20 bytes written per cell: HBM-bound territory); the packed-u16 pairs-across-quads
// mapping of the one-piece kernels carries over (two more packed recurrences per register) and is the next step for it.
// Traceback: the reference's rule (gap_affine_2piece.rs:639-794, :944-1043) on the five planes with the same uniqueness
// certificate as the one-piece pass; one lane per query (a chain of dependent reads; the speculative walk of
// poa_traceback_kernel is not ported to five planes yet).
#pragma once

namespace poa_amd {

// Every query has its own pitch, its planes at plane_off[qi] of the batch's workspace and its pairs at scratch_off[qi] of the
// batch's scratch, as the one-piece kernels take them (FwdParams / TbParams).
struct TwoPieceParams {
    const RowMeta* rows;
    const uint32_t* pred_rows;
    uint32_t n_rows, start_row, end_row;
    const uint8_t* qseq;
    const uint64_t* qoff;
    uint32_t first_query, n_queries;   // chunk
    uint32_t* planes;                  // per query: [5][n_rows][pitch] of the kernel's plane type (u32, or u16 when every score that matters fits): M, I1, D1, I2, D2
    const uint32_t* q_pitch;           // [total] columns per plane row (multiple of 64)
    const uint64_t* plane_off;         // [total] offset of the query's five planes, in units of off_scale plane elements
    uint32_t off_scale;                // plane elements per unit of plane_off (2: u16 planes under the batch's 4-byte plan)
    uint32_t x, oe, e1, e2, o1;
    uint32_t* score;                   // [total]
    uint32_t* flags;                   // [total]
    uint32_t* n_pairs;                 // [total]
    poa_aln_pair_t* scratch;
    const uint64_t* scratch_off;       // [total + 1] per-query region in `scratch` (capacity len + n_rows), written back to front
    // replayed search (poa2_exact_kernel ran on u32 planes): where each walk starts and what became of the search
    uint32_t exact_pass;
    const uint32_t* ex_status;         // [total] EX_*
    const uint32_t* ex_end;            // [2 * total] (row, offset) the search stopped at
};

// where a query's planes and pairs live
__device__ __forceinline__ uint32_t tp_pitch(const TwoPieceParams& P, uint32_t qi) { return P.q_pitch[qi]; }
template <typename T>
__device__ __forceinline__ T* tp_planes(const TwoPieceParams& P, uint32_t qi) {
    return reinterpret_cast<T*>(P.planes) + P.plane_off[qi] * P.off_scale;
}
__device__ __forceinline__ poa_aln_pair_t* tp_out(const TwoPieceParams& P, uint32_t qi, uint32_t& cap) {
    cap = (uint32_t)(P.scratch_off[qi + 1] - P.scratch_off[qi]);
    return P.scratch + P.scratch_off[qi];
}
// pairs reported: clamped to the region as poa_traceback_kernel does (scan and compaction read n_pairs unchecked)
__device__ __forceinline__ uint32_t tp_n_pairs(uint32_t n_out, uint32_t cap) { return n_out < cap ? n_out : cap; }

// Replay of the reference's two-piece search (Affine2PieceMinGapCost / Affine2PieceDijkstra with or without pruning,
// config.rs:160-272; astar.rs:124-226 over gap_affine_2piece.rs): the search object of poa_exact.hpp instantiated with
// EX_AS_TWO_PIECE — the generic code, five plain u32 planes (the layout the traceback below reads), linked-list queue with
// five stacks per priority in the reference's pop order.  One search per lane, `lanes_per_wave` lanes of a wave active.
struct TwoPieceExact {
    ExactGraph G;
    ExactCosts C;
    uint64_t* reached; uint64_t* rsum; uint32_t wpn, swpn;   // per slot: n_exit * wpn / n_exit * swpn words
    uint32_t* head; uint32_t n_prio;                          // per slot: 5 * n_prio
    ExQEntry* pool; uint32_t pool_cap;
    ExStackEntry* stack; uint32_t stack_cap;
    uint32_t* status;        // [total]
    uint32_t* end_cell;      // [2 * total]
    uint32_t* counters;      // [4 * total] num_queued, num_visited, num_pruned, queue entries live at once (high water)
    uint32_t lanes_per_wave;
    uint32_t lds_graph, n_succ, n_nbm;   // 1: the launch carries exact_lds_bytes() of dynamic LDS for the graph arrays
};

constexpr int EXACT2_BLOCK = 1024;   // 16 waves share one LDS copy of the graph

__global__ __launch_bounds__(EXACT2_BLOCK) void poa2_exact_kernel(TwoPieceParams P, TwoPieceExact X) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds2[];
    if (X.lds_graph) { const ExactGraph src = X.G; exact_stage_graph(X.G, src, lds2, X.n_succ, X.n_nbm); }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane >= X.lanes_per_wave) return;
    const uint32_t slot = (blockIdx.x * (EXACT2_BLOCK / 64) + wave) * X.lanes_per_wave + lane;
    if (slot >= P.n_queries) return;
    const uint32_t qi = P.first_query + slot;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    ExactWork W;
    W.T = tp_planes<uint32_t>(P, qi);
    W.n_rows = P.n_rows; W.pitch = tp_pitch(P, qi);
    W.reached = X.reached + (uint64_t)slot * X.G.n_exit * X.wpn;
    W.rsum = X.rsum + (uint64_t)slot * X.G.n_exit * X.swpn;
    W.wpn = X.wpn; W.swpn = X.swpn;
    W.head = X.head + (uint64_t)slot * 5 * X.n_prio; W.n_prio = X.n_prio;
    W.pool = X.pool + (uint64_t)slot * X.pool_cap; W.pool_cap = X.pool_cap;
    W.stack = X.stack + (uint64_t)slot * X.stack_cap; W.stack_cap = X.stack_cap;
    ExactSearchT<EX_AS_NO_SPEC | EX_AS_TWO_PIECE> S(X.G, W, P.qseq + qbeg, L, X.C);
    const ExactResult R = S.run();
    X.status[qi] = R.status;
    X.end_cell[2 * qi] = R.end_row; X.end_cell[2 * qi + 1] = R.end_off;
    X.counters[4 * qi] = R.num_queued; X.counters[4 * qi + 1] = R.num_visited; X.counters[4 * qi + 2] = R.num_pruned;
    X.counters[4 * qi + 3] = S.pool_top;
}

__device__ __forceinline__ uint32_t tp_sat(uint32_t a, uint32_t b) {
    const uint32_t r = a + b;
    return r < a ? 0xFFFFFFFFu : r;
}

// inclusive min-plus scan over the lanes with a constant decay per lane step: out(l) = min over l' <= l of v(l') + (l - l') * step
// (DPP row shifts and broadcasts, no LDS pipe: wave_scan_min_plus of the one-piece kernels)
__device__ __forceinline__ uint32_t tp_scan(uint32_t v, uint32_t step, uint32_t lane) {
    return wave_scan_min_plus(v, step, ((lane & 15u) + 1u) * step, (lane - 31u) * step);
}

// One pass of one row: the recurrences of the header on my K columns from column j, given the minima over the predecessors
// (pm, pd, pd2) — every kernel of the model runs this one body; where the predecessors come from and where the row goes is the
// caller's business (five planes: poa2_forward_kernel; slots, snapshots and a window: poa_checkpoint2.hpp).  cpm, c1, c2 carry
// M of the predecessors' last column, I1 and I2 from pass to pass; `first`: the pass that holds column 0.  Columns past L
// come back INF in all five rows.  Arithmetic is u32 in registers whatever the plane type.
struct TpPassCosts { uint32_t x, oe, e1, e2; };
template <int K>
__device__ __forceinline__ void tp_row_pass(const TpPassCosts& C, const RowMeta& rm, const bool is_end, const bool is_start, const bool first,
                                            const uint32_t j, const uint32_t L, const uint32_t lane, const uint8_t* q,
                                            const uint32_t (&pm)[K], const uint32_t (&pd)[K], const uint32_t (&pd2)[K],
                                            uint32_t& cpm, uint32_t& c1, uint32_t& c2,
                                            uint32_t (&m)[K], uint32_t (&v1)[K], uint32_t (&d1)[K], uint32_t (&v2)[K], uint32_t (&d2)[K]) {
    constexpr uint32_t INF = 0xFFFFFFFFu;
    uint32_t qs[K], qm;                       // q[j + k] (0 past the end: never a symbol), q[j - 1]
#pragma unroll
    for (int k = 0; k < K; ++k) qs[k] = (j + k < L) ? (uint32_t)q[j + k] : 0u;
    qm = (j > 0 && j - 1 < L) ? (uint32_t)q[j - 1] : 0u;
    // M of the predecessors one column to the left of my first column
    const uint32_t pml = wave_shr1(pm[K - 1], cpm);   // lane 0: the last column of the previous pass
    cpm = (uint32_t)__builtin_amdgcn_readlane((int)pm[K - 1], 63);
    uint32_t h[K], a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t col = j + k;
        const bool col_in = col <= L;
        d1[k] = tp_sat(pd[k], C.e1);
        if (!is_end && (col >= L || rm.sym != qs[k])) d1[k] = min(d1[k], tp_sat(pm[k], C.oe));   // openD
        d2[k] = tp_sat(min(pd[k], pd2[k]), C.e2);
        const uint32_t left = k == 0 ? pml : pm[k - 1];
        const uint32_t ql = k == 0 ? qm : qs[k - 1];
        uint32_t diag = INF;
        if (is_end) diag = pm[k];
        else if (col > 0) diag = tp_sat(left, rm.sym != ql ? C.x : 0u);
        h[k] = min(diag, min(d1[k], d2[k]));
        if (is_start && col == 0) h[k] = 0;
        if (!col_in) { h[k] = INF; d1[k] = INF; d2[k] = INF; }
        bool open_i = false;
        if (col < L && !is_end) {
            if (rm.flags & ROW_OPENI_ALWAYS) open_i = true;
            else if (rm.flags & ROW_OPENI_NEVER) open_i = false;
            else open_i = rm.child_sym != qs[k];
        }
        a[k] = open_i ? tp_sat(h[k], C.oe) : INF;   // what column col opens INTO col + 1
    }
    // I1: chain inside the lane with nothing entering, then what enters from the left
    v1[0] = INF;
#pragma unroll
    for (int k = 1; k < K; ++k) v1[k] = min(tp_sat(v1[k - 1], C.e1), a[k - 1]);
    const uint32_t out1 = min(tp_sat(v1[K - 1], C.e1), a[K - 1]);   // leaves my last column towards the next lane
    const uint32_t s1 = tp_scan(out1, K * C.e1, lane);
    uint32_t in1 = wave_shr1(s1, INF);
    in1 = min(in1, tp_sat(c1, lane * K * C.e1));
    if (first && lane == 0) in1 = INF;                              // I1[v][0] = INF
#pragma unroll
    for (int k = 0; k < K; ++k) v1[k] = min(v1[k], tp_sat(in1, (uint32_t)k * C.e1));
    c1 = min((uint32_t)__builtin_amdgcn_readlane((int)s1, 63), tp_sat(c1, 64 * K * C.e1));
    // I2 over the finished I1: I2[c] = min(I1[c-1], I2[c-1]) + e2
    v2[0] = INF;
#pragma unroll
    for (int k = 1; k < K; ++k) v2[k] = tp_sat(min(v2[k - 1], v1[k - 1]), C.e2);
    const uint32_t out2 = tp_sat(min(v2[K - 1], v1[K - 1]), C.e2);
    const uint32_t s2 = tp_scan(out2, K * C.e2, lane);
    uint32_t in2 = wave_shr1(s2, INF);
    in2 = min(in2, tp_sat(c2, lane * K * C.e2));
    if (first && lane == 0) in2 = INF;
#pragma unroll
    for (int k = 0; k < K; ++k) v2[k] = min(v2[k], tp_sat(in2, (uint32_t)k * C.e2));
    c2 = min((uint32_t)__builtin_amdgcn_readlane((int)s2, 63), tp_sat(c2, 64 * K * C.e2));
    if (is_end) {
#pragma unroll
        for (int k = 0; k < K; ++k) { v1[k] = INF; v2[k] = INF; }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        m[k] = min(h[k], min(v1[k], v2[k]));
        if (j + k > L) { m[k] = INF; v1[k] = INF; v2[k] = INF; }   // padding columns read as unvisited
    }
}

// K consecutive columns per lane (4 with u32 planes, 8 with u16), 64 K columns per pass: every plane access is one 16-byte
// load / store per lane, 1 KiB contiguous per wave-instruction; the insertion recurrences run as a K-step chain in the lane
// plus one wave scan per pass and plane (I1 with decay K*e1 per lane, I2 over the finished I1 with decay K*e2), carries
// between passes in registers.  T = uint16_t (same saturation argument as the one-piece u16 planes: poa_batch_run_ex) halves
// the bytes of a kernel that lives on its stores; arithmetic is u32 in registers either way (PlaneIO widens 0xFFFF to INF).
// NP: passes whose previous row stays in registers (rows of up to NP * 64 * K columns): a chain row — one predecessor, the
// previous row — then reads nothing back from the planes (6 of the 16 bytes of traffic per cell with u16 planes).
// All rows of query qi, written against `const TwoPieceParams&`: the single-graph kernel below and poa2_forward_multi_kernel
// (poa_multi_dense2.hpp, a wave per query on its own graph's parameter block) call this one body.
template <typename T, int NP>
__device__ __forceinline__ void poa2_forward_query(const TwoPieceParams& P, const uint32_t qi, const uint32_t lane) {
    using IO = PlaneIO<T>;
    constexpr int K = IO::K;
    constexpr uint32_t PW = 64 * K;   // columns per pass
    constexpr uint32_t INF = 0xFFFFFFFFu;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    const uint8_t* q = P.qseq + qbeg;
    const uint32_t pitch = tp_pitch(P, qi);   // (the query's own: a pass may end inside its padding, never past it)
    const uint64_t plane = (uint64_t)P.n_rows * pitch;
    T* M = tp_planes<T>(P, qi);
    T* I1 = M + plane; T* D1 = I1 + plane; T* I2 = D1 + plane; T* D2 = I2 + plane;
    const uint32_t n_pass = (L + 1 + PW - 1) / PW;   // pitch is a multiple of 64: a pass may end inside the row's padding
    constexpr int NPA = NP > 0 ? NP : 1;
    uint32_t keepM[NPA][K], keepD1[NPA][K], keepD2[NPA][K];   // M, D1, D2 of the previous row, my columns of every pass
    const bool keep = NP > 0 && n_pass <= (uint32_t)NP;
    const TpPassCosts PC{P.x, P.oe, P.e1, P.e2};
    for (uint32_t r = 0; r < P.n_rows; ++r) {
        const RowMeta rm = P.rows[r];
        const bool is_end = r == P.end_row, is_start = r == P.start_row;
        const uint64_t ro = (uint64_t)r * pitch;
        uint32_t c1 = INF, c2 = INF;   // I1 / I2 entering the first column of the pass
        uint32_t cpm = INF;             // min over predecessors of M[p][first column of the pass - 1]
        const bool from_regs = keep && r > 0 && (rm.flags & ROW_CHAIN);
        auto do_pass = [&](const uint32_t ps, uint32_t (&kM)[K], uint32_t (&kD1)[K], uint32_t (&kD2)[K]) {
            const uint32_t j = ps * PW + K * lane;    // my first column
            const bool in = j < pitch;              // (whole 16-byte groups lie inside or outside the plane row)
            uint32_t pm[K], pd[K], pd2[K];
#pragma unroll
            for (int k = 0; k < K; ++k) { pm[k] = INF; pd[k] = INF; pd2[k] = INF; }
            if (from_regs) {
#pragma unroll
                for (int k = 0; k < K; ++k) { pm[k] = kM[k]; pd[k] = kD1[k]; pd2[k] = kD2[k]; }
            } else if (in)
                for (uint32_t e = 0; e < rm.pred_count; ++e) {
                    const uint64_t po = (uint64_t)P.pred_rows[rm.pred_begin + e] * pitch + j;
                    uint32_t a[K], b[K], c[K];
                    IO::load(M + po, a); IO::load(D1 + po, b); IO::load(D2 + po, c);
#pragma unroll
                    for (int k = 0; k < K; ++k) { pm[k] = min(pm[k], a[k]); pd[k] = min(pd[k], b[k]); pd2[k] = min(pd2[k], c[k]); }
                }
            uint32_t m[K], v1[K], d1[K], v2[K], d2[K];
            tp_row_pass<K>(PC, rm, is_end, is_start, ps == 0, j, L, lane, q, pm, pd, pd2, cpm, c1, c2, m, v1, d1, v2, d2);
            if (in) {
                IO::store(M + ro + j, m); IO::store(I1 + ro + j, v1); IO::store(D1 + ro + j, d1);
                IO::store(I2 + ro + j, v2); IO::store(D2 + ro + j, d2);
                if (keep) {
#pragma unroll
                    for (int k = 0; k < K; ++k) { kM[k] = m[k]; kD1[k] = d1[k]; kD2[k] = d2[k]; }
                }
            } else if (keep) {
#pragma unroll
                for (int k = 0; k < K; ++k) { kM[k] = INF; kD1[k] = INF; kD2[k] = INF; }
            }
        };
        if (keep) {
#pragma unroll
            for (int ps = 0; ps < NPA; ++ps)
                if ((uint32_t)ps < n_pass) do_pass((uint32_t)ps, keepM[ps], keepD1[ps], keepD2[ps]);
        } else {
            for (uint32_t ps = 0; ps < n_pass; ++ps) do_pass(ps, keepM[0], keepD1[0], keepD2[0]);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the next rows read this one back (same wave)
    }
    if (lane == 0) P.score[qi] = IO::get(M + (uint64_t)P.end_row * pitch + L);
}

template <typename T, int NP>
__global__ __launch_bounds__(64) void poa2_forward_kernel(TwoPieceParams P) {
    poa2_forward_query<T, NP>(P, P.first_query + blockIdx.x, threadIdx.x);
}

// The walk of the two-piece traceback, shared by every kernel that takes it (poa2_traceback_kernel here on full planes,
// poa2_ckpt_trace_kernel of poa_checkpoint2.hpp on a segment window): the reference's backtrace rule with every test of a step
// evaluated, so that the certificate (exactly one candidate, no phantom below the target of an open test) can be decided.
// WHERE a cell lives is the kernel's business, behind an addressing policy `Cells`:
//   at(row, j, st)        a cell of the row the walk stands on
//   pred(e, p, j, st)     a cell of predecessor row p, reached through edge e (an index into pred_rows: a window addresses the
//                         row through its edge, full planes through the row)
//   up(rm, v, j)          M[v - 1][j - 1] for the Match step on a chain row (INF where there is none)
enum : uint32_t { TP_SM = 0, TP_SI = 1, TP_SD = 2, TP_SI2 = 3, TP_SD2 = 4 };   // plane order

struct TpWalkCtx {
    const RowMeta* rows;
    const uint32_t* pred_rows;
    const uint8_t* q;
    uint32_t L, start_row, end_row;
    uint32_t x, o1, e1, e2;
    poa_aln_pair_t* out;   // the query's pair region, written back to front
    uint32_t cap;
};
struct TpStep { uint32_t row, j, st; bool found; };
// the walk between two steps; `done` with `reached_start` unset is a truncated walk
struct TpWalk {
    uint32_t row, j, st, n_out, fl;
    bool done, reached_start;
};

__device__ __forceinline__ bool tp_sym_eq(const TpWalkCtx& W, uint32_t row, uint8_t c) { return row == W.end_row || W.rows[row].sym == c; }
__device__ __forceinline__ void tp_emit(const TpWalkCtx& W, TpWalk& S, uint32_t rpos, uint32_t qpos) {
    if (S.n_out < W.cap) W.out[W.cap - 1 - S.n_out] = poa_aln_pair_t{rpos, qpos};
    S.n_out++;
}

// one step back from (v, j, st): the first candidate in the reference's order; nc candidates in all, plt: a phantom below the
// target of an open test, pn: a Score subtraction wrapped onto u32::MAX (the reference panics there)
template <typename Cells>
__device__ __forceinline__ TpStep tp_step(const TpWalkCtx& W, const Cells& C, uint32_t v, uint32_t j, uint32_t st, uint32_t& nc, bool& plt, bool& pn) {
    constexpr uint32_t INF = 0xFFFFFFFFu;
    TpStep first{0, 0, TP_SM, false};
    nc = 0; plt = false; pn = false;
    auto sub = [&](uint32_t a, uint32_t b) { const uint32_t r = a - b; if (r == INF) pn = true; return r; };
    auto cand = [&](uint32_t r2, uint32_t j2, uint32_t s2) { if (!first.found) first = TpStep{r2, j2, s2, true}; nc++; };
    // every load of a Match-state step on a chain row goes out before the first use: one memory round trip instead of
    // three (row record -> predecessor list -> predecessor cell); the walk is a chain of such steps
    const uint32_t cs = C.at(v, j, st);
    const RowMeta rm = W.rows[v];
    uint32_t up = INF, gd = INF, gd2 = INF, gi = INF, gi2 = INF;
    if (st == TP_SM) {
        up = C.up(rm, v, j);
        gd = C.at(v, j, TP_SD); gd2 = C.at(v, j, TP_SD2); gi = C.at(v, j, TP_SI); gi2 = C.at(v, j, TP_SI2);
    }
    if (cs == INF) return first;
    const uint32_t pb = rm.pred_begin;
    if (st == TP_SM) {
        if (j > 0) {
            const bool moe = tp_sym_eq(W, v, W.q[j - 1]);
            const uint32_t pj = v == W.end_row ? j : j - 1;
            const uint32_t target = (moe || rm.pred_count == 0) ? cs : sub(cs, W.x);
            if ((rm.flags & ROW_CHAIN) && v != W.end_row) {
                if (up == target) cand(v - 1, pj, TP_SM);
            } else {
                for (uint32_t k = 0; k < rm.pred_count; ++k) { const uint32_t p = W.pred_rows[pb + k]; if (C.pred(pb + k, p, pj, TP_SM) == target) cand(p, pj, TP_SM); }
            }
        }
        if (gd == cs) cand(v, j, TP_SD);
        if (gd2 == cs) cand(v, j, TP_SD2);
        if (gi == cs) cand(v, j, TP_SI);
        if (gi2 == cs) cand(v, j, TP_SI2);
    } else if (st == TP_SD) {
        const uint32_t t_open = sub(sub(cs, W.o1), W.e1), t_ext = sub(cs, W.e1);
        const bool real_open = v != W.end_row && (j >= W.L || rm.sym != W.q[j]);
        for (uint32_t k = 0; k < rm.pred_count; ++k) {
            const uint32_t p = W.pred_rows[pb + k];
            const uint32_t ps = C.pred(pb + k, p, j, TP_SM);
            if (ps == t_open) cand(p, j, TP_SM);
            else if (!real_open && ps < t_open) plt = true;
        }
        for (uint32_t k = 0; k < rm.pred_count; ++k) { const uint32_t p = W.pred_rows[pb + k]; if (C.pred(pb + k, p, j, TP_SD) == t_ext) cand(p, j, TP_SD); }
    } else if (st == TP_SD2) {
        const uint32_t t = sub(cs, W.e2);
        for (uint32_t k = 0; k < rm.pred_count; ++k) { const uint32_t p = W.pred_rows[pb + k]; if (C.pred(pb + k, p, j, TP_SD) == t) cand(p, j, TP_SD); }
        for (uint32_t k = 0; k < rm.pred_count; ++k) { const uint32_t p = W.pred_rows[pb + k]; if (C.pred(pb + k, p, j, TP_SD2) == t) cand(p, j, TP_SD2); }
    } else if (st == TP_SI) {
        if (j > 0) {
            const uint32_t t_open = sub(sub(cs, W.o1), W.e1), t_ext = sub(cs, W.e1);
            const uint32_t ps = C.at(v, j - 1, TP_SM);
            bool open_i = false;
            if (j - 1 < W.L && v != W.end_row) {
                if (rm.flags & ROW_OPENI_ALWAYS) open_i = true;
                else if (rm.flags & ROW_OPENI_NEVER) open_i = false;
                else open_i = rm.child_sym != W.q[j - 1];
            }
            if (ps == t_open) cand(v, j - 1, TP_SM);
            else if (!open_i && ps < t_open) plt = true;
            if (C.at(v, j - 1, TP_SI) == t_ext) cand(v, j - 1, TP_SI);
        }
    } else {
        if (j > 0) {
            const uint32_t t = sub(cs, W.e2);
            if (C.at(v, j - 1, TP_SI) == t) cand(v, j - 1, TP_SI);
            if (C.at(v, j - 1, TP_SI2) == t) cand(v, j - 1, TP_SI2);
        }
    }
    return first;
}

// The first hop from the cell (tb_row, tb_off) the walk starts at; short_flag: what a one-symbol query is flagged with
// (gap_affine_2piece.rs:952-965).  Reads the start cell's row and its predecessors only.
template <typename Cells>
__device__ __forceinline__ void tp_walk_begin(const TpWalkCtx& W, const Cells& C, TpWalk& S, uint32_t tb_row, uint32_t tb_off, uint32_t short_flag) {
    S = TpWalk{tb_row, tb_off, TP_SM, 0, 0, false, false};
    if (W.L == 0) { S.done = true; S.reached_start = true; return; }
    if (W.L == 1 && tb_off == 1 && tp_sym_eq(W, tb_row, W.q[0])) {   // (Global: the end node equals every symbol)
        tp_emit(W, S, W.rows[tb_row].node, 0);
        S.fl = short_flag; S.done = true; S.reached_start = true;
        return;
    }
    uint32_t nc; bool plt, pn;
    TpStep cur = tp_step(W, C, tb_row, tb_off, TP_SM, nc, plt, pn);
    bool dead = false;
    if (pn) { S.fl |= POA_FLAG_REF_PANIC | POA_FLAG_TRUNCATED; dead = true; }
    else if (cur.found && (nc != 1 || plt)) S.fl |= POA_FLAG_AMBIGUOUS;
    if (!dead && !cur.found) {
        const uint32_t order[4] = {TP_SI, TP_SI2, TP_SD, TP_SD2};   // gap_affine_2piece.rs:972-978
        for (int k = 0; k < 4 && !cur.found && !dead; ++k) {
            cur = tp_step(W, C, tb_row, tb_off, order[k], nc, plt, pn);
            if (pn) { S.fl |= POA_FLAG_REF_PANIC | POA_FLAG_TRUNCATED; dead = true; }
        }
        if (!dead && !cur.found) { S.fl |= POA_FLAG_REF_PANIC; dead = true; }
        if (!dead) S.fl |= POA_FLAG_AMBIGUOUS;
    }
    if (dead) { S.done = true; S.reached_start = true; return; }   // (nothing walked: nothing more to truncate)
    S.row = cur.row; S.j = cur.j; S.st = cur.st;
}

// Steps while the walk stands on a row >= lo_row (0: to the end); a window calls it once per segment.
template <typename Cells>
__device__ __forceinline__ void tp_walk_run(const TpWalkCtx& W, const Cells& C, TpWalk& S, uint32_t lo_row) {
    while (!S.done && S.row >= lo_row) {
        uint32_t nc; bool plt, pn;
        const TpStep bt = tp_step(W, C, S.row, S.j, S.st, nc, plt, pn);
        if (pn) { S.fl |= POA_FLAG_REF_PANIC; S.done = true; break; }
        if (!bt.found) { S.done = true; break; }
        if (nc != 1 || plt) S.fl |= POA_FLAG_AMBIGUOUS;
        if (S.st == TP_SM && bt.st != TP_SM) { S.row = bt.row; S.j = bt.j; S.st = bt.st; continue; }
        if (S.st == TP_SM) tp_emit(W, S, W.rows[S.row].node, S.j - 1);
        else if (S.st == TP_SI || S.st == TP_SI2) tp_emit(W, S, POA_NONE, S.j - 1);
        else tp_emit(W, S, W.rows[S.row].node, POA_NONE);
        if (bt.st == TP_SM && bt.j == 0 && bt.row != W.start_row && S.st != TP_SD && S.st != TP_SD2 && tp_sym_eq(W, bt.row, W.q[0])) S.fl |= POA_FLAG_START_QUIRK;
        if (bt.row == W.start_row) { S.reached_start = true; S.done = true; break; }
        S.row = bt.row; S.j = bt.j; S.st = bt.st;
    }
}
__device__ __forceinline__ uint32_t tp_walk_flags(const TpWalk& S) { return S.reached_start ? S.fl : (S.fl | POA_FLAG_TRUNCATED); }

// full planes: cell = row * pitch.  dense pass: five planes; replayed search (u32): [row][offset][state] (ExactSearchT::cix)
template <typename T>
struct TpPlaneCells {
    const T* base;
    uint64_t plane;
    uint32_t pitch, tiled;
    __device__ __forceinline__ uint32_t at(uint32_t row, uint32_t j, uint32_t st) const {
        return tiled ? PlaneIO<T>::get(base + ((uint64_t)row * pitch + j) * 5u + st) : PlaneIO<T>::get(base + st * plane + (uint64_t)row * pitch + j);
    }
    __device__ __forceinline__ uint32_t pred(uint32_t, uint32_t p, uint32_t j, uint32_t st) const { return at(p, j, st); }
    __device__ __forceinline__ uint32_t up(const RowMeta&, uint32_t v, uint32_t j) const { return (v > 0 && j > 0) ? at(v - 1, j - 1, TP_SM) : 0xFFFFFFFFu; }
};

// One lane per query: the walk on the five planes.
template <typename T>
__global__ __launch_bounds__(64) void poa2_traceback_kernel(TwoPieceParams P) {
    const uint32_t slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= P.n_queries) return;
    const uint32_t qi = P.first_query + slot;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    const uint32_t pitch = tp_pitch(P, qi);
    const uint64_t plane = (uint64_t)P.n_rows * pitch;
    const TpPlaneCells<T> C{tp_planes<T>(P, qi), plane, pitch, P.exact_pass};
    TpWalkCtx W;
    W.rows = P.rows; W.pred_rows = P.pred_rows; W.q = P.qseq + qbeg; W.L = L; W.start_row = P.start_row; W.end_row = P.end_row;
    W.x = P.x; W.o1 = P.o1; W.e1 = P.e1; W.e2 = P.e2;
    W.out = tp_out(P, qi, W.cap);
    // the cell the walk starts from: (end row, L) in the dense Global pass; where the replayed search stopped otherwise
    uint32_t tb_row = P.end_row, tb_off = L;
    if (P.exact_pass) {
        const uint32_t stt = P.ex_status[qi];
        if (stt != 0) {   // the reference panics ("Could not align sequence!", a Score overflow) / the workspace ran out
            P.flags[qi] = stt == 1 ? POA_FLAG_REF_PANIC : POA_FLAG_EXACT_OVERFLOW;
            P.n_pairs[qi] = 0; P.score[qi] = 0xFFFFFFFFu;
            return;
        }
        tb_row = P.ex_end[2 * qi]; tb_off = P.ex_end[2 * qi + 1];
        P.score[qi] = C.at(tb_row, tb_off, TP_SM);
    }
    TpWalk S;
    tp_walk_begin(W, C, S, tb_row, tb_off, P.exact_pass ? 0u : POA_FLAG_SHORT_QUERY);
    tp_walk_run(W, C, S, 0u);
    const uint32_t fl = tp_walk_flags(S);
    // (a replayed table IS the reference's: its backtrace takes the first candidate, nothing to certify)
    P.flags[qi] = P.exact_pass ? (fl & (POA_FLAG_REF_PANIC | POA_FLAG_TRUNCATED)) : fl;
    P.n_pairs[qi] = tp_n_pairs(S.n_out, W.cap);
}

}  // namespace poa_amd
