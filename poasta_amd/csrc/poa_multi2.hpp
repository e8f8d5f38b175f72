// Multi-graph checkpointed batches under the two-piece affine model (poa_multi_*_2piece) for gfx950: the two passes of
// poa_checkpoint2.hpp over the queries of many graphs in one launch.  The scheme is poa_multi.hpp's: one
// wavefront per query in both passes, nothing ordered between waves, so the four waves of a block may belong to four graphs.
//
// What a single-graph launch passes as its kernel argument, Ckpt2Params, lies here once per listed graph in a device array.  A
// wave reads its query's graph id, copies that graph's block into registers, patches what belongs to the launch (the chunk,
// the costs, its own strip carries) and calls the SAME row body (ckpt2_rows) and the SAME walk (tp_walk_begin / tp_walk_run
// behind Ckpt2Cells) as the single-graph kernels, which take `const Ckpt2Params&` and never see where it came from.  The graph
// id and the wave's query index go through readfirstlane (multi_uni): the block's address is a scalar, the copy is a run of
// scalar loads into SGPRs, and every table pointer and row count the bodies use stays as uniform as a kernel argument is.
//
// Strip carries: ckpt2_rows addresses carry + 6 * wq * P.n_rows, a stride that holds for one graph only.  Here every query has
// its own offset into the chunk's carry buffer (MultiPlan::carry_off: 6 x n_rows(graph) words for a query wider than one
// strip, nothing for the others); the wave sets P.carry to its own place and calls the body with wq = 0.  A strip is
// 64 lanes x K x NP columns: 1024 for <uint16_t, 2> and <uint32_t, 4>, the widest variants, and at least the chunk's largest
// pitch for every smaller variant the launch code selects, so a query of pitch <= 1024 never touches a carry.
//
// The driver of the walk — the loop over the segments around ckpt2_rows<PASS 2>, tp_walk_begin and tp_walk_run — is restated
// here from poa2_ckpt_trace_kernel, statement for statement: it lives inside that __global__ function, and the single-graph
// kernels stay as they are.  A change to the loop there has to be made here too; tests/test_multi_graph_2piece.py compares
// both families on the same inputs, pair for pair.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_checkpoint2.hpp"
#include "poa_multi.hpp"

namespace poa_amd {

struct Multi2GraphParams {
    Ckpt2Params P;         // everything of the graph and of the batch; first_query, n_queries, carry and the costs are patched per wave
    uint32_t empty;        // the graph has no real nodes: score 4 * len, POA_FLAG_EMPTY_GRAPH, no pairs
    uint32_t pad;
};

struct Multi2Launch {
    const Multi2GraphParams* graphs;  // [n_graphs]
    const uint32_t* graph_of;         // [total] graph of a query
    const uint32_t* carry_off;        // [total] words into `carry`, relative to the query's chunk
    uint32_t* carry;
    uint32_t first_query, n_queries;  // the chunk
    uint32_t x, oe, o1, e1, e2;
};

// the wave's query and its graph's parameter block; false: no query for this wave
__device__ __forceinline__ bool multi2_load(const Multi2Launch& A, uint32_t& qi, Ckpt2Params& P, uint32_t& empty) {
    const uint32_t wq = multi_uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wq >= A.n_queries) return false;
    qi = A.first_query + wq;
    const uint32_t gid = multi_uni(A.graph_of[qi]);
    const Multi2GraphParams* __restrict__ gp = A.graphs + gid;
    P = gp->P;
    empty = gp->empty;
    P.first_query = A.first_query; P.n_queries = A.n_queries;
    P.carry = A.carry + multi_uni(A.carry_off[qi]);
    P.x = A.x; P.oe = A.oe; P.o1 = A.o1; P.e1 = A.e1; P.e2 = A.e2;
    return true;
}

template <typename T, int NP>
__global__ __launch_bounds__(256) void poa2_ckpt_sweep_multi_kernel(Multi2Launch A) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t qi, empty;
    Ckpt2Params P;
    if (!multi2_load(A, qi, P, empty)) return;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    if (empty) {
        if (lane == 0) { P.score[qi] = L * 4u; P.flags[qi] = POA_FLAG_EMPTY_GRAPH; P.n_pairs[qi] = 0; }
        return;
    }
    const uint32_t pitch = P.pitch[qi];
    const Ckpt2Region<T> R(P, qi, pitch);
    ckpt2_rows<T, NP, 1>(P, R, qi, 0u, lane, 0u, P.n_rows, pitch, L, P.qseq + qbeg);
}

template <typename T, int NP>
__global__ __launch_bounds__(256) void poa2_ckpt_trace_multi_kernel(Multi2Launch A) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t qi, empty;
    Ckpt2Params P;
    if (!multi2_load(A, qi, P, empty)) return;
    if (empty) return;   // pass 1 wrote the result
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

    // the walk's state, wave-uniform between the segments (poa2_ckpt_trace_kernel)
    TpWalk S{P.end_row, L, TP_SM, 0, 0, false, false};
    bool first_hop = true;
    uint32_t seg = P.n_segments - 1;
    while (!S.done) {
        while (S.row < P.boundary[seg]) --seg;   // (segments the walk jumped over are not recomputed)
        const uint32_t b0 = P.boundary[seg], b1 = P.boundary[seg + 1];
        if (L > 1) {   // (a query of at most one symbol is answered from the row records alone)
            ckpt2_rows<T, NP, 2>(P, R, qi, 0u, lane, b0, b1, pitch, L, q);
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
        S.row = multi_uni(Wk.row); S.j = multi_uni(Wk.j); S.st = multi_uni(Wk.st); S.n_out = multi_uni(Wk.n_out); S.fl = multi_uni(Wk.fl);
        S.done = multi_uni(Wk.done ? 1u : 0u) != 0; S.reached_start = multi_uni(Wk.reached_start ? 1u : 0u) != 0;
        first_hop = false;
    }
    if (lane == 0) {
        P.flags[qi] = tp_walk_flags(S);
        P.n_pairs[qi] = S.n_out < W.cap ? S.n_out : W.cap;
    }
}

}  // namespace poa_amd
