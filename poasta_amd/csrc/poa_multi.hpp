// Multi-graph checkpointed batches (poa_multi_*) for gfx950: the two passes of poa_checkpoint.hpp over the queries of many
// graphs in one launch.  One wavefront per query in both passes, as there; nothing is ordered between waves,
// so the four waves of a block may belong to four graphs.
//
// What a single-graph launch passes as its kernel argument, CkptParams, lies here once per graph in a device array.  A wave
// reads its query's graph id, copies that graph's block into registers, patches what belongs to the launch (the chunk, the
// costs, its own strip carries) and calls the SAME row body (ckpt_rows) and the SAME walk rule (ckpt_step) as the
// single-graph kernels, which take `const CkptParams&` and never see where it came from.  The graph id goes through
// readfirstlane, and so does the wave's query index (threadIdx.x >> 6 is wave-uniform, but not provably so for the compiler):
// the block's address is then a scalar, the copy is a run of scalar loads into SGPRs, and every table pointer and row count the
// bodies use stays as uniform as a kernel argument is.
//
// Strip carries: ckpt_rows addresses carry + 4 * wq * P.n_rows, a stride that holds for one graph only.  Here every query has
// its own offset into the chunk's carry buffer (MultiPlan::carry_off: 4 x n_rows(graph) words for a query wider than one
// strip, nothing for the others); the wave sets P.carry to its own place and calls the body with wq = 0.
//
// The driver of the walk — the loop over the segments around ckpt_rows<PASS 2> and ckpt_step, with the first hop's fall-backs —
// is restated here from poa_ckpt_trace_kernel, statement for statement: it lives inside that __global__ function, and the
// single-graph kernels stay as they are.  A change to the walk there has to be made here too; tests/test_multi_graph.py
// compares both families on the same inputs, pair for pair.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_checkpoint.hpp"

namespace poa_amd {

struct MultiGraphParams {
    CkptParams P;          // everything of the graph and of the batch; first_query, n_queries, carry and the costs are patched per wave
    uint32_t empty;        // the graph has no real nodes: score 4 * len, POA_FLAG_EMPTY_GRAPH, no pairs (PoastaAligner::align, mod.rs:124-142)
    uint32_t pad;
};

struct MultiLaunch {
    const MultiGraphParams* graphs;   // [n_graphs]
    const uint32_t* graph_of;         // [total] graph of a query
    const uint32_t* carry_off;        // [total] words into `carry`, relative to the query's chunk
    uint32_t* carry;
    uint32_t first_query, n_queries;  // the chunk
    uint32_t cost_x, cost_o, cost_e;
};

__device__ __forceinline__ uint32_t multi_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the wave's query and its graph's parameter block; false: no query for this wave
__device__ __forceinline__ bool multi_load(const MultiLaunch& A, uint32_t& qi, CkptParams& P, uint32_t& empty) {
    const uint32_t wq = multi_uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wq >= A.n_queries) return false;
    qi = A.first_query + wq;
    const uint32_t gid = multi_uni(A.graph_of[qi]);
    const MultiGraphParams* __restrict__ gp = A.graphs + gid;
    P = gp->P;
    empty = gp->empty;
    P.first_query = A.first_query; P.n_queries = A.n_queries;
    P.carry = A.carry + multi_uni(A.carry_off[qi]);
    P.cost_x = A.cost_x; P.cost_o = A.cost_o; P.cost_e = A.cost_e;
    return true;
}

template <int Q, typename T>
__global__ __launch_bounds__(256) void poa_ckpt_sweep_multi_kernel(MultiLaunch A) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t qi, empty;
    CkptParams P;
    if (!multi_load(A, qi, P, empty)) return;
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    if (empty) {
        if (lane == 0) { P.score[qi] = L * 4u; P.flags[qi] = POA_FLAG_EMPTY_GRAPH; P.n_pairs[qi] = 0; }
        return;
    }
    const uint32_t pitch = P.pitch[qi];
    const CkptRegion<T> R(P, qi, pitch);
    ckpt_rows<Q, T, 1>(P, R, qi, 0u, lane, 0u, P.n_rows, pitch, L, P.qseq + qbeg);
}

template <int Q, typename T>
__global__ __launch_bounds__(256) void poa_ckpt_trace_multi_kernel(MultiLaunch A) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t qi, empty;
    CkptParams P;
    if (!multi_load(A, qi, P, empty)) return;
    if (empty) return;   // pass 1 wrote the result
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

    // the walk's state, wave-uniform between the segments (poa_ckpt_trace_kernel)
    uint32_t crow = P.end_row, cj = L, cst = 0, cnt = 0, flags = 0;
    uint32_t done = 0, reached_start = 0, first_hop = 1;
    if (L == 0) { done = 1; reached_start = 1; }
    else if (L == 1) {
        flags |= POA_FLAG_SHORT_QUERY;
        if (lane == 0) emit_at(0, end_node, 0);
        cnt = 1; done = 1; reached_start = 1;
    }
    uint32_t seg = P.n_segments - 1;
    while (!done) {
        while (crow < P.boundary[seg]) --seg;
        const uint32_t b0 = P.boundary[seg], b1 = P.boundary[seg + 1];
        ckpt_rows<Q, T, 2>(P, R, qi, 0u, lane, b0, b1, pitch, L, q);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");   // lane 0 reads what all lanes stored
        uint32_t w_row = crow, w_j = cj, w_st = cst, w_cnt = cnt, w_flags = flags, w_done = 0, w_reached = 0;
        if (lane == 0) {
            CkptCells<T> c;
            c.rows = P.rows; c.pred_rows = P.pred_rows; c.pred_src = P.pred_src;
            c.win_m = R.win_m; c.win_i = R.win_i; c.win_d = R.win_d; c.snap_m = R.snap_m; c.snap_d = R.snap_d;
            c.q = q; c.b0 = b0; c.pitch = pitch; c.L = L; c.x = P.cost_x; c.o = P.cost_o; c.e = P.cost_e;
            if (first_hop) {
                uint32_t nc, fallback = 0;
                bool bad = false, pn = false;
                TbStep cur = ckpt_step<T>(c, w_row, w_j, 0, nc, bad, pn);
                if (cur.found && !pn && (nc != 1 || bad)) w_flags |= POA_FLAG_AMBIGUOUS;
                if (!cur.found && !pn) {
                    cur = ckpt_step<T>(c, w_row, w_j, 2, nc, bad, pn);
                    if (!cur.found && !pn) cur = ckpt_step<T>(c, w_row, w_j, 1, nc, bad, pn);
                    if (!pn) {
                        if (!cur.found) { w_flags |= POA_FLAG_REF_PANIC; fallback = 1; }
                        else w_flags |= POA_FLAG_AMBIGUOUS;
                    }
                }
                if (pn) { w_flags |= POA_FLAG_REF_PANIC; fallback = 2; }
                if (fallback) {
                    if (fallback == 2) w_flags |= POA_FLAG_TRUNCATED;
                    if (fallback == 1 && L <= 3) {
                        for (uint32_t k = 0; k < L; ++k) emit_at(k, end_node, L - 1 - k);
                        w_cnt = L;
                    }
                    w_done = 1; w_reached = 1;
                } else {
                    w_row = cur.row; w_j = cur.j; w_st = cur.st;
                }
            }
            while (!w_done && w_row >= b0) {
                uint32_t nc;
                bool bad = false, pn = false;
                const TbStep bt = ckpt_step<T>(c, w_row, w_j, w_st, nc, bad, pn);
                if (pn) { w_flags |= POA_FLAG_REF_PANIC; w_done = 1; break; }
                if (!bt.found) { w_done = 1; break; }
                if (nc != 1 || bad) w_flags |= POA_FLAG_AMBIGUOUS;
                if (w_st == 0 && bt.st != 0) {
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
        crow = multi_uni(w_row); cj = multi_uni(w_j); cst = multi_uni(w_st); cnt = multi_uni(w_cnt); flags = multi_uni(w_flags);
        done = multi_uni(w_done); reached_start = multi_uni(w_reached);
        first_hop = 0;
    }
    if (!reached_start) flags |= POA_FLAG_TRUNCATED;
    if (lane == 0) {
        P.flags[qi] = flags;
        P.n_pairs[qi] = cnt < cap ? cnt : cap;
    }
}

}  // namespace poa_amd
