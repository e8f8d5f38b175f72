// Multi-graph checkpointed batches (poa_multi_*, poa_multi_*_2piece) for gfx950: the two passes of poa_checkpoint.hpp, or of
// poa_checkpoint2.hpp under the two-piece model, over the queries of many graphs in one launch.  One wavefront
// per query in both passes, as there; nothing is ordered between waves, so the four waves of a block may belong to four graphs.
//
// What a single-graph launch passes as its kernel argument, CkptParams or Ckpt2Params, lies here once per graph in a device
// array (MultiGraphBlock).  A wave reads its query's graph id, copies that graph's block into registers and patches what belongs
// to the launch: the chunk, the costs, its own strip carries (multi_load).  From there on the kernels here ARE the single-graph
// ones: pass 1 calls the same row body (ckpt_rows, ckpt2_rows), pass 2 the same per-query driver of the walk (ckpt_trace_query,
// ckpt2_trace_query), which take `const CkptParams&` / `const Ckpt2Params&` and never see where it came from.  The graph id goes
// through readfirstlane (wave_uni), and so does the wave's query index (threadIdx.x >> 6 is wave-uniform, but not provably so
// for the compiler): the block's address is then a scalar, the copy is a run of scalar loads into SGPRs, and every table pointer
// and row count the bodies use stays as uniform as a kernel argument is.
//
// Strip carries: the row bodies address carry + 4 * wq * P.n_rows (two-piece: 6 *), a stride that holds for one graph only.
// Here every query has its own offset into the chunk's carry buffer (MultiPlan::carry_off: 4 or 6 x n_rows(graph) words for a
// query wider than one strip, nothing for the others); the wave sets P.carry to its own place and calls the body with wq = 0.
// A two-piece strip is 64 lanes x K x NP columns: 1024 for <uint16_t, 2> and <uint32_t, 4>, the widest variants, and at least
// the chunk's largest pitch for every smaller variant the launch code selects, so a query of pitch <= 1024 never touches a carry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_checkpoint.hpp"
#include "poa_checkpoint2.hpp"

namespace poa_amd {

template <typename KP>
struct MultiGraphBlock {
    KP P;                  // everything of the graph and of the batch; first_query, n_queries, carry and the costs are patched per wave
    uint32_t empty;        // the graph has no real nodes: score 4 * len, POA_FLAG_EMPTY_GRAPH, no pairs (PoastaAligner::align, mod.rs:124-142)
    uint32_t pad;
};
using MultiGraphParams = MultiGraphBlock<CkptParams>;
using Multi2GraphParams = MultiGraphBlock<Ckpt2Params>;
static_assert(sizeof(MultiGraphParams) == sizeof(CkptParams) + 8 && sizeof(Multi2GraphParams) == sizeof(Ckpt2Params) + 8,
              "a block is its parameters, then empty and pad: what the host fills and uploads");

struct MultiLaunch {
    const MultiGraphParams* graphs;   // [n_graphs]
    const uint32_t* graph_of;         // [total] graph of a query
    const uint32_t* carry_off;        // [total] words into `carry`, relative to the query's chunk
    uint32_t* carry;
    uint32_t first_query, n_queries;  // the chunk
    uint32_t cost_x, cost_o, cost_e;
};

struct Multi2Launch {
    const Multi2GraphParams* graphs;  // [n_graphs]
    const uint32_t* graph_of, *carry_off;   // as in MultiLaunch
    uint32_t* carry;
    uint32_t first_query, n_queries;  // the chunk
    uint32_t x, oe, o1, e1, e2;
};

// the costs of the run: the one part of a block's patch that depends on the model
__device__ __forceinline__ void multi_costs(const MultiLaunch& A, CkptParams& P) { P.cost_x = A.cost_x; P.cost_o = A.cost_o; P.cost_e = A.cost_e; }
__device__ __forceinline__ void multi_costs(const Multi2Launch& A, Ckpt2Params& P) { P.x = A.x; P.oe = A.oe; P.o1 = A.o1; P.e1 = A.e1; P.e2 = A.e2; }

// the wave's query and its graph's parameter block; false: no query for this wave
template <typename Launch, typename KP>
__device__ __forceinline__ bool multi_load(const Launch& A, uint32_t& qi, KP& P, uint32_t& empty) {
    const uint32_t wq = wave_uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wq >= A.n_queries) return false;
    qi = A.first_query + wq;
    const uint32_t gid = wave_uni(A.graph_of[qi]);
    const MultiGraphBlock<KP>* __restrict__ gp = A.graphs + gid;
    P = gp->P;
    empty = gp->empty;
    P.first_query = A.first_query; P.n_queries = A.n_queries;
    P.carry = A.carry + wave_uni(A.carry_off[qi]);
    multi_costs(A, P);
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
    uint32_t qi, empty;
    CkptParams P;
    if (!multi_load(A, qi, P, empty)) return;
    if (empty) return;   // pass 1 wrote the result
    ckpt_trace_query<Q, T>(P, qi, 0u, threadIdx.x & 63u);
}

template <typename T, int NP>
__global__ __launch_bounds__(256) void poa2_ckpt_sweep_multi_kernel(Multi2Launch A) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t qi, empty;
    Ckpt2Params P;
    if (!multi_load(A, qi, P, empty)) return;
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
    uint32_t qi, empty;
    Ckpt2Params P;
    if (!multi_load(A, qi, P, empty)) return;
    if (empty) return;   // pass 1 wrote the result
    ckpt2_trace_query<T, NP>(P, qi, 0u, threadIdx.x & 63u);
}

}  // namespace poa_amd
