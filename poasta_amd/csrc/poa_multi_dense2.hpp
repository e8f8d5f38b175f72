// Dense two-piece multi-graph batches (poa_multi_*_dense_2piece) for gfx950: the dense two-piece pass of poa_twopiece.hpp over
// the queries of many graphs in one launch each.  Five u16 planes per query (M, I1, D1, I2, D2), no
// checkpoints: one forward launch and one walk launch per chunk.
//
// The idiom is the one at the head of poa_multi.hpp.  What a single-graph launch passes as its kernel argument, TwoPieceParams,
// lies here once per listed graph in a device array (MultiDense2Block), filled on the host.  A wave reads its query's graph id,
// copies that graph's block and patches what belongs to the launch: the chunk, the costs, the planes base.
//
// Forward launch: one wavefront per query, four waves per block; nothing is ordered between waves, so the four waves of a block
// may belong to four graphs.  The wave's query index and the graph id go through readfirstlane (wave_uni): the block's address
// is a scalar, the copy a run of scalar loads, and every table pointer and row count stays as uniform as a kernel argument is.
// The rows are poa2_forward_query<uint16_t, 2> of poa_twopiece.hpp, the body poa2_forward_kernel itself calls: a query of any
// length (rows of up to 1024 columns keep the previous row in registers; wider ones read it back from the planes).
//
// Walk launch: ONE LANE PER QUERY, 64 queries per wave, as poa2_traceback_kernel maps it.  The 64 lanes of a wave then belong
// to different graphs, so here the idiom above is wrong: nothing derived from a lane's own query may go through wave_uni /
// readfirstlane.  The graph id is a per-lane vector load, and the block (rows, pred_rows, n_rows, start_row, end_row, empty) is
// copied per lane through vector loads from a per-lane address.  The walk itself is tp_walk_begin / tp_walk_run /
// tp_walk_flags over TpPlaneCells<uint16_t>, unchanged.  (The other mapping, one wave per query with lane 0 walking, would keep
// the block scalar and leave 63 lanes idle on a chain of dependent reads; not taken.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_twopiece.hpp"

namespace poa_amd {

struct MultiDense2Block {
    TwoPieceParams P;      // everything of the graph and of the batch; first_query, n_queries, the costs and planes are patched per launch
    uint32_t empty;        // the graph has no real nodes: score 4 * len, POA_FLAG_EMPTY_GRAPH, no pairs (PoastaAligner::align, mod.rs:124-142)
    uint32_t pad;
};
static_assert(sizeof(MultiDense2Block) == sizeof(TwoPieceParams) + 8, "a block is its parameters, then empty and pad: what the host fills and uploads");

struct MultiDense2Launch {
    const MultiDense2Block* graphs;   // [n_graphs]
    const uint32_t* graph_of;         // [total] graph of a query
    uint32_t* planes;                 // the chunk's five u16 planes per query, at plane_off[qi] two-byte elements
    uint32_t first_query, n_queries;  // the chunk
    uint32_t x, oe, o1, e1, e2;
};

// what belongs to the launch
__device__ __forceinline__ void multi_dense2_patch(const MultiDense2Launch& A, TwoPieceParams& P) {
    P.first_query = A.first_query; P.n_queries = A.n_queries;
    P.planes = A.planes; P.off_scale = 1u;   // (region_off is in two-byte elements already)
    P.x = A.x; P.oe = A.oe; P.o1 = A.o1; P.e1 = A.e1; P.e2 = A.e2;
    P.exact_pass = 0; P.ex_status = nullptr; P.ex_end = nullptr;
}

template <typename T, int NP>
__global__ __launch_bounds__(256) void poa2_forward_multi_kernel(MultiDense2Launch A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wq = wave_uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wq >= A.n_queries) return;
    const uint32_t qi = A.first_query + wq;
    const uint32_t gid = wave_uni(A.graph_of[qi]);
    const MultiDense2Block* __restrict__ gp = A.graphs + gid;
    TwoPieceParams P = gp->P;
    multi_dense2_patch(A, P);
    if (gp->empty) {
        const uint32_t L = (uint32_t)(P.qoff[qi + 1] - P.qoff[qi]);
        if (lane == 0) { P.score[qi] = L * 4u; P.flags[qi] = POA_FLAG_EMPTY_GRAPH; P.n_pairs[qi] = 0; }
        return;
    }
    poa2_forward_query<T, NP>(P, qi, lane);
}

// One lane per query: everything of the lane's graph comes through per-lane vector loads (see the head of this file).
template <typename T>
__global__ __launch_bounds__(64) void poa2_traceback_multi_kernel(MultiDense2Launch A) {
    const uint32_t slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= A.n_queries) return;
    const uint32_t qi = A.first_query + slot;
    const uint32_t gid = A.graph_of[qi];             // per lane
    const MultiDense2Block* gp = A.graphs + gid;     // a per-lane address
    if (gp->empty) return;                           // the forward launch wrote the result
    TwoPieceParams P = gp->P;
    multi_dense2_patch(A, P);
    const uint64_t qbeg = P.qoff[qi];
    const uint32_t L = (uint32_t)(P.qoff[qi + 1] - qbeg);
    const uint32_t pitch = tp_pitch(P, qi);
    const uint64_t plane = (uint64_t)P.n_rows * pitch;
    const TpPlaneCells<T> C{tp_planes<T>(P, qi), plane, pitch, 0u};
    TpWalkCtx W;
    W.rows = P.rows; W.pred_rows = P.pred_rows; W.q = P.qseq + qbeg; W.L = L; W.start_row = P.start_row; W.end_row = P.end_row;
    W.x = P.x; W.o1 = P.o1; W.e1 = P.e1; W.e2 = P.e2;
    W.out = tp_out(P, qi, W.cap);
    TpWalk S;
    tp_walk_begin(W, C, S, P.end_row, L, POA_FLAG_SHORT_QUERY);   // the dense Global pass: from (end row, L)
    tp_walk_run(W, C, S, 0u);
    P.flags[qi] = tp_walk_flags(S);
    P.n_pairs[qi] = tp_n_pairs(S.n_out, W.cap);
}

}  // namespace poa_amd
