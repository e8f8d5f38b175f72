// Exact multi-graph batches (poa_multi_*_exact) for gfx950: the replay of the reference's search (poa_wsearch.hpp) and the u32
// walk over what it leaves, for the queries of many graphs in one launch each.  The dense kind's forward and
// walk launches (poa_multi_dense.hpp) run in front unchanged; three kernels here follow them per chunk:
//
//   poa_fill_tables_multi_kernel      INF-fills the u32 visited table of every query that will be replayed (poa_fill_planes_kernel
//                                     with the rows of the query's own graph);
//   poa_wsearch_multi_kernel<LDS>     one workgroup of ONE wave per query.  The wave reads its query's graph id (wave_uni, as
//                                     multi_dense_block does), copies that graph's MultiExactBlock, stages the graph's arrays
//                                     and row records into its own dynamic LDS in the order of ws_kernel_body, clears its ring,
//                                     builds the WSearchParams a single-graph launch would pass and calls ws_search_query: the
//                                     search IS the single-graph one.  LDS = true is the all-in-LDS instantiation
//                                     (poa_wsearch_kernel's flags), LDS = false the generic-pointer one (poa_wsearch_global_kernel's)
//                                     for a chunk whose largest graph plus ring does not fit the launch's LDS budget;
//   poa_traceback_multi_exact_kernel  traceback_wave<uint32_t, false, 64> with the graph's TbParams pointed at the u32 tables.
//
// The slot stride.  ws_search_query addresses slot s's reached sets as E.reached + s * E.G.n_exit * E.wpn (rsum likewise).  With
// a per-graph n_exit those strides differ from wave to wave and the slots would overlap; the search would still terminate and
// quietly prune against another query's marks.  Every slot owns MultiExactLaunch::reached_stride words (the batch-wide maximum,
// poa_multi_plan.hpp), and the wave hands the search a base biased by s * (stride - n_exit * wpn): the search's own expression
// then lands on base + s * stride.  poa_wsearch.hpp stays as it is.  Stack, queue pool and ring are addressed by sizes that are
// launch-wide already.
//
// Not ported, on purpose: the persistent schedule (a wave per query, as many workgroups as queries), several queries per wave,
// the lane and flat implementations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_multi_dense.hpp"
#include "poa_wsearch.hpp"

namespace poa_amd {

struct MultiExactBlock {
    ExactGraph G;            // the graph's arrays in the concatenated tables, graph-local values
    uint32_t n_succ, n_nbm;  // lengths of G.succ / G.nbm
    uint32_t graph_lds;      // exact_lds_bytes of the graph
    uint32_t rec_lds;        // bytes of its row records, padded to 16 (0: the graph has none)
    uint32_t empty;          // no real nodes: the dense forward launch wrote the result
    uint32_t pad;
};

struct MultiExactLaunch {
    MultiDenseLaunch D;               // the dense blocks, graph_of, the chunk, the costs, the walk's depth
    const MultiExactBlock* graphs;    // [n_graphs]
    uint32_t* tables;                 // the workspace as four-byte cells
    const uint64_t* table_off;        // [total] the query's visited table, in four-byte cells
    uint32_t hybrid;                  // 1: only queries whose dense flags are non-zero
    const uint32_t* dense_flags;      // [total]
    const uint8_t* qseq; const uint64_t* qoff; const uint32_t* pitch;
    // one slot per query of the chunk (poa_multi_plan.hpp: MultiExactSlot)
    uint64_t* reached; uint64_t* rsum;
    uint64_t reached_stride, rsum_stride;
    uint32_t wpn, swpn;
    ExStackEntry* stack; uint32_t stack_cap;
    ExU4* chunks; uint32_t chunk_cap;
    uint32_t win;
    uint32_t* ring_global;            // null: the rings live in LDS
    uint32_t stage_rec;               // 1: the launch's LDS holds the row records too
    uint32_t max_lanes, adapt_lanes;
    ExactCosts C;
    uint32_t* status; uint32_t* end_cell; uint32_t* counters;
};

__global__ __launch_bounds__(256) void poa_fill_tables_multi_kernel(MultiExactLaunch A) {
    const uint32_t qi = A.D.first_query + blockIdx.x;   // (the query in x: a chunk may hold more queries than a grid has rows)
    if (A.hybrid && A.dense_flags[qi] == 0) return;
    const MultiExactBlock* __restrict__ gp = A.graphs + A.D.graph_of[qi];
    if (gp->empty) return;
    const uint64_t n4 = 3ull * gp->G.n_rows * A.pitch[qi] / 4;  // pitch is a multiple of 64
    uint4* p = reinterpret_cast<uint4*>(A.tables + A.table_off[qi]);
    const uint4 v = make_uint4(EX_INF, EX_INF, EX_INF, EX_INF);
    for (uint64_t i = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; i < n4; i += (uint64_t)gridDim.y * blockDim.x) p[i] = v;
}

// One wave per workgroup, one query per wave.  The second launch-bounds argument holds the search to the 128 VGPRs it has under
// the 1024-thread bound of poa_wsearch_kernel (four waves per SIMD).
template <bool LDS>
__global__ __launch_bounds__(64, 4) void poa_wsearch_multi_kernel(MultiExactLaunch A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t slot = blockIdx.x;   // (uniform: a kernel argument's kin)
    if (slot >= A.D.n_queries) return;
    const uint32_t qi = A.D.first_query + slot;
    const uint32_t gid = wave_uni(A.D.graph_of[qi]);
    const MultiExactBlock* __restrict__ gp = A.graphs + gid;
    if (gp->empty) return;                                  // the forward launch wrote the result
    if (A.hybrid && A.dense_flags[qi] == 0) return;         // (ws_search_query asks again: no staging for a query that is not replayed)
    const uint32_t lane = threadIdx.x & 63u;

    WSearchParams P;
    ExactParams& E = P.E;
    E.G = gp->G;
    E.first_query = A.D.first_query; E.n_queries = A.D.n_queries;
    E.hybrid = A.hybrid; E.dense_flags = A.dense_flags;
    E.qseq = A.qseq; E.qoff = A.qoff; E.pitch = A.pitch; E.plane_off = A.table_off;
    E.planes = A.tables;
    // the slot stride (head of this file): ws_search_query adds slot * n_exit * wpn
    E.reached = A.reached + (uint64_t)slot * (A.reached_stride - (uint64_t)E.G.n_exit * A.wpn);
    E.rsum = A.rsum + (uint64_t)slot * (A.rsum_stride - (uint64_t)E.G.n_exit * A.swpn);
    E.wpn = A.wpn; E.swpn = A.swpn;
    E.head = nullptr; E.n_prio = 0xFFFFFFFFu; E.pool = nullptr; E.pool_cap = 0;
    E.stack = A.stack; E.stack_cap = A.stack_cap;
    E.C = A.C;
    E.status = A.status; E.end_cell = A.end_cell;
    E.lanes_per_wave = 64; E.lds_graph = LDS ? 1u : 0u;
    E.n_succ = gp->n_succ; E.n_nbm = gp->n_nbm;
    P.chunks = A.chunks; P.chunk_cap = A.chunk_cap;
    P.win = A.win;
    P.ring_global = LDS ? nullptr : A.ring_global;
    P.graph_lds = LDS ? gp->graph_lds : 0u;
    P.waves_per_block = 1;
    P.rec_lds = (LDS && A.stage_rec) ? gp->rec_lds : 0u;
    P.max_lanes = A.max_lanes; P.adapt_lanes = A.adapt_lanes;
    P.group = 64;
    P.work_counter = nullptr; P.order = nullptr;
    P.counters = A.counters; P.prof = nullptr;

    ExactGraph G = E.G;
    uint32_t* ring;
    if constexpr (LDS) {
        // the staging order of ws_kernel_body
        uint32_t at = 0;
        auto stage = [&](const void* src, uint64_t bytes) {
            uint8_t* dst = lds + at;
            const uint32_t words = (uint32_t)((bytes + 3) / 4);
            const uint32_t* s32 = static_cast<const uint32_t*>(src);
            for (uint32_t i = lane; i < words; i += 64) reinterpret_cast<uint32_t*>(dst)[i] = s32[i];
            at += (uint32_t)((bytes + 15) & ~15ull);
            return dst;
        };
        const uint32_t n = E.G.n_rows;
        G.sym = stage(E.G.sym, n);
        G.succ_off = reinterpret_cast<const uint32_t*>(stage(E.G.succ_off, 4ull * (n + 1)));
        G.nbm_off = reinterpret_cast<const uint32_t*>(stage(E.G.nbm_off, 4ull * (n + 1)));
        G.succ = reinterpret_cast<const uint32_t*>(stage(E.G.succ, 4ull * E.n_succ));
        G.dist_min = reinterpret_cast<const uint32_t*>(stage(E.G.dist_min, 4ull * n));
        G.dist_max = reinterpret_cast<const uint32_t*>(stage(E.G.dist_max, 4ull * n));
        G.exit_idx = reinterpret_cast<const uint32_t*>(stage(E.G.exit_idx, 4ull * n));
        G.nbm = reinterpret_cast<const FlatGraph::NodeBubble*>(stage(E.G.nbm, sizeof(FlatGraph::NodeBubble) * (uint64_t)E.n_nbm));
        if (P.rec_lds) G.rec = reinterpret_cast<const FlatGraph::RowRec*>(stage(E.G.rec, sizeof(FlatGraph::RowRec) * (uint64_t)n));
        ring = reinterpret_cast<uint32_t*>(lds + P.graph_lds + P.rec_lds);
    } else {
        ring = A.ring_global + (uint64_t)slot * 3 * A.win;
    }
    if (!P.rec_lds) G.rec = nullptr;
    for (uint32_t i = lane; i < 3 * A.win; i += 64) ring[i] = BQ_EMPTY;
    __syncthreads();
    if constexpr (LDS) ws_search_query<EX_AS_GRAPH_LDS | EX_AS_RING_LDS | EX_AS_REC_LDS | EX_AS_NO_SPEC>(P, G, ring, lane, 0u);
    else ws_search_query<EX_AS_NO_SPEC>(P, G, ring, lane, 0u);
}

// the counterpart of poa_traceback_multi_kernel over the replayed tables
__global__ __launch_bounds__(256) void poa_traceback_multi_exact_kernel(MultiExactLaunch A) {
    uint32_t wq;
    const MultiDenseBlock* __restrict__ gp = multi_dense_block(A.D, wq);
    if (!gp) return;
    if (gp->empty) return;   // the forward pass wrote the result
    TbParams P = gp->T;
    P.first_query = A.D.first_query; P.n_queries = A.D.n_queries;
    P.cost_x = A.D.cost_x; P.cost_o = A.D.cost_o; P.cost_e = A.D.cost_e;
    P.spec_depth = A.D.spec_depth; P.code_fmt = A.D.code_fmt;
    P.planes = A.tables; P.plane_off = A.table_off;
    P.exact_pass = 1; P.ex_status = A.status; P.ex_end = A.end_cell; P.row_depth = nullptr;
    traceback_wave<uint32_t, false, 64>(P, A.D.first_query + wq, threadIdx.x & 63u);
}

}  // namespace poa_amd
