// Score sets (poa_scoreset_*) for gfx950: the score-only sweep of poa_forward_sweep.hpp over a list of (query, graph) PAIRS of
// many graphs in one launch.  One wavefront per pair; nothing is ordered between waves, so the four waves of
// a block may belong to four graphs.
//
// What a single-graph launch passes as its kernel argument, SweepParams, lies here once per graph in a device array.  A wave
// reads its pair's graph id and query id, copies that graph's block into registers, patches the costs and calls the SAME row
// bodies (sweep_rows, sweep_px_rows) as the single-graph kernels, which take `const SweepParams&` and never see where it came
// from.  The ids go through readfirstlane, as in poa_multi.hpp: the block's address is then a scalar, the copy is a run of
// scalar loads into SGPRs, and every table pointer and row count the bodies use stays as uniform as a kernel argument is.
//
// A launch covers one kernel CLASS of one chunk (ScoreSetPlan): `list` holds the chunk's pairs of that class, wave w takes
// pair list[w].  Results are written at the pair's own index, so they land in pair order whatever the class order is.
// A pair's slot region starts at its own offset into the chunk's workspace (4-byte cells, whatever the cell type of the run: a
// u16 run and the packed kernel's 2048-byte slot rows use the front of a region sized for u32), its strip carries at
// carry_off[p] (4 x n_rows(graph) words, only for a pair wider than 1024 columns).
//
// Capped runs (poa_scoreset_run_capped): kernels of their own, which call the capped form of the same row bodies (SweepCap) with
// the pair's cap and its graph's check rows.  The uncapped kernels and their argument block are untouched by them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poa_forward_sweep.hpp"

namespace poa_amd {

struct ScoreGraphParams {
    SweepParams P;         // the graph's tables, n_rows, n_slots, score / flags; the costs are patched per wave, the rest is unused
    uint32_t empty;        // the graph has no real nodes: score 4 * len, POA_FLAG_EMPTY_GRAPH (PoastaAligner::align, mod.rs:124-142)
    uint32_t pad;
};

struct ScoreSetLaunch {
    const ScoreGraphParams* graphs;   // [n_graphs]
    const uint32_t* list;             // [n] pairs of this launch
    const uint32_t* pair_graph;       // [n_pairs]
    const uint32_t* pair_query;       // [n_pairs]
    const uint32_t* pitch;            // [n_pairs]
    const uint64_t* region_off;       // [n_pairs] 4-byte cells from the start of the pair's chunk
    const uint32_t* carry_off;        // [n_pairs] words into `carry`, relative to the pair's chunk
    const uint8_t* qseq;
    const uint64_t* qoff;             // [n_queries + 1]
    uint32_t* planes;
    uint32_t* carry;
    uint32_t n;
    uint32_t cost_x, cost_oe, cost_e;
};

// what a capped run adds to a launch
struct ScoreSetCapLaunch {
    ScoreSetLaunch A;
    const uint32_t* cap;              // [n_pairs] POA_SCORE_UNVISITED: no cap
    uint32_t* swept;                  // [n_pairs] row bodies executed
    const uint32_t* check_rows;       // concatenated like the row tables: per graph its check rows, ascending, then 0xFFFFFFFF
    const RowMeta* rows_base;         // start of the concatenated row tables: a graph's rows - rows_base is its base in check_rows
};

// the wave's pair, its query and its graph's parameter block; false: nothing to compute for this wave (no pair, or a pair
// against a graph without real nodes, whose shortcut result is written here)
__device__ __forceinline__ bool scoreset_load(const ScoreSetLaunch& A, uint32_t lane, uint32_t& p, SweepParams& P, uint32_t& L,
                                              const uint8_t*& q) {
    const uint32_t w = wave_uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (w >= A.n) return false;
    p = wave_uni(A.list[w]);
    const uint32_t gid = wave_uni(A.pair_graph[p]);
    const uint32_t qid = wave_uni(A.pair_query[p]);
    const ScoreGraphParams* __restrict__ gp = A.graphs + gid;
    P = gp->P;
    const uint32_t empty = gp->empty;
    P.cost_x = A.cost_x; P.cost_oe = A.cost_oe; P.cost_e = A.cost_e;
    const uint64_t qbeg = A.qoff[qid];
    L = (uint32_t)(A.qoff[qid + 1] - qbeg);
    q = A.qseq + qbeg;
    if (empty) {
        if (lane == 0) { P.score[p] = L * 4u; P.flags[p] = POA_FLAG_EMPTY_GRAPH; }
        return false;
    }
    return true;
}

// the same for a capped run (a function of its own, so that the uncapped kernels are compiled from the text they had): the
// pair's cap applies to the shortcut result as to any other, and no row body runs for it
__device__ __forceinline__ bool scoreset_load_capped(const ScoreSetCapLaunch& C, uint32_t lane, uint32_t& p, SweepParams& P, uint32_t& L,
                                                     const uint8_t*& q) {
    const ScoreSetLaunch& A = C.A;
    const uint32_t w = wave_uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (w >= A.n) return false;
    p = wave_uni(A.list[w]);
    const uint32_t gid = wave_uni(A.pair_graph[p]);
    const uint32_t qid = wave_uni(A.pair_query[p]);
    const ScoreGraphParams* __restrict__ gp = A.graphs + gid;
    P = gp->P;
    const uint32_t empty = gp->empty;
    P.cost_x = A.cost_x; P.cost_oe = A.cost_oe; P.cost_e = A.cost_e;
    const uint64_t qbeg = A.qoff[qid];
    L = (uint32_t)(A.qoff[qid + 1] - qbeg);
    q = A.qseq + qbeg;
    if (empty) {
        const bool over = L * 4u > C.cap[p];
        if (lane == 0) {
            P.score[p] = over ? 0xFFFFFFFFu : L * 4u;
            P.flags[p] = POA_FLAG_EMPTY_GRAPH | (over ? POA_FLAG_CAPPED : 0u);
            C.swept[p] = 0;
        }
        return false;
    }
    return true;
}

// the pair's cap and its graph's check rows, uniform like the pair's ids
__device__ __forceinline__ SweepCap scoreset_cap(const ScoreSetCapLaunch& C, const SweepParams& P, uint32_t p) {
    return SweepCap{wave_uni(C.cap[p]), C.check_rows + (P.rows - C.rows_base), C.swept};
}

template <int Q, typename T>
__global__ __launch_bounds__(256) void poa_scoreset_sweep_kernel(ScoreSetLaunch A) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t p, L;
    const uint8_t* q;
    SweepParams P;
    if (!scoreset_load(A, lane, p, P, L, q)) return;
    sweep_rows<Q, T>(P, p, lane, L, q, wave_uni(A.pitch[p]), reinterpret_cast<T*>(A.planes + A.region_off[p]),
                     A.carry + wave_uni(A.carry_off[p]));
}

// pairs of one strip, 512 < pitch <= 1024, on a u16 run: slot rows in the packed kernel's register layout, 2048 bytes each
__global__ __launch_bounds__(256) void poa_scoreset_sweep_px_kernel(ScoreSetLaunch A) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t p, L;
    const uint8_t* q;
    SweepParams P;
    if (!scoreset_load(A, lane, p, P, L, q)) return;
    sweep_px_rows(P, p, lane, L, q, reinterpret_cast<uint4*>(A.planes + A.region_off[p]) + lane);
}

template <int Q, typename T>
__global__ __launch_bounds__(256) void poa_scoreset_sweep_capped_kernel(ScoreSetCapLaunch C) {
    const ScoreSetLaunch& A = C.A;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t p, L;
    const uint8_t* q;
    SweepParams P;
    if (!scoreset_load_capped(C, lane, p, P, L, q)) return;
    sweep_rows<Q, T, SweepCap>(P, p, lane, L, q, wave_uni(A.pitch[p]), reinterpret_cast<T*>(A.planes + A.region_off[p]),
                           A.carry + wave_uni(A.carry_off[p]), scoreset_cap(C, P, p));
}

__global__ __launch_bounds__(256) void poa_scoreset_sweep_px_capped_kernel(ScoreSetCapLaunch C) {
    const ScoreSetLaunch& A = C.A;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t p, L;
    const uint8_t* q;
    SweepParams P;
    if (!scoreset_load_capped(C, lane, p, P, L, q)) return;
    sweep_px_rows<SweepCap>(P, p, lane, L, q, reinterpret_cast<uint4*>(A.planes + A.region_off[p]) + lane, scoreset_cap(C, P, p));
}

// ---- best-of runs (poa_scoreset_run_best) --------------------------------------------------------------------------------------
// Kernels and an argument block of their own again: the row bodies in their SweepBest form, whose cap is the running best of the
// pair's QUERY (best[pair_query[p]]) plus the run's slack, under the query's limit.  An init kernel resets the best words at
// the start of every run, a finalize kernel turns them and the per-pair results into one poa_best_t per query.
struct ScoreSetBestLaunch {
    ScoreSetLaunch A;
    unsigned long long* best;         // [n_queries] score << 32 | pair index of the best finished pair; all ones: none yet
    const uint32_t* limit;            // [n_queries] POA_SCORE_UNVISITED: no ceiling
    uint32_t slack;
    uint32_t* swept;                  // [n_pairs]
    const uint32_t* check_rows;       // as ScoreSetCapLaunch
    const RowMeta* rows_base;
};

// the device's image of poa_best_t (include/poasta_amd_scoreset_best.h)
struct ScoreSetBest {
    uint32_t pair, score, flags, second_score, n_within, reserved[3];
};
static_assert(sizeof(ScoreSetBest) == 32, "poa_best_t is 32 bytes");

// scoreset_load for a best-of run; `cap` is the wave's policy, ready for the row bodies.  A pair against a graph without real
// nodes takes part with its shortcut score like any other pair: tested against the cap of the moment, published if within it.
__device__ __forceinline__ bool scoreset_load_best(const ScoreSetBestLaunch& B, uint32_t lane, uint32_t& p, SweepParams& P, uint32_t& L,
                                                   const uint8_t*& q, SweepBest& cap) {
    const ScoreSetLaunch& A = B.A;
    const uint32_t w = wave_uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (w >= A.n) return false;
    p = wave_uni(A.list[w]);
    const uint32_t gid = wave_uni(A.pair_graph[p]);
    const uint32_t qid = wave_uni(A.pair_query[p]);
    const ScoreGraphParams* __restrict__ gp = A.graphs + gid;
    P = gp->P;
    const uint32_t empty = gp->empty;
    P.cost_x = A.cost_x; P.cost_oe = A.cost_oe; P.cost_e = A.cost_e;
    const uint64_t qbeg = A.qoff[qid];
    L = (uint32_t)(A.qoff[qid + 1] - qbeg);
    q = A.qseq + qbeg;
    cap = SweepBest{B.best + qid, B.slack, wave_uni(B.limit[qid]), B.check_rows + (P.rows - B.rows_base), B.swept};
    if (empty) {
        if (lane == 0) {
            const bool over = L * 4u > cap.now_lane();
            P.score[p] = over ? 0xFFFFFFFFu : L * 4u;
            P.flags[p] = POA_FLAG_EMPTY_GRAPH | (over ? POA_FLAG_CAPPED : 0u);
            B.swept[p] = 0;
            if (!over) cap.publish(L * 4u, p);
        }
        return false;
    }
    return true;
}

template <int Q, typename T>
__global__ __launch_bounds__(256) void poa_scoreset_sweep_best_kernel(ScoreSetBestLaunch B) {
    const ScoreSetLaunch& A = B.A;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t p, L;
    const uint8_t* q;
    SweepParams P;
    SweepBest cap;
    if (!scoreset_load_best(B, lane, p, P, L, q, cap)) return;
    sweep_rows<Q, T, SweepBest>(P, p, lane, L, q, wave_uni(A.pitch[p]), reinterpret_cast<T*>(A.planes + A.region_off[p]),
                                A.carry + wave_uni(A.carry_off[p]), cap);
}

__global__ __launch_bounds__(256) void poa_scoreset_sweep_px_best_kernel(ScoreSetBestLaunch B) {
    const ScoreSetLaunch& A = B.A;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t p, L;
    const uint8_t* q;
    SweepParams P;
    SweepBest cap;
    if (!scoreset_load_best(B, lane, p, P, L, q, cap)) return;
    sweep_px_rows<SweepBest>(P, p, lane, L, q, reinterpret_cast<uint4*>(A.planes + A.region_off[p]) + lane, cap);
}

// start of every best-of run: no query has a result yet; a run without limits gets "none" for every query
__global__ __launch_bounds__(256) void poa_scoreset_best_init_kernel(unsigned long long* best, uint32_t* limit, uint32_t n_queries,
                                                                     uint32_t has_limit) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= n_queries) return;
    best[qi] = ~0ull;
    if (!has_limit) limit[qi] = 0xFFFFFFFFu;
}

// end of the run, one query per thread: its pairs (q_off / q_pairs, ascending pair index) against T = min(best score + slack,
// limit).  The rule s <= T is applied here to the scores as written: a pair that happened to finish above T does not count, a
// stopped pair (POA_SCORE_UNVISITED with POA_FLAG_CAPPED) lies above T by the contract.
__global__ __launch_bounds__(256) void poa_scoreset_best_finalize_kernel(const unsigned long long* best, const uint32_t* limit, uint32_t slack,
                                                                         const uint32_t* q_off, const uint32_t* q_pairs,
                                                                         const uint32_t* score, const uint32_t* flags, ScoreSetBest* out,
                                                                         uint32_t n_queries) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= n_queries) return;
    const unsigned long long w = best[qi];
    const uint32_t lim = limit[qi];
    ScoreSetBest r;
    r.pair = 0xFFFFFFFFu; r.score = 0xFFFFFFFFu; r.flags = 0; r.second_score = 0xFFFFFFFFu; r.n_within = 0;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    uint32_t T = lim;
    if (w != ~0ull) {
        r.pair = (uint32_t)w; r.score = (uint32_t)(w >> 32); r.flags = flags[r.pair];
        const uint32_t t = r.score + slack;
        T = umin(t < r.score ? 0xFFFFFFFFu : t, lim);
    }
    for (uint32_t k = q_off[qi]; k < q_off[qi + 1]; ++k) {
        const uint32_t p = q_pairs[k];
        const uint32_t s = score[p];
        if (s > T) continue;
        r.n_within++;
        if (p != r.pair) r.second_score = umin(r.second_score, s);
    }
    out[qi] = r;
}

}  // namespace poa_amd
