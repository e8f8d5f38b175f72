// What the dense one-piece pass (poa_batch_run_ex) runs: one decision per run (cell width, layout, chunk plan, overrides) and one per
// chunk (forward kernel, column groups, waves, cell encoding, traceback lanes and depth).  Host code, no device dependency: the
// launcher in poa_engine.hip only carries the records out, and tests/dense_plan_host checks the rule on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/poasta_amd.h"

// poa_config_t.tune: what a call overrides (the library reads no environment variable)
struct TuneView {
    int val[POA_TUNE_COUNT]; bool set[POA_TUNE_COUNT];
    explicit TuneView(const poa_config_t* cfg) { for (int k = 0; k < POA_TUNE_COUNT; ++k) { set[k] = cfg && cfg->tune[k] != 0; val[k] = set[k] ? (int)cfg->tune[k] - 1 : 0; } }
    const int* ptr(int k) const { return set[k] ? &val[k] : nullptr; }
};

namespace poa_amd {
constexpr uint32_t DENSE_MW_MAX_WAVES = 16;   // waves per workgroup of a multi-wave kernel at most (MW_MAX_WAVES, poa_kernels.hpp)
uint64_t score_bound(uint64_t open, uint64_t extend, uint64_t n_open, uint64_t n_extend);
bool u16_cells_suffice(uint64_t open, uint64_t extend, uint64_t n_open, uint64_t n_extend);
bool planes32(const TuneView& T);

// What the batch constructors share (the create frame in poa_engine.hip; tests/create_host checks both on the CPU).
// choose_workspace: bytes of plane workspace, or WORKSPACE_NO_FIT when the largest item does not fit in device memory.
constexpr uint64_t WORKSPACE_NO_FIT = ~0ull;
uint64_t choose_workspace(uint64_t requested, uint64_t free_bytes, uint64_t fixed, uint64_t bytes_total, uint64_t largest, bool own_footprint);
// The workspace a one-shot call of the two-piece model asks its batch to hold, from what the device has free and the queries'
// plane bytes (all of them, the largest one's).  Dense pass: min(60 % of free, 64 GiB).  Replay: planes and search workspaces
// (replay_slot_bytes per query of a chunk) share 85 % of free as max_slots queries of the largest size would; a chunk then
// takes at most max_slots queries, so shorter queries never add search workspaces beyond that.  Never more than bytes_total,
// never less than `largest`.
struct TwoPieceWorkspace { uint64_t bytes; uint32_t max_slots; };
TwoPieceWorkspace two_piece_workspace(uint64_t free_bytes, uint64_t bytes_total, uint64_t largest, uint64_t replay_slot_bytes, bool replay);
// The concatenated table of a batch over many graphs: the table src_of(g) of every graph that owns its tables (a handle's first
// listing, table_of == g) copied to that graph's base in `dst`, which the plan sized; a repeated handle is copied once.
template <typename T, typename GraphPlan, typename SrcOf>
void concat_tables(std::vector<T>& dst, const std::vector<GraphPlan>& graphs, uint64_t GraphPlan::*base, SrcOf&& src_of) {
    for (uint32_t g = 0; g < graphs.size(); ++g) {
        if (graphs[g].table_of != g) continue;
        const std::vector<T>& src = src_of(g);
        std::copy(src.begin(), src.end(), dst.begin() + (std::ptrdiff_t)(graphs[g].*base));
    }
}
uint32_t mw_waves(uint32_t strips);
bool pxmw_ok(const TuneView& T, uint32_t count, uint32_t max_pitch);

struct DenseRunPlan {
    uint64_t ub;                             // bound on the optimal score of any query of the batch
    bool narrow, compact, relative, packed;  // u16 cells; compact layout; relative encoding; packed-u16 arithmetic kernels
    int plan;                                // chunk plan of the batch: 0 (4-byte elements), 1 (u16 full planes), 2 (compact)
    bool fuse_tb, want_band;
    int quads_override, band_pair, tb_group; // 0: no override; -1: by the rule; 0: by the chunk's count
    int band_narrow;                         // the narrow tier of the paired banded pass: -1 by the rule, 0 never, 1 whenever paired
    uint32_t band_cap, spec_depth;
    int tb_lean;                             // the lean walk kernel (poa_traceback_mf.hpp): -1 by the rule, 0 never, 1 wherever eligible
    bool tb_lean_mode;                       // the run is one whose walk may be lean at all (POA_MODE_DENSE)
};
DenseRunPlan plan_dense_run(uint32_t gap_open, uint32_t gap_extend, uint64_t max_len, uint64_t min_path_nodes, uint32_t mode, bool full_planes,
                            bool plan16_same, const TuneView& T);

struct DenseChunkPlan {
    uint32_t v[8];     // poa_batch_last_launch: kernel, quads, POA_LAUNCH_* bits, waves per workgroup, code_fmt, traceback lanes (0: fused), depth, queries
    int mf;            // flag variant of the px kernel and of the banded pair, -1 where another kernel runs
    bool band;         // the banded pair runs (v[0] == POA_KERNEL_BAND)
    bool separate_tb;  // the traceback is a launch of its own (v[5] != 0)
    bool lean_tb;      // ... and it is poa_traceback_mf_kernel<v[5]> (tb_lean_eligible), else poa_traceback_kernel
};
// plane_elems: 2-byte elements of the largest query's planes in the chunk (compact_plane_elems).  A caller that does not say is
// taken not to fit 32-bit offsets: it gets the launch record alone and the generic walk, never the lean kernel unchecked
DenseChunkPlan plan_dense_chunk(const DenseRunPlan& R, uint32_t count, uint32_t max_pitch, const TuneView& T, uint64_t plane_elems = ~0ull);
// the lean walk kernel's case: a separate launch over u16 compact cells of code_fmt 4, absolute encoding, every element offset
// within a query's planes below 2^32
bool tb_lean_eligible(const DenseRunPlan& R, uint32_t tb_lanes, uint32_t code_fmt, uint64_t plane_elems);
uint32_t band_narrow_class(uint32_t d_n, uint32_t L);
uint32_t band_narrow_pairs(const DenseRunPlan& R, bool pair_by_rule, uint32_t n_rule, uint32_t n_any);
}  // namespace poa_amd
