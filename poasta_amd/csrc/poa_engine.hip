// C ABI of the gfx950 POA alignment engine (include/poasta_amd.h).  Product code.
// Host side: graph flattening, query upload, chunked score-plane workspace, kernel launches on a
// caller-supplied HIP stream, result compaction and download.  No CPU alignment path exists here:
// without a HIP device every entry point that computes returns POA_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/poasta_amd.h"
#include "poa_graph.hpp"
#include "poa_exact_kernel.hpp"
#include "poa_wsearch.hpp"
#include "poa_fsearch.hpp"

#include "poa_dense_plan.hpp"
#include "poa_kernels.hpp"
#include "poa_traceback_mf.hpp"
#include "poa_forward_packed.hpp"
#include "poa_forward_px.hpp"
#include "poa_band_plan.hpp"
#include "poa_forward_band.hpp"
#include "poa_twopiece.hpp"
#include "poa_sweep_rows.hpp"
#include "poa_forward_sweep.hpp"
#include "poa_checkpoint.hpp"
#include "poa_checkpoint2.hpp"
#include "poa_multi_plan.hpp"
#include "poa_multi.hpp"
#include "poa_multi_dense.hpp"
#include "poa_multi_dense2.hpp"
#include "poa_multi_exact.hpp"
#include "poa_scoreset_plan.hpp"
#include "poa_scoreset.hpp"

using namespace poa_amd;

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(POA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
    } while (0)

// Device buffers come from a small per-device cache of released blocks: a host that calls poa_align_batch once per
// batch of reads would otherwise spend more time in hipMalloc / hipFree (measured 12 ms per call for the ~15 buffers of
// a config-2 batch) than in the kernels.  poa_release_cache() returns everything to the driver.
struct BufCache {
    static constexpr size_t kMaxCachedBytes = 8ull << 30;  // per device, not counting the plane workspace
    std::mutex mu;
    std::multimap<size_t, void*> free_blocks[16];
    size_t cached_bytes[16] = {};
    void* take(int dev, size_t need, size_t* got) {
        if (dev < 0 || dev >= 16) return nullptr;
        std::lock_guard<std::mutex> lk(mu);
        auto it = free_blocks[dev].lower_bound(need);
        if (it == free_blocks[dev].end() || it->first > 2 * need + (1u << 20)) return nullptr;
        void* p = it->second;
        *got = it->first;
        cached_bytes[dev] -= it->first;
        free_blocks[dev].erase(it);
        return p;
    }
    bool give(int dev, void* p, size_t bytes) {
        if (dev < 0 || dev >= 16) return false;
        std::lock_guard<std::mutex> lk(mu);
        if (cached_bytes[dev] + bytes > kMaxCachedBytes) return false;
        free_blocks[dev].emplace(bytes, p);
        cached_bytes[dev] += bytes;
        return true;
    }
    void release_all() {
        std::lock_guard<std::mutex> lk(mu);
        for (int d = 0; d < 16; ++d) {
            if (free_blocks[d].empty()) continue;
            (void)hipSetDevice(d);
            for (auto& kv : free_blocks[d]) (void)hipFree(kv.second);
            free_blocks[d].clear();
            cached_bytes[d] = 0;
        }
    }
};
static BufCache g_buf_cache;

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    size_t cap_bytes = 0;
    int dev = -1;
    ~DevBuf() { drop(); }
    void drop() {
        if (!p) return;
        if (!g_buf_cache.give(dev, p, cap_bytes)) { (void)hipSetDevice(dev); (void)hipFree(p); }
        p = nullptr; cap_bytes = 0;
    }
    hipError_t alloc(size_t count) {
        drop();
        n = count;
        if (count == 0) return hipSuccess;
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
        const size_t need = (count * sizeof(T) + 255) & ~(size_t)255;
        if (void* c = g_buf_cache.take(dev, need, &cap_bytes)) { p = (T*)c; return hipSuccess; }
        cap_bytes = need;
        return hipMalloc((void**)&p, need);
    }
};
}  // namespace

// One cached plane workspace per device.  hipMalloc / hipFree of tens of GB cost seconds (measured: 0.8-6 s per
// poa_align_batch on config 2 against 10 ms of kernels), and a host that calls poa_align_batch once per batch of reads
// must not pay that every time: a released workspace is parked here and handed to the next batch on that device.
struct PlaneWorkspace {
    uint32_t* p = nullptr;
    size_t bytes = 0;
    int device = -1;
    bool acquire(int dev, size_t need, std::string& err, bool exact = false);
    void release();
    ~PlaneWorkspace() { release(); }
};
namespace {
struct WsCache {
    std::mutex mu;
    void* p[16] = {};
    size_t bytes[16] = {};
} g_ws_cache;
}  // namespace
// exact: a parked block is taken only if it has exactly the size asked for (score-only batches: what the batch holds is what
// its slots need, poa_batch_workspace_bytes), and a parked block of another size stays parked for the next dense batch
bool PlaneWorkspace::acquire(int dev, size_t need, std::string& err, bool exact) {
    release();
    device = dev;
    if (dev >= 0 && dev < 16) {
        std::lock_guard<std::mutex> lk(g_ws_cache.mu);
        if (g_ws_cache.p[dev] && (exact ? g_ws_cache.bytes[dev] == need : g_ws_cache.bytes[dev] >= need)) {
            p = (uint32_t*)g_ws_cache.p[dev]; bytes = g_ws_cache.bytes[dev];
            g_ws_cache.p[dev] = nullptr; g_ws_cache.bytes[dev] = 0;
            return true;
        }
        if (g_ws_cache.p[dev] && !exact) {  // too small: give it back before asking for a bigger one
            (void)hipFree(g_ws_cache.p[dev]);
            g_ws_cache.p[dev] = nullptr; g_ws_cache.bytes[dev] = 0;
        }
    }
    const hipError_t e = hipMalloc((void**)&p, need);
    if (e != hipSuccess) { p = nullptr; err = hipGetErrorString(e); return false; }
    bytes = need;
    return true;
}
// what a batch on `dev` can take over besides the device's free memory
static size_t parked_workspace_bytes(int dev) {
    if (dev < 0 || dev >= 16) return 0;
    std::lock_guard<std::mutex> lk(g_ws_cache.mu);
    return g_ws_cache.bytes[dev];
}
void PlaneWorkspace::release() {
    if (!p) return;
    void* victim = p;
    if (device >= 0 && device < 16) {
        std::lock_guard<std::mutex> lk(g_ws_cache.mu);
        if (!g_ws_cache.p[device] || g_ws_cache.bytes[device] < bytes) {
            victim = g_ws_cache.p[device];
            g_ws_cache.p[device] = p; g_ws_cache.bytes[device] = bytes;
        }
    }
    if (victim) { (void)hipSetDevice(device); (void)hipFree(victim); }
    p = nullptr; bytes = 0;
}

struct poa_graph {
    FlatGraph g;
    SweepRows sweep;        // row liveness / slots of the score-only sweep (poa_sweep_rows.hpp), rebuilt with g
    CheckpointPlan ckpt;    // segment plan of the checkpointed mode at the engine's own segment length, rebuilt with g
    CheckpointPlan ckpt2;   // the same for the two-piece model (POA_MODE_CHECKPOINT2: three kept planes, five window planes)
    std::mutex bubble_mu;   // the bubble index (exact / hybrid mode only) is built on first use; batches on other threads may share the handle
};

struct poa_batch {
    const poa_graph* graph = nullptr;
    int device = 0;
    uint32_t n_queries = 0;
    uint64_t total_bases = 0, total_cells = 0, plane_bytes_total = 0;
    std::vector<uint64_t> h_qoff;
    std::vector<uint32_t> h_pitch;
    std::vector<uint64_t> h_scratch_off;
    struct Chunk { uint32_t first, count; };
    // How the queries share the plane workspace.  plan[0]: 4-byte elements (u32 planes, exact replay);
    // plan[1]: 2-byte elements, three full planes (POA_CFG_FULL_PLANES with u16 scores) — twice the queries per chunk when
    // the batch needs chunks; plan[2]: the compact layout at its real size (compact_plane_elems, ~2.7 bytes per cell).
    struct Plan {
        std::vector<Chunk> chunks;
        std::vector<uint64_t> off;   // per query: offset of its planes in ELEMENTS of the layout's type
        uint32_t max_chunk = 0;
        DevBuf<uint64_t> d_off;
    };
    // plan[3]: 4-byte elements, five full planes (u32 run of the two-piece model, poa_batch_run_2piece) — built on first use;
    // the five u16 planes of a two-piece run fit a query's region of plan[0] (2.5 of its 3 x rows x pitch elements)
    Plan plan[4];
    uint64_t plan_ws = 0;            // bytes of workspace the plans were cut for
    bool two_piece = false;          // the last run was a two-piece run over five full planes: the dense pass, or (last_mode EXACT / HYBRID) the replay
    bool plan16_same = true;         // plan[1], plan[2] not built: everything fits in one chunk anyway
    int active_plan = 0;             // plan of the last run
    const Plan& cur() const { return plan[active_plan]; }
    uint64_t max_len = 0;
    bool narrow = false;  // last run used u16 planes
    bool compact = false; // last run used the compact layout (no I plane, partial D)
    int cols_per_lane = 16;

    DevBuf<RowMeta> d_rows;
    DevBuf<uint32_t> d_pred_rows;
    DevBuf<uint32_t> d_row_depth, d_pred_k;   // depth potential of the relative u16 encoding (FlatGraph::row_depth / pred_k)
    DevBuf<uint32_t> d_dslot, d_pred_dslot;   // compact layout: slots of the kept D rows (FlatGraph::d_slot / pred_dslot)
    bool relative = false;                    // last run stored scores relative to that potential
    bool dense_narrow = false, dense_compact = false, dense_relative = false, dense_derived_gaps = false;   // layout of the last run's dense pass (poa_batch_last_layout)
    DevBuf<uint8_t> d_qseq;
    DevBuf<uint64_t> d_qoff, d_scratch_off, d_pair_off;
    DevBuf<uint32_t> d_pitch, d_carry, d_score, d_flags, d_npairs;
    PlaneWorkspace d_planes;
    DevBuf<uint2> d_scratch, d_pairs;
    // exact-replay mode (allocated on first use)
    DevBuf<uint32_t> d_succ_off, d_succ_rows, d_dist_min, d_dist_max, d_nbm_off, d_ex_status, d_exit_idx, d_ex_head, d_node_row, d_sp_to_end, d_ex_end;
    DevBuf<FlatGraph::NodeBubble> d_nbm;
    DevBuf<uint8_t> d_ex_sym;
    DevBuf<uint64_t> d_ex_reached, d_ex_rsum;
    DevBuf<ExQEntry> d_ex_pool;
    DevBuf<ExStackEntry> d_ex_stack;
    uint32_t ex_n_prio = 0, ex_pool_cap = 0, ex_stack_cap = 0, ex_wpn = 0, ex_swpn = 0;
    uint32_t ex_win = 64;              // wave search: priorities in the descriptor ring (power of two)
    uint32_t ex_skew = 0;              // max over nodes of dist_to_end max - min: bounds how far the min-gap heuristic can grow along a greedy extension
    DevBuf<uint32_t> d_ex_order;         // wave search, persistent scheduling: [0] work counter, [1..] query order
    DevBuf<uint32_t> d_pipeline_error;   // FwdParams::pipeline_error
    DevBuf<unsigned long long> d_ex_prof;
    DevBuf<uint32_t> d_ex_counters;    // wave search: num_queued, num_visited, num_pruned, steps per query
    DevBuf<uint32_t> d_ex_logs;        // parallel-step search (poa_fsearch.hpp): the lanes' push logs, per resident wave
    DevBuf<FlatGraph::RowRec> d_ex_rec; // per-row records of its lean step (FlatGraph::row_rec)
    bool ex_tables_ready = false;      // the replay's view of the graph and its per-query result buffers are there (prepare_exact_tables)
    bool exact_ready = false;          // the search workspace is sized for the one-piece replay (prepare_exact); prepare_replay2 clears it
    bool prof_on = false;              // the last run asked for the replay kernel's cycle counts (POA_TUNE_WS_PROF)
    uint32_t last_mode = 0;
    // score-only batch (poa_batch_create_ex with POA_MODE_SCORE): the workspace holds n_sweep_slots rows of M and D per query,
    // d_dslot / d_pred_dslot hold SweepRows::slot / pred_slot, no pair buffers exist
    bool sweep = false;
    uint32_t sweep_slots = 1;          // max(n_sweep_slots, 1)
    uint64_t sweep_slotted = 0;        // rows per query that are stored at all
    uint64_t sweep_bytes_written = 0;  // slot bytes the last score-only run stored (poa_stats_t.plane_bytes)
    // checkpointed batch (poa_batch_create_ex with POA_MODE_CHECKPOINT): per query the sweep's slots, the snapshots and one
    // segment window (poa_checkpoint.hpp); d_dslot / d_pred_dslot hold SweepRows::slot / pred_slot; pair buffers as in dense mode
    bool ckpt = false;
    CheckpointPlan ckpt_plan;          // the plan the batch was sized for (POA_TUNE_CKPT_ROWS at creation, else the graph's own)
    uint32_t ckpt_slots = 0;
    bool ckpt2 = false;                // a checkpointed batch of the two-piece model (POA_MODE_CHECKPOINT2, poa_checkpoint2.hpp): `ckpt` is set too
    DevBuf<uint32_t> d_ck_snap_off, d_ck_snap_dst, d_ck_pred_src, d_ck_boundary;

    // banded forward pass (poa_forward_band.hpp): one band class per distinct query length, planned at the first run that
    // takes the banded kernel (the plan depends on the graph and the lengths alone) and kept
    bool band_ready = false;
    uint32_t band_n_seg = 0;
    std::vector<uint32_t> h_band_cls, h_band_d;          // per query: class; per class: band distance D
    DevBuf<uint32_t> d_band_cls, d_band_d, d_band_base;  // the same on the device, and the window bases [class][segment]
    DevBuf<uint32_t> d_band_list, d_band_count;          // queries the full kernel redoes: [n_queries], and their number per chunk
    // narrow tier (poa_forward_band2_kernel<6>): the classes' second plan for a window of BAND_WINDOW_NARROW columns, and the list
    // of the queries it could not certify, which the 512 pass then takes.  d_band_count holds three counters per chunk:
    // [chunk] the full pass's list, [n_chunks + chunk] the narrow tier's list, [2 * n_chunks + chunk] those of it the 512 pass missed too
    std::vector<uint32_t> h_band_dn;
    DevBuf<uint32_t> d_band_dn, d_band_base_n, d_band_list_n;
    std::vector<uint32_t> h_band_order;                              // the host's copy of d_band_order
    std::vector<uint32_t> h_band_nnarrow_rule, h_band_nnarrow_any;   // per chunk: its leading pairs whose class takes the tier by the rule / has D_n >= 4
    uint32_t narrow_ran = 0, narrow_how = 0, narrow_chunks = 0;      // the last run (poa_batch_band_narrow_info)
    uint32_t tb_kernel = 0, tb_lanes = 0, tb_depth = 0, tb_walks = 0; // the dense pass's separate traceback launches of the last run (poa_batch_tb_info)
    // paired banded pass (poa_forward_band2_kernel): per chunk of plan[band_pair_plan] the queries in launch order - the pairs
    // (A, B, A, B, ...), then the singles - built from the lengths alone at the first run that may pair and kept
    int band_pair_plan = -1;
    std::vector<uint32_t> h_band_npair;                  // per chunk: its pairs
    DevBuf<uint32_t> d_band_order;                       // [n_queries], a chunk's part at its first query
    uint32_t pair_paired = 0, pair_single = 0;           // the last run (poa_batch_band_pair_info)
    // the last run (poa_batch_band_info)
    bool band_used = false;
    uint32_t band_queries = 0, band_min_d = 0, band_chunks = 0;
    // what the dense one-piece path launched per chunk of the last run (poa_batch_last_launch); empty after any other run
    std::vector<DenseChunkPlan> launches;
    // what the exact replay launched per chunk of the last run (poa_batch_replay_info / poa_multi_replay_info)
    struct ReplayRecord { uint32_t v[8]; };   // kernel, win, lanes per query, waves per block, POA_REPLAY_BIT_*, resident, blocks, LDS bytes
    std::vector<ReplayRecord> replays;

    // one event set per run since the last stats call, written by RunFrame and read by collect_stats
    std::vector<std::vector<hipEvent_t>> runs;
    std::vector<std::vector<hipEvent_t>> free_sets;
    bool ran = false;
    hipStream_t last_stream = nullptr;
    float ms_h2d = 0.f;

    ~poa_batch() {
        for (auto& r : runs) for (auto e : r) (void)hipEventDestroy(e);
        for (auto& r : free_sets) for (auto e : r) (void)hipEventDestroy(e);
    }
};

// sums the HIP-event timings of every run recorded since the last call; the stream must be idle.
// a wave of the multi-wave pipeline gave up waiting for its neighbour (mw_wait_gt): the planes are not to be trusted
static int check_pipeline_error(poa_batch* b) {
    uint32_t w = 0;
    HIP_TRY(hipMemcpy(&w, b->d_pipeline_error.p, 4, hipMemcpyDeviceToHost));
    if (w) {
        (void)hipMemset(b->d_pipeline_error.p, 0, 4);
        return fail(POA_ERR_HIP, "multi-wave forward pipeline timed out waiting for a neighbouring strip: results discarded");
    }
    return POA_OK;
}

static void collect_stats(poa_batch* b, poa_stats_t* stats) {
    const uint32_t n = b->n_queries;
    const uint32_t keep_flagged = stats->n_flagged;
    stats->cells = b->total_cells; stats->bases = b->total_bases; stats->plane_bytes = (b->sweep || b->ckpt) ? b->sweep_bytes_written : (b->two_piece ? b->total_cells * 5 * (b->narrow ? 2 : 4) : b->plane_bytes_total);
    stats->n_queries = n; stats->n_chunks = (uint32_t)b->cur().chunks.size();
    stats->n_flagged = keep_flagged;
    stats->ms_h2d = b->ms_h2d; stats->ms_d2h = 0.f;
    float fwd = 0.f, tb = 0.f, ex = 0.f, total = 0.f;
    uint32_t launches = 0;
    for (auto& events : b->runs) {
        if (n) {
            size_t ev = 1;
            hipEvent_t prev = events[0];
            const size_t n_chunks = (events.size() - 2) / 3;
            for (size_t c = 0; c < n_chunks; ++c) {
                float a = 0.f, t2 = 0.f, t3 = 0.f;
                (void)hipEventElapsedTime(&a, prev, events[ev]);
                (void)hipEventElapsedTime(&t2, events[ev], events[ev + 1]);
                (void)hipEventElapsedTime(&t3, events[ev + 1], events[ev + 2]);
                fwd += a; tb += t2; ex += t3;
                prev = events[ev + 2];
                ev += 3;
                launches++;
            }
            float tail = 0.f, tot = 0.f;
            (void)hipEventElapsedTime(&tail, prev, events[ev]);
            tb += tail;
            (void)hipEventElapsedTime(&tot, events[0], events[ev]);
            total += tot;
        }
    }
    stats->n_runs = (uint32_t)b->runs.size();
    stats->n_forward_launches = launches;
    if (b->sweep) tb = 0.f;   // nothing but the sweep runs
    if (b->two_piece && b->last_mode != POA_MODE_DENSE) { ex = fwd; fwd = 0.f; }   // the two-piece replay: the search runs where the forward pass would
    stats->ms_forward = fwd; stats->ms_traceback = tb; stats->ms_exact = ex; stats->ms_total = total;
    for (auto& r : b->runs) b->free_sets.push_back(std::move(r));
    b->runs.clear();
}

// ---- the frame of a run: every run path of a poa_batch (and of the batches built around one) goes through here ------------
// The event set collect_stats reads back is written here and nowhere else: [begin, (forward end, traceback end, exact end) per
// chunk ..., end], 2 + 3 x chunks events.  A path calls open, begin, three marks per chunk, and one of the ends.
struct RunFrame {
    poa_batch* b = nullptr;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> events;
    size_t ev = 1;

    // At most 256 event sets wait for poa_*_stats / _fetch; `refusal` is the entry point's own text.  A path writes nothing into
    // the batch before this passes, so a refused run leaves the batch as the previous run left it.
    int open(poa_batch* batch, const std::string& refusal) {
        b = batch;
        if (b->runs.size() >= 256) return fail(POA_ERR_UNSUPPORTED, refusal);
        return POA_OK;
    }
    // takes a free event set of the run's size or creates one, and records the begin event
    int begin(hipStream_t s, size_t n_chunks) {
        stream = s;
        b->last_stream = stream;
        const size_t n_events = 2 + 3 * n_chunks;
        for (size_t k = 0; k < b->free_sets.size(); ++k) {
            if (b->free_sets[k].size() == n_events) {
                events = std::move(b->free_sets[k]);
                b->free_sets.erase(b->free_sets.begin() + (long)k);
                break;
            }
        }
        if (events.empty()) {
            events.reserve(n_events);
            while (events.size() < n_events) {
                hipEvent_t e;
                const hipError_t rc = hipEventCreate(&e);
                if (rc != hipSuccess) {
                    for (auto made : events) (void)hipEventDestroy(made);
                    return fail(POA_ERR_HIP, std::string("hipEventCreate(&e): ") + hipGetErrorString(rc));
                }
                events.push_back(e);
            }
        }
        b->runs.push_back(events);
        HIP_TRY(hipEventRecord(events[0], stream));
        return POA_OK;
    }
    // the next `n` marks of the current chunk, in the order forward end, traceback end, exact end
    int mark(int n = 1) {
        while (n-- > 0) HIP_TRY(hipEventRecord(events[ev++], stream));
        return POA_OK;
    }
    int end() {
        HIP_TRY(hipEventRecord(events[ev], stream));
        b->ran = true;
        return POA_OK;
    }
    // a batch without queries: an empty pair list where the batch has pair buffers, and the run is over
    int end_empty(bool has_pairs) {
        if (has_pairs) HIP_TRY(hipMemsetAsync(b->d_pair_off.p, 0, 8, stream));
        return end();
    }
    // the pairs of all queries: offsets by a scan of the counts, then compaction of the traceback scratch into d_pairs
    int end_pairs() {
        hipLaunchKernelGGL(poa_scan_kernel, dim3(1), dim3(1024), 0, stream, b->d_npairs.p, b->d_pair_off.p, b->n_queries);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(poa_compact_kernel, dim3((b->n_queries + 3) / 4), dim3(256), 0, stream, b->d_scratch.p,
                           b->d_scratch_off.p, b->d_npairs.p, b->d_pair_off.p, b->d_pairs.p, b->n_queries);
        HIP_TRY(hipGetLastError());
        return end();
    }
};

// ---- the frame of a create: every batch constructor goes through here -------------------------------------------------------
// A constructor is its mode and argument checks (no device needed), its plan callable and `fixed`, the calls below in the order
// they stand here, and between them what only its kind has: its tables, its carries, its parameter blocks.  Everything behind
// the null check of `out` runs inside guarded(), and the handle is released into *out by the constructor's last statement.
struct CreateFrame {
    std::string who;   // the entry point, as its messages name it
    int device = 0;
    struct Events {    // of the timed upload; destroyed on every way out
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() { for (auto ev : e) if (ev) (void)hipEventDestroy(ev); }
    } timed;

    // nothing but an error code leaves a constructor: a host allocation that fails anywhere in `body` is the refusal `text`
    template <typename Body>
    static int guarded(const std::string& text, Body&& body) {
        try { return body(); } catch (const std::bad_alloc&) { return fail(POA_ERR_OUT_OF_MEMORY, text); }
    }
    // the C entry of a constructor: the null check of `out`, then `body`, which is all the rest, under that guard
    template <typename Handle, typename Body>
    static int enter(const std::string& who, Handle** out, const std::string& text, Body&& body) {
        if (!out) return fail(POA_ERR_INVALID_ARG, who + ": out is null");
        *out = nullptr;
        return guarded(text, body);
    }
    // the device check; nothing touches the device before it
    int open(int dev) {
        device = dev;
        const int ndev = poa_device_count();
        if (ndev <= 0) return fail(POA_ERR_NO_DEVICE, "no HIP device visible: the gfx950 path has no CPU fallback");
        if (device < 0 || device >= ndev) return fail(POA_ERR_INVALID_ARG, who + ": device ordinal out of range");
        HIP_TRY(hipSetDevice(device));
        return POA_OK;
    }
    // the workspace rule (choose_workspace, poa_dense_plan.cpp) on what the device has free now; `refusal` is the kind's own text
    int workspace(uint64_t requested, uint64_t fixed, uint64_t bytes_total, uint64_t largest, bool own_footprint, const char* refusal, uint64_t& ws) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        ws = choose_workspace(requested, free_b, fixed, bytes_total, largest, own_footprint);
        if (ws == WORKSPACE_NO_FIT) return fail(POA_ERR_OUT_OF_MEMORY, refusal);
        return POA_OK;
    }
    // The second pass of the two-pass plan.  The first, plan_of(0, pl), ran in front of the device check: it holds the argument
    // checks and gave the footprint the workspace is chosen from; the plan is cut again only when that workspace is a cap.
    template <typename Plan, typename PlanOf>
    int plan_capped(Plan& pl, uint64_t requested, uint64_t fixed, uint64_t largest, const char* refusal, PlanOf&& plan_of) {
        uint64_t ws = 0;
        if (const int rc = workspace(requested, fixed, pl.bytes_total, largest, false, refusal, ws)) return rc;
        return ws < pl.bytes_total ? plan_of(ws, pl) : POA_OK;
    }
    // the core batch of a kind that is built around one: `n` items in the plan's chunks, no graph of its own
    template <typename Plan>
    void fill_core(poa_batch* b, const Plan& pl, uint32_t n, uint64_t plane_bytes) const {
        b->graph = nullptr; b->device = device; b->n_queries = n;
        b->total_bases = pl.total_bases; b->total_cells = pl.total_cells; b->plane_bytes_total = plane_bytes;
        b->plan_ws = pl.workspace_bytes;
        b->active_plan = 0;
        for (const auto& c : pl.chunks) {
            b->plan[0].chunks.push_back({c.first, c.count});
            b->plan[0].max_chunk = std::max(b->plan[0].max_chunk, c.count);
        }
    }
    // ... and of a multi-graph batch, whose items are queries: the host's copies of their offsets and pitches as well
    void fill_core(poa_batch* b, const MultiPlan& pl, uint64_t plane_bytes, const uint64_t* qoff) const {
        fill_core(b, pl, pl.n_queries, plane_bytes);
        for (const auto& gp : pl.graphs) b->max_len = std::max(b->max_len, gp.max_len);
        b->h_qoff.assign(qoff, qoff + pl.n_queries + 1);
        b->h_pitch = pl.pitch;
        b->h_scratch_off = pl.scratch_off;
        b->plan[0].off = pl.region_off;
    }
    // `n` elements, and one where there are none: a kernel argument is a valid address even in a batch without queries
    template <typename... Bufs>
    static hipError_t alloc_each(uint64_t n, Bufs&... bufs) {
        hipError_t e = hipSuccess;
        ((e = e != hipSuccess ? e : bufs.alloc(std::max<uint64_t>(n, 1))), ...);
        return e;
    }
    // what every kind holds: the queries, the items' pitches and regions, their results and, where runs return pairs, the pair
    // buffers (scratch_total pairs of capacity).  n_queries differs from the items `n` in a score set alone.
    int alloc_results(poa_batch* b, uint64_t n_bases, uint64_t n_queries, uint64_t n, bool has_pairs, uint64_t scratch_total) const {
        HIP_TRY(alloc_each(n_bases, b->d_qseq));
        HIP_TRY(alloc_each(n_queries + 1, b->d_qoff));
        HIP_TRY(alloc_each(n, b->d_pitch, b->plan[0].d_off, b->d_score, b->d_flags));
        if (has_pairs) {
            HIP_TRY(alloc_each(n + 1, b->d_scratch_off, b->d_pair_off));
            HIP_TRY(alloc_each(n, b->d_npairs));
            HIP_TRY(alloc_each(scratch_total, b->d_scratch, b->d_pairs));
        }
        HIP_TRY(alloc_each(1, b->d_pipeline_error));
        HIP_TRY(hipMemset(b->d_pipeline_error.p, 0, 4));
        return POA_OK;
    }
    // the plane workspace, none for a batch without items; `what` opens the kind's own refusal
    int acquire_planes(poa_batch* b, uint64_t bytes, bool exact, const char* what) const {
        if (!b->n_queries) return POA_OK;
        std::string werr;
        if (!b->d_planes.acquire(device, bytes, werr, exact)) return fail(POA_ERR_OUT_OF_MEMORY, std::string(what) + ": " + werr);
        return POA_OK;
    }
    // The timed upload: poa_stats_t.ms_h2d is the interval between begin_upload and end_upload, the copies and no allocation.
    static hipError_t upload(void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) : hipSuccess; }
    template <typename T>
    static hipError_t upload(DevBuf<T>& dst, const std::vector<T>& src) { return upload(dst.p, src.data(), src.size() * sizeof(T)); }
    int begin_upload() {
        for (auto& ev : timed.e) HIP_TRY(hipEventCreate(&ev));
        HIP_TRY(hipEventRecord(timed.e[0], nullptr));
        return POA_OK;
    }
    // the shared part of it: sequences and offsets of n_queries queries, pitch and region of `n` items, scratch_off where there are pairs
    int upload_queries(poa_batch* b, const uint8_t* qseq, const uint64_t* qoff, size_t n_queries, const uint64_t* scratch_off,
                       const uint32_t* pitch, const uint64_t* region_off, size_t n) const {
        HIP_TRY(upload(b->d_qseq.p, qseq, qoff[n_queries]));
        HIP_TRY(upload(b->d_qoff.p, qoff, (n_queries + 1) * 8));
        if (scratch_off) HIP_TRY(upload(b->d_scratch_off.p, scratch_off, (n + 1) * 8));
        HIP_TRY(upload(b->d_pitch.p, pitch, n * 4));
        HIP_TRY(upload(b->plan[0].d_off.p, region_off, n * 8));
        return POA_OK;
    }
    int end_upload(poa_batch* b) {
        HIP_TRY(hipEventRecord(timed.e[1], nullptr));
        HIP_TRY(hipEventSynchronize(timed.e[1]));
        (void)hipEventElapsedTime(&b->ms_h2d, timed.e[0], timed.e[1]);
        return POA_OK;
    }
};

// u16_cells_suffice (poa_dense_plan.cpp) for one graph and the longest query that meets it
static bool u16_cells_suffice(uint64_t open, uint64_t extend, uint64_t max_len, const FlatGraph& fg) {
    return u16_cells_suffice(open, extend, (max_len ? 1 : 0) + (fg.min_path_nodes ? 1 : 0), max_len + fg.min_path_nodes);
}
// ... and for a batch over many graphs: u16 cells only if every graph's own bound (the longest query that meets it and its shortest
// path) allows them.  The constructors note a graph's two counts; a run holds them against its costs.
static void note_graph_bound(std::vector<uint64_t>& ub_open, std::vector<uint64_t>& ub_extend, uint64_t max_len, const FlatGraph& fg) {
    ub_open.push_back((max_len ? 1 : 0) + (fg.min_path_nodes ? 1 : 0));
    ub_extend.push_back(max_len + fg.min_path_nodes);
}
static bool all_graphs_u16(const std::vector<uint64_t>& ub_open, const std::vector<uint64_t>& ub_extend, uint64_t open, uint64_t extend) {
    for (size_t g = 0; g < ub_open.size(); ++g)
        if (!u16_cells_suffice(open, extend, ub_open[g], ub_extend[g])) return false;
    return true;
}
static_assert(DENSE_MW_MAX_WAVES == MW_MAX_WAVES, "the plan's waves per workgroup are the kernels'");

// the layout of the last run, as poa_batch_last_layout and the plane fetches read it
static void set_layout(poa_batch* b, bool narrow, bool compact = false, bool relative = false) {
    b->narrow = narrow; b->compact = compact; b->relative = relative;
    b->dense_narrow = narrow; b->dense_compact = compact; b->dense_relative = relative; b->dense_derived_gaps = false;
}

// The kernels that keep a row in registers take the cell type and the number of column groups per lane as template arguments: a
// group is 512 columns of u16 cells or 256 of u32, and the chunk's largest pitch says how many a strip of up to 1024 columns
// needs.  `launch` receives both as tags (a value of the cell type, a std::integral_constant) and names the kernel.
template <typename Launch>
static void launch_by_pitch(bool narrow, uint32_t max_pitch, Launch&& launch) {
    using std::integral_constant;
    if (narrow) {
        if (max_pitch <= 512) launch(uint16_t{}, integral_constant<int, 1>{});
        else launch(uint16_t{}, integral_constant<int, 2>{});
    } else {
        if (max_pitch <= 256) launch(uint32_t{}, integral_constant<int, 1>{});
        else if (max_pitch <= 512) launch(uint32_t{}, integral_constant<int, 2>{});
        else launch(uint32_t{}, integral_constant<int, 4>{});
    }
}

// the band plan of a resident batch: classes by query length, their band distances and window bases, uploaded once
static int prepare_band(poa_batch* b) {
    if (b->band_ready) return POA_OK;
    const FlatGraph& fg = b->graph->g;
    BandTables bt;
    build_band_tables(fg, bt);
    b->band_n_seg = band_segments(fg.n);
    std::map<uint64_t, uint32_t> cls_of_len;
    std::vector<uint32_t> bases;
    b->h_band_cls.resize(b->n_queries);
    b->h_band_d.clear();
    b->h_band_dn.clear();
    std::vector<uint32_t> bases_n;
    for (uint32_t i = 0; i < b->n_queries; ++i) {
        const uint64_t len = b->h_qoff[i + 1] - b->h_qoff[i];
        auto it = cls_of_len.find(len);
        if (it == cls_of_len.end()) {
            it = cls_of_len.emplace(len, (uint32_t)b->h_band_d.size()).first;
            bases.resize(bases.size() + b->band_n_seg);
            b->h_band_d.push_back(plan_band(fg, bt, (uint32_t)len, BAND_SEG_ROWS, BAND_WINDOW, bases.data() + bases.size() - b->band_n_seg));
            bases_n.resize(bases.size());
            b->h_band_dn.push_back(plan_band(fg, bt, (uint32_t)len, BAND_SEG_ROWS, BAND_WINDOW_NARROW, bases_n.data() + bases_n.size() - b->band_n_seg));
        }
        b->h_band_cls[i] = it->second;
    }
    HIP_TRY(b->d_band_cls.alloc(b->n_queries));
    HIP_TRY(b->d_band_d.alloc(b->h_band_d.size()));
    HIP_TRY(b->d_band_base.alloc(bases.size()));
    HIP_TRY(b->d_band_list.alloc(b->n_queries));
    HIP_TRY(hipMemcpy(b->d_band_cls.p, b->h_band_cls.data(), b->h_band_cls.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_band_d.p, b->h_band_d.data(), b->h_band_d.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_band_base.p, bases.data(), bases.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(b->d_band_dn.alloc(b->h_band_dn.size()));
    HIP_TRY(b->d_band_base_n.alloc(bases_n.size()));
    HIP_TRY(b->d_band_list_n.alloc(b->n_queries));
    HIP_TRY(hipMemcpy(b->d_band_dn.p, b->h_band_dn.data(), b->h_band_dn.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_band_base_n.p, bases_n.data(), bases_n.size() * 4, hipMemcpyHostToDevice));
    b->band_ready = true;
    return POA_OK;
}

// who pairs (poa_forward_band2_kernel): within a chunk, in query order, every second query of a band class with D >= 4 joins
// the class's waiting one; what is left over - odd members, classes of one, classes without a band - runs as singles.
// Depends on the lengths and the chunk plan alone: uploaded once per chunk plan.
static int prepare_band_pairs(poa_batch* b) {
    if (b->band_pair_plan == b->active_plan) return POA_OK;
    const poa_batch::Plan& PL = b->cur();
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    std::vector<uint32_t> order(b->n_queries), waiting(b->h_band_d.size(), NONE), singles;
    b->h_band_npair.assign(PL.chunks.size(), 0);
    b->h_band_nnarrow_rule.assign(PL.chunks.size(), 0); b->h_band_nnarrow_any.assign(PL.chunks.size(), 0);
    for (size_t ci = 0; ci < PL.chunks.size(); ++ci) {
        const auto& ch = PL.chunks[ci];
        uint32_t at = ch.first;
        singles.clear();
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
            const uint32_t cl = b->h_band_cls[i];
            if (b->h_band_d[cl] < 4) singles.push_back(i);
            else if (waiting[cl] == NONE) waiting[cl] = i;
            else { order[at++] = waiting[cl]; order[at++] = i; waiting[cl] = NONE; }
        }
        b->h_band_npair[ci] = (at - ch.first) / 2;
        // the pairs the narrow tier can take come first, those it takes by the rule before those only an override sends there
        // (band_narrow_class, poa_dense_plan.cpp): the tier's launch is then a prefix of the chunk's pairs
        std::vector<std::array<uint32_t, 3>> pr;   // {class of narrow tier, A, B}
        uint32_t n_of[3] = {0, 0, 0};
        for (uint32_t k = ch.first; k < at; k += 2) {
            const uint32_t cl = b->h_band_cls[order[k]];
            const uint32_t t = band_narrow_class(b->h_band_dn[cl], (uint32_t)(b->h_qoff[order[k] + 1] - b->h_qoff[order[k]]));
            pr.push_back({t, order[k], order[k + 1]});
            ++n_of[t];
        }
        std::stable_sort(pr.begin(), pr.end(), [](const auto& x, const auto& y) { return x[0] < y[0]; });
        for (size_t k = 0; k < pr.size(); ++k) { order[ch.first + 2 * k] = pr[k][1]; order[ch.first + 2 * k + 1] = pr[k][2]; }
        b->h_band_nnarrow_rule[ci] = n_of[0]; b->h_band_nnarrow_any[ci] = n_of[0] + n_of[1];
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
            uint32_t& w = waiting[b->h_band_cls[i]];
            if (w == i) { singles.push_back(i); w = NONE; }
        }
        std::sort(singles.begin(), singles.end());
        for (uint32_t i : singles) order[at++] = i;
    }
    b->h_band_order = order;
    if (b->d_band_order.n < b->n_queries) HIP_TRY(b->d_band_order.alloc(b->n_queries));
    HIP_TRY(hipMemcpy(b->d_band_order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice));
    b->band_pair_plan = b->active_plan;
    return POA_OK;
}

// Greedy chunking of the queries over `ws` bytes of workspace (elems_of(i) elements of elem_bytes each), with the chunks evened
// out: the forward kernels that take a workgroup per query finish with their most loaded CU, so 2 000 queries that fit 527 at
// a time run as 4 x 500, not 3 x 527 + 419 (measured on configs[4]: 434 -> 320 ms).  max_count: queries per chunk at most (the
// two-piece replay, which holds a search workspace per query of a chunk).
template <typename ElemsOf>
static void build_chunk_plan(poa_batch::Plan& pl, uint32_t n_queries, uint64_t ws, uint64_t elem_bytes, ElemsOf elems_of, uint32_t max_count = ~0u) {
    auto need_of = [&](uint32_t i) { return (uint64_t)elems_of(i) * elem_bytes; };
    auto greedy = [&](uint64_t budget, std::vector<poa_batch::Chunk>& chunks, std::vector<uint64_t>& off) {
        chunks.clear();
        off.assign(n_queries, 0);
        uint32_t first = 0;
        uint64_t used = 0;
        for (uint32_t i = 0; i < n_queries; ++i) {
            const uint64_t need = need_of(i);
            if ((used + need > budget || i - first >= max_count) && i > first) {
                chunks.push_back({first, i - first});
                first = i; used = 0;
            }
            off[i] = used / elem_bytes;
            used += need;
        }
        if (n_queries > first) chunks.push_back({first, n_queries - first});
    };
    greedy(ws, pl.chunks, pl.off);
    if (pl.chunks.size() > 1) {
        uint64_t total = 0;
        for (uint32_t i = 0; i < n_queries; ++i) total += need_of(i);
        const uint64_t target = (total + pl.chunks.size() - 1) / pl.chunks.size();
        std::vector<poa_batch::Chunk> c2;
        std::vector<uint64_t> o2;
        for (double slack : {1.0, 1.02, 1.05, 1.1}) {
            const uint64_t budget = std::min<uint64_t>(ws, (uint64_t)((double)target * slack));
            greedy(budget, c2, o2);
            if (c2.size() == pl.chunks.size()) { pl.chunks = c2; pl.off = o2; break; }
        }
    }
    pl.max_chunk = 0;
    for (auto& c : pl.chunks) pl.max_chunk = std::max(pl.max_chunk, c.count);
}

// ---- the dense one-piece pass (poa_batch_run_ex): the records of poa_dense_plan.cpp, carried out ---------------------------
namespace {
// every forward launch of a chunk but the banded pair: the kernel and its template arguments as the chunk's record names them
void launch_forward(const DenseRunPlan& R, const DenseChunkPlan& c, const FwdParams& fp, const TbParams& tp, hipStream_t stream) {
    using std::integral_constant;
    const uint32_t quads = c.v[1];
    const bool fuse = c.v[2] & POA_LAUNCH_FUSE, mw = c.v[2] & POA_LAUNCH_MW;
    // multi-wave: one workgroup per query, a wave per strip at a time; else four queries per workgroup
    const dim3 grid(mw ? c.v[7] : (c.v[7] + 3) / 4), block(mw ? 64 * c.v[3] : 256);
    auto plain = [&](auto cell, auto q) {   // full planes: fused walk or not
        if (fuse) hipLaunchKernelGGL((poa_forward_kernel<decltype(q)::value, decltype(cell), true, false>), grid, block, 0, stream, fp, tp);
        else hipLaunchKernelGGL((poa_forward_kernel<decltype(q)::value, decltype(cell), false, false>), grid, block, 0, stream, fp, tp);
    };
    switch (c.v[0]) {
    case POA_KERNEL_PX:
        if (c.mf == 3) hipLaunchKernelGGL(poa_forward_px_kernel<3>, grid, block, 0, stream, fp);
        else if (c.mf == 2) hipLaunchKernelGGL(poa_forward_px_kernel<2>, grid, block, 0, stream, fp);
        else if (c.mf == 1) hipLaunchKernelGGL(poa_forward_px_kernel<1>, grid, block, 0, stream, fp);
        else hipLaunchKernelGGL(poa_forward_px_kernel<0>, grid, block, 0, stream, fp);
        break;
    case POA_KERNEL_PXMW:
        hipLaunchKernelGGL(poa_forward_pxmw_kernel, grid, block, 0, stream, fp);
        break;
    case POA_KERNEL_PACKED:
        if (mw && quads == 1) hipLaunchKernelGGL((poa_forward_packed_kernel<1, false, true>), grid, block, 0, stream, fp, tp);
        else if (mw) hipLaunchKernelGGL((poa_forward_packed_kernel<2, false, true>), grid, block, 0, stream, fp, tp);
        else if (quads == 1 && fuse) hipLaunchKernelGGL((poa_forward_packed_kernel<1, true, false>), grid, block, 0, stream, fp, tp);
        else if (quads == 1) hipLaunchKernelGGL((poa_forward_packed_kernel<1, false, false>), grid, block, 0, stream, fp, tp);
        else if (fuse) hipLaunchKernelGGL((poa_forward_packed_kernel<2, true, false>), grid, block, 0, stream, fp, tp);
        else hipLaunchKernelGGL((poa_forward_packed_kernel<2, false, false>), grid, block, 0, stream, fp, tp);
        break;
    default:   // POA_KERNEL_FORWARD
        if (mw && quads == 4) hipLaunchKernelGGL((poa_forward_kernel<4, uint32_t, false, false, true>), grid, block, 0, stream, fp, tp);
        else if (mw) hipLaunchKernelGGL((poa_forward_kernel<2, uint32_t, false, false, true>), grid, block, 0, stream, fp, tp);
        else if (R.compact && quads == 1) hipLaunchKernelGGL((poa_forward_kernel<1, uint16_t, false, true>), grid, block, 0, stream, fp, tp);
        else if (R.compact) hipLaunchKernelGGL((poa_forward_kernel<2, uint16_t, false, true>), grid, block, 0, stream, fp, tp);
        else if (R.narrow && quads == 1) plain(uint16_t{}, integral_constant<int, 1>{});
        else if (R.narrow) plain(uint16_t{}, integral_constant<int, 2>{});
        else if (quads == 1) plain(uint32_t{}, integral_constant<int, 1>{});
        else if (quads == 2) plain(uint32_t{}, integral_constant<int, 2>{});
        else plain(uint32_t{}, integral_constant<int, 4>{});
    }
}

// the banded pass, then the full pass (the same kernel with eight registers per row array and one window of 1024 columns) over
// the queries it could not certify: the grid is sized for the chunk and the waves past the device-side count return at once,
// so the host never waits for the count
int launch_band(poa_batch* b, size_t ci, const DenseRunPlan& R, const FwdParams& fp, hipStream_t stream) {
    const poa_batch::Chunk& ch = b->cur().chunks[ci];
    const uint32_t blocks = (ch.count + 3) / 4;
    if (const int rc = prepare_band(b)) return rc;
    BandParams bp;
    bp.cls = b->d_band_cls.p; bp.cls_d = b->d_band_d.p; bp.cls_base = b->d_band_base.p; bp.n_seg = b->band_n_seg;
    bp.d_cap = R.band_cap; bp.list = b->d_band_list.p; bp.count = b->d_band_count.p + ci; bp.order = nullptr;
    bp.n_order = nullptr; bp.count_nf = nullptr;
    const size_t n_chunks = b->cur().chunks.size();
    uint32_t n_pairs = 0, n_narrow = 0;
    if (R.band_pair != 0) {
        if (const int rc = prepare_band_pairs(b)) return rc;
        n_pairs = b->h_band_npair[ci];
        const bool by_rule = band_pair_rule(2 * n_pairs);
        if (R.band_pair < 0 && !by_rule) n_pairs = 0;
        if (n_pairs) n_narrow = band_narrow_pairs(R, by_rule, b->h_band_nnarrow_rule[ci], b->h_band_nnarrow_any[ci]);
    }
    if (n_pairs) {
        // the pairs, then the singles one per wave: grids sized on the host, nothing read back
        const uint32_t n_single = ch.count - 2 * n_pairs;
        FwdParams fq = fp;
        BandParams bq = bp;
        if (n_narrow) {
            // the narrow tier over the leading pairs, under the classes' narrow plan; what it cannot certify goes to a list of
            // its own, which the 512 pass works off one query per wave (its grid sized for all of them: the waves past the
            // device-side count return at once); what that pass cannot certify joins the full pass's list
            BandParams bn = bp;
            bn.cls_d = b->d_band_dn.p; bn.cls_base = b->d_band_base_n.p;
            bn.list = b->d_band_list_n.p; bn.count = b->d_band_count.p + n_chunks + ci;
            fq.n_queries = n_narrow; bn.order = b->d_band_order.p + ch.first;
            hipLaunchKernelGGL(poa_forward_band2_kernel<6>, dim3((n_narrow + 3) / 4), dim3(256), 0, stream, fq, bn);
            HIP_TRY(hipGetLastError());
            fq.n_queries = 2 * n_narrow; bq.order = b->d_band_list_n.p + fp.first_query;
            bq.n_order = bn.count; bq.count_nf = b->d_band_count.p + 2 * n_chunks + ci;
            hipLaunchKernelGGL((poa_forward_band_kernel<false, true>), dim3((2 * n_narrow + 3) / 4), dim3(256), 0, stream, fq, bq);
            HIP_TRY(hipGetLastError());
            bq.n_order = nullptr; bq.count_nf = nullptr;
            b->narrow_ran += 2 * n_narrow; b->narrow_chunks = (uint32_t)ci + 1;
            b->narrow_how = R.band_narrow > 0 ? 2u : 1u;
        }
        if (n_pairs > n_narrow) {
            fq.n_queries = n_pairs - n_narrow; bq.order = b->d_band_order.p + ch.first + 2 * n_narrow;
            hipLaunchKernelGGL(poa_forward_band2_kernel<8>, dim3((n_pairs - n_narrow + 3) / 4), dim3(256), 0, stream, fq, bq);
        }
        if (n_single) {
            HIP_TRY(hipGetLastError());
            fq.n_queries = n_single; bq.order = b->d_band_order.p + ch.first + 2 * n_pairs;
            hipLaunchKernelGGL((poa_forward_band_kernel<false, true>), dim3((n_single + 3) / 4), dim3(256), 0, stream, fq, bq);
        }
        b->pair_paired += 2 * n_pairs; b->pair_single += n_single;
    } else {
        hipLaunchKernelGGL(poa_forward_band_kernel<false>, dim3(blocks), dim3(256), 0, stream, fp, bp);
        b->pair_single += ch.count;
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(poa_forward_band_kernel<true>, dim3(blocks), dim3(256), 0, stream, fp, bp);
    uint32_t min_d = 0xFFFFFFFFu;
    for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) min_d = std::min(min_d, std::min(b->h_band_d[b->h_band_cls[i]], R.band_cap));
    // (the queries of the narrow tier: the D of the tier that ran first)
    for (uint32_t k = 0; k < 2 * n_narrow; ++k) min_d = std::min(min_d, std::min(b->h_band_dn[b->h_band_cls[b->h_band_order[ch.first + k]]], R.band_cap));
    b->band_min_d = b->band_used ? std::min(b->band_min_d, min_d) : min_d;
    b->band_used = true; b->band_queries += ch.count; b->band_chunks = (uint32_t)ci + 1;
    return POA_OK;
}

// the separate traceback launch of a chunk: 256 / lanes walks per workgroup; the compact layout at the depth that goes with its lanes
void launch_traceback(const DenseRunPlan& R, const DenseChunkPlan& c, const TbParams& tp, hipStream_t stream) {
    const uint32_t lanes = c.v[5], per_block = 256 / lanes;
    const dim3 grid((c.v[7] + per_block - 1) / per_block), block(256);
    TbParams tpg = tp;
    tpg.spec_depth = c.v[6];
    if (c.lean_tb && lanes == 16) hipLaunchKernelGGL((poa_traceback_mf_kernel<16>), grid, block, 0, stream, tpg);
    else if (c.lean_tb && lanes == 32) hipLaunchKernelGGL((poa_traceback_mf_kernel<32>), grid, block, 0, stream, tpg);
    else if (c.lean_tb && lanes == 8) hipLaunchKernelGGL((poa_traceback_mf_kernel<8>), grid, block, 0, stream, tpg);
    else if (c.lean_tb) hipLaunchKernelGGL((poa_traceback_mf_kernel<64>), grid, block, 0, stream, tpg);
    else if (R.compact && lanes == 16) hipLaunchKernelGGL((poa_traceback_kernel<uint16_t, true, 16>), grid, block, 0, stream, tpg);
    else if (R.compact && lanes == 32) hipLaunchKernelGGL((poa_traceback_kernel<uint16_t, true, 32>), grid, block, 0, stream, tpg);
    else if (R.compact && lanes == 8) hipLaunchKernelGGL((poa_traceback_kernel<uint16_t, true, 8>), grid, block, 0, stream, tpg);
    else if (R.compact) hipLaunchKernelGGL((poa_traceback_kernel<uint16_t, true>), grid, block, 0, stream, tpg);
    else if (R.narrow) hipLaunchKernelGGL((poa_traceback_kernel<uint16_t, false>), grid, block, 0, stream, tp);
    else hipLaunchKernelGGL((poa_traceback_kernel<uint32_t, false>), grid, block, 0, stream, tp);
}

// ---- exact replay of the reference's search on the (re-initialised, u32) planes of a chunk ---------------------------------
// what the wave and the flat search take alike: the chunked queues in the pool (POA_WS_CHUNK_CAP caps them), the descriptor ring's
// size, the counters, the per-phase cycle counts (POA_WS_PROF: diagnostics) and, until a persistent schedule says otherwise, no order
template <typename SearchParams>
void fill_search_params(SearchParams& sp, poa_batch* b, const ExactParams& ep, const TuneView& T) {
    sp.E = ep;
    sp.chunks = reinterpret_cast<ExU4*>(b->d_ex_pool.p);
    sp.chunk_cap = b->ex_pool_cap / BQ_CHUNK;
    if (const int* cv = T.ptr(POA_TUNE_WS_CHUNK_CAP)) { const int v = (*cv); if (v >= 1 && (uint32_t)v < sp.chunk_cap) sp.chunk_cap = (uint32_t)v; }
    sp.win = b->ex_win;
    sp.counters = b->d_ex_counters.p;
    sp.prof = T.ptr(POA_TUNE_WS_PROF) ? b->d_ex_prof.p : nullptr;
    sp.work_counter = nullptr; sp.order = nullptr;
}

// blocks of a replay kernel that are resident on the device at once
uint32_t resident_blocks(poa_batch* b, const void* kfn, uint32_t wpb, uint32_t lds_bytes) {
    int per_cu = 1, cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, (int)(64 * wpb), lds_bytes) != hipSuccess || per_cu < 1) per_cu = 1;
    return (uint32_t)cus * (uint32_t)per_cu;
}

// persistent waves: as many blocks as are resident at once; queries handed out longest-expected-search first (by the dense
// pass's score: more edits, more buckets).  The sort needs the scores on the host: one small copy behind the dense pass of
// this chunk.  Sets the work counter and the order of `sp` and cuts n_blocks to `resident`.
template <typename SearchParams>
int persistent_schedule(poa_batch* b, const poa_batch::Chunk& ch, uint32_t resident, hipStream_t stream, SearchParams& sp, uint32_t& n_blocks) {
    std::vector<uint32_t> sc(ch.count), ord(ch.count);
    HIP_TRY(hipMemcpyAsync(sc.data(), b->d_score.p + ch.first, (size_t)ch.count * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < ch.count; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t c2) { return sc[a] > sc[c2]; });
    HIP_TRY(b->d_ex_order.alloc(ch.count + 1));
    HIP_TRY(hipMemcpyAsync(b->d_ex_order.p + 1, ord.data(), (size_t)ch.count * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(b->d_ex_order.p, 0, 4, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // `ord` is a host temporary
    sp.work_counter = b->d_ex_order.p; sp.order = b->d_ex_order.p + 1;
    n_blocks = resident;
    return POA_OK;
}

// "flat": the parallel-step kernel (poa_fsearch.hpp) — bit-identical like the others, not the fastest yet.
// The next entries in pop order expanded at once, one per lane, several queries per wave.
int replay_flat(poa_batch* b, const poa_batch::Chunk& ch, const ExactParams& ep, const TuneView& T, bool ends_free, int lds_cap, hipStream_t stream) {
    const FlatGraph& fg = b->graph->g;
    const uint32_t win = b->ex_win, graph_lds = exact_lds_bytes(fg.n, ep.n_succ, ep.n_nbm);
    FSearchParams pp;
    fill_search_params(pp, b, ep, T);
    pp.max_lanes = 63;   // (capped at the group's lanes below)
    if (const int* lv = T.ptr(POA_TUNE_PS_LANES)) { const int v = (*lv); if (v >= 1 && v <= 63) pp.max_lanes = (uint32_t)v; }
    // Lanes per query: a step commits a dozen lanes on the benchmark's reads, and the kernel waits for memory more than it
    // issues — so four searches share a wave (16 lanes each), all stepping through one instruction stream.
    pp.lean = (!fg.row_rec.empty() && !ends_free) ? 1u : 0u;
    if (const int* lv = T.ptr(POA_TUNE_PS_LEAN)) pp.lean = (pp.lean && (*lv) != 0) ? 1u : 0u;
    const uint32_t group = pp.lean ? 8u : 16u;   // (the group sizes poa_fsearch.hpp is built for)
    const uint32_t qpw = 64 / group;
    pp.group = group;
    if (pp.max_lanes > group) pp.max_lanes = group;
    // LDS of a block: the staged graph (shared by its waves) + per wave the descriptor rings of its queries and the
    // logs / read sets / conflict tables of the step.  As many waves per block as fit 160 KB, at most 8 (two per SIMD:
    // the kernel keeps a lane's search state in ~250 registers).
    const uint64_t lds_budget = std::min<uint64_t>((uint64_t)lds_cap, 160u * 1024u);
    const uint64_t ring_b = ((uint64_t)qpw * 3 * win * 4 + 15) & ~15ull;
    // the lean step reads one 32-byte record per row: those are staged (the arrays of the generic code, which it
    // falls back to for a row in a thousand, stay in global memory); without records the generic code runs in log mode
    const uint64_t rec_b = pp.lean ? ((sizeof(FlatGraph::RowRec) * (uint64_t)fg.n + 15) & ~15ull) : 0;
    const uint64_t stage_b = pp.lean ? rec_b : graph_lds;
    bool ring_lds = ring_b + ps_lds_bytes() <= lds_budget && !T.ptr(POA_TUNE_WS_RING_GLOBAL);
    uint64_t per_wave = (ring_lds ? ring_b : 0) + ps_lds_bytes();
    bool stage = stage_b + per_wave <= lds_budget;
    if (const int* gv = T.ptr(POA_TUNE_EXACT_LDS)) stage = stage && (*gv) != 0;
    uint32_t wpb = (uint32_t)std::min<uint64_t>(8, (lds_budget - (stage ? stage_b : 0)) / per_wave);
    if (const int* wv = T.ptr(POA_TUNE_WS_WAVES)) { const int v = (*wv); if (v >= 1 && (uint32_t)v <= wpb) wpb = (uint32_t)v; }
    if (wpb < 1) return fail(POA_ERR_UNSUPPORTED, "exact replay: the step's logs do not fit the LDS");
    pp.graph_lds = (stage && !pp.lean) ? graph_lds : 0;
    pp.rec_lds = (stage && pp.lean) ? (uint32_t)rec_b : 0;
    pp.waves_per_block = wpb;
    pp.ring_global = ring_lds ? nullptr : b->d_ex_head.p;   // [slots * 3 * ex_n_prio] holds slots * 3 * win
    const uint32_t lds_bytes = pp.graph_lds + pp.rec_lds + (uint32_t)(wpb * per_wave);
    const void* kfn = pp.lean ? reinterpret_cast<const void*>(poa_fsearch_lean_kernel) : reinterpret_cast<const void*>(poa_fsearch_kernel);
    if (lds_bytes > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    const uint32_t per_block = wpb * qpw;
    uint32_t n_blocks = (ch.count + per_block - 1) / per_block;
    const uint32_t resident = resident_blocks(b, kfn, wpb, lds_bytes);
    if (n_blocks > resident && !T.ptr(POA_TUNE_WS_STATIC)) {   // persistent waves, longest expected search first
        if (const int rc = persistent_schedule(b, ch, resident, stream, pp, n_blocks)) return rc;
    }
    b->replays.push_back({{pp.lean ? (uint32_t)POA_REPLAY_FLAT_LEAN : (uint32_t)POA_REPLAY_FLAT_GENERIC, win, group, wpb,
                           (pp.graph_lds || pp.rec_lds ? POA_REPLAY_BIT_GRAPH_LDS : 0u) | (pp.rec_lds ? POA_REPLAY_BIT_REC_LDS : 0u) |
                               (pp.ring_global ? POA_REPLAY_BIT_RING_GLOBAL : 0u) | (pp.order ? POA_REPLAY_BIT_PERSISTENT : 0u),
                           resident, n_blocks, lds_bytes}});
    HIP_TRY(b->d_ex_logs.alloc((size_t)n_blocks * wpb * ps_scratch_words()));
    pp.scratch = b->d_ex_logs.p;
    if (pp.lean) hipLaunchKernelGGL(poa_fsearch_lean_kernel, dim3(n_blocks), dim3(64 * wpb), lds_bytes, stream, pp);
    else hipLaunchKernelGGL(poa_fsearch_kernel, dim3(n_blocks), dim3(64 * wpb), lds_bytes, stream, pp);
    return POA_OK;
}

// wave-per-query search (poa_wsearch.hpp)
int replay_wave(poa_batch* b, const poa_batch::Chunk& ch, const ExactParams& ep, const TuneView& T, int lds_cap, hipStream_t stream) {
    const FlatGraph& fg = b->graph->g;
    const uint32_t win = b->ex_win, graph_lds = exact_lds_bytes(fg.n, ep.n_succ, ep.n_nbm);
    WSearchParams wp;
    fill_search_params(wp, b, ep, T);
    wp.max_lanes = 32;   // entries tested per step at most: runs of stale / pruned entries are short (1.85 pops per step)
    if (const int* lv = T.ptr(POA_TUNE_WS_LANES)) { const int v = (*lv); if (v >= 1 && v <= 63) wp.max_lanes = (uint32_t)v; }
    wp.adapt_lanes = 4;   // after an expansion the top of the stack is fresh: few entries tested; a run that used up its lanes widens
    if (const int* av = T.ptr(POA_TUNE_WS_ADAPT)) { const int v = (*av); if (v >= 0 && v <= 63) wp.adapt_lanes = (uint32_t)v; }
    // Lanes per query.  One query per wave (64) with persistent scheduling is the default.  Several queries per wave
    // (POA_WS_GROUP = 32 / 16 / 8 lanes each, all through one instruction stream) issue fewer instructions in
    // all but lose: the iteration takes the union of the groups' code paths and every wave waits for its slowest
    // query (measured on config 2, 10 000 queries: 1.09 s at 64 persistent, 1.83 s at 64 static, 1.49 / 1.85 /
    // 2.53 s at 32 / 16 / 8).  Waves per block: as many as share one staged copy of the graph, at most 16.
    uint32_t group = 64;
    if (const int* gv = T.ptr(POA_TUNE_WS_GROUP)) { const int v = (*gv); if (v == 8 || v == 16 || v == 32 || v == 64) group = (uint32_t)v; }
    uint32_t wpb = 16;
    if (const int* wv = T.ptr(POA_TUNE_WS_WAVES)) { const int v = (*wv); if (v >= 1 && v <= 16) wpb = (uint32_t)v; }
    const uint64_t lds_budget = std::min<uint64_t>((uint64_t)lds_cap, 80u * 1024u);
    bool ring_lds = false, stage = false;
    // per-row records of the one-round-trip path (one query per wave: a block of 16 waves has the CU to itself)
    uint32_t rec_lds = 0;
    for (;;) {
        const uint64_t rb = (uint64_t)wpb * (64 / group) * win * 12;
        ring_lds = rb <= lds_budget && !T.ptr(POA_TUNE_WS_RING_GLOBAL);
        stage = graph_lds + (ring_lds ? rb : 0) <= lds_budget;
        if (const int* gv = T.ptr(POA_TUNE_EXACT_LDS)) stage = stage && (*gv) != 0;
        if (group == 64 || (ring_lds && stage)) break;
        // several queries per wave need everything in LDS: fewer waves per block first, then fewer queries per wave
        if (wpb > 2 && !T.ptr(POA_TUNE_WS_WAVES)) wpb /= 2; else { group *= 2; if (!T.ptr(POA_TUNE_WS_WAVES)) wpb = 16; }
    }
    const uint64_t ring_bytes = ring_lds ? (uint64_t)wpb * (64 / group) * win * 12 : 0;
    if (group == 64 && stage && ring_lds && !fg.row_rec.empty() && !(T.ptr(POA_TUNE_WS_REC) && *T.ptr(POA_TUNE_WS_REC) == 0)) {
        const uint64_t rb = (fg.row_rec.size() * sizeof(FlatGraph::RowRec) + 15) & ~15ull;
        if (graph_lds + rb + ring_bytes <= std::min<uint64_t>((uint64_t)lds_cap, 150u * 1024u)) rec_lds = (uint32_t)rb;
    }
    wp.rec_lds = rec_lds;
    wp.graph_lds = stage ? graph_lds : 0;
    wp.waves_per_block = wpb;
    wp.group = group;
    wp.ring_global = nullptr;
    if (!ring_lds) wp.ring_global = b->d_ex_head.p;  // [slots * 3 * ex_n_prio] holds slots * 3 * win
    const uint32_t lds_bytes = wp.graph_lds + wp.rec_lds + (uint32_t)ring_bytes;
    const bool lds_all = wp.graph_lds && !wp.ring_global;   // (else the kernel whose search reads through generic pointers)
    const void* kfn = group != 64 ? reinterpret_cast<const void*>(poa_wsearch_groups_kernel)
                                  : (lds_all ? reinterpret_cast<const void*>(poa_wsearch_kernel) : reinterpret_cast<const void*>(poa_wsearch_global_kernel));
    if (lds_bytes > 48u * 1024u)
        HIP_TRY(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    const uint32_t per_block = wpb * (64 / group);
    uint32_t n_blocks = (ch.count + per_block - 1) / per_block, resident = 0;
    if (group == 64 && !T.ptr(POA_TUNE_WS_STATIC)) {
        resident = resident_blocks(b, kfn, wpb, lds_bytes);
        if (n_blocks > resident) { if (const int rc = persistent_schedule(b, ch, resident, stream, wp, n_blocks)) return rc; }
    }
    b->replays.push_back({{group != 64 ? (uint32_t)POA_REPLAY_WAVE_GROUPS : (lds_all ? (uint32_t)POA_REPLAY_WAVE_LDS : (uint32_t)POA_REPLAY_WAVE_GENERIC),
                           win, group, wpb,
                           (wp.graph_lds ? POA_REPLAY_BIT_GRAPH_LDS : 0u) | (wp.rec_lds ? POA_REPLAY_BIT_REC_LDS : 0u) |
                               (wp.ring_global ? POA_REPLAY_BIT_RING_GLOBAL : 0u) | (wp.order ? POA_REPLAY_BIT_PERSISTENT : 0u),
                           resident, n_blocks, lds_bytes}});
    if (group != 64) hipLaunchKernelGGL(poa_wsearch_groups_kernel, dim3(n_blocks), dim3(64 * wpb), lds_bytes, stream, wp);
    else if (lds_all) hipLaunchKernelGGL(poa_wsearch_kernel, dim3(n_blocks), dim3(64 * wpb), lds_bytes, stream, wp);
    else hipLaunchKernelGGL(poa_wsearch_global_kernel, dim3(n_blocks), dim3(64 * wpb), lds_bytes, stream, wp);
    return POA_OK;
}

// one sequential search per lane (poa_exact_kernel)
int replay_lane(poa_batch* b, const poa_batch::Chunk& ch, ExactParams ep, const TuneView& T, hipStream_t stream) {
    const FlatGraph& fg = b->graph->g;
    // active lanes per wave: one sequential search per lane.  Few lanes = little divergence but many
    // waves; enough waves to fill the chip (~16 per CU) first, then more lanes per wave.
    uint32_t lanes = (ch.count + 4095) / 4096;
    if (lanes > 64) lanes = 64;
    if (const int* lv = T.ptr(POA_TUNE_EXACT_LANES)) { const int v = (*lv); if (v >= 1 && v <= 64) lanes = (uint32_t)v; }
    ep.lanes_per_wave = lanes;
    // graph arrays in LDS when they fit beside three other blocks of the same CU (160 KB per CU)
    uint32_t lds_bytes = exact_lds_bytes(fg.n, ep.n_succ, ep.n_nbm);
    bool lds_graph = lds_bytes <= 160u * 1024u / 3u;
    if (const int* gv = T.ptr(POA_TUNE_EXACT_LDS)) lds_graph = lds_graph && (*gv) != 0;
    if (lds_graph && lds_bytes > 48u * 1024u)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(poa_exact_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    ep.lds_graph = lds_graph ? 1u : 0u;
    if (lds_graph && !T.ptr(POA_TUNE_EXACT_LANES)) {
        // all blocks resident at once (no tail round): LDS bounds the blocks per CU
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device);
        const uint32_t per_cu = std::max(1u, std::min(8u, 160u * 1024u / std::max(lds_bytes, 1u)));
        const uint32_t cap_waves = (uint32_t)cus * per_cu * (EXACT_BLOCK / 64);
        lanes = std::min(64u, std::max(lanes, (ch.count + cap_waves - 1) / cap_waves));
        ep.lanes_per_wave = lanes;
    }
    const uint32_t per_block = lanes * (EXACT_BLOCK / 64);
    b->replays.push_back({{POA_REPLAY_LANE, b->ex_win, 1u, EXACT_BLOCK / 64, lds_graph ? POA_REPLAY_BIT_GRAPH_LDS : 0u, 0u,
                           (ch.count + per_block - 1) / per_block, lds_graph ? lds_bytes : 0u}});
    hipLaunchKernelGGL(poa_exact_kernel, dim3((ch.count + per_block - 1) / per_block), dim3(EXACT_BLOCK), lds_graph ? lds_bytes : 0, stream, ep);
    return POA_OK;
}

// the replay's view of a chunk: graph tables, queries, planes, queues, costs and the ends-free bounds
ExactParams exact_params(poa_batch* b, const poa_batch::Chunk& ch, const poa_costs_t* costs, const poa_config_t* cfg, uint32_t hybrid, bool ends_free) {
    const FlatGraph& fg = b->graph->g;
    ExactParams ep;
    ep.G = ExactGraph{fg.n, fg.start_row, fg.end_row, b->d_ex_sym.p, b->d_succ_off.p, b->d_succ_rows.p, b->d_dist_min.p,
                      b->d_dist_max.p, b->d_exit_idx.p, fg.n_exit, b->d_nbm_off.p, b->d_nbm.p, b->d_node_row.p, b->d_sp_to_end.p,
                      fg.row_rec.empty() ? nullptr : b->d_ex_rec.p};
    ep.first_query = ch.first; ep.n_queries = ch.count; ep.hybrid = hybrid; ep.dense_flags = b->d_flags.p;
    ep.qseq = b->d_qseq.p; ep.qoff = b->d_qoff.p; ep.pitch = b->d_pitch.p; ep.plane_off = b->cur().d_off.p;
    ep.planes = b->d_planes.p;
    ep.reached = b->d_ex_reached.p; ep.rsum = b->d_ex_rsum.p; ep.wpn = b->ex_wpn; ep.swpn = b->ex_swpn;
    ep.head = b->d_ex_head.p; ep.n_prio = b->ex_n_prio; ep.pool = b->d_ex_pool.p; ep.pool_cap = b->ex_pool_cap;
    ep.stack = b->d_ex_stack.p; ep.stack_cap = b->ex_stack_cap;
    ep.C = ExactCosts{costs->mismatch, costs->gap_open, costs->gap_extend, cfg ? cfg->heuristic : POA_HEURISTIC_MINGAP,
                      cfg ? cfg->pruning : 1u, 0, 0, 0, 0, 0, 0};
    if (ends_free) {
        ep.C.ends_free = 1;
        ep.C.qfe_kind = cfg->qry_free_end.kind; ep.C.qfe_val = cfg->qry_free_end.value;
        ep.C.gfb_kind = cfg->graph_free_begin.kind;
        ep.C.gfe_kind = cfg->graph_free_end.kind; ep.C.gfe_val = cfg->graph_free_end.value;
    }
    ep.status = b->d_ex_status.p;
    ep.end_cell = b->d_ex_end.p;
    ep.n_succ = (uint32_t)fg.succ_rows.size(); ep.n_nbm = (uint32_t)fg.nbm.size();
    return ep;
}

// exact / hybrid mode: the replay of one chunk behind its dense pass, then the u32 traceback over what it left (`tp`: the dense
// pass's traceback parameters)
int replay_chunk(poa_batch* b, const poa_batch::Chunk& ch, const poa_costs_t* costs, const poa_config_t* cfg, const TuneView& T, uint32_t hybrid,
                 bool ends_free, TbParams tp, hipStream_t stream) {
    const FlatGraph& fg = b->graph->g;
    HIP_TRY(hipMemsetAsync(b->d_ex_status.p + ch.first, 0xFF, (size_t)ch.count * 4, stream));
    HIP_TRY(hipMemsetAsync(b->d_ex_counters.p + 4 * (size_t)ch.first, 0, (size_t)ch.count * 16, stream));
    hipLaunchKernelGGL(poa_fill_planes_kernel, dim3(64, ch.count), dim3(256), 0, stream, b->d_planes.p, b->cur().d_off.p,
                       b->d_pitch.p, fg.n, ch.first, hybrid, b->d_flags.p);
    HIP_TRY(hipGetLastError());
    if (fg.n_exit) {
        HIP_TRY(hipMemsetAsync(b->d_ex_reached.p, 0, (size_t)ch.count * fg.n_exit * b->ex_wpn * 8, stream));
        HIP_TRY(hipMemsetAsync(b->d_ex_rsum.p, 0, (size_t)ch.count * fg.n_exit * b->ex_swpn * 8, stream));
    }
    HIP_TRY(hipMemsetAsync(b->d_ex_head.p, 0xFF, (size_t)ch.count * 3 * b->ex_n_prio * 4, stream));
    const ExactParams ep = exact_params(b, ch, costs, cfg, hybrid, ends_free);
    // Wave-per-query search (poa_wsearch.hpp) unless its descriptor ring cannot hold the priorities that are live
    // at once: one pop pushes at most max(x, o+e) above its own priority plus what the heuristic can jump along
    // one edge and a state change (o), and the greedy extension walks that jump once more.
    // live priority range: a pop at priority f pushes at most max(x, o+e) + o + e * (spread + 3) above f, where
    // spread = max over nodes of dist_max - dist_min (the heuristic's gap length grows by at most that along any
    // greedy extension: heuristic.rs:70-102)
    int lds_cap = 64 * 1024;
    (void)hipDeviceGetAttribute(&lds_cap, hipDeviceAttributeMaxSharedMemoryPerBlock, b->device);
    const int* impl = T.ptr(POA_TUNE_EXACT_IMPL);   // 1 lane, 2 wave, 3 flat
    const bool wave_search = !(impl && *impl == 1) && b->ex_win <= b->ex_n_prio;
    int rc;
    if (wave_search && impl && *impl == 3) rc = replay_flat(b, ch, ep, T, ends_free, lds_cap, stream);
    else if (wave_search) rc = replay_wave(b, ch, ep, T, lds_cap, stream);
    else rc = replay_lane(b, ch, ep, T, stream);
    if (rc != POA_OK) return rc;
    HIP_TRY(hipGetLastError());
    tp.exact_pass = 1; tp.ex_status = b->d_ex_status.p; tp.ex_end = b->d_ex_end.p; tp.row_depth = nullptr;
    hipLaunchKernelGGL((poa_traceback_kernel<uint32_t, false>), dim3((ch.count + 3) / 4), dim3(256), 0, stream, tp);
    HIP_TRY(hipGetLastError());
    b->narrow = false; b->compact = false; b->relative = false;  // the planes now hold the replayed u32 table
    return POA_OK;
}
}  // namespace

extern "C" {

const char* poa_version(void) { return "poasta_amd 0.2 (gfx950)"; }
const char* poa_last_error(void) { return g_err.c_str(); }

int poa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int poa_graph_create(uint32_t n, uint32_t start, uint32_t end, const uint8_t* symbol, const uint32_t* succ_off,
                     const uint32_t* succ, const uint32_t* pred_off, const uint32_t* pred, poa_graph_t** out) {
    if (!out) return fail(POA_ERR_INVALID_ARG, "poa_graph_create: out is null");
    *out = nullptr;
    std::unique_ptr<poa_graph> h(new (std::nothrow) poa_graph);
    if (!h) return fail(POA_ERR_OUT_OF_MEMORY, "poa_graph_create: host allocation failed");
    std::string err;
    int rc;
    try {
        rc = build_flat_graph(n, start, end, symbol, succ_off, succ, pred_off, pred, h->g, err);
    } catch (const std::bad_alloc&) {
        return fail(POA_ERR_OUT_OF_MEMORY, "poa_graph_create: host allocation failed");
    }
    if (rc != POA_OK) return fail(rc, err);
    try {
        build_sweep_rows(h->g, h->sweep);
        build_checkpoint_plan(h->g, h->sweep, 0, h->ckpt);
        build_checkpoint_plan(h->g, h->sweep, 0, h->ckpt2, true);
    } catch (const std::bad_alloc&) {
        return fail(POA_ERR_OUT_OF_MEMORY, "poa_graph_create: host allocation failed");
    }
    *out = h.release();
    return POA_OK;
}

void poa_graph_destroy(poa_graph_t* g) { delete g; }
uint32_t poa_graph_rows(const poa_graph_t* g) { return g ? g->g.n : 0; }
int poa_graph_update(poa_graph_t* g, uint32_t n, uint32_t start, uint32_t end, const uint8_t* symbol, const uint32_t* succ_off,
                     const uint32_t* succ, const uint32_t* pred_off, const uint32_t* pred) {
    if (!g) return fail(POA_ERR_INVALID_ARG, "poa_graph_update: null graph");
    std::string err;
    int rc;
    FlatGraph ng;
    SweepRows nsw;
    CheckpointPlan nck, nck2;
    try {
        rc = build_flat_graph(n, start, end, symbol, succ_off, succ, pred_off, pred, ng, err);
        if (rc == POA_OK) { build_sweep_rows(ng, nsw); build_checkpoint_plan(ng, nsw, 0, nck); build_checkpoint_plan(ng, nsw, 0, nck2, true); }
    } catch (const std::bad_alloc&) {
        return fail(POA_ERR_OUT_OF_MEMORY, "poa_graph_update: host allocation failed");
    }
    if (rc != POA_OK) return fail(rc, err);   // (the handle keeps the graph it had)
    std::lock_guard<std::mutex> lk(g->bubble_mu);
    g->g = std::move(ng);
    g->sweep = std::move(nsw);
    g->ckpt = std::move(nck);
    g->ckpt2 = std::move(nck2);
    return POA_OK;
}

int poa_graph_sweep_checks(const poa_graph_t* g, uint32_t stride, uint8_t* check, uint32_t* n_checks) {
    if (!g || !n_checks) return fail(POA_ERR_INVALID_ARG, "poa_graph_sweep_checks: null argument");
    std::vector<uint32_t> rows;
    try {
        build_sweep_checks(g->sweep.cut.data(), (uint32_t)g->sweep.cut.size(), stride, rows);
    } catch (const std::bad_alloc&) { return fail(POA_ERR_OUT_OF_MEMORY, "poa_graph_sweep_checks: host allocation failed"); }
    if (check) {
        std::memset(check, 0, g->sweep.cut.size());
        for (uint32_t r : rows) check[r] = 1;
    }
    *n_checks = (uint32_t)rows.size();
    return POA_OK;
}

int poa_graph_sweep_slots(const poa_graph_t* g, uint32_t* slot, uint32_t* n_slots) {
    if (!g || !n_slots) return fail(POA_ERR_INVALID_ARG, "poa_graph_sweep_slots: null argument");
    if (slot && !g->sweep.slot.empty()) std::memcpy(slot, g->sweep.slot.data(), g->sweep.slot.size() * sizeof(uint32_t));
    *n_slots = g->sweep.n_slots;
    return POA_OK;
}

static int checkpoint_plan_out(const poa_graph_t* g, bool two_piece, uint32_t segment_rows, uint32_t* n_segments, uint32_t* boundary, uint32_t* rows_per_query) {
    const std::string who = two_piece ? "poa_graph_checkpoint_plan2" : "poa_graph_checkpoint_plan";
    if (!g || !n_segments || !rows_per_query) return fail(POA_ERR_INVALID_ARG, who + ": null argument");
    CheckpointPlan own;
    const CheckpointPlan* pl = two_piece ? &g->ckpt2 : &g->ckpt;
    if (segment_rows != 0 && segment_rows != pl->segment_rows) {
        try {
            build_checkpoint_plan(g->g, g->sweep, segment_rows, own, two_piece);
        } catch (const std::bad_alloc&) { return fail(POA_ERR_OUT_OF_MEMORY, who + ": host allocation failed"); }
        pl = &own;
    }
    *n_segments = pl->n_segments();
    *rows_per_query = pl->rows_per_query;
    if (boundary) std::memcpy(boundary, pl->boundary.data(), pl->boundary.size() * sizeof(uint32_t));
    return POA_OK;
}

int poa_graph_checkpoint_plan(const poa_graph_t* g, uint32_t segment_rows, uint32_t* n_segments, uint32_t* boundary, uint32_t* rows_per_query) {
    return checkpoint_plan_out(g, false, segment_rows, n_segments, boundary, rows_per_query);
}

int poa_graph_checkpoint_plan2(const poa_graph_t* g, uint32_t segment_rows, uint32_t* n_segments, uint32_t* boundary, uint32_t* rows_per_query) {
    return checkpoint_plan_out(g, true, segment_rows, n_segments, boundary, rows_per_query);
}

int poa_graph_node_rows(const poa_graph_t* g, uint32_t* rank) {
    if (!g || !rank) return fail(POA_ERR_INVALID_ARG, "poa_graph_node_rows: null argument");
    std::memcpy(rank, g->g.node_row.data(), g->g.n * sizeof(uint32_t));
    return POA_OK;
}

static int batch_create_impl(const poa_graph_t* g, int device, uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff,
                             uint64_t workspace_bytes, bool sweep, poa_batch_t** out, bool ckpt = false, uint32_t ckpt_rows = 0, bool ckpt2 = false);

int poa_batch_create(const poa_graph_t* g, int device, uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff,
                     uint64_t workspace_bytes, poa_batch_t** out) {
    return batch_create_impl(g, device, n_queries, qseq, qoff, workspace_bytes, false, out);
}

int poa_batch_create_ex(const poa_graph_t* g, int device, uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff,
                        const poa_config_t* cfg, uint64_t workspace_bytes, poa_batch_t** out) {
    if (cfg && cfg->mode > POA_MODE_CHECKPOINT2) return fail(POA_ERR_INVALID_ARG, "poa_batch_create_ex: unknown mode");
    const bool sweep = cfg && cfg->mode == POA_MODE_SCORE;
    if (sweep && cfg->span == POA_SPAN_ENDS_FREE)
        return fail(POA_ERR_UNSUPPORTED, "score-only mode is Global: an ends-free result is defined by the reference's search");
    const bool ckpt2 = cfg && cfg->mode == POA_MODE_CHECKPOINT2;   // the two-piece model's checkpointed batch: its own footprint
    const bool ckpt = ckpt2 || (cfg && cfg->mode == POA_MODE_CHECKPOINT);
    if (ckpt && cfg->span == POA_SPAN_ENDS_FREE)
        return fail(POA_ERR_UNSUPPORTED, "checkpointed mode is Global: an ends-free result is defined by the reference's search");
    uint32_t ckpt_rows = 0;
    if (ckpt) { const TuneView T(cfg); if (const int* v = T.ptr(POA_TUNE_CKPT_ROWS)) ckpt_rows = (*v) > 0 ? (uint32_t)(*v) : 0u; }
    return batch_create_impl(g, device, n_queries, qseq, qoff, workspace_bytes, sweep, out, ckpt, ckpt_rows, ckpt2);
}

int poa_batch_workspace_bytes(poa_batch_t* b, uint64_t* bytes) {
    if (!b || !bytes) return fail(POA_ERR_INVALID_ARG, "poa_batch_workspace_bytes: null argument");
    *bytes = b->d_planes.bytes;
    return POA_OK;
}

// the constructor behind the null check of `out` (batch_create_impl below: CreateFrame::guarded)
static int batch_create_body(const poa_graph_t* g, int device, uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff,
                             uint64_t workspace_bytes, bool sweep, poa_batch_t** out, bool ckpt, uint32_t ckpt_rows, bool ckpt2) {
    if (!g || !qoff || (n_queries && qoff[n_queries] && !qseq))
        return fail(POA_ERR_INVALID_ARG, "poa_batch_create: null argument");
    for (uint32_t i = 0; i < n_queries; ++i) {
        if (qoff[i + 1] < qoff[i]) return fail(POA_ERR_INVALID_ARG, "poa_batch_create: qoff not monotone");
        if (qoff[i + 1] - qoff[i] > 0x7FFFFFF0ull) return fail(POA_ERR_UNSUPPORTED, "query longer than 2^31");
    }
    CreateFrame frame{"poa_batch_create"};
    if (const int rc = frame.open(device)) return rc;

    std::unique_ptr<poa_batch> b(new (std::nothrow) poa_batch);
    if (!b) return fail(POA_ERR_OUT_OF_MEMORY, "host allocation failed");
    const FlatGraph& fg = g->g;
    b->graph = g; b->device = device; b->n_queries = n_queries;
    const uint32_t rows = fg.n;
    b->sweep = sweep;
    b->sweep_slots = std::max<uint32_t>(g->sweep.n_slots, 1u);
    b->sweep_slotted = g->sweep.n_slotted;
    b->ckpt = ckpt;
    b->ckpt2 = ckpt2;
    b->ckpt_slots = g->sweep.n_slots;
    if (ckpt) {
        const CheckpointPlan& own = ckpt2 ? g->ckpt2 : g->ckpt;
        if (ckpt_rows == 0 || ckpt_rows == own.segment_rows) b->ckpt_plan = own;
        else build_checkpoint_plan(fg, g->sweep, ckpt_rows, b->ckpt_plan, ckpt2);
    }
    b->h_qoff.assign(qoff, qoff + n_queries + 1);
    b->h_pitch.resize(n_queries);
    b->h_scratch_off.resize((size_t)n_queries + 1);

    uint64_t scratch_total = 0, max_len = 0, biggest = 0;
    std::vector<uint64_t> q_plane_elems(n_queries);
    for (uint32_t i = 0; i < n_queries; ++i) {
        const uint64_t L = qoff[i + 1] - qoff[i];
        max_len = std::max(max_len, L);
        const uint32_t pitch = (uint32_t)(((L + 1 + 63) / 64) * 64);
        b->h_pitch[i] = pitch;
        // score-only: n_sweep_slots rows of M and of D (4-byte cells: what the widest layout needs; u16 runs use half of it)
        // checkpointed: slots + snapshots + one segment window (CheckpointPlan::rows_per_query rows), sized for 4-byte cells too
        q_plane_elems[i] = sweep ? 2ull * b->sweep_slots * pitch : (ckpt ? (uint64_t)b->ckpt_plan.rows_per_query * pitch : 3ull * rows * pitch);
        b->h_scratch_off[i] = scratch_total;
        if (!sweep) scratch_total += L + rows;   // (no pairs, no traceback scratch)
        b->max_len = std::max<uint64_t>(b->max_len, L);
        b->total_bases += L;
        b->total_cells += (uint64_t)rows * (L + 1);
        b->plane_bytes_total += q_plane_elems[i] * 4;
        biggest = std::max(biggest, q_plane_elems[i] * 4);
    }
    b->h_scratch_off[n_queries] = scratch_total;

    // workspace: as many queries' planes as fit; chunks reuse it.
    // score-only: the carries between strips (two parities x two words per row and query in flight, poa_forward_sweep.hpp) exist
    // only when some query is longer than one 1024-column strip; they are part of what the batch holds besides the slots
    // (the two-piece checkpointed passes carry three words per row and parity: poa_checkpoint2.hpp)
    const bool sweep_carry = (sweep || ckpt) && max_len + 1 > 1024;
    const uint64_t carry_words = ckpt2 ? 6 : 4;
    const uint64_t fixed = scratch_total * 16 + (uint64_t)n_queries * 64 + qoff[n_queries] + (64ull << 20) +
                           (sweep_carry ? 4ull * carry_words * n_queries * rows : 0);
    // (a score-only or checkpointed batch holds its own footprint, never more: workspace_bytes is a cap)
    uint64_t ws = 0;
    if (const int rc = frame.workspace(workspace_bytes, fixed, b->plane_bytes_total, biggest, sweep || ckpt,
                                       "score planes of the largest query do not fit in device memory", ws)) return rc;
    // chunking, once per layout (build_chunk_plan)
    auto make_plan = [&](poa_batch::Plan& pl, uint64_t elem_bytes, bool compact_size) {
        build_chunk_plan(pl, n_queries, ws, elem_bytes, [&](uint32_t i) {
            return compact_size ? compact_plane_elems(rows, b->h_pitch[i], fg.n_store_d) : q_plane_elems[i];
        });
    };
    b->plan_ws = ws;
    make_plan(b->plan[0], 4, false);
    b->plan16_same = sweep || b->plan[0].chunks.size() <= 1;
    // (a checkpointed batch has no compact layout: its u16 runs take plan[1], and plan[2] is a copy of it)
    if (!b->plan16_same) { make_plan(b->plan[1], 2, false); make_plan(b->plan[2], 2, !ckpt); }
    const uint32_t max_chunk_any = std::max(b->plan[0].max_chunk, std::max(b->plan[1].max_chunk, b->plan[2].max_chunk));
    b->cols_per_lane = 16;

    // device buffers
    HIP_TRY(b->d_rows.alloc(fg.rows.size()));
    HIP_TRY(b->d_pred_rows.alloc(std::max<size_t>(fg.pred_rows.size(), 1)));
    HIP_TRY(b->d_pred_k.alloc(std::max<size_t>(fg.pred_k.size(), 1)));
    HIP_TRY(b->d_row_depth.alloc(std::max<size_t>(fg.row_depth.size(), 1)));
    const bool sweep_tables = sweep || ckpt;
    HIP_TRY(b->d_dslot.alloc(std::max<size_t>(sweep_tables ? g->sweep.slot.size() : fg.d_slot.size(), 1)));
    HIP_TRY(b->d_pred_dslot.alloc(std::max<size_t>(sweep_tables ? g->sweep.pred_slot.size() : fg.pred_dslot.size(), 1)));
    if (ckpt) {
        const CheckpointPlan& cp = b->ckpt_plan;
        HIP_TRY(b->d_ck_snap_off.alloc(cp.snap_off.size()));
        HIP_TRY(b->d_ck_snap_dst.alloc(std::max<size_t>(cp.snap_dst.size(), 1)));
        HIP_TRY(b->d_ck_pred_src.alloc(std::max<size_t>(cp.pred_src.size(), 1)));
        HIP_TRY(b->d_ck_boundary.alloc(cp.boundary.size()));
        HIP_TRY(hipMemcpy(b->d_ck_snap_off.p, cp.snap_off.data(), cp.snap_off.size() * 4, hipMemcpyHostToDevice));
        if (!cp.snap_dst.empty()) HIP_TRY(hipMemcpy(b->d_ck_snap_dst.p, cp.snap_dst.data(), cp.snap_dst.size() * 4, hipMemcpyHostToDevice));
        if (!cp.pred_src.empty()) HIP_TRY(hipMemcpy(b->d_ck_pred_src.p, cp.pred_src.data(), cp.pred_src.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b->d_ck_boundary.p, cp.boundary.data(), cp.boundary.size() * 4, hipMemcpyHostToDevice));
    }
    if (const int rc = frame.alloc_results(b.get(), qoff[n_queries], n_queries, n_queries, true, scratch_total)) return rc;
    if (!b->plan16_same) HIP_TRY(CreateFrame::alloc_each(n_queries, b->plan[1].d_off, b->plan[2].d_off));
    HIP_TRY(CreateFrame::alloc_each((sweep_tables ? (sweep_carry ? carry_words : 0ull) : 2ull) * max_chunk_any * rows, b->d_carry));
    if (const int rc = frame.acquire_planes(b.get(), ws + 256, sweep_tables, "score-plane workspace")) return rc;

    if (const int rc = frame.begin_upload()) return rc;
    HIP_TRY(CreateFrame::upload(b->d_rows, fg.rows));
    HIP_TRY(CreateFrame::upload(b->d_pred_rows, fg.pred_rows));
    HIP_TRY(CreateFrame::upload(b->d_pred_k, fg.pred_k));
    HIP_TRY(CreateFrame::upload(b->d_row_depth, fg.row_depth));
    HIP_TRY(CreateFrame::upload(b->d_dslot, sweep_tables ? g->sweep.slot : fg.d_slot));
    HIP_TRY(CreateFrame::upload(b->d_pred_dslot, sweep_tables ? g->sweep.pred_slot : fg.pred_dslot));
    if (sweep) HIP_TRY(hipMemset(b->d_pair_off.p, 0, ((size_t)n_queries + 1) * 8));
    if (const int rc = frame.upload_queries(b.get(), qseq, qoff, n_queries, b->h_scratch_off.data(), b->h_pitch.data(), b->plan[0].off.data(), n_queries)) return rc;
    if (!b->plan16_same) for (int k = 1; k < 3; ++k) HIP_TRY(CreateFrame::upload(b->plan[k].d_off, b->plan[k].off));
    if (const int rc = frame.end_upload(b.get())) return rc;

    *out = b.release();
    return POA_OK;
}

static int batch_create_impl(const poa_graph_t* g, int device, uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff,
                             uint64_t workspace_bytes, bool sweep, poa_batch_t** out, bool ckpt, uint32_t ckpt_rows, bool ckpt2) {
    return CreateFrame::enter("poa_batch_create", out, "host allocation failed", [&] {
        return batch_create_body(g, device, n_queries, qseq, qoff, workspace_bytes, sweep, out, ckpt, ckpt_rows, ckpt2);
    });
}

// The replay's view of the graph (the bubble index is built by now) and the per-query result buffers of a search, uploaded once
// per batch: what the one-piece replay (prepare_exact) and the two-piece one (prepare_replay2) share.
static int prepare_exact_tables(poa_batch* b) {
    if (b->ex_tables_ready) return POA_OK;
    const FlatGraph& fg = b->graph->g;
    const uint32_t n = fg.n;
    HIP_TRY(b->d_succ_off.alloc(fg.succ_row_off.size()));
    HIP_TRY(b->d_succ_rows.alloc(std::max<size_t>(fg.succ_rows.size(), 1)));
    HIP_TRY(b->d_dist_min.alloc(n)); HIP_TRY(b->d_dist_max.alloc(n)); HIP_TRY(b->d_exit_idx.alloc(n));
    HIP_TRY(b->d_node_row.alloc(n)); HIP_TRY(b->d_sp_to_end.alloc(n));
    HIP_TRY(b->d_ex_end.alloc(2 * (size_t)std::max<uint32_t>(b->n_queries, 1)));
    HIP_TRY(hipMemcpy(b->d_node_row.p, fg.node_row.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_sp_to_end.p, fg.sp_to_end.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(b->d_ex_sym.alloc((size_t)n + 4));
    {
        std::vector<uint8_t> row_sym((size_t)n + 4, 0);
        for (uint32_t r = 0; r < n; ++r) row_sym[r] = fg.rows[r].sym;
        HIP_TRY(hipMemcpy(b->d_ex_sym.p, row_sym.data(), row_sym.size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(b->d_nbm_off.alloc(n + 1)); HIP_TRY(b->d_nbm.alloc(std::max<size_t>(fg.nbm.size(), 1)));
    if (!fg.row_rec.empty()) {
        HIP_TRY(b->d_ex_rec.alloc(fg.row_rec.size()));
        HIP_TRY(hipMemcpy(b->d_ex_rec.p, fg.row_rec.data(), fg.row_rec.size() * sizeof(FlatGraph::RowRec), hipMemcpyHostToDevice));
    }
    HIP_TRY(b->d_ex_status.alloc(std::max<uint32_t>(b->n_queries, 1)));
    HIP_TRY(b->d_ex_counters.alloc(4 * (size_t)std::max<uint32_t>(b->n_queries, 1)));
    HIP_TRY(b->d_ex_prof.alloc(8 * (size_t)std::max<uint32_t>(b->n_queries, 1)));   // (diagnostics; once, not per chunk while a kernel may write it)
    HIP_TRY(hipMemcpy(b->d_succ_off.p, fg.succ_row_off.data(), fg.succ_row_off.size() * 4, hipMemcpyHostToDevice));
    if (!fg.succ_rows.empty()) HIP_TRY(hipMemcpy(b->d_succ_rows.p, fg.succ_rows.data(), fg.succ_rows.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_dist_min.p, fg.dist_min.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_dist_max.p, fg.dist_max.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_exit_idx.p, fg.exit_idx.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_nbm_off.p, fg.nbm_off.data(), (n + 1) * 4, hipMemcpyHostToDevice));
    if (!fg.nbm.empty()) HIP_TRY(hipMemcpy(b->d_nbm.p, fg.nbm.data(), fg.nbm.size() * sizeof(FlatGraph::NodeBubble), hipMemcpyHostToDevice));
    b->ex_tables_ready = true;
    return POA_OK;
}

static int prepare_exact(poa_batch* b, const poa_costs_t* costs, const poa_config_t* cfg) {
    const FlatGraph& fg = b->graph->g;
    std::string err;
    int rc;
    {
        std::lock_guard<std::mutex> lk(const_cast<poa_graph*>(b->graph)->bubble_mu);
        rc = build_bubble_index(const_cast<FlatGraph&>(fg), err);
    }
    if (rc != POA_OK) return fail(rc, err);
    const uint32_t n = fg.n;
    {
        // spread of the path lengths to the end: bounds how far the min-gap heuristic can grow along a greedy extension
        // (heuristic.rs:70-102), hence the priority range the wave search keeps live at once (its descriptor ring)
        uint32_t skew = 0;
        for (uint32_t r = 0; r < n; ++r) skew = std::max<uint32_t>(skew, fg.dist_max[r] - std::min(fg.dist_min[r], fg.dist_max[r]));
        b->ex_skew = skew;
    }
    const uint32_t maxc = std::max<uint32_t>(costs->mismatch, (uint32_t)costs->gap_open + costs->gap_extend);
    const uint64_t n_prio64 = ((uint64_t)n + b->max_len + 2) * maxc + costs->gap_open + ((uint64_t)n + b->max_len) * costs->gap_extend + 64;
    if (n_prio64 > (1ull << 26)) return fail(POA_ERR_UNSUPPORTED, "exact replay: priority range too large for this graph / query size");
    if (3ull * n * (((uint64_t)b->max_len + 64) & ~63ull) >= (1ull << 32))
        return fail(POA_ERR_UNSUPPORTED, "exact replay: the visited table of one query exceeds 2^32 cells");
    if ((uint64_t)fg.n_exit * ((b->max_len + 64) / 64) >= (1ull << 32))   // (the reached sets are indexed in 32-bit arithmetic)
        return fail(POA_ERR_UNSUPPORTED, "exact replay: reached sets of one query exceed 2^32 words");
    const float f = (cfg && cfg->queue_entries_per_cell > 0.f) ? cfg->queue_entries_per_cell : 0.25f;
    const uint64_t pool64 = std::max<uint64_t>(256, (uint64_t)(f * (double)n * (double)(b->max_len + 1)));
    if (pool64 > 0xFFFFFFF0ull) return fail(POA_ERR_UNSUPPORTED, "exact replay: queue pool too large");
    // wave search: the descriptor ring covers `win` priorities (see the launch), and every live stack holds a chunk of its own
    uint32_t win = 64;
    {
        // exact_replay_win (poa_multi_plan.hpp) holds the rule; a free graph begin adds the spread of the initial priorities
        ExactWinIn wi;
        wi.x = costs->mismatch; wi.o = costs->gap_open; wi.e = costs->gap_extend; wi.skew = b->ex_skew;
        wi.mingap = !cfg || cfg->heuristic == POA_HEURISTIC_MINGAP;
        wi.free_begin = cfg && cfg->span == POA_SPAN_ENDS_FREE && cfg->graph_free_begin.kind == POA_BOUND_UNBOUNDED;
        wi.max_len = b->max_len;
        for (uint32_t r = 0; r < n; ++r) wi.dist_max = std::max<uint32_t>(wi.dist_max, fg.dist_max[r]);
        win = exact_replay_win(wi);
    }
    const uint64_t pool_ws = pool64 + (uint64_t)BQ_CHUNK * (3ull * win + 8);
    if (pool_ws > 0xFFFFFFF0ull) return fail(POA_ERR_UNSUPPORTED, "exact replay: queue pool too large");
    const uint32_t n_prio = (uint32_t)n_prio64, pool_cap = (uint32_t)pool_ws;
    b->ex_win = win;
    const uint32_t stack_cap = (uint32_t)(n + b->max_len + 8), wpn = (uint32_t)((b->max_len + 1 + 63) / 64), swpn = (wpn + 63) / 64;
    if (b->exact_ready && b->ex_n_prio >= n_prio && b->ex_pool_cap >= pool_cap) return POA_OK;
    // the workspace below is re-allocated: released blocks go to the buffer cache, where another batch may pick them up,
    // so nothing of an earlier run on this batch may still be in flight
    if (b->ran) HIP_TRY(hipStreamSynchronize(b->last_stream));
    const uint64_t slots = b->plan[0].max_chunk;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const uint64_t need = slots * ((uint64_t)fg.n_exit * (wpn + swpn) * 8 + 3ull * n_prio * 4 + (uint64_t)stack_cap * 12 + (uint64_t)pool_cap * 16);
    if (need + (256ull << 20) > free_b + b->d_ex_pool.n * 16 + b->d_ex_head.n * 4 + b->d_ex_reached.n * 8)
        return fail(POA_ERR_OUT_OF_MEMORY, "exact replay workspace does not fit: create the batch with a smaller workspace_bytes (fewer queries per chunk) or lower queue_entries_per_cell");
    if (const int trc = prepare_exact_tables(b)) return trc;
    HIP_TRY(b->d_ex_reached.alloc(std::max<uint64_t>(slots * fg.n_exit * wpn, 1)));
    HIP_TRY(b->d_ex_rsum.alloc(std::max<uint64_t>(slots * fg.n_exit * swpn, 1)));
    HIP_TRY(b->d_ex_head.alloc(slots * 3 * n_prio));
    HIP_TRY(b->d_ex_stack.alloc(slots * stack_cap));
    {
        hipError_t e = b->d_ex_pool.alloc(slots * pool_cap);
        if (e != hipSuccess) return fail(POA_ERR_OUT_OF_MEMORY, std::string("exact replay queue pool: ") + hipGetErrorString(e));
    }
    b->ex_n_prio = n_prio; b->ex_pool_cap = pool_cap; b->ex_stack_cap = stack_cap; b->ex_wpn = wpn; b->ex_swpn = swpn;
    b->exact_ready = true;
    return POA_OK;
}

// Score-only run of a batch created for it: one sweep launch per chunk, nothing else.  Costs are 32-bit here: the two-piece
// reduction (poa_align_batch_2piece_ex) opens a gap at open1 + extend1 - extend2, which need not fit poa_costs_t.
static int run_sweep(poa_batch* b, uint32_t cost_x, uint32_t cost_o, uint32_t cost_e, const TuneView& T, hipStream_t stream) {
    HIP_TRY(hipSetDevice(b->device));
    const FlatGraph& fg = b->graph->g;
    RunFrame run;
    if (const int rc = run.open(b, "poa_batch_run: call poa_batch_stats/fetch at least every 256 runs")) return rc;
    const bool narrow = u16_cells_suffice(cost_o, cost_e, b->max_len, fg) && !planes32(T);
    bool want_px = true;
    if (const int* xv = T.ptr(POA_TUNE_PX)) want_px = (*xv) != 0;
    if (const int rc = run.begin(stream, b->plan[0].chunks.size())) return rc;
    b->last_mode = POA_MODE_SCORE;
    b->two_piece = false;
    set_layout(b, narrow);
    b->active_plan = 0;
    const poa_batch::Plan& PL = b->cur();
    if (b->n_queries == 0) return run.end_empty(false);
    b->sweep_bytes_written = 0;
    for (const auto& ch : PL.chunks) {
        SweepParams sp;
        sp.rows = b->d_rows.p; sp.pred_rows = b->d_pred_rows.p; sp.slot = b->d_dslot.p; sp.pred_slot = b->d_pred_dslot.p;
        sp.n_rows = fg.n; sp.n_slots = b->sweep_slots;
        sp.first_query = ch.first; sp.n_queries = ch.count;
        sp.qseq = b->d_qseq.p; sp.qoff = b->d_qoff.p; sp.pitch = b->d_pitch.p; sp.plane_off = PL.d_off.p;
        sp.planes = b->d_planes.p; sp.carry = b->d_carry.p;
        sp.cost_x = cost_x; sp.cost_oe = cost_o + cost_e; sp.cost_e = cost_e;
        sp.score = b->d_score.p; sp.flags = b->d_flags.p;
        uint32_t max_pitch = 0;
        uint64_t pitch_sum = 0;
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) { max_pitch = std::max(max_pitch, b->h_pitch[i]); pitch_sum += b->h_pitch[i]; }
        const uint32_t blocks = (ch.count + 3) / 4;
        // The one-strip packed kernel keeps a slot row in its register layout, 1024 two-byte cells whatever the pitch: it is
        // taken where the chunk is one strip wide and those rows fit what the chunk was given (8 bytes per slot and column).
        const bool px = narrow && want_px && max_pitch > 512 && max_pitch <= 1024 && pitch_sum >= 512ull * ch.count;
        // slot bytes stored: kept rows x 2 planes x (1024 two-byte cells in the packed kernel's register layout, else the pitch)
        b->sweep_bytes_written += 2ull * b->sweep_slotted * (px ? 2048ull * ch.count : pitch_sum * (narrow ? 2 : 4));
        if (px) hipLaunchKernelGGL(poa_sweep_px_kernel, dim3(blocks), dim3(256), 0, stream, sp);
        else launch_by_pitch(narrow, max_pitch, [&](auto cell, auto q) {
            hipLaunchKernelGGL((poa_sweep_kernel<decltype(q)::value, decltype(cell)>), dim3(blocks), dim3(256), 0, stream, sp);
        });
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark(3)) return rc;
    }
    return run.end();
}

// Checkpointed run of a batch created for it: per chunk the sweep with snapshots (pass 1), then recompute-and-walk (pass 2);
// scan and compaction of the pairs as in dense mode.
static int run_ckpt(poa_batch* b, const poa_costs_t* costs, const TuneView& T, hipStream_t stream) {
    HIP_TRY(hipSetDevice(b->device));
    const FlatGraph& fg = b->graph->g;
    const CheckpointPlan& cp = b->ckpt_plan;
    RunFrame run;
    if (const int rc = run.open(b, "poa_batch_run: call poa_batch_stats/fetch at least every 256 runs")) return rc;
    const bool narrow = u16_cells_suffice(costs->gap_open, costs->gap_extend, b->max_len, fg) && !planes32(T);
    const int plan = (narrow && !b->plan16_same) ? 1 : 0;
    if (const int rc = run.begin(stream, b->plan[plan].chunks.size())) return rc;
    b->last_mode = POA_MODE_CHECKPOINT;
    b->two_piece = false;
    set_layout(b, narrow);
    b->active_plan = plan;
    const poa_batch::Plan& PL = b->cur();
    if (b->n_queries == 0) return run.end_empty(true);
    b->sweep_bytes_written = 0;
    for (const auto& ch : PL.chunks) {
        CkptParams kp;
        kp.rows = b->d_rows.p; kp.pred_rows = b->d_pred_rows.p; kp.slot = b->d_dslot.p; kp.pred_slot = b->d_pred_dslot.p;
        kp.snap_off = b->d_ck_snap_off.p; kp.snap_dst = b->d_ck_snap_dst.p; kp.pred_src = b->d_ck_pred_src.p; kp.boundary = b->d_ck_boundary.p;
        kp.n_rows = fg.n; kp.n_slots = b->ckpt_slots; kp.n_snap = cp.n_snap_rows; kp.seg_rows = cp.max_segment; kp.n_segments = cp.n_segments();
        kp.start_row = fg.start_row; kp.end_row = fg.end_row;
        kp.first_query = ch.first; kp.n_queries = ch.count;
        kp.qseq = b->d_qseq.p; kp.qoff = b->d_qoff.p; kp.pitch = b->d_pitch.p; kp.plane_off = PL.d_off.p;
        kp.planes = b->d_planes.p; kp.carry = b->d_carry.p;
        kp.cost_x = costs->mismatch; kp.cost_o = costs->gap_open; kp.cost_e = costs->gap_extend;
        kp.scratch_off = b->d_scratch_off.p; kp.scratch = b->d_scratch.p;
        kp.score = b->d_score.p; kp.flags = b->d_flags.p; kp.n_pairs = b->d_npairs.p;
        uint32_t max_pitch = 0;
        uint64_t pitch_sum = 0;
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) { max_pitch = std::max(max_pitch, b->h_pitch[i]); pitch_sum += b->h_pitch[i]; }
        // cells stored: pass 1 its slotted rows and the snapshots (M, D), pass 2 every row once (M, I, D) when the walk enters
        // every segment, which a Global alignment does unless an edge skips one
        b->sweep_bytes_written += (2ull * (b->sweep_slotted + cp.n_snap_rows) + 3ull * fg.n) * pitch_sum * (narrow ? 2 : 4);
        const dim3 grid((ch.count + 3) / 4), block(256);
        launch_by_pitch(narrow, max_pitch, [&](auto cell, auto q) {
            hipLaunchKernelGGL((poa_ckpt_sweep_kernel<decltype(q)::value, decltype(cell)>), grid, block, 0, stream, kp);
        });
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        launch_by_pitch(narrow, max_pitch, [&](auto cell, auto q) {
            hipLaunchKernelGGL((poa_ckpt_trace_kernel<decltype(q)::value, decltype(cell)>), grid, block, 0, stream, kp);
        });
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark(2)) return rc;
    }
    return run.end_pairs();
}

int poa_batch_run(poa_batch_t* b, const poa_costs_t* costs, void* stream_v) { return poa_batch_run_ex(b, costs, nullptr, stream_v); }

int poa_batch_run_ex(poa_batch_t* b, const poa_costs_t* costs, const poa_config_t* cfg, void* stream_v) {
    if (!b || !costs) return fail(POA_ERR_INVALID_ARG, "poa_batch_run: null argument");
    const TuneView T(cfg);   // what this call overrides, read once
    uint32_t mode = cfg ? cfg->mode : POA_MODE_DENSE;
    if (mode == POA_MODE_CHECKPOINT2) {
        if (b->ckpt2) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: a POA_MODE_CHECKPOINT2 batch runs through poa_batch_run_2piece only");
        return fail(POA_ERR_UNSUPPORTED, "POA_MODE_CHECKPOINT2 is the two-piece model's checkpointed mode: poa_batch_run_2piece / poa_align_batch_2piece_ex");
    }
    if (mode > POA_MODE_CHECKPOINT2) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: unknown mode");
    if (b->ckpt2) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: the batch was created for POA_MODE_CHECKPOINT2 (it runs in that mode through poa_batch_run_2piece only)");
    if (cfg && cfg->span > POA_SPAN_ENDS_FREE) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: unknown alignment span");
    const bool ends_free = cfg && cfg->span == POA_SPAN_ENDS_FREE;
    if (mode == POA_MODE_SCORE) {
        if (ends_free) return fail(POA_ERR_UNSUPPORTED, "score-only mode is Global: an ends-free result is defined by the reference's search");
        if (!b->sweep) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: POA_MODE_SCORE needs a batch created by poa_batch_create_ex with that mode");   // (a checkpointed batch included)
        return run_sweep(b, costs->mismatch, costs->gap_open, costs->gap_extend, T, (hipStream_t)stream_v);
    }
    if (mode == POA_MODE_CHECKPOINT) {
        if (ends_free) return fail(POA_ERR_UNSUPPORTED, "checkpointed mode is Global: an ends-free result is defined by the reference's search");
        if (!b->ckpt) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: POA_MODE_CHECKPOINT needs a batch created by poa_batch_create_ex with that mode");
        return run_ckpt(b, costs, T, (hipStream_t)stream_v);
    }
    if (b->sweep) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: the batch was created for POA_MODE_SCORE (it holds no score planes)");
    if (b->ckpt) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: the batch was created for POA_MODE_CHECKPOINT (it holds no full score planes)");
    if (ends_free) {
        if (cfg->qry_free_end.kind > POA_BOUND_EXCLUDED || cfg->graph_free_begin.kind > POA_BOUND_EXCLUDED ||
            cfg->graph_free_end.kind > POA_BOUND_EXCLUDED || cfg->qry_free_begin.kind > POA_BOUND_EXCLUDED)
            return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: unknown bound kind");
        mode = POA_MODE_EXACT;  // an ends-free result is defined by the reference's search: replay it for every query
    }
    if (cfg && cfg->heuristic > POA_HEURISTIC_MINGAP) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_ex: unknown heuristic");
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(b->device));
    const FlatGraph& fg = b->graph->g;
    if (mode != POA_MODE_DENSE && b->n_queries) {
        int rc = prepare_exact(b, costs, cfg);
        if (rc != POA_OK) return rc;
    }
    RunFrame run;
    if (const int rc = run.open(b, "poa_batch_run: call poa_batch_stats/fetch at least every 256 runs")) return rc;
    const DenseRunPlan R = plan_dense_run(costs->gap_open, costs->gap_extend, b->max_len, fg.min_path_nodes, mode,
                                          cfg && (cfg->flags & POA_CFG_FULL_PLANES), b->plan16_same, T);
    if (const int rc = run.begin(stream, b->plan[R.plan].chunks.size())) return rc;
    b->prof_on = T.ptr(POA_TUNE_WS_PROF) != nullptr;
    b->last_mode = mode;
    b->two_piece = false;
    set_layout(b, R.narrow, R.compact, R.relative);
    b->launches.clear();
    b->replays.clear();
    b->band_used = false; b->band_queries = 0; b->band_min_d = 0; b->band_chunks = 0;
    b->pair_paired = 0; b->pair_single = 0;
    b->narrow_ran = 0; b->narrow_how = 0; b->narrow_chunks = 0;
    b->tb_kernel = POA_TB_KERNEL_NONE; b->tb_lanes = 0; b->tb_depth = 0; b->tb_walks = 0;
    b->active_plan = R.plan;
    const poa_batch::Plan& PL = b->cur();
    if (b->n_queries == 0) return run.end_empty(true);
    if (R.want_band && !PL.chunks.empty()) {   // one fallback counter per chunk, cleared per run
        if (b->d_band_count.n < 3 * PL.chunks.size()) HIP_TRY(b->d_band_count.alloc(3 * PL.chunks.size()));
        HIP_TRY(hipMemsetAsync(b->d_band_count.p, 0, 3 * PL.chunks.size() * 4, stream));
    }
    for (size_t ci = 0; ci < PL.chunks.size(); ++ci) {
        const auto& ch = PL.chunks[ci];
        uint32_t max_pitch = 0;
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) max_pitch = std::max(max_pitch, b->h_pitch[i]);
        const DenseChunkPlan C = plan_dense_chunk(R, ch.count, max_pitch, T, compact_plane_elems(fg.n, max_pitch, fg.d_slot.empty() ? fg.n : fg.n_store_d));
        TbParams tp;
        tp.rows = b->d_rows.p; tp.pred_rows = b->d_pred_rows.p; tp.n_rows = fg.n;
        tp.start_row = fg.start_row; tp.end_row = fg.end_row;
        tp.first_query = ch.first; tp.n_queries = ch.count;
        tp.qseq = b->d_qseq.p; tp.qoff = b->d_qoff.p; tp.pitch = b->d_pitch.p; tp.plane_off = PL.d_off.p;
        tp.planes = b->d_planes.p; tp.scratch_off = b->d_scratch_off.p; tp.scratch = b->d_scratch.p;
        tp.score = b->d_score.p; tp.flags = b->d_flags.p; tp.n_pairs = b->d_npairs.p;
        tp.cost_x = costs->mismatch; tp.cost_o = costs->gap_open; tp.cost_e = costs->gap_extend;
        tp.spec_depth = R.spec_depth;
        tp.exact_pass = 0; tp.ex_status = nullptr; tp.ex_end = nullptr; tp.code_fmt = C.v[4];
        tp.row_depth = R.relative ? b->d_row_depth.p : nullptr;
        tp.d_slot = fg.d_slot.empty() ? nullptr : b->d_dslot.p; tp.pred_dslot = fg.d_slot.empty() ? nullptr : b->d_pred_dslot.p;
        FwdParams fp;
        fp.rows = b->d_rows.p; fp.pred_rows = b->d_pred_rows.p; fp.n_rows = fg.n;
        fp.first_query = ch.first; fp.n_queries = ch.count;
        fp.qseq = b->d_qseq.p; fp.qoff = b->d_qoff.p; fp.pitch = b->d_pitch.p; fp.plane_off = PL.d_off.p;
        fp.planes = b->d_planes.p; fp.strip_carry = b->d_carry.p;
        fp.cost_x = costs->mismatch; fp.cost_oe = (uint32_t)costs->gap_open + costs->gap_extend; fp.cost_e = costs->gap_extend;
        // the same recurrences under the depth potential: deletions lose the e the potential already charges per row,
        // insertions pay it twice, every predecessor edge adds e * pred_k
        fp.cost_de = R.relative ? 0u : fp.cost_e;
        fp.cost_doe = R.relative ? (uint32_t)costs->gap_open : fp.cost_oe;
        fp.cost_ie = R.relative ? 2u * fp.cost_e : fp.cost_e;
        fp.cost_ioe = R.relative ? fp.cost_oe + fp.cost_e : fp.cost_oe;
        fp.pred_k = R.relative ? b->d_pred_k.p : nullptr;
        fp.d_slot = fg.d_slot.empty() ? nullptr : b->d_dslot.p; fp.pred_dslot = fg.d_slot.empty() ? nullptr : b->d_pred_dslot.p;
        fp.pipeline_error = b->d_pipeline_error.p;
        if (C.mf >= 0) b->dense_derived_gaps = C.mf == 3;   // the px branch: the gap-state flags are the traceback's to derive
        if (C.band) { if (const int rc = launch_band(b, ci, R, fp, stream)) return rc; }
        else launch_forward(R, C, fp, tp, stream);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;

        if (C.separate_tb) {
            launch_traceback(R, C, tp, stream);
            HIP_TRY(hipGetLastError());
            if (!C.lean_tb) b->tb_kernel = POA_TB_KERNEL_GENERIC;
            else if (b->tb_kernel == POA_TB_KERNEL_NONE) b->tb_kernel = POA_TB_KERNEL_LEAN;
            b->tb_lanes = C.v[5]; b->tb_depth = C.v[6]; b->tb_walks += C.v[7];
        }
        if (mode == POA_MODE_DENSE) b->launches.push_back(C);
        if (const int rc = run.mark()) return rc;

        if (mode != POA_MODE_DENSE) {
            if (const int rc = replay_chunk(b, ch, costs, cfg, T, mode == POA_MODE_HYBRID ? 1u : 0u, ends_free, tp, stream)) return rc;
        }
        if (const int rc = run.mark()) return rc;
    }
    return run.end_pairs();
}

int poa_batch_fetch(poa_batch_t* b, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                    uint32_t* flags, poa_stats_t* stats) {
    if (!b) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch: null batch");
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch: poa_batch_run has not been called");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    {
        int prc = check_pipeline_error(b);
        if (prc != POA_OK) return prc;
    }
    const uint32_t n = b->n_queries;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, nullptr));
    std::vector<uint64_t> off_local;
    uint64_t* off = pair_off;
    if (!off) { off_local.resize((size_t)n + 1); off = off_local.data(); }
    HIP_TRY(hipMemcpy(off, b->d_pair_off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    int rc = POA_OK;
    uint32_t n_exact = 0;
    if (n) {
        if (score) HIP_TRY(hipMemcpy(score, b->d_score.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> fl_local;
        uint32_t* fl = flags;
        if (!fl && stats) { fl_local.resize(n); fl = fl_local.data(); }
        if (fl) HIP_TRY(hipMemcpy(fl, b->d_flags.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (pairs) {
            if (off[n] > pair_capacity) rc = fail(POA_ERR_CAPACITY, "pair_capacity too small; pair_off[n] holds the needed total");
            else if (off[n]) HIP_TRY(hipMemcpy(pairs, b->d_pairs.p, off[n] * sizeof(poa_aln_pair_t), hipMemcpyDeviceToHost));
        }
        if (stats && fl) {
            uint32_t nf = 0;
            for (uint32_t i = 0; i < n; ++i) nf += fl[i] != 0;
            stats->n_flagged = nf;
        }
        if (stats && b->two_piece && b->last_mode != POA_MODE_DENSE) n_exact = n;   // (the two-piece replay searches for every query)
        else if (stats && (b->last_mode == POA_MODE_EXACT || b->last_mode == POA_MODE_HYBRID)) {
            std::vector<uint32_t> stt(n);
            HIP_TRY(hipMemcpy(stt.data(), b->d_ex_status.p, (size_t)n * 4, hipMemcpyDeviceToHost));
            uint32_t ne = 0;
            for (uint32_t i = 0; i < n; ++i) ne += stt[i] == 0;
            n_exact = ne;
        }
    } else if (stats) {
        stats->n_flagged = 0;
    }
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    float ms_d2h = 0.f;
    (void)hipEventElapsedTime(&ms_d2h, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (stats) {
        collect_stats(b, stats);
        stats->ms_d2h = ms_d2h;
        stats->n_exact = n_exact;
    }
    return rc;
}

int poa_batch_stats(poa_batch_t* b, poa_stats_t* stats) {
    if (!b || !stats) return fail(POA_ERR_INVALID_ARG, "poa_batch_stats: null argument");
    HIP_TRY(hipSetDevice(b->device));
    if (b->ran) HIP_TRY(hipStreamSynchronize(b->last_stream));
    std::memset(stats, 0, sizeof(*stats));
    collect_stats(b, stats);
    return b->ran ? check_pipeline_error(b) : POA_OK;
}

int poa_batch_fetch_search_counters(poa_batch_t* b, uint32_t* out) {
    if (!b || !out) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_search_counters: null argument");
    if (!b->ran || b->last_mode == POA_MODE_DENSE || b->last_mode == POA_MODE_SCORE || b->last_mode == POA_MODE_CHECKPOINT || b->last_mode == POA_MODE_CHECKPOINT2 || !b->d_ex_counters.p)
        return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_search_counters: the last run was not an exact / hybrid run");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    if (b->n_queries) HIP_TRY(hipMemcpy(out, b->d_ex_counters.p, (size_t)b->n_queries * 16, hipMemcpyDeviceToHost));
    if (b->prof_on && b->d_ex_prof.p && b->n_queries) {
        std::vector<unsigned long long> pr(8 * (size_t)b->n_queries);
        HIP_TRY(hipMemcpy(pr.data(), b->d_ex_prof.p, pr.size() * 8, hipMemcpyDeviceToHost));
        unsigned long long sum[8] = {0};
        for (size_t i = 0; i < pr.size(); ++i) sum[i & 7] += pr[i];
        // wave search: queue+entries, parallel test, drop, fast expand, generic, (counts: fast, generic); parallel-step search: queue+entries,
        // log-mode phase, conflict test, commit, sequential code, pushes, (counts: sequential steps, lanes committed)
        fprintf(stderr, "[ws prof] cycles / counts: %llu %llu %llu %llu %llu %llu %llu %llu\n", sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6], sum[7]);
    }
    return POA_OK;
}

int poa_batch_device_results(poa_batch_t* b, void** score, void** flags, void** pair_off, void** pairs) {
    if (!b) return fail(POA_ERR_INVALID_ARG, "poa_batch_device_results: null batch");
    // the results of the last run: wait for it and report a multi-wave pipeline that gave up (as poa_batch_fetch / _stats do), so
    // that a caller gathering straight from HBM (poasta_amd/dist.py) never ships the output of a failed run
    if (b->ran) {
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipStreamSynchronize(b->last_stream));
        const int prc = check_pipeline_error(b);
        if (prc != POA_OK) return prc;
    }
    if (score) *score = b->d_score.p;
    if (flags) *flags = b->d_flags.p;
    if (pair_off) *pair_off = b->d_pair_off.p;
    if (pairs) *pairs = b->d_pairs.p;
    return POA_OK;
}

int poa_batch_last_layout(poa_batch_t* b, uint32_t* layout) {
    if (!b || !layout) return fail(POA_ERR_INVALID_ARG, "poa_batch_last_layout: null argument");
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_batch_last_layout: poa_batch_run has not been called");
    *layout = (b->dense_narrow ? POA_LAYOUT_U16 : 0u) | (b->dense_compact ? POA_LAYOUT_COMPACT : 0u) | (b->dense_relative ? POA_LAYOUT_RELATIVE : 0u) |
              (b->dense_derived_gaps ? POA_LAYOUT_DERIVED_GAPS : 0u);
    return POA_OK;
}

int poa_batch_last_launch(poa_batch_t* b, uint32_t chunk, uint32_t out[8]) {
    if (!b || !out) return fail(POA_ERR_INVALID_ARG, "poa_batch_last_launch: null argument");
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_batch_last_launch: poa_batch_run has not been called");
    if (b->two_piece || b->sweep || b->ckpt || b->last_mode != POA_MODE_DENSE)
        return fail(POA_ERR_UNSUPPORTED, "poa_batch_last_launch: the last run was not a dense one-piece run");
    if (chunk >= b->launches.size()) return fail(POA_ERR_INVALID_ARG, "poa_batch_last_launch: the last run had no such chunk");
    for (int k = 0; k < 8; ++k) out[k] = b->launches[chunk].v[k];
    return POA_OK;
}

int poa_batch_replay_info(poa_batch_t* b, uint32_t chunk, uint32_t out[8]) {
    if (!b || !out) return fail(POA_ERR_INVALID_ARG, "poa_batch_replay_info: null argument");
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_batch_replay_info: poa_batch_run has not been called");
    if (b->two_piece || b->sweep || b->ckpt || (b->last_mode != POA_MODE_EXACT && b->last_mode != POA_MODE_HYBRID))
        return fail(POA_ERR_UNSUPPORTED, "poa_batch_replay_info: the last run replayed nothing (its mode was neither exact nor hybrid, and its span not ends-free)");
    if (chunk >= b->replays.size()) return fail(POA_ERR_INVALID_ARG, "poa_batch_replay_info: the last run had no such chunk");
    for (int k = 0; k < 8; ++k) out[k] = b->replays[chunk].v[k];
    return POA_OK;
}

int poa_batch_band_info(poa_batch_t* b, uint32_t out[4]) {
    if (!b || !out) return fail(POA_ERR_INVALID_ARG, "poa_batch_band_info: null argument");
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_batch_band_info: poa_batch_run has not been called");
    out[0] = b->band_used ? 1u : 0u; out[1] = 0; out[2] = 0; out[3] = b->band_used ? b->band_min_d : 0u;
    if (!b->band_used) return POA_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    std::vector<uint32_t> counts(b->band_chunks);
    HIP_TRY(hipMemcpy(counts.data(), b->d_band_count.p, counts.size() * 4, hipMemcpyDeviceToHost));
    uint32_t fell = 0;
    for (uint32_t c : counts) fell += c;
    out[2] = fell; out[1] = b->band_queries - std::min(fell, b->band_queries);
    return POA_OK;
}

int poa_batch_band_narrow_info(poa_batch_t* b, uint32_t out[4]) {
    if (!b || !out) return fail(POA_ERR_INVALID_ARG, "poa_batch_band_narrow_info: null argument");
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_batch_band_narrow_info: poa_batch_run has not been called");
    out[0] = b->narrow_ran; out[1] = 0; out[2] = 0; out[3] = b->narrow_how;
    if (!b->narrow_ran) return POA_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    const size_t n_chunks = b->cur().chunks.size();
    std::vector<uint32_t> counts(3 * n_chunks);
    HIP_TRY(hipMemcpy(counts.data(), b->d_band_count.p, counts.size() * 4, hipMemcpyDeviceToHost));
    uint32_t missed = 0, missed_both = 0;
    for (size_t c = 0; c < n_chunks; ++c) { missed += counts[n_chunks + c]; missed_both += counts[2 * n_chunks + c]; }
    out[1] = b->narrow_ran - std::min(missed, b->narrow_ran); out[2] = missed - std::min(missed_both, missed);
    return POA_OK;
}

int poa_batch_tb_info(poa_batch_t* b, uint32_t out[4]) {
    if (!b || !out) return fail(POA_ERR_INVALID_ARG, "poa_batch_tb_info: null argument");
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_batch_tb_info: poa_batch_run has not been called");
    const bool dense_family = !(b->two_piece || b->sweep || b->ckpt);
    out[0] = dense_family ? b->tb_kernel : (uint32_t)POA_TB_KERNEL_NONE;
    out[1] = dense_family ? b->tb_lanes : 0u; out[2] = dense_family ? b->tb_depth : 0u; out[3] = dense_family ? b->tb_walks : 0u;
    return POA_OK;
}

int poa_batch_band_pair_info(poa_batch_t* b, uint32_t out[4]) {
    if (!b || !out) return fail(POA_ERR_INVALID_ARG, "poa_batch_band_pair_info: null argument");
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_batch_band_pair_info: poa_batch_run has not been called");
    out[0] = b->pair_paired; out[1] = b->pair_single; out[2] = BAND_PAIR_MIN_QUERIES; out[3] = b->pair_paired ? 1u : 0u;
    return POA_OK;
}

int poa_batch_fetch_planes(poa_batch_t* b, uint32_t query, uint32_t* m, uint32_t* i, uint32_t* d) {
    if (!b || !m || !i || !d) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_planes: null argument");
    if (!b->ran || query >= b->n_queries) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_planes: bad query / not run");
    if (b->compact) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_planes: the last run used the compact layout; run with POA_CFG_FULL_PLANES");
    if (b->sweep) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_planes: a score-only batch keeps no score planes");
    if (b->ckpt) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_planes: a checkpointed batch keeps snapshots and one segment window, no score planes");
    if (b->last_mode != POA_MODE_DENSE) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_planes: after an exact / hybrid run the workspace holds the replayed search's tiled table");
    if (b->two_piece) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_planes: the last run was a two-piece run; its five planes come from poa_batch_fetch_planes_2piece");
    const auto& last = b->cur().chunks.back();
    if (query < last.first || query >= last.first + last.count)
        return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_planes: the query's planes were overwritten by a later chunk");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    const uint32_t rows = b->graph->g.n, pitch = b->h_pitch[query];
    const uint32_t cols = (uint32_t)(b->h_qoff[query + 1] - b->h_qoff[query]) + 1;
    const uint64_t RP = (uint64_t)rows * pitch;
    uint32_t* dst[3] = {m, i, d};
    if (!b->narrow) {
        for (int k = 0; k < 3; ++k) {
            const uint32_t* src = b->d_planes.p + b->cur().off[query] + k * RP;
            HIP_TRY(hipMemcpy2D(dst[k], (size_t)cols * 4, src, (size_t)pitch * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToHost));
        }
    } else {
        std::vector<uint16_t> tmp((size_t)rows * cols);
        const uint16_t* base = reinterpret_cast<const uint16_t*>(b->d_planes.p) + b->cur().off[query];
        for (int k = 0; k < 3; ++k) {
            HIP_TRY(hipMemcpy2D(tmp.data(), (size_t)cols * 2, base + k * RP, (size_t)pitch * 2, (size_t)cols * 2, rows, hipMemcpyDeviceToHost));
            for (size_t t = 0; t < tmp.size(); ++t) dst[k][t] = tmp[t] == 0xFFFFu ? 0xFFFFFFFFu : tmp[t];
        }
    }
    return POA_OK;
}

int poa_batch_fetch_compact(poa_batch_t* b, uint32_t query, uint16_t* m_raw, uint16_t* d, uint8_t* d_kept) {
    if (!b || !m_raw || !d || !d_kept) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_compact: null argument");
    if (!b->ran || query >= b->n_queries) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_compact: bad query / not run");
    if (b->sweep) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_compact: a score-only batch keeps no score planes");
    if (b->ckpt || b->ckpt2) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_compact: a checkpointed batch keeps snapshots and one segment window, no score planes");
    if (b->last_mode != POA_MODE_DENSE) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_compact: after an exact / hybrid run the workspace holds the replayed search's tiled table");
    if (b->two_piece) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_compact: the last run was a two-piece run; its five planes come from poa_batch_fetch_planes_2piece");
    if (!b->compact || !b->dense_derived_gaps || b->dense_relative)
        return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_compact: the last run did not store the compact derived-gaps layout (poa_batch_last_layout)");
    const auto& last = b->cur().chunks.back();
    if (query < last.first || query >= last.first + last.count)
        return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_compact: the query's planes were overwritten by a later chunk");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    const FlatGraph& fg = b->graph->g;
    const uint32_t rows = fg.n, pitch = b->h_pitch[query];
    const uint32_t cols = (uint32_t)(b->h_qoff[query + 1] - b->h_qoff[query]) + 1;
    const uint64_t RP = (uint64_t)rows * pitch;
    const uint16_t* Mp = reinterpret_cast<const uint16_t*>(b->d_planes.p) + b->cur().off[query];
    const uint16_t* Dp = Mp + RP + RP / 4;   // the kept D rows, row r at slot d_slot[r] (compact_plane_elems)
    HIP_TRY(hipMemcpy2D(m_raw, (size_t)cols * 2, Mp, (size_t)pitch * 2, (size_t)cols * 2, rows, hipMemcpyDeviceToHost));
    const uint32_t n_slots = fg.d_slot.empty() ? rows : fg.n_store_d;
    std::vector<uint16_t> kept((size_t)n_slots * cols);
    if (n_slots) HIP_TRY(hipMemcpy2D(kept.data(), (size_t)cols * 2, Dp, (size_t)pitch * 2, (size_t)cols * 2, n_slots, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t slot = fg.d_slot.empty() ? r : fg.d_slot[r];
        d_kept[r] = (fg.rows[r].flags & ROW_STORE_D) && slot < n_slots ? 1 : 0;
        if (d_kept[r]) std::copy(kept.begin() + (size_t)slot * cols, kept.begin() + (size_t)(slot + 1) * cols, d + (size_t)r * cols);
        else std::fill(d + (size_t)r * cols, d + (size_t)(r + 1) * cols, (uint16_t)0xFFFFu);
    }
    return POA_OK;
}

// ---- two-piece model on a resident batch (kernels: poa_twopiece.hpp) ---------------------------------------------------------------
// The u32 plan of the two-piece pass, cut on the first u32 run: five planes of 4-byte cells per query.  The batch's workspace
// was sized for three; it is replaced by a larger one only if the longest query's five planes do not fit it.
// max_count: queries per chunk at most; the two-piece replay alone passes one (build_chunk_plan).
static int prepare_two_piece_u32(poa_batch* b, uint32_t max_count = ~0u) {
    const uint32_t rows = b->graph->g.n, n = b->n_queries;
    uint64_t biggest = 0;
    for (uint32_t i = 0; i < n; ++i) biggest = std::max<uint64_t>(biggest, 5ull * rows * b->h_pitch[i] * 4);
    const uint64_t ws = std::max(b->plan_ws, biggest);
    if (b->d_planes.bytes < ws + 256) {
        if (b->ran) HIP_TRY(hipStreamSynchronize(b->last_stream));   // (an earlier run may still read the workspace given up here)
        const size_t held = b->d_planes.bytes;
        std::string werr;
        if (!b->d_planes.acquire(b->device, ws + 256, werr)) {
            std::string again;
            (void)b->d_planes.acquire(b->device, held, again);
            return fail(POA_ERR_OUT_OF_MEMORY, "two-piece u32 planes of the largest query: " + werr);
        }
    }
    poa_batch::Plan& pl = b->plan[3];
    try {
        build_chunk_plan(pl, n, ws, 4, [&](uint32_t i) { return 5ull * rows * b->h_pitch[i]; }, max_count);
    } catch (const std::bad_alloc&) { pl.chunks.clear(); return fail(POA_ERR_OUT_OF_MEMORY, "host allocation failed"); }
    if (pl.d_off.alloc(n) != hipSuccess) { pl.chunks.clear(); return fail(POA_ERR_OUT_OF_MEMORY, "two-piece u32 plan: device allocation failed"); }
    if (hipMemcpy(pl.d_off.p, pl.off.data(), (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) { pl.chunks.clear(); return fail(POA_ERR_HIP, "two-piece u32 plan: upload failed"); }
    return POA_OK;
}

// Checkpointed run of a two-piece batch created for it (POA_MODE_CHECKPOINT2): per chunk the two-piece sweep with snapshots
// (pass 1), then recompute-and-walk over five window planes (pass 2); scan and compaction of the pairs as in dense mode.
static int run_ckpt2(poa_batch* b, const poa_costs2_t* costs, hipStream_t stream) {
    HIP_TRY(hipSetDevice(b->device));
    const FlatGraph& fg = b->graph->g;
    const CheckpointPlan& cp = b->ckpt_plan;
    RunFrame run;
    if (const int rc = run.open(b, "poa_batch_run: call poa_batch_stats/fetch at least every 256 runs")) return rc;
    if (b->n_queries && cp.n_segments() == 0) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_2piece: the graph has no rows");
    // cell width: the first piece's costs bound the optimum; wide_planes forces u32
    const bool narrow = u16_cells_suffice(costs->gap_open1, costs->gap_extend1, b->max_len, fg) && !costs->wide_planes;
    const int plan = (narrow && !b->plan16_same) ? 1 : 0;   // the batch is sized for u32: a u16 run packs twice the queries per chunk
    if (const int rc = run.begin(stream, b->plan[plan].chunks.size())) return rc;
    b->last_mode = POA_MODE_CHECKPOINT2;
    b->two_piece = false;   // (no full planes to fetch)
    set_layout(b, narrow);
    b->active_plan = plan;
    const poa_batch::Plan& PL = b->cur();
    if (b->n_queries == 0) return run.end_empty(true);
    b->sweep_bytes_written = 0;
    Ckpt2Params kp;
    kp.rows = b->d_rows.p; kp.pred_rows = b->d_pred_rows.p; kp.slot = b->d_dslot.p; kp.pred_slot = b->d_pred_dslot.p;
    kp.snap_off = b->d_ck_snap_off.p; kp.snap_dst = b->d_ck_snap_dst.p; kp.pred_src = b->d_ck_pred_src.p; kp.boundary = b->d_ck_boundary.p;
    kp.n_rows = fg.n; kp.n_slots = b->ckpt_slots; kp.n_snap = cp.n_snap_rows; kp.seg_rows = cp.max_segment; kp.n_segments = cp.n_segments();
    kp.start_row = fg.start_row; kp.end_row = fg.end_row;
    kp.qseq = b->d_qseq.p; kp.qoff = b->d_qoff.p; kp.pitch = b->d_pitch.p; kp.plane_off = PL.d_off.p;
    kp.planes = b->d_planes.p; kp.carry = b->d_carry.p;
    kp.x = costs->mismatch; kp.o1 = costs->gap_open1; kp.e1 = costs->gap_extend1; kp.e2 = costs->gap_extend2;
    kp.oe = (uint32_t)costs->gap_open1 + costs->gap_extend1;
    kp.scratch_off = b->d_scratch_off.p; kp.scratch = reinterpret_cast<poa_aln_pair_t*>(b->d_scratch.p);
    kp.score = b->d_score.p; kp.flags = b->d_flags.p; kp.n_pairs = b->d_npairs.p;
    for (const auto& ch : PL.chunks) {
        kp.first_query = ch.first; kp.n_queries = ch.count;
        uint64_t pitch_sum = 0;
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) pitch_sum += b->h_pitch[i];
        // cells stored: pass 1 its slotted rows and the snapshots (M, D1, D2), pass 2 every row once (five planes) when the walk
        // enters every segment, which a Global alignment does unless an edge skips one
        b->sweep_bytes_written += (3ull * (b->sweep_slotted + cp.n_snap_rows) + 5ull * fg.n) * pitch_sum * (narrow ? 2 : 4);
        // one wave per query; a strip of 1024 columns (u16: two passes of 512, u32: four of 256) keeps the previous row in registers
        if (narrow) hipLaunchKernelGGL((poa2_ckpt_sweep_kernel<uint16_t, 2>), dim3(ch.count), dim3(64), 0, stream, kp);
        else hipLaunchKernelGGL((poa2_ckpt_sweep_kernel<uint32_t, 4>), dim3(ch.count), dim3(64), 0, stream, kp);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        if (narrow) hipLaunchKernelGGL((poa2_ckpt_trace_kernel<uint16_t, 2>), dim3(ch.count), dim3(64), 0, stream, kp);
        else hipLaunchKernelGGL((poa2_ckpt_trace_kernel<uint32_t, 4>), dim3(ch.count), dim3(64), 0, stream, kp);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark(2)) return rc;
    }
    return run.end_pairs();
}

// the parameter block of the two-piece kernels over the batch's active plan: u32 planes, no replay; a run sets what differs
static TwoPieceParams two_piece_params(poa_batch* b, const poa_costs2_t* costs) {
    const FlatGraph& fg = b->graph->g;
    TwoPieceParams P;
    P.rows = b->d_rows.p; P.pred_rows = b->d_pred_rows.p; P.n_rows = fg.n; P.start_row = fg.start_row; P.end_row = fg.end_row;
    P.qseq = b->d_qseq.p; P.qoff = b->d_qoff.p; P.first_query = 0; P.n_queries = 0;
    P.planes = b->d_planes.p; P.q_pitch = b->d_pitch.p; P.plane_off = b->cur().d_off.p; P.off_scale = 1u;
    P.x = costs->mismatch; P.o1 = costs->gap_open1; P.e1 = costs->gap_extend1; P.e2 = costs->gap_extend2;
    P.oe = (uint32_t)costs->gap_open1 + costs->gap_extend1;
    P.score = b->d_score.p; P.flags = b->d_flags.p; P.n_pairs = b->d_npairs.p;
    P.scratch = reinterpret_cast<poa_aln_pair_t*>(b->d_scratch.p); P.scratch_off = b->d_scratch_off.p;
    P.exact_pass = 0; P.ex_status = nullptr; P.ex_end = nullptr;
    return P;
}

// ---- the replay of the reference's two-piece search (mode EXACT / HYBRID of poa_align_batch_2piece_ex) ---------------------------
// What one search holds besides its five u32 planes: prepare_exact's sizes with five stacks per priority; the pool holds the
// entries live at once - popped slots are reused - at cfg->queue_entries_per_cell entries per cell, default 0.5.  The refusals
// need no device.
struct Replay2Sizes {
    uint32_t n_prio, pool_cap, stack_cap, wpn, swpn;
    uint64_t slot_bytes;
};
static int replay2_sizes(const poa_graph_t* g, uint64_t max_len, const poa_costs2_t* costs, const poa_config_t* cfg, Replay2Sizes& z) {
    const FlatGraph& fg = g->g;
    if (5ull * fg.n * ((max_len + 64) & ~63ull) >= (1ull << 32))
        return fail(POA_ERR_UNSUPPORTED, "two-piece replay: the visited table of one query exceeds 2^32 cells");
    std::string err;
    int rc;
    {
        std::lock_guard<std::mutex> lk(const_cast<poa_graph*>(g)->bubble_mu);
        rc = build_bubble_index(const_cast<FlatGraph&>(fg), err);
    }
    if (rc != POA_OK) return fail(rc, err);
    const uint32_t om = std::max<uint32_t>(costs->gap_open1, costs->gap_open2);
    const uint32_t maxc = std::max<uint32_t>(costs->mismatch, om + costs->gap_extend1);
    const uint64_t n_prio64 = ((uint64_t)fg.n + max_len + 2) * maxc + 2ull * (om + ((uint64_t)fg.n + max_len) * costs->gap_extend1) + 64;
    if (n_prio64 > (1ull << 26)) return fail(POA_ERR_UNSUPPORTED, "two-piece replay: priority range too large for this graph / query size");
    const float f = (cfg->queue_entries_per_cell > 0.f) ? cfg->queue_entries_per_cell : 0.5f;
    const uint64_t pool64 = std::max<uint64_t>(1024, (uint64_t)(f * (double)fg.n * (double)(max_len + 1)));
    if (pool64 > 0xFFFFFFF0ull) return fail(POA_ERR_UNSUPPORTED, "two-piece replay: queue pool too large");
    z.n_prio = (uint32_t)n_prio64; z.pool_cap = (uint32_t)pool64; z.stack_cap = (uint32_t)(fg.n + max_len + 8);
    z.wpn = (uint32_t)((max_len + 1 + 63) / 64); z.swpn = (z.wpn + 63) / 64;
    z.slot_bytes = (uint64_t)fg.n_exit * (z.wpn + z.swpn) * 8 + 5ull * z.n_prio * 4 + (uint64_t)z.stack_cap * 12 + (uint64_t)z.pool_cap * 16;
    return POA_OK;
}

// The graph tables, the u32 plan of five planes with at most max_slots queries per chunk, and the search workspace of the
// largest chunk in the batch's replay buffers.
static int prepare_replay2(poa_batch* b, const Replay2Sizes& z, uint32_t max_slots) {
    const FlatGraph& fg = b->graph->g;
    if (const int rc = prepare_exact_tables(b)) return rc;
    if (const int rc = prepare_two_piece_u32(b, max_slots)) return rc;
    const uint64_t slots = b->plan[3].max_chunk;
    HIP_TRY(b->d_ex_reached.alloc(std::max<uint64_t>(slots * fg.n_exit * z.wpn, 1)));
    HIP_TRY(b->d_ex_rsum.alloc(std::max<uint64_t>(slots * fg.n_exit * z.swpn, 1)));
    HIP_TRY(b->d_ex_head.alloc(slots * 5 * z.n_prio));
    HIP_TRY(b->d_ex_stack.alloc(slots * z.stack_cap));
    if (b->d_ex_pool.alloc(slots * z.pool_cap) != hipSuccess) return fail(POA_ERR_OUT_OF_MEMORY, "two-piece replay: queue pool");
    b->ex_n_prio = z.n_prio; b->ex_pool_cap = z.pool_cap; b->ex_stack_cap = z.stack_cap; b->ex_wpn = z.wpn; b->ex_swpn = z.swpn;
    b->exact_ready = false;   // (the shared buffers now have the two-piece sizes)
    return POA_OK;
}

// The replay for EVERY query of a batch created for the dense pass: per chunk the search (poa2_exact_kernel) into tables that
// start unvisited, then the walk from the cell each search stopped at; scan and compaction of the pairs as in dense mode.
// Reached by the one-shot call alone (poa_batch_run_2piece refuses the mode): a fresh batch with queries, which runs once.
static int run_replay2(poa_batch* b, const poa_costs2_t* costs, const poa_config_t* cfg, const TuneView& T, const Replay2Sizes& z,
                       uint32_t max_slots, hipStream_t stream) {
    HIP_TRY(hipSetDevice(b->device));
    const FlatGraph& fg = b->graph->g;
    RunFrame run;
    if (const int rc = run.open(b, "poa_batch_run: call poa_batch_stats/fetch at least every 256 runs")) return rc;
    if (const int rc = prepare_replay2(b, z, max_slots)) return rc;
    if (const int rc = run.begin(stream, b->plan[3].chunks.size())) return rc;
    b->last_mode = cfg->mode;
    b->two_piece = true;
    set_layout(b, false);
    b->active_plan = 3;
    const poa_batch::Plan& PL = b->cur();
    TwoPieceParams P = two_piece_params(b, costs);
    P.exact_pass = 1; P.ex_status = b->d_ex_status.p; P.ex_end = b->d_ex_end.p;
    TwoPieceExact X;
    X.G = ExactGraph{fg.n, fg.start_row, fg.end_row, b->d_ex_sym.p, b->d_succ_off.p, b->d_succ_rows.p, b->d_dist_min.p, b->d_dist_max.p,
                     b->d_exit_idx.p, fg.n_exit, b->d_nbm_off.p, b->d_nbm.p, b->d_node_row.p, b->d_sp_to_end.p, nullptr};
    X.C = ExactCosts{costs->mismatch, costs->gap_open1, costs->gap_extend1, cfg->heuristic, cfg->pruning, 0, 0, 0, 0, 0, 0,
                     costs->gap_open2, costs->gap_extend2};
    if (cfg->span == POA_SPAN_ENDS_FREE) {
        X.C.ends_free = 1;
        X.C.qfe_kind = cfg->qry_free_end.kind; X.C.qfe_val = cfg->qry_free_end.value;
        X.C.gfb_kind = cfg->graph_free_begin.kind;
        X.C.gfe_kind = cfg->graph_free_end.kind; X.C.gfe_val = cfg->graph_free_end.value;
    }
    X.reached = b->d_ex_reached.p; X.rsum = b->d_ex_rsum.p; X.wpn = b->ex_wpn; X.swpn = b->ex_swpn;
    X.head = b->d_ex_head.p; X.n_prio = b->ex_n_prio; X.pool = b->d_ex_pool.p; X.pool_cap = b->ex_pool_cap;
    X.stack = b->d_ex_stack.p; X.stack_cap = b->ex_stack_cap;
    X.status = b->d_ex_status.p; X.end_cell = b->d_ex_end.p; X.counters = b->d_ex_counters.p;
    X.n_succ = (uint32_t)fg.succ_rows.size(); X.n_nbm = (uint32_t)fg.nbm.size();
    for (const auto& ch : PL.chunks) {
        P.first_query = ch.first; P.n_queries = ch.count;
        // the search fills its table from nothing: unvisited planes (a chunk's regions lie back to back from the start of the
        // workspace, build_chunk_plan), empty stacks, empty reached sets
        const uint32_t last = ch.first + ch.count - 1;
        HIP_TRY(hipMemsetAsync(b->d_planes.p, 0xFF, (PL.off[last] + 5ull * fg.n * b->h_pitch[last]) * 4, stream));
        HIP_TRY(hipMemsetAsync(b->d_ex_head.p, 0xFF, (size_t)ch.count * 5 * b->ex_n_prio * 4, stream));
        if (fg.n_exit) {
            HIP_TRY(hipMemsetAsync(b->d_ex_reached.p, 0, (size_t)ch.count * fg.n_exit * b->ex_wpn * 8, stream));
            HIP_TRY(hipMemsetAsync(b->d_ex_rsum.p, 0, (size_t)ch.count * fg.n_exit * b->ex_swpn * 8, stream));
        }
        // active lanes per wave: enough waves to fill the chip first (one divergent search per lane), then more lanes
        uint32_t lanes = (ch.count + 8191) / 8192;
        if (lanes > 64) lanes = 64;
        if (const int* lv = T.ptr(POA_TUNE_EXACT_LANES)) { const int v = (*lv); if (v >= 1 && v <= 64) lanes = (uint32_t)v; }
        X.lanes_per_wave = lanes;
        // graph arrays in LDS when they fit (one copy per block of 16 waves)
        const uint32_t lds_bytes = exact_lds_bytes(fg.n, X.n_succ, X.n_nbm);
        bool lds_graph = lds_bytes <= 150u * 1024u;
        if (const int* gv = T.ptr(POA_TUNE_EXACT_LDS)) lds_graph = lds_graph && (*gv) != 0;
        if (lds_graph && lds_bytes > 48u * 1024u)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(poa2_exact_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        X.lds_graph = lds_graph ? 1u : 0u;
        const uint32_t per_block = lanes * (EXACT2_BLOCK / 64);
        hipLaunchKernelGGL(poa2_exact_kernel, dim3((ch.count + per_block - 1) / per_block), dim3(EXACT2_BLOCK), lds_graph ? lds_bytes : 0, stream, P, X);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        hipLaunchKernelGGL(poa2_traceback_kernel<uint32_t>, dim3((ch.count + 63) / 64), dim3(64), 0, stream, P);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark(2)) return rc;
    }
    return run.end_pairs();
}

int poa_batch_run_2piece(poa_batch_t* b, const poa_costs2_t* costs, const poa_config_t* cfg, void* stream_v) {
    if (!b || !costs) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_2piece: null argument");
    const uint32_t mode = cfg ? cfg->mode : POA_MODE_DENSE;
    if (mode > POA_MODE_CHECKPOINT2) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_2piece: unknown mode");
    if (cfg && cfg->span > POA_SPAN_ENDS_FREE) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_2piece: unknown alignment span");
    // a CHECKPOINT2 batch runs in that mode only, and no other batch runs in it
    if (b->ckpt2 != (mode == POA_MODE_CHECKPOINT2))
        return fail(POA_ERR_INVALID_ARG, b->ckpt2 ? "poa_batch_run_2piece: the batch was created for POA_MODE_CHECKPOINT2 (it holds no full score planes and runs in that mode only)"
                                                  : "poa_batch_run_2piece: POA_MODE_CHECKPOINT2 needs a batch created by poa_batch_create_ex with that mode (a batch created for another mode than the run's)");
    if (mode == POA_MODE_EXACT || mode == POA_MODE_HYBRID)
        return fail(POA_ERR_UNSUPPORTED, "poa_batch_run_2piece: the replay of the reference's two-piece search keeps a workspace of its own (poa_align_batch_2piece_ex)");
    if (mode == POA_MODE_CHECKPOINT) return fail(POA_ERR_UNSUPPORTED, "checkpointed mode: one-piece gap-affine model only");
    if (cfg && cfg->span == POA_SPAN_ENDS_FREE)
        return fail(POA_ERR_UNSUPPORTED, "two-piece model: ends-free alignment needs the exact replay (poa_align_batch_2piece_ex, mode EXACT)");
    if (costs->gap_extend1 < costs->gap_extend2)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    const TuneView T(cfg);
    hipStream_t stream = (hipStream_t)stream_v;
    if (mode == POA_MODE_CHECKPOINT2) return run_ckpt2(b, costs, stream);
    if (mode == POA_MODE_SCORE) {
        if (!b->sweep) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_2piece: POA_MODE_SCORE needs a batch created by poa_batch_create_ex with that mode");
        // the two-piece optimum is the one-piece optimum under open' = open1 + extend1 - extend2, extend' = extend2
        return run_sweep(b, costs->mismatch, (uint32_t)costs->gap_open1 + costs->gap_extend1 - costs->gap_extend2, costs->gap_extend2, T, stream);
    }
    if (b->sweep) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_2piece: the batch was created for POA_MODE_SCORE (it holds no score planes)");
    if (b->ckpt) return fail(POA_ERR_INVALID_ARG, "poa_batch_run_2piece: the batch was created for POA_MODE_CHECKPOINT (it holds no full score planes)");
    HIP_TRY(hipSetDevice(b->device));
    const FlatGraph& fg = b->graph->g;
    RunFrame run;
    if (const int rc = run.open(b, "poa_batch_run: call poa_batch_stats/fetch at least every 256 runs")) return rc;
    // cell width: the first piece's costs bound the optimum; wide_planes forces u32
    const bool narrow = u16_cells_suffice(costs->gap_open1, costs->gap_extend1, b->max_len, fg) && !costs->wide_planes;
    if (!narrow && b->n_queries && b->plan[3].chunks.empty()) {
        const int rc = prepare_two_piece_u32(b);
        if (rc != POA_OK) return rc;
    }
    // u16: five 2-byte planes inside the query's region of the 4-byte plan (2.5 of its 3 x rows x pitch elements)
    const int plan = narrow ? 0 : 3;
    if (const int rc = run.begin(stream, b->plan[plan].chunks.size())) return rc;
    b->last_mode = POA_MODE_DENSE;
    b->two_piece = true;
    set_layout(b, narrow);
    b->active_plan = plan;
    const poa_batch::Plan& PL = b->cur();
    if (b->n_queries == 0) return run.end_empty(true);
    TwoPieceParams P = two_piece_params(b, costs);
    P.off_scale = narrow ? 2u : 1u;
    for (const auto& ch : PL.chunks) {
        P.first_query = ch.first; P.n_queries = ch.count;
        // one wave per query, previous row in registers for up to 1024 columns (u16: two passes of 512, u32: four of 256)
        if (narrow) hipLaunchKernelGGL((poa2_forward_kernel<uint16_t, 2>), dim3(ch.count), dim3(64), 0, stream, P);
        else hipLaunchKernelGGL((poa2_forward_kernel<uint32_t, 4>), dim3(ch.count), dim3(64), 0, stream, P);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        if (narrow) hipLaunchKernelGGL(poa2_traceback_kernel<uint16_t>, dim3((ch.count + 63) / 64), dim3(64), 0, stream, P);
        else hipLaunchKernelGGL(poa2_traceback_kernel<uint32_t>, dim3((ch.count + 63) / 64), dim3(64), 0, stream, P);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark(2)) return rc;
    }
    return run.end_pairs();
}

int poa_batch_fetch_planes_2piece(poa_batch_t* b, uint32_t query, uint32_t* m, uint32_t* i1, uint32_t* d1, uint32_t* i2, uint32_t* d2) {
    if (!b || !m || !i1 || !d1 || !i2 || !d2) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_planes_2piece: null argument");
    if (!b->ran || query >= b->n_queries) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_planes_2piece: bad query / not run");
    if (b->ckpt2) return fail(POA_ERR_UNSUPPORTED, "poa_batch_fetch_planes_2piece: a checkpointed batch keeps snapshots and one segment window, no score planes");
    if (!b->two_piece || b->last_mode != POA_MODE_DENSE) return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_planes_2piece: the last run was not a dense two-piece run");
    const auto& last = b->cur().chunks.back();
    if (query < last.first || query >= last.first + last.count)
        return fail(POA_ERR_INVALID_ARG, "poa_batch_fetch_planes_2piece: the query's planes were overwritten by a later chunk");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    const uint32_t rows = b->graph->g.n, pitch = b->h_pitch[query];
    const uint32_t cols = (uint32_t)(b->h_qoff[query + 1] - b->h_qoff[query]) + 1;
    const uint64_t RP = (uint64_t)rows * pitch;
    uint32_t* dst[5] = {m, i1, d1, i2, d2};
    if (!b->narrow) {
        for (int k = 0; k < 5; ++k) {
            const uint32_t* src = b->d_planes.p + b->cur().off[query] + k * RP;
            HIP_TRY(hipMemcpy2D(dst[k], (size_t)cols * 4, src, (size_t)pitch * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToHost));
        }
    } else {
        std::vector<uint16_t> tmp((size_t)rows * cols);
        const uint16_t* base = reinterpret_cast<const uint16_t*>(b->d_planes.p) + 2 * b->cur().off[query];   // (the 4-byte plan's offset)
        for (int k = 0; k < 5; ++k) {
            HIP_TRY(hipMemcpy2D(tmp.data(), (size_t)cols * 2, base + k * RP, (size_t)pitch * 2, (size_t)cols * 2, rows, hipMemcpyDeviceToHost));
            for (size_t t = 0; t < tmp.size(); ++t) dst[k][t] = tmp[t] == 0xFFFFu ? 0xFFFFFFFFu : tmp[t];
        }
    }
    return POA_OK;
}

void poa_batch_destroy(poa_batch_t* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->ran) (void)hipStreamSynchronize(b->last_stream);  // the plane workspace may be handed to another batch next
    delete b;
}

// one-shot score-only call: a batch sized from the slot footprint, one run, scores and flags back; pair_off all zero.
// First version: it creates and destroys a whole resident batch per call (device tables, events, a workspace that is reused
// from the parked one only at exactly the same size), a fixed cost that has not been measured against the kernel's few
// milliseconds; a host that screens many small batches keeps a batch per shape (poa_batch_create_ex) or batches more reads.
static int sweep_one_shot(const poa_graph_t* g, uint32_t cost_x, uint32_t cost_o, uint32_t cost_e, const poa_config_t* cfg,
                          uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint32_t* score, uint64_t* pair_off,
                          uint32_t* flags, poa_stats_t* stats, int device) {
    const TuneView T(cfg);
    poa_batch_t* b = nullptr;
    int rc = batch_create_impl(g, device, n_queries, qseq, qoff, 0, true, &b);
    if (rc != POA_OK) return rc;
    rc = run_sweep(b, cost_x, cost_o, cost_e, T, nullptr);
    if (rc == POA_OK) rc = poa_batch_fetch(b, score, nullptr, pair_off, 0, flags, stats);
    poa_batch_destroy(b);
    return rc;
}

int poa_align_batch(const poa_graph_t* g, const poa_costs_t* costs, uint32_t n_queries, const uint8_t* qseq,
                    const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off,
                    uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats, int device) {
    return poa_align_batch_ex(g, costs, nullptr, n_queries, qseq, qoff, score, pairs, pair_off, pair_capacity, flags, stats, device);
}

int poa_align_batch_ex(const poa_graph_t* g, const poa_costs_t* costs, const poa_config_t* cfg, uint32_t n_queries,
                       const uint8_t* qseq, const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off,
                       uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats, int device) {
    if (!g || !costs || !qoff) return fail(POA_ERR_INVALID_ARG, "poa_align_batch: null argument");
    if (cfg && cfg->mode == POA_MODE_CHECKPOINT2)
        return fail(POA_ERR_UNSUPPORTED, "POA_MODE_CHECKPOINT2 is the two-piece model's checkpointed mode: poa_align_batch_2piece_ex / poa_batch_run_2piece");
    const TuneView T(cfg);
    if (stats) std::memset(stats, 0, sizeof(*stats));
    // PoastaAligner::align, empty-graph shortcut (src/aligner/mod.rs:124-142): score 4*len, no pairs
    if (g->g.n_real == 0) {
        for (uint32_t i = 0; i < n_queries; ++i) {
            const uint64_t L = qoff[i + 1] - qoff[i];
            if (score) score[i] = (uint32_t)(L * 4);
            if (flags) flags[i] = POA_FLAG_EMPTY_GRAPH;
            if (pair_off) pair_off[i] = 0;
        }
        if (pair_off) pair_off[n_queries] = 0;
        if (stats) { stats->n_queries = n_queries; stats->n_flagged = n_queries; }
        return POA_OK;
    }
    if (cfg && cfg->mode == POA_MODE_SCORE) {
        if (cfg->span == POA_SPAN_ENDS_FREE)
            return fail(POA_ERR_UNSUPPORTED, "score-only mode is Global: an ends-free result is defined by the reference's search");
        return sweep_one_shot(g, costs->mismatch, costs->gap_open, costs->gap_extend, cfg, n_queries, qseq, qoff, score, pair_off, flags, stats, device);
    }
    if (cfg && cfg->mode == POA_MODE_CHECKPOINT) {
        // one-shot checkpointed call: a batch sized from the plan's footprint, one run, everything dense mode returns
        if (cfg->span == POA_SPAN_ENDS_FREE)
            return fail(POA_ERR_UNSUPPORTED, "checkpointed mode is Global: an ends-free result is defined by the reference's search");
        poa_batch_t* cb = nullptr;
        int crc = poa_batch_create_ex(g, device, n_queries, qseq, qoff, cfg, 0, &cb);
        if (crc != POA_OK) return crc;
        crc = poa_batch_run_ex(cb, costs, cfg, nullptr);
        if (crc == POA_OK) crc = poa_batch_fetch(cb, score, pairs, pair_off, pair_capacity, flags, stats);
        poa_batch_destroy(cb);
        return crc;
    }
    // size the workspace for the layout this run will use (2-byte elements when the dense pass can run in u16)
    uint64_t ws_hint = 0;
    {
        uint64_t max_len = 0, elems = 0;
        for (uint32_t i = 0; i < n_queries; ++i) {
            const uint64_t L = qoff[i + 1] - qoff[i];
            max_len = std::max(max_len, L);
            elems += 3ull * g->g.n * (((L + 1 + 63) / 64) * 64);
        }
        const bool dense = !cfg || (cfg->mode == POA_MODE_DENSE && cfg->span == POA_SPAN_GLOBAL);
        if (dense && u16_cells_suffice(costs->gap_open, costs->gap_extend, max_len, g->g) && !T.ptr(POA_TUNE_PLANES)) {
            size_t free_b = 0, total_b = 0;
            if (hipSetDevice(device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && elems * 2 < free_b / 2)
                ws_hint = elems * 2;
        }
    }
    const bool timing = T.ptr(POA_TUNE_TIMING);
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    poa_batch_t* b = nullptr;
    int rc = poa_batch_create(g, device, n_queries, qseq, qoff, ws_hint, &b);
    if (rc != POA_OK) return rc;
    const double t1 = now();
    rc = poa_batch_run_ex(b, costs, cfg, nullptr);
    const double t2 = now();
    if (rc == POA_OK) rc = poa_batch_fetch(b, score, pairs, pair_off, pair_capacity, flags, stats);
    // replay out of queue space (POA_FLAG_EXACT_OVERFLOW keeps the dense result): before settling for that, run again with
    // a queue pool 8x, then 64x the size (unless the caller fixed a tiny budget on purpose: queue_entries_per_cell < 1e-3)
    if (rc == POA_OK && cfg && cfg->mode != POA_MODE_DENSE && flags && !(cfg->queue_entries_per_cell > 0.f && cfg->queue_entries_per_cell < 1e-3f)) {
        poa_config_t c2 = *cfg;
        float f = cfg->queue_entries_per_cell > 0.f ? cfg->queue_entries_per_cell : 0.25f;
        for (int attempt = 0; attempt < 2; ++attempt) {
            bool over = false;
            for (uint32_t i = 0; i < n_queries && !over; ++i) over = (flags[i] & POA_FLAG_EXACT_OVERFLOW) != 0;
            if (!over) break;
            f *= 8.f;
            c2.queue_entries_per_cell = f;
            rc = poa_batch_run_ex(b, costs, &c2, nullptr);
            if (rc == POA_ERR_OUT_OF_MEMORY) { rc = POA_OK; break; }   // the larger pool does not fit: keep what the first run gave
            if (rc == POA_OK) rc = poa_batch_fetch(b, score, pairs, pair_off, pair_capacity, flags, stats);
            if (rc != POA_OK) break;
        }
    }
    const double t3 = now();
    poa_batch_destroy(b);
    if (timing) std::fprintf(stderr, "poa_align_batch: create %.2f ms, launch %.2f ms, fetch (sync + copies) %.2f ms, destroy %.2f ms\n", t1 - t0, t2 - t1, t3 - t2, now() - t3);
    return rc;
}

void poa_release_cache(void) {
    g_buf_cache.release_all();
    std::lock_guard<std::mutex> lk(g_ws_cache.mu);
    for (int d = 0; d < 16; ++d) {
        if (!g_ws_cache.p[d]) continue;
        (void)hipSetDevice(d);
        (void)hipFree(g_ws_cache.p[d]);
        g_ws_cache.p[d] = nullptr; g_ws_cache.bytes[d] = 0;
    }
}

}  // extern "C"


// ---- two-piece affine model (poa_twopiece.hpp): the one-shot calls ------------------------------------------------------------
// Like every one-shot call: the checks, then a batch, one run through its frame, fetch, destroy.  mode: DENSE = the dense
// Global pass; EXACT / HYBRID = the replay of the reference's search for EVERY query (under this model a dense flag of 0
// certifies the alignment only where the reference's search is optimal, and it need not be: DESIGN.md §6a - so there is no
// cheaper hybrid).  fetch_extra(batch) reads what else the caller wants from a run that went well, before the results' fetch.
namespace {
template <typename FetchExtra>
int two_piece_one_shot(const poa_graph_t* g, const poa_costs2_t* costs, const poa_config_t* cfg, uint32_t n_queries, const uint8_t* qseq,
                       const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity, uint32_t* flags,
                       poa_stats_t* stats, int device, FetchExtra&& fetch_extra) {
    if (!g || !costs || (n_queries && (!qseq || !qoff))) return fail(POA_ERR_INVALID_ARG, "poa_align_batch_2piece: null argument");
    const bool score_only = cfg && cfg->mode == POA_MODE_SCORE;
    const bool exact = cfg && cfg->mode != POA_MODE_DENSE && !score_only && cfg->mode != POA_MODE_CHECKPOINT2;
    if (cfg && cfg->mode == POA_MODE_CHECKPOINT) return fail(POA_ERR_UNSUPPORTED, "checkpointed mode: one-piece gap-affine model only");
    if (cfg && cfg->mode > POA_MODE_CHECKPOINT2) return fail(POA_ERR_INVALID_ARG, "poa_align_batch_2piece_ex: unknown mode");
    const bool ckpt2 = cfg && cfg->mode == POA_MODE_CHECKPOINT2;
    if (ckpt2 && cfg->span == POA_SPAN_ENDS_FREE)
        return fail(POA_ERR_UNSUPPORTED, "checkpointed mode is Global: an ends-free result is defined by the reference's search");
    if (score_only && cfg->span == POA_SPAN_ENDS_FREE)
        return fail(POA_ERR_UNSUPPORTED, "score-only mode is Global: an ends-free result is defined by the reference's search");
    if (cfg && cfg->span > POA_SPAN_ENDS_FREE) return fail(POA_ERR_INVALID_ARG, "poa_align_batch_2piece_ex: unknown alignment span");
    const bool ends_free = cfg && cfg->span == POA_SPAN_ENDS_FREE;
    if (ends_free && !exact) return fail(POA_ERR_UNSUPPORTED, "two-piece model: ends-free alignment needs the exact replay (mode EXACT)");
    const TuneView T(cfg);
    if (costs->gap_extend1 < costs->gap_extend2)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    if (poa_device_count() <= 0) return fail(POA_ERR_NO_DEVICE, "no HIP device: the engine has no CPU alignment path");
    const FlatGraph& fg = g->g;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (pair_off) pair_off[0] = 0;
    if (n_queries == 0) return POA_OK;
    uint64_t max_len = 0;
    for (uint32_t i = 0; i < n_queries; ++i) {
        if (qoff[i + 1] < qoff[i]) return fail(POA_ERR_INVALID_ARG, "qoff must be non-decreasing");
        max_len = std::max<uint64_t>(max_len, qoff[i + 1] - qoff[i]);
    }
    if (fg.n_real == 0) {  // empty graph: mod.rs:124-142
        for (uint32_t i = 0; i < n_queries; ++i) {
            if (score) score[i] = (uint32_t)(4 * (qoff[i + 1] - qoff[i]));
            if (flags) flags[i] = POA_FLAG_EMPTY_GRAPH;
            if (pair_off) pair_off[i + 1] = 0;
        }
        if (stats) { stats->n_queries = n_queries; stats->n_flagged = n_queries; }
        return POA_OK;
    }
    if (score_only) {
        // the two-piece optimum is the one-piece optimum under open' = open1 + extend1 - extend2, extend' = extend2
        // (a gap of length k costs open1 + extend1 + (k - 1) * extend2 at its cheapest): the same sweep, wider cost fields
        if (pair_off) std::memset(pair_off, 0, ((size_t)n_queries + 1) * sizeof(uint64_t));
        return sweep_one_shot(g, costs->mismatch, (uint32_t)costs->gap_open1 + costs->gap_extend1 - costs->gap_extend2, costs->gap_extend2, cfg,
                              n_queries, qseq, qoff, score, pair_off, flags, stats, device);
    }
    if (!ckpt2 && 5ull * fg.n * ((max_len + 64) & ~63ull) >= (1ull << 34)) return fail(POA_ERR_UNSUPPORTED, "two-piece pass: planes of one query too large");
    Replay2Sizes z{};
    if (exact)
        if (const int rc = replay2_sizes(g, max_len, costs, cfg, z)) return rc;
    // The workspace the batch is asked to hold (two_piece_workspace, poa_dense_plan.cpp), in the bytes per cell of pitch the run
    // addresses: 20 for five u32 planes; a u16 run lives in the batch's 4-byte three-plane regions, 12, of which it uses 10.
    // A checkpointed batch holds its own footprint.  (A device that cannot be asked is refused by the constructor.)
    uint64_t ws_request = 0;
    uint32_t max_slots = ~0u;
    if (!ckpt2) {
        const bool narrow = u16_cells_suffice(costs->gap_open1, costs->gap_extend1, max_len, fg) && !costs->wide_planes && !exact;
        uint64_t total = 0, largest = 0;
        for (uint32_t i = 0; i < n_queries; ++i) {
            const uint64_t bytes = (narrow ? 12ull : 20ull) * fg.n * ((qoff[i + 1] - qoff[i] + 64) & ~63ull);
            total += bytes; largest = std::max(largest, bytes);
        }
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            // a parked workspace counts as free for the dense pass, whose batch takes it over or frees it; the replay's search
            // workspaces come out of what is free now, so its budget counts that alone
            const TwoPieceWorkspace w = two_piece_workspace(free_b + (exact ? 0 : parked_workspace_bytes(device)), total, largest, z.slot_bytes, exact);
            ws_request = w.bytes; max_slots = w.max_slots;
        }
    }
    poa_batch_t* b = nullptr;
    int rc = ckpt2 ? poa_batch_create_ex(g, device, n_queries, qseq, qoff, cfg, 0, &b) : poa_batch_create(g, device, n_queries, qseq, qoff, ws_request, &b);
    if (rc != POA_OK) return rc;
    rc = exact ? run_replay2(b, costs, cfg, T, z, max_slots, nullptr) : poa_batch_run_2piece(b, costs, cfg, nullptr);
    if (rc == POA_OK) rc = fetch_extra(b);   // (before the fetch: a pair_capacity that is too small keeps nothing else back)
    if (rc == POA_OK) rc = poa_batch_fetch(b, score, pairs, pair_off, pair_capacity, flags, stats);
    poa_batch_destroy(b);
    return rc;
}
}  // namespace

int poa_align_batch_2piece(const poa_graph_t* g, const poa_costs2_t* costs, uint32_t n_queries, const uint8_t* qseq,
                           const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off,
                           uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats, int device) {
    return two_piece_one_shot(g, costs, nullptr, n_queries, qseq, qoff, score, pairs, pair_off, pair_capacity, flags, stats, device,
                              [](poa_batch_t*) { return POA_OK; });
}

int poa_align_batch_2piece_ex(const poa_graph_t* g, const poa_costs2_t* costs, const poa_config_t* cfg, uint32_t n_queries,
                              const uint8_t* qseq, const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off,
                              uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats, uint32_t* search_counters, int device) {
    return two_piece_one_shot(g, costs, cfg, n_queries, qseq, qoff, score, pairs, pair_off, pair_capacity, flags, stats, device, [&](poa_batch_t* b) {
        const bool replayed = b->two_piece && b->last_mode != POA_MODE_DENSE;
        return replayed && search_counters ? poa_batch_fetch_search_counters(b, search_counters) : POA_OK;
    });
}

// the five planes of one query: a batch of one, one dense run, the planes of its last (only) chunk
int poa_planes_2piece(const poa_graph_t* g, const poa_costs2_t* costs, const uint8_t* seq, uint32_t len, uint32_t* m,
                      uint32_t* i1, uint32_t* d1, uint32_t* i2, uint32_t* d2, int device) {
    if (!m || !i1 || !d1 || !i2 || !d2) return fail(POA_ERR_INVALID_ARG, "poa_planes_2piece: null plane");
    const uint64_t qoff[2] = {0, len};
    return two_piece_one_shot(g, costs, nullptr, 1, seq, qoff, nullptr, nullptr, nullptr, 0, nullptr, nullptr, device,
                              [&](poa_batch_t* b) { return poa_batch_fetch_planes_2piece(b, 0, m, i1, d1, i2, d2); });
}

// ---- multi-graph checkpointed batch (poa_multi.hpp, poa_multi_plan.hpp) -----------------------------------------------------
// The batch's buffers, events, fetch and statistics are those of a poa_batch (`core`, no graph of its own): poa_batch_fetch,
// poa_batch_stats and poa_batch_device_results serve it unchanged.  What is new lies beside it: the plan, the concatenated
// tables of all graphs and one parameter block per graph.
struct poa_multi {
    poa_batch core;
    MultiPlan plan;
    std::vector<uint64_t> ub_open, ub_extend;   // per graph with queries: the u16 bound is open * ub_open + extend * ub_extend
    uint64_t stored_rows_pitch = 0;             // sum over queries of (2 x (slotted + snapshot rows) + 3 x rows) x pitch: cells a run stores
    DevBuf<uint32_t> d_slot, d_pred_slot, d_graph_of, d_carry_off;
    DevBuf<MultiGraphParams> d_params;
    DevBuf<Multi2GraphParams> d_params2;        // a batch of poa_multi_create_2piece holds these instead (core.ckpt2 is set)
    // a batch of poa_multi_create_dense (poa_multi_dense.hpp): compact u16 planes in the workspace, d_slot / d_pred_slot hold
    // FlatGraph::d_slot by row / pred_dslot by edge, one MultiDenseBlock per listed graph; core.ckpt is not set
    bool dense = false;
    DevBuf<MultiDenseBlock> d_dense;
    // a batch of poa_multi_create_exact (poa_multi_exact.hpp): the dense batch's buffers (`dense` is NOT set: the kinds refuse each
    // other's run calls), behind every chunk's dense regions the u32 visited tables, the ExactGraph arrays of all graphs
    // concatenated, one MultiExactBlock per listed graph, and the slots' replay workspace in one buffer (MultiExactSlot)
    bool exact = false;
    // a batch of poa_multi_create_dense_2piece (poa_multi_dense2.hpp): five full u16 planes per query in the workspace, one
    // MultiDense2Block per listed graph; neither core.ckpt nor `dense` is set
    bool dense2 = false;
    DevBuf<MultiDense2Block> d_dense2;
    DevBuf<MultiExactBlock> d_exact;
    DevBuf<uint64_t> d_table_off;
    DevBuf<uint8_t> d_x_sym, d_x_ws;
    DevBuf<uint32_t> d_x_succ_off, d_x_nbm_off, d_x_succ, d_x_dist_min, d_x_dist_max, d_x_exit_idx;
    DevBuf<FlatGraph::NodeBubble> d_x_nbm;
    DevBuf<FlatGraph::RowRec> d_x_rec;
    std::vector<MultiExactBlock> h_exact;   // the host's copy: LDS sizes per graph
    MultiExactSlot x_slot;                  // what d_x_ws is laid out for
};

namespace {
enum class MultiKind { checkpoint, checkpoint2, dense, Exact, dense2 };   // what a poa_multi holds: its plan, its footprint, its run

int multi_mode_check(const poa_config_t* cfg, const char* who, bool two_piece = false) {
    if (cfg && cfg->mode != (two_piece ? POA_MODE_CHECKPOINT2 : POA_MODE_CHECKPOINT))
        return fail(POA_ERR_UNSUPPORTED, std::string(who) + (two_piece ? ": a two-piece multi-graph batch runs in POA_MODE_CHECKPOINT2 only"
                                                                       : ": a multi-graph batch runs in POA_MODE_CHECKPOINT only"));
    if (cfg && cfg->span != POA_SPAN_GLOBAL)
        return fail(POA_ERR_UNSUPPORTED, std::string(who) + ": checkpointed mode is Global: an ends-free result is defined by the reference's search");
    return POA_OK;
}
int multi_dense_mode_check(const poa_config_t* cfg, const char* who) {
    if (cfg && cfg->mode != POA_MODE_DENSE)
        return fail(POA_ERR_UNSUPPORTED, std::string(who) + ": a dense multi-graph batch runs in POA_MODE_DENSE only (the checkpointed batches: poa_multi_create, poa_multi_create_2piece)");
    if (cfg && cfg->span != POA_SPAN_GLOBAL)
        return fail(POA_ERR_UNSUPPORTED, std::string(who) + ": a dense multi-graph batch is Global: an ends-free result is defined by the reference's search");
    return POA_OK;
}
// the exact kind: POA_MODE_EXACT (NULL cfg too) or POA_MODE_HYBRID, Global, a known heuristic
int multi_exact_mode_check(const poa_config_t* cfg, const char* who) {
    if (cfg && cfg->mode != POA_MODE_EXACT && cfg->mode != POA_MODE_HYBRID)
        return fail(POA_ERR_UNSUPPORTED, std::string(who) + ": an exact multi-graph batch runs in POA_MODE_EXACT or POA_MODE_HYBRID only (every other mode of one "
                                         "graph: poa_align_batch_ex; the dense and checkpointed batches: poa_multi_create_dense, poa_multi_create)");
    if (cfg && cfg->span != POA_SPAN_GLOBAL)
        return fail(POA_ERR_UNSUPPORTED, std::string(who) + ": an exact multi-graph batch is Global: an ends-free replay runs one graph at a time (poa_align_batch_ex)");
    if (cfg && cfg->heuristic > POA_HEURISTIC_MINGAP) return fail(POA_ERR_INVALID_ARG, std::string(who) + ": unknown heuristic");
    return POA_OK;
}
int multi_mode_check(MultiKind kind, const poa_config_t* cfg, const char* who) {
    if (kind == MultiKind::Exact) return multi_exact_mode_check(cfg, who);
    if (kind == MultiKind::dense || kind == MultiKind::dense2) return multi_dense_mode_check(cfg, who);
    return multi_mode_check(cfg, who, kind == MultiKind::checkpoint2);
}

// the plan of the kind (build_multi_plan with the model's weights, build_multi_dense_plan) behind the checks of the handles
int multi_plan_of(MultiKind kind, const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                  const poa_config_t* cfg, uint64_t workspace_bytes, MultiPlan& plan, const char* who) {
    if (!graph_qoff || !qoff || (n_graphs && !graphs)) return fail(POA_ERR_INVALID_ARG, std::string(who) + ": null argument");
    const bool two_piece = kind == MultiKind::checkpoint2;
    std::vector<MultiGraphIn> in(n_graphs);
    for (uint32_t g = 0; g < n_graphs; ++g) {
        if (!graphs[g]) return fail(POA_ERR_INVALID_ARG, std::string(who) + ": null graph");
        in[g] = MultiGraphIn{&graphs[g]->g, &graphs[g]->sweep, two_piece ? &graphs[g]->ckpt2 : &graphs[g]->ckpt};
    }
    std::string err;
    int rc;
    const bool wide = cfg && (cfg->flags & POA_CFG_WIDE_QUERIES);   // read by the dense and exact kinds alone
    if (kind == MultiKind::Exact) {
        // the bubble index of every listed graph, under the handle's lock as prepare_exact builds it
        for (uint32_t g = 0; g < n_graphs; ++g) {
            poa_graph* gr = const_cast<poa_graph*>(graphs[g]);
            std::lock_guard<std::mutex> lk(gr->bubble_mu);
            if (const int brc = build_bubble_index(gr->g, err)) return fail(brc, std::string(who) + ": " + err);
        }
        MultiExactCosts xc;   // the default costs' ring (64 priorities): a run with other costs recomputes the slot
        xc.queue_entries_per_cell = cfg ? cfg->queue_entries_per_cell : 0.f;
        rc = build_multi_exact_plan(in.data(), n_graphs, graph_qoff, qoff, workspace_bytes, xc, plan, err, wide);
    } else if (kind == MultiKind::dense) {
        rc = build_multi_dense_plan(in.data(), n_graphs, graph_qoff, qoff, workspace_bytes, plan, err, wide);
    } else if (kind == MultiKind::dense2) {
        rc = build_multi_dense2_plan(in.data(), n_graphs, graph_qoff, qoff, workspace_bytes, plan, err);
    } else {
        uint32_t seg_rows = 0;
        { const TuneView T(cfg); if (const int* v = T.ptr(POA_TUNE_CKPT_ROWS)) seg_rows = (*v) > 0 ? (uint32_t)(*v) : 0u; }
        rc = build_multi_plan(in.data(), n_graphs, graph_qoff, qoff, seg_rows, workspace_bytes, plan, err, two_piece);
    }
    if (rc != 0) return fail(rc, std::string(who) + ": " + err);
    return POA_OK;
}

// poa_multi_footprint, _2piece and _dense: the same sum with the plan of the kind
int multi_footprint_impl(MultiKind kind, const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                         const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes, const char* who_c) {
    const std::string who(who_c);
    if (!bytes && !largest_query_bytes) return fail(POA_ERR_INVALID_ARG, who + ": null argument");
    if (const int rc = multi_mode_check(kind, cfg, who_c)) return rc;
    return CreateFrame::guarded(who + ": host allocation failed", [&]() -> int {
        MultiPlan plan;
        if (const int rc = multi_plan_of(kind, graphs, n_graphs, graph_qoff, qoff, cfg, 0, plan, who_c)) return rc;
        if (bytes) *bytes = plan.bytes_total + plan.exact_bytes;   // (exact_bytes: the exact kind's slots, 0 for the others)
        if (largest_query_bytes) *largest_query_bytes = plan.largest_query_bytes;
        return POA_OK;
    });
}

// What the constructors of a poa_multi share in front of their tables: the handle, the two-pass plan around the device check,
// the core batch.
int multi_create_open(CreateFrame& frame, MultiKind kind, std::unique_ptr<poa_multi>& m, const poa_graph_t* const* graphs, uint32_t n_graphs,
                      const uint64_t* graph_qoff, int device, const uint8_t* qseq, const uint64_t* qoff, const poa_config_t* cfg,
                      uint64_t workspace_bytes, const char* refusal) {
    const char* who_c = frame.who.c_str();
    if (const int rc = multi_mode_check(kind, cfg, who_c)) return rc;
    m.reset(new (std::nothrow) poa_multi);
    if (!m) return fail(POA_ERR_OUT_OF_MEMORY, "host allocation failed");
    m->dense = kind == MultiKind::dense;
    m->exact = kind == MultiKind::Exact;
    m->dense2 = kind == MultiKind::dense2;
    MultiPlan& pl = m->plan;
    auto plan_of = [&](uint64_t ws, MultiPlan& plan) { return multi_plan_of(kind, graphs, n_graphs, graph_qoff, qoff, cfg, ws, plan, who_c); };
    // a first plan without a cap: the argument checks (no device needed) and the footprint the cap is chosen from
    if (const int rc = plan_of(0, pl)) return rc;
    const uint32_t n = pl.n_queries;
    if (n && qoff[n] && !qseq) return fail(POA_ERR_INVALID_ARG, frame.who + ": null argument");
    if (const int rc = frame.open(device)) return rc;
    const uint64_t fixed = pl.scratch_off[n] * 16 + (uint64_t)n * 64 + qoff[n] + (64ull << 20) + pl.max_carry_words * 4 +
                           (pl.n_rows_total + pl.n_edges_total) * 32 +
                           (kind == MultiKind::Exact ? pl.exact_bytes + pl.n_rows_total * 64 + (pl.n_succ_total + pl.n_nbm_total) * 16 : 0);
    if (const int rc = frame.plan_capped(pl, workspace_bytes, fixed, pl.largest_query_bytes, refusal, plan_of)) return rc;
    // the core batch: queries, results, pair buffers, events
    frame.fill_core(&m->core, pl, (m->dense || m->exact || m->dense2) ? pl.plane_bytes : pl.bytes_total, qoff);
    return POA_OK;
}

// poa_align_multi, _2piece and _dense: create, run, fetch, destroy
template <typename Create, typename Run>
int multi_one_shot(Create&& create, Run&& run, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                   uint32_t* flags, poa_stats_t* stats) {
    poa_multi_t* m = nullptr;
    int rc = create(&m);
    if (rc != POA_OK) return rc;
    rc = run(m);
    if (rc == POA_OK) rc = poa_multi_fetch(m, score, pairs, pair_off, pair_capacity, flags, stats);
    poa_multi_destroy(m);
    return rc;
}

// poa_multi_create and poa_multi_create_2piece: one batch, the plan's weights, the carries and the parameter blocks by the model
int multi_create_impl(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device, const uint8_t* qseq,
                      const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes, poa_multi_t** out, bool two_piece,
                      const char* who_c) {
    CreateFrame frame{who_c};
    std::unique_ptr<poa_multi> m;
    if (const int rc = multi_create_open(frame, two_piece ? MultiKind::checkpoint2 : MultiKind::checkpoint, m, graphs, n_graphs, graph_qoff, device,
                                         qseq, qoff, cfg, workspace_bytes, "the checkpointed footprint of the largest query does not fit in device memory"))
        return rc;
    const MultiPlan& pl = m->plan;
    const uint32_t n = pl.n_queries;
    poa_batch* b = &m->core;
    b->ckpt = true; b->ckpt2 = two_piece; b->last_mode = two_piece ? POA_MODE_CHECKPOINT2 : POA_MODE_CHECKPOINT;

    // concatenated tables, one copy per distinct handle
    std::vector<RowMeta> h_rows(pl.n_rows_total);
    std::vector<uint32_t> h_slot(pl.n_rows_total), h_pred_rows(pl.n_edges_total), h_pred_slot(pl.n_edges_total), h_pred_src(pl.n_edges_total);
    std::vector<uint32_t> h_snap_off(pl.n_snap_off_total), h_snap_dst(pl.n_snap_dst_total), h_boundary(pl.n_boundary_total);
    using GP = MultiGraphPlan;
    concat_tables(h_rows, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->g.rows; });
    concat_tables(h_slot, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->sweep.slot; });
    concat_tables(h_pred_rows, pl.graphs, &GP::edge_base, [&](uint32_t g) -> auto& { return graphs[g]->g.pred_rows; });
    concat_tables(h_pred_slot, pl.graphs, &GP::edge_base, [&](uint32_t g) -> auto& { return graphs[g]->sweep.pred_slot; });
    concat_tables(h_pred_src, pl.graphs, &GP::edge_base, [&](uint32_t g) -> auto& { return pl.graphs[g].ckpt.pred_src; });
    concat_tables(h_snap_off, pl.graphs, &GP::snap_off_base, [&](uint32_t g) -> auto& { return pl.graphs[g].ckpt.snap_off; });
    concat_tables(h_snap_dst, pl.graphs, &GP::snap_dst_base, [&](uint32_t g) -> auto& { return pl.graphs[g].ckpt.snap_dst; });
    concat_tables(h_boundary, pl.graphs, &GP::boundary_base, [&](uint32_t g) -> auto& { return pl.graphs[g].ckpt.boundary; });
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const MultiGraphPlan& gp = pl.graphs[g];
        // (two-piece: M, D1, D2 of the kept rows and five window planes, run_ckpt2's rule)
        const uint64_t stored = two_piece ? 3ull * (graphs[g]->sweep.n_slotted + gp.ckpt.n_snap_rows) + 5ull * gp.n_rows
                                          : 2ull * (graphs[g]->sweep.n_slotted + gp.ckpt.n_snap_rows) + 3ull * gp.n_rows;
        for (uint64_t i = graph_qoff[g]; i < graph_qoff[g + 1]; ++i) m->stored_rows_pitch += stored * pl.pitch[i];
        if (gp.n_queries) note_graph_bound(m->ub_open, m->ub_extend, gp.max_len, graphs[g]->g);
    }

    HIP_TRY(CreateFrame::alloc_each(pl.n_rows_total, b->d_rows, m->d_slot));
    HIP_TRY(CreateFrame::alloc_each(pl.n_edges_total, b->d_pred_rows, m->d_pred_slot, b->d_ck_pred_src));
    HIP_TRY(CreateFrame::alloc_each(pl.n_snap_off_total, b->d_ck_snap_off));
    HIP_TRY(CreateFrame::alloc_each(pl.n_snap_dst_total, b->d_ck_snap_dst));
    HIP_TRY(CreateFrame::alloc_each(pl.n_boundary_total, b->d_ck_boundary));
    HIP_TRY(CreateFrame::alloc_each(n, m->d_graph_of, m->d_carry_off));
    if (two_piece) HIP_TRY(CreateFrame::alloc_each(n_graphs, m->d_params2));
    else HIP_TRY(CreateFrame::alloc_each(n_graphs, m->d_params));
    if (const int rc = frame.alloc_results(b, qoff[n], n, n, true, pl.scratch_off[n])) return rc;
    HIP_TRY(CreateFrame::alloc_each(pl.max_carry_words, b->d_carry));
    if (const int rc = frame.acquire_planes(b, pl.workspace_bytes, true, "checkpointed workspace")) return rc;

    // one block per listed graph, CkptParams or Ckpt2Params by the model: the same fields but for the type of `scratch`
    std::vector<MultiGraphParams> h_params(two_piece ? 0 : n_graphs);
    std::vector<Multi2GraphParams> h_params2(two_piece ? n_graphs : 0);
    auto fill = [&](auto& mp, uint32_t g) {
        const MultiGraphPlan& gp = pl.graphs[g];
        const FlatGraph& fg = graphs[g]->g;
        std::memset(&mp, 0, sizeof(mp));
        auto& kp = mp.P;
        kp.rows = b->d_rows.p + gp.row_base; kp.slot = m->d_slot.p + gp.row_base;
        kp.pred_rows = b->d_pred_rows.p + gp.edge_base; kp.pred_slot = m->d_pred_slot.p + gp.edge_base; kp.pred_src = b->d_ck_pred_src.p + gp.edge_base;
        kp.snap_off = b->d_ck_snap_off.p + gp.snap_off_base; kp.snap_dst = b->d_ck_snap_dst.p + gp.snap_dst_base;
        kp.boundary = b->d_ck_boundary.p + gp.boundary_base;
        kp.n_rows = fg.n; kp.n_slots = gp.n_slots; kp.n_snap = gp.ckpt.n_snap_rows; kp.seg_rows = gp.ckpt.max_segment; kp.n_segments = gp.ckpt.n_segments();
        kp.start_row = fg.start_row; kp.end_row = fg.end_row;
        kp.qseq = b->d_qseq.p; kp.qoff = b->d_qoff.p; kp.pitch = b->d_pitch.p; kp.plane_off = b->plan[0].d_off.p;
        kp.planes = b->d_planes.p; kp.carry = b->d_carry.p;
        kp.scratch_off = b->d_scratch_off.p; kp.scratch = reinterpret_cast<decltype(kp.scratch)>(b->d_scratch.p);
        kp.score = b->d_score.p; kp.flags = b->d_flags.p; kp.n_pairs = b->d_npairs.p;
        mp.empty = fg.n_real == 0 ? 1u : 0u;
    };
    for (uint32_t g = 0; g < n_graphs; ++g) {
        if (two_piece) fill(h_params2[g], g);
        else fill(h_params[g], g);
    }

    if (const int rc = frame.begin_upload()) return rc;
    HIP_TRY(CreateFrame::upload(b->d_rows, h_rows));
    HIP_TRY(CreateFrame::upload(b->d_pred_rows, h_pred_rows));
    HIP_TRY(CreateFrame::upload(m->d_slot, h_slot));
    HIP_TRY(CreateFrame::upload(m->d_pred_slot, h_pred_slot));
    HIP_TRY(CreateFrame::upload(b->d_ck_pred_src, h_pred_src));
    HIP_TRY(CreateFrame::upload(b->d_ck_snap_off, h_snap_off));
    HIP_TRY(CreateFrame::upload(b->d_ck_snap_dst, h_snap_dst));
    HIP_TRY(CreateFrame::upload(b->d_ck_boundary, h_boundary));
    if (two_piece) HIP_TRY(CreateFrame::upload(m->d_params2, h_params2));
    else HIP_TRY(CreateFrame::upload(m->d_params, h_params));
    HIP_TRY(CreateFrame::upload(m->d_graph_of.p, pl.graph_of.data(), (size_t)n * 4));
    HIP_TRY(CreateFrame::upload(m->d_carry_off.p, pl.carry_off.data(), (size_t)n * 4));
    if (const int rc = frame.upload_queries(b, qseq, qoff, n, pl.scratch_off.data(), pl.pitch.data(), pl.region_off.data(), n)) return rc;
    if (const int rc = frame.end_upload(b)) return rc;

    *out = m.release();
    return POA_OK;
}

// poa_multi_create_dense: one batch of compact u16 planes, one MultiDenseBlock per listed graph
int multi_create_exact_tables(poa_multi* m, const poa_graph_t* const* graphs, uint32_t n_graphs);

// (exact: the same batch with the exact kind's plan; its own tables follow the dense ones, multi_create_exact_tables)
int multi_create_dense_impl(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device, const uint8_t* qseq,
                            const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes, poa_multi_t** out, bool exact = false) {
    CreateFrame frame{exact ? "poa_multi_create_exact" : "poa_multi_create_dense"};
    std::unique_ptr<poa_multi> m;
    if (const int rc = multi_create_open(frame, exact ? MultiKind::Exact : MultiKind::dense, m, graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, workspace_bytes,
                                         exact ? "the compact planes and the visited table of the largest query do not fit in device memory"
                                               : "the compact planes of the largest query do not fit in device memory"))
        return rc;
    const MultiPlan& pl = m->plan;
    const uint32_t n = pl.n_queries;
    poa_batch* b = &m->core;
    b->last_mode = exact ? POA_MODE_EXACT : POA_MODE_DENSE;

    // concatenated tables, one copy per distinct handle: rows and d_slot by row, pred_rows and pred_dslot by edge
    // (a graph without a d_slot table keeps its D rows by row: its part stays zero and its blocks carry null table pointers)
    std::vector<RowMeta> h_rows(pl.n_rows_total);
    std::vector<uint32_t> h_dslot(pl.n_rows_total, 0u), h_pred_rows(pl.n_edges_total), h_pred_dslot(pl.n_edges_total, 0u);
    using GP = MultiGraphPlan;
    concat_tables(h_rows, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->g.rows; });
    concat_tables(h_pred_rows, pl.graphs, &GP::edge_base, [&](uint32_t g) -> auto& { return graphs[g]->g.pred_rows; });
    concat_tables(h_dslot, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->g.d_slot; });
    concat_tables(h_pred_dslot, pl.graphs, &GP::edge_base, [&](uint32_t g) -> auto& { return graphs[g]->g.pred_dslot; });
    for (uint32_t g = 0; g < n_graphs; ++g)
        if (pl.graphs[g].n_queries) note_graph_bound(m->ub_open, m->ub_extend, pl.graphs[g].max_len, graphs[g]->g);

    HIP_TRY(CreateFrame::alloc_each(pl.n_rows_total, b->d_rows, m->d_slot));
    HIP_TRY(CreateFrame::alloc_each(pl.n_edges_total, b->d_pred_rows, m->d_pred_slot));
    HIP_TRY(CreateFrame::alloc_each(n, m->d_graph_of, m->d_carry_off));
    HIP_TRY(CreateFrame::alloc_each(n_graphs, m->d_dense));
    if (const int rc = frame.alloc_results(b, qoff[n], n, n, true, pl.scratch_off[n])) return rc;
    // the largest chunk's strip carries (POA_CFG_WIDE_QUERIES: 2 x rows words per query wider than one strip); at least one word,
    // FwdParams::strip_carry is a valid address that one-strip queries never touch
    HIP_TRY(CreateFrame::alloc_each(std::max<uint64_t>(1, pl.max_carry_words), b->d_carry));
    if (const int rc = frame.acquire_planes(b, pl.workspace_bytes, true, "dense multi-graph workspace")) return rc;

    // one block per listed graph: what poa_batch_run_ex puts into FwdParams / TbParams for that graph alone, absolute encoding
    std::vector<MultiDenseBlock> h_blocks(n_graphs);
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const MultiGraphPlan& gp = pl.graphs[g];
        const FlatGraph& fg = graphs[g]->g;
        MultiDenseBlock& mb = h_blocks[g];
        std::memset(&mb, 0, sizeof(mb));
        const bool by_row = fg.d_slot.empty();
        FwdParams& fp = mb.F;
        fp.rows = b->d_rows.p + gp.row_base; fp.pred_rows = b->d_pred_rows.p + gp.edge_base; fp.n_rows = fg.n;
        fp.qseq = b->d_qseq.p; fp.qoff = b->d_qoff.p; fp.pitch = b->d_pitch.p; fp.plane_off = b->plan[0].d_off.p;
        fp.planes = b->d_planes.p; fp.strip_carry = b->d_carry.p;
        fp.pred_k = nullptr;
        fp.d_slot = by_row ? nullptr : m->d_slot.p + gp.row_base; fp.pred_dslot = by_row ? nullptr : m->d_pred_slot.p + gp.edge_base;
        fp.pipeline_error = b->d_pipeline_error.p;
        TbParams& tp = mb.T;
        tp.rows = fp.rows; tp.pred_rows = fp.pred_rows; tp.n_rows = fg.n;
        tp.start_row = fg.start_row; tp.end_row = fg.end_row;
        tp.qseq = fp.qseq; tp.qoff = fp.qoff; tp.pitch = fp.pitch; tp.plane_off = fp.plane_off;
        tp.planes = b->d_planes.p; tp.scratch_off = b->d_scratch_off.p; tp.scratch = b->d_scratch.p;
        tp.score = b->d_score.p; tp.flags = b->d_flags.p; tp.n_pairs = b->d_npairs.p;
        tp.exact_pass = 0; tp.ex_status = nullptr; tp.ex_end = nullptr; tp.code_fmt = 0;
        tp.row_depth = nullptr;
        tp.d_slot = fp.d_slot; tp.pred_dslot = fp.pred_dslot;
        mb.empty = fg.n_real == 0 ? 1u : 0u;
    }

    if (const int rc = frame.begin_upload()) return rc;
    HIP_TRY(CreateFrame::upload(b->d_rows, h_rows));
    HIP_TRY(CreateFrame::upload(b->d_pred_rows, h_pred_rows));
    HIP_TRY(CreateFrame::upload(m->d_slot, h_dslot));
    HIP_TRY(CreateFrame::upload(m->d_pred_slot, h_pred_dslot));
    HIP_TRY(CreateFrame::upload(m->d_dense, h_blocks));
    HIP_TRY(CreateFrame::upload(m->d_graph_of.p, pl.graph_of.data(), (size_t)n * 4));
    HIP_TRY(CreateFrame::upload(m->d_carry_off.p, pl.carry_off.data(), (size_t)n * 4));
    if (const int rc = frame.upload_queries(b, qseq, qoff, n, pl.scratch_off.data(), pl.pitch.data(), pl.region_off.data(), n)) return rc;
    if (exact) { if (const int rc = multi_create_exact_tables(m.get(), graphs, n_graphs)) return rc; }
    if (const int rc = frame.end_upload(b)) return rc;

    *out = m.release();
    return POA_OK;
}

// what an exact batch holds beside the dense batch's buffers: the ExactGraph arrays of all graphs concatenated (graph-local
// values, one copy per distinct handle), one MultiExactBlock per listed graph, the table offsets, the per-query replay results
int multi_create_exact_tables(poa_multi* m, const poa_graph_t* const* graphs, uint32_t n_graphs) {
    const MultiPlan& pl = m->plan;
    const uint32_t n = pl.n_queries;
    poa_batch* b = &m->core;
    using GP = MultiGraphPlan;
    std::vector<uint8_t> h_sym(pl.n_sym_total, 0);
    std::vector<uint32_t> h_succ_off(pl.n_off_total), h_nbm_off(pl.n_off_total), h_succ(pl.n_succ_total), h_dmin(pl.n_rows_total),
        h_dmax(pl.n_rows_total), h_exit(pl.n_rows_total);
    std::vector<FlatGraph::NodeBubble> h_nbm(pl.n_nbm_total);
    std::vector<FlatGraph::RowRec> h_rec(pl.n_rows_total);   // (a graph without records leaves its part zero and its block a null pointer)
    std::vector<std::vector<uint8_t>> row_sym(n_graphs);
    for (uint32_t g = 0; g < n_graphs; ++g) {
        if (pl.graphs[g].table_of != g) continue;
        const FlatGraph& fg = graphs[g]->g;
        row_sym[g].resize(fg.n);
        for (uint32_t r = 0; r < fg.n; ++r) row_sym[g][r] = fg.rows[r].sym;
    }
    concat_tables(h_sym, pl.graphs, &GP::sym_base, [&](uint32_t g) -> auto& { return row_sym[g]; });
    concat_tables(h_succ_off, pl.graphs, &GP::off_base, [&](uint32_t g) -> auto& { return graphs[g]->g.succ_row_off; });
    concat_tables(h_nbm_off, pl.graphs, &GP::off_base, [&](uint32_t g) -> auto& { return graphs[g]->g.nbm_off; });
    concat_tables(h_succ, pl.graphs, &GP::succ_base, [&](uint32_t g) -> auto& { return graphs[g]->g.succ_rows; });
    concat_tables(h_dmin, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->g.dist_min; });
    concat_tables(h_dmax, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->g.dist_max; });
    concat_tables(h_exit, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->g.exit_idx; });
    concat_tables(h_nbm, pl.graphs, &GP::nbm_base, [&](uint32_t g) -> auto& { return graphs[g]->g.nbm; });
    concat_tables(h_rec, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->g.row_rec; });

    HIP_TRY(CreateFrame::alloc_each(pl.n_sym_total, m->d_x_sym));
    HIP_TRY(CreateFrame::alloc_each(pl.n_off_total, m->d_x_succ_off, m->d_x_nbm_off));
    HIP_TRY(CreateFrame::alloc_each(pl.n_succ_total, m->d_x_succ));
    HIP_TRY(CreateFrame::alloc_each(pl.n_rows_total, m->d_x_dist_min, m->d_x_dist_max, m->d_x_exit_idx, m->d_x_rec));
    HIP_TRY(CreateFrame::alloc_each(pl.n_nbm_total, m->d_x_nbm));
    HIP_TRY(CreateFrame::alloc_each(n_graphs, m->d_exact));
    HIP_TRY(CreateFrame::alloc_each(n, m->d_table_off, b->d_ex_status));
    HIP_TRY(CreateFrame::alloc_each(2 * (uint64_t)n, b->d_ex_end));
    HIP_TRY(CreateFrame::alloc_each(4 * (uint64_t)n, b->d_ex_counters));

    m->h_exact.assign(n_graphs, MultiExactBlock());
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const MultiGraphPlan& gp = pl.graphs[g];
        const FlatGraph& fg = graphs[g]->g;
        MultiExactBlock& xb = m->h_exact[g];
        std::memset(&xb, 0, sizeof(xb));
        xb.G = ExactGraph{fg.n, fg.start_row, fg.end_row, m->d_x_sym.p + gp.sym_base, m->d_x_succ_off.p + gp.off_base, m->d_x_succ.p + gp.succ_base,
                          m->d_x_dist_min.p + gp.row_base, m->d_x_dist_max.p + gp.row_base, m->d_x_exit_idx.p + gp.row_base, fg.n_exit,
                          m->d_x_nbm_off.p + gp.off_base, m->d_x_nbm.p + gp.nbm_base, nullptr, nullptr,   // (node_row, sp_to_end: ends-free spans only)
                          fg.row_rec.empty() ? nullptr : m->d_x_rec.p + gp.row_base};
        xb.n_succ = gp.n_succ; xb.n_nbm = gp.n_nbm;
        xb.graph_lds = exact_lds_bytes(fg.n, gp.n_succ, gp.n_nbm);
        xb.rec_lds = fg.row_rec.empty() ? 0u : (uint32_t)((fg.row_rec.size() * sizeof(FlatGraph::RowRec) + 15) & ~15ull);
        xb.empty = fg.n_real == 0 ? 1u : 0u;
    }
    HIP_TRY(CreateFrame::upload(m->d_x_sym, h_sym));
    HIP_TRY(CreateFrame::upload(m->d_x_succ_off, h_succ_off));
    HIP_TRY(CreateFrame::upload(m->d_x_nbm_off, h_nbm_off));
    HIP_TRY(CreateFrame::upload(m->d_x_succ, h_succ));
    HIP_TRY(CreateFrame::upload(m->d_x_dist_min, h_dmin));
    HIP_TRY(CreateFrame::upload(m->d_x_dist_max, h_dmax));
    HIP_TRY(CreateFrame::upload(m->d_x_exit_idx, h_exit));
    HIP_TRY(CreateFrame::upload(m->d_x_nbm, h_nbm));
    HIP_TRY(CreateFrame::upload(m->d_x_rec, h_rec));
    HIP_TRY(CreateFrame::upload(m->d_exact, m->h_exact));
    HIP_TRY(CreateFrame::upload(m->d_table_off.p, pl.table_off.data(), (size_t)n * 8));
    return POA_OK;
}
}  // namespace

extern "C" {

int poa_multi_footprint(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                        const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes) {
    return multi_footprint_impl(MultiKind::checkpoint, graphs, n_graphs, graph_qoff, qoff, cfg, bytes, largest_query_bytes, "poa_multi_footprint");
}

int poa_multi_footprint_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                               const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes) {
    return multi_footprint_impl(MultiKind::checkpoint2, graphs, n_graphs, graph_qoff, qoff, cfg, bytes, largest_query_bytes, "poa_multi_footprint_2piece");
}

int poa_multi_create(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device, const uint8_t* qseq,
                     const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes, poa_multi_t** out) {
    const char* who = "poa_multi_create";
    return CreateFrame::enter(who, out, std::string(who) + ": host allocation failed",
                              [&] { return multi_create_impl(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, workspace_bytes, out, false, who); });
}

int poa_multi_create_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device, const uint8_t* qseq,
                            const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes, poa_multi_t** out) {
    const char* who = "poa_multi_create_2piece";
    return CreateFrame::enter(who, out, std::string(who) + ": host allocation failed",
                              [&] { return multi_create_impl(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, workspace_bytes, out, true, who); });
}

// per chunk the sweep with snapshots (pass 1), then recompute-and-walk (pass 2), over the queries of all graphs; scan and
// compaction of the pairs over all queries
int poa_multi_run(poa_multi_t* m, const poa_costs_t* costs, const poa_config_t* cfg, void* stream_v) {
    if (!m || !costs) return fail(POA_ERR_INVALID_ARG, "poa_multi_run: null argument");
    // (the batch's model first: whatever the mode, this entry point cannot run a two-piece batch)
    if (m->core.ckpt2) return fail(POA_ERR_INVALID_ARG, "poa_multi_run: the batch was created by poa_multi_create_2piece (it runs through poa_multi_run_2piece only)");
    if (m->dense) return fail(POA_ERR_INVALID_ARG, "poa_multi_run: the batch was created by poa_multi_create_dense (it runs through poa_multi_run_dense only)");
    if (m->exact) return fail(POA_ERR_INVALID_ARG, "poa_multi_run: the batch was created by poa_multi_create_exact (it runs through poa_multi_run_exact only)");
    if (m->dense2) return fail(POA_ERR_INVALID_ARG, "poa_multi_run: the batch was created by poa_multi_create_dense_2piece (it runs through poa_multi_run_dense_2piece only)");
    const int mrc = multi_mode_check(cfg, "poa_multi_run");
    if (mrc != POA_OK) return mrc;
    const TuneView T(cfg);
    poa_batch* b = &m->core;
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(b->device));
    RunFrame run;
    if (const int rc = run.open(b, "poa_multi_run: call poa_multi_stats/fetch at least every 256 runs")) return rc;
    // u16 cells only if every graph's own bound (that graph's longest query and shortest path) allows them
    const bool narrow = !planes32(T) && all_graphs_u16(m->ub_open, m->ub_extend, costs->gap_open, costs->gap_extend);
    const MultiPlan& pl = m->plan;
    if (const int rc = run.begin(stream, pl.chunks.size())) return rc;
    b->last_mode = POA_MODE_CHECKPOINT;
    b->two_piece = false;
    set_layout(b, narrow);
    b->active_plan = 0;
    if (b->n_queries == 0) return run.end_empty(true);
    b->sweep_bytes_written = m->stored_rows_pitch * (narrow ? 2 : 4);
    for (const auto& ch : pl.chunks) {
        MultiLaunch ml;
        ml.graphs = m->d_params.p; ml.graph_of = m->d_graph_of.p; ml.carry_off = m->d_carry_off.p; ml.carry = b->d_carry.p;
        ml.first_query = ch.first; ml.n_queries = ch.count;
        ml.cost_x = costs->mismatch; ml.cost_o = costs->gap_open; ml.cost_e = costs->gap_extend;
        const uint32_t max_pitch = ch.max_pitch;
        const dim3 grid((ch.count + 3) / 4), block(256);
        launch_by_pitch(narrow, max_pitch, [&](auto cell, auto q) {
            hipLaunchKernelGGL((poa_ckpt_sweep_multi_kernel<decltype(q)::value, decltype(cell)>), grid, block, 0, stream, ml);
        });
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        launch_by_pitch(narrow, max_pitch, [&](auto cell, auto q) {
            hipLaunchKernelGGL((poa_ckpt_trace_multi_kernel<decltype(q)::value, decltype(cell)>), grid, block, 0, stream, ml);
        });
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark(2)) return rc;
    }
    return run.end_pairs();
}

// The same run under the two-piece model (poa_multi.hpp), on a batch of poa_multi_create_2piece: the cell width by the first
// piece's bound for every graph that has queries, the chunks of the batch under either width.
int poa_multi_run_2piece(poa_multi_t* m, const poa_costs2_t* costs, const poa_config_t* cfg, void* stream_v) {
    if (!m || !costs) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_2piece: null argument");
    if (m->dense) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_2piece: the batch was created by poa_multi_create_dense (it runs through poa_multi_run_dense only)");
    if (m->exact) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_2piece: the batch was created by poa_multi_create_exact (it runs through poa_multi_run_exact only)");
    if (m->dense2) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_2piece: the batch was created by poa_multi_create_dense_2piece (it runs through poa_multi_run_dense_2piece only)");
    if (!m->core.ckpt2) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_2piece: the batch was created by poa_multi_create (a two-piece run needs poa_multi_create_2piece: its footprint differs)");
    const int mrc = multi_mode_check(cfg, "poa_multi_run_2piece", true);
    if (mrc != POA_OK) return mrc;
    const TuneView T(cfg);
    poa_batch* b = &m->core;
    if (costs->gap_extend1 < costs->gap_extend2)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(b->device));
    RunFrame run;
    if (const int rc = run.open(b, "poa_multi_run_2piece: call poa_multi_stats/fetch at least every 256 runs")) return rc;
    // u16 cells only if every graph's own bound (the first piece's costs, that graph's longest query and shortest path) allows
    // them, and neither wide_planes nor the planes tunable asks for u32
    const bool narrow = !costs->wide_planes && !planes32(T) && all_graphs_u16(m->ub_open, m->ub_extend, costs->gap_open1, costs->gap_extend1);
    const MultiPlan& pl = m->plan;
    if (const int rc = run.begin(stream, pl.chunks.size())) return rc;
    b->last_mode = POA_MODE_CHECKPOINT2;
    b->two_piece = false;   // (no full planes to fetch)
    set_layout(b, narrow);
    b->active_plan = 0;
    if (b->n_queries == 0) return run.end_empty(true);
    b->sweep_bytes_written = m->stored_rows_pitch * (narrow ? 2 : 4);
    for (const auto& ch : pl.chunks) {
        Multi2Launch ml;
        ml.graphs = m->d_params2.p; ml.graph_of = m->d_graph_of.p; ml.carry_off = m->d_carry_off.p; ml.carry = b->d_carry.p;
        ml.first_query = ch.first; ml.n_queries = ch.count;
        ml.x = costs->mismatch; ml.o1 = costs->gap_open1; ml.e1 = costs->gap_extend1; ml.e2 = costs->gap_extend2;
        ml.oe = (uint32_t)costs->gap_open1 + costs->gap_extend1;
        const uint32_t max_pitch = ch.max_pitch;
        const dim3 grid((ch.count + 3) / 4), block(256);
        // NP follows the chunk's largest pitch: a strip of 64 x K x NP columns (K 8 for u16, 4 for u32) covers it up to 1024 columns
        launch_by_pitch(narrow, max_pitch, [&](auto cell, auto np) {
            hipLaunchKernelGGL((poa2_ckpt_sweep_multi_kernel<decltype(cell), decltype(np)::value>), grid, block, 0, stream, ml);
        });
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        launch_by_pitch(narrow, max_pitch, [&](auto cell, auto np) {
            hipLaunchKernelGGL((poa2_ckpt_trace_multi_kernel<decltype(cell), decltype(np)::value>), grid, block, 0, stream, ml);
        });
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark(2)) return rc;
    }
    return run.end_pairs();
}

int poa_multi_fetch(poa_multi_t* m, uint32_t* score, poa_aln_pair_t* pairs, uint64_t* pair_off, uint64_t pair_capacity,
                    uint32_t* flags, poa_stats_t* stats) {
    if (!m) return fail(POA_ERR_INVALID_ARG, "poa_multi_fetch: null batch");
    if (!m->core.ran) return fail(POA_ERR_INVALID_ARG, "poa_multi_fetch: poa_multi_run has not been called");
    return poa_batch_fetch(&m->core, score, pairs, pair_off, pair_capacity, flags, stats);
}

int poa_multi_stats(poa_multi_t* m, poa_stats_t* stats) {
    if (!m || !stats) return fail(POA_ERR_INVALID_ARG, "poa_multi_stats: null argument");
    return poa_batch_stats(&m->core, stats);
}

int poa_multi_device_results(poa_multi_t* m, void** score, void** flags, void** pair_off, void** pairs) {
    if (!m) return fail(POA_ERR_INVALID_ARG, "poa_multi_device_results: null batch");
    return poa_batch_device_results(&m->core, score, flags, pair_off, pairs);
}

int poa_multi_workspace_bytes(poa_multi_t* m, uint64_t* bytes) {
    if (!m || !bytes) return fail(POA_ERR_INVALID_ARG, "poa_multi_workspace_bytes: null argument");
    *bytes = m->core.d_planes.bytes;
    return POA_OK;
}

void poa_multi_destroy(poa_multi_t* m) {
    if (!m) return;
    (void)hipSetDevice(m->core.device);
    if (m->core.ran) (void)hipStreamSynchronize(m->core.last_stream);  // the plane workspace may be handed to another batch next
    delete m;
}

int poa_align_multi(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const poa_costs_t* costs,
                    const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs,
                    uint64_t* pair_off, uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats, int device) {
    if (!costs) return fail(POA_ERR_INVALID_ARG, "poa_align_multi: null argument");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return multi_one_shot([&](poa_multi_t** m) { return poa_multi_create(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, 0, m); },
                          [&](poa_multi_t* m) { return poa_multi_run(m, costs, cfg, nullptr); }, score, pairs, pair_off, pair_capacity, flags, stats);
}

int poa_align_multi_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const poa_costs2_t* costs,
                           const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs,
                           uint64_t* pair_off, uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats, int device) {
    if (!costs) return fail(POA_ERR_INVALID_ARG, "poa_align_multi_2piece: null argument");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (costs->gap_extend1 < costs->gap_extend2)   // (before a batch is made for it)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    return multi_one_shot([&](poa_multi_t** m) { return poa_multi_create_2piece(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, 0, m); },
                          [&](poa_multi_t* m) { return poa_multi_run_2piece(m, costs, cfg, nullptr); }, score, pairs, pair_off, pair_capacity, flags, stats);
}

}  // extern "C"


// ---- dense multi-graph batch (poa_multi_dense.hpp, build_multi_dense_plan) --------------------------------------------------
// The same object as the checkpointed batches above, of a third kind (poa_multi::dense): the workspace holds every query's
// compact u16 planes, a run is the packed forward launch and the walk launch per chunk, then the scan and compaction of pairs.
// The core is a dense poa_batch (ckpt not set), so poa_multi_fetch / _stats / _device_results / _workspace_bytes / _destroy
// serve it unchanged and poa_stats_t.plane_bytes is the planes' own size.  Its mode check, plan and constructor stand with the
// other two kinds' above (MultiKind::dense, multi_create_dense_impl).
namespace {
// The forward launch of one chunk of a dense or exact batch.  A chunk whose widest query is one strip launches the one-strip
// kernel by its quads, in a batch created with POA_CFG_WIDE_QUERIES too; a chunk with a wider query (only such a batch has one)
// launches the strip loop once for all its queries.  Returns the launch bits of the chunk's record.
uint32_t multi_dense_forward(const MultiDenseLaunch& ml, uint32_t max_pitch, dim3 grid, dim3 block, hipStream_t stream) {
    if (max_pitch > MULTI_STRIP_COLUMNS) {
        hipLaunchKernelGGL(poa_forward_packed_multi_wide_kernel, grid, block, 0, stream, ml);
        return POA_LAUNCH_STRIPS;
    }
    if (max_pitch <= 512) hipLaunchKernelGGL((poa_forward_packed_multi_kernel<1>), grid, block, 0, stream, ml);
    else hipLaunchKernelGGL((poa_forward_packed_multi_kernel<2>), grid, block, 0, stream, ml);
    return 0u;
}
}  // namespace

extern "C" {

int poa_graph_compact_elems(const poa_graph_t* g, uint32_t len, uint64_t* elems) {
    if (!g || !elems) return fail(POA_ERR_INVALID_ARG, "poa_graph_compact_elems: null argument");
    if (len > 0x7FFFFFF0u) return fail(POA_ERR_UNSUPPORTED, "poa_graph_compact_elems: query longer than 2^31");
    *elems = multi_dense_query_elems(g->g, len);
    return POA_OK;
}

int poa_multi_footprint_dense(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                              const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes) {
    return multi_footprint_impl(MultiKind::dense, graphs, n_graphs, graph_qoff, qoff, cfg, bytes, largest_query_bytes, "poa_multi_footprint_dense");
}

int poa_multi_create_dense(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device, const uint8_t* qseq,
                           const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes, poa_multi_t** out) {
    return CreateFrame::enter("poa_multi_create_dense", out, "poa_multi_create_dense: host allocation failed",
                              [&] { return multi_create_dense_impl(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, workspace_bytes, out); });
}

// per chunk the packed forward launch over the queries of all graphs, then the walk launch; scan and compaction of the pairs
// over all queries.  Nothing is written into the batch before every refusal has passed.
int poa_multi_run_dense(poa_multi_t* m, const poa_costs_t* costs, const poa_config_t* cfg, void* stream_v) {
    if (!m || !costs) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_dense: null argument");
    if (m->exact) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_dense: the batch was created by poa_multi_create_exact (it runs through poa_multi_run_exact only)");
    if (m->dense2) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_dense: the batch was created by poa_multi_create_dense_2piece (it runs through poa_multi_run_dense_2piece only)");
    if (!m->dense) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_dense: the batch was not created by poa_multi_create_dense (a checkpointed batch runs through poa_multi_run / poa_multi_run_2piece)");
    const int mrc = multi_dense_mode_check(cfg, "poa_multi_run_dense");
    if (mrc != POA_OK) return mrc;
    const TuneView T(cfg);
    // the batch is sized for u16 compact cells: every graph's own bound (its longest query and shortest path) must allow them
    const bool narrow = !planes32(T) && all_graphs_u16(m->ub_open, m->ub_extend, costs->gap_open, costs->gap_extend);
    if (!narrow)
        return fail(POA_ERR_UNSUPPORTED, "poa_multi_run_dense: the run needs u32 cells (the costs' score bound exceeds 65534 for some graph, or "
                                         "tune[POA_TUNE_PLANES] = 32) and a dense multi-graph batch holds u16 compact cells only; the checkpointed "
                                         "batch (poa_multi_create, poa_multi_run) runs either width");
    poa_batch* b = &m->core;
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(b->device));
    RunFrame run;
    if (const int rc = run.open(b, "poa_multi_run_dense: call poa_multi_stats/fetch at least every 256 runs")) return rc;
    const MultiPlan& pl = m->plan;
    if (const int rc = run.begin(stream, pl.chunks.size())) return rc;
    b->last_mode = POA_MODE_DENSE;
    b->two_piece = false;
    set_layout(b, true, true, false);
    b->active_plan = 0;
    b->launches.clear();
    if (b->n_queries == 0) return run.end_empty(true);
    for (const auto& ch : pl.chunks) {
        MultiDenseLaunch ml;
        ml.graphs = m->d_dense.p; ml.graph_of = m->d_graph_of.p;
        ml.first_query = ch.first; ml.n_queries = ch.count;
        ml.cost_x = costs->mismatch; ml.cost_o = costs->gap_open; ml.cost_e = costs->gap_extend;
        ml.spec_depth = 32;   // what plan_dense_chunk pairs with 64 lanes per walk on the compact layout
        ml.code_fmt = 0;
        ml.carry = b->d_carry.p; ml.carry_off = m->d_carry_off.p;
        const uint32_t quads = ch.max_pitch <= 512 ? 1u : 2u;   // 512 columns per quad
        const dim3 grid((ch.count + 3) / 4), block(256);
        const uint32_t strips = multi_dense_forward(ml, ch.max_pitch, grid, block, stream);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        hipLaunchKernelGGL(poa_traceback_multi_kernel, grid, block, 0, stream, ml);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark(2)) return rc;
        // the record of poa_batch_last_launch: kernel, quads, launch bits, waves per workgroup, code_fmt, lanes per walk, depth, queries
        b->launches.push_back(DenseChunkPlan{{POA_KERNEL_PACKED, quads, strips, 4u, ml.code_fmt, 64u, ml.spec_depth, ch.count}, -1, false, true, false});
    }
    return run.end_pairs();
}

int poa_multi_last_launch(poa_multi_t* m, uint32_t chunk, uint32_t out[8]) {
    if (!m || !out) return fail(POA_ERR_INVALID_ARG, "poa_multi_last_launch: null argument");
    if (!m->dense && !m->exact) return fail(POA_ERR_INVALID_ARG, "poa_multi_last_launch: the batch was not created by poa_multi_create_dense or poa_multi_create_exact");
    if (!m->core.ran) return fail(POA_ERR_INVALID_ARG, "poa_multi_last_launch: the batch has not been run");
    if (chunk >= m->core.launches.size()) return fail(POA_ERR_INVALID_ARG, "poa_multi_last_launch: the last run had no such chunk");
    for (int k = 0; k < 8; ++k) out[k] = m->core.launches[chunk].v[k];
    return POA_OK;
}

int poa_align_multi_dense(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const poa_costs_t* costs,
                          const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs,
                          uint64_t* pair_off, uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats, int device) {
    if (!costs) return fail(POA_ERR_INVALID_ARG, "poa_align_multi_dense: null argument");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return multi_one_shot([&](poa_multi_t** m) { return poa_multi_create_dense(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, 0, m); },
                          [&](poa_multi_t* m) { return poa_multi_run_dense(m, costs, cfg, nullptr); }, score, pairs, pair_off, pair_capacity, flags, stats);
}

}  // extern "C"


// ---- dense two-piece multi-graph batch (poa_multi_dense2.hpp, build_multi_dense2_plan) --------------------------------------
// A fifth kind of the same object (poa_multi::dense2): the workspace holds every query's five u16 planes, a run is per chunk the
// dense two-piece forward launch and the walk launch over the queries of all graphs, then the scan and compaction of pairs.  The
// core is a dense poa_batch (ckpt not set, two_piece not set: the stored bytes are the plan's, pitch included), so
// poa_multi_fetch / _stats / _device_results / _workspace_bytes / _destroy serve it unchanged.
namespace {
int multi_create_dense2_impl(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device, const uint8_t* qseq,
                             const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes, poa_multi_t** out) {
    CreateFrame frame{"poa_multi_create_dense_2piece"};
    std::unique_ptr<poa_multi> m;
    if (const int rc = multi_create_open(frame, MultiKind::dense2, m, graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, workspace_bytes,
                                         "the five score planes of the largest query do not fit in device memory"))
        return rc;
    const MultiPlan& pl = m->plan;
    const uint32_t n = pl.n_queries;
    poa_batch* b = &m->core;
    b->last_mode = POA_MODE_DENSE;

    // concatenated tables, one copy per distinct handle: rows by row, pred_rows by edge
    std::vector<RowMeta> h_rows(pl.n_rows_total);
    std::vector<uint32_t> h_pred_rows(pl.n_edges_total);
    using GP = MultiGraphPlan;
    concat_tables(h_rows, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->g.rows; });
    concat_tables(h_pred_rows, pl.graphs, &GP::edge_base, [&](uint32_t g) -> auto& { return graphs[g]->g.pred_rows; });
    for (uint32_t g = 0; g < n_graphs; ++g)
        if (pl.graphs[g].n_queries) note_graph_bound(m->ub_open, m->ub_extend, pl.graphs[g].max_len, graphs[g]->g);

    HIP_TRY(CreateFrame::alloc_each(pl.n_rows_total, b->d_rows));
    HIP_TRY(CreateFrame::alloc_each(pl.n_edges_total, b->d_pred_rows));
    HIP_TRY(CreateFrame::alloc_each(n, m->d_graph_of));
    HIP_TRY(CreateFrame::alloc_each(n_graphs, m->d_dense2));
    if (const int rc = frame.alloc_results(b, qoff[n], n, n, true, pl.scratch_off[n])) return rc;
    if (const int rc = frame.acquire_planes(b, pl.workspace_bytes, true, "dense two-piece multi-graph workspace")) return rc;

    // one block per listed graph: what poa_batch_run_2piece puts into TwoPieceParams for that graph alone; the chunk, the costs
    // and the planes base belong to the launch
    std::vector<MultiDense2Block> h_blocks(n_graphs);
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const MultiGraphPlan& gp = pl.graphs[g];
        const FlatGraph& fg = graphs[g]->g;
        MultiDense2Block& mb = h_blocks[g];
        std::memset(&mb, 0, sizeof(mb));
        TwoPieceParams& tp = mb.P;
        tp.rows = b->d_rows.p + gp.row_base; tp.pred_rows = b->d_pred_rows.p + gp.edge_base;
        tp.n_rows = fg.n; tp.start_row = fg.start_row; tp.end_row = fg.end_row;
        tp.qseq = b->d_qseq.p; tp.qoff = b->d_qoff.p;
        tp.q_pitch = b->d_pitch.p; tp.plane_off = b->plan[0].d_off.p; tp.off_scale = 1u;
        tp.score = b->d_score.p; tp.flags = b->d_flags.p; tp.n_pairs = b->d_npairs.p;
        tp.scratch = reinterpret_cast<poa_aln_pair_t*>(b->d_scratch.p); tp.scratch_off = b->d_scratch_off.p;
        mb.empty = fg.n_real == 0 ? 1u : 0u;
    }

    if (const int rc = frame.begin_upload()) return rc;
    HIP_TRY(CreateFrame::upload(b->d_rows, h_rows));
    HIP_TRY(CreateFrame::upload(b->d_pred_rows, h_pred_rows));
    HIP_TRY(CreateFrame::upload(m->d_dense2, h_blocks));
    HIP_TRY(CreateFrame::upload(m->d_graph_of.p, pl.graph_of.data(), (size_t)n * 4));
    if (const int rc = frame.upload_queries(b, qseq, qoff, n, pl.scratch_off.data(), pl.pitch.data(), pl.region_off.data(), n)) return rc;
    if (const int rc = frame.end_upload(b)) return rc;

    *out = m.release();
    return POA_OK;
}
}  // namespace

extern "C" {

int poa_multi_footprint_dense_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                                     const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes) {
    return multi_footprint_impl(MultiKind::dense2, graphs, n_graphs, graph_qoff, qoff, cfg, bytes, largest_query_bytes, "poa_multi_footprint_dense_2piece");
}

int poa_multi_create_dense_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device, const uint8_t* qseq,
                                  const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes, poa_multi_t** out) {
    return CreateFrame::enter("poa_multi_create_dense_2piece", out, "poa_multi_create_dense_2piece: host allocation failed",
                              [&] { return multi_create_dense2_impl(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, workspace_bytes, out); });
}

// per chunk the dense two-piece forward launch over the queries of all graphs (a wave per query), then the walk launch (a lane
// per query); scan and compaction of the pairs over all queries.  Nothing is written into the batch before every refusal has passed.
int poa_multi_run_dense_2piece(poa_multi_t* m, const poa_costs2_t* costs, const poa_config_t* cfg, void* stream_v) {
    const char* who = "poa_multi_run_dense_2piece";
    if (!m || !costs) return fail(POA_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (!m->dense2)
        return fail(POA_ERR_INVALID_ARG, std::string(who) + ": the batch was not created by poa_multi_create_dense_2piece (a checkpointed batch runs through "
                                         "poa_multi_run / poa_multi_run_2piece, a dense one through poa_multi_run_dense, an exact one through poa_multi_run_exact)");
    if (const int mrc = multi_dense_mode_check(cfg, who)) return mrc;
    if (costs->gap_extend1 < costs->gap_extend2)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    const TuneView T(cfg);
    // the batch is sized for u16 cells: every graph's own bound (the first piece's costs, its longest query and shortest path) must
    // allow them, and neither wide_planes nor the planes tunable may ask for u32
    const bool narrow = !costs->wide_planes && !planes32(T) && all_graphs_u16(m->ub_open, m->ub_extend, costs->gap_open1, costs->gap_extend1);
    if (!narrow)
        return fail(POA_ERR_UNSUPPORTED, std::string(who) + ": the run needs u32 cells (the first piece's score bound exceeds 65534 for some graph, "
                                         "costs->wide_planes, or tune[POA_TUNE_PLANES] = 32) and a dense two-piece multi-graph batch holds u16 cells "
                                         "only; the checkpointed batch (poa_multi_create_2piece, poa_multi_run_2piece) runs either width");
    poa_batch* b = &m->core;
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(b->device));
    RunFrame run;
    if (const int rc = run.open(b, std::string(who) + ": call poa_multi_stats/fetch at least every 256 runs")) return rc;
    const MultiPlan& pl = m->plan;
    if (const int rc = run.begin(stream, pl.chunks.size())) return rc;
    b->last_mode = POA_MODE_DENSE;
    b->two_piece = false;   // (poa_stats_t.plane_bytes is the plan's: whole pitches)
    set_layout(b, true);
    b->active_plan = 0;
    b->launches.clear();
    if (b->n_queries == 0) return run.end_empty(true);
    for (const auto& ch : pl.chunks) {
        MultiDense2Launch ml;
        ml.graphs = m->d_dense2.p; ml.graph_of = m->d_graph_of.p; ml.planes = b->d_planes.p;
        ml.first_query = ch.first; ml.n_queries = ch.count;
        ml.x = costs->mismatch; ml.o1 = costs->gap_open1; ml.e1 = costs->gap_extend1; ml.e2 = costs->gap_extend2;
        ml.oe = (uint32_t)costs->gap_open1 + costs->gap_extend1;
        // one wave per query, previous row in registers for up to 1024 columns (two passes of 512): poa_batch_run_2piece's variant
        hipLaunchKernelGGL((poa2_forward_multi_kernel<uint16_t, 2>), dim3((ch.count + 3) / 4), dim3(256), 0, stream, ml);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        hipLaunchKernelGGL(poa2_traceback_multi_kernel<uint16_t>, dim3((ch.count + 63) / 64), dim3(64), 0, stream, ml);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark(2)) return rc;
    }
    return run.end_pairs();
}

int poa_multi_fetch_planes_2piece(poa_multi_t* m, uint32_t query, uint32_t* mp, uint32_t* i1, uint32_t* d1, uint32_t* i2, uint32_t* d2) {
    const char* who = "poa_multi_fetch_planes_2piece";
    if (!m || !mp || !i1 || !d1 || !i2 || !d2) return fail(POA_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (!m->dense2) return fail(POA_ERR_INVALID_ARG, std::string(who) + ": the batch was not created by poa_multi_create_dense_2piece (no other kind keeps five planes)");
    poa_batch* b = &m->core;
    if (!b->ran || query >= b->n_queries) return fail(POA_ERR_INVALID_ARG, std::string(who) + ": bad query / not run");
    const MultiPlan& pl = m->plan;
    const auto& last = pl.chunks.back();
    if (query < last.first || query >= last.first + last.count)
        return fail(POA_ERR_INVALID_ARG, std::string(who) + ": the query's planes were overwritten by a later chunk");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    const uint32_t rows = pl.graphs[pl.graph_of[query]].n_rows, pitch = pl.pitch[query];
    const uint32_t cols = (uint32_t)(b->h_qoff[query + 1] - b->h_qoff[query]) + 1;
    const uint64_t RP = (uint64_t)rows * pitch;
    uint32_t* dst[5] = {mp, i1, d1, i2, d2};
    return CreateFrame::guarded(std::string(who) + ": host allocation failed", [&]() -> int {
        std::vector<uint16_t> tmp((size_t)rows * cols);
        const uint16_t* base = reinterpret_cast<const uint16_t*>(b->d_planes.p) + pl.region_off[query];
        for (int k = 0; k < 5; ++k) {
            HIP_TRY(hipMemcpy2D(tmp.data(), (size_t)cols * 2, base + k * RP, (size_t)pitch * 2, (size_t)cols * 2, rows, hipMemcpyDeviceToHost));
            for (size_t t = 0; t < tmp.size(); ++t) dst[k][t] = tmp[t] == 0xFFFFu ? 0xFFFFFFFFu : tmp[t];
        }
        return POA_OK;
    });
}

int poa_align_multi_dense_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const poa_costs2_t* costs,
                                 const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs,
                                 uint64_t* pair_off, uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats, int device) {
    if (!costs) return fail(POA_ERR_INVALID_ARG, "poa_align_multi_dense_2piece: null argument");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (costs->gap_extend1 < costs->gap_extend2)   // (before a batch is made for it)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    return multi_one_shot([&](poa_multi_t** m) { return poa_multi_create_dense_2piece(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, 0, m); },
                          [&](poa_multi_t* m) { return poa_multi_run_dense_2piece(m, costs, cfg, nullptr); }, score, pairs, pair_off, pair_capacity, flags, stats);
}

}  // extern "C"


// ---- exact multi-graph batch (poa_multi_exact.hpp, build_multi_exact_plan) --------------------------------------------------
// The dense batch above with the replay of the reference's search behind every chunk's dense pass (poa_multi::exact): per chunk
// the dense kind's two launches unchanged, the INF-fill of the replayed queries' u32 tables, ONE replay launch (a wave per query,
// every wave on its own graph's tables), ONE u32 walk launch over the replayed tables, then the scan and compaction.  It mirrors
// replay_chunk for one graph.  The core's last_mode is EXACT or HYBRID, so poa_multi_fetch counts n_exact and
// poa_batch_fetch_search_counters serves the counters.
extern "C" {

int poa_multi_footprint_exact(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const uint64_t* qoff,
                              const poa_config_t* cfg, uint64_t* bytes, uint64_t* largest_query_bytes) {
    return multi_footprint_impl(MultiKind::Exact, graphs, n_graphs, graph_qoff, qoff, cfg, bytes, largest_query_bytes, "poa_multi_footprint_exact");
}

int poa_multi_create_exact(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, int device, const uint8_t* qseq,
                           const uint64_t* qoff, const poa_config_t* cfg, uint64_t workspace_bytes, poa_multi_t** out) {
    return CreateFrame::enter("poa_multi_create_exact", out, "poa_multi_create_exact: host allocation failed",
                              [&] { return multi_create_dense_impl(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, workspace_bytes, out, true); });
}

int poa_multi_run_exact(poa_multi_t* m, const poa_costs_t* costs, const poa_config_t* cfg, void* stream_v) {
    const char* who = "poa_multi_run_exact";
    if (!m || !costs) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_exact: null argument");
    if (!m->exact) return fail(POA_ERR_INVALID_ARG, "poa_multi_run_exact: the batch was not created by poa_multi_create_exact (a dense batch runs through poa_multi_run_dense, a checkpointed one through poa_multi_run / poa_multi_run_2piece)");
    if (const int mrc = multi_exact_mode_check(cfg, who)) return mrc;
    const TuneView T(cfg);
    if (const int* iv = T.ptr(POA_TUNE_EXACT_IMPL)) {
        if (*iv != 0 && *iv != 2)
            return fail(POA_ERR_UNSUPPORTED, "poa_multi_run_exact: the lane and flat replay implementations run one graph at a time (poa_align_batch_ex); a multi-graph batch runs the wave search only");
    }
    if (const int* gv = T.ptr(POA_TUNE_WS_GROUP)) {
        if (*gv != 64)
            return fail(POA_ERR_UNSUPPORTED, "poa_multi_run_exact: several queries per wave run one graph at a time (poa_align_batch_ex); a multi-graph batch runs one query per wave");
    }
    const bool narrow = !planes32(T) && all_graphs_u16(m->ub_open, m->ub_extend, costs->gap_open, costs->gap_extend);
    if (!narrow)
        return fail(POA_ERR_UNSUPPORTED, "poa_multi_run_exact: the dense pass needs u32 cells (the costs' score bound exceeds 65534 for some graph, or "
                                         "tune[POA_TUNE_PLANES] = 32) and an exact multi-graph batch holds u16 compact cells only; poa_align_batch_ex "
                                         "runs either width, one graph at a time");
    poa_batch* b = &m->core;
    const MultiPlan& pl = m->plan;
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(b->device));
    // one slot's workspace under these costs: the maxima over the graphs that have queries (poa_multi_plan.hpp)
    MultiExactSlot slot;
    {
        MultiExactCosts xc;
        xc.x = costs->mismatch; xc.o = costs->gap_open; xc.e = costs->gap_extend;
        xc.queue_entries_per_cell = cfg ? cfg->queue_entries_per_cell : 0.f;
        std::string err;
        if (const int rc = multi_exact_slot(pl, xc, slot, err)) return fail(rc, std::string(who) + ": " + err);
    }
    const uint64_t slots = pl.exact_slots;
    if (b->n_queries && m->d_x_ws.n < slot.buffer_bytes(slots)) {
        // the buffer is re-allocated: nothing of an earlier run on this batch may still be in flight (prepare_exact's rule)
        if (b->ran) HIP_TRY(hipStreamSynchronize(b->last_stream));
        const hipError_t e = m->d_x_ws.alloc(slot.buffer_bytes(slots));
        if (e != hipSuccess)
            return fail(POA_ERR_OUT_OF_MEMORY, std::string("poa_multi_run_exact: the replay workspace does not fit (create the batch with a smaller workspace_bytes: fewer "
                                                           "queries per chunk, or lower queue_entries_per_cell): ") + hipGetErrorString(e));
    }
    m->x_slot = slot;
    RunFrame run;
    if (const int rc = run.open(b, "poa_multi_run_exact: call poa_multi_stats/fetch at least every 256 runs")) return rc;
    if (const int rc = run.begin(stream, pl.chunks.size())) return rc;
    const uint32_t hybrid = (cfg && cfg->mode == POA_MODE_HYBRID) ? 1u : 0u;
    b->last_mode = hybrid ? POA_MODE_HYBRID : POA_MODE_EXACT;
    b->prof_on = false;
    b->two_piece = false;
    set_layout(b, true, true, false);
    b->active_plan = 0;
    b->launches.clear();
    b->replays.clear();
    if (b->n_queries == 0) return run.end_empty(true);

    int lds_cap = 64 * 1024;
    (void)hipDeviceGetAttribute(&lds_cap, hipDeviceAttributeMaxSharedMemoryPerBlock, b->device);
    MultiExactLaunch xl;
    xl.graphs = m->d_exact.p;
    xl.tables = b->d_planes.p; xl.table_off = m->d_table_off.p;
    xl.hybrid = hybrid; xl.dense_flags = b->d_flags.p;
    xl.qseq = b->d_qseq.p; xl.qoff = b->d_qoff.p; xl.pitch = b->d_pitch.p;
    uint8_t* ws = m->d_x_ws.p;
    xl.reached = reinterpret_cast<uint64_t*>(ws + slot.off_reached(slots));
    xl.rsum = reinterpret_cast<uint64_t*>(ws + slot.off_rsum(slots));
    xl.reached_stride = slot.reached_stride; xl.rsum_stride = slot.rsum_stride;
    xl.wpn = slot.wpn; xl.swpn = slot.swpn;
    xl.stack = reinterpret_cast<ExStackEntry*>(ws + slot.off_stack(slots)); xl.stack_cap = slot.stack_cap;
    xl.chunks = reinterpret_cast<ExU4*>(ws + slot.off_pool(slots)); xl.chunk_cap = slot.pool_cap / BQ_CHUNK;
    if (const int* cv = T.ptr(POA_TUNE_WS_CHUNK_CAP)) { const int v = (*cv); if (v >= 1 && (uint32_t)v < xl.chunk_cap) xl.chunk_cap = (uint32_t)v; }
    xl.win = slot.win;
    xl.max_lanes = 32; xl.adapt_lanes = 4;   // replay_wave's defaults and overrides
    if (const int* lv = T.ptr(POA_TUNE_WS_LANES)) { const int v = (*lv); if (v >= 1 && v <= 63) xl.max_lanes = (uint32_t)v; }
    if (const int* av = T.ptr(POA_TUNE_WS_ADAPT)) { const int v = (*av); if (v >= 0 && v <= 63) xl.adapt_lanes = (uint32_t)v; }
    xl.C = ExactCosts{costs->mismatch, costs->gap_open, costs->gap_extend, cfg ? cfg->heuristic : POA_HEURISTIC_MINGAP, cfg ? cfg->pruning : 1u, 0, 0, 0, 0, 0, 0};
    xl.status = b->d_ex_status.p; xl.end_cell = b->d_ex_end.p; xl.counters = b->d_ex_counters.p;
    const uint64_t ring_b = 3ull * slot.win * 4;
    const bool want_lds = !(T.ptr(POA_TUNE_EXACT_LDS) && *T.ptr(POA_TUNE_EXACT_LDS) == 0) && !T.ptr(POA_TUNE_WS_RING_GLOBAL);
    const bool want_rec = !(T.ptr(POA_TUNE_WS_REC) && *T.ptr(POA_TUNE_WS_REC) == 0);

    for (const auto& ch : pl.chunks) {
        MultiDenseLaunch& ml = xl.D;
        ml.graphs = m->d_dense.p; ml.graph_of = m->d_graph_of.p;
        ml.first_query = ch.first; ml.n_queries = ch.count;
        ml.cost_x = costs->mismatch; ml.cost_o = costs->gap_open; ml.cost_e = costs->gap_extend;
        ml.spec_depth = 32; ml.code_fmt = 0;
        ml.carry = b->d_carry.p; ml.carry_off = m->d_carry_off.p;
        const uint32_t quads = ch.max_pitch <= 512 ? 1u : 2u;
        const dim3 grid((ch.count + 3) / 4), block(256);
        // 1. the dense kind's forward and walk launches
        const uint32_t strips = multi_dense_forward(ml, ch.max_pitch, grid, block, stream);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        hipLaunchKernelGGL(poa_traceback_multi_kernel, grid, block, 0, stream, ml);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        // 2. the replayed queries' tables, the chunk's statuses, counters, reached sets (and rings, where they are global)
        HIP_TRY(hipMemsetAsync(b->d_ex_status.p + ch.first, 0xFF, (size_t)ch.count * 4, stream));
        HIP_TRY(hipMemsetAsync(b->d_ex_counters.p + 4 * (size_t)ch.first, 0, (size_t)ch.count * 16, stream));
        hipLaunchKernelGGL(poa_fill_tables_multi_kernel, dim3(ch.count, 16), dim3(256), 0, stream, xl);
        HIP_TRY(hipGetLastError());
        if (slot.reached_stride) HIP_TRY(hipMemsetAsync(xl.reached, 0, (size_t)ch.count * slot.reached_stride * 8, stream));
        if (slot.rsum_stride) HIP_TRY(hipMemsetAsync(xl.rsum, 0, (size_t)ch.count * slot.rsum_stride * 8, stream));
        // 3. one replay launch.  The all-in-LDS instantiation when the chunk's largest graph, its records and the ring fit the
        // launch's LDS budget (replay_wave's: 80 KB for graph and ring, 150 KB with the records), else the generic-pointer one
        uint64_t g_lds = 0, g_rec = 0;
        for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
            const MultiExactBlock& xb = m->h_exact[pl.graph_of[i]];
            if (xb.empty) continue;
            g_lds = std::max<uint64_t>(g_lds, xb.graph_lds);
            g_rec = std::max<uint64_t>(g_rec, (uint64_t)xb.graph_lds + xb.rec_lds);
        }
        const bool lds_all = want_lds && g_lds + ring_b <= std::min<uint64_t>((uint64_t)lds_cap, 80u * 1024u);
        xl.stage_rec = (lds_all && want_rec && g_rec + ring_b <= std::min<uint64_t>((uint64_t)lds_cap, 150u * 1024u)) ? 1u : 0u;
        xl.ring_global = lds_all ? nullptr : reinterpret_cast<uint32_t*>(ws + slot.off_ring(slots));
        const uint32_t lds_bytes = lds_all ? (uint32_t)((xl.stage_rec ? g_rec : g_lds) + ring_b) : 0u;
        const void* kfn = lds_all ? reinterpret_cast<const void*>(poa_wsearch_multi_kernel<true>) : reinterpret_cast<const void*>(poa_wsearch_multi_kernel<false>);
        if (lds_bytes > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        if (lds_all) hipLaunchKernelGGL((poa_wsearch_multi_kernel<true>), dim3(ch.count), dim3(64), lds_bytes, stream, xl);
        else hipLaunchKernelGGL((poa_wsearch_multi_kernel<false>), dim3(ch.count), dim3(64), 0, stream, xl);
        HIP_TRY(hipGetLastError());
        // 4. one u32 walk launch over the replayed tables
        hipLaunchKernelGGL(poa_traceback_multi_exact_kernel, grid, block, 0, stream, xl);
        HIP_TRY(hipGetLastError());
        if (const int rc = run.mark()) return rc;
        // the record of poa_multi_last_launch: the dense kind's, with the replay kernel in the low two launch bits (1: all in LDS,
        // 2: generic pointers) and POA_LAUNCH_STRIPS on top
        b->launches.push_back(DenseChunkPlan{{POA_KERNEL_PACKED, quads, (lds_all ? 1u : 2u) | strips, 4u, ml.code_fmt, 64u, ml.spec_depth, ch.count}, -1, false, true, false});
        b->replays.push_back({{lds_all ? (uint32_t)POA_REPLAY_WAVE_LDS : (uint32_t)POA_REPLAY_WAVE_GENERIC, slot.win, 64u, 1u,
                               (lds_all ? POA_REPLAY_BIT_GRAPH_LDS : 0u) | (xl.stage_rec ? POA_REPLAY_BIT_REC_LDS : 0u) | (lds_all ? 0u : POA_REPLAY_BIT_RING_GLOBAL),
                               0u, ch.count, lds_bytes}});
    }
    return run.end_pairs();
}

int poa_multi_replay_info(poa_multi_t* m, uint32_t chunk, uint32_t out[8]) {
    if (!m || !out) return fail(POA_ERR_INVALID_ARG, "poa_multi_replay_info: null argument");
    if (!m->exact) return fail(POA_ERR_INVALID_ARG, "poa_multi_replay_info: the batch was not created by poa_multi_create_exact");
    if (!m->core.ran) return fail(POA_ERR_INVALID_ARG, "poa_multi_replay_info: poa_multi_run_exact has not been called");
    return poa_batch_replay_info(&m->core, chunk, out);
}

int poa_multi_fetch_search_counters(poa_multi_t* m, uint32_t* out) {
    if (!m || !out) return fail(POA_ERR_INVALID_ARG, "poa_multi_fetch_search_counters: null argument");
    if (!m->exact) return fail(POA_ERR_INVALID_ARG, "poa_multi_fetch_search_counters: the batch was not created by poa_multi_create_exact");
    if (!m->core.ran) return fail(POA_ERR_INVALID_ARG, "poa_multi_fetch_search_counters: poa_multi_run_exact has not been called");
    return poa_batch_fetch_search_counters(&m->core, out);
}

int poa_align_multi_exact(const poa_graph_t* const* graphs, uint32_t n_graphs, const uint64_t* graph_qoff, const poa_costs_t* costs,
                          const poa_config_t* cfg, const uint8_t* qseq, const uint64_t* qoff, uint32_t* score, poa_aln_pair_t* pairs,
                          uint64_t* pair_off, uint64_t pair_capacity, uint32_t* flags, poa_stats_t* stats, int device) {
    if (!costs) return fail(POA_ERR_INVALID_ARG, "poa_align_multi_exact: null argument");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return multi_one_shot([&](poa_multi_t** m) { return poa_multi_create_exact(graphs, n_graphs, graph_qoff, device, qseq, qoff, cfg, 0, m); },
                          [&](poa_multi_t* m) { return poa_multi_run_exact(m, costs, cfg, nullptr); }, score, pairs, pair_off, pair_capacity, flags, stats);
}

}  // extern "C"


// ---- score set (poa_scoreset.hpp, poa_scoreset_plan.hpp) ---------------------------------------------------------------------
// Score-only runs over (query, graph) pairs of many graphs.  The set's result buffers, events and statistics are those of a
// score-mode poa_batch (`core`, no graph of its own, one "query" per pair); what is new lies beside it: the plan, the
// concatenated tables of all graphs, one parameter block per graph and the class lists of the three run variants.
struct poa_scoreset {
    poa_batch core;
    ScoreSetPlan plan;
    std::vector<uint64_t> ub_open, ub_extend;   // per graph with pairs: the u16 bound is open * ub_open + extend * ub_extend
    DevBuf<uint32_t> d_slot, d_pred_slot, d_pair_graph, d_pair_query, d_carry_off, d_class_list[SS_N_VARIANTS];
    DevBuf<ScoreGraphParams> d_params;
    // capped runs (poa_scoreset_run_capped): the device buffers and the pinned staging area are made by the set's first one
    std::vector<uint8_t> cut;          // [n_rows_total] SweepRows::cut of every graph, concatenated like the row tables
    DevBuf<uint32_t> d_cap, d_swept, d_check_rows;
    uint32_t* h_stage = nullptr;       // pinned: [max(n_pairs, n_queries)] caps or limits, then [n_rows_total] check rows
    hipEvent_t stage_done = nullptr;   // the copies out of h_stage of the last capped run
    bool stage_busy = false;
    uint32_t check_stride = 0;         // the stride d_check_rows was built for (0: not built)
    bool last_capped = false;          // the last run wrote d_swept
    // best-of runs (poa_scoreset_run_best): made by the set's first one, with the capped runs' buffers if they are not there yet
    DevBuf<unsigned long long> d_best_word;
    DevBuf<uint32_t> d_limit, d_query_off, d_query_pairs, d_best_list[SS_N_VARIANTS];
    DevBuf<ScoreSetBest> d_best;
    bool last_best = false;            // the last run was a best-of run: d_best holds its result
    ~poa_scoreset() {
        if (h_stage) (void)hipHostFree(h_stage);
        if (stage_done) (void)hipEventDestroy(stage_done);
    }
};

namespace {
int scoreset_mode_check(const poa_config_t* cfg, const char* who) {
    if (cfg && cfg->mode != POA_MODE_SCORE)
        return fail(POA_ERR_UNSUPPORTED, std::string(who) + ": a score set runs in POA_MODE_SCORE only");
    if (cfg && cfg->span != POA_SPAN_GLOBAL)
        return fail(POA_ERR_UNSUPPORTED, std::string(who) + ": score-only mode is Global: an ends-free result is defined by the reference's search");
    return POA_OK;
}

int scoreset_plan_of(const poa_graph_t* const* graphs, uint32_t n_graphs, uint32_t n_queries, const uint64_t* qoff, uint64_t n_pairs,
                     const uint32_t* pair_query, const uint32_t* pair_graph, uint64_t workspace_bytes, ScoreSetPlan& plan, const char* who) {
    if (!qoff || (n_graphs && !graphs)) return fail(POA_ERR_INVALID_ARG, std::string(who) + ": null argument");
    std::vector<ScoreSetGraphIn> in(n_graphs);
    for (uint32_t g = 0; g < n_graphs; ++g) {
        if (!graphs[g]) return fail(POA_ERR_INVALID_ARG, std::string(who) + ": null graph");
        in[g] = ScoreSetGraphIn{&graphs[g]->g, &graphs[g]->sweep};
    }
    std::string err;
    const int rc = build_scoreset_plan(in.data(), n_graphs, n_queries, qoff, n_pairs, pair_query, pair_graph, workspace_bytes, plan, err);
    if (rc != 0) return fail(rc, std::string(who) + ": " + err);
    return POA_OK;
}

// words at the front of the staging area: the caps of a capped run or the limits of a best-of run
size_t scoreset_stage_front(const poa_scoreset* s) { return std::max<size_t>(s->core.n_queries, s->plan.n_queries); }

// what a capped run needs beyond the set's own buffers; made once
int scoreset_cap_buffers(poa_scoreset* s) {
    const size_t n = s->core.n_queries, n_rows = s->plan.n_rows_total;
    if (!s->d_cap.p) HIP_TRY(s->d_cap.alloc(std::max<size_t>(n, 1)));
    if (!s->d_swept.p) HIP_TRY(s->d_swept.alloc(std::max<size_t>(n, 1)));
    if (!s->d_check_rows.p) HIP_TRY(s->d_check_rows.alloc(std::max<size_t>(n_rows, 1)));
    if (!s->h_stage) HIP_TRY(hipHostMalloc((void**)&s->h_stage, (scoreset_stage_front(s) + n_rows + 1) * sizeof(uint32_t), hipHostMallocDefault));
    if (!s->stage_done) HIP_TRY(hipEventCreateWithFlags(&s->stage_done, hipEventDisableTiming));
    return POA_OK;
}

// the caps of this run (dst = d_cap, n = n_pairs) or the limits of a best-of run (dst = d_limit, n = n_queries; cap null:
// nothing to copy) and, if the stride changed, the check rows: through the pinned staging area, on the run's stream
int scoreset_cap_upload(poa_scoreset* s, const uint32_t* cap, uint32_t* dst, size_t n, uint32_t stride, hipStream_t stream) {
    if (s->stage_busy) HIP_TRY(hipEventSynchronize(s->stage_done));   // the previous capped run's copies, not its kernels
    s->stage_busy = false;
    if (cap && n) {
        std::memcpy(s->h_stage, cap, n * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(dst, s->h_stage, n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    }
    if (s->check_stride != stride && s->plan.n_rows_total) {
        uint32_t* h_check = s->h_stage + scoreset_stage_front(s);
        std::fill(h_check, h_check + s->plan.n_rows_total, 0xFFFFFFFFu);
        std::vector<uint32_t> rows;
        for (uint32_t g = 0; g < s->plan.graphs.size(); ++g) {
            const ScoreSetGraphPlan& gp = s->plan.graphs[g];
            if (gp.table_of != g) continue;
            build_sweep_checks(s->cut.data() + gp.row_base, gp.n_rows, stride, rows);   // fewer than n_rows: a 0xFFFFFFFF follows
            std::copy(rows.begin(), rows.end(), h_check + gp.row_base);
        }
        HIP_TRY(hipMemcpyAsync(s->d_check_rows.p, h_check, s->plan.n_rows_total * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        s->check_stride = stride;
    }
    HIP_TRY(hipEventRecord(s->stage_done, stream));
    s->stage_busy = true;
    return POA_OK;
}

// what a best-of run needs beyond the capped runs' buffers; made once: the best words, limits and records per query, the
// query-to-pairs lists and the best-of launch orders (host plan: build_scoreset_best_order), uploaded here
int scoreset_best_buffers(poa_scoreset* s) {
    if (s->d_best.p) return POA_OK;
    ScoreSetPlan& pl = s->plan;
    const size_t n = pl.n_pairs, nq = pl.n_queries;
    build_scoreset_best_order(pl);
    HIP_TRY(s->d_best_word.alloc(std::max<size_t>(nq, 1)));
    HIP_TRY(s->d_limit.alloc(std::max<size_t>(nq, 1)));
    HIP_TRY(s->d_query_off.alloc(nq + 1));
    HIP_TRY(s->d_query_pairs.alloc(std::max<size_t>(n, 1)));
    for (uint32_t v = 0; v < SS_N_VARIANTS; ++v) HIP_TRY(s->d_best_list[v].alloc(std::max<size_t>(n, 1)));
    HIP_TRY(hipMemcpy(s->d_query_off.p, pl.query_off.data(), (nq + 1) * 4, hipMemcpyHostToDevice));
    if (n) {
        HIP_TRY(hipMemcpy(s->d_query_pairs.p, pl.query_pairs.data(), n * 4, hipMemcpyHostToDevice));
        for (uint32_t v = 0; v < SS_N_VARIANTS; ++v)
            HIP_TRY(hipMemcpy(s->d_best_list[v].p, pl.best_list[v].data(), n * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(s->d_best.alloc(std::max<size_t>(nq, 1)));   // last: its presence says the rest is there
    return POA_OK;
}

struct ScoreSetBestArgs {
    uint32_t slack;
    const uint32_t* limit;   // [n_queries] or null
};

// one sweep launch per chunk and non-empty kernel class, nothing else.  Costs are 32-bit, as in run_sweep.
// cap: nullptr, or the caps of a capped run in pair order (the capped kernels, which also write the swept-row counts).
// best: nullptr, or the slack and limits of a best-of run (kernels of their own again, between an init and a finalize launch).
int scoreset_run(poa_scoreset* s, uint32_t cost_x, uint32_t cost_o, uint32_t cost_e, const poa_config_t* cfg, hipStream_t stream, const char* who,
                 const uint32_t* cap = nullptr, const ScoreSetBestArgs* best = nullptr) {
    const TuneView T(cfg);
    poa_batch* b = &s->core;
    HIP_TRY(hipSetDevice(b->device));
    RunFrame run;
    if (const int rc = run.open(b, std::string(who) + ": call poa_scoreset_stats/fetch at least every 256 runs")) return rc;
    uint32_t cap_stride = SWEEP_CHECK_STRIDE;
    if (cap || best) {
        if (const int* sv = T.ptr(POA_TUNE_CAP_STRIDE)) { if ((*sv) > 0) cap_stride = (uint32_t)(*sv); }
        if (const int rc = scoreset_cap_buffers(s)) return rc;
    }
    if (best) {
        try {
            if (const int rc = scoreset_best_buffers(s)) return rc;
        } catch (const std::bad_alloc&) { return fail(POA_ERR_OUT_OF_MEMORY, std::string(who) + ": host allocation failed"); }
    }
    // u16 cells only if every graph's own bound (the longest query paired with it and its shortest path) allows them
    const bool narrow = !planes32(T) && all_graphs_u16(s->ub_open, s->ub_extend, cost_o, cost_e);
    bool want_px = true;
    if (const int* xv = T.ptr(POA_TUNE_PX)) want_px = (*xv) != 0;
    const ScoreSetPlan& pl = s->plan;
    const uint32_t variant = narrow ? (want_px ? SS_VAR_U16_PX : SS_VAR_U16) : SS_VAR_U32;
    if (const int rc = run.begin(stream, pl.chunks.size())) return rc;
    b->last_mode = POA_MODE_SCORE;
    b->two_piece = false;
    set_layout(b, narrow);
    b->active_plan = 0;
    s->last_capped = cap != nullptr || best != nullptr;
    s->last_best = best != nullptr;
    const dim3 qgrid((pl.n_queries + 255) / 256), qblock(256);
    auto finalize = [&]() -> int {   // (best) one record per query from its best word and the per-pair results
        if (!pl.n_queries) return POA_OK;
        hipLaunchKernelGGL(poa_scoreset_best_finalize_kernel, qgrid, qblock, 0, stream, s->d_best_word.p, s->d_limit.p, best->slack,
                           s->d_query_off.p, s->d_query_pairs.p, b->d_score.p, b->d_flags.p, s->d_best.p, pl.n_queries);
        HIP_TRY(hipGetLastError());
        return POA_OK;
    };
    if (best) {
        try {
            if (const int rc = scoreset_cap_upload(s, best->limit, s->d_limit.p, pl.n_queries, cap_stride, stream)) return rc;
        } catch (const std::bad_alloc&) { return fail(POA_ERR_OUT_OF_MEMORY, std::string(who) + ": host allocation failed"); }
        if (pl.n_queries) {
            hipLaunchKernelGGL(poa_scoreset_best_init_kernel, qgrid, qblock, 0, stream, s->d_best_word.p, s->d_limit.p, pl.n_queries,
                               best->limit ? 1u : 0u);
            HIP_TRY(hipGetLastError());
        }
    }
    if (b->n_queries == 0) {
        if (best) { if (const int rc = finalize()) return rc; }
        return run.end_empty(false);
    }
    if (cap) {
        try {
            if (const int rc = scoreset_cap_upload(s, cap, s->d_cap.p, b->n_queries, cap_stride, stream)) return rc;
        } catch (const std::bad_alloc&) { return fail(POA_ERR_OUT_OF_MEMORY, std::string(who) + ": host allocation failed"); }
    }
    // a best-of run launches from the best-of order of the same (chunk, class) ranges
    const bool pair_order = cfg && (cfg->flags & POA_CFG_BEST_PAIR_ORDER);
    const uint32_t* d_list = best && !pair_order ? s->d_best_list[variant].p : s->d_class_list[variant].p;
    // slot bytes stored: kept rows x 2 planes x (1024 two-byte cells in the packed kernel's register layout, else the pitch)
    b->sweep_bytes_written = variant == SS_VAR_U16_PX ? 2ull * (pl.slotted_px * 2048ull + pl.slotted_pitch * 2ull)
                                                      : 2ull * pl.slotted_pitch_all * (narrow ? 2ull : 4ull);
    for (const auto& ch : pl.chunks) {
        ScoreSetLaunch sl;
        sl.graphs = s->d_params.p; sl.pair_graph = s->d_pair_graph.p; sl.pair_query = s->d_pair_query.p;
        sl.pitch = b->d_pitch.p; sl.region_off = b->plan[0].d_off.p; sl.carry_off = s->d_carry_off.p;
        sl.qseq = b->d_qseq.p; sl.qoff = b->d_qoff.p; sl.planes = b->d_planes.p; sl.carry = b->d_carry.p;
        sl.cost_x = cost_x; sl.cost_oe = cost_o + cost_e; sl.cost_e = cost_e;
        for (uint32_t c = 0; c < SS_N_CLASSES; ++c) {
            const uint32_t begin = ch.class_begin[variant][c], count = ch.class_begin[variant][c + 1] - begin;
            if (!count) continue;
            sl.list = d_list + begin; sl.n = count;
            const dim3 grid((count + 3) / 4), block(256);
            if (best) {
                const ScoreSetBestLaunch bl{sl, s->d_best_word.p, s->d_limit.p, best->slack, s->d_swept.p, s->d_check_rows.p, b->d_rows.p};
                if (c == SS_CLASS_PX) hipLaunchKernelGGL(poa_scoreset_sweep_px_best_kernel, grid, block, 0, stream, bl);
                else if (narrow) {
                    if (c == SS_CLASS_Q1) hipLaunchKernelGGL((poa_scoreset_sweep_best_kernel<1, uint16_t>), grid, block, 0, stream, bl);
                    else hipLaunchKernelGGL((poa_scoreset_sweep_best_kernel<2, uint16_t>), grid, block, 0, stream, bl);
                } else {
                    if (c == SS_CLASS_Q1) hipLaunchKernelGGL((poa_scoreset_sweep_best_kernel<1, uint32_t>), grid, block, 0, stream, bl);
                    else if (c == SS_CLASS_Q2) hipLaunchKernelGGL((poa_scoreset_sweep_best_kernel<2, uint32_t>), grid, block, 0, stream, bl);
                    else hipLaunchKernelGGL((poa_scoreset_sweep_best_kernel<4, uint32_t>), grid, block, 0, stream, bl);
                }
            } else if (cap) {
                const ScoreSetCapLaunch cl{sl, s->d_cap.p, s->d_swept.p, s->d_check_rows.p, b->d_rows.p};
                if (c == SS_CLASS_PX) hipLaunchKernelGGL(poa_scoreset_sweep_px_capped_kernel, grid, block, 0, stream, cl);
                else if (narrow) {
                    if (c == SS_CLASS_Q1) hipLaunchKernelGGL((poa_scoreset_sweep_capped_kernel<1, uint16_t>), grid, block, 0, stream, cl);
                    else hipLaunchKernelGGL((poa_scoreset_sweep_capped_kernel<2, uint16_t>), grid, block, 0, stream, cl);
                } else {
                    if (c == SS_CLASS_Q1) hipLaunchKernelGGL((poa_scoreset_sweep_capped_kernel<1, uint32_t>), grid, block, 0, stream, cl);
                    else if (c == SS_CLASS_Q2) hipLaunchKernelGGL((poa_scoreset_sweep_capped_kernel<2, uint32_t>), grid, block, 0, stream, cl);
                    else hipLaunchKernelGGL((poa_scoreset_sweep_capped_kernel<4, uint32_t>), grid, block, 0, stream, cl);
                }
            } else if (c == SS_CLASS_PX) hipLaunchKernelGGL(poa_scoreset_sweep_px_kernel, grid, block, 0, stream, sl);
            else if (narrow) {
                if (c == SS_CLASS_Q1) hipLaunchKernelGGL((poa_scoreset_sweep_kernel<1, uint16_t>), grid, block, 0, stream, sl);
                else hipLaunchKernelGGL((poa_scoreset_sweep_kernel<2, uint16_t>), grid, block, 0, stream, sl);
            } else {
                if (c == SS_CLASS_Q1) hipLaunchKernelGGL((poa_scoreset_sweep_kernel<1, uint32_t>), grid, block, 0, stream, sl);
                else if (c == SS_CLASS_Q2) hipLaunchKernelGGL((poa_scoreset_sweep_kernel<2, uint32_t>), grid, block, 0, stream, sl);
                else hipLaunchKernelGGL((poa_scoreset_sweep_kernel<4, uint32_t>), grid, block, 0, stream, sl);
            }
            HIP_TRY(hipGetLastError());
        }
        // (the finalize launch in front of the last chunk's marks: poa_stats_t counts it with the sweep)
        if (best && &ch == &pl.chunks.back()) { if (const int rc = finalize()) return rc; }
        if (const int rc = run.mark(3)) return rc;
    }
    return run.end();
}

// poa_scoreset_create behind the null check of `out`
int scoreset_create_impl(const poa_graph_t* const* graphs, uint32_t n_graphs, int device, uint32_t n_queries, const uint8_t* qseq,
                         const uint64_t* qoff, uint64_t n_pairs, const uint32_t* pair_query, const uint32_t* pair_graph,
                         const poa_config_t* cfg, uint64_t workspace_bytes, poa_scoreset_t** out) {
    CreateFrame frame{"poa_scoreset_create"};
    if (const int rc = scoreset_mode_check(cfg, "poa_scoreset_create")) return rc;
    std::unique_ptr<poa_scoreset> s(new (std::nothrow) poa_scoreset);
    if (!s) return fail(POA_ERR_OUT_OF_MEMORY, "host allocation failed");
    ScoreSetPlan& pl = s->plan;
    auto plan_of = [&](uint64_t ws, ScoreSetPlan& plan) {
        return scoreset_plan_of(graphs, n_graphs, n_queries, qoff, n_pairs, pair_query, pair_graph, ws, plan, "poa_scoreset_create");
    };
    // a first plan without a cap: the argument checks (no device needed) and the footprint the cap is chosen from
    if (const int rc = plan_of(0, pl)) return rc;
    const uint32_t n = pl.n_pairs;
    if (n_queries && qoff[n_queries] && !qseq) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_create: null argument");
    if (const int rc = frame.open(device)) return rc;
    const uint64_t fixed = (uint64_t)n * 64 + (uint64_t)n_queries * 8 + qoff[n_queries] + (64ull << 20) + pl.max_carry_words * 4 +
                           (pl.n_rows_total + pl.n_edges_total) * 32;
    if (const int rc = frame.plan_capped(pl, workspace_bytes, fixed, pl.largest_pair_bytes,
                                         "the slot footprint of the largest pair does not fit in device memory", plan_of)) return rc;

    // the core batch: one "query" per pair — results, events, statistics
    poa_batch* b = &s->core;
    frame.fill_core(b, pl, n, pl.bytes_total);
    b->sweep = true; b->last_mode = POA_MODE_SCORE;

    // concatenated tables, one copy per distinct handle
    std::vector<RowMeta> h_rows(pl.n_rows_total);
    std::vector<uint32_t> h_slot(pl.n_rows_total), h_pred_rows(pl.n_edges_total), h_pred_slot(pl.n_edges_total);
    s->cut.assign(pl.n_rows_total, 0);
    using GP = ScoreSetGraphPlan;
    concat_tables(s->cut, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->sweep.cut; });
    concat_tables(h_rows, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->g.rows; });
    concat_tables(h_slot, pl.graphs, &GP::row_base, [&](uint32_t g) -> auto& { return graphs[g]->sweep.slot; });
    concat_tables(h_pred_rows, pl.graphs, &GP::edge_base, [&](uint32_t g) -> auto& { return graphs[g]->g.pred_rows; });
    concat_tables(h_pred_slot, pl.graphs, &GP::edge_base, [&](uint32_t g) -> auto& { return graphs[g]->sweep.pred_slot; });
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const ScoreSetGraphPlan& gp = pl.graphs[g];
        if (!gp.n_pairs) continue;
        note_graph_bound(s->ub_open, s->ub_extend, gp.max_len, graphs[g]->g);
        b->max_len = std::max(b->max_len, gp.max_len);
    }

    HIP_TRY(CreateFrame::alloc_each(pl.n_rows_total, b->d_rows, s->d_slot));
    HIP_TRY(CreateFrame::alloc_each(pl.n_edges_total, b->d_pred_rows, s->d_pred_slot));
    HIP_TRY(CreateFrame::alloc_each(n, s->d_pair_graph, s->d_pair_query, s->d_carry_off));
    for (auto& list : s->d_class_list) HIP_TRY(CreateFrame::alloc_each(n, list));
    HIP_TRY(CreateFrame::alloc_each(n_graphs, s->d_params));
    if (const int rc = frame.alloc_results(b, qoff[n_queries], n_queries, n, false, 0)) return rc;
    HIP_TRY(CreateFrame::alloc_each(pl.max_carry_words, b->d_carry));
    if (const int rc = frame.acquire_planes(b, pl.workspace_bytes, true, "score-set workspace")) return rc;

    std::vector<ScoreGraphParams> h_params(n_graphs);
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const ScoreSetGraphPlan& gp = pl.graphs[g];
        ScoreGraphParams& sp = h_params[g];
        std::memset(&sp, 0, sizeof(sp));
        SweepParams& kp = sp.P;
        kp.rows = b->d_rows.p + gp.row_base; kp.slot = s->d_slot.p + gp.row_base;
        kp.pred_rows = b->d_pred_rows.p + gp.edge_base; kp.pred_slot = s->d_pred_slot.p + gp.edge_base;
        kp.n_rows = gp.n_rows; kp.n_slots = std::max<uint32_t>(gp.n_slots, 1u);
        kp.qseq = b->d_qseq.p; kp.qoff = b->d_qoff.p; kp.pitch = b->d_pitch.p; kp.plane_off = b->plan[0].d_off.p;
        kp.planes = b->d_planes.p; kp.carry = b->d_carry.p;
        kp.score = b->d_score.p; kp.flags = b->d_flags.p;
        sp.empty = gp.empty ? 1u : 0u;
    }

    if (const int rc = frame.begin_upload()) return rc;
    HIP_TRY(CreateFrame::upload(b->d_rows, h_rows));
    HIP_TRY(CreateFrame::upload(b->d_pred_rows, h_pred_rows));
    HIP_TRY(CreateFrame::upload(s->d_slot, h_slot));
    HIP_TRY(CreateFrame::upload(s->d_pred_slot, h_pred_slot));
    HIP_TRY(CreateFrame::upload(s->d_params, h_params));
    HIP_TRY(CreateFrame::upload(s->d_pair_graph.p, pl.pair_graph.data(), (size_t)n * 4));
    HIP_TRY(CreateFrame::upload(s->d_pair_query.p, pl.pair_query.data(), (size_t)n * 4));
    HIP_TRY(CreateFrame::upload(s->d_carry_off.p, pl.carry_off.data(), (size_t)n * 4));
    for (uint32_t v = 0; v < SS_N_VARIANTS; ++v) HIP_TRY(CreateFrame::upload(s->d_class_list[v].p, pl.class_list[v].data(), (size_t)n * 4));
    if (const int rc = frame.upload_queries(b, qseq, qoff, n_queries, nullptr, pl.pitch.data(), pl.region_off.data(), n)) return rc;
    if (const int rc = frame.end_upload(b)) return rc;

    *out = s.release();
    return POA_OK;
}
}  // namespace

extern "C" {

int poa_scoreset_footprint(const poa_graph_t* const* graphs, uint32_t n_graphs, uint32_t n_queries, const uint64_t* qoff, uint64_t n_pairs,
                           const uint32_t* pair_query, const uint32_t* pair_graph, const poa_config_t* cfg, uint64_t* bytes,
                           uint64_t* largest_pair_bytes) {
    if (!bytes && !largest_pair_bytes) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_footprint: null argument");
    if (const int rc = scoreset_mode_check(cfg, "poa_scoreset_footprint")) return rc;
    return CreateFrame::guarded("poa_scoreset_footprint: host allocation failed", [&]() -> int {
        ScoreSetPlan plan;
        if (const int rc = scoreset_plan_of(graphs, n_graphs, n_queries, qoff, n_pairs, pair_query, pair_graph, 0, plan, "poa_scoreset_footprint")) return rc;
        if (bytes) *bytes = plan.bytes_total;
        if (largest_pair_bytes) *largest_pair_bytes = plan.largest_pair_bytes;
        return POA_OK;
    });
}

int poa_scoreset_create(const poa_graph_t* const* graphs, uint32_t n_graphs, int device, uint32_t n_queries, const uint8_t* qseq,
                        const uint64_t* qoff, uint64_t n_pairs, const uint32_t* pair_query, const uint32_t* pair_graph,
                        const poa_config_t* cfg, uint64_t workspace_bytes, poa_scoreset_t** out) {
    return CreateFrame::enter("poa_scoreset_create", out, "poa_scoreset_create: host allocation failed", [&] {
        return scoreset_create_impl(graphs, n_graphs, device, n_queries, qseq, qoff, n_pairs, pair_query, pair_graph, cfg, workspace_bytes, out);
    });
}

int poa_scoreset_run(poa_scoreset_t* s, const poa_costs_t* costs, const poa_config_t* cfg, void* stream) {
    if (!s || !costs) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_run: null argument");
    const int rc = scoreset_mode_check(cfg, "poa_scoreset_run");
    if (rc != POA_OK) return rc;
    return scoreset_run(s, costs->mismatch, costs->gap_open, costs->gap_extend, cfg, (hipStream_t)stream, "poa_scoreset_run");
}

int poa_scoreset_run_2piece(poa_scoreset_t* s, const poa_costs2_t* costs, const poa_config_t* cfg, void* stream) {
    if (!s || !costs) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_run_2piece: null argument");
    const int rc = scoreset_mode_check(cfg, "poa_scoreset_run_2piece");
    if (rc != POA_OK) return rc;
    if (costs->gap_extend1 < costs->gap_extend2)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    // the two-piece optimum is the one-piece optimum under open' = open1 + extend1 - extend2, extend' = extend2
    return scoreset_run(s, costs->mismatch, (uint32_t)costs->gap_open1 + costs->gap_extend1 - costs->gap_extend2, costs->gap_extend2, cfg,
                        (hipStream_t)stream, "poa_scoreset_run_2piece");
}

int poa_scoreset_run_capped(poa_scoreset_t* s, const poa_costs_t* costs, const poa_config_t* cfg, const uint32_t* cap, void* stream) {
    if (!s || !costs || !cap) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_run_capped: null argument");
    const int rc = scoreset_mode_check(cfg, "poa_scoreset_run_capped");
    if (rc != POA_OK) return rc;
    return scoreset_run(s, costs->mismatch, costs->gap_open, costs->gap_extend, cfg, (hipStream_t)stream, "poa_scoreset_run_capped", cap);
}

int poa_scoreset_run_2piece_capped(poa_scoreset_t* s, const poa_costs2_t* costs, const poa_config_t* cfg, const uint32_t* cap, void* stream) {
    if (!s || !costs || !cap) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_run_2piece_capped: null argument");
    const int rc = scoreset_mode_check(cfg, "poa_scoreset_run_2piece_capped");
    if (rc != POA_OK) return rc;
    if (costs->gap_extend1 < costs->gap_extend2)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    // the cap is compared with the score under the reduced costs, which is the two-piece score
    return scoreset_run(s, costs->mismatch, (uint32_t)costs->gap_open1 + costs->gap_extend1 - costs->gap_extend2, costs->gap_extend2, cfg,
                        (hipStream_t)stream, "poa_scoreset_run_2piece_capped", cap);
}

int poa_scoreset_run_best(poa_scoreset_t* s, const poa_costs_t* costs, const poa_config_t* cfg, uint32_t slack, const uint32_t* limit,
                          void* stream) {
    if (!s || !costs) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_run_best: null argument");
    const int rc = scoreset_mode_check(cfg, "poa_scoreset_run_best");
    if (rc != POA_OK) return rc;
    const ScoreSetBestArgs best{slack, limit};
    return scoreset_run(s, costs->mismatch, costs->gap_open, costs->gap_extend, cfg, (hipStream_t)stream, "poa_scoreset_run_best", nullptr, &best);
}

int poa_scoreset_run_2piece_best(poa_scoreset_t* s, const poa_costs2_t* costs, const poa_config_t* cfg, uint32_t slack, const uint32_t* limit,
                                 void* stream) {
    if (!s || !costs) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_run_2piece_best: null argument");
    const int rc = scoreset_mode_check(cfg, "poa_scoreset_run_2piece_best");
    if (rc != POA_OK) return rc;
    if (costs->gap_extend1 < costs->gap_extend2)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    // bests, slack and limits are compared with the score under the reduced costs, which is the two-piece score
    const ScoreSetBestArgs best{slack, limit};
    return scoreset_run(s, costs->mismatch, (uint32_t)costs->gap_open1 + costs->gap_extend1 - costs->gap_extend2, costs->gap_extend2, cfg,
                        (hipStream_t)stream, "poa_scoreset_run_2piece_best", nullptr, &best);
}

int poa_scoreset_fetch_best(poa_scoreset_t* s, poa_best_t* best) {
    if (!s || !best) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_fetch_best: null argument");
    poa_batch* b = &s->core;
    if (!b->ran || !s->last_best) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_fetch_best: the last run was not a best-of run (poa_scoreset_run_best)");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    static_assert(sizeof(poa_best_t) == sizeof(ScoreSetBest), "poa_best_t is the device record");
    if (s->plan.n_queries) HIP_TRY(hipMemcpy(best, s->d_best.p, (size_t)s->plan.n_queries * sizeof(poa_best_t), hipMemcpyDeviceToHost));
    return POA_OK;
}

int poa_scoreset_device_best(poa_scoreset_t* s, void** best) {
    if (!s || !best) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_device_best: null argument");
    if (!s->d_best.p) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_device_best: poa_scoreset_run_best has not been called");
    *best = s->d_best.p;
    return POA_OK;
}

int poa_scoreset_fetch_swept(poa_scoreset_t* s, uint32_t* swept) {
    if (!s || !swept) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_fetch_swept: null argument");
    poa_batch* b = &s->core;
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_fetch_swept: poa_scoreset_run has not been called");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    const uint32_t n = b->n_queries;
    if (!n) return POA_OK;
    if (s->last_capped) {
        HIP_TRY(hipMemcpy(swept, s->d_swept.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    } else {
        // an uncapped run executes every row of every strip (strips of SCORESET_STRIP_COLUMNS columns: only a pair wider than
        // that has more than one, whatever its kernel class)
        const ScoreSetPlan& pl = s->plan;
        for (uint32_t p = 0; p < n; ++p) {
            const ScoreSetGraphPlan& gp = pl.graphs[pl.pair_graph[p]];
            swept[p] = gp.empty ? 0u : gp.n_rows * ((pl.pitch[p] + SCORESET_STRIP_COLUMNS - 1) / SCORESET_STRIP_COLUMNS);
        }
    }
    return POA_OK;
}

int poa_scoreset_fetch(poa_scoreset_t* s, uint32_t* score, uint32_t* flags, poa_stats_t* stats) {
    if (!s) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_fetch: null set");
    poa_batch* b = &s->core;
    if (!b->ran) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_fetch: poa_scoreset_run has not been called");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    const uint32_t n = b->n_queries;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t n_flagged = 0;
    if (n) {
        if (score) HIP_TRY(hipMemcpy(score, b->d_score.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> fl_local;
        uint32_t* fl = flags;
        if (!fl && stats) { fl_local.resize(n); fl = fl_local.data(); }
        if (fl) HIP_TRY(hipMemcpy(fl, b->d_flags.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (fl) for (uint32_t i = 0; i < n; ++i) n_flagged += fl[i] != 0;
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        collect_stats(b, stats);
        stats->n_flagged = n_flagged;
        stats->ms_d2h = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();   // blocking copies: host time
    }
    return POA_OK;
}

int poa_scoreset_stats(poa_scoreset_t* s, poa_stats_t* stats) {
    if (!s || !stats) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_stats: null argument");
    return poa_batch_stats(&s->core, stats);
}

int poa_scoreset_device_results(poa_scoreset_t* s, void** score, void** flags) {
    if (!s) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_device_results: null set");
    return poa_batch_device_results(&s->core, score, flags, nullptr, nullptr);
}

int poa_scoreset_workspace_bytes(poa_scoreset_t* s, uint64_t* bytes) {
    if (!s || !bytes) return fail(POA_ERR_INVALID_ARG, "poa_scoreset_workspace_bytes: null argument");
    *bytes = s->core.d_planes.bytes;
    return POA_OK;
}

void poa_scoreset_destroy(poa_scoreset_t* s) {
    if (!s) return;
    (void)hipSetDevice(s->core.device);
    if (s->core.ran) (void)hipStreamSynchronize(s->core.last_stream);  // the workspace may be handed to another batch next
    delete s;
}

// one-shot: exactly one of costs / costs2 is set
static int score_pairs_impl(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs_t* costs, const poa_costs2_t* costs2,
                            const poa_config_t* cfg, uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs,
                            const uint32_t* pair_query, const uint32_t* pair_graph, uint32_t* score, uint32_t* flags, poa_stats_t* stats,
                            int device) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    poa_scoreset_t* s = nullptr;
    int rc = poa_scoreset_create(graphs, n_graphs, device, n_queries, qseq, qoff, n_pairs, pair_query, pair_graph, cfg, 0, &s);
    if (rc != POA_OK) return rc;
    rc = costs ? poa_scoreset_run(s, costs, cfg, nullptr) : poa_scoreset_run_2piece(s, costs2, cfg, nullptr);
    if (rc == POA_OK) rc = poa_scoreset_fetch(s, score, flags, stats);
    poa_scoreset_destroy(s);
    return rc;
}

// one-shot best-of: exactly one of costs / costs2 is set
static int score_best_impl(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs_t* costs, const poa_costs2_t* costs2,
                           const poa_config_t* cfg, uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs,
                           const uint32_t* pair_query, const uint32_t* pair_graph, uint32_t slack, const uint32_t* limit, poa_best_t* best,
                           uint32_t* score, uint32_t* flags, poa_stats_t* stats, int device) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    poa_scoreset_t* s = nullptr;
    int rc = poa_scoreset_create(graphs, n_graphs, device, n_queries, qseq, qoff, n_pairs, pair_query, pair_graph, cfg, 0, &s);
    if (rc != POA_OK) return rc;
    rc = costs ? poa_scoreset_run_best(s, costs, cfg, slack, limit, nullptr) : poa_scoreset_run_2piece_best(s, costs2, cfg, slack, limit, nullptr);
    if (rc == POA_OK) rc = poa_scoreset_fetch_best(s, best);
    if (rc == POA_OK && (score || flags || stats)) rc = poa_scoreset_fetch(s, score, flags, stats);
    poa_scoreset_destroy(s);
    return rc;
}

int poa_score_best(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs_t* costs, const poa_config_t* cfg,
                   uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs, const uint32_t* pair_query,
                   const uint32_t* pair_graph, uint32_t slack, const uint32_t* limit, poa_best_t* best, uint32_t* score,
                   uint32_t* flags, poa_stats_t* stats, int device) {
    if (!costs || !best) return fail(POA_ERR_INVALID_ARG, "poa_score_best: null argument");
    return score_best_impl(graphs, n_graphs, costs, nullptr, cfg, n_queries, qseq, qoff, n_pairs, pair_query, pair_graph, slack, limit, best,
                           score, flags, stats, device);
}

int poa_score_best_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs2_t* costs, const poa_config_t* cfg,
                          uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs, const uint32_t* pair_query,
                          const uint32_t* pair_graph, uint32_t slack, const uint32_t* limit, poa_best_t* best, uint32_t* score,
                          uint32_t* flags, poa_stats_t* stats, int device) {
    if (!costs || !best) return fail(POA_ERR_INVALID_ARG, "poa_score_best_2piece: null argument");
    if (costs->gap_extend1 < costs->gap_extend2)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    return score_best_impl(graphs, n_graphs, nullptr, costs, cfg, n_queries, qseq, qoff, n_pairs, pair_query, pair_graph, slack, limit, best,
                           score, flags, stats, device);
}

int poa_score_pairs(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs_t* costs, const poa_config_t* cfg,
                    uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs, const uint32_t* pair_query,
                    const uint32_t* pair_graph, uint32_t* score, uint32_t* flags, poa_stats_t* stats, int device) {
    if (!costs) return fail(POA_ERR_INVALID_ARG, "poa_score_pairs: null argument");
    return score_pairs_impl(graphs, n_graphs, costs, nullptr, cfg, n_queries, qseq, qoff, n_pairs, pair_query, pair_graph, score, flags, stats, device);
}

int poa_score_pairs_2piece(const poa_graph_t* const* graphs, uint32_t n_graphs, const poa_costs2_t* costs, const poa_config_t* cfg,
                           uint32_t n_queries, const uint8_t* qseq, const uint64_t* qoff, uint64_t n_pairs, const uint32_t* pair_query,
                           const uint32_t* pair_graph, uint32_t* score, uint32_t* flags, poa_stats_t* stats, int device) {
    if (!costs) return fail(POA_ERR_INVALID_ARG, "poa_score_pairs_2piece: null argument");
    if (costs->gap_extend1 < costs->gap_extend2)
        return fail(POA_ERR_INVALID_ARG, "gap_extend1 must be greater than or equal to gap_extend2 for two-piece model");
    return score_pairs_impl(graphs, n_graphs, nullptr, costs, cfg, n_queries, qseq, qoff, n_pairs, pair_query, pair_graph, score, flags, stats, device);
}

}  // extern "C"
