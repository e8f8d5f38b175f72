// Test harness (CPU): compiles the PRODUCT's selection rule of the dense one-piece pass (poasta_amd/csrc/poa_dense_plan.cpp) for
// the host.  tests/test_dense_launch_matrix.py loads it as a shared library and holds dense_plan_host() against the rule's
// restatement in Python (`predict`); built as a program of its own under -fsanitize=address,undefined, main() walks the grid of
// that test (without the case table's own overrides) and checks what the launcher relies on.  Exit code 0 and
// "dense_plan_host ok" on success.  Not shipped.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../poasta_amd/csrc/poa_dense_plan.hpp"

using namespace poa_amd;

extern "C" {

// tune[POA_TUNE_COUNT] as in poa_config_t (0: not set, else value + 1).  out[0..7]: the launch record of the chunk
// (poa_batch_last_launch), out[8]: POA_LAYOUT_* bits, out[9]: the banded pair runs, out[10]: the chunk plan of the run (0 / 1 / 2).
void dense_plan_host(uint32_t mismatch, uint32_t open, uint32_t extend, uint64_t max_len, uint64_t min_path_nodes, uint32_t mode,
                     uint32_t full_planes, uint32_t plan16_same, const uint32_t* tune, uint32_t count, uint32_t max_pitch, uint32_t* out) {
    (void)mismatch;   // no rule reads it
    poa_config_t cfg = {};
    for (int k = 0; k < POA_TUNE_COUNT; ++k) cfg.tune[k] = tune[k];
    const TuneView T(&cfg);
    const DenseRunPlan R = plan_dense_run(open, extend, max_len, min_path_nodes, mode, full_planes != 0, plan16_same != 0, T);
    const DenseChunkPlan C = plan_dense_chunk(R, count, max_pitch, T);
    for (int k = 0; k < 8; ++k) out[k] = C.v[k];
    out[8] = (R.narrow ? POA_LAYOUT_U16 : 0u) | (R.compact ? POA_LAYOUT_COMPACT : 0u) | (R.relative ? POA_LAYOUT_RELATIVE : 0u) |
             (C.mf == 3 ? POA_LAYOUT_DERIVED_GAPS : 0u);
    out[9] = C.band ? 1u : 0u;
    out[10] = (uint32_t)R.plan;
}

}  // extern "C"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            std::fprintf(stderr, "dense_plan_host: line %d: %s (costs %u %u, mpn %u, max_len %u, pitch %u, count %u, tune %d = %d, full %u)\n", \
                         __LINE__, #cond, oe.first, oe.second, mpn, max_len, pitch, count, key, val, full);                  \
            std::exit(1);                                                                                                    \
        }                                                                                                                    \
    } while (0)

int main() {
    const std::pair<uint32_t, uint32_t> costs[] = {{6, 2}, {6, 0}, {0, 1}, {6, 8}, {6, 30}, {6, 255}};
    const uint32_t mpns[] = {0, 1, 180, 5000}, batch_len[] = {0, 3000, 33000};   // 0: the chunk's own longest query
    const uint32_t cols[] = {1, 64, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 8192, 8193, 10241};
    const uint32_t counts[] = {1, 511, 512, 1023, 1024, 4095, 4096, 6144, 6145, 12288, 12289};
    // no override, then every selection key alone at each value the rule distinguishes
    std::vector<std::pair<int, int>> tunes = {{-1, 0}, {POA_TUNE_PLANES, 32}, {POA_TUNE_FUSE_TB, 1}};
    for (int k : {POA_TUNE_COMPACT, POA_TUNE_PACKED, POA_TUNE_PX, POA_TUNE_MW, POA_TUNE_PXMW, POA_TUNE_BAND, POA_TUNE_RELATIVE})
        for (int v : {0, 1}) tunes.push_back({k, v});
    for (int v : {0, 1, 2, 3}) tunes.push_back({POA_TUNE_MF, v});
    for (int v : {1, 2, 4}) tunes.push_back({POA_TUNE_FWD_QUADS, v});
    for (int v : {8, 16, 32, 64, 7}) tunes.push_back({POA_TUNE_TB_GROUP, v});
    for (int v : {1, 64, 65}) tunes.push_back({POA_TUNE_TB_DEPTH, v});
    for (int v : {0, 5}) tunes.push_back({POA_TUNE_BAND_DELTA, v});
    unsigned long long checked = 0;
    for (const auto& oe : costs) for (uint32_t mpn : mpns) for (uint32_t bl : batch_len) for (uint32_t c : cols) {
        const uint32_t pitch = (c + 63) / 64 * 64, max_len = bl ? bl : c - 1;
        if (max_len < c - 1) continue;   // the batch's longest query is no shorter than the chunk's
        for (uint32_t count : counts) for (uint32_t full : {0u, 1u}) for (const auto& kv : tunes) {
            const int key = kv.first, val = kv.second;
            uint32_t tune[POA_TUNE_COUNT] = {}, o[11];
            if (key >= 0) tune[key] = (uint32_t)val + 1;
            dense_plan_host(4, oe.first, oe.second, max_len, mpn, POA_MODE_DENSE, full, 0, tune, count, pitch, o);
            const bool u16 = o[8] & POA_LAYOUT_U16, compact = o[8] & POA_LAYOUT_COMPACT, relative = o[8] & POA_LAYOUT_RELATIVE;
            CHECK(o[0] != POA_KERNEL_NONE && o[0] <= POA_KERNEL_BAND);
            CHECK(o[1] == 1 || o[1] == 2 || (!u16 && o[1] == 4));
            CHECK(o[3] >= 1 && o[3] <= 16);
            if (o[2] & POA_LAUNCH_MW) {   // the groups of a workgroup's waves, one after the other, cover the widest row
                const uint32_t strip = (u16 ? 512u : 256u) * o[1], strips = (pitch + strip - 1) / strip, groups = (strips + o[3] - 1) / o[3];
                CHECK((unsigned long long)o[3] * groups * strip >= pitch);
                CHECK(!(o[2] & POA_LAUNCH_FUSE));
            }
            CHECK(o[5] == 0 || o[5] == 8 || o[5] == 16 || o[5] == 32 || o[5] == 64);
            CHECK(o[6] >= 1 && o[6] <= 64 && o[7] == count);
            CHECK(!relative || (compact && u16));
            CHECK(!compact || u16);
            CHECK((o[9] != 0) == (o[0] == POA_KERNEL_BAND) && (!o[9] || (o[8] & POA_LAYOUT_DERIVED_GAPS)));
            CHECK(o[10] == (u16 ? (compact ? 2u : 1u) : 0u));
            ++checked;
        }
    }
    std::printf("dense_plan_host ok: %llu records\n", checked);
    return 0;
}
