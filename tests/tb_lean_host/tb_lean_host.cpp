// Test harness (CPU): the PRODUCT's choice of the traceback walk kernel (tb_lean_eligible / plan_dense_chunk of
// poasta_amd/csrc/poa_dense_plan.cpp) compiled for the host.  tests/test_tb_lean.py loads it as a shared library and holds
// tb_lean_host() against the rule restated in Python; built as a program of its own under -fsanitize=address,undefined, main()
// walks a grid of shapes and overrides and checks what the launcher relies on.  Exit code 0 and "tb_lean_host ok" on success.
// Not shipped.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../poasta_amd/csrc/poa_dense_plan.hpp"

using namespace poa_amd;

extern "C" {

// tune[POA_TUNE_COUNT] as in poa_config_t.  out[0..7]: the launch record of the chunk, out[8]: 1 if the lean walk kernel runs
void tb_lean_host(uint32_t open, uint32_t extend, uint64_t max_len, uint64_t min_path_nodes, uint32_t mode, uint32_t full_planes,
                  const uint32_t* tune, uint32_t count, uint32_t max_pitch, uint64_t plane_elems, uint32_t* out) {
    poa_config_t cfg = {};
    for (int k = 0; k < POA_TUNE_COUNT; ++k) cfg.tune[k] = tune[k];
    const TuneView T(&cfg);
    const DenseRunPlan R = plan_dense_run(open, extend, max_len, min_path_nodes, mode, full_planes != 0, false, T);
    const DenseChunkPlan C = plan_dense_chunk(R, count, max_pitch, T, plane_elems);
    for (int k = 0; k < 8; ++k) out[k] = C.v[k];
    out[8] = C.lean_tb ? 1u : 0u;
}

}  // extern "C"

#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            std::fprintf(stderr, "tb_lean_host: line %d: %s (open %u, extend %u, pitch %u, count %u, lean %d, key %d = %d, mode %u)\n", __LINE__, \
                         #cond, open, extend, pitch, count, lean, key, val, mode);                                               \
            std::exit(1);                                                                                                        \
        }                                                                                                                        \
    } while (0)

int main() {
    const uint32_t opens[] = {6, 0, 30}, extends[] = {2, 0, 8, 255};
    const uint32_t pitches[] = {64, 512, 576, 1024, 1088, 8192}, counts[] = {1, 6144, 6145, 12288, 12289};
    const int keys[][2] = {{-1, 0}, {POA_TUNE_MF, 0}, {POA_TUNE_MF, 1}, {POA_TUNE_MF, 2}, {POA_TUNE_MF, 3}, {POA_TUNE_PLANES, 32}, {POA_TUNE_RELATIVE, 1},
                           {POA_TUNE_FUSE_TB, 1}, {POA_TUNE_COMPACT, 0}, {POA_TUNE_PX, 0}, {POA_TUNE_TB_GROUP, 8}, {POA_TUNE_TB_GROUP, 32}, {POA_TUNE_BAND, 0}};
    unsigned long long checked = 0, n_lean = 0;
    for (uint32_t open : opens) for (uint32_t extend : extends) for (uint32_t pitch : pitches) for (uint32_t count : counts)
        for (const auto& kv : keys) for (int lean : {-1, 0, 1}) for (uint32_t mode : {(uint32_t)POA_MODE_DENSE, (uint32_t)POA_MODE_HYBRID}) {
            const int key = kv[0], val = kv[1];
            uint32_t tune[POA_TUNE_COUNT] = {}, plain[9], o[9], big[9];
            if (key >= 0) tune[key] = (uint32_t)val + 1;
            tb_lean_host(open, extend, pitch - 1, 180, mode, 0, tune, count, pitch, 0, plain);
            if (lean >= 0) tune[POA_TUNE_BAND_PAIR] = (uint32_t)(POA_BAND_PAIR_RULE | ((lean + 1) << POA_TB_LEAN_SHIFT)) + 1;
            tb_lean_host(open, extend, pitch - 1, 180, mode, 0, tune, count, pitch, 0, o);
            tb_lean_host(open, extend, pitch - 1, 180, mode, 0, tune, count, pitch, 1ull << 32, big);
            for (int k = 0; k < 8; ++k) CHECK(o[k] == plain[k] && big[k] == plain[k]);   // the override moves nothing of the launch record
            CHECK(big[8] == 0);                                                        // offsets that do not fit 32 bits: never lean
            if (o[8]) {
                CHECK(mode == POA_MODE_DENSE && lean != 0);
                CHECK(o[4] == 4 && o[5] != 0);          // cells of code_fmt 4 and a separate launch
                CHECK(key != POA_TUNE_PLANES && key != POA_TUNE_RELATIVE && key != POA_TUNE_FUSE_TB && key != POA_TUNE_COMPACT);
                ++n_lean;
            } else if (lean != 0 && mode == POA_MODE_DENSE) CHECK(o[4] != 4 || o[5] == 0);
            CHECK(lean != -1 || o[8] == plain[8]);      // unset == the rule
            if (lean == 1) { uint32_t t2[POA_TUNE_COUNT] = {}; if (key >= 0) t2[key] = (uint32_t)val + 1; uint32_t r[9];
                             tb_lean_host(open, extend, pitch - 1, 180, mode, 0, t2, count, pitch, 0, r); CHECK(r[8] == o[8]); }   // 1 == the rule today
            ++checked;
        }
    if (!n_lean) { std::fprintf(stderr, "tb_lean_host: no shape of the grid takes the lean kernel\n"); return 1; }
    std::printf("tb_lean_host ok: %llu records, %llu lean\n", checked, n_lean);
    return 0;
}
