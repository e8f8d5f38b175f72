// Test harness (CPU): compiles the PRODUCT's rule for the narrow tier of the paired banded pass (band_narrow_class and
// band_narrow_pairs in poasta_amd/csrc/poa_dense_plan.cpp, with the override as plan_dense_run decodes it from
// POA_TUNE_BAND_PAIR) for the host.  tests/test_band_narrow_plan.py loads it as a shared library.  Not shipped.
#include <cstdint>

#include "../../poasta_amd/csrc/poa_dense_plan.hpp"

using namespace poa_amd;

extern "C" {

// 0: the rule takes the class, 1: only the override does, 2: never (no narrow band)
uint32_t band_narrow_host_class(uint32_t d_n, uint32_t L) { return band_narrow_class(d_n, L); }

// tune_pair: the value of tune[POA_TUNE_BAND_PAIR] as in poa_config_t (0: not set, else value + 1).  out[0] the run's band_pair
// (-1 by the rule, 0, 1), out[1] its band_narrow (-1 by the rule, 0, 1), out[2] the leading pairs of a chunk that run the
// narrow tier, given whether the chunk pairs by the count rule, the pairs of classes the rule takes and those with a narrow band
void band_narrow_host_pairs(uint32_t tune_pair, uint32_t pair_by_rule, uint32_t n_rule, uint32_t n_any, int32_t* out) {
    poa_config_t cfg = {};
    cfg.tune[POA_TUNE_BAND_PAIR] = tune_pair;
    const TuneView T(&cfg);
    const DenseRunPlan R = plan_dense_run(6, 2, 1000, 1000, POA_MODE_DENSE, false, false, T);
    out[0] = R.band_pair; out[1] = R.band_narrow;
    out[2] = (int32_t)band_narrow_pairs(R, pair_by_rule != 0, n_rule, n_any);
}

}  // extern "C"
