// rl_tally.hip -- the usage tally's kernels (rl_tally.h) as a translation unit
// of their own, and the two launchers rl_engine.hip calls.
#define RL_TALLY_DEVICE
#include "rl_tally.h"

#include <algorithm>

namespace rl {

hipError_t tally_launch(uint64_t m, const uint64_t* key, const uint32_t* cfg, const int64_t* n, const uint8_t* dec,
                        uint32_t ncfg, tally_u64* cfgc, tally_u64* glob, TallyKey* keys, uint64_t slots,
                        hipStream_t s) {
    // m == 0 (rl_tally_enable's warm-up): one block that finds nothing to do
    const int grid = (int)std::clamp<uint64_t>((m + TALLY_BLOCK - 1) / TALLY_BLOCK, 1, (uint64_t)TALLY_GRID);
    k_tally<<<grid, TALLY_BLOCK, 0, s>>>(m, key, cfg, n, dec, ncfg, cfgc, glob, keys, slots - 1,
                                         std::min<uint64_t>(slots, TALLY_PROBES));
    return hipGetLastError();
}

hipError_t tally_clear_launch(TallyKey* keys, uint64_t slots, tally_u64* cfgc, uint64_t cfg_words, tally_u64* glob,
                              hipStream_t s) {
    k_tally_clear<<<256, 256, 0, s>>>(keys, slots, cfgc, cfg_words, glob);
    return hipGetLastError();
}

}  // namespace rl
