// C entry points to the host-side decisions of the band norms (csrc/ndwt_select.h: norms_chunks, norms_per_band and the constant the
// rule is written in) for tests/test_norms_select.py and tests/test_gpu_norms.py
// (host C++ only: g++ -std=c++17 -Wall -Wextra -Werror -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

// workgroups per (band, item) block of BandNorms
extern "C" long long sel_norms_chunks(long long item_scalars, int comp, int vec, long long bands, long long items, int num_cus, int target_blocks) {
    return norms_chunks(item_scalars, comp, vec != 0, bands, items, num_cus, target_blocks);
}
// 1: one launch per band (more (band, item) blocks than a launch can number)
extern "C" int sel_norms_per_band(long long bands, long long items) { return norms_per_band(bands, items); }
// the turns of its loop every thread keeps before a block gets a further chunk
extern "C" int sel_norms_turns() { return kSelectTurns; }
