// C entry points to the host-side decisions of the order statistics of a band (csrc/ndwt_select.h: select_passes, select_digit_shift /
// select_digit_bits, select_vec, select_grid, select_fits, select_agg) for tests/test_abi_select.py and tests/test_gpu_select.py
// (host C++ only: g++ -std=c++17 -Wall -Wextra -Werror -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

extern "C" int sel_select_passes(int f64) { return select_passes(f64 != 0); }
extern "C" int sel_select_key_bits(int f64) { return select_key_bits(f64 != 0); }
extern "C" int sel_select_digit_shift(int f64, int pass) { return select_digit_shift(f64 != 0, pass); }
extern "C" int sel_select_digit_bits(int f64, int pass) { return select_digit_bits(f64 != 0, pass); }
extern "C" int sel_select_vec(unsigned long long addr, long long n_scalars, int scalar_bytes) { return select_vec(addr, n_scalars, scalar_bytes); }
extern "C" long long sel_select_grid(long long n_scalars, int comp, int vec, int num_cus, int target_blocks) {
    return select_grid(n_scalars, comp, vec != 0, num_cus, target_blocks);
}
extern "C" int sel_select_fits(long long n_elements) { return select_fits(n_elements); }
extern "C" int sel_select_agg(int variant_fwd) { return select_agg(variant_fwd); }
extern "C" int sel_select_consts(int which) { return which == 0 ? kSelectDigitBits : which == 1 ? kSelectBins : kSelectMaxRanks; }
