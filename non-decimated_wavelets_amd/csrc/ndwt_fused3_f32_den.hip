// Level 1 of a denoising step (dec -> shrink -> rec) without its detail bands in memory, float, real data, tap lengths 2 .. 8:
// Den3 (analysis of the haloed tile + thresholding + synthesis in one launch) and the approximation-only analysis Fwd3<.., LOWONLY>
// that feeds the deeper levels (ndwt_denoise chooses both).  Reference use case: README.md:2 ("iterative algorithm").
#include "ndwt_fused_kernels.h"
namespace ndwt {

template <int LL> static int go_den(const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    typedef Den3<float, LL, 1024, 4, (LL == 8 ? 6 : 0)> K;   // 8 taps: 6 of the 8 pending z sums in LDS (no spills)
    return launch_fused3<K>(a, taps_dev, s);
}

int launch_den3_f32(const Fused3Args<float>& a, int Lp, const void* taps_dev, hipStream_t s) {
    switch (Lp) {
        case 2: return go_den<2>(a, taps_dev, s);
        case 4: return go_den<4>(a, taps_dev, s);
        case 6: return go_den<6>(a, taps_dev, s);
        case 8: return go_den<8>(a, taps_dev, s);
        default: return -1;
    }
}

// band 0 only, on the tile the caller laid out: TILE 2 = the tall 64 x 32 tile of the float analysis (1024 threads, one workgroup per
// CU), 0 = 64 x 16 (256 threads)
#define NDWT_LAUNCH_LOW(LL, TILE, V)                                                                           \
    if (Lp == LL && tile == TILE && vec4 == V) return launch_fused3<NDWT_FUSED_K(Fwd3, false, float, LL, TILE, V, 1, true)>(a, taps_dev, s);
#define NDWT_LOW2(LL, TILE) NDWT_LAUNCH_LOW(LL, TILE, true) NDWT_LAUNCH_LOW(LL, TILE, false)
#define NDWT_LOW8(TILE) NDWT_LOW2(2, TILE) NDWT_LOW2(4, TILE) NDWT_LOW2(6, TILE) NDWT_LOW2(8, TILE)
int launch_fwd3_low_f32(const Fused3Args<float>& a, int Lp, bool vec4, int tile, const void* taps_dev, hipStream_t s) {
    NDWT_LOW8(0) NDWT_LOW8(2)
    return -1;
}

// 4-D analysis with the t axis folded in (Fwd3<.., TPRE>): chosen by the pick, as every instance of the other units
int launch3_f32_den(const Fused3Instance& k, const Fused3Args<float>& a, const void* taps_dev, hipStream_t s) {
    NDWT_LIST_F32_DEN(NDWT_LAUNCH_F)
    return -1;
}
}  // namespace ndwt
