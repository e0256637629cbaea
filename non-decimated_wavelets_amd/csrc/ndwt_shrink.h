// ndwt_shrink.h -- the thresholding arithmetic, once: shrink_kernel (ndwt_api.hip) runs it on coefficients in memory, Den1C
// (ndwt_device_1d.h) on coefficients in a lane's registers.
#pragma once
#include "ndwt_device.h"
#ifdef NDWT_HOST_EMU
#include <math.h>
#endif

namespace ndwt {

// Element-wise, 1 read + 1 write per coefficient.  COMP = 2: interleaved complex, the magnitude
// is shrunk and the phase kept.  mode 0 soft: c * max(|c| - t, 0) / |c|; mode 1 hard: c if |c| > t else 0.
// the magnitude of an interleaved complex coefficient as the shrink compares it with its threshold -- and as the order statistics of a
// band order it (BandHist, ndwt_device_select.h)
template <typename T> NDWT_DEV T shrink_magnitude(T re, T im) { return sqrt(re * re + im * im); }

template <typename T, int COMP> NDWT_DEV void shrink_group(T* c, T thr, int hard) {
    if (COMP == 1) {
        const T m = c[0] < T(0) ? -c[0] : c[0];
        if (hard) c[0] = m > thr ? c[0] : T(0);
        else c[0] = m > thr ? (c[0] < T(0) ? c[0] + thr : c[0] - thr) : T(0);
    } else {
        const T m = shrink_magnitude(c[0], c[1]);
        const T g = m > thr ? (hard ? T(1) : (m - thr) / m) : T(0);
        c[0] *= g;
        c[1] *= g;
    }
}

}  // namespace ndwt
