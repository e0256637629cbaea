// The tap tables the host builds (csrc/ndwt_taps_host.h: what the library uploads and what the emulators run on) against the structs the
// kernels read (Taps3, Taps3Y, TapsDen of csrc/ndwt_device.h) -- a program of its own for AddressSanitizer + UBSan
// (tests/test_taps_host.py compiles it with -fsanitize=address,undefined and runs it as a child process).
// Every even L from 2 to 20 for float and double, TapsDen<float, L> for L = 2 .. 8.  The taps are distinct numbers (100 axis + j + 1,
// the high-pass ones 1000 more, the analysis ones 5000 more), so a transposed or shifted index shows; the table is copied from a heap
// block of exactly its size into a heap struct of exactly its size, and every field is compared by name with its definition.
// Exit status 0: every table agrees.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#define NDWT_HOST_EMU 1
#include "ndwt_taps_host.h"

using namespace ndwt;

static int g_bad = 0, g_tables = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            if (++g_bad <= 20) { std::fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, ": %s\n", #cond); } \
        }                                                                                  \
    } while (0)

// mirrored: hi of x and y derived from lo as the Den3 kernel derives them, ahi[j] = (-1)^j alo[L-1-j]
static FusedTapsD distinct_taps(int L, double base, bool mirrored) {
    FusedTapsD t;
    std::memset(&t, 0, sizeof t);
    t.Lp = L;
    for (int ax = 0; ax < 3; ++ax)
        for (int j = 0; j < L; ++j) {
            t.lo[ax][j] = base + 100 * ax + j + 1;
            t.hi[ax][j] = base + 1000 + 100 * ax + j + 1;
        }
    for (int ax = 0; ax < 2 && mirrored; ++ax)
        for (int j = 0; j < L; ++j) t.hi[ax][j] = (j % 2 ? -1.0 : 1.0) * t.lo[ax][L - 1 - j];
    return t;
}

// the builder's scalars -> a heap block of exactly their size -> a heap struct, which must be as large
template <class TP, typename T> static std::unique_ptr<TP> as_struct(const std::vector<T>& h, int L, const char* what) {
    std::unique_ptr<TP> tp(new TP);
    CHECK(h.size() * sizeof(T) == sizeof(TP), "%s L=%d: %zu scalars for a struct of %zu bytes", what, L, h.size(), sizeof(TP));
    if (h.size() * sizeof(T) != sizeof(TP)) return nullptr;
    std::unique_ptr<T[]> block(new T[h.size()]);
    std::memcpy(block.get(), h.data(), h.size() * sizeof(T));
    std::memcpy(tp.get(), block.get(), sizeof(TP));
    ++g_tables;
    return tp;
}

template <class TP, typename T> static void check_lo_hi(const TP& tp, const FusedTapsD& t, int L, const char* what) {
    for (int ax = 0; ax < 3; ++ax)
        for (int j = 0; j < L; ++j) {
            CHECK(tp.lo[ax][j] == (T)t.lo[ax][j], "%s L=%d lo[%d][%d]", what, L, ax, j);
            CHECK(tp.hi[ax][j] == (T)t.hi[ax][j], "%s L=%d hi[%d][%d]", what, L, ax, j);
        }
}
// pairs[k][h] = taps[k - h], 0 outside [0, L)
template <typename T, int N> static void check_pairs(const T (&pairs)[N][2], const double* taps, int L, const char* what) {
    CHECK(N == L + 1, "%s L=%d: %d pairs", what, L, N);
    for (int k = 0; k < N; ++k)
        for (int h = 0; h < 2; ++h) {
            const int j = k - h;
            CHECK(pairs[k][h] == (j >= 0 && j < L ? (T)taps[j] : T(0)), "%s L=%d [%d][%d]", what, L, k, h);
        }
}

template <typename T, int L> static void check_taps3() {
    const FusedTapsD t = distinct_taps(L, 0, false);
    std::vector<T> h;
    append_taps3(h, t, false);
    if (auto tp = as_struct<Taps3<T, L>>(h, L, "Taps3")) check_lo_hi<Taps3<T, L>, T>(*tp, t, L, "Taps3");
    h.clear();
    append_taps3(h, t, true);
    if (auto tp = as_struct<Taps3Y<T, L>>(h, L, "Taps3Y")) {
        check_lo_hi<Taps3Y<T, L>, T>(*tp, t, L, "Taps3Y");
        check_pairs(tp->xplo, t.lo[0], L, "Taps3Y xplo");
        check_pairs(tp->xphi, t.hi[0], L, "Taps3Y xphi");
    }
}

template <int L> static void check_taps_den() {
    const FusedTapsD syn = distinct_taps(L, 0, false), ana = distinct_taps(L, 5000, true);
    std::vector<float> h;
    CHECK(build_taps_den(h, syn, ana), "TapsDen L=%d: mirrored taps refused", L);
    if (auto tp = as_struct<TapsDen<float, L>>(h, L, "TapsDen")) {
        check_lo_hi<Taps3Y<float, L>, float>(tp->syn, syn, L, "TapsDen syn");
        check_pairs(tp->syn.xplo, syn.lo[0], L, "TapsDen syn.xplo");
        check_pairs(tp->syn.xphi, syn.hi[0], L, "TapsDen syn.xphi");
        for (int ax = 0; ax < 3; ++ax)
            for (int j = 0; j < L; ++j) CHECK(tp->alo[ax][j] == (float)ana.lo[ax][j], "TapsDen L=%d alo[%d][%d]", L, ax, j);
        for (int j = 0; j < L; ++j) {
            CHECK(tp->azp[j][0] == (float)ana.lo[2][j], "TapsDen L=%d azp[%d][0]", L, j);
            CHECK(tp->azp[j][1] == (float)ana.hi[2][j], "TapsDen L=%d azp[%d][1]", L, j);
        }
        check_pairs(tp->axp, ana.lo[0], L, "TapsDen axp");
    }
    // high-pass taps of x (or y) that are not the mirror of the low-pass ones: no table
    for (int ax = 0; ax < 2; ++ax) {
        FusedTapsD off = ana;
        off.hi[ax][L - 1] += 1;
        CHECK(!build_taps_den(h, syn, off), "TapsDen L=%d: taps of axis %d that are no mirrored pair accepted", L, ax);
    }
}

template <int... Ls> static void all_lengths() {
    (check_taps3<float, Ls>(), ...);
    (check_taps3<double, Ls>(), ...);
}

int main() {
    all_lengths<2, 4, 6, 8, 10, 12, 14, 16, 18, 20>();
    check_taps_den<2>();
    check_taps_den<4>();
    check_taps_den<6>();
    check_taps_den<8>();
    if (g_bad) { std::fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    std::printf("%d tap tables ok\n", g_tables);
    return 0;
}
