// The cases of tests/test_emulated_select_items.py as a program of its own, for AddressSanitizer + UBSan (the test compiles it and
// ndwt_emu_select_items.cpp with -fsanitize=address,undefined and runs it as a child process).
// argv[1]: a case file the test wrote --
//   int32 ncases; per case: int32 f64, comp, vec, nk, exact; int64 n_scalars, items; int64 k[4]; double want[items][4];
//   then the items (items x n_scalars scalars in the case's precision).
// exact = 1 (real data): values[j][i] must be want[j][i] bit for bit (a NaN for a NaN).  exact = 0 (complex data): with m = hypot(re, im)
// in double over item j and eps = 4 machine epsilons of the scalar type, count(m < v (1 - eps)) <= k < count(m <= v (1 + eps)).
// The items are one heap block of exactly their size (vec = 0 cases: one element past a 32-byte boundary, off the groups of 4 scalars),
// so a step of a loop too far is a sanitizer report; the block is compared with its copy afterwards.  After the select, ShrinkItems runs
// on a copy of the same block as a coefficient array of one band with thresholds 0, 0.5, 1, ... per item, against shrink_group element
// by element.  Exit status 0: every case ran and passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

extern "C" int ndwt_emu_select_items(int f64, int comp, int vec, const void* y, long long n_scalars, long long items, int nk, const long long* k,
                                     double* values);
extern "C" int ndwt_emu_shrink_items(int f64, int comp, void* y, long long pitch, long long n_scalars, const double* thr, long long items, int nb,
                                     int chunks, int hard);

template <typename T> static void soft(T* c, int comp, T thr) {   // (the arithmetic of shrink_group, soft mode)
    if (comp == 1) {
        const T m = c[0] < T(0) ? -c[0] : c[0];
        c[0] = m > thr ? (c[0] < T(0) ? c[0] + thr : c[0] - thr) : T(0);
    } else {
        const T m = std::sqrt(c[0] * c[0] + c[1] * c[1]);
        const T g = m > thr ? (m - thr) / m : T(0);
        c[0] *= g;
        c[1] *= g;
    }
}

template <typename T> static int run_case(FILE* f, const int* h, long long n, long long items, const long long* k, const std::vector<double>& want) {
    const size_t total = (size_t)(n * items);
    std::vector<T> in(total);
    if (std::fread(in.data(), sizeof(T), total, f) != total) return 2;
    const size_t skew = h[2] == 0 ? (size_t)h[1] : 0;           // (one element: complex data lies on whole elements)
    struct Free { void operator()(T* q) const { ::operator delete(q, std::align_val_t(32)); } };
    std::unique_ptr<T, Free> block(static_cast<T*>(::operator new((total + skew) * sizeof(T), std::align_val_t(32))));
    T* const y = block.get() + skew;
    std::memcpy(y, in.data(), total * sizeof(T));
    std::vector<double> v((size_t)items * h[3], -1.0);
    if (ndwt_emu_select_items(h[0], h[1], h[2], y, n, items, h[3], k, v.data()) != 0) return 3;
    if (std::memcmp(y, in.data(), total * sizeof(T)) != 0) return 5;             // the band is read only
    for (long long j = 0; j < items; ++j)
        for (int i = 0; i < h[3]; ++i) {
            const double got = v[(size_t)j * h[3] + i], w = want[(size_t)j * 4 + i];
            if (h[4]) {
                if (!(std::memcmp(&got, &w, sizeof(double)) == 0 || (std::isnan(got) && std::isnan(w)))) {
                    std::fprintf(stderr, "item %lld rank %lld: got %.17g, want %.17g\n", j, k[i], got, w);
                    return 4;
                }
            } else {
                const double eps = 4.0 * (sizeof(T) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16);
                long long below = 0, upto = 0, numbers = 0;
                for (long long e = 0; e < n / 2; ++e) {
                    const double m = std::hypot((double)in[(size_t)(j * n + 2 * e)], (double)in[(size_t)(j * n + 2 * e + 1)]);
                    below += m < got * (1 - eps);
                    upto += m <= got * (1 + eps);
                    numbers += !std::isnan((double)in[(size_t)(j * n + 2 * e)]) && !std::isnan((double)in[(size_t)(j * n + 2 * e + 1)]);
                }
                if (std::isnan(got) ? k[i] < numbers : !(below <= k[i] && k[i] < upto)) {   // (a NaN: only past the item's numbers)
                    std::fprintf(stderr, "item %lld rank %lld: got %.17g with %lld magnitudes below and %lld up to it\n", j, k[i], got, below, upto);
                    return 4;
                }
            }
        }
    // ShrinkItems on the same block: one band, item j with the threshold j / 2 (item 0: left alone)
    std::vector<double> thr((size_t)items);
    for (long long j = 0; j < items; ++j) thr[(size_t)j] = 0.5 * (double)j;
    const int vec = ndwt_emu_shrink_items(h[0], h[1], y, n * items, n, thr.data(), items, 1, 2, 0);
    if (vec < 0) return 6;
    std::vector<T> ref(in);
    for (long long j = 1; j < items; ++j)
        for (long long e = 0; e < n; e += h[1]) soft(&ref[(size_t)(j * n + e)], h[1], (T)thr[(size_t)j]);
    if (std::memcmp(y, ref.data(), total * sizeof(T)) != 0) return 7;
    std::printf("  ok: f64 %d comp %d vec %d nk %d  %lld items of %lld scalars (shrink: %s form)\n", h[0], h[1], h[2], h[3], items, n, vec ? "4-scalar" : "element-wise");
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 64; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 66; }
    int ncases = 0;
    if (std::fread(&ncases, sizeof(int), 1, f) != 1 || ncases < 1) return 65;
    for (int c = 0; c < ncases; ++c) {
        int h[5];
        long long n, items, k[4];
        if (std::fread(h, sizeof(int), 5, f) != 5 || std::fread(&n, sizeof n, 1, f) != 1 || std::fread(&items, sizeof items, 1, f) != 1 ||
            std::fread(k, sizeof(long long), 4, f) != 4 || n < 1 || items < 1) return 65;
        std::vector<double> want((size_t)items * 4);
        if (std::fread(want.data(), sizeof(double), want.size(), f) != want.size()) return 65;
        const int rc = h[0] ? run_case<double>(f, h, n, items, k, want) : run_case<float>(f, h, n, items, k, want);
        if (rc) { std::fprintf(stderr, "case %d failed (%d)\n", c, rc); return 1; }
    }
    std::fclose(f);
    std::printf("%d cases ok\n", ncases);
    return 0;
}
