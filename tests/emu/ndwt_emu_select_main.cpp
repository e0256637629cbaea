// The cases of tests/test_emulated_select.py as a program of its own, for AddressSanitizer + UBSan (the test compiles it and
// ndwt_emu_select.cpp with -fsanitize=address,undefined and runs it as a child process).
// argv[1]: a case file the test wrote --
//   int32 ncases; per case: int32 f64, comp, vec, nk, nblocks, exact; int64 n_scalars; int64 k[4]; double want[4];
//   then the band (n_scalars scalars in the case's precision).
// exact = 1 (real data): values[i] must be want[i] bit for bit (a NaN for a NaN).  exact = 0 (complex data): with m = hypot(re, im) in
// double and eps = 4 machine epsilons of the scalar type, count(m < v (1 - eps)) <= k < count(m <= v (1 + eps)).
// The band is a heap block of exactly its size, so a step of a loop too far is a sanitizer report; it is compared with its copy
// afterwards.  Exit status 0: every case ran and passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

extern "C" int ndwt_emu_select(int f64, int comp, int vec, const void* y, long long n_scalars, int nk, const long long* k, int nblocks, double* values);

template <typename T> static int run_case(FILE* f, const int* h, long long n, const long long* k, const double* want) {
    std::vector<T> in((size_t)n);
    if (std::fread(in.data(), sizeof(T), (size_t)n, f) != (size_t)n) return 2;
    struct Free { void operator()(T* q) const { ::operator delete(q, std::align_val_t(32)); } };   // (32 bytes: the 4-scalar form of double data)
    std::unique_ptr<T, Free> y(static_cast<T*>(::operator new((size_t)n * sizeof(T), std::align_val_t(32))));
    std::memcpy(y.get(), in.data(), (size_t)n * sizeof(T));
    double v[4] = {-1, -1, -1, -1};
    if (ndwt_emu_select(h[0], h[1], h[2], y.get(), n, h[3], k, h[4], v) != 0) return 3;
    if (std::memcmp(y.get(), in.data(), (size_t)n * sizeof(T)) != 0) return 5;      // the band is read only
    for (int i = 0; i < h[3]; ++i) {
        if (h[5]) {
            if (!(std::memcmp(&v[i], &want[i], sizeof(double)) == 0 || (std::isnan(v[i]) && std::isnan(want[i])))) {
                std::fprintf(stderr, "rank %lld: got %.17g, want %.17g\n", k[i], v[i], want[i]);
                return 4;
            }
        } else {
            const double eps = 4.0 * (sizeof(T) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16);
            long long below = 0, upto = 0;
            for (long long e = 0; e < n / 2; ++e) {
                const double m = std::hypot((double)in[(size_t)(2 * e)], (double)in[(size_t)(2 * e + 1)]);
                below += m < v[i] * (1 - eps);
                upto += m <= v[i] * (1 + eps);
            }
            if (!(below <= k[i] && k[i] < upto)) {
                std::fprintf(stderr, "rank %lld: got %.17g with %lld magnitudes below and %lld up to it\n", k[i], v[i], below, upto);
                return 4;
            }
        }
    }
    std::printf("  ok: f64 %d comp %d vec %d nk %d blocks %d  %lld scalars\n", h[0], h[1], h[2], h[3], h[4], n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 64; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 66; }
    int ncases = 0;
    if (std::fread(&ncases, sizeof(int), 1, f) != 1 || ncases < 1) return 65;
    for (int c = 0; c < ncases; ++c) {
        int h[6];
        long long n, k[4];
        double want[4];
        if (std::fread(h, sizeof(int), 6, f) != 6 || std::fread(&n, sizeof n, 1, f) != 1 || std::fread(k, sizeof(long long), 4, f) != 4 ||
            std::fread(want, sizeof(double), 4, f) != 4 || n < 1) return 65;
        const int rc = h[0] ? run_case<double>(f, h, n, k, want) : run_case<float>(f, h, n, k, want);
        if (rc) { std::fprintf(stderr, "case %d failed (%d)\n", c, rc); return 1; }
    }
    std::fclose(f);
    std::printf("%d cases ok\n", ncases);
    return 0;
}
