// The cases of tests/test_emulated_den1r.py as a program of its own, for AddressSanitizer + UBSan (the test compiles it and
// ndwt_emu_den1r.cpp with -fsanitize=address,undefined and runs it as a child process).
// argv[1]: a case file the test wrote --
//   int32 ncases; per case: int32 which, f64, nlev, row, outer, hard; double taps[80]; double thr[outer][1 + nlev];
//   then the input (outer rows of `row` scalars in the case's precision).
// Every buffer is a heap block of exactly its size.  Per case: the ROWTHR kernel on all rows with the table, then the uniform kernel
// once per row with that row's thresholds; row j of the first must be row j of the j-th run bit for bit.  Exit status 0: every case passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

extern "C" int ndwt_emu1r_denoise(int which, const void* in, void* out, long long row, long long outer, const double* taps, const double* thr, int hard,
                                  int rowthr);

template <typename T> static int run_case(FILE* f, const int* h, const double* taps, const std::vector<double>& thr) {
    const size_t row = (size_t)h[3], K = (size_t)h[4], n = row * K, nb = 1 + (size_t)h[2];
    std::vector<T> in(n);
    if (std::fread(in.data(), sizeof(T), n, f) != n) return 2;
    std::unique_ptr<T[]> src(new T[n]), got(new T[n]), one(new T[n]);
    std::memcpy(src.get(), in.data(), n * sizeof(T));
    for (size_t i = 0; i < n; ++i) got[i] = std::nan("");
    if (ndwt_emu1r_denoise(h[0], src.get(), got.get(), (long long)row, (long long)K, taps, thr.data(), h[5], 1) < 0) return 3;
    for (size_t j = 0; j < K; ++j) {
        for (size_t i = 0; i < n; ++i) one[i] = std::nan("");
        if (ndwt_emu1r_denoise(h[0], src.get(), one.get(), (long long)row, (long long)K, taps, thr.data() + j * nb, h[5], 0) < 0) return 3;
        if (std::memcmp(got.get() + j * row, one.get() + j * row, row * sizeof(T)) != 0) { std::fprintf(stderr, "row %zu differs\n", j); return 4; }
    }
    if (std::memcmp(src.get(), in.data(), n * sizeof(T)) != 0) return 5;
    std::printf("  ok: instance %d, %zu rows of %zu scalars, hard %d\n", h[0], K, row, h[5]);
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
        double taps[80];
        if (std::fread(h, sizeof(int), 6, f) != 6 || std::fread(taps, sizeof(double), 80, f) != 80 || h[4] < 1 || h[2] < 1 || h[2] > 4) return 65;
        std::vector<double> thr((size_t)h[4] * (size_t)(1 + h[2]));
        if (std::fread(thr.data(), sizeof(double), thr.size(), f) != thr.size()) return 65;
        const int rc = h[1] ? run_case<double>(f, h, taps, thr) : run_case<float>(f, h, taps, thr);
        if (rc) { std::fprintf(stderr, "case %d failed (%d)\n", c, rc); return 1; }
    }
    std::fclose(f);
    std::printf("%d cases ok\n", ncases);
    return 0;
}
