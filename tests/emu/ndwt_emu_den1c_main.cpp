// The cases of tests/test_emulated_den1c.py as a program of its own, for AddressSanitizer + UBSan (the test compiles it with
// -fsanitize=address,undefined, links it with the parts of ndwt_emu_den1c.cpp built the same way, and runs it as a child process).
// argv[1]: a case file the test wrote --
//   int32 ncases; per case: int32 f64, ew, L, nlev, row, outer, hard; double taps[80], thr[5], tol;
//   the input (outer rows of `row` scalars), then the expected output, in the case's precision.
// Every buffer is a heap block of exactly its size, so a lane or a row too far is a sanitizer report.  Exit status 0: every case
// ran and agrees with its expected output to its tolerance.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

extern "C" int ndwt_emu1_denoise(int f64, int ew, int L, int nlev, const void* in, void* out, long long row, long long outer, const double* taps,
                                 const double* thr, int hard);

template <typename T> static int run_case(FILE* f, const int* h, const double* taps, const double* thr, double tol) {
    const size_t n = (size_t)h[4] * (size_t)h[5];
    std::vector<T> in(n), want(n);
    if (std::fread(in.data(), sizeof(T), n, f) != n || std::fread(want.data(), sizeof(T), n, f) != n) return 2;
    std::unique_ptr<T[]> src(new T[n]), out(new T[n]);
    std::memcpy(src.get(), in.data(), n * sizeof(T));
    for (size_t i = 0; i < n; ++i) out[i] = std::nan("");
    if (ndwt_emu1_denoise(h[0], h[1], h[2], h[3], src.get(), out.get(), h[4], h[5], taps, thr, h[6]) != 0) return 3;
    double worst = 0;
    for (size_t i = 0; i < n; ++i) {
        const double d = std::fabs((double)out[i] - (double)want[i]);
        if (!(d <= tol)) { std::fprintf(stderr, "element %zu: got %g, want %g (tolerance %g)\n", i, (double)out[i], (double)want[i], tol); return 4; }
        worst = d > worst ? d : worst;
    }
    std::printf("  ok: f64 %d ew %d L %d nlev %d row %d x %d signals hard %d  max error %.3g (tolerance %.3g)\n", h[0], h[1], h[2], h[3], h[4], h[5], h[6],
                worst, tol);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 64; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 66; }
    int ncases = 0;
    if (std::fread(&ncases, sizeof(int), 1, f) != 1 || ncases < 1) return 65;
    for (int c = 0; c < ncases; ++c) {
        int h[7];
        double taps[80], thr[5], tol;
        if (std::fread(h, sizeof(int), 7, f) != 7 || std::fread(taps, sizeof(double), 80, f) != 80 || std::fread(thr, sizeof(double), 5, f) != 5 ||
            std::fread(&tol, sizeof(double), 1, f) != 1) return 65;
        const int rc = h[0] ? run_case<double>(f, h, taps, thr, tol) : run_case<float>(f, h, taps, thr, tol);
        if (rc) { std::fprintf(stderr, "case %d failed (%d)\n", c, rc); return 1; }
    }
    std::fclose(f);
    std::printf("%d cases ok\n", ncases);
    return 0;
}
