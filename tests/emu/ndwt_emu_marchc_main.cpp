// The cases of tests/test_emulated_marchc.py as a program of its own, for AddressSanitizer + UBSan (the test compiles it with
// -fsanitize=address,undefined, links it with ndwt_emu_marchc.cpp built the same way, and runs it as a child process).
// argv[1]: a case file the test wrote --
//   int32 ncases; per case: int32 inverse, f64, L, nlev, inner, n, outer, chunk; double lo[20], hi[20], tol;
//   the input (outer x n x inner scalars, or its 1 + nlev bands), then the expected output, in the case's precision.
// Every buffer is a heap block of exactly its size, so a group, a plane, an item or a band too far is a sanitizer report.  Exit status
// 0: every case ran and agrees with its expected output to its tolerance.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

extern "C" int ndwt_emu_marchc(int inverse, int f64, int L, int nlev, const void* in, void* out, long long inner, long long n, long long outer,
                               int chunk, const double* lo, const double* hi);

template <typename T> static int run_case(FILE* f, const int* h, const double* lo, const double* hi, double tol) {
    const int inverse = h[0], nlev = h[3];
    const size_t vol = (size_t)h[4] * (size_t)h[5] * (size_t)h[6], nin = inverse ? vol * (1 + nlev) : vol, nout = inverse ? vol : vol * (1 + nlev);
    std::vector<T> in(nin), want(nout);
    if (std::fread(in.data(), sizeof(T), nin, f) != nin || std::fread(want.data(), sizeof(T), nout, f) != nout) return 2;
    std::unique_ptr<T[]> src(new T[nin]), out(new T[nout]);
    std::memcpy(src.get(), in.data(), nin * sizeof(T));
    for (size_t i = 0; i < nout; ++i) out[i] = std::nan("");
    if (ndwt_emu_marchc(inverse, h[1], h[2], nlev, src.get(), out.get(), h[4], h[5], h[6], h[7], lo, hi) != 0) return 3;
    double worst = 0;
    for (size_t i = 0; i < nout; ++i) {
        const double d = std::fabs((double)out[i] - (double)want[i]);
        if (!(d <= tol)) { std::fprintf(stderr, "element %zu: got %g, want %g (tolerance %g)\n", i, (double)out[i], (double)want[i], tol); return 4; }
        worst = d > worst ? d : worst;
    }
    std::printf("  ok: inverse %d f64 %d L %d nlev %d  %d scalars x %d planes x %d items, chunk %d  max error %.3g (tolerance %.3g)\n", h[0], h[1], h[2],
                h[3], h[4], h[5], h[6], h[7], worst, tol);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 64; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 66; }
    int ncases = 0;
    if (std::fread(&ncases, sizeof(int), 1, f) != 1 || ncases < 1) return 65;
    for (int c = 0; c < ncases; ++c) {
        int h[8];
        double lo[20], hi[20], tol;
        if (std::fread(h, sizeof(int), 8, f) != 8 || std::fread(lo, sizeof(double), 20, f) != 20 || std::fread(hi, sizeof(double), 20, f) != 20 ||
            std::fread(&tol, sizeof(double), 1, f) != 1) return 65;
        const int rc = h[1] ? run_case<double>(f, h, lo, hi, tol) : run_case<float>(f, h, lo, hi, tol);
        if (rc) { std::fprintf(stderr, "case %d failed (%d)\n", c, rc); return 1; }
    }
    std::fclose(f);
    std::printf("%d cases ok\n", ncases);
    return 0;
}
