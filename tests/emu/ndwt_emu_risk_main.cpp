// The cases of tests/test_emulated_risk.py as a program of its own, for AddressSanitizer + UBSan (the test compiles it and
// ndwt_emu_risk.cpp with -fsanitize=address,undefined and runs it as a child process).
// argv[1]: a case file the test wrote --
//   int32 ncases; per case: int32 f64, comp, vec, chunks, nb, nc; int64 n_scalars, items, pitch; double cand[items][nb][nc];
//   double want[items][nb][nc][3]; double tol[items][nb][nc][3]; then the array: (nb - 1) * pitch + items * n_scalars scalars in the
//   case's precision.
// values must be want within the relative tolerance tol; a tolerance of 0: equal; a NaN for a NaN.
// The array is one heap block of exactly its size -- it ends with the last item of the last band -- (vec = 0 cases: one element past a
// 32-byte boundary, off the groups of 4 scalars), so a step of a loop too far is a sanitizer report; the block is compared with its copy
// afterwards.  Exit status 0: every case ran and passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

extern "C" int ndwt_emu_band_risk(int f64, int comp, int vec, const void* y, long long pitch, long long n_scalars, long long items, int nb, int chunks, int nc,
                                  const double* cand, double* out);

template <typename T> static int run_case(FILE* f, const int* h, long long n, long long items, long long pitch, const std::vector<double>& cand,
                                          const std::vector<double>& want, const std::vector<double>& tol) {
    const int nb = h[4], nc = h[5];
    const size_t total = (size_t)((nb - 1) * pitch + items * n);
    std::vector<T> in(total);
    if (std::fread(in.data(), sizeof(T), total, f) != total) return 2;
    const size_t skew = h[2] == 0 ? (size_t)h[1] : 0;           // (one element: complex data lies on whole elements)
    struct Free { void operator()(T* q) const { ::operator delete(q, std::align_val_t(32)); } };
    std::unique_ptr<T, Free> block(static_cast<T*>(::operator new((total + skew) * sizeof(T), std::align_val_t(32))));
    T* const y = block.get() + skew;
    std::memcpy(y, in.data(), total * sizeof(T));
    std::unique_ptr<double[]> c(new double[cand.size()]);           // (exactly the candidates)
    std::memcpy(c.get(), cand.data(), cand.size() * sizeof(double));
    std::unique_ptr<double[]> v(new double[want.size()]);           // (exactly the results)
    const int form = ndwt_emu_band_risk(h[0], h[1], h[2], y, pitch, n, items, nb, h[3], nc, c.get(), v.get());
    if (form != h[2]) return 3;
    if (std::memcmp(y, in.data(), total * sizeof(T)) != 0) return 5;   // the array is read only
    for (size_t i = 0; i < want.size(); ++i) {
        const double got = v[i], w = want[i];
        const bool ok = (std::isnan(got) && std::isnan(w)) || (got == w) || (tol[i] > 0 && std::fabs(got - w) <= tol[i] * std::fabs(w));
        if (!ok) {
            std::fprintf(stderr, "block %zu candidate %zu statistic %zu: got %.17g, want %.17g (tolerance %.3g)\n", i / 3 / nc, i / 3 % nc, i % 3, got, w, tol[i]);
            return 4;
        }
    }
    std::printf("  ok: f64 %d comp %d vec %d chunks %d nc %d  %d bands of %lld items of %lld scalars, pitch %lld\n", h[0], h[1], h[2], h[3], nc, nb, items, n, pitch);
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
        long long n, items, pitch;
        if (std::fread(h, sizeof(int), 6, f) != 6 || std::fread(&n, sizeof n, 1, f) != 1 || std::fread(&items, sizeof items, 1, f) != 1 ||
            std::fread(&pitch, sizeof pitch, 1, f) != 1 || n < 1 || items < 1 || h[4] < 1 || h[5] < 1 || pitch < items * n) return 65;
        std::vector<double> cand((size_t)items * h[4] * h[5]), want(cand.size() * 3), tol(want.size());
        if (std::fread(cand.data(), sizeof(double), cand.size(), f) != cand.size() || std::fread(want.data(), sizeof(double), want.size(), f) != want.size() ||
            std::fread(tol.data(), sizeof(double), tol.size(), f) != tol.size()) return 65;
        const int rc = h[0] ? run_case<double>(f, h, n, items, pitch, cand, want, tol) : run_case<float>(f, h, n, items, pitch, cand, want, tol);
        if (rc) { std::fprintf(stderr, "case %d failed (%d)\n", c, rc); return 1; }
    }
    std::fclose(f);
    std::printf("%d cases ok\n", ncases);
    return 0;
}
