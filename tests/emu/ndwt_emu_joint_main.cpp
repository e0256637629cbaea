// The cases of tests/test_emulated_joint.py as a program of its own, for AddressSanitizer + UBSan (the test compiles it and
// ndwt_emu_joint.cpp with -fsanitize=address,undefined and runs it as a child process).
// argv[1]: a case file the test wrote --
//   int32 ncases; per case: int32 f64, comp, vec, reg, chunks, nb, hard; int64 n_scalars, items, pitch; double thr[nb];
//   double want[nb][4]; double tol[nb][4]; then the array and the array after the joint shrink, each (nb - 1) * pitch + items * n_scalars
//   scalars in the case's precision.
// The shrunk array must equal the expected one bit for bit; the group norms of the array, norms[b][s], must be want[b][s] within the
// relative tolerance tol[b][s]; a tolerance of 0: bit for bit; a NaN for a NaN.
// The array is one heap block of exactly its size -- it ends with the last item of the last band -- (vec = 0 cases: one element past a
// 32-byte boundary, off the groups of 4 scalars), so a step of a loop too far is a sanitizer report; the norms leave it unchanged.
// Exit status 0: every case ran and passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

extern "C" int ndwt_emu_joint_shrink(int f64, int comp, int vec, int reg, void* y, long long pitch, long long n_scalars, long long items, int nb, int chunks,
                                     const double* thr, int hard);
extern "C" int ndwt_emu_group_norms(int f64, int comp, int vec, const void* y, long long pitch, long long n_scalars, long long items, int nb, int chunks,
                                    double* out);

template <typename T> static int run_case(FILE* f, const int* h, long long n, long long items, long long pitch, const std::vector<double>& thr,
                                          const std::vector<double>& want, const std::vector<double>& tol) {
    const int vec = h[2], reg = h[3], chunks = h[4], nb = h[5], hard = h[6];
    const size_t total = (size_t)((nb - 1) * pitch + items * n);
    std::vector<T> in(total), expect(total);
    if (std::fread(in.data(), sizeof(T), total, f) != total || std::fread(expect.data(), sizeof(T), total, f) != total) return 2;
    const size_t skew = vec == 0 ? (size_t)h[1] : 0;            // (one element: complex data lies on whole elements)
    struct Free { void operator()(T* q) const { ::operator delete(q, std::align_val_t(32)); } };
    std::unique_ptr<T, Free> block(static_cast<T*>(::operator new((total + skew) * sizeof(T), std::align_val_t(32))));
    T* const y = block.get() + skew;
    std::memcpy(y, in.data(), total * sizeof(T));
    std::unique_ptr<double[]> v(new double[(size_t)nb * 4]);     // (exactly the results)
    if (ndwt_emu_group_norms(h[0], h[1], vec, y, pitch, n, items, nb, chunks, v.get()) != vec) return 3;
    if (std::memcmp(y, in.data(), total * sizeof(T)) != 0) return 5;   // the norms read only
    for (size_t i = 0; i < (size_t)nb * 4; ++i) {
        const double got = v[i], w = want[i];
        const bool ok = std::memcmp(&got, &w, sizeof(double)) == 0 || (std::isnan(got) && std::isnan(w)) || (got == w) ||
                        (tol[i] > 0 && std::fabs(got - w) <= tol[i] * std::fabs(w));
        if (!ok) {
            std::fprintf(stderr, "band %zu statistic %zu: got %.17g, want %.17g (tolerance %.3g)\n", i / 4, i % 4, got, w, tol[i]);
            return 4;
        }
    }
    if (ndwt_emu_joint_shrink(h[0], h[1], vec, reg, y, pitch, n, items, nb, chunks, thr.data(), hard) != vec + 2 * reg) return 6;
    for (size_t i = 0; i < total; ++i)
        if (std::memcmp(&y[i], &expect[i], sizeof(T)) != 0) {
            std::fprintf(stderr, "scalar %zu (band %zu): got %.17g, want %.17g, was %.17g\n", i, i / (size_t)pitch, (double)y[i], (double)expect[i], (double)in[i]);
            return 7;
        }
    std::printf("  ok: f64 %d comp %d vec %d reg %d chunks %d hard %d  %d bands of %lld items of %lld scalars, pitch %lld\n", h[0], h[1], vec, reg, chunks, hard,
                nb, items, n, pitch);
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
        long long n, items, pitch;
        if (std::fread(h, sizeof(int), 7, f) != 7 || std::fread(&n, sizeof n, 1, f) != 1 || std::fread(&items, sizeof items, 1, f) != 1 ||
            std::fread(&pitch, sizeof pitch, 1, f) != 1 || n < 1 || items < 1 || h[5] < 1 || pitch < items * n) return 65;
        std::vector<double> thr((size_t)h[5]), want((size_t)h[5] * 4), tol(want.size());
        if (std::fread(thr.data(), sizeof(double), thr.size(), f) != thr.size() || std::fread(want.data(), sizeof(double), want.size(), f) != want.size() ||
            std::fread(tol.data(), sizeof(double), tol.size(), f) != tol.size()) return 65;
        const int rc = h[0] ? run_case<double>(f, h, n, items, pitch, thr, want, tol) : run_case<float>(f, h, n, items, pitch, thr, want, tol);
        if (rc) { std::fprintf(stderr, "case %d failed (%d)\n", c, rc); return 1; }
    }
    std::fclose(f);
    std::printf("%d cases ok\n", ncases);
    return 0;
}
