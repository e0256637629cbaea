// The cases of tests/test_emulated_joint_tile.py as a program of its own, for AddressSanitizer + UBSan (the test compiles it and
// ndwt_emu_joint_tile.cpp with -fsanitize=address,undefined and runs it as a child process).
// argv[1]: a case file the test wrote --
//   int32 ncases; per case: int32 f64, comp, vec, nb, hard; int64 n_scalars, items, pitch; double thr[nb]; double want[nb][4];
//   double tol[nb][4]; then the array and the array after the joint shrink, each (nb - 1) * pitch + items * n_scalars scalars in the
//   case's precision.
// The array after JointTile must equal the expected one bit for bit, and so must the array after JointShrink; the norms of GroupNormsTile,
// norms[b][s], must be want[b][s] within the relative tolerance tol[b][s] (0: bit for bit; a NaN for a NaN), and their max and count
// must be GroupNorms' bit for bit.
// The array is one heap block of exactly its size -- it ends with the last item of the last band -- (vec = 0 cases: one element past a
// 32-byte boundary, off the groups of 4 scalars), so a step of a loop too far is a sanitizer report; the norms leave it unchanged.
// Exit status 0: every case ran and passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

extern "C" int ndwt_emu_jt_shrink(int f64, int comp, int vec, int tile, void* y, long long pitch, long long n_scalars, long long items, int nb, const double* thr,
                                  int hard);
extern "C" int ndwt_emu_jt_norms(int f64, int comp, int vec, int tile, const void* y, long long pitch, long long n_scalars, long long items, int nb, double* out);

template <typename T> static int run_case(FILE* f, const int* h, long long n, long long items, long long pitch, const std::vector<double>& thr,
                                          const std::vector<double>& want, const std::vector<double>& tol) {
    const int vec = h[2], nb = h[3], hard = h[4];
    const size_t total = (size_t)((nb - 1) * pitch + items * n);
    std::vector<T> in(total), expect(total);
    if (std::fread(in.data(), sizeof(T), total, f) != total || std::fread(expect.data(), sizeof(T), total, f) != total) return 2;
    const size_t skew = vec == 0 ? (size_t)h[1] : 0;            // (one element: complex data lies on whole elements)
    struct Free { void operator()(T* q) const { ::operator delete(q, std::align_val_t(32)); } };
    std::unique_ptr<T, Free> block(static_cast<T*>(::operator new((total + skew) * sizeof(T), std::align_val_t(32))));
    T* const y = block.get() + skew;
    std::memcpy(y, in.data(), total * sizeof(T));
    std::unique_ptr<double[]> v(new double[(size_t)nb * 4]), old(new double[(size_t)nb * 4]);     // (exactly the results)
    if (ndwt_emu_jt_norms(h[0], h[1], vec, 1, y, pitch, n, items, nb, v.get()) != vec) return 3;
    if (ndwt_emu_jt_norms(h[0], h[1], vec, 0, y, pitch, n, items, nb, old.get()) != vec) return 3;
    if (std::memcmp(y, in.data(), total * sizeof(T)) != 0) return 5;   // the norms read only
    for (size_t i = 0; i < (size_t)nb * 4; ++i) {
        const double got = v[i], w = want[i];
        const bool ok = std::memcmp(&got, &w, sizeof(double)) == 0 || (std::isnan(got) && std::isnan(w)) || (got == w) ||
                        (tol[i] > 0 && std::fabs(got - w) <= tol[i] * std::fabs(w));
        if (!ok) {
            std::fprintf(stderr, "band %zu statistic %zu: got %.17g, want %.17g (tolerance %.3g)\n", i / 4, i % 4, got, w, tol[i]);
            return 4;
        }
        if (i % 4 >= 2 && std::memcmp(&got, &old[i], sizeof(double)) != 0) {
            std::fprintf(stderr, "band %zu statistic %zu: the tile form %.17g, the chunk form %.17g\n", i / 4, i % 4, got, old[i]);
            return 8;
        }
    }
    for (int tile = 1; tile >= 0; --tile) {
        std::memcpy(y, in.data(), total * sizeof(T));
        if (ndwt_emu_jt_shrink(h[0], h[1], vec, tile, y, pitch, n, items, nb, thr.data(), hard) != vec) return 6;
        for (size_t i = 0; i < total; ++i)
            if (std::memcmp(&y[i], &expect[i], sizeof(T)) != 0) {
                std::fprintf(stderr, "tile %d scalar %zu (band %zu): got %.17g, want %.17g, was %.17g\n", tile, i, i / (size_t)pitch, (double)y[i], (double)expect[i],
                             (double)in[i]);
                return 7;
            }
    }
    std::printf("  ok: f64 %d comp %d vec %d hard %d  %d bands of %lld items of %lld scalars, pitch %lld\n", h[0], h[1], vec, hard, nb, items, n, pitch);
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
        long long n, items, pitch;
        if (std::fread(h, sizeof(int), 5, f) != 5 || std::fread(&n, sizeof n, 1, f) != 1 || std::fread(&items, sizeof items, 1, f) != 1 ||
            std::fread(&pitch, sizeof pitch, 1, f) != 1 || n < 1 || items < 1 || h[3] < 1 || pitch < items * n) return 65;
        std::vector<double> thr((size_t)h[3]), want((size_t)h[3] * 4), tol(want.size());
        if (std::fread(thr.data(), sizeof(double), thr.size(), f) != thr.size() || std::fread(want.data(), sizeof(double), want.size(), f) != want.size() ||
            std::fread(tol.data(), sizeof(double), tol.size(), f) != tol.size()) return 65;
        const int rc = h[0] ? run_case<double>(f, h, n, items, pitch, thr, want, tol) : run_case<float>(f, h, n, items, pitch, thr, want, tol);
        if (rc) { std::fprintf(stderr, "case %d failed (%d)\n", c, rc); return 1; }
    }
    std::fclose(f);
    std::printf("%d cases ok\n", ncases);
    return 0;
}
