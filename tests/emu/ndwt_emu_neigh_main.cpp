// The cases of tests/test_emulated_neigh.py as a program of its own, for AddressSanitizer + UBSan (the test compiles it and
// ndwt_emu_neigh.cpp with -fsanitize=address,undefined and runs it as a child process).
// argv[1]: a case file the test wrote (tests/neigh_cases.py: pack_case) --
//   int32 ncases; per case: int32 f64, comp, nd, r, hard, nb, ntx, nty, chunk, nchunks, n0, n1, n2; int64 items, lead, pitch;
//   double thr[nb]; then the array and the expected output, each lead + nb * pitch scalars in the case's precision: `lead` guard
//   scalars, then the bands.
// The input and the output are heap blocks of exactly (nb - 1) * pitch + items * n scalars each -- they begin with band 0 and end with
// the last item of the last band -- so a step of a loop too far, on either side, is a sanitizer report.  The output starts as the
// expected buffer's guard value everywhere; afterwards it must equal the expected output bit for bit, the scalars between the bands
// included, and the input must be unchanged.  Exit status 0: every case ran and passed.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

extern "C" int ndwt_emu_neigh_shrink(int f64, int comp, int nd, int r, const void* y, void* out, long long pitch, const int* n, long long items, int nb,
                                     const int* geom, const double* thr, int hard);

template <typename T> static int run_case(FILE* f, const int* h, long long items, long long lead, long long pitch, const std::vector<double>& thr) {
    const int comp = h[1], nd = h[2], r = h[3], hard = h[4], nb = h[5];
    const long long n = (long long)h[10] * h[11] * h[12] * comp;
    const size_t file_total = (size_t)(lead + nb * pitch), total = (size_t)((nb - 1) * pitch + items * n);
    std::vector<T> in(file_total), expect(file_total);
    if (std::fread(in.data(), sizeof(T), file_total, f) != file_total || std::fread(expect.data(), sizeof(T), file_total, f) != file_total) return 2;
    std::unique_ptr<T[]> y(new T[total]), out(new T[total]);       // (exactly the arrays)
    std::memcpy(y.get(), in.data() + lead, total * sizeof(T));
    for (size_t i = 0; i < total; ++i) out[i] = expect[0];         // (the leading guard of the expected buffer: its fill value)
    if (ndwt_emu_neigh_shrink(h[0], comp, nd, r, y.get(), out.get(), pitch, h + 10, items, nb, h + 6, thr.data(), hard) != 0) return 3;
    if (std::memcmp(y.get(), in.data() + lead, total * sizeof(T)) != 0) return 5;   // the input is read only
    for (size_t i = 0; i < total; ++i)
        if (std::memcmp(&out[i], &expect[lead + i], sizeof(T)) != 0) {
            std::fprintf(stderr, "scalar %zu (band %zu, offset %zu): got %.17g, want %.17g, was %.17g\n", i, i / (size_t)pitch, i % (size_t)pitch, (double)out[i],
                         (double)expect[lead + i], (double)y[i]);
            return 7;
        }
    std::printf("  ok: f64 %d comp %d nd %d r %d hard %d  %d bands of %lld items of %d x %d x %d, pitch %lld, tiles %d x %d, %d chunks of %d\n", h[0], comp, nd, r, hard,
                nb, items, h[10], h[11], h[12], pitch, h[6], h[7], h[9], h[8]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 64; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 66; }
    int ncases = 0;
    if (std::fread(&ncases, sizeof(int), 1, f) != 1 || ncases < 1) return 65;
    for (int c = 0; c < ncases; ++c) {
        int h[13];
        long long q[3];
        if (std::fread(h, sizeof(int), 13, f) != 13 || std::fread(q, sizeof(long long), 3, f) != 3 || h[5] < 1 || q[0] < 1 || q[1] < 0 ||
            q[2] < q[0] * h[10] * h[11] * h[12] * h[1])
            return 65;
        std::vector<double> thr((size_t)h[5]);
        if (std::fread(thr.data(), sizeof(double), thr.size(), f) != thr.size()) return 65;
        const int rc = h[0] ? run_case<double>(f, h, q[0], q[1], q[2], thr) : run_case<float>(f, h, q[0], q[1], q[2], thr);
        if (rc) { std::fprintf(stderr, "case %d failed (%d)\n", c, rc); return 1; }
    }
    std::fclose(f);
    std::printf("%d cases ok\n", ncases);
    return 0;
}
