/* A plain DFT behind the seven FFTW symbols of fftw3.h -- TEST INFRASTRUCTURE ONLY (oracle/Makefile, target `ref`).
 *
 * It lets mex/nddwt.c of the reference compile and run unchanged on a host without FFTW, so that the tests can compare the oracle and
 * the HIP kernels with the reference's own C control flow.  What it implements is what that file asks for and nothing more:
 *   - a guru split plan records rank, n, is, os and ONE howmany dimension;
 *   - execute is the forward DFT (sign -1) along every axis in turn.  The caller gets the unnormalised inverse the FFTW way, by swapping
 *     the real and imaginary pointers;
 *   - every line is an O(n^2) sum over a per-length twiddle table computed once per plan in long double, accumulated in long double and
 *     rounded to double on store.  No FFT: the shapes of the tests are small, and a direct sum has nothing to get wrong but its index;
 *   - the thread calls do nothing.
 * tests/test_reference_c.py checks it against numpy.fft.fftn on its own, before anything is concluded from the reference built on it. */
#include <math.h>
#include <stdlib.h>

#include "fftw3.h"

#define NDWT_REF_MAX_RANK 8

struct ndwt_ref_plan_s {
    int rank;
    int n[NDWT_REF_MAX_RANK], is[NDWT_REF_MAX_RANK], os[NDWT_REF_MAX_RANK];
    int hn, his, hos;                       /* the one howmany dimension */
    long double *wr[NDWT_REF_MAX_RANK];     /* wr[a][k] + i wi[a][k] = exp(-2 pi i k / n[a]) */
    long double *wi[NDWT_REF_MAX_RANK];
    long double *lr, *li;                   /* one gathered line */
};

void fftw_destroy_plan(fftw_plan p) {
    if (!p) return;
    for (int a = 0; a < p->rank; a++) {
        free(p->wr[a]);
        free(p->wi[a]);
    }
    free(p->lr);
    free(p->li);
    free(p);
}

fftw_plan fftw_plan_guru_split_dft(int rank, const fftw_iodim *dims, int howmany_rank, const fftw_iodim *howmany_dims,
                                   double *ri, double *ii, double *ro, double *io, unsigned flags) {
    (void)ri; (void)ii; (void)ro; (void)io; (void)flags;            /* FFTW_ESTIMATE plans touch no data; neither does this */
    if (rank < 1 || rank > NDWT_REF_MAX_RANK || howmany_rank < 0 || howmany_rank > 1) return NULL;
    fftw_plan p = (fftw_plan)calloc(1, sizeof(*p));
    if (!p) return NULL;
    const long double two_pi = 8.0L * atanl(1.0L);
    int nmax = 1;
    p->rank = rank;
    for (int a = 0; a < rank; a++) {
        int n = dims[a].n;
        if (n < 1) { fftw_destroy_plan(p); return NULL; }
        p->n[a] = n;
        p->is[a] = dims[a].is;
        p->os[a] = dims[a].os;
        if (n > nmax) nmax = n;
        p->wr[a] = (long double *)malloc(sizeof(long double) * (size_t)n);
        p->wi[a] = (long double *)malloc(sizeof(long double) * (size_t)n);
        if (!p->wr[a] || !p->wi[a]) { fftw_destroy_plan(p); return NULL; }
        for (int k = 0; k < n; k++) {
            long double ang = two_pi * (long double)k / (long double)n;
            p->wr[a][k] = cosl(ang);
            p->wi[a][k] = -sinl(ang);
        }
    }
    p->hn = howmany_rank ? howmany_dims[0].n : 1;
    p->his = howmany_rank ? howmany_dims[0].is : 0;
    p->hos = howmany_rank ? howmany_dims[0].os : 0;
    p->lr = (long double *)malloc(sizeof(long double) * (size_t)nmax);
    p->li = (long double *)malloc(sizeof(long double) * (size_t)nmax);
    if (!p->lr || !p->li || p->hn < 1) { fftw_destroy_plan(p); return NULL; }
    return p;
}

/* offset of element `idx` of the rank-dimensional index space, axis `skip` left at 0 (skip = -1: no axis left out), first axis fastest */
static long offset_of(const struct ndwt_ref_plan_s *p, long idx, int skip, const int *stride) {
    long off = 0;
    for (int b = 0; b < p->rank; b++) {
        if (b == skip) continue;
        off += (idx % p->n[b]) * (long)stride[b];
        idx /= p->n[b];
    }
    return off;
}

static void dft_line(const struct ndwt_ref_plan_s *p, int a, double *re, double *im) {
    const int n = p->n[a];
    const long s = p->os[a];
    const long double *wr = p->wr[a], *wi = p->wi[a];
    long double *lr = p->lr, *li = p->li;
    for (int j = 0; j < n; j++) {
        lr[j] = re[j * s];
        li[j] = im[j * s];
    }
    for (int k = 0; k < n; k++) {
        long double sr = 0.0L, si = 0.0L;
        int t = 0;                                                  /* (j * k) mod n */
        for (int j = 0; j < n; j++) {
            sr += lr[j] * wr[t] - li[j] * wi[t];
            si += lr[j] * wi[t] + li[j] * wr[t];
            t += k;
            if (t >= n) t -= n;
        }
        re[k * s] = (double)sr;
        im[k * s] = (double)si;
    }
}

void fftw_execute_split_dft(const fftw_plan p, double *ri, double *ii, double *ro, double *io) {
    if (!p) return;
    long numel = 1;
    for (int a = 0; a < p->rank; a++) numel *= p->n[a];
    for (int h = 0; h < p->hn; h++) {
        double *re = ro + (long)h * p->hos, *im = io + (long)h * p->hos;
        if (ro != ri || io != ii) {                                 /* out of place: copy, then transform the output where it lies */
            const double *sr = ri + (long)h * p->his, *si = ii + (long)h * p->his;
            for (long e = 0; e < numel; e++) {
                long oi = offset_of(p, e, -1, p->is), oo = offset_of(p, e, -1, p->os);
                re[oo] = sr[oi];
                im[oo] = si[oi];
            }
        }
        for (int a = 0; a < p->rank; a++) {
            if (p->n[a] == 1) continue;
            long lines = numel / p->n[a];
            for (long l = 0; l < lines; l++) {
                long off = offset_of(p, l, a, p->os);
                dft_line(p, a, re + off, im + off);
            }
        }
    }
}

int fftw_init_threads(void) { return 1; }

void fftw_plan_with_nthreads(int nthreads) { (void)nthreads; }
