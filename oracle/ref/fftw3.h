/* The seven FFTW symbols mex/nddwt.c of the reference uses, declared with FFTW 3's public signatures, so that the reference file compiles
 * unchanged without FFTW (oracle/Makefile, target `ref`).  fftw_split_dft.c defines them with a plain long-double DFT.
 * TEST INFRASTRUCTURE ONLY: nothing the package ships includes or links this. */
#ifndef NDWT_REF_FFTW3_H
#define NDWT_REF_FFTW3_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ndwt_ref_plan_s *fftw_plan;

typedef struct {
    int n;  /* length of the dimension */
    int is; /* input stride, in doubles */
    int os; /* output stride */
} fftw_iodim;

#define FFTW_ESTIMATE (1U << 6)

fftw_plan fftw_plan_guru_split_dft(int rank, const fftw_iodim *dims, int howmany_rank, const fftw_iodim *howmany_dims,
                                   double *ri, double *ii, double *ro, double *io, unsigned flags);
void fftw_execute_split_dft(const fftw_plan p, double *ri, double *ii, double *ro, double *io);
void fftw_destroy_plan(fftw_plan p);
int fftw_init_threads(void);
void fftw_plan_with_nthreads(int nthreads);

#ifdef __cplusplus
}
#endif
#endif
