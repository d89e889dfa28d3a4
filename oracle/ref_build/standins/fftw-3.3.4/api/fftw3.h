/* stand-in: the FFTW back end is not built; its wrapper's header only needs these two names to parse */
#ifndef PEBBLE_ORACLE_FFTW3_STANDIN_H
#define PEBBLE_ORACLE_FFTW3_STANDIN_H
typedef double fftw_complex[2];
typedef struct fftw_plan_standin *fftw_plan;
#endif
