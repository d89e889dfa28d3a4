/* Stand-in for the seven vDSP entry points the reference calls (decimator.cpp, fftaccelerate.cpp), written from
 * Apple's public documentation of their semantics.  Plain loops, left-to-right summation, and a standard
 * unscaled DFT (forward e^{-j}, inverse e^{+j}).  These are OUR arithmetic: the reference pins hold the code
 * around them, not these two primitives (the strided FIR and the DFT). */
#ifndef PEBBLE_ORACLE_ACCELERATE_STANDIN_H
#define PEBBLE_ORACLE_ACCELERATE_STANDIN_H
#include <cstddef>
typedef unsigned long vDSP_Length;
typedef long vDSP_Stride;
typedef struct { double real, imag; } DSPDoubleComplex;
typedef struct { double *realp, *imagp; } DSPDoubleSplitComplex;
typedef struct vdsp_fftsetup_standin *FFTSetupD;
typedef int FFTRadix;
typedef int FFTDirection;
enum { FFT_RADIX2 = 0 };
enum { kFFTDirection_Forward = +1, kFFTDirection_Inverse = -1 };

/* interleaved -> split; ic counts doubles (2 = every complex element) */
void vDSP_ctozD(const DSPDoubleComplex *c, vDSP_Stride ic, const DSPDoubleSplitComplex *z, vDSP_Stride iz, vDSP_Length n);
void vDSP_ztocD(const DSPDoubleSplitComplex *z, vDSP_Stride iz, DSPDoubleComplex *c, vDSP_Stride ic, vDSP_Length n);
void vDSP_zvmovD(const DSPDoubleSplitComplex *a, vDSP_Stride ia, const DSPDoubleSplitComplex *c, vDSP_Stride ic, vDSP_Length n);
/* c = sum_{i<n} a[i*ia] * b[i*ib] */
void vDSP_zrdotprD(const DSPDoubleSplitComplex *a, vDSP_Stride ia, const double *b, vDSP_Stride ib, const DSPDoubleSplitComplex *c,
                   vDSP_Length n);
/* c[i] = sum_{p<P} a[i*df + p] * f[p],  i < n */
void vDSP_zrdesampD(const DSPDoubleSplitComplex *a, vDSP_Stride df, const double *f, const DSPDoubleSplitComplex *c, vDSP_Length n,
                    vDSP_Length p);
FFTSetupD vDSP_create_fftsetupD(vDSP_Length log2n, FFTRadix radix);
void vDSP_destroy_fftsetupD(FFTSetupD s);
/* in-place complex transform of 2^log2n points, unscaled in both directions; the temporary buffer is not needed */
void vDSP_fft_ziptD(FFTSetupD s, const DSPDoubleSplitComplex *c, vDSP_Stride ic, const DSPDoubleSplitComplex *tmp, vDSP_Length log2n,
                    FFTDirection dir);
#endif
