/* See Accelerate.h: plain-loop stand-ins for seven vDSP functions. */
#include "Accelerate.h"
#include <cmath>
#include <vector>

void vDSP_ctozD(const DSPDoubleComplex *c, vDSP_Stride ic, const DSPDoubleSplitComplex *z, vDSP_Stride iz, vDSP_Length n)
{
    const double *d = (const double *)c;
    for (vDSP_Length i = 0; i < n; i++) {
        z->realp[i * iz] = d[i * ic];
        z->imagp[i * iz] = d[i * ic + 1];
    }
}

void vDSP_ztocD(const DSPDoubleSplitComplex *z, vDSP_Stride iz, DSPDoubleComplex *c, vDSP_Stride ic, vDSP_Length n)
{
    double *d = (double *)c;
    for (vDSP_Length i = 0; i < n; i++) {
        d[i * ic] = z->realp[i * iz];
        d[i * ic + 1] = z->imagp[i * iz];
    }
}

void vDSP_zvmovD(const DSPDoubleSplitComplex *a, vDSP_Stride ia, const DSPDoubleSplitComplex *c, vDSP_Stride ic, vDSP_Length n)
{
    /* ascending copy; the reference's uses move towards lower addresses or between separate buffers */
    for (vDSP_Length i = 0; i < n; i++) {
        c->realp[i * ic] = a->realp[i * ia];
        c->imagp[i * ic] = a->imagp[i * ia];
    }
}

void vDSP_zrdotprD(const DSPDoubleSplitComplex *a, vDSP_Stride ia, const double *b, vDSP_Stride ib, const DSPDoubleSplitComplex *c,
                   vDSP_Length n)
{
    double re = 0.0, im = 0.0;
    for (vDSP_Length i = 0; i < n; i++) {
        re += a->realp[i * ia] * b[i * ib];
        im += a->imagp[i * ia] * b[i * ib];
    }
    c->realp[0] = re;
    c->imagp[0] = im;
}

void vDSP_zrdesampD(const DSPDoubleSplitComplex *a, vDSP_Stride df, const double *f, const DSPDoubleSplitComplex *c, vDSP_Length n,
                    vDSP_Length p)
{
    for (vDSP_Length i = 0; i < n; i++) {
        double re = 0.0, im = 0.0;
        for (vDSP_Length k = 0; k < p; k++) {
            re += a->realp[i * df + k] * f[k];
            im += a->imagp[i * df + k] * f[k];
        }
        c->realp[i] = re;
        c->imagp[i] = im;
    }
}

struct vdsp_fftsetup_standin {
    vDSP_Length log2n;
    std::vector<double> wr, wi; /* e^{-j 2 pi k / N}, k < N/2, N = 2^log2n */
};

FFTSetupD vDSP_create_fftsetupD(vDSP_Length log2n, FFTRadix)
{
    vdsp_fftsetup_standin *s = new vdsp_fftsetup_standin;
    s->log2n = log2n;
    size_t n = size_t(1) << log2n;
    s->wr.resize(n / 2 + 1);
    s->wi.resize(n / 2 + 1);
    for (size_t k = 0; k < n / 2; k++) {
        double a = -2.0 * M_PI * double(k) / double(n);
        s->wr[k] = cos(a);
        s->wi[k] = sin(a);
    }
    return s;
}

void vDSP_destroy_fftsetupD(FFTSetupD s) { delete s; }

/* textbook iterative radix-2 decimation in time */
void vDSP_fft_ziptD(FFTSetupD s, const DSPDoubleSplitComplex *c, vDSP_Stride ic, const DSPDoubleSplitComplex *, vDSP_Length log2n,
                    FFTDirection dir)
{
    size_t n = size_t(1) << log2n;
    size_t tstep = (size_t(1) << s->log2n) / n; /* a setup serves every size up to its own */
    double *re = c->realp, *im = c->imagp;
    for (size_t i = 1, j = 0; i < n; i++) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1)
            j ^= bit;
        j ^= bit;
        if (i < j) {
            double t = re[i * ic]; re[i * ic] = re[j * ic]; re[j * ic] = t;
            t = im[i * ic]; im[i * ic] = im[j * ic]; im[j * ic] = t;
        }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        size_t half = len / 2, step = n / len * tstep;
        for (size_t base = 0; base < n; base += len) {
            for (size_t k = 0; k < half; k++) {
                double wr = s->wr[k * step], wi = (dir == kFFTDirection_Forward) ? s->wi[k * step] : -s->wi[k * step];
                size_t p = (base + k) * ic, q = (base + k + half) * ic;
                double tr = re[q] * wr - im[q] * wi, ti = re[q] * wi + im[q] * wr;
                re[q] = re[p] - tr; im[q] = im[p] - ti;
                re[p] = re[p] + tr; im[p] = im[p] + ti;
            }
        }
    }
}
