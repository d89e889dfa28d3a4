// kernels_fastfir.h -- CFastFIR::ProcessData (pebblelib/fastfir.cpp:281-334) as batched overlap-save.
//
// One workgroup per (block, channel): gather N = L + (taps-1) samples [overlap | L new] straight into
// the strided register layout, forward FFT, multiply by the channel's H (1/N already folded into the
// taps, fastfir.cpp:244-245), inverse FFT, keep samples taps-1 .. N-1.  Forward-last and inverse-first
// passes share the register layout (fft_lds.h), so the product needs no exchange.
//
// The input buffer carries taps-1 samples of head-room holding the previous call's tail, which is
// exactly m_pFFTOverlapBuf (zero before the first call, fastfir.cpp:104-105).  A caller-owned buffer
// without head-room passes `tail` instead ([channel][taps-1], refreshed by the host side after the call).
//
// taps-1 <= L (FastFirCore::init refuses longer filters): block b >= 1 starts at b L - (taps-1) >= 0, inside its own row, so with `tail`
// only block 0 looks in front of the row, and it takes those samples from `tail`.
//
// Bound: HBM.  Algorithmic bytes per demod-rate sample: 8 read + 8 written (+ H once per block: with
// taps-1 = N/2 the overlap doubles the read to 16 B unless L2 serves the second touch).
#pragma once
#include "fft_lds.h"
#include "fft_t128.h"
#include "mixer_osc.h"
#include "params.h"

namespace pg {

template <int N>
__global__ __launch_bounds__(256) void k_fastfir(const float2 *__restrict__ in, long long in_pitch,
                                                  float2 *__restrict__ out, long long out_pitch,
                                                  const float2 *__restrict__ H, const float2 *__restrict__ tw,
                                                  int overlap /* taps-1 */, const float2 *__restrict__ tail)
{
    constexpr int E = N / 256;
    __shared__ float2 lds[FftLds<N>::kSlots];
    const int tid = threadIdx.x, c = blockIdx.y;
    const int L = N - overlap;
    const long long b = blockIdx.x;
    const float2 *x = in + (long long)c * in_pitch + b * L - overlap;  // first sample of [overlap | new]
    const float2 *h = H + (long long)c * N;
    float2 v[E];
    if (tail != nullptr && b == 0) {  // caller's buffer has no head-room: the overlap of block 0 lives in `tail` [c][overlap]
        const float2 *t = tail + (long long)c * overlap;
#pragma unroll
        for (int m = 0; m < E; m++) {
            const int i = tid + 256 * m;
            v[m] = i < overlap ? t[i] : x[i];
        }
    } else {
#pragma unroll
        for (int m = 0; m < E; m++) v[m] = x[tid + 256 * m];
    }
    fft_regs<N, +1>(v, lds, tw, tid);
#pragma unroll
    for (int m = 0; m < E; m++) v[m] = cmul(h[tid + 256 * m], v[m]);  // CpxMpy, fastfir.cpp:325-334
    fft_regs<N, -1>(v, lds, tw, tid);
    float2 *y = out + (long long)c * out_pitch + b * L;
#pragma unroll
    for (int m = 0; m < E; m++) {
        const int i = tid + 256 * m;
        if (i >= overlap) y[i - overlap] = v[m];
    }
}

// The 2048/1025 case (the reference's stock sizes) on the two-wave transform: a 128-item workgroup per block, 16 points
// per work-item, barriers that only involve its own two waves.  The inverse transform is the forward one between two
// conjugations.  grid (n / L, channels), block 128.
template <bool TWLDS = true>
static __global__ __launch_bounds__(128) void k_fastfir_t128(const float2 *__restrict__ in, long long in_pitch,
                                                             float2 *__restrict__ out, long long out_pitch,
                                                             const float2 *__restrict__ H, const float2 *__restrict__ tw128,
                                                             int overlap /* taps-1 */, const float2 *__restrict__ tail,
                                                             float2 *__restrict__ tail_out /* or null: [c][overlap] receives the call's last `overlap` input samples */,
                                                             int nb, int nchan)
{
    constexpr int N = 2048, E = 16;
    __shared__ float2 lds[FftLds<N>::kSlots];
    __shared__ float2 tw_lds_[TWLDS ? kTw128Count : 1];
    const float2 *tw_lds = TWLDS ? tw_lds_ : tw128;  // (A/B: the twiddle table read through the vector cache instead of a copy per workgroup)
    const int t = threadIdx.x;
    const int L = N - overlap;
    // Workgroup -> (block, channel).  A block's window repeats the `overlap` samples in front of it, which are the previous block's new
    // samples, and every block of a channel reads the channel's 16 KiB of H: with (block, channel) = (blockIdx.x, blockIdx.y) consecutive
    // blocks go to consecutive XCDs -- eight separate L2s -- and both come from HBM again.  nchan > 0 (a one-dimensional grid): the
    // workgroup id's low three bits are the XCD; each XCD walks ITS eighth of the blocks in (channel, block) order, so a block's neighbour
    // and its H are in the same L2 a moment before it.
    int c;
    long long b;
    if (nchan > 0) {
        const long long total = (long long)nb * nchan, per = (total + 7) >> 3;
        const long long q = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
        if ((long long)(blockIdx.x >> 3) >= per || q >= total) return;  // (uniform: the whole workgroup)
        c = (int)(q / nb);
        b = q - (long long)c * nb;
    } else {
        c = blockIdx.y;
        b = blockIdx.x;
        nb = (int)gridDim.x;
    }
    const float2 *x = in + (long long)c * in_pitch + b * L - overlap;  // first sample of [overlap | new]
    const float2 *h = H + (long long)c * N;
    if (TWLDS) for (int i = t; i < kTw128Count; i += 128) tw_lds_[i] = tw128[i];
    float2 v[E];
    if (tail != nullptr && b == 0) {
        const float2 *tl = tail + (long long)c * overlap;
#pragma unroll
        for (int m = 0; m < E; m++) {
            const int i = t + 128 * m;
            v[m] = i < overlap ? tl[i] : x[i];
        }
    } else {
#pragma unroll
        for (int m = 0; m < E; m++) v[m] = x[t + 128 * m];
    }
    if (tail_out != nullptr && b == (long long)nb - 1) {
        // m_pFFTOverlapBuf for the next call (fastfir.cpp:312-316): the last block's window ends with them.  A different buffer
        // from `tail`, which block 0 of this launch may still be reading
        float2 *to = tail_out + (long long)c * overlap;
#pragma unroll
        for (int m = 0; m < E; m++) {
            const int i = t + 128 * m;
            if (i >= L) to[i - L] = v[m];
        }
    }
    __syncthreads();
    fft2048_t128(v, lds, tw_lds, t, [] { __syncthreads(); });
#pragma unroll
    for (int m = 0; m < E; m++) {
        const float2 p = cmul(h[t + 128 * m], v[m]);  // CpxMpy, fastfir.cpp:325-334
        v[m] = make_float2(p.x, -p.y);                // conj: IFFT(z) = conj(FFT(conj(z))), unscaled (1/N is in the taps)
    }
    fft2048_t128(v, lds, tw_lds, t, [] { __syncthreads(); });  // (the forward transform ends behind a barrier: the image is free)
    float2 *y = out + (long long)c * out_pitch + b * L;
#pragma unroll
    for (int m = 0; m < E; m++) {
        const int i = t + 128 * m;
        if (i >= overlap) y[i - overlap] = make_float2(v[m].x, -v[m].y);
    }
}

// k_fastfir_t128 for the stream bank's raw calls: the new samples are read in the device's own sample format (RawSrc,
// pebblegpu_iq_format FMT; `in_pitch` counts IQ pairs) and converted in the load, point by point in the same t + 128 m layout -- a wave
// instruction fetches 64 adjacent pairs (128 bytes of int8 pairs, 256 of int16): as many load instructions as the float2 kernel issues,
// for a quarter or half of the bytes, and no exchange in front of the transform.  raw_load1 rounds the product with the scale on its
// own: the first butterfly ADDS converted samples, and a fused multiply-add there would differ from the float2 route in the last bit.
// The overlap of block 0 still comes from the float2 `tail` (never null here: it lies in front of the caller's buffer), and `tail_out`
// receives CONVERTED samples, so raw and float2 calls continue each other exactly.  Twiddles through the vector cache, as the stream
// bank's float2 default.  A kernel of its own rather than a parameter of the one above: written as one body with two entry points,
// k_fastfir_t128<false> came out at 126 registers instead of 96, and the receivers run that instance.
template <int FMT>
static __global__ __launch_bounds__(128) void k_fastfir_t128_raw(long long in_pitch, float2 *__restrict__ out, long long out_pitch,
                                                                 const float2 *__restrict__ H, const float2 *__restrict__ tw128,
                                                                 int overlap /* taps-1 */, const float2 *__restrict__ tail,
                                                                 float2 *__restrict__ tail_out /* or null, as above */,
                                                                 int nb, int nchan, RawSrc raw)
{
    constexpr int N = 2048, E = 16;
    __shared__ float2 lds[FftLds<N>::kSlots];
    const int t = threadIdx.x;
    const int L = N - overlap;
    int c;
    long long b;
    if (nchan > 0) {  // the XCD-ordered one-dimensional grid, as above
        const long long total = (long long)nb * nchan, per = (total + 7) >> 3;
        const long long q = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
        if ((long long)(blockIdx.x >> 3) >= per || q >= total) return;  // (uniform: the whole workgroup)
        c = (int)(q / nb);
        b = q - (long long)c * nb;
    } else {
        c = blockIdx.y;
        b = blockIdx.x;
        nb = (int)gridDim.x;
    }
    const long long x0 = (long long)c * in_pitch + b * L - overlap;  // first sample of [overlap | new]
    const float2 *h = H + (long long)c * N;
    float2 v[E];
    if (b == 0) {
        const float2 *tl = tail + (long long)c * overlap;
#pragma unroll
        for (int m = 0; m < E; m++) {
            const int i = t + 128 * m;
            if (i < overlap) v[m] = tl[i];
            else v[m] = raw_load1<FMT>(raw, x0 + i);  // (i >= overlap: x0 + i >= c * in_pitch.  Blocks b >= 1 below rest on overlap <= L: b L - overlap >= 0)
        }
    } else {
#pragma unroll
        for (int m = 0; m < E; m++) v[m] = raw_load1<FMT>(raw, x0 + t + 128 * m);
    }
    if (tail_out != nullptr && b == (long long)nb - 1) {
        float2 *to = tail_out + (long long)c * overlap;
#pragma unroll
        for (int m = 0; m < E; m++) {
            const int i = t + 128 * m;
            if (i >= L) to[i - L] = v[m];
        }
    }
    __syncthreads();
    fft2048_t128(v, lds, tw128, t, [] { __syncthreads(); });
#pragma unroll
    for (int m = 0; m < E; m++) {
        const float2 p = cmul(h[t + 128 * m], v[m]);
        v[m] = make_float2(p.x, -p.y);
    }
    fft2048_t128(v, lds, tw128, t, [] { __syncthreads(); });
    float2 *y = out + (long long)c * out_pitch + b * L;
#pragma unroll
    for (int m = 0; m < E; m++) {
        const int i = t + 128 * m;
        if (i >= overlap) y[i - overlap] = make_float2(v[m].x, -v[m].y);
    }
}

// k_fastfir_t128 for a receiver without a decimator (an empty chain: 48 kHz narrow): the band-pass reads the INPUT stream and rotates
// every sample by its channel's oscillator on the way into the registers (mixer_osc, the value k_mixer multiplies by), so the mixed
// row is neither written nor read back -- per channel one write where mixer + band-pass make four crossings (mixer write, band-pass
// read with its 2x overlap, band-pass write); a shared stream stays in cache.  Blocks behind the first recompute their overlap from the
// stream with the call's oscillator (the frequency cannot change inside a call).  Block 0's overlap are MIXED samples of the previous
// call -- mixed at the old frequency after a retune, as m_pFFTOverlapBuf holds them: `tail` [c][tail_pitch], and the last block leaves
// the next call's in `tail_out` [c][overlap] (a different buffer).  Sample s of the call sits at in[s] of its stream.
static __global__ __launch_bounds__(128) void k_fastfir_t128_mix(const float2 *__restrict__ in, long long in_pitch, int shared_input,
                                                                 float2 *__restrict__ out, long long out_pitch,
                                                                 const float2 *__restrict__ H, const float2 *__restrict__ tw128,
                                                                 int overlap /* taps-1 */, const float2 *__restrict__ tail, long long tail_pitch,
                                                                 float2 *__restrict__ tail_out, int nb, int nchan,
                                                                 const ChanOsc *__restrict__ osc, const float *__restrict__ amp_tab, float a_inf,
                                                                 OscDynInline dyn)
{
    constexpr int N = 2048, E = 16;
    __shared__ float2 lds[FftLds<N>::kSlots];
    const int t = threadIdx.x;
    const int L = N - overlap;
    int c;
    long long b;
    if (nchan > 0) {  // the XCD-ordered one-dimensional grid, as above
        const long long total = (long long)nb * nchan, per = (total + 7) >> 3;
        const long long q = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
        if ((long long)(blockIdx.x >> 3) >= per || q >= total) return;  // (uniform: the whole workgroup)
        c = (int)(q / nb);
        b = q - (long long)c * nb;
    } else {
        c = blockIdx.y;
        b = blockIdx.x;
        nb = (int)gridDim.x;
    }
    const ChanOsc *o = &osc[c];
    const double phase0 = dyn.use ? dyn.d[c].phase0 : o->phase0;
    const uint32_t n0 = dyn.use ? dyn.d[c].n0 : o->n0;
    const bool mix = (dyn.use ? dyn.d[c].mix_on : o->mix_on) != 0;
    const float2 *x = in + (shared_input ? 0 : (long long)c * in_pitch);
    const long long s0 = b * L - overlap;  // the call's sample under point 0 of [overlap | new]: negative in block 0 only (overlap <= L)
    const float2 *h = H + (long long)c * N;
    const float2 *tl = tail + (long long)c * tail_pitch;
    float2 v[E];
#pragma unroll
    for (int m = 0; m < E; m++) {
        const int i = t + 128 * m;
        const long long s = s0 + i;
        if (s < 0) v[m] = tl[i];  // (s < 0: b == 0 and i < overlap)
        else if (mix) v[m] = cmul(mixer_osc(o, phase0, n0, amp_tab, a_inf, s), x[s]);
        else v[m] = x[s];         // frequency 0: Mixer::processBlock returns its input (mixer.cpp:51-53)
    }
    if (b == (long long)nb - 1) {
        float2 *to = tail_out + (long long)c * overlap;
#pragma unroll
        for (int m = 0; m < E; m++) {
            const int i = t + 128 * m;
            if (i >= L) to[i - L] = v[m];
        }
    }
    __syncthreads();
    fft2048_t128(v, lds, tw128, t, [] { __syncthreads(); });
#pragma unroll
    for (int m = 0; m < E; m++) {
        const float2 p = cmul(h[t + 128 * m], v[m]);
        v[m] = make_float2(p.x, -p.y);
    }
    fft2048_t128(v, lds, tw128, t, [] { __syncthreads(); });
    float2 *y = out + (long long)c * out_pitch + b * L;
#pragma unroll
    for (int m = 0; m < E; m++) {
        const int i = t + 128 * m;
        if (i >= overlap) y[i - overlap] = make_float2(v[m].x, -v[m].y);
    }
}

}  // namespace pg
