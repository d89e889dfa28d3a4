// kernels_strength.h -- the stream bank's S-meter and squelch gate (streambank.hip): SignalStrength::fdEstimate
// (application/signalstrength.cpp:287-380) per (stream, computed spectrum row), and the per-(stream, frame) decision
// m_avgDb < m_squelchDb (application/receiver.cpp:959-965) that the IQ ring's packing kernel obeys.  The rule's windows are
// strength_windows (params.h, shared with Receiver::apply_controls); its end -- power sums to four dB values -- is strength_finish
// (params.h), shared by this kernel, the receivers' k_signal_strength and the host twin (pebblegpu_signal_strength_row).
#pragma once
#include <cmath>
#include "common.h"
#include "egress.h"
#include "params.h"

namespace pg {

// (strength_finish stands in params.h beside strength_windows, so that the receivers' k_signal_strength ends through it as well: a
// window without a noise bin, or without any bin, divides 0 by 0, and the NaN comes out as the reference's qBound gives it -- the
// LOWER bound: -120 dB for peak, avg and floor, 0 for snr.  Nothing the S-meter reports is NaN.)

// One 256-lane workgroup per (stream, computed row): grid = n_streams * n_rows, row = s * n_rows + j reads spec + s * stream_pitch + j * bins
// and writes out[s * out_pitch + j]; the call's last row also goes to carry[s] (the row a later call's gate reads).  Only the aligned span
// of float4 that covers [nlo, min(nhi, bins - 1)] is loaded (rows are 16-byte aligned, bins a multiple of 4, so the span stays inside the
// row); elements outside the window are masked one by one.  Per lane: double partials for the in-band total, the in-band peak and the noise
// total, an integer noise count.  xor-shuffle tree inside the wave, then the four waves' values through LDS, added in wave order by lane 0:
// no atomics, one fixed order, the same bits on every run.  The compulsory traffic is 4 bytes per bin of the noise window.
static __global__ __launch_bounds__(256) void k_stream_strength(const float *__restrict__ spec, long long stream_pitch, int bins, int n_rows,
                                                                const SmBins *__restrict__ win, float4 *__restrict__ out, long long out_pitch,
                                                                float4 *__restrict__ carry)
{
#pragma clang fp contract(off)
    const int s = (int)(blockIdx.x / (unsigned)n_rows), j = (int)(blockIdx.x - (unsigned)s * (unsigned)n_rows);
    const SmBins b = win[s];
    const float4 *x = reinterpret_cast<const float4 *>(spec + (long long)s * stream_pitch + (long long)j * bins);
    const int last = b.nhi < bins - 1 ? b.nhi : bins - 1;  // the reference's loop ends at i == noiseHighBin or at the last bin
    const int v0 = b.nlo >> 2, v1 = (last + 4) >> 2;       // [v0, v1) float4s; empty when nlo > last (a window clamped to `bins`)
    double total = 0.0, peak = 0.0, noise = 0.0;
    int nn = 0;
    for (int k = v0 + (int)threadIdx.x; k < v1; k += 256) {
        const float4 v = x[k];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = 4 * k + q;
            if (i < b.nlo || i > last) continue;
            const double pwr = exp10((double)e[q] / 10.0);  // DB::dBToPower
            if (i >= b.lo && i <= b.hi) {
                total += pwr;
                if (pwr > peak) peak = pwr;
            } else {
                noise += pwr;
                nn++;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        total += __shfl_xor(total, m, 64);
        noise += __shfl_xor(noise, m, 64);
        nn += __shfl_xor(nn, m, 64);
        const double o = __shfl_xor(peak, m, 64);
        if (o > peak) peak = o;
    }
    __shared__ double w_total[4], w_peak[4], w_noise[4];
    __shared__ int w_nn[4];
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        w_total[w] = total;
        w_peak[w] = peak;
        w_noise[w] = noise;
        w_nn[w] = nn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = w_total[0], p = w_peak[0], z = w_noise[0];
        int c = w_nn[0];
        for (int w = 1; w < 4; w++) {
            t += w_total[w];
            z += w_noise[w];
            c += w_nn[w];
            if (w_peak[w] > p) p = w_peak[w];
        }
        const float4 r = strength_finish(t, p, z, c, b.bp_bins);
        out[(long long)s * out_pitch + j] = r;
        if (j == n_rows - 1) carry[s] = r;
    }
}

// The decision per (block row r, frame j0 + j of the call), written as the trailer entry gate[r * n_frames + j0 + j]: frame f reads its own
// S-meter row when the call computed one for it, else the latest computed at or before it -- rows.row[j] is that compact row of this call,
// kGateRowCarried (carried[stream]: the last row of an earlier call) or kGateRowNone (no row yet: values 0, the gate open).
// closed = avgDb < squelch_db on the float the S-meter reported; -120 and below never closes.
static __global__ __launch_bounds__(256) void k_stream_gate_eval(const float4 *__restrict__ smeter, long long smeter_pitch, const float4 *__restrict__ carried,
                                                                 const float *__restrict__ squelch_db, const uint32_t *__restrict__ tab, int n_sel, int n_frames,
                                                                 StreamGate *__restrict__ gate, GateRows rows)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sel * rows.n) return;
    const int r = i / rows.n, j = i % rows.n;
    const uint32_t s = tab[r];
    const int row = rows.row[j];
    StreamGate g;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row >= 0) v = smeter[(long long)s * smeter_pitch + row];
    else if (row == kGateRowCarried) v = carried[s];
    g.peak_db = v.x; g.avg_db = v.y; g.snr_db = v.z; g.floor_db = v.w;
    g.row = row >= 0 ? (uint32_t)row : (row == kGateRowCarried ? kStreamGateCarried : kStreamGateNone);
    g.open = (row != kGateRowNone && v.y < squelch_db[s]) ? 0u : 1u;  // (avgDb is clipped to >= -120: a threshold of -120 or below never closes)
    gate[(long long)r * n_frames + rows.j0 + j] = g;
}

}  // namespace pg
