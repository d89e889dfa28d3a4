// kernels_condition.h -- the stream bank's input conditioners, parallel in time (include/pebblegpu.h, "Stream bank: input conditioners").
//
// DCRemoval, IQBalance, NoiseBlanker::ProcessBlock and ProcessBlock2 (application/receiver.cpp:814-823) ahead of the bank's transforms.
// The receivers' forms (k_iir_scan in its sequential mode, k_iq_balance, k_noise_blank; kernels_demod.h) walk a stream's whole call with
// one wave or one lane.  Here a stream's call is cut into CHUNKS of kCondChunk samples and every chunk is one workgroup (one wave), so a
// configs[4] shard (128 streams x 262144 samples) is 16384 workgroups per pass.  Every stage that carries state has the same three steps:
//
//   sum      every chunk but the last computes what it adds to the state from a ZERO entry state        grid (chunks - 1, streams)
//   combine  one wave per stream turns the summaries into every chunk's ENTRY state, in order            grid (streams)
//   apply    every chunk re-runs from its true entry state and writes; the last one stores the state     grid (chunks, streams)
//
// Inside a chunk the wave takes kSub = 512 samples at a time through LDS (coalesced row loads, lane l owns samples 8 l .. 8 l + 7), as
// k_iir_scan does, and carries the state from one 512 to the next.  All scans are Hillis-Steele over lanes with shuffles: a fixed order,
// so the same call sequence gives the same bits.
//
//   DC removal   a biquad: linear.  scan_sub (kernels_demod.h) as it is, fp64 state; chunk summaries combined with the transition matrix
//                to the power kCondChunk (design::m2_pow) and its squares, in the basis (w1, w1 - w2) -- see k_cond_dc_combine.  No
//                warm-up mode; the carried state is the last chunk's exact end state.
//   NB1 / NB2    the magnitude averages a <- (float)(0.999 a + 0.001 mag) are, without the float rounding, linear recurrences of the
//                input magnitudes.  Every LANE gets its entry value from the fp64 scan and then runs its 8 samples with the reference's
//                per-step float rounding, so an average here is never more than 8 float roundings away from the exact recurrence; the
//                serial form's is the whole stream's rounding history away from it (2e-6 relative, measured).  The two differ in the last
//                bits, and so can a blanker's decision where |mag - 3.3 avg| is within those bits.  NB2's complex average (pole 0.75,
//                fp64 state, never rounded to float in the reference either) the same way.
//   NB1 counter  the spike count is a map on {0..7} per sample (candidate with count 0: -> 6; else max(count - 1, 0)); maps compose
//                associatively: 8 nibbles of a 32-bit word, composed per lane, scanned over lanes, chunks and streams' calls.
//   IQ balance   nonlinear, restarts every frame: one workgroup per (stream, frame), the frame staged through LDS 512 samples at a
//                time, lane 0 walks them.  Latency-bound by construction.
#pragma once
#include "kernels_demod.h"

namespace pg {

constexpr int kCondSubs = 4;                  // 512-sample steps per chunk
constexpr int kCondChunk = kCondSubs * kSub;  // samples per workgroup
constexpr int kCondLds = kSub + kSub / kSeg + 1;

// per stream, uploaded when a setter changed something: what the next call's kernels do
struct CondPar {
    int flags;        // PEBBLEGPU_COND_*
    int reset;        // 4 / 8: the blanker was switched on since the last call (setNbEnabled / setNb2Enabled reset its averages)
    double gain, phase;
};
// per stream, carried from call to call
struct CondState {
    double dc[2][2];      // DCRemoval: [re, im][w1, w2]
    double nb2_avg[2];
    float nb1_avg, nb2_avg_mag;
    int nb1_count, pad_;
    float2 nb1_prev[2];   // DelayLine(8, 2): NB1's last two inputs
};
// a one-pole average u <- d u + g x: P[k] = d^(kSeg << k), chunk = d^kCondChunk
struct CondAvg { double d, g, P[6], chunk; };

__device__ __forceinline__ float cond_mag(float2 v) { return (float)sqrt((double)v.x * (double)v.x + (double)v.y * (double)v.y); }

// 512 samples of a row into LDS; past the row's end zeros (they add nothing to an average and no state is read behind them)
__device__ __forceinline__ void cond_load(const float2 *__restrict__ x, long long off, int nv, float *re, float *im, int lane)
{
    for (int j = lane; j < kSub; j += 64) {
        const float2 v = j < nv ? x[off + j] : make_float2(0.f, 0.f);
        re[spad(j)] = v.x;
        im[spad(j)] = v.y;
    }
}
__device__ __forceinline__ void cond_store(float2 *__restrict__ y, long long off, int nv, const float *re, const float *im, int lane)
{
    for (int j = lane; j < nv; j += 64) y[off + j] = make_float2(re[spad(j)], im[spad(j)]);
}
__device__ __forceinline__ void cond_copy_chunk(const float2 *__restrict__ x, float2 *__restrict__ y, long long n, int lane)
{
    const long long lo = (long long)blockIdx.x * kCondChunk;
    const long long hi = lo + kCondChunk < n ? lo + kCondChunk : n;
    for (long long j = lo + lane; j < hi; j += 64) y[j] = x[j];
}

// The entry value of this lane's 8 samples u[] for the average A, given the value E entering the wave's 512 (the same in every lane);
// E becomes the value behind them.  All 64 lanes call it.
__device__ __forceinline__ double cond_avg_entry(const CondAvg &A, const double (&u)[kSeg], double &E, int lane)
{
    double s = lane == 0 ? E : 0.0;
#pragma unroll
    for (int i = 0; i < kSeg; i++) s = (A.d * s) + (A.g * u[i]);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double t = __shfl_up(s, 1u << k);
        if (lane >= (1 << k)) s += A.P[k] * t;
    }
    double e = __shfl_up(s, 1u);
    if (lane == 0) e = E;
    E = __shfl(s, 63);
    return e;
}

// ---- maps on NB1's spike count: nibble c of the word is where count c goes ----
constexpr unsigned kMapId = 0x76543210u, kMapPlain = 0x65432100u, kMapCand = 0x65432106u;
__device__ __forceinline__ int map_at(unsigned m, int c) { return (int)((m >> (4 * c)) & 7u); }
__device__ __forceinline__ unsigned map_then(unsigned first, unsigned then)
{
    unsigned h = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) h |= (unsigned)map_at(then, map_at(first, c)) << (4 * c);
    return h;
}
// inclusive scan over the lanes, lower lanes first
__device__ __forceinline__ unsigned map_scan(unsigned m, int lane)
{
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const unsigned t = __shfl_up(m, 1u << k);
        if (lane >= (1 << k)) m = map_then(t, m);
    }
    return m;
}

// ------------------------------------------------------------------------------------------------
// state: first use and the setters' resets, in stream order ahead of the call that consumes them
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(64) void k_cond_reset(CondState *__restrict__ st, const CondPar *__restrict__ par, int n_streams, int init)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_streams) return;
    CondState b = st[s];
    if (init) {
        b = CondState{};
        b.nb1_avg = 1.f;  // NoiseBlanker ctor, noiseblanker.cpp:9-15
        b.nb2_avg_mag = 1.f;
    }
    const int r = par[s].reset;
    if (r & 4) { b.nb1_count = 0; b.nb1_avg = 0.f; }
    if (r & 8) { b.nb2_avg_mag = 0.f; b.nb2_avg[0] = b.nb2_avg[1] = 0.0; }
    st[s] = b;
}

// ------------------------------------------------------------------------------------------------
// DC removal.  zsum / entry: [stream][chunk][4] doubles = [re, im][w1, w2]
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(64) void k_cond_dc_sum(const float2 *__restrict__ in, long long pitch, ScanParams<1> sp,
                                                           const CondPar *__restrict__ par, double *__restrict__ zsum, int nc)
{
    __shared__ float re[kCondLds];
    __shared__ float im[kCondLds];
    const int lane = threadIdx.x, c = blockIdx.x, s = blockIdx.y;  // c < nc - 1: every 512 of it is whole
    if (!(par[s].flags & 1)) return;
    const float2 *x = in + (long long)s * pitch;
    double st[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int sub = 0; sub < kCondSubs; sub++) {
        cond_load(x, (long long)c * kCondChunk + (long long)sub * kSub, kSub, re, im, lane);
        __syncthreads();
        scan_sub(sp.sec[0], re, kSub, st[0][0], st[0][1], lane);
        scan_sub(sp.sec[0], im, kSub, st[1][0], st[1][1], lane);
        __syncthreads();
    }
    if (lane == 0) {
        double *z = zsum + ((long long)s * nc + c) * 4;
        z[0] = st[0][0]; z[1] = st[0][1]; z[2] = st[1][0]; z[3] = st[1][1];
    }
}

// entry[0] = the carried state, entry[k + 1] = M^kCondChunk entry[k] + zsum[k]; 64 chunks per step of the lane scan.
// The scan runs on (w1, w1 - w2), not on (w1, w2): the 10 Hz high-pass at 20 Msps is a double integrator to within 1e-11, its state grows
// with the square of the stream's length (3e8 after 262144 samples of a 0.01 offset) and M^n = [[n + 1, -n], [n, -(n - 1)]] up to that
// 1e-11 -- squaring it cancels n^2 against n^2, and what is left of the last bits, times the state, is an output error of 1e-4
// relative (measured).  In the other basis A^n = [[1, n], [-n 1e-11, 1]]: nothing cancels, and the error stays at 3e-7.
// a_*: A^kCondChunk, A = [[-a1 - a2, a2], [-a1 - a2 - 1, a2]].
static __global__ __launch_bounds__(64) void k_cond_dc_combine(const double *__restrict__ zsum, double *__restrict__ entry,
                                                               const CondState *__restrict__ state, const CondPar *__restrict__ par,
                                                               double a_a, double a_b, double a_c, double a_d, int nc)
{
    const int lane = threadIdx.x, s = blockIdx.x;
    if (!(par[s].flags & 1)) return;
    double P[6][4] = {{a_a, a_b, a_c, a_d}};
#pragma unroll
    for (int k = 1; k < 6; k++) {
        const double *q = P[k - 1];
        P[k][0] = q[0] * q[0] + q[1] * q[2];
        P[k][1] = q[0] * q[1] + q[1] * q[3];
        P[k][2] = q[2] * q[0] + q[3] * q[2];
        P[k][3] = q[2] * q[1] + q[3] * q[3];
    }
    for (int comp = 0; comp < 2; comp++) {
        double c0 = state[s].dc[comp][0], c1 = c0 - state[s].dc[comp][1];
        for (int base = 0; base < nc; base += 64) {
            const int k = base + lane;
            const double *z = zsum + ((long long)s * nc + k) * 4 + comp * 2;
            double s0 = k < nc - 1 ? z[0] : 0.0, s1 = k < nc - 1 ? z[0] - z[1] : 0.0;
            if (lane == 0) {
                entry[((long long)s * nc + base) * 4 + comp * 2] = c0;
                entry[((long long)s * nc + base) * 4 + comp * 2 + 1] = c0 - c1;
                s0 += a_a * c0 + a_b * c1;
                s1 += a_c * c0 + a_d * c1;
            }
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const double t0 = __shfl_up(s0, 1u << j), t1 = __shfl_up(s1, 1u << j);
                if (lane >= (1 << j)) {
                    s0 += P[j][0] * t0 + P[j][1] * t1;
                    s1 += P[j][2] * t0 + P[j][3] * t1;
                }
            }
            if (lane < 63 && k + 1 < nc) {
                entry[((long long)s * nc + k + 1) * 4 + comp * 2] = s0;
                entry[((long long)s * nc + k + 1) * 4 + comp * 2 + 1] = s0 - s1;
            }
            c0 = __shfl(s0, 63);
            c1 = __shfl(s1, 63);
        }
    }
}

// in == out is allowed (every workgroup reads its 512 before it writes them); a stream without the flag is copied when in != out
static __global__ __launch_bounds__(64) void k_cond_dc_apply(const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n,
                                                             ScanParams<1> sp, const CondPar *__restrict__ par, const double *__restrict__ entry,
                                                             CondState *__restrict__ state, int nc)
{
    __shared__ float re[kCondLds];
    __shared__ float im[kCondLds];
    const int lane = threadIdx.x, c = blockIdx.x, s = blockIdx.y;
    const float2 *x = in + (long long)s * in_pitch;
    float2 *y = out + (long long)s * out_pitch;
    if (!(par[s].flags & 1)) {
        if (x != y) cond_copy_chunk(x, y, n, lane);
        return;
    }
    const double *e = entry + ((long long)s * nc + c) * 4;
    double st[2][2] = {{e[0], e[1]}, {e[2], e[3]}};
    for (int sub = 0; sub < kCondSubs; sub++) {
        const long long off = (long long)c * kCondChunk + (long long)sub * kSub;
        if (off >= n) break;  // workgroup-uniform
        const int nv = (int)(n - off < kSub ? n - off : kSub);
        cond_load(x, off, nv, re, im, lane);
        __syncthreads();
        scan_sub(sp.sec[0], re, nv, st[0][0], st[0][1], lane);
        scan_sub(sp.sec[0], im, nv, st[1][0], st[1][1], lane);
        __syncthreads();
        cond_store(y, off, nv, re, im, lane);
        __syncthreads();
    }
    if (c == nc - 1 && lane == 0) {
        state[s].dc[0][0] = st[0][0]; state[s].dc[0][1] = st[0][1];
        state[s].dc[1][0] = st[1][0]; state[s].dc[1][1] = st[1][1];
    }
}

// ------------------------------------------------------------------------------------------------
// IQ balance (application/iqbalance.cpp:65-86; k_iq_balance's arithmetic): grid (frames, streams), in place
// ------------------------------------------------------------------------------------------------
// one sample: t1 = out + t2 conj(out), t2 = t2 (1 - mu 1e-6) - t1 t1 mu
__device__ __forceinline__ float2 iq_step(float2 v, double gx, double gy, double &t2r, double &t2i)
{
    const float mu = 0.0025f;
    const double sc = 1.0 - mu * 0.000001;
    const double orr = (double)v.x * gx;
    const double oi = (double)v.y + ((double)v.x * gy);
    const double t1r = orr + (t2r * orr + t2i * oi);
    const double t1i = oi + (t2i * orr - t2r * oi);
    const double sqr = t1r * t1r - t1i * t1i, sqi = 2.0 * t1r * t1i;
    t2r = t2r * sc - sqr * mu;
    t2i = t2i * sc - sqi * mu;
    return make_float2((float)t1r, (float)t1i);
}
static __global__ __launch_bounds__(64) void k_cond_iq(float2 *__restrict__ buf, long long pitch, int nf, const CondPar *__restrict__ par)
{
    __shared__ float2 tile[kSub];
    const int lane = threadIdx.x, s = blockIdx.y;
    if (!(par[s].flags & 2)) return;
    const double gx = par[s].gain, gy = par[s].phase;
    float2 *x = buf + (long long)s * pitch + (long long)blockIdx.x * nf;
    double t2r = 0, t2i = 0;
    for (int off = 0; off < nf; off += kSub) {
        const int nv = nf - off < kSub ? nf - off : kSub;
        for (int j = lane; j < nv; j += 64) tile[j] = x[off + j];
        __syncthreads();
        if (lane == 0) {
            // 8 samples out of LDS at once, their 8 dependent steps, 8 stores: one LDS wait per 8 steps (a frame's last samples one by one)
            int i0 = 0;
            for (; i0 + kSeg <= nv; i0 += kSeg) {
                float2 v[kSeg];
#pragma unroll
                for (int i = 0; i < kSeg; i++) v[i] = tile[i0 + i];
#pragma unroll
                for (int i = 0; i < kSeg; i++) v[i] = iq_step(v[i], gx, gy, t2r, t2i);
#pragma unroll
                for (int i = 0; i < kSeg; i++) tile[i0 + i] = v[i];
            }
            for (; i0 < nv; i0++) tile[i0] = iq_step(tile[i0], gx, gy, t2r, t2i);
        }
        __syncthreads();
        for (int j = lane; j < nv; j += 64) x[off + j] = tile[j];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// the blankers' averages.  zsum / entry: [stream][chunk][4] doubles; NB1 uses [0], NB2 [0..2] = (re, im, magnitude)
// ------------------------------------------------------------------------------------------------
// WHICH 1: NB1's magnitude average; 2: NB2's three.  grid (chunks - 1, streams)
template <int WHICH>
static __global__ __launch_bounds__(64) void k_cond_nb_sum(const float2 *__restrict__ in, long long pitch, CondAvg mag_avg, CondAvg cpx_avg,
                                                           const CondPar *__restrict__ par, double *__restrict__ zsum, int nc)
{
    __shared__ float re[kCondLds];
    __shared__ float im[kCondLds];
    const int lane = threadIdx.x, c = blockIdx.x, s = blockIdx.y;
    if (!(par[s].flags & (WHICH == 1 ? 4 : 8))) return;
    const float2 *x = in + (long long)s * pitch;
    double Em = 0.0, Er = 0.0, Ei = 0.0;
    for (int sub = 0; sub < kCondSubs; sub++) {
        cond_load(x, (long long)c * kCondChunk + (long long)sub * kSub, kSub, re, im, lane);
        __syncthreads();
        double um[kSeg], ur[kSeg], ui[kSeg];
#pragma unroll
        for (int i = 0; i < kSeg; i++) {
            const int a = spad(lane * kSeg + i);
            const float2 v = make_float2(re[a], im[a]);
            um[i] = (double)cond_mag(v);
            ur[i] = (double)v.x;
            ui[i] = (double)v.y;
        }
        (void)cond_avg_entry(mag_avg, um, Em, lane);
        if (WHICH == 2) {
            (void)cond_avg_entry(cpx_avg, ur, Er, lane);
            (void)cond_avg_entry(cpx_avg, ui, Ei, lane);
        }
        __syncthreads();
    }
    if (lane == 0) {
        double *z = zsum + ((long long)s * nc + c) * 4;
        if (WHICH == 1) z[0] = Em;
        else { z[0] = Er; z[1] = Ei; z[2] = Em; }
    }
}

// entry[0] = the carried value, entry[k + 1] = d^kCondChunk entry[k] + zsum[k].  grid (streams)
template <int WHICH>
static __global__ __launch_bounds__(64) void k_cond_nb_combine(const double *__restrict__ zsum, double *__restrict__ entry,
                                                               const CondState *__restrict__ state, const CondPar *__restrict__ par,
                                                               double d_mag, double d_cpx, int nc)
{
    const int lane = threadIdx.x, s = blockIdx.x;
    if (!(par[s].flags & (WHICH == 1 ? 4 : 8))) return;
    for (int q = 0; q < (WHICH == 1 ? 1 : 3); q++) {
        const double d = (WHICH == 1 || q == 2) ? d_mag : d_cpx;
        double P[6] = {d};
#pragma unroll
        for (int k = 1; k < 6; k++) P[k] = P[k - 1] * P[k - 1];
        double c = WHICH == 1 ? (double)state[s].nb1_avg : q == 2 ? (double)state[s].nb2_avg_mag : state[s].nb2_avg[q];
        for (int base = 0; base < nc; base += 64) {
            const int k = base + lane;
            double v = k < nc - 1 ? zsum[((long long)s * nc + k) * 4 + q] : 0.0;
            if (lane == 0) {
                entry[((long long)s * nc + base) * 4 + q] = c;
                v += d * c;
            }
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const double t = __shfl_up(v, 1u << j);
                if (lane >= (1 << j)) v += P[j] * t;
            }
            if (lane < 63 && k + 1 < nc) entry[((long long)s * nc + k + 1) * 4 + q] = v;
            c = __shfl(v, 63);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// NB1 (noiseblanker.cpp:45-75)
// ------------------------------------------------------------------------------------------------
// this lane's 8 steps of the magnitude average from its entry value, the reference's rounding per step (no fused multiply-add: the map
// pass and the apply pass must find the same candidates) -> the candidates, bit i.  a_last: the value behind sample `last` of the lane
__device__ __forceinline__ unsigned nb1_candidates(const double (&um)[kSeg], float &a, long long last, float &a_last)
{
#pragma clang fp contract(off)
    unsigned cand = 0;
#pragma unroll
    for (int i = 0; i < kSeg; i++) {
        a = (float)((0.999 * (double)a) + (0.001 * um[i]));
        if (um[i] > ((double)a * 3.3)) cand |= 1u << i;
        if (i == last) a_last = a;
    }
    return cand;
}

// every chunk's map of the spike count, from its candidates.  grid (chunks - 1, streams)
static __global__ __launch_bounds__(64) void k_cond_nb1_map(const float2 *__restrict__ in, long long pitch, CondAvg mag_avg,
                                                            const CondPar *__restrict__ par, const double *__restrict__ entry,
                                                            unsigned *__restrict__ zmap, int nc)
{
    __shared__ float re[kCondLds];
    __shared__ float im[kCondLds];
    const int lane = threadIdx.x, c = blockIdx.x, s = blockIdx.y;
    if (!(par[s].flags & 4)) return;
    const float2 *x = in + (long long)s * pitch;
    double Em = entry[((long long)s * nc + c) * 4];
    unsigned chunk_map = kMapId;
    for (int sub = 0; sub < kCondSubs; sub++) {
        cond_load(x, (long long)c * kCondChunk + (long long)sub * kSub, kSub, re, im, lane);
        __syncthreads();
        double um[kSeg];
#pragma unroll
        for (int i = 0; i < kSeg; i++) {
            const int a = spad(lane * kSeg + i);
            um[i] = (double)cond_mag(make_float2(re[a], im[a]));
        }
        float a = (float)cond_avg_entry(mag_avg, um, Em, lane);
        float unused = 0.f;
        const unsigned cand = nb1_candidates(um, a, -1, unused);
        unsigned m = kMapId;
#pragma unroll
        for (int i = 0; i < kSeg; i++) m = map_then(m, (cand >> i) & 1u ? kMapCand : kMapPlain);
        m = map_scan(m, lane);
        chunk_map = map_then(chunk_map, __shfl(m, 63));
        __syncthreads();
    }
    if (lane == 0) zmap[(long long)s * nc + c] = chunk_map;
}

// the count entering every chunk; the two samples in front of the call for the apply pass, and the two the next call will need.
// grid (streams)
static __global__ __launch_bounds__(64) void k_cond_nb1_map_combine(const unsigned *__restrict__ zmap, int *__restrict__ ecount, float2 *__restrict__ eprev,
                                                                    CondState *__restrict__ state, const CondPar *__restrict__ par,
                                                                    const float2 *__restrict__ in, long long pitch, long long n, int nc)
{
    const int lane = threadIdx.x, s = blockIdx.x;
    if (!(par[s].flags & 4)) return;
    int cnt = state[s].nb1_count;
    for (int base = 0; base < nc; base += 64) {
        const int k = base + lane;
        unsigned m = k < nc - 1 ? zmap[(long long)s * nc + k] : kMapId;
        m = map_scan(m, lane);
        if (lane == 0) ecount[(long long)s * nc + base] = cnt;
        if (lane < 63 && k + 1 < nc) ecount[(long long)s * nc + k + 1] = map_at(m, cnt);
        cnt = map_at(__shfl(m, 63), cnt);
    }
    if (lane == 0) {
        const float2 p0 = state[s].nb1_prev[0], p1 = state[s].nb1_prev[1];
        eprev[2 * s] = p0;
        eprev[2 * s + 1] = p1;
        const float2 *x = in + (long long)s * pitch;
        state[s].nb1_prev[0] = n >= 2 ? x[n - 2] : p1;
        state[s].nb1_prev[1] = x[n - 1];
    }
}

// out != in: a sample's output is the input two samples earlier, which another workgroup may own.  grid (chunks, streams)
static __global__ __launch_bounds__(64) void k_cond_nb1_apply(const float2 *__restrict__ in, long long in_pitch, float2 *__restrict__ out, long long out_pitch,
                                                              long long n, CondAvg mag_avg, const CondPar *__restrict__ par,
                                                              const double *__restrict__ entry, const int *__restrict__ ecount,
                                                              const float2 *__restrict__ eprev, CondState *__restrict__ state, int nc)
{
    __shared__ float re[kCondLds];
    __shared__ float im[kCondLds];
    const int lane = threadIdx.x, c = blockIdx.x, s = blockIdx.y;
    const float2 *x = in + (long long)s * in_pitch;
    float2 *y = out + (long long)s * out_pitch;
    if (!(par[s].flags & 4)) {
        cond_copy_chunk(x, y, n, lane);
        return;
    }
    double Em = entry[((long long)s * nc + c) * 4];
    int cnt0 = ecount[(long long)s * nc + c];
    for (int sub = 0; sub < kCondSubs; sub++) {
        const long long off = (long long)c * kCondChunk + (long long)sub * kSub;
        if (off >= n) break;  // workgroup-uniform
        const int nv = (int)(n - off < kSub ? n - off : kSub);
        cond_load(x, off, nv, re, im, lane);
        __syncthreads();
        // this lane's 8 samples and the two in front of them
        float2 v[kSeg + 2];
#pragma unroll
        for (int i = 0; i < kSeg + 2; i++) {
            const int j = lane * kSeg + i - 2;
            if (j >= 0) v[i] = make_float2(re[spad(j)], im[spad(j)]);
            else v[i] = off > 0 ? x[off + j] : eprev[2 * s + 2 + j];
        }
        __syncthreads();
        double um[kSeg];
#pragma unroll
        for (int i = 0; i < kSeg; i++) um[i] = (double)cond_mag(v[i + 2]);
        float a = (float)cond_avg_entry(mag_avg, um, Em, lane);
        // the averages step by step again (the candidates as k_cond_nb1_map found them), the value behind the call's last sample kept
        const long long g0 = off + (long long)lane * kSeg;
        float a_last = 0.f;
        const unsigned cand = nb1_candidates(um, a, n - 1 - g0, a_last);
        unsigned m = kMapId;
#pragma unroll
        for (int i = 0; i < kSeg; i++) m = map_then(m, (cand >> i) & 1u ? kMapCand : kMapPlain);
        m = map_scan(m, lane);
        unsigned before = __shfl_up(m, 1u);
        if (lane == 0) before = kMapId;
        int cnt = map_at(before, cnt0);
        cnt0 = map_at(__shfl(m, 63), cnt0);
#pragma unroll
        for (int i = 0; i < kSeg; i++) {
            bool blank;
            if (cnt == 0 && ((cand >> i) & 1u)) { cnt = 6; blank = true; }  // m_spikeCount = 7, then the decrement of the same step
            else if (cnt > 0) { cnt--; blank = true; }
            else blank = false;
            const float2 o = blank ? make_float2(0.f, 0.f) : v[i];  // DelayLine(8, 2): the input two samples earlier
            const int a2 = spad(lane * kSeg + i);
            re[a2] = o.x;
            im[a2] = o.y;
            if (g0 + i == n - 1) {
                state[s].nb1_avg = a_last;
                state[s].nb1_count = cnt;
            }
        }
        __syncthreads();
        cond_store(y, off, nv, re, im, lane);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// NB2 (noiseblanker.cpp:77-97).  in == out is allowed; a stream without the flag is copied when in != out.  grid (chunks, streams)
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(64) void k_cond_nb2_apply(const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n,
                                                              CondAvg mag_avg, CondAvg cpx_avg, const CondPar *__restrict__ par,
                                                              const double *__restrict__ entry, CondState *__restrict__ state, int nc)
{
    __shared__ float re[kCondLds];
    __shared__ float im[kCondLds];
    const int lane = threadIdx.x, c = blockIdx.x, s = blockIdx.y;
    const float2 *x = in + (long long)s * in_pitch;
    float2 *y = out + (long long)s * out_pitch;
    if (!(par[s].flags & 8)) {
        if (x != y) cond_copy_chunk(x, y, n, lane);
        return;
    }
    const double *e = entry + ((long long)s * nc + c) * 4;
    double Er = e[0], Ei = e[1], Em = e[2];
    for (int sub = 0; sub < kCondSubs; sub++) {
        const long long off = (long long)c * kCondChunk + (long long)sub * kSub;
        if (off >= n) break;  // workgroup-uniform
        const int nv = (int)(n - off < kSub ? n - off : kSub);
        cond_load(x, off, nv, re, im, lane);
        __syncthreads();
        float2 v[kSeg];
        double um[kSeg], ur[kSeg], ui[kSeg];
#pragma unroll
        for (int i = 0; i < kSeg; i++) {
            const int a = spad(lane * kSeg + i);
            v[i] = make_float2(re[a], im[a]);
            um[i] = (double)cond_mag(v[i]);
            ur[i] = (double)v[i].x;
            ui[i] = (double)v[i].y;
        }
        float am = (float)cond_avg_entry(mag_avg, um, Em, lane);
        double ar = cond_avg_entry(cpx_avg, ur, Er, lane);
        double ai = cond_avg_entry(cpx_avg, ui, Ei, lane);
        const long long g0 = off + (long long)lane * kSeg;
#pragma unroll
        for (int i = 0; i < kSeg; i++) {
#pragma clang fp contract(off)
            ar = ar * 0.75 + ur[i] * 0.25;
            ai = ai * 0.75 + ui[i] * 0.25;
            am = (float)(0.999 * (double)am + 0.001 * um[i]);
            if (um[i] > (3.3 * (double)am)) v[i] = make_float2((float)ar, (float)ai);
            const int a = spad(lane * kSeg + i);
            re[a] = v[i].x;
            im[a] = v[i].y;
            if (g0 + i == n - 1) {
                state[s].nb2_avg[0] = ar;
                state[s].nb2_avg[1] = ai;
                state[s].nb2_avg_mag = am;
            }
        }
        __syncthreads();
        cond_store(y, off, nv, re, im, lane);
        __syncthreads();
    }
}

}  // namespace pg
