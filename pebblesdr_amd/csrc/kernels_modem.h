// kernels_modem.h -- the Morse digital modem (plugins/MorseDigitalModem, Goertzel path) on the device: the modem's decimator, one
// Goertzel bin per (channel, result block), and one serial lane per channel for GoertzelOOK's TH_PEAK threshold and Morse::stateMachine.
// The threshold and state-machine code is __host__ __device__: the host runs the same updateThresholds when it (re)initialises a channel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "params.h"

// the reference's double arithmetic, operation by operation: no fused multiply-adds in this header or in what includes it (morse.hip)
#pragma clang fp contract(off)

namespace pg {

__host__ __device__ inline double morse_sma(MorseState &s, double x)  // MovingAvgFilter::newSample, SimpleMovingAverage branch
{
    if (!s.sma_primed) {
        for (int i = 0; i < 8; i++) s.sma[i] = x;
        s.sma_primed = 1;
        s.sma_sum = x * 8.0;
        s.sma_avg = x;
    } else {
        const double oldest = s.sma[s.sma_idx];
        s.sma_sum = s.sma_sum - oldest + x;
        s.sma_avg = s.sma_sum / 8.0;
        s.sma[s.sma_idx] = x;
        s.sma_idx = (s.sma_idx + 1) % 8;
    }
    return s.sma_avg;
}

// Morse::updateThresholds, morse.cpp:605-720 (the limits are the init values 10 / 50 throughout)
__host__ __device__ inline void morse_update_thresholds(MorseState &s, uint32_t usec_new, bool force)
{
    uint32_t dot = 0, dash = 0;
    if (force) {
        dot = usec_new;
        dash = dot * 3;
        s.usec_last_mark = dot;
    } else {
        if (s.usec_last_mark == 0) return;
        const double ratio = (double)((float)usec_new / (float)s.usec_last_mark);
        if (ratio >= 2 && ratio <= 4) {
            dot = s.usec_last_mark;
            dash = usec_new;
        } else if (ratio >= 0.25 && ratio <= 0.50) {
            dot = usec_new;
            dash = s.usec_last_mark;
        } else {
            return;
        }
    }
    const uint32_t ddt = (uint32_t)morse_sma(s, (double)((dash + dot) / 2));
    dot = ddt / 2;
    uint32_t wpm = dot ? kMorseDotMagic / dot : 0xffffffffu;
    if (!force && wpm < kMorseWpmLow) {
        s.below = 1;
        s.above = 0;
    } else if (!force && wpm > kMorseWpmHigh) {
        s.below = 0;
        s.above = 1;
    } else {
        s.below = 0;
        s.above = 0;
        if (wpm > kMorseWpmHigh - kMorseWpmVar) wpm -= kMorseWpmVar;
        else if (wpm < kMorseWpmLow + kMorseWpmVar) wpm += kMorseWpmVar;
        s.ddt = ddt;
        s.spike = (uint32_t)(dot * 0.50);
        s.fade = (uint32_t)(dot * 0.50);
        s.element = (uint32_t)(dot * 0.25);
        s.wpm = (int32_t)wpm;
        s.dot = dot;
        s.dash = dash;
        s.chr = dot * 2;
        s.word = dot * 4;
    }
}

// SampleClock::uSecDelta, sampleclock.cpp:19-25
__host__ __device__ inline uint32_t morse_usec(uint32_t earlier, uint32_t later, uint32_t rate)
{
    if (earlier >= later) return 0;
    return (uint32_t)(uint64_t)(((double)(later - earlier) * 1.0e6) / (double)rate);
}

__host__ __device__ inline void morse_reset_clock(MorseState &s)  // Morse::resetModemClock, morse.cpp:733-740 (m_toneStart is 0 throughout)
{
    s.clk = 0;
    s.tone_end = 0;
    s.usec_mark = 0;
    s.usec_space = 0;
}

// GoertzelOOK::processResult, TH_PEAK (goertzel.cpp:664-777); the avgPower / stdDev side path reaches no output there
__device__ inline bool morse_th_peak(MorseState &s, double p)
{
    const double aw = 1.0 / 20.0, dw = 1.0 / 500.0;  // goertzel.h:141-144
    const double wp = p > s.peak ? aw : dw;
    s.peak_avg = p * wp + s.peak_avg * (1 - wp);       // MovingAvgFilter::newSample(sample, weight), movingavgfilter.cpp:58-64
    s.peak = s.peak_avg;
    const double wm = p < s.minp ? aw : dw;
    s.min_avg = p * wm + s.min_avg * (1 - wm);
    s.minp = s.min_avg;
    const double delta = s.peak - s.minp;
    const double up = s.minp + (delta * 0.67), down = s.minp + (delta * 0.33);
    bool tone;
    if (p >= up) tone = true;
    else if (p <= down) tone = false;
    else tone = s.last_tone != 0;
    s.last_tone = tone;
    return tone;
}

// Morse::stateMachine, morse.cpp:938-1140.  Returns -1, or the kind of the event it output (*token for a character)
__device__ inline int morse_state_machine(MorseState &s, bool tone, uint32_t rate, uint32_t *token)
{
    switch (s.state) {
    case kMsIdle:
        if (tone) {
            s.dd_len = 0; s.dd_bits = 0;
            morse_reset_clock(s);
            s.last_state = kMsIdle;
            s.state = kMsMark;
        } else {
            s.last_state = kMsIdle;
        }
        break;
    case kMsMark:
        if (tone) {
            s.last_state = kMsMark;
        } else {
            s.tone_end = s.clk;
            s.usec_mark = morse_usec(0, s.tone_end, rate);
            if (s.usec_mark < s.shortest) {
                s.state = s.last_state;
                break;
            }
            morse_update_thresholds(s, s.usec_mark, false);
            s.usec_last_mark = s.usec_mark;
            s.usec_space = 0;
            s.mark_handled = 0;
            s.last_state = kMsMark;
            s.state = kMsInterElement;
        }
        break;
    case kMsInterElement:
        if (tone) {
            if (s.mark_handled) {
                morse_reset_clock(s);
                s.last_state = kMsInterElement;
                s.state = kMsMark;
            }
        } else {
            s.usec_space = morse_usec(s.tone_end, s.clk, rate);
            if (!s.mark_handled && s.usec_space > s.element) {
                if (s.dd_len >= kMorseMaxLen) {
                    s.last_state = s.state;
                    s.state = kMsIdle;
                    return -1;
                }
                s.dd_bits = (s.dd_bits << 1) | (s.usec_mark <= s.ddt ? 0u : 1u);
                s.dd_len++;
                s.mark_handled = 1;
            }
            if (s.usec_space < s.chr) {
                s.last_state = kMsInterElement;
            } else if (s.usec_space >= s.chr && s.usec_space <= s.word) {
                if (s.dd_len > 0) {
                    *token = (1u << s.dd_len) | s.dd_bits;
                    s.usec_last_space = s.usec_space;
                    s.dd_len = 0; s.dd_bits = 0;
                    s.last_state = kMsInterElement;
                    s.state = kMsWordSpace;
                    return 0;
                }
                s.last_state = kMsInterElement;
                s.state = kMsIdle;
            } else {
                s.last_state = kMsInterElement;
                s.state = kMsIdle;
            }
        }
        break;
    case kMsWordSpace:
        if (tone) {
            s.usec_last_space = s.usec_space;
            s.dd_len = 0; s.dd_bits = 0;
            morse_reset_clock(s);
            s.last_state = kMsWordSpace;
            s.state = kMsMark;
        } else {
            s.usec_space = morse_usec(s.tone_end, s.clk, rate);
            if (s.usec_space < s.word) {
                s.last_state = kMsWordSpace;
            } else {
                *token = 0;
                s.usec_last_space = s.usec_space;
                s.last_state = kMsWordSpace;
                s.state = kMsIdle;
                return 1;
            }
        }
        break;
    }
    return -1;
}

// One decimation stage of the modem's Decimator (pebblelib/decimator.cpp, as design::build_chain merges it): out[o] = sum_p h[p] x[o D - (T-1) + p]
// where x[< 0] is the previous call's input tail (hist, [channel][hist_pitch], the last T-1 samples, oldest first).  The first stage reads
// the receiver's audio rows in place, which have no head-room.  grid (ceil(n_out / 256), listed channels)
static __global__ __launch_bounds__(256) void k_morse_fir(const float2 *__restrict__ in, long long in_pitch, const float2 *__restrict__ hist,
                                                          int hist_pitch, float2 *__restrict__ out, long long out_pitch, long long n_out,
                                                          int stride, const float *__restrict__ taps, int T, const int *__restrict__ list)
{
    __shared__ float h[kMaxTaps];
    const int c = list[blockIdx.y];
    if (threadIdx.x < T) h[threadIdx.x] = taps[threadIdx.x];
    __syncthreads();
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_out) return;
    const float2 *x = in + (long long)c * in_pitch;
    const float2 *hx = hist + (long long)c * hist_pitch + (T - 1);  // hx[i] for i in [-(T-1), 0)
    const long long b = o * stride - (T - 1);
    float2 acc = make_float2(0.f, 0.f);
    for (int p = 0; p < T; p++) {
        const long long i = b + p;
        const float2 v = i >= 0 ? x[i] : hx[i];
        acc.x = fmaf(v.x, h[p], acc.x);
        acc.y = fmaf(v.y, h[p], acc.y);
    }
    out[(long long)c * out_pitch + o] = acc;
}

// the input tails of every stage after the call's last read: hist_j[c] = last T_j - 1 inputs of stage j (each call gives every stage at
// least T_j inputs, MorseCore::check).  grid (stages, listed channels), one work-item per tail sample
struct MorseTails {
    const float2 *in[kMaxStages];
    long long in_pitch[kMaxStages], n[kMaxStages];
    float2 *hist[kMaxStages];
    int keep[kMaxStages];
};
static __global__ __launch_bounds__(64) void k_morse_tails(MorseTails t, int hist_pitch, const int *__restrict__ list)
{
    const int j = blockIdx.x, c = list[blockIdx.y];
    const int k = t.keep[j];
    for (int i = threadIdx.x; i < k; i += 64)
        t.hist[j][(long long)c * hist_pitch + i] = t.in[j][(long long)c * t.in_pitch[j] + t.n[j] - k + i];
}

// Goertzel::processSample(CPX), goertzel.cpp:230-266, over the call's m modem samples: work-item b of a channel runs result block b (the
// first continues from the carried (s1, s2, count) with the coefficients in force); the trailing partial block carries its sums on.
// grid (listed channels), 64 work-items looping over the blocks
static __global__ __launch_bounds__(64) void k_morse_goertzel(const float2 *__restrict__ in, long long in_pitch, long long m, MorseParams p,
                                                              MorseState *__restrict__ st, double *__restrict__ power, long long rpitch,
                                                              const int *__restrict__ list)
{
    const int c = list[blockIdx.x];
    MorseState *S = st + c;
    const uint32_t N = p.N, cnt0 = S->count;
    const int q = S->neg ? 1 : 0;
    const double c1r = S->s1r, c1i = S->s1i, c2r = S->s2r, c2i = S->s2i;
    __syncthreads();  // every read of the carried state before its one write
    const double B = p.B[q], Cr = p.Cr[q], Ci = p.Ci[q], Dr = p.Dr[q], Di = p.Di[q];
    const long long first = (long long)(N - cnt0);
    const long long r = ((long long)cnt0 + m) / (long long)N;
    const float2 *x = in + (long long)c * in_pitch;
    for (long long b = threadIdx.x; b <= r; b += 64) {
        const long long beg = b == 0 ? 0 : first + (b - 1) * (long long)N;
        const long long end = b < r ? first + b * (long long)N : m;
        double s1r = 0, s1i = 0, s2r = 0, s2i = 0;
        uint32_t k = 0;
        if (b == 0) { s1r = c1r; s1i = c1i; s2r = c2r; s2i = c2i; k = cnt0; }
        for (long long i = beg; i < end; i++) {
            const float2 v = x[i];
            const double s0r = (double)v.x + B * s1r - s2r, s0i = (double)v.y + B * s1i - s2i;
            if (k < N - 1) {
                s2r = s1r; s2i = s1i;
                s1r = s0r; s1i = s0i;
                k++;
            } else {
                double yr = s0r - (s1r * Cr - s1i * Ci), yi = s0i - (s1r * Ci + s1i * Cr);
                const double zr = yr * Dr - yi * Di, zi = yr * Di + yi * Dr;
                yr = zr / (double)N;
                yi = zi / (double)N;
                power[(long long)c * rpitch + b] = yr * yr + yi * yi;
                k = 0;
                s1r = s1i = s2r = s2i = 0;
            }
        }
        if (b == r) {
            S->s1r = s1r; S->s1i = s1i; S->s2r = s2r; S->s2i = s2i;
            S->count = k;
            S->nres = (uint32_t)r;
            S->first_end = (uint32_t)(first - 1);
        }
    }
}

// per channel, serially over the call's results: SampleClock ticks, GoertzelOOK::processResult (TH_PEAK) and Morse::stateMachine;
// events go to the channel's log (a ring of log_cap entries; the host drains it before it can wrap, MorseCore::run).
// tone (optional, [channel][rpitch]): the decisions, for the stand-alone step's parity read-out.  grid (ceil(listed / 64)) x 64
static __global__ __launch_bounds__(64) void k_morse_decide(const double *__restrict__ power, long long rpitch, long long m, uint32_t N, uint32_t rate,
                                                            MorseState *__restrict__ st, MorseEvent *__restrict__ log, int log_cap,
                                                            unsigned char *__restrict__ tone_out, const int *__restrict__ list, int n_list)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_list) return;
    const int c = list[i];
    MorseState s = st[c];
    const double *pw = power + (long long)c * rpitch;
    long long prev = -1;
    for (uint32_t b = 0; b < s.nres; b++) {
        const long long e = (long long)s.first_end + (long long)b * N;
        s.clk += (uint32_t)(e - prev);
        prev = e;
        const bool tone = morse_th_peak(s, pw[b]);
        if (tone_out) tone_out[(long long)c * rpitch + b] = tone ? 1 : 0;
        uint32_t token = 0;
        const int kind = morse_state_machine(s, tone, rate, &token);
        if (kind >= 0) {
            MorseEvent ev;
            ev.sample = s.abs + (uint64_t)e + 1;
            ev.token = token;
            ev.kind = (uint32_t)kind;
            log[(long long)c * log_cap + (long long)(s.n_events % (uint64_t)log_cap)] = ev;
            s.n_events++;
        }
    }
    s.clk += (uint32_t)(m - 1 - prev);
    s.abs += (uint64_t)m;
    st[c] = s;
}

}  // namespace pg
