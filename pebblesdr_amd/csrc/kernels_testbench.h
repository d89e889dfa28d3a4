// kernels_testbench.h -- the test bench's signal generator on the device (TestBenchCore, receiver.h):
// NCO::genSweep (pebblelib/nco.cpp:140-212) and NCO::genNoise (:87-116) as TestBench::genSweep / genNoise call them at the head of
// Receiver::processIQData (application/testbench.cpp:518-544, application/receiver.cpp:797-798), in ONE pass over the streams.
//
// Sweep.  The reference accumulates the phase serially (m_sweepAcc += m_sweepFreq * m_sweepFreqNorm, m_sweepFreq += m_sweepRateInc per
// sample, fmod once per call).  Here every sample evaluates the closed form of its sweep leg, in double and in TURNS (phase / 2 pi, so
// that the reduction before the sincos is an exact subtraction):
//     turns(k) = turns0 + (f0 * j + inc * j (j - 1) / 2) / fs,   j = k - k0,
// with (k0, turns0, f0, inc) from the call's leg table, which the host writes relative to the CALL's first sample (indexing from the
// stream's first sample would lose the low bits of j^2).  A leg ends where the reference's frequency reaches the stop frequency
// (nco.cpp:188-207); SINGLE then holds (inc = 0), REPEAT starts over, REPEAT_REVERSE runs back.
// Pulse modulation (nco.cpp:149-156) is a serial double accumulation of 1 / fs whose edges depend on rounding: the host runs it once
// (TestBenchCore::set_sweep) and the kernel gates by (absolute sample number mod period).
//
// Noise.  The Knop polar method of the reference with its rand() replaced by a counter-based draw: a pure function of
// (seed, stream, absolute sample number, attempt, which of the two), so a sample's noise depends neither on call sizes nor on the lane
// that makes it.  tests/testbench_ref.py restates the function; the integers are reproduced exactly.
#pragma once
#include "common.h"
#include "receiver.h"

namespace pg {

// ---- the counter-based draw ----
__host__ __device__ __forceinline__ unsigned long long tb_mix64(unsigned long long z)  // the splitmix64 finaliser
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr unsigned long long kTbGolden = 0x9E3779B97F4A7C15ull;
__host__ __device__ __forceinline__ unsigned long long tb_stream_key(unsigned long long seed, unsigned stream)
{
    return tb_mix64(seed + kTbGolden * (unsigned long long)(stream + 1u));
}
// attempt a of sample n: 64 bits, the two 31-bit draws are bits 63..33 and 31..1
__device__ __forceinline__ unsigned long long tb_draw(unsigned long long key, unsigned long long n, int a)
{
    return tb_mix64(tb_mix64(key ^ n) + kTbGolden * (unsigned long long)(a + 1));
}
// NCO::genNoise's loop body for one sample (nco.cpp:98-107), amplitude 1: at most kTbNoiseAttempts attempts (an attempt is accepted
// with probability pi / 4; all of them failing, 0.215^32 = 4e-22 per sample, leaves the sample without noise).  *att: the accepted
// attempt's number, kTbNoiseAttempts when none was
__device__ __forceinline__ double2 tb_noise(unsigned long long key, unsigned long long n, unsigned *r1, unsigned *r2, int *att)
{
    for (int a = 0; a < kTbNoiseAttempts; a++) {
        const unsigned long long h = tb_draw(key, n, a);
        const unsigned ra = (unsigned)(h >> 33), rb = (unsigned)(h >> 1) & 0x7FFFFFFFu;
        const double u1 = 1.0 - 2.0 * (double)ra / 2147483647.0;
        const double u2 = 1.0 - 2.0 * (double)rb / 2147483647.0;
        const double s = __dadd_rn(__dmul_rn(u1, u1), __dmul_rn(u2, u2));  // (no contraction: the acceptance test sees the reference's s)
        if (s >= 1.0 || s == 0.0) continue;
        const double rad = sqrt(-2.0 * log(s) / s);
        *r1 = ra; *r2 = rb; *att = a;
        return make_double2(u1 * rad, u2 * rad);
    }
    *r1 = 0; *r2 = 0; *att = kTbNoiseAttempts;
    return make_double2(0.0, 0.0);
}

// the last leg that starts at or before call-relative sample k (legs[0].k0 == 0), by bisection.  Called with a wave-uniform k (the first
// sample of the wave's stretch), so the table is read through scalar loads, once per wave and step instead of once per sample
__device__ __forceinline__ int tb_find_leg(const SweepLeg *__restrict__ legs, int n_legs, unsigned long long k)
{
    int lo = 0, hi = n_legs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (legs[mid].k0 <= k) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ unsigned long long tb_uniform(unsigned long long v)  // the first active lane's value, in scalar registers
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (unsigned long long)hi << 32 | lo;
}

// one output sample: `in` + sweep + noise, formed in double and rounded to float once.  leg: a leg at or before the sample's (the wave's
// first sample's leg); the sample's own is at most a few entries further (a wave spans 128 samples, a whole leg at least kTbMinLeg)
// kAdd (k_morsegen): `add`, the stations' sum at this sample, goes in between the sweep and the noise
template <bool kAdd = false>
__device__ __forceinline__ float2 tb_sample(const TbParams &p, const SweepLeg *__restrict__ legs, int leg, unsigned long long noise_key, long long k, float2 in,
                                            double2 add = make_double2(0.0, 0.0))
{
    double re = (double)in.x, im = (double)in.y;
    const unsigned long long n_abs = p.n0 + (unsigned long long)k;
    if (p.sweep_on) {
        double amp = p.amp;
        if (p.pulse_period) {  // on while the reference's timer is <= the width: its first pulse_on increments, and the one that resets it
            const unsigned long long m = n_abs % p.pulse_period;
            if (m >= p.pulse_on && m != p.pulse_period - 1) amp = 0.0;
        }
        while (leg + 1 < p.n_legs && legs[leg + 1].k0 <= (unsigned long long)k) leg++;
        const SweepLeg lg = legs[leg];
        const unsigned long long j = (unsigned long long)k - lg.k0;
        const unsigned long long tri = (j & 1) ? j * ((j - 1) >> 1) : (j >> 1) * (j - 1);
        double t = lg.turns0 + (lg.f0 * (double)j + lg.inc * (double)tri) * p.fs_inv;  // (j < 2^26: the host splits longer pieces, tri is exact)
        t -= rint(t);
        double s, c;
        sincospi(2.0 * t, &s, &c);
        if (p.mix) { re += amp * c; im += amp * s; }
        else { re = amp * c; im = amp * s; }
    }
    if (kAdd) { re += add.x; im += add.y; }
    if (p.noise_on) {
        unsigned r1, r2;
        int att;
        const double2 g = tb_noise(noise_key, n_abs, &r1, &r2, &att);
        re += p.noise_amp * g.x;
        im += p.noise_amp * g.y;
    }
    return make_float2((float)re, (float)im);
}

// in == nullptr: silence in (a generator that replaces, or a stand-alone buffer that is only written); in may equal out.
// One work-item makes two neighbouring samples per step (16-byte accesses) when the rows allow it (vec: pointers 16-byte aligned, even
// pitches), else one.  grid (x, streams)
static __global__ __launch_bounds__(256) void k_testbench(const float2 *in, float2 *out, long long in_pitch, long long out_pitch, long long n, int vec,
                                                          TbParams p, const SweepLeg *__restrict__ legs)
{
    const unsigned s = blockIdx.y;
    const unsigned long long key = tb_stream_key(p.seed, p.stream0 + s);
    const float2 *src = in ? in + (long long)s * in_pitch : nullptr;
    float2 *dst = out + (long long)s * out_pitch;
    const long long step = (long long)gridDim.x * 256;
    if (vec) {
        const long long pairs = n >> 1;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < pairs; q += step) {
            const int leg = p.sweep_on ? tb_find_leg(legs, p.n_legs, tb_uniform(2ull * (unsigned long long)(q - (threadIdx.x & 63)))) : 0;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (src) v = reinterpret_cast<const float4 *>(src)[q];
            const float2 a = tb_sample(p, legs, leg, key, 2 * q, make_float2(v.x, v.y));
            const float2 b = tb_sample(p, legs, leg, key, 2 * q + 1, make_float2(v.z, v.w));
            reinterpret_cast<float4 *>(dst)[q] = make_float4(a.x, a.y, b.x, b.y);
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = tb_sample(p, legs, p.sweep_on ? tb_find_leg(legs, p.n_legs, (unsigned long long)(n - 1)) : 0, key, n - 1, src ? src[n - 1] : make_float2(0.f, 0.f));
    } else {
        for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += step) {
            const int leg = p.sweep_on ? tb_find_leg(legs, p.n_legs, tb_uniform((unsigned long long)(k - (threadIdx.x & 63)))) : 0;
            dst[k] = tb_sample(p, legs, leg, key, k, src ? src[k] : make_float2(0.f, 0.f));
        }
    }
}

// ---- keyed Morse stations (MorseGen, plugins/MorseGenDevice/morsegen.cpp) ----
// the envelope at sample i of a mark of L samples (morsegen.cpp:95-117): ampInc (i + 1) over the rise, m_amplitude, then m_amplitude - ampInc (i + 1)
// over the fall; 0 outside the mark
__device__ __forceinline__ double morse_env(const MorseStationDev &h, long long L, long long i)
{
    if ((unsigned long long)i >= (unsigned long long)L) return 0.0;
    const long long fall0 = L - (long long)h.rise;
    return i < (long long)h.rise ? h.inc * (double)(i + 1) : i < fall0 ? h.amp : h.amp - h.inc * (double)(i - fall0 + 1);
}

// the stations' sum at the lane's kMorseRun consecutive samples a .. a + kMorseRun - 1 (call-relative).  [w0, w1) is the wave's stretch: the
// station loop, the bisection and the marks it visits are wave-uniform (scalar loads); a station whose stretch lies wholly in a gap costs
// the bisection and nothing else.  Inside a mark the lane takes the carrier at its first sample from one sincospi -- the phase in turns,
// (a - start) * f / fs with the product's rounding error recovered by an fma, so the reduction is exact -- and the following ones by
// rotating with exp(j 2 pi f / fs) in double (kMorseRun - 1 rotations: 1e-16 each).
__device__ __forceinline__ void morse_sum(const MorseStationDev *__restrict__ st, const long long *__restrict__ marks, int n_st, long long w0, long long w1, long long a,
                                          double2 (&acc)[kMorseRun])
{
    for (int i = 0; i < n_st; i++) {
        const MorseStationDev h = st[i];
        if (!h.count) continue;
        const long long *__restrict__ m = marks + h.first;
        // the last mark that starts at or before w0 (marks do not overlap: no earlier one reaches into the stretch), else the first
        int lo = 0, hi = (int)h.count - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((m[mid] >> 1) <= w0) lo = mid;
            else hi = mid - 1;
        }
        for (int j = lo; j < (int)h.count; j++) {
            const long long enc = m[j], start = enc >> 1;
            if (start >= w1) break;
            const long long L = (enc & 1) ? (long long)h.dash : (long long)h.dot;
            if (start + L <= w0) continue;
            const long long i0 = a - start;  // (|i0| < 2^26 + 64 kMorseRun: exact in a double)
            if (i0 + kMorseRun <= 0 || i0 >= L) continue;
            const double x = (double)i0;
            double t = x * h.tps;
            const double t_lo = fma(x, h.tps, -t);
            t = (t - rint(t)) + t_lo;
            double s, c;
            sincospi(2.0 * t, &s, &c);
#pragma unroll
            for (int r = 0; r < kMorseRun; r++) {
                const double e = morse_env(h, L, i0 + r);
                acc[r].x += e * c;
                acc[r].y += e * s;
                const double c1 = c * h.rot_c - s * h.rot_s;
                s = c * h.rot_s + s * h.rot_c;
                c = c1;
            }
        }
    }
}

// k_testbench with stations: in + sweep + stations + noise in ONE pass over the streams.  A work-item makes kMorseRun neighbouring samples
// per step, of every stream: the stations' sum is formed once per sample position and added to each stream.  grid (x); in == nullptr:
// silence in; in may equal out; vec as k_testbench's (16-byte accesses, two samples each)
static __global__ __launch_bounds__(256) void k_morsegen(const float2 *in, float2 *out, long long in_pitch, long long out_pitch, long long n, int streams, int vec,
                                                         TbParams p, const SweepLeg *__restrict__ legs, const MorseStationDev *__restrict__ st,
                                                         const long long *__restrict__ marks, int n_st)
{
    const long long runs = (n + kMorseRun - 1) / kMorseRun;
    const long long step = (long long)gridDim.x * 256;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x;; q += step) {
        const long long q0 = (long long)tb_uniform((unsigned long long)(q - (threadIdx.x & 63)));
        if (q0 >= runs) break;
        const long long w0 = q0 * kMorseRun, w1 = min(n, w0 + 64ll * kMorseRun), a = q * kMorseRun;
        double2 acc[kMorseRun];
#pragma unroll
        for (int r = 0; r < kMorseRun; r++) acc[r] = make_double2(0.0, 0.0);
        morse_sum(st, marks, n_st, w0, w1, a, acc);
        if (a >= n) continue;
        const int leg = p.sweep_on ? tb_find_leg(legs, p.n_legs, (unsigned long long)w0) : 0;
        for (int s = 0; s < streams; s++) {
            const unsigned long long key = tb_stream_key(p.seed, p.stream0 + (unsigned)s);
            const float2 *src = in ? in + (long long)s * in_pitch : nullptr;
            float2 *dst = out + (long long)s * out_pitch;
#pragma unroll
            for (int r = 0; r < kMorseRun; r += 2) {
                const long long k = a + r;
                if (vec && k + 1 < n) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (src) v = *reinterpret_cast<const float4 *>(src + k);
                    const float2 y0 = tb_sample<true>(p, legs, leg, key, k, make_float2(v.x, v.y), acc[r]);
                    const float2 y1 = tb_sample<true>(p, legs, leg, key, k + 1, make_float2(v.z, v.w), acc[r + 1]);
                    *reinterpret_cast<float4 *>(dst + k) = make_float4(y0.x, y0.y, y1.x, y1.y);
                } else {
                    if (k < n) dst[k] = tb_sample<true>(p, legs, leg, key, k, src ? src[k] : make_float2(0.f, 0.f), acc[r]);
                    if (k + 1 < n) dst[k + 1] = tb_sample<true>(p, legs, leg, key, k + 1, src ? src[k + 1] : make_float2(0.f, 0.f), acc[r + 1]);
                }
            }
        }
    }
}

// the accepted draws of samples first .. first + n - 1 of one stream (parity checks against the restatement): r [n][2], attempt [n]
static __global__ __launch_bounds__(256) void k_testbench_draws(unsigned long long seed, unsigned stream, unsigned long long first, int n,
                                                                unsigned *__restrict__ r, unsigned char *__restrict__ attempt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned r1, r2;
    int att;
    (void)tb_noise(tb_stream_key(seed, stream), first + (unsigned long long)i, &r1, &r2, &att);
    r[2 * i] = r1;
    r[2 * i + 1] = r2;
    attempt[i] = (unsigned char)att;
}

// ---- host side ----
// (definitions with external linkage: EXACTLY ONE translation unit, steps.hip, includes this header; receiver.hip and the rest see the
// declarations in receiver.h)

// NCO::initSweep + the serial pulse timer of NCO::genSweep, run once: no device needed
int tb_plan_sweep(double fs, const pebblegpu_sweep *s, TbSweepPlan *plan)
{
    if (!s || !plan) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (s->struct_size != sizeof(pebblegpu_sweep)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_sweep size mismatch (ABI %d)", PEBBLEGPU_ABI_VERSION);
    if (!(fs > 0) || s->sweep_type < 0 || s->sweep_type > 2) return fail(PEBBLEGPU_E_INVALID, "bad sample rate or sweep type");
    if (!std::isfinite(s->start_hz) || !std::isfinite(s->stop_hz) || !std::isfinite(s->rate_hz_per_s) || !std::isfinite(s->amplitude) ||
        !std::isfinite(s->pulse_width_s) || !std::isfinite(s->pulse_period_s))
        return fail(PEBBLEGPU_E_INVALID, "sweep parameters must be finite");
    TbSweepPlan pl;
    pl.inc = s->rate_hz_per_s / fs;  // m_sweepRateInc
    pl.leg = 0;                      // 0: the leg never ends
    if (pl.inc > 0) {
        // the frequency after j steps reaches the stop frequency at j = ceil(|stop - start| / inc); the test comes after a step, so j >= 1
        const double q = std::ceil(std::fabs(s->stop_hz - s->start_hz) / pl.inc);
        if (q < 9.0e18) {  // (else: not reached within a 64-bit sample count)
            pl.leg = q < 1.0 ? 1ull : (unsigned long long)q;
            if (pl.leg < (unsigned long long)kTbMinLeg)
                return fail(PEBBLEGPU_E_UNSUPPORTED, "sweep legs of %llu samples: the leg table is built for %d or more (DESIGN.md section 7)", pl.leg, kTbMinLeg);
        }
    } else {
        pl.inc = 0.0;  // "if (m_sweepRateInc > 0)", nco.cpp:181: the frequency never moves
    }
    pl.pulse_period = pl.pulse_on = 0;
    if (s->pulse_width_s > 0.0) {
        // m_sweepPulseTimer += 1 / fs until it exceeds the period (then it is reset: the pattern repeats); the first increment that leaves it
        // above the width starts the gap
        const double dt = 1.0 / fs;
        // (the sum below is run here, under the owner's lock: 2^28 additions are a fraction of a second; the reference's 0.5 s is 1e7 samples at 20 Msps)
        if (!(s->pulse_period_s * fs < (double)kTbMaxPulsePeriod)) return fail(PEBBLEGPU_E_UNSUPPORTED, "pulse periods of 2^28 samples or more are not built");
        double t = 0.0;
        unsigned long long i = 0, first_off = 0;
        do {
            t += dt;
            i++;
            if (!first_off && t > s->pulse_width_s) first_off = i;
        } while (!(t > s->pulse_period_s));
        pl.pulse_period = i;
        // samples 0 .. pulse_on - 1 of a period are on, and its last (the increment that resets the timer leaves 0, which is never above a width > 0)
        pl.pulse_on = first_off ? first_off - 1 : i;
    }
    *plan = pl;
    return 0;
}

// MorseGen::setParams' sizes (morsegen.cpp:45-87) and one pass through the text: no device needed
int tb_plan_morse(double fs, const pebblegpu_morse_station *st, MorsePlan *plan)
{
    if (!st || !plan) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (st->struct_size != sizeof(pebblegpu_morse_station)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_morse_station size mismatch (ABI %d)", PEBBLEGPU_ABI_VERSION);
    if (!(fs > 0) || !std::isfinite(fs)) return fail(PEBBLEGPU_E_INVALID, "bad sample rate");
    if (!std::isfinite(st->frequency_hz) || !std::isfinite(st->amplitude)) return fail(PEBBLEGPU_E_INVALID, "station parameters must be finite");
    if (!(std::fabs(st->frequency_hz) < fs / 2)) return fail(PEBBLEGPU_E_INVALID, "station frequency %g Hz is outside +-fs/2", st->frequency_hz);
    if (st->n_tokens == 0 || !st->tokens) return fail(PEBBLEGPU_E_INVALID, "a station needs at least one token");
    for (uint32_t i = 0; i < st->n_tokens; i++)
        if (st->tokens[i] >= 0x200) return fail(PEBBLEGPU_E_INVALID, "token %#x has more than nine bits (morsegen.cpp:244)", (unsigned)st->tokens[i]);
    if (st->wpm == 0) return fail(PEBBLEGPU_E_UNSUPPORTED, "0 words per minute");
    const uint32_t ms_tcw = 1200u / st->wpm;  // MorseCode::wpmToTcwMs
    const double spt_d = (double)ms_tcw / (1000.0 / fs), rise_d = (double)st->ms_rise / (1000.0 / fs);  // morsegen.cpp:47, 55-56
    if (ms_tcw == 0 || !(spt_d >= 1.0)) return fail(PEBBLEGPU_E_UNSUPPORTED, "%u words per minute at %g Hz: no sample per Tcw", st->wpm, fs);
    if (!(3.0 * spt_d + rise_d < (double)kMorseMaxMark)) return fail(PEBBLEGPU_E_UNSUPPORTED, "marks of 2^26 samples or more are not built");
    MorsePlan pl;
    pl.spt = (unsigned long long)spt_d;
    pl.rise = (unsigned long long)rise_d;
    // m_numSamplesDot = samplesPerTcw - (rise + fall) / 2 (:58-59) is unsigned: below one sample the reference wraps
    if (pl.spt <= pl.rise) return fail(PEBBLEGPU_E_UNSUPPORTED, "a rise of %llu samples leaves no dot at %llu samples per Tcw", pl.rise, pl.spt);
    pl.dot = 2 * pl.rise + (pl.spt - pl.rise);       // :61
    pl.dash = 2 * pl.rise + (3 * pl.spt - pl.rise);  // :66-67
    if (pl.dash >= kMorseMaxMark) return fail(PEBBLEGPU_E_UNSUPPORTED, "marks of 2^26 samples or more are not built");
    pl.period = 0;
    for (uint32_t i = 0; i < st->n_tokens; i++) {
        const unsigned tok = st->tokens[i];
        if (!tok) { pl.period += 7 * pl.spt - 3; continue; }  // genWord, :84
        int top = 8;
        while (!((tok >> top) & 1u)) top--;
        for (int b = top - 1; b >= 0; b--) pl.period += (b < top - 1 ? pl.spt : 0) + (((tok >> b) & 1u) ? pl.dash : pl.dot);  // genDot / genDash
        pl.period += 3 * pl.spt;  // genChar
        if (pl.period >= kMorseMaxPeriod) break;
    }
    if (pl.period >= kMorseMaxPeriod) return fail(PEBBLEGPU_E_UNSUPPORTED, "texts of 2^40 samples or more are not built");
    *plan = pl;
    return 0;
}

// the plan, the kernel's constants and where the marks of one pass start (genToken :236-267 over the tokens, in order)
int tb_morse_station(double fs, const pebblegpu_morse_station *st, MorseStationHost *out)
{
    MorseStationHost h;
    if (int rc = tb_plan_morse(fs, st, &h.plan)) return rc;
    const MorsePlan &pl = h.plan;
    h.dev.tps = st->frequency_hz / fs;
    h.dev.amp = st->amplitude;
    h.dev.inc = pl.rise ? st->amplitude / (double)pl.rise : 0.0;  // ampInc, :95 (never used with hard keying)
    h.dev.rot_c = (double)cosl(2.0L * 3.14159265358979323846264338327950288L * (long double)h.dev.tps);
    h.dev.rot_s = (double)sinl(2.0L * 3.14159265358979323846264338327950288L * (long double)h.dev.tps);
    h.dev.rise = (unsigned)pl.rise;
    h.dev.dot = (unsigned)pl.dot;
    h.dev.dash = (unsigned)pl.dash;
    unsigned long long at = 0;
    for (uint32_t i = 0; i < st->n_tokens; i++) {
        const unsigned tok = st->tokens[i];
        if (!tok) { at += 7 * pl.spt - 3; continue; }
        int top = 8;
        while (!((tok >> top) & 1u)) top--;
        for (int b = top - 1; b >= 0; b--) {
            if (b < top - 1) at += pl.spt;  // the element space: between two marks of one character only (:272-275)
            const bool dash = (tok >> b) & 1u;
            h.mark_off.push_back(at);
            h.mark_dash.push_back(dash ? 1 : 0);
            at += dash ? pl.dash : pl.dot;
        }
        at += 3 * pl.spt;
    }
    h.pos = 0;
    *out = std::move(h);
    return 0;
}

void tb_morse_marks(const MorseStationHost &st, unsigned long long n, std::vector<long long> &marks)
{
    if (st.mark_off.empty()) return;
    const long long period = (long long)st.plan.period;
    // pass by pass: `base` is where a pass starts relative to the call's first sample (the first one at -pos)
    for (long long base = -(long long)st.pos; base < (long long)n; base += period) {
        // the first mark of the pass that ends behind the call's first sample (every mark ends inside its pass: a character space follows)
        size_t j = 0;
        if (base < 0) {
            const unsigned long long from = (unsigned long long)(-base);
            j = (size_t)(std::upper_bound(st.mark_off.begin(), st.mark_off.end(), from) - st.mark_off.begin());
            if (j > 0 && st.mark_off[j - 1] + (st.mark_dash[j - 1] ? st.plan.dash : st.plan.dot) > from) j--;
        }
        for (; j < st.mark_off.size(); j++) {
            const long long start = base + (long long)st.mark_off[j];
            if (start >= (long long)n) return;
            marks.push_back(start * 2 + st.mark_dash[j]);
            if (marks.size() > kMorseMaxCallMarks) return;
        }
    }
}

int TestBenchCore::set_morse(const pebblegpu_morse_station *st, uint32_t n, int mix)
{
    if (n > PEBBLEGPU_MORSE_MAX_STATIONS) return fail(PEBBLEGPU_E_INVALID, "%u stations: at most %d", n, PEBBLEGPU_MORSE_MAX_STATIONS);
    if (n && !st) return fail(PEBBLEGPU_E_INVALID, "null argument");
    std::vector<MorseStationHost> next(n);
    for (uint32_t i = 0; i < n; i++)
        if (int rc = tb_morse_station(fs, &st[i], &next[i])) return rc;
    stations.swap(next);  // every station at its first token; the sweep and the noise counter stay where they are
    morse_mix = mix != 0;
    return 0;
}

int TestBenchCore::ensure_events()
{
    for (int i = 0; i < 2; i++)
        if (!h_done[i]) PG_HIP(hipEventCreateWithFlags(&h_done[i], hipEventDisableTiming));
    return 0;
}

int TestBenchCore::init(double sample_rate, uint32_t streams)
{
    fs = sample_rate;
    S = streams;
    return 0;
}

void TestBenchCore::release()
{
    for (hipEvent_t &e : h_done) {  // (the tables go with the object)
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

// TestBench::reset(): the sweep restarts at the start frequency with phase 0 and pulse timer 0, the noise counter at 0
void TestBenchCore::reset()
{
    n_abs = 0;
    turns = 0.0;
    leg_pos = 0;
    if (sweep_on) {
        start = sw.start_hz;
        stop = sw.stop_hz;
        up = start < stop;  // m_sweepUp
        f_leg = start;
        inc = up ? plan.inc : -plan.inc;
        leg_len = plan.leg;
    }
}

int TestBenchCore::set_sweep(const pebblegpu_sweep *s)
{
    if (!s) {
        sweep_on = false;
        reset();
        return 0;
    }
    TbSweepPlan pl;
    if (int rc = tb_plan_sweep(fs, s, &pl)) return rc;
    sw = *s;
    plan = pl;
    sweep_on = true;
    reset();
    return 0;
}

int TestBenchCore::set_noise(double amplitude, uint64_t seed_)
{
    if (!std::isfinite(amplitude)) return fail(PEBBLEGPU_E_INVALID, "the noise amplitude must be finite");
    noise_on = amplitude > 0.0;
    noise_amp = noise_on ? amplitude : 0.0;
    seed = seed_;
    reset();
    return 0;
}

// the legs of the next n samples, relative to the call's first; advances the carried (phase, frequency, leg, direction)
int TestBenchCore::build_legs(long long n, std::vector<SweepLeg> &legs)
{
    legs.clear();
    unsigned long long k = 0;
    while (k < (unsigned long long)n) {
        const unsigned long long left = (unsigned long long)n - k;
        // (a piece is at most kTbMaxPiece samples: j (j - 1) / 2 stays exact in the kernel's double, however slow the sweep and long the call)
        const unsigned long long len = std::min(leg_len ? std::min(left, leg_len - leg_pos) : left, kTbMaxPiece);
        const double f0 = f_leg + inc * (double)leg_pos;
        legs.push_back(SweepLeg{k, turns, f0, inc});
        // the phase where the piece ends, as the kernel would evaluate it one sample further (long double: the carry is made once per piece)
        const long double tri = (long double)len * (long double)(len - 1) / 2.0L;
        long double t = (long double)turns + ((long double)f0 * (long double)len + (long double)inc * tri) / (long double)fs;
        t -= floorl(t);
        turns = (double)t;
        if (turns >= 1.0) turns = 0.0;
        k += len;
        leg_pos += len;
        if (leg_len && leg_pos == leg_len) {  // reached end of sweep (nco.cpp:188-207)
            leg_pos = 0;
            switch (sw.sweep_type) {
            case 0:  // SINGLE: m_sweepRateInc = 0, the frequency stays where the last step left it
                f_leg = f_leg + inc * (double)leg_len;
                inc = 0.0;
                leg_len = 0;
                break;
            case 1:  // REPEAT
                break;
            default:  // REPEAT_REVERSE: swap start and stop, reverse
                std::swap(start, stop);
                up = !up;
                inc = -inc;
                f_leg = start;
                break;
            }
        }
    }
    return 0;
}

// in (may be nullptr: silence) -> out (may be in), `streams` rows of n samples; the carried state moves on by n samples
int TestBenchCore::run(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n, uint32_t streams, uint32_t stream0)
{
    if (!any() || n <= 0) return 0;
    TbParams p;
    memset(&p, 0, sizeof(p));
    p.fs_inv = 1.0 / fs;
    p.n0 = n_abs;
    p.seed = seed;
    p.stream0 = stream0;
    p.noise_on = noise_on ? 1 : 0;
    p.noise_amp = noise_amp;
    const int slot = parity;
    const bool table = sweep_on || morse_on();  // the call uploads a table through pinned slot `slot`
    size_t n_marks = 0;
    if (morse_on()) {  // (first: a call too long for the mark table is refused before anything moves)
        marks_.clear();
        for (MorseStationHost &st : stations) {
            st.dev.first = (unsigned)marks_.size();
            tb_morse_marks(st, (unsigned long long)n, marks_);
            if (marks_.size() > kMorseMaxCallMarks) return fail(PEBBLEGPU_E_UNSUPPORTED, "more than 2^22 marks in one call: make shorter calls");
            st.dev.count = (unsigned)marks_.size() - st.dev.first;
        }
        n_marks = marks_.size();
    }
    if (sweep_on) {
        p.sweep_on = 1;
        p.mix = sw.mix != 0;
        p.amp = sw.amplitude;
        p.pulse_period = plan.pulse_period;
        p.pulse_on = plan.pulse_on;
        if (int rc = build_legs(n, legs_)) return rc;
        if (legs_.size() > leg_cap) {  // (a call longer, or legs shorter, than any before: both tables grow; rare)
            PG_HIP(hipStreamSynchronize(s));
            const size_t cap = legs_.size() + legs_.size() / 2 + 8;
            if (int rc = ensure_events()) return rc;
            for (int i = 0; i < 2; i++) {
                PG_HIP(hipEventSynchronize(h_done[i]));
                leg_cap = 0;
                PG_TRY(d_legs[i].alloc(cap));
                PG_TRY(h_legs[i].alloc(cap));
            }
            leg_cap = cap;
            used[0] = used[1] = false;
        }
    }
    const size_t morse_bytes = sizeof(MorseStationDev) * stations.size() + sizeof(long long) * n_marks;
    if (morse_on() && morse_bytes > morse_cap) {  // (more stations, or more marks in a call, than any before; rare)
        PG_HIP(hipStreamSynchronize(s));
        const size_t cap = morse_bytes + morse_bytes / 2 + 256;
        if (int rc = ensure_events()) return rc;
        for (int i = 0; i < 2; i++) {
            PG_HIP(hipEventSynchronize(h_done[i]));
            morse_cap = 0;
            PG_TRY(d_morse[i].alloc(cap));
            PG_TRY(h_morse[i].alloc(cap));
        }
        morse_cap = cap;
        used[0] = used[1] = false;
    }
    if (table && used[slot]) PG_HIP(hipEventSynchronize(h_done[slot]));  // the upload two calls back has left the pinned slot
    if (sweep_on) {
        memcpy(h_legs[slot], legs_.data(), sizeof(SweepLeg) * legs_.size());
        PG_HIP(hipMemcpyAsync(d_legs[slot], h_legs[slot], sizeof(SweepLeg) * legs_.size(), hipMemcpyHostToDevice, s));
        p.n_legs = (int)legs_.size();
    }
    if (morse_on()) {
        MorseStationDev *hd = reinterpret_cast<MorseStationDev *>(h_morse[slot].get());
        for (size_t i = 0; i < stations.size(); i++) hd[i] = stations[i].dev;
        if (n_marks) memcpy(h_morse[slot] + sizeof(MorseStationDev) * stations.size(), marks_.data(), sizeof(long long) * n_marks);
        PG_HIP(hipMemcpyAsync(d_morse[slot], h_morse[slot], morse_bytes, hipMemcpyHostToDevice, s));
    }
    if (table) {
        PG_HIP(hipEventRecord(h_done[slot], s));
        used[slot] = true;
        parity ^= 1;
    }
    const bool mix_in = in != nullptr && !(sweep_on && !sw.mix) && !(morse_on() && !morse_mix);  // a generator that replaces never reads the input
    const float2 *src = mix_in ? in : nullptr;
    const int vec = ((reinterpret_cast<uintptr_t>(out) | (src ? reinterpret_cast<uintptr_t>(src) : 0)) & 15) == 0 && (streams == 1 || ((in_pitch | out_pitch) & 1) == 0);
    if (morse_on()) {
        const long long runs = (n + kMorseRun - 1) / kMorseRun;
        long long blocks = (runs + 255) / 256;
        if (blocks > 256 * 8) blocks = 256 * 8;
        launch(k_morsegen, dim3((unsigned)blocks), dim3(256), s, src, out, in_pitch, out_pitch, n, (int)streams, vec, p, (const SweepLeg *)(sweep_on ? d_legs[slot].get() : nullptr),
               (const MorseStationDev *)d_morse[slot].get(), (const long long *)(d_morse[slot] + sizeof(MorseStationDev) * stations.size()), (int)stations.size());
        PG_HIP(hipGetLastError());
        for (MorseStationHost &st : stations) st.pos = (st.pos + (unsigned long long)n) % st.plan.period;
    } else {
        const long long items = vec ? (n + 1) / 2 : n;
        long long blocks = (items + 255) / 256;
        if (blocks > 256 * 8) blocks = 256 * 8;
        launch(k_testbench, dim3((unsigned)blocks, streams), dim3(256), s, src, out, in_pitch, out_pitch, n, vec, p, (const SweepLeg *)(sweep_on ? d_legs[slot].get() : nullptr));
        PG_HIP(hipGetLastError());
    }
    n_abs += (unsigned long long)n;
    return 0;
}

int TestBenchCore::draws(hipStream_t s, uint32_t stream, uint64_t first, uint32_t n, uint32_t *r, uint8_t *attempt)
{
    if (!n) return 0;
    DevBuf<unsigned> d_r;
    DevBuf<unsigned char> d_a;
    PG_TRY(d_r.alloc(2 * (size_t)n));
    PG_TRY(d_a.alloc(n));
    launch(k_testbench_draws, dim3((n + 255) / 256), dim3(256), s, (unsigned long long)seed, stream, (unsigned long long)first, (int)n, d_r, d_a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(r, d_r, sizeof(unsigned) * 2 * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(attempt, d_a, n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PEBBLEGPU_E_HIP, "noise draws: %s", hipGetErrorString(e));
    return 0;
}

}  // namespace pg
