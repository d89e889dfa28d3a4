// params.h -- plain structs shared by the host objects and the kernels (passed by value or uploaded).
#pragma once
#include <cmath>
#include <type_traits>
#include "common.h"
#include "decim_route.h"
#include "raw_load.h"

namespace pg {

// Per-channel oscillator block, rewritten by the host before every call (a few hundred bytes/channel).
// Mixer::processBlock (pebblelib/mixer.cpp:48-81) restated in closed form:
//   osc_i = a_{n0+i} * exp(j*2*pi*(phase0 + (i+1)*inc)),  a_0 = 1, a_{k+1} = a_k*(1.95 - a_k^2)
struct ChanOsc {
    // --- first 16 bytes change every call (uploaded alone, asynchronously) ---
    double phase0;          // cycles; accumulated phase at the end of the previous call (0 after a retune)
    uint32_t n0;            // samples since the last retune, saturated at kAmpTab
    uint32_t mix_on;        // 0 => f == 0: Mixer returns its input untouched (mixer.cpp:51-53)
    // --- the rest changes only on a retune ---
    double inc;             // cycles per sample = -f/Fs (the reference negates f, mixer.cpp:31)
    float2 step[kMaxTaps];  // exp(j*2*pi*d*inc), d = 0..kMaxTaps-1, rounded from fp64
    float2 step512;         // exp(j*2*pi*512*inc): advance of one 256-lane float4 sweep
    float2 pad_;
};

struct FirTaps {
    int ntaps;
    int stride;
    int cic3;   // 1: CIC3 decimate-by-`stride` in the reference's merged form (decimator.cpp:719-737)
    float gain; // applied to the output (gain restore on the last stage, receiver.cpp:935-938), else 1
    float h[kMaxTaps];
};

// the wide hb11 stage behind a merged CIC3, as kernel arguments of k_mix_cic_hb
struct FrontTaps { float h[kFrontT1]; int stride; };

// later decimation stages fused in one kernel (k_cascade): taps live in the kernel-argument segment
struct CascadeParams {
    int nst, outb;            // fused stages, final outputs per workgroup
    int lds_half, pad_;       // float2 slots of the first ping-pong buffer
    float gain;               // applied to the final stage's output
    int ntaps[kMaxCascade], stride[kMaxCascade];
    float h[kMaxCascade][60];
};

constexpr size_t kChanOscDynBytes = 16;
// The per-call part of ChanOsc for small banks travels in the kernel arguments instead of a host-to-device copy in the
// stream (which costs a ~10 us bubble per call); use == 0: read it from the ChanOsc block.
constexpr int kOscInline = 8;
struct OscDyn { double phase0; uint32_t n0, mix_on; };
struct OscDynInline {
    OscDyn d[kOscInline];
    int use, pad_;
};

constexpr int kSeg = 8;               // consecutive samples one lane runs serially
constexpr int kSub = 64 * kSeg;       // samples one wave scans at a time

enum ScanType { kOnePoleDiff = 0, kOnePoleAvg = 1, kBiquadDf2 = 2 };

struct ScanSection {
    int type;
    int pad_;
    double c[5];      // kOnePoleDiff: c0 = alpha.  kOnePoleAvg: c0 = alpha.  kBiquadDf2: b0 b1 b2 a1 a2
    double P[6][4];   // M^(kSeg * 2^k), row-major 2x2, k = 0..5
};
template <int NSEC> struct ScanParams { ScanSection sec[NSEC]; };

// PLL demodulators (k_pll_demod): loop constants and per-channel state, floats as the reference declares them
struct PllParams {
    int mode;                 // 0: NFM, 1: SAM
    float lo, hi, alpha, beta;
    float dc_alpha, out_gain; // NFM only
    int pad_;
};
struct PllState {             // per channel
    float freq, phase, err_dc, pad_;
    double dc_re_last, dc_im_last;  // SAM DC removal (doubles, demod_sam.h:27-31)
};

// history-tail refresh jobs, one launch for all buffers: for every channel c, dst[c][j] = data[c][n - hist + j], j < hist,
// where dst is the buffer's own head-room (data[c][-hist + j]) unless a separate history buffer is given
struct TailJob {
    float2 *data;
    long long pitch, n;
    int hist, pad_;
    float2 *dst;           // nullptr: the head-room in front of data
    long long dst_pitch;
    const int *list;       // nullptr: every row of the launch; else rows list[0 .. n_list) only (the rest keep their head-room)
    int n_list, pad2_;
};
constexpr int kMaxTailJobs = 12;
// The oscillators' per-call fields can ride on the same launch: osc[c].phase0 += adv[c] (mod 1), n0 += adv_n (saturating at
// kAmpTab) for c < osc_count -- OscBank::advance restated on the device, so a bank too large for kernel-argument transport
// needs no host-to-device copy per call (a DMA-engine copy in the stream cost ~20 us of idle GPU each call).
struct OscAdvance {
    ChanOsc *osc;        // nullptr: nothing to advance
    const double *adv;   // [osc_count] frac(n * inc), computed on the host in long double for this call length
    uint32_t adv_n, osc_count;
};
struct TailJobs {
    int count, pad_;
    OscAdvance oa;
    TailJob job[kMaxTailJobs];
};

// Demod_WFM::processDataStereo before its pilot PLL drops out (application/demod/demod_wfm.cpp:255-297, :392-429): the constants of one
// demodulator rate and the state one channel carries.  hilb: [2][61] the 61-tap Hilbert pair (I taps, Q taps) in device memory.
struct WfmPilotParams {
    double b0, b2, a1, a2;                 // pilot band-pass biquad (b1 = 0), iir.cpp:131-146
    double nco_lo, nco_hi, alpha, beta;    // initPilotPll, :371-386
    double err_alpha, phase_adjust;
    int block;                             // samples per processDataStereo call (the lock decision is per block)
    int L4;                                // length of the audio response the (L - R) part will go through
};
struct WfmPilotState {
    double d1_re, d1_im;                   // the discriminator's previous sample
    double z[61];                          // the Hilbert filter's delay line (discriminator values), circular
    double w1a, w2a, w1b, w2b;             // pilot band-pass
    double nco_phase, nco_freq, err_ave;
    int zpos;
    int dropped;                           // a block has ended without lock: from here on the block copies the mono signal (see WfmCore)
    long long quiet;                       // (L - R) samples that have been zero at the end of the stream so far, saturating
    int skip, pad_;                        // this call adds nothing to the output (set per call for the FIR behind)
};

// The RDS branch of Demod_WFM::processDataStereo (application/demod/demod_wfm.cpp:296-357, 488-757): constants of one demodulator
// rate, the state one dmFMS channel carries and the record of a group put into m_RdsGroupQueue
struct RdsParams {
    double osc_turns;                      // m_RdsDownConvert's oscillator, turns per demodulator-rate sample
    double nco_lo, nco_hi, alpha, beta;    // processRdsPll, :499-503
    double b0, b2, a1, a2;                 // bit-rate resonator (b1 = 0), :522
    int block;                             // RDS-rate samples per processDataStereo call of the reference
    int mtaps;                             // matched filter
    int log_cap;                           // entries of a channel's group log (a ring)
    int pad_;
};
struct RdsEvent {
    unsigned short a, b, c, d;             // tRDS_GROUPS; all zero: the queue was cleared (:642-647)
    unsigned flags;                        // 1: this entry is the clear + zero group of a lost signal
    long long frame;                       // processDataStereo call (counted from the object's first) that produced it
};
struct RdsState {
    double prev_re, prev_im;               // the discriminator's previous sample
    double nco_phase, nco_freq;
    double w1, w2;                         // resonator
    double last_sync, last_slope, last_data;
    long long n0;                          // samples the down-converter's oscillator has produced
    long long frames;                      // processDataStereo calls so far
    unsigned long long n_events;           // groups logged so far (the log is a ring of log_cap entries)
    unsigned in_bits;                      // m_InBitStream
    int last_bit, bit_pos, cur_block, state, bgroup, block_errors;
    unsigned short block[4];
    int pad_;
};

// A stream still in the device's own sample format (RawSrc), its scale and the loads that convert it: raw_load.h, which a plain C++
// compiler accepts too

// The raw sample format as a compile-time constant: f(std::integral_constant<int, F>) for the runtime fmt, so that one generic lambda
// picks a kernel's instance per format (0..4: pebblegpu_iq_format; anything else takes 4's place).  with_sample_fmt also knows -1,
// "the samples are float2 already" (no RawSrc).
template <class Fn>
inline void with_raw_fmt(int fmt, Fn &&f)
{
    switch (fmt) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
    }
}
template <class Fn>
inline void with_sample_fmt(const RawSrc *raw, Fn &&f)
{
    if (!raw) f(std::integral_constant<int, -1>{});
    else with_raw_fmt(raw->fmt, f);
}

// Per-channel squelch gate of a bank (receiver.cpp:959-965 per channel): open[c * stride + j] != 0 <=> channel c's super-frame j of
// this call passes.  The kernels behind the band-pass take one super-frame j at a time and leave a closed channel alone
// (no output, no state change).  open == nullptr: no gate.
struct Gate {
    const unsigned char *open;
    int stride, j;
    __host__ __device__ bool closed(int c) const { return open != nullptr && open[(long long)c * stride + j] == 0; }
};

// fdEstimate's bin windows for one channel: noise [nlo, nhi] around the band-pass [lo, hi]; stream = which spectrum it reads
struct SmBins { int nlo, lo, hi, nhi, bp_bins, stream, pad_[2]; };
// ... as the reference works them out (signalstrength.cpp:313-337): integer bin width sample_rate / bins (the caller makes sure it is not 0),
// truncating conversions, qBound(0, ., bins)
inline SmBins strength_windows(uint32_t bins, uint32_t sample_rate, float bp_lo, float bp_hi, double mixer_freq, int stream)
{
    const int nb = (int)bins;
    const double bin_width = (double)(sample_rate / bins);
    auto qb = [nb](int v) { return v < 0 ? 0 : (v > nb ? nb : v); };
    const int mixer_bin = qb((int)(nb / 2 + (mixer_freq / bin_width)));
    SmBins b{};
    b.lo = qb((int)(mixer_bin + (bp_lo / bin_width)));
    b.hi = qb((int)(mixer_bin + (bp_hi / bin_width)));
    b.bp_bins = b.hi - b.lo;
    b.nlo = qb(b.lo - b.bp_bins);
    b.nhi = qb(b.hi + b.bp_bins);
    b.stream = stream;
    return b;
}

// fdEstimate behind its loop (signalstrength.cpp:355-380): total / peak over the band-pass bins, noise over the noise_bins bins either
// side.  DB::powerTodB(0) = -120, DB::clip bounds to -120..0, snr to 0..120.  bp_bins == 0 with a bin in the window gives avg +inf -> 0 dB;
// no noise bin, or no bin at all, gives 0 / 0.  The reference bounds with qBound(lo, v, hi) = qMax(lo, qMin(hi, v)), where Qt words
// qMin(a, b) = a < b ? a : b and qMax(a, b) = a < b ? b : a: every comparison with NaN is false, so a NaN comes out as the LOWER bound,
// -120 dB for peak, avg and floor, 0 for snr (strength_bound keeps that order of comparisons).  One rule for the receivers' kernel
// (k_signal_strength), the stream bank's (k_stream_strength) and the host twin (pebblegpu_signal_strength_row).
__host__ __device__ inline double strength_bound(double lo, double v, double hi)
{
    const double m = hi < v ? hi : v;
    return lo < m ? m : lo;
}
__host__ __device__ inline float4 strength_finish(double total, double peak, double noise_total, int noise_bins, int bp_bins)
{
#pragma clang fp contract(off)
    const double avg = total / (double)bp_bins, navg = noise_total / (double)noise_bins;
    const double pk_db = peak == 0.0 ? -120.0 : 10.0 * log10(peak);
    const double avg_db = avg == 0.0 ? -120.0 : 10.0 * log10(avg);
    const double fl_db = navg == 0.0 ? -120.0 : 10.0 * log10(navg);
    const double snr = (navg == 0.0 || peak == 0.0) ? -120.0 : 10.0 * log10(peak / navg);
    float4 o;
    o.x = (float)strength_bound(-120.0, pk_db, 0.0);
    o.y = (float)strength_bound(-120.0, avg_db, 0.0);
    o.z = (float)strength_bound(0.0, snr, 120.0);
    o.w = (float)strength_bound(-120.0, fl_db, 0.0);
    return o;
}

// k_spectrum_t128<.., DEC = true>: the one-channel mixer + decimator hb11 x 8, hb15, hb23, hb47 (20 Msps -> 312.5 kHz; the halfbands'
// coefficients are literals of the kernel, hb_const.h) computed by the
// display transform's workgroups from the frames they hold in LDS anyway -- the stream crosses HBM once instead of twice, and no
// first-stage buffer is written or read (kernels_spectrum.h)
struct DecFuse {
    float2 *y;               // final outputs, 32 per frame: y[32 f + i]
    float2 *y0_tail;         // the call's last 256 first-stage outputs (for a later call that takes the general kernels)
    const float2 *xtail;     // the WINDOWED frame in front of the call (the previous call's last frame; zeros at the very start)
    float2 *xtail_next;      // this call's last frame, windowed: the next call's xtail
    double phase0, inc;      // oscillator at input sample n of the call: a_inf e^{j 2 pi (phase0 + (n + 1) inc)}
    float a_inf, gain0, gain_last;
    int mix_on;
    int pad_;                // (keeps the layout the kernels were measured with)
    float2 wfr;              // e^{j 2 pi 2048 inc}: an output's oscillator from one frame to the next
    float2 *ph_scratch;      // [chains][256]: the first stage's oscillator per output, carried from frame to frame of a chain (L2-resident)
    const float2 *c0tab;     // [7][256]: step[d] h0[d] / w[8 jf - 10 + d] for the seven non-zero taps d = 0 2 4 5 6 8 10: the first stage's taps against
                             // WINDOWED samples with the oscillator's advance over the window folded in (rebuilt on a retune)
};

struct SpectrumParams {
    long long in_pitch;      // samples between streams
    long long n_frames;      // frames in this call (per stream)
    int frames_per_group;    // G
    float scale;             // 1 / (coherentGain * maxBinPower), maxBinPower = NF (fft.cpp:84)
    long long out_pitch;     // floats between streams (= n_frames*bins)
};

// The frames of a gated call (SignalSpectrum's update timer, signalspectrum.cpp:63-113): a short list of far-apart frames, worked out
// by the host before anything is queued and carried in the kernel arguments (k_spectrum_list_*); longer lists take several launches.
constexpr int kListMax = 64;
struct FrameList {
    int n;                   // listed frames of this launch
    int row0;                // output row of idx[0] (rows are compact: [stream][n_selected][bins])
    long long pred;          // the listed frame in front of idx[0], whose amplitudes pair with idx[0]'s; -1: the carried buffer
    int last;                // != 0: idx[n - 1] is the call's last listed frame: its amplitudes go to the carried buffer
    int pad_;
    uint32_t idx[kListMax];  // frame numbers relative to the call's first frame, ascending
};
// the squelch gate of a bank under the update timer: per super-frame the compact row of the latest computed spectrum at or before the
// super-frame's last raw frame (k_gate_eval_rows); kGateRowCarried: the row carried from an earlier call; kGateRowNone: no spectrum yet
constexpr int kGateRowCarried = -1, kGateRowNone = -2;
struct GateRows {
    int n, j0;               // super-frames j0 .. j0 + n - 1 of the call
    int row[kListMax];
};

// ---- the Morse digital modem (kernels_modem.h) ----
constexpr uint32_t kMorseDotMagic = 1200000;  // MorseCode::c_uSecDotMagic, morsecode.h:58
constexpr uint32_t kMorseWpmLow = 10, kMorseWpmHigh = 50, kMorseWpmVar = 2;  // morse.h:82-83, :169
constexpr int kMorseMaxLen = 8;               // MorseCode::c_maxMorseLen, morsecode.h:51
enum MorseRx { kMsIdle = 0, kMsMark = 1, kMsInterElement = 2, kMsWordSpace = 3 };  // DECODE_STATE, morse.h

// one decided output of Morse::outputString: a character (the dot-dash token of morsecode.cpp:160-185) or the word space " "
struct MorseEvent {
    uint64_t sample;  // modem-rate samples since the modem was enabled, up to and including the one whose result decided it
    uint32_t token;   // kind 0: leading 1, then 1 per dash and 0 per dot (oldest element first); kind 1: 0
    uint32_t kind;    // 0 character, 1 word space
};

// the modem rate's constants: Goertzel::setFreq (goertzel.cpp:154-219) for +1000 Hz ([0]) and -1000 Hz moved up by the rate ([1])
struct MorseParams {
    double B[2], Cr[2], Ci[2], Dr[2], Di[2];
    uint32_t N, rate;
};

// everything Morse, GoertzelOOK, Goertzel and the dot-dash threshold filter carry from one sample to the next, per channel
struct MorseState {
    double s1r, s1i, s2r, s2i;        // Goertzel m_s1, m_s2
    double peak, minp;                // GoertzelOOK m_peakPower, m_minPower
    double peak_avg, min_avg;         // ... their DecayMovingAverage filters' m_movingAvg
    double sma[8];                    // m_dotDashThresholdFilter: SimpleMovingAverage(8), movingavgfilter.cpp:66-130
    double sma_sum, sma_avg;
    uint64_t abs;                     // modem samples since enabled
    uint64_t n_events;                // events appended to the channel's log since enabled
    uint32_t count;                   // Goertzel m_nCount
    uint32_t neg;                     // the tone sits at -1000 Hz (CWL / LSB): MorseParams [1]
    uint32_t nres, first_end;         // this call's results and the call index of the first one's last sample (k_morse_goertzel -> k_morse_decide)
    int32_t last_tone, sma_primed, sma_idx;
    int32_t state, last_state, mark_handled, dd_len;
    uint32_t dd_bits;                 // m_dotDashBuf as a token without its leading 1
    uint32_t clk;                     // SampleClock m_clock
    uint32_t tone_end, usec_mark, usec_space, usec_last_mark, usec_last_space;
    uint32_t ddt, element, chr, word, spike, fade, dot, dash, shortest;
    int32_t wpm, above, below;
};

}  // namespace pg
