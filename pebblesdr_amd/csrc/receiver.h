// receiver.h -- host-side objects behind the C ABI (include/pebblegpu.h).
//
// Five device "cores", one per reference class on the hot path, each owning its device state and
// launching its kernels on a caller-supplied stream:
//   DecimCore   <- Mixer + Decimator           (pebblelib/mixer.cpp, decimator.cpp)
//   FastFirCore <- CFastFIR / BandPassFilter   (pebblelib/fastfir.cpp, application/bandpassfilter.cpp)
//   AmCore      <- Demod_AM                    (application/demod/demod_am.cpp)
//   WfmCore     <- Demod_WFM (mono)            (application/demod/demod_wfm.cpp)
//   SpectrumCore<- FFT::fftSpectrum            (pebblelib/fft.cpp)
// Receiver composes them the way Receiver::processIQData does; the stand-alone steps (steps.hip) wrap one
// core each behind the reference's per-class call shapes.  What one call asks of a core travels in that call's arguments
// (DecimCall / DecimDone, AmCore::run's defer_tail); the route of a Receiver call is planned once, in call_route.h, and the kernels of
// a DecimCore::run call in decim_route.h (both plain C++ that the CPU tier compiles).
#pragma once
#include <algorithm>
#include <complex>
#include <mutex>
#include <vector>
#include "../../include/pebblegpu.h"
#include "call_route.h"
#include "common.h"
#include "decim_route.h"
#include "devmem.h"
#include "design.h"
#include "egress.h"
#include "ingest.h"
#include "params.h"
#include "tuning.h"

namespace pg {

// [channel][hist | data] complex buffer; data(c) points at the first new sample, data(c)[-hist..-1] is history.
// Move-only: it owns `base`.
struct HistBuf {
    DevBuf<float2> base;
    long long pitch = 0;  // samples per channel row (hist + capacity, even)
    int hist = 0;
    long long cap = 0;
    int chans = 0;
    float2 *data(int c = 0) const { return base + (long long)c * pitch + hist; }
    int alloc(int channels, int hist_len, long long capacity);
    void release() { base.release(); }
};

void fill_scan_section(ScanSection &s, int type, const double *c);
int make_twiddles(int n, DevBuf<float2> &tw);
int make_twiddles_t128(DevBuf<float2> &tw);
int make_twiddles_t128q(DevBuf<float2> &tw);  // four tables, the pruned transform's per-work-item factor folded in (k_spectrum_t128)
int run_save_tails(hipStream_t s, const std::vector<TailJob> &jobs, uint32_t channels, const OscAdvance *oa = nullptr);
// the rows of the channels in d_list (device memory, n_list entries) only: for buffers that only those channels' kernels fill
int run_save_tails_listed(hipStream_t s, const std::vector<TailJob> &jobs, const int *d_list, int n_list);
int run_nap(hipStream_t s, unsigned ticks_100mhz);  // one sleeping wave (k_nap)
int run_fir_dec(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n_out, int stride,
                const float *d_taps, int ntaps, uint32_t channels);
int fill_tail_jobs(TailJobs &tj, const std::vector<TailJob> &jobs, const OscAdvance *oa);  // 0, or a failure code (too many / too deep)
int run_normalize_iq(int fmt, int order, double gain, const void *d_src, long long n, float2 *d_dst, hipStream_t s, bool wait, const float *final_scale = nullptr);
int run_gate_eval(hipStream_t s, const float4 *d_smeter, long long smeter_pitch, int frames_per_sf, int k, const float *d_squelch, unsigned char *d_gate,
                  int stride, uint32_t channels);
int run_gate_eval_rows(hipStream_t s, const float4 *d_smeter, long long smeter_pitch, const float4 *d_carried, const int *rows, int k, const float *d_squelch,
                       unsigned char *d_gate, int stride, uint32_t channels);
int run_gate_zero(hipStream_t s, float2 *audio, long long pitch, long long spf, const unsigned char *d_gate, int stride, uint32_t channels, int k);
int run_signal_strength(hipStream_t s, const float *d_spec, long long stream_pitch, int bins, long long n_frames, const SmBins *d_bins,
                        float4 *d_out, long long out_pitch, uint32_t channels);
// FFT::mapFFTToScreen (display.hip, kernels_display.h): rows = n_streams x n_frames of fft_size float dB, row (s, j) at
// in + s * stream_pitch + j * frame_pitch, to out[(s * n_frames + j) * x_pixels + i].  edges: (startFreq, stopFreq), one pair for
// every stream or (per_stream) one per stream
int run_screen_map(hipStream_t s, const float *in, long long stream_pitch, long long frame_pitch, int n_streams, int n_frames, int32_t fft_size,
                   double sample_rate, const int32_t *edges, bool per_stream, int32_t y_pixels, int32_t x_pixels, double max_db, double min_db,
                   int32_t *out);
// SignalSpectrum::mapFFTZoomedToScreen's (startFreq, stopFreq) for one channel
void zoom_span_edges(uint32_t hires_rate, double zoom, int32_t mode_offset, int32_t *start, int32_t *stop);
// the refusals every mapping shares (x_pixels, y_pixels, max_db == min_db); 0 when the request can be queued
int check_screen_map(int32_t y_pixels, int32_t x_pixels, double max_db, double min_db);

// ---- oscillator bank (Mixer state for C channels) ----
struct OscBank {
    struct Ctl { double freq = 0, inc = 0, phase0 = 0; uint64_t n0 = 0; bool dirty = true; };
    double fs = 0;
    uint32_t C = 0;
    std::vector<Ctl> ctl;
    std::vector<ChanOsc> h_osc;               // host master copy
    struct Dyn { double phase0; uint32_t n0, mix_on; };
    OscDynInline inline_dyn = {};             // filled by upload() when allow_inline and C <= kOscInline
    bool allow_inline = false;                // set by owners whose kernels take OscDynInline
    PinnedBuf<Dyn> h_dyn[2];                  // pinned staging of the per-call fields, ping-pong: no host sync per call
    hipEvent_t h_done[2] = {nullptr, nullptr};
    int h_idx = 0;
    DevBuf<ChanOsc> d_osc;
    DevBuf<float> d_amp;
    float a_inf = 0;
    // Banks too large for kernel-argument transport (C > kOscInline): with device_advance set by the owner, the per-call fields
    // are advanced ON the device at the end of each call (k_save_tails, OscAdvance) instead of being copied up before the next;
    // the owner passes advance_job(n) to its tail-refresh launch.  d_adv holds frac(n * inc) per channel for the current call
    // length, rebuilt (long double, as advance() computes) when the length or a frequency changes.
    bool device_advance = false;
    bool dev_dyn_valid = false;    // the device blocks hold the per-call fields of the coming call
    DevBuf<double> d_adv;
    uint64_t adv_n = 0;
    bool adv_stale = true;
    uint64_t dyn_epoch = 0;        // counts host writes of the device blocks' per-call fields (a retune's block, the per-call upload)
    int advance_job(hipStream_t s, uint64_t n, OscAdvance *oa);  // fills *oa (osc == nullptr when the device is not advancing)
    int init(uint32_t channels, double sample_rate);
    void release();
    void retune(uint32_t ch, double f);           // Mixer::setFrequency, mixer.cpp:25-40
    void retune_keep(uint32_t ch, double f);      // CDownConvert::SetFrequency, downconvert.cpp:100-112: phase and amplitude carry on
    bool force_mix = false;                       // no "frequency 0 returns the input" exit (CDownConvert always multiplies)
    int upload(hipStream_t s);                     // refresh the device blocks (async, from pinned staging)
    void advance(uint64_t n);                      // after a call consumed n samples
    bool any_transient() const;                    // some oscillator is inside its amplitude transient (n0 < kAmpTab)
};

// ---- Mixer + Decimator ----
// what one DecimCore::run call is asked for, and what it reports back
struct DecimCall {
    bool lds_free = false;            // the first kernel should leave LDS alone (it runs beside the display transform)
    bool rotate3 = true;              // this call rotates three output buffers (ignored without fin3)
    hipEvent_t done_event = nullptr;  // an event to complete WITH the call's last launch when that is the bank kernel
    bool mix_in_consumer = false;     // an empty chain only: the consumer (the band-pass) rotates the samples in its own loads
};
struct DecimDone {
    bool osc_advanced = false;        // the route's kernel advanced the oscillators itself
    bool done_recorded = false;       // DecimCall::done_event was completed (else the caller records it)
};

// ---- shape: DecimShape (decim_route.h), what init derives from the chain -- C, zero_stage, bank_front, wide, fused_front, fused_all,
// bank_mfma, fused_hy, xh_depth ... -- assigned whole by init() and release() ----
struct DecimCore : DecimShape {
    design::Chain chain;
    Tuning tun;                      // the owner's switches (init)

    // ---- buffers and tap values ----
    FirTaps first;                   // stage 0 (fused with the mixer)
    CascadeParams casc;              // stages 1.. (one fused kernel)
    HistBuf buf0, fin;               // stage-0 output (head-room = look-back of its reader), final output (absent for 1-stage chains)
    HistBuf buf1;                    // the wide stage's output (DecimShape::wide)
    const HistBuf &y0_buf() const { return fused_front ? buf1 : buf0; }  // the first-stage (hb11) outputs' buffer: its head-room is the one-kernel routes' history
    FrontTaps wide_fir;              // the wide stage's taps as kernel arguments (fused_front)
    DevBuf<float> d_wide_taps;
    FrontTaps bank_taps;
    // An empty chain whose consumer may mix in its own loads (DecimCall::mix_in_consumer; k_fastfir_t128_mix): run() then launches nothing and
    // hands out where block 0's overlap of MIXED samples lies and where the consumer's last block leaves the next call's (mix_tail).
    // Hand-over between the two routes, in both directions, at the switch only: such a call behind a k_mixer call reads its overlap
    // straight from buf0's head-room (that call's tail job has refreshed it); a k_mixer call behind such a call first copies the
    // consumer's row into the head-room (ovl_pending).
    DevBuf<float2> d_ovl[2];                       // [C][ovl_len] the consumer's overlap rows, written by alternate calls
    int ovl_len = 0;
    struct FusedDecParams *fused_p = nullptr;   // host copy of k_mix_dec_fused's parameter block
    DevBuf<float2> d_xhist[2];                  // [xh_depth] raw input tail of the previous call, ping-pong with hist_parity
    float2 *d_y0stage = nullptr;                // a view of d_y0stage2[.]: [C][HY] the call's last first-stage outputs, copied into buf0's head-room by the tail refresh (k_mix_dec_fused: = d_y0stage2[0])
    DevBuf<float2> d_y0stage2[2];               // k_mix_dec_mfma stages them alternately and reads the previous launch's directly (y0_cur: the one written last)
    DevBuf<float2> d_bank_state[2];             // [C][38] the halfbands' running sums where the last k_mix_dec_mfma call ended (ping-pong)
    DevBuf<OscDyn> d_dyn[2];                    // [C] the oscillators' per-call fields as k_mix_dec_mfma hands them from call to call (ping-pong)
    DevBuf<float2> d_hist_mixed[2];             // [C][kMaxTaps]: mixed-sample history of stage 0 (read one, write the other)
    DevBuf<unsigned long long> d_clk;           // Tuning::bank_clk: the waves' clock counts of the last k_mix_dec_mfma launch
    // One channel through hb11 x 8, hb15, hb23, hb47 beside an 8192-bin display transform: k_spectrum_t128<.., DEC> computes the whole
    // decimator from the frames it holds in LDS (DecFuse, kernels_spectrum.h).  Its look-back is the previous call's last frame, kept
    // WINDOWED (the transform's workgroups park windowed frames): written by that kernel, or by k_window_tail behind a call that took
    // the general kernels, so either route can follow the other.
    DevBuf<float2> d_xtail_w[2];                   // [2048] ping-pong
    const float *fuse_window = nullptr;            // a view of the display transform's window, SpectrumCore::d_window (set by the owner; nullptr: never fused)
    DevBuf<float2> d_c0tab;                        // [7][256] first-stage taps over that window times the oscillator's step per tap (DecFuse::c0tab)
    std::vector<float> h_r0;                       // ... the real part of it: h0[d] / w[n]
    std::vector<float2> h_c0;
    bool c0_valid = false;
    double c0_inc = 0;
    int c0_mix = 0;
    DevBuf<float2> d_ph_scratch;                   // DecFuse::ph_scratch (grows)
    // Two output buffers, written by alternate calls, so that whatever reads a call's output (the band-pass) may run on another stream
    // beside the NEXT call's decimator: the consumer's look-back (the head-room) is carried from the buffer just written into the other
    // one's head-room.  tail_jobs() = tail_jobs_dec() (the decimator's own histories: its stream) + tail_job_out() (the consumer's stream)
    HistBuf fin2, fin3;                      // fin: this call's; fin2: the next call's (its head-room filled by this call's consumer); fin3: a third, written by the call after that,
                                             // so that a call's decimator waits for the consumer of the call THREE back (long over) instead of two (often still running)

    // ---- what one call hands to the next: reset whole by release() ----
    struct Carried {
        int hist_parity = 0;           // d_xhist / d_hist_mixed: read [p], write [p ^ 1]
        int y0_cur = 0;                // the d_y0stage2 written last
        bool y0_pending = false;       // d_y0stage holds first-stage history the stage-0 head-room has not received yet (copied when a call needs it there)
        int bank_state_parity = 0;
        bool bank_state_valid = false; // the previous call took the k_mix_dec_mfma route (else the next one warms up from the first-stage history)
        int dyn_parity = 0;
        bool dyn_valid = false;        // d_dyn[dyn_parity] holds this call's fields (the previous call was such a launch and nothing was uploaded since)
        uint64_t dyn_epoch_seen = 0;
        int ovl_parity = 0;
        bool ovl_pending = false;      // d_ovl[ovl_parity] is newer than buf0's head-room
        int xtail_parity = 0;
        DecimRoute last;               // the route of the last run() (run_beside_spectrum: DecimFront::InSpectrum)
    } st;
    bool last_in_consumer() const { return st.last.front == DecimFront::InConsumer; }  // the last run() left the mixing to the consumer: buf0 was not written
    const char *front_name() const { return st.last.front_name(); }  // the kernel the last run() used for the mixer + first stage (bench / profiling labels)
    const char *rest_name() const { return st.last.rest_name(); }    // ... and for the remaining stages

    // ---- what the last call produced ----
    long long len0 = 0, len1 = 0, len_out = 0;     // lengths produced by the last run
    struct MixTail { const float2 *tail = nullptr; long long tail_pitch = 0; float2 *tail_out = nullptr; };
    MixTail mix_tail;                              // of the last run() with DecimCall::mix_in_consumer

    // ---- API ----
    // last_hist: head-room of the final buffer (what the consumer looks back at); last_gain: folded into the final stage
    int init(uint32_t channels, const design::Chain &c, long long max_in, int last_hist, float last_gain, const Tuning &t);
    void release();
    int enable_mix_in_consumer();                  // after init(), zero-stage only: allocates the consumer's overlap rows (last_hist samples each)
    bool mix_in_consumer_ready() const { return d_ovl[0].get() != nullptr; }
    int enable_double_out();                 // after init(); fails for a single-stage chain (its output is the first stage's buffer)
    bool double_out() const { return fin2.base.get() != nullptr; }
    int set_fuse_window(const float *d_window, const std::vector<float> &w);  // the owner's display transform uses this window
    bool shape_for_spectrum() const;               // the chain is the one the kernel is built for
    bool fuse_shape() const { return shape_for_spectrum() && fuse_window; }  // ... and the owner's transform has handed over its window
    // lds_free: the call asks for a first kernel that leaves LDS alone (DecimCall::lds_free)
    bool spectrum_can_run(const OscBank &osc, bool lds_free) const { return fuse_shape() && lds_free && !osc.any_transient(); }
    // fills the kernel's parameter block for a call of n samples (before the transform is launched)
    int fill_dec_fuse(hipStream_t s, DecFuse *df, const OscBank &osc, long long n);
    // what is left for the chain's stream in such a call: the mixed-sample history for a later general call (two workgroups)
    int run_beside_spectrum(hipStream_t s, const float2 *d_in, long long in_pitch, bool shared_input, long long n, const OscBank &osc, const RawSrc *raw);
    // the first kernels this call would run read raw device-format samples themselves (DecimShape::raw_front)
    bool raw_ready(const OscBank &osc, bool lds_free) const { return raw_front() && lds_free && !osc.any_transient(); }
    // a call of this many input samples is "long": chunks of 128 outputs or more, where two output buffers do as well as three
    bool long_call(long long n) const { return bank_long_call(n / (long long)chain.total, C); }
    // n must be a multiple of chain.total; any such n streams exactly (no minimum frame length)
    // oa (from OscBank::advance_job for this call, or nullptr): when the route's kernel can advance the oscillators itself it does, and
    // DecimDone::osc_advanced says so (the caller then leaves the advance out of its tail launch)
    int run(hipStream_t s, const float2 *d_in, long long in_pitch, bool shared_input, long long n, const OscBank &osc,
            hipEvent_t after_first = nullptr, const RawSrc *raw = nullptr, const OscAdvance *oa = nullptr, DecimCall call = DecimCall{}, DecimDone *done = nullptr);
    void tail_jobs(std::vector<TailJob> &jobs) const;  // after run(): what must be refreshed before the next call
    void tail_jobs_dec(std::vector<TailJob> &jobs) const;
    void tail_job_out(std::vector<TailJob> &jobs) const;
    const HistBuf &out() const { return casc.nst > 0 ? fin : buf0; }
    long long out_len() const { return len_out; }

    // ---- run()'s steps: one launcher per route (DecimRoute, decim_route.h), the rest stages, the hand-overs ----
    struct Launch { hipStream_t s; const float2 *in; long long in_pitch; bool shared_input; long long n; const OscBank &osc; const RawSrc *raw; };
    DecimCallFacts call_facts(const Launch &l, const DecimCall &call) const;
    int run_in_consumer(const DecimRoute &r);
    int run_mixer_only(const Launch &l, const DecimRoute &r);
    int run_bank_mfma(hipStream_t s, const float2 *d_in, long long n, const OscBank &osc, const OscAdvance *oa, hipEvent_t done_event, DecimDone *done);
    int report_clk(hipStream_t s, unsigned n_wg, long long L);  // waits for the launch, prints its clock counts on stderr
    int flush_y0(hipStream_t s);
    int run_edges(const Launch &l, int R);  // the two-workgroup k_mix_hb11_bank launch: a call's first outputs and its mixed history
    int run_fused(const Launch &l, const DecimRoute &r);
    int run_cic_hb(const Launch &l, const DecimRoute &r);
    int run_lean(const Launch &l, const DecimRoute &r);
    int run_hb11_bank(const Launch &l, const DecimRoute &r);
    int run_dec1(const Launch &l, const DecimRoute &r);
    int run_rest(const Launch &l, const DecimRoute &r);
    int hand_over(const Launch &l);  // what a general call leaves for a one-kernel call or a decimator inside the transform behind it
};

// ---- CFastFIR ----
struct FastFirCore {
    uint32_t C = 0, fft_n = 2048, taps = 1025;
    DevBuf<float2> d_H, d_tw;
    DevBuf<float2> d_tw128;      // 2048-point case: table of the two-wave transform (fft_t128.h)
    Tuning tun;                  // the owner's switches (init)
    int init(uint32_t channels, uint32_t fft_size, uint32_t fir_size, const Tuning &t);
    long long block_len() const { return (long long)fft_n - (taps - 1); }
    // *ok = false (and H left alone) on the reference's "Filter Parameter error"
    int design(hipStream_t s, uint32_t ch, double lo, double hi, double offset, double rate, bool *ok);
    // in: buffer with taps-1 head-room; n multiple of block_len()
    int run(hipStream_t s, const HistBuf &in, long long n, float2 *out, long long out_pitch);
    // caller-owned rows without head-room; d_tail [C][taps-1] carries the overlap between calls and is refreshed here
    // d_tail_next (2048-point plan only): a second [C][taps-1] buffer that receives the next call's overlap straight from the
    // kernel (the caller alternates the two) instead of a copy launched behind it
    // raw (2048-point plan with both tail buffers only): the rows are still in the device's sample format (`in` unused, in_pitch in IQ
    // pairs) and converted in the kernel's loads; the overlap buffers stay float2 and hold converted samples
    int run_ext(hipStream_t s, const float2 *in, long long in_pitch, float2 *d_tail, long long n, float2 *out, long long out_pitch, float2 *d_tail_next = nullptr,
                const RawSrc *raw = nullptr);
    bool raw_ready() const { return fft_n == 2048; }  // k_fastfir_t128_raw exists for this plan
    // the band-pass of a receiver without a decimator, mixing in its loads (k_fastfir_t128_mix): in = the input stream(s), n samples per
    // row; tail [C][tail_pitch] block 0's overlap of mixed samples, tail_out [C][taps-1] receives the next call's
    bool mix_ready() const { return fft_n == 2048; }
    int run_mixing(hipStream_t s, const float2 *in, long long in_pitch, bool shared_input, long long n, float2 *out, long long out_pitch,
                   const OscBank &osc, const float2 *tail, long long tail_pitch, float2 *tail_out);
};

// ---- Demod_AM ----
struct AmCore {
    uint32_t C = 0;
    double rate = 0;
    HistBuf tmp;                    // DC-blocked magnitude, head-room for the audio FIR
    DevBuf<float> d_taps;           // [C][kMaxTaps]
    DevBuf<int> d_ntaps, d_list;
    DevBuf<double> d_state;         // [C][1][2][2]
    ScanParams<1> scan;
    std::vector<int> list;
    int init(uint32_t channels, double demod_rate, long long max_n);
    int set_bandwidth(hipStream_t s, uint32_t ch, double bw);   // Demod_AM::setBandwidth, demod_am.cpp:17-21
    int set_list(hipStream_t s, const std::vector<int> &am_channels);
    // in/out rows may be the same buffer (the scan reads `in`, the FIR writes `out`)
    // defer_tail: run() leaves the refresh of tmp's head-room to the caller's tail launch (tail_jobs: the rows of the AM list only, as
    // k_save_tail -- a channel that left AM keeps the end of its last AM call there, like the idle Demod_AM's delay line, whatever the
    // lengths of the calls it sits out; not for gated calls, whose closed channels keep their history)
    int run(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n, Gate gate = Gate{nullptr, 0, 0}, bool defer_tail = false);
    long long deferred_n = 0;       // samples of the last run() whose tail refresh was left to the caller (0: none)
    void tail_jobs(std::vector<TailJob> &jobs) const { if (!list.empty() && deferred_n > 0) jobs.push_back(TailJob{tmp.data(), tmp.pitch, deferred_n, tmp.hist, 0, nullptr, 0, d_list, (int)list.size(), 0}); }
};

// ---- Demod_NFM / Demod_SAM (PLL demodulators) ----
struct PllCore {
    uint32_t C = 0;
    double rate = 0;
    int mode = 0, ntaps = 0;        // 0 NFM, 1 SAM
    PllParams pp;
    HistBuf tmp;                    // PLL output, head-room for the CFir
    DevBuf<float> d_taps_i, d_taps_q;
    DevBuf<PllState> d_state;
    DevBuf<int> d_list;
    std::vector<int> list;
    int init(uint32_t channels, double demod_rate, long long max_n, int which);
    int set_list(hipStream_t s, const std::vector<int> &channels);
    // blk_len, blk_frame: the band-pass releases whole blocks of blk_len per frame of blk_frame samples and Demod_NFM wraps its phase at the end
    // of what each frame released (k_pll_demod); 0, 0: the call is one processBlock
    int run(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n, Gate gate = Gate{nullptr, 0, 0},
            int blk_len = 0, int blk_frame = 0);
};

// ---- Demod_WFM mono ----
// ---- the RDS branch of Demod_WFM::processDataStereo (demod_wfm.cpp:296-357, 488-786) for the dmFMS channels of a WfmCore ----
// Device side (kernels_rds.h): discriminator -> Hilbert pair -> m_RdsDownConvert -> 2400 Hz low-pass -> PLL -> matched filter -> bit-rate
// resonator, slicer, block synchroniser; every completed group goes into a per-channel log with the number of the processDataStereo
// call (frame) it fell in.  Host side: m_RdsGroupQueue (a ring of RDS_Q_SIZE with the reference's head / tail arithmetic) replayed from
// that log together with its consumer, Demod::fmStereo (demod.cpp:196-226: ONE getNextRdsGroupData per frame) -- groups() hands out
// what that consumer popped, each with getNextRdsGroupData's return value (the group differs from the one before it).
struct RdsGroup { uint16_t a, b, c, d; };
struct RdsCore {
    uint32_t C = 0;
    long long cap = 0;               // demodulator-rate samples per call at most
    bool on = false;                 // allocated (first dmFMS channel of the owner)
    design::RdsDesign des;
    int D = 1;                       // the chain's decimation
    RdsParams pp{};
    HistBuf raw, mag;                // rows of double
    std::vector<HistBuf> st;         // rows of double2: st[j] the input of stage j, st[nst] the low-pass's input
    DevBuf<double2> d_lp;            // [C][cap / D]
    DevBuf<double> d_data;           // [C][cap / D] m_RdsData of the last call
    DevBuf<RdsState> d_state;
    DevBuf<RdsEvent> d_log;          // [C][log_cap]
    DevBuf<double> d_amp, d_matched;
    std::vector<DevBuf<double>> d_taps;  // per stage, oldest sample first
    std::vector<int> ntaps, newest;
    long long last_len = 0;
    struct Host {                    // m_RdsGroupQueue and its consumer
        RdsGroup q[100];
        int head = 0, tail = 0;
        RdsGroup last{0, 0, 0, 0};
        unsigned long long seen = 0; // log entries replayed
        long long frames = 0;        // frames whose pop has been replayed
        std::vector<RdsGroup> out;
        std::vector<unsigned char> changed;
        unsigned long long lost = 0; // log entries overwritten before a collect() read them
    };
    std::vector<Host> host;
    int init(uint32_t channels, double demod_rate, long long max_n);
    // queues the branch for the listed channels; block: demodulator-rate samples per processDataStereo call of the reference
    int check(long long n, int block) const;   // the sizes run() accepts (the owner asks before it queues anything of the call)
    // the frame rule check() applies; reference_history: also refuse frames below which the reference's in-place history is not the stream's
    // (what a receiver, whose frame is fixed at creation, asks when a channel is switched to dmFMS)
    int check_frame(int block, bool reference_history) const;
    int run(hipStream_t s, const float2 *in, long long in_pitch, long long n, const double *d_hilb, const int *d_list, int n_list, int block);
    int collect(hipStream_t s, uint32_t ch);   // waits for the stream, replays the channel's new log entries
    int groups(hipStream_t s, uint32_t ch, RdsGroup *g, unsigned char *changed, uint32_t cap_out, uint32_t *n_out);
    int signal(hipStream_t s, uint32_t ch, double *data, uint32_t cap_out, uint32_t *n_out);  // m_RdsData of the last call
};

// ---- the Morse digital modem behind the noise filter (plugins/MorseDigitalModem, Goertzel path; morse.hip, kernels_modem.h) ----
struct MorseStatus { int32_t wpm, above, below; uint32_t rate, samples_per_result; };  // what Morse::refreshOutput shows (morse.cpp:477-500)
struct MorseCore {
    uint32_t C = 0, in_rate = 0;
    design::Chain chain;                       // Decimator::buildDecimationChain(demodRate, 1000, 8000), morse.cpp:193
    MorseParams pp = {};
    long long cap_in = 0, rpitch = 0;          // input samples per call at most; results per channel row
    int log_cap = 0;                           // events per channel the device log holds
    std::vector<DevBuf<float>> d_taps;         // per stage
    std::vector<DevBuf<float2>> d_hist, d_out; // per stage: [C][kMaxTaps] the input's tail of the last call; [C][out_pitch] the output
    std::vector<long long> out_pitch;
    DevBuf<double> d_power;                    // [C][rpitch] this call's Goertzel powers
    DevBuf<unsigned char> d_tone;              // [C][rpitch] ... and decisions (stand-alone step only)
    DevBuf<MorseState> d_state;                // [C]
    DevBuf<MorseEvent> d_log;                  // [C][log_cap] ring
    DevBuf<int> d_list;                        // the channels the modem runs for (on, and not in dmNONE)
    std::vector<int> list;
    std::vector<unsigned char> on, tune_only;
    std::vector<int32_t> wpm;                  // where the next enable starts: m_wpmSpeedCurrent outlives setSampleRate (morse.h:223)
    struct Host { uint64_t seen = 0; std::vector<MorseEvent> q; };
    std::vector<Host> host;
    std::vector<MorseState> h_state;
    std::vector<MorseEvent> h_log;
    long long since_drain = 0;                 // results queued since the log was last drained (each adds at most one event)
    hipEvent_t done = nullptr;                 // behind the last decide launch
    bool recorded = false;
    int n_on = 0;
    bool any() const { return n_on > 0; }
    int init(uint32_t channels, uint32_t demod_rate, long long max_n, bool keep_tone);
    void release();
    int check(long long n) const;              // refusals for a call of n input samples (before anything is queued)
    int enable(uint32_t ch, bool on, int mode);  // setDigitalModem + setSampleRate (on), drop the state (off); synchronous
    int set_mode(uint32_t ch, int mode);       // Morse::setDemodMode (and dmNONE leaves the channel out); synchronous
    int run(hipStream_t s, const float2 *in, long long in_pitch, long long n);
    int drain();                               // waits for the last call, moves every channel's new events to the host
    int events(uint32_t ch, MorseEvent *ev, uint32_t cap, uint32_t *n);
    int status(uint32_t ch, MorseStatus *st);
    int upload_list();
};

struct WfmCore {
    uint32_t C = 0;
    double rate = 0;
    HistBuf a, b, c;                // low-passed IQ (hist 1), discriminator (hist FIR), FIR out
    DevBuf<float> d_taps;
    int ntaps = 0;
    bool lp_on = false;
    ScanParams<1> lp;
    ScanParams<2> dn;
    int parity = 0;
    DevBuf<double> d_lp_state[2], d_dn_state[2];
    bool fused = false;             // single-kernel FIR-ised path (k_wfm_fir); else the multi-kernel sequential fallback
    int L4 = 0, Llp = 1;            // fused: combined audio response (padded to 16) and low-pass response lengths
    DevBuf<float> d_h;              // [L4 + 16]  (k_wfm_lmr_fir)
    DevBuf<float> d_hm;             // [wfm_mx_table_floats(L4)]: the same response in the order k_wfm_fir's matrix operand walks (wfm_fir_geom.h)
    DevBuf<float> d_hlp;            // [Llp]
    DevBuf<float2> d_xtail[2];                // [C][L4 + Llp] input history, ping-pong
    const float2 *deferred_in = nullptr;      // a view of the caller's input rows, set by run(): the history copy is left to tail_jobs()
    long long deferred_pitch = 0;
    // dmFMS as the reference delivers it: processDataStereo's pilot PLL does not hold lock, so the block
    // copies the discriminator output to both channels -- processDataMono without its 75 kHz pre-filter (demod_wfm.cpp:255-293)
    std::vector<unsigned char> stereo;        // per channel: 1 = dmFMS
    DevBuf<unsigned char> d_stereo;           // device copy, uploaded by run() when dirty; null until a channel asks for it
    bool stereo_dirty = false;
    int set_stereo(uint32_t ch, bool on);
    // ... and before it drops out (at most the first blocks of a stream): k_wfm_pilot runs the discriminator, the Hilbert pair, the
    // pilot band-pass and the PLL serially per dmFMS channel and leaves the (L - R) contribution of the blocks that end locked in `lm`;
    // k_wfm_lmr_fir sends it through the audio response and adds / subtracts it.  Allocated when a channel first asks for dmFMS.
    HistBuf lm;                               // [C] rows, .x = lmr, head-room = the audio response's look-back
    long long lm_pending = 0;                 // head-room samples that may still be non-zero once no channel is in dmFMS (run() flushes them)
    DevBuf<struct WfmPilotState> d_pilot;     // [C]
    DevBuf<double> d_hilb;                    // [2][61]
    DevBuf<int> d_stereo_list;                // the dmFMS channels
    int n_stereo = 0;
    long long max_n_ = 0;
    int stereo_block = 2048;                  // samples per processDataStereo call in the reference (the owner's frame length)
    WfmPilotParams pilot;
    RdsCore rds;                              // the RDS branch (Tuning::rds = false leaves it out)
    // Demod_WFM::getStereoLock (demod_wfm.cpp:436-447): m_PilotLocked after the last block, and whether it differs from the value the
    // previous call of this function saw (m_LastPilotLocked starts as the opposite of m_PilotLocked: the first call reports a change)
    std::vector<char> stereo_ran, last_lock;
    int stereo_lock(hipStream_t s, uint32_t ch, int *lock, int *changed);
    Tuning tun;                               // the owner's switches (init)
    int init(uint32_t channels, double demod_rate, long long max_n, const Tuning &t);
    // more_tails / oa: the caller's other tail-refresh jobs and oscillator advance; when the single-kernel path runs it carries
    // them (and its own history copy) in extra workgroups of its launch and sets *carried -- the caller then skips its own
    // tail-refresh launch (one launch and ~5 us fewer on the call's critical path)
    int run(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n,
            const std::vector<TailJob> *more_tails = nullptr, const OscAdvance *oa = nullptr, bool *carried = nullptr);
    void tail_jobs(std::vector<TailJob> &jobs) const;
    long long last_n = 0;
};

// ---- AGC (application/agc.cpp), on the band-passed samples of the narrow branch ----
struct AgcCore {
    uint32_t C = 0;
    double rate = 0;
    DevBuf<struct AgcState> d_state;
    DevBuf<int> d_list;
    std::vector<int> list;          // channels the kernel visits: every mode but OFF-with-unit-gain
    struct Host { int mode = 0, threshold = 1, use_hang = 0, thr = 0, decay = 0; double slope = 0, sample_rate = 100.0, manual = 1.0; bool dirty = false; };
    std::vector<Host> host;
    int init(uint32_t channels, double demod_rate);
    int set_mode(uint32_t ch, int mode, int threshold);      // AGC::setAgcMode, agc.cpp:53-82
    std::vector<char> muted;        // channels the owner keeps out of the list (dmNONE: the reference returns before the AGC)
    void set_muted(uint32_t ch, bool m) { if (muted.size() != C) muted.assign(C, 0); if ((muted[ch] != 0) != m) { muted[ch] = m; list_dirty = true; } }
    int apply(hipStream_t s);                                // upload changed parameters and the channel list
    int run(hipStream_t s, float2 *buf, long long pitch, long long n, Gate gate = Gate{nullptr, 0, 0});
    bool list_dirty = false;
};

// ---- DCRemoval, IQBalance, NoiseBlanker on the input streams (receiver.cpp:814-823) and NoiseFilter/ANF (receiver.cpp:974) ----
struct ConditionCore {
    uint32_t S = 0, nf = 0;
    double fs = 0;
    long long cap = 0;
    struct Host { int flags = 0; double gain = 1, phase = 0; };
    std::vector<Host> host;
    bool any = false, dirty = false;
    DevBuf<float2> d_buf;             // [S][cap] conditioned copy of the input (allocated on first enable)
    DevBuf<double> d_dc_state;        // [S][1][2][2]
    DevBuf<int> d_dc_list;
    std::vector<int> dc_list;
    DevBuf<struct IqFactors> d_iq;    // [S] (gain, phase, on)
    DevBuf<struct NbState> d_nb;      // [S]
    ScanParams<1> dc;
    bool iq_any = false, nb_any = false;
    int init(uint32_t streams, uint32_t frame, double sample_rate, long long max_n);
    int set(uint32_t stream, int flags, double gain, double phase);
    int apply(hipStream_t s);
    // copies d_in to the internal buffer and runs the enabled steps on it; *out = what the rest of the call should read
    int run(hipStream_t s, const float2 *d_in, long long in_pitch, long long n, const float2 **out, long long *out_pitch);
};
struct AnfCore {
    uint32_t C = 0;
    DevBuf<struct AnfState> d_state;
    DevBuf<int> d_list;
    std::vector<int> list;
    std::vector<char> on, muted;   // muted: dmNONE channels (the reference returns before the noise filter)
    bool dirty = false;
    void set_muted(uint32_t ch, bool m) { if (muted.size() != C) muted.assign(C, 0); if ((muted[ch] != 0) != m) { muted[ch] = m; dirty = true; } }
    int init(uint32_t channels);
    int set(uint32_t ch, bool enable);
    int apply(hipStream_t s);
    int run(hipStream_t s, float2 *buf, long long pitch, long long n, Gate gate = Gate{nullptr, 0, 0});
};

// ---- the test bench's generator: NCO::genSweep + NCO::genNoise at the head of the chain (receiver.cpp:797-798; kernels_testbench.h) ----
constexpr int kTbNoiseAttempts = 32;  // polar-method attempts per sample at most (all failing: the sample gets no noise)
constexpr int kTbMinLeg = 64;         // shortest sweep leg, in samples, the per-call leg table is built for
constexpr unsigned long long kTbMaxPiece = 1ull << 26;        // longest stretch one leg-table entry covers (longer ones are split on the host)
constexpr unsigned long long kTbMaxPulsePeriod = 1ull << 28;  // pulse periods from here on are refused (the setter runs the timer's serial sum once)
struct SweepLeg { unsigned long long k0; double turns0, f0, inc; };  // from call-relative sample k0 on: phase (turns) and frequency there, Hz per sample
struct TbParams {                     // k_testbench's argument block
    double fs_inv, amp, noise_amp;
    unsigned long long n0, seed;      // absolute number of the call's first sample (pulse timer, noise counter)
    unsigned long long pulse_period, pulse_on;  // 0: no pulse modulation
    unsigned stream0;
    int n_legs, sweep_on, mix, noise_on;
};
struct TbSweepPlan { double inc = 0; unsigned long long leg = 0, pulse_period = 0, pulse_on = 0; };
int tb_plan_sweep(double fs, const pebblegpu_sweep *s, TbSweepPlan *plan);  // host only: leg length and the pulse timer's period / width in samples
// Keyed Morse stations (MorseGen, plugins/MorseGenDevice/morsegen.cpp:33-328).  Per call the host lists, station by station, the marks that
// intersect the call: (start relative to the call's first sample) * 2 + (1: dash), ascending; a mark that began in an earlier call has a
// negative start.  The call's table is one block: n stations' MorseStationDev, then all marks.
constexpr unsigned long long kMorseMaxMark = 1ull << 26;    // marks from here on are refused (the phase's product stays far inside a double)
constexpr unsigned long long kMorseMaxPeriod = 1ull << 40;  // one pass through a text
constexpr size_t kMorseMaxCallMarks = (size_t)1 << 22;      // marks of all stations in one call (a call of days of Morse is refused)
constexpr int kMorseRun = 8;                                // consecutive samples one lane makes from one sincospi (k_morsegen)
struct MorsePlan { unsigned long long spt = 0, rise = 0, dot = 0, dash = 0, period = 0; };  // samplesPerTcw, rise = fall, mark buffers, one pass
int tb_plan_morse(double fs, const pebblegpu_morse_station *st, MorsePlan *plan);  // host only
struct MorseStationDev {
    double tps, amp, inc, rot_c, rot_s;  // turns per sample (f / fs), m_amplitude, ampInc (0 with hard keying), exp(j 2 pi f / fs)
    unsigned rise, dot, dash;            // samples: rise = fall, the dot's and the dash's whole buffer
    unsigned first, count;               // this call's marks: marks[first .. first + count)
    unsigned pad;
};
struct MorseStationHost {
    MorsePlan plan;
    MorseStationDev dev = {};
    std::vector<unsigned long long> mark_off;  // one pass: where each mark starts ...
    std::vector<unsigned char> mark_dash;      // ... and which it is
    unsigned long long pos = 0;                // where in its pass the station stands at the next sample
};
// the marks of `st` that intersect the next n samples, appended to `marks` (encoded as above); does not move the station
void tb_morse_marks(const MorseStationHost &st, unsigned long long n, std::vector<long long> &marks);
int tb_morse_station(double fs, const pebblegpu_morse_station *st, MorseStationHost *out);  // plan + one pass's marks; host only

struct TestBenchCore {
    double fs = 0;
    uint32_t S = 1;
    bool sweep_on = false, noise_on = false;
    // stations: set_morse replaces them and restarts them; reset() (the sweep's and the noise's setters) leaves them alone
    std::vector<MorseStationHost> stations;
    bool morse_mix = true;
    std::vector<long long> marks_;
    DevBuf<unsigned char> d_morse[2];
    PinnedBuf<unsigned char> h_morse[2];  // the call's station table, ping-pong like the legs
    size_t morse_cap = 0;
    bool morse_on() const { return !stations.empty(); }
    int set_morse(const pebblegpu_morse_station *st, uint32_t n, int mix);  // n == 0: off
    int ensure_events();
    pebblegpu_sweep sw = {};
    TbSweepPlan plan;
    double noise_amp = 0;
    uint64_t seed = 0;
    // carried from call to call: samples since the last setter, phase in turns, and where the sweep stands in its leg
    unsigned long long n_abs = 0, leg_pos = 0, leg_len = 0;
    double turns = 0, f_leg = 0, inc = 0, start = 0, stop = 0;
    bool up = true;
    std::vector<SweepLeg> legs_;
    DevBuf<SweepLeg> d_legs[2];
    PinnedBuf<SweepLeg> h_legs[2];  // the call's leg table, ping-pong (pinned staging: no host wait per call)
    hipEvent_t h_done[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    size_t leg_cap = 0;
    int parity = 0;
    bool any() const { return sweep_on || noise_on || morse_on(); }
    int init(double sample_rate, uint32_t streams);
    void release();
    void reset();                                        // TestBench::reset
    int set_sweep(const pebblegpu_sweep *s);             // nullptr: off
    int set_noise(double amplitude, uint64_t seed);      // amplitude <= 0: off
    int build_legs(long long n, std::vector<SweepLeg> &legs);
    int run(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n, uint32_t streams, uint32_t stream0);
    int draws(hipStream_t s, uint32_t stream, uint64_t first, uint32_t n, uint32_t *r, uint8_t *attempt);
};

// ---- CFractResampler (complex), pebblelib/fractresampler.cpp ----
struct ResampCore {
    uint32_t C = 0, nf = 0;                  // nf: the shortest part (max_out's bound on outputs lost to rounding per part)
    // The reference resamples what each of its frames hands on, and takes the frame's length off its running time sum after each
    // (fractresampler.cpp:186).  parts: those lengths over one super-frame, in order -- {nf} for a WFM receiver and wherever the band-pass's
    // block divides the frame; the blocks each frame released otherwise (a frame that released none runs nothing).  The sum's rounding
    // follows the partition: with a rational ratio such as 48000 / 11025 an output time lands on a whole sample every 147 outputs, and
    // another partition delivers that output one call earlier or later.
    std::vector<uint32_t> parts;
    uint64_t period = 0;                     // their sum: the demodulator-rate samples of one super-frame
    double dt = 1.0, float_time = 0.0;     // Rate = input rate / output rate; m_FloatTime
    DevBuf<float> d_sinc;
    DevBuf<float2> d_hist[2];                // [C][28] last inputs of the previous call, ping-pong
    DevBuf<struct ResampFrame> d_frames;
    PinnedBuf<struct ResampFrame> h_frames[2];
    hipEvent_t h_done[2] = {nullptr, nullptr};
    int parity = 0, pin = 0;
    uint32_t max_frames = 0;
    int init(uint32_t channels, const std::vector<uint32_t> &parts_per_superframe, double rate, uint32_t superframes_per_call);
    void release();
    long long max_out(long long n) const { return (long long)((double)n / dt) + (long long)(n / (nf ? nf : 1)) + 8; }
    // n: whole super-frames; returns the output count of this call in *n_out (no device sync)
    int run(hipStream_t s, const float2 *in, long long in_pitch, long long n, float2 *out, long long out_pitch, long long *n_out);
};

// ---- FFT::fftSpectrum ----
struct SpectrumCore {
    uint32_t S = 0, nf = 2048, bins = 0;
    DevBuf<float> d_prev[2];
    DevBuf<float> d_window;
    DevBuf<float2> d_btab, d_tw_nf;                // btab: [bins/nf][32] wave-uniform pre-twiddle factors
    DevBuf<float2> d_btab128, d_tw128;                // the same for the two-wave transform (fft_t128.h), 8192 bins
    DevBuf<float2> d_ftab;            // [bins/nf][nf] window[n] * W_bins^{n q}: the one factor per point of k_spectrum_q128
    std::vector<float> h_window;      // host copy of the window (the decimator's taps against windowed samples)
    bool last_fullc = false;          // the last run used k_spectrum_t128's register-held twiddles (nothing ran beside it)
    Tuning tun;                       // the owner's switches (init)
    bool use_w64 = false;             // 8192 bins on k_spectrum_w64 (Tuning::spectrum_w64)
    int stagger = 0, pad_lds = 0;     // k_spectrum_t128: barrier intervals between the two halves of a 1024-item workgroup (0: 512-item workgroups)
    bool per_q = false;               // k_spectrum_q128 (one transform per 128-item workgroup) instead of the shared-frame kernels
    // 65536-sample frames / 65536 bins (four-step, kernels_spectrum.h): the [S][F][32][2048] intermediate
    bool big = false;
    DevBuf<float2> d_Y;               // (grows)
    float scale = 0;
    int parity = 0;
    // any other frame length, and frames shorter than samplesPerBuffer (un-windowed): k_spectrum_any
    bool any = false;                 // the frame length / bin count has none of the kernels above: every call takes the general kernel
    int any_M = 0, any_logM = 0, any_zp_log2 = 0;
    DevBuf<float2> d_twM;             // W_M^k, k < M / 2
    int run_any(hipStream_t s, const float2 *d_in, long long in_pitch, long long n_frames, float *d_out, int n_in, bool windowed);
    int init(uint32_t streams, uint32_t frame, uint32_t fft_size, const Tuning &t);
    int size_Y(hipStream_t s, long long per_stream, long long *bs);  // the stream batch of a 65536-point call; grows d_Y to hold one
    int run(hipStream_t s, const float2 *d_in, long long in_pitch, long long n_frames, float *d_out, const RawSrc *raw = nullptr, const DecFuse *df = nullptr, bool nothing_beside = false);
    // the transform over a frame list (the update timer's selection, k_spectrum_list_*): rows compact, |X_prev| = the previous listed frame
    const float2 *d_list_ftab = nullptr, *d_list_tw128 = nullptr;  // views: k_spectrum_list_q128's tables -- d_ftab / d_tw128 where k_spectrum_q128 is the plan's, else the two below
    DevBuf<float2> own_list_ftab, own_list_tw128;
    int init_list();
    int run_list(hipStream_t s, const float2 *d_in, long long in_pitch, const uint32_t *idx, long long n_sel, float *d_out, const RawSrc *raw = nullptr);
    int run_list_big(hipStream_t s, const float2 *d_in, long long in_pitch, const uint32_t *idx, long long n_sel, float *d_out, const RawSrc *raw);  // 65536 points
    bool dec_ready() const { return !big && !per_q && bins == 8192 && !use_w64; }  // k_spectrum_t128<.., DEC> exists for this plan
    bool raw_ready() const { return !big && !any && !per_q && bins == 8192; }  // k_spectrum_t128 converts in its loads (2048-sample frames only)
    bool raw_ready_big() const { return big && !tun.big_split32; }      // k_big256_cols_raw converts in its loads (the stream bank's raw calls)
};

// HIP events around each kernel group, kept for the last kRing calls so a caller can run calls back to back
// (no host sync per call) and read the per-kernel durations afterwards.
struct Timers {
    static constexpr int kRing = 64;
    hipEvent_t ev[kRing][8] = {};
    hipEvent_t start_ev[kRing] = {};  // where the call began (its ev[0])
    hipEvent_t end_ev[kRing] = {};    // where it ended: its ev[6], or the next call's ev[0] (a side-by-side call records no end of its own)
    int open_slot = -1;               // the last call's end is not known yet (Receiver::close_timing)
    bool detailed[kRing] = {};   // per-kernel events (2..5) were recorded for that call
    bool has_mid[kRing] = {};    // event 1 (behind the display transform) was recorded: calls without a spectrum skip it unless profiling
    uint64_t calls = 0;
    hipEvent_t *slot() { return ev[calls % kRing]; }
};

// SignalSpectrum's update timer (m_spectrumTimer / m_hiResTimer, signalspectrum.cpp:63-113) on the stream's own sample clock: frames are
// numbered from the handle's creation, the first one starts the timer and gets no spectrum, after that frame f gets one iff
// (f - f_last) * frame_len * 1000 / rate >= period_ms in integer arithmetic, and then becomes f_last.  Host only: the list is known
// before anything is queued.
struct UpdateTimer {
    bool started = false;
    uint64_t next = 0;    // number of the next frame of the stream
    uint64_t f_last = 0;  // the frame that last restarted the timer
    // the n frames of a call; the selected ones, relative to the call's first frame, are appended to *sel.
    // ups -1: every frame gets a spectrum and restarts the timer (nothing is appended); 0: none does (m_updatesPerSec == 0)
    void advance(int ups, uint64_t period_ms, uint64_t n, uint64_t frame_len, uint64_t rate, std::vector<uint32_t> *sel);
};

class Receiver {
public:
    int create(const pebblegpu_config *cfg);
    // SignalSpectrum::setUpdatesPerSec (signalspectrum.cpp:124-135); PEBBLEGPU_SPECTRUM_EVERY_FRAME (-1, the default): no gate
    int set_spectrum_updates(int updates_per_sec);
    // which frames of the last call got an unprocessed (zoomed) spectrum, relative to the call's first frame
    int spectrum_frames(bool zoomed, uint32_t *idx, uint32_t cap, uint32_t *n) const;
    bool gated() const { return spec_ups_ != -1; }
    ~Receiver();
    int set_mixer(uint32_t ch, double f);
    int set_bandpass(uint32_t ch, double lo, double hi);
    int set_mode(uint32_t ch, int mode);
    int set_agc(uint32_t ch, int mode, int threshold);
    int set_conditioners(uint32_t stream, int flags, double iq_gain, double iq_phase);
    int set_noise_filter(uint32_t ch, bool on);
    int process_raw(int fmt, int order, double gain, const void *d_raw, uint64_t n);  // normalizeIQ on the library's stream, then process()
    // host ingest through library-owned pinned buffers (two slots): the device plugin writes its raw samples into a slot, the upload
    // of one slot travels on a copy stream while the call on the other computes
    int ingest_acquire(uint32_t slot, uint64_t bytes, void **host_ptr);
    int ingest_submit(uint32_t slot, uint64_t bytes);
    int process_ingested(uint32_t slot, int fmt, int order, double gain, uint64_t n);
    // The same three steps for an owner of several receivers that share ONE pinned host buffer (the multibank's slots, multibank.hip):
    // the receiver keeps only the slot's device twin (a second ring, so that the two ways in never mix).  ingest_wait blocks until the
    // last call that read the twin is over; ingest_upload queues the copy of `bytes` from h_src on the copy stream; process_uploaded
    // is process_raw on the twin, ordered behind that copy on the device.
    int ingest_wait(uint32_t slot);
    int ingest_upload(uint32_t slot, const void *h_src, uint64_t bytes);
    int process_uploaded(uint32_t slot, int fmt, int order, double gain, uint64_t n);
    int set_squelch(uint32_t ch, double squelch_db);   // Receiver::squelchChanged, receiver.cpp:704-707
    // dmFMS channels of a WFM bank: what Demod::fmStereo took from the RDS group queue since the last call (waits for queued work)
    int rds_groups(uint32_t ch, RdsGroup *g, unsigned char *changed, uint32_t cap, uint32_t *n);
    int stereo_lock(uint32_t ch, int *lock, int *changed);
    // the digital-modem hook between the noise filter and the AGC (receiver.cpp:977-980): the Morse decoder per channel
    int set_morse(uint32_t ch, bool on);
    int morse_events(uint32_t ch, MorseEvent *ev, uint32_t cap, uint32_t *n);
    int morse_status(uint32_t ch, MorseStatus *st);
    // the test bench on the batched path: the generator at the head of the chain (TestBench::genSweep / genNoise, receiver.cpp:797-798) and
    // copies of the signal at the reference's displayData points (:803, :945, :953, :992) and at the digital-modem hook (:979-980)
    int set_testbench_sweep(const pebblegpu_sweep *s);
    int set_testbench_noise(double amplitude, uint64_t seed);
    int set_testbench_morse(const pebblegpu_morse_station *stations, uint32_t n_stations, int mix);
    int set_taps(uint32_t mask);
    const float2 *tap(int point, uint64_t *n_per_row, uint64_t *pitch, double *rate) const;
    // the conditioned copy of the streams the last call read (ConditionCore::d_buf); NULL and zeros when that call conditioned nothing
    const float2 *conditioned(uint64_t *n_per_stream, uint64_t *pitch) const;
    int process(const float2 *d_iq, uint64_t n, bool with_spectrum, bool with_chain, const RawSrc *raw = nullptr);
    // spectrum_updated (may be null): whether this frame got a spectrum (always, without the update timer)
    int process_iq(const double *iq, uint16_t n, double *audio, uint32_t *n_audio, double *spectrum_db, uint32_t *spectrum_updated = nullptr);
    // FFT::mapFFTToScreen of frames first + j * step (j < n) of the last call's unprocessed spectrum (zoom = false) or zoomed spectra
    // (zoom = true; edges per channel), queued behind that call's transform and ahead of the next call's: out [stream][n][x_pixels]
    int map_spectrum(bool zoom, const int32_t *edges, bool per_stream, int32_t y_pixels, int32_t x_pixels, double max_db, double min_db,
                     uint32_t first, uint32_t n, uint32_t step, int32_t *d_out);
    // host egress (egress.h): the audio output stage (Audio::SendToOutput, receiver.cpp:1029-1035) and IQ recording (receiver.cpp:800-801),
    // each a ring of pinned slots filled behind the call; open / close / the level setter take the handle's lock, the reader's
    // next / release take the ring's own
    int audio_out_open(int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots);
    int audio_out_close();
    int set_audio_level(uint32_t ch, float gain, int mute);  // Receiver::m_gain (0..100), m_mute
    int audio_out_next(int wait, pebblegpu_audio_block *b);
    int audio_out_release(uint64_t call_index);
    int audio_out_dropped(uint64_t *blocks);
    int record_open(uint32_t n_slots);
    int record_close();
    int record_next(int wait, pebblegpu_audio_block *b);
    int record_release(uint64_t call_index);
    // the modem hook ring: the rows m_iDigitalModem->processBlock receives (receiver.cpp:979-980) for a selection of channels, with a
    // trailer that says which (row, super-frame) the reference would have handed to the hook at all
    int modem_out_open(int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots);
    // the same ring with every row through the reference's Decimator chain for (max_bw, min_rate) on the device (k_modem_rate_pack)
    int modem_out_open_rate(int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots, uint32_t max_bw, uint32_t min_rate);
    int modem_out_close();
    int modem_out_next(int wait, pebblegpu_modem_block *b);
    int modem_out_release(uint64_t call_index);
    int modem_out_dropped(uint64_t *blocks);
    // the display ring (display.hip): the rows a call's display transforms computed, one or two panes per block, through the same slots
    int display_open(const pebblegpu_display_pane *panes, uint32_t n_panes, uint32_t n_slots);
    int display_close();
    int display_set_pane(uint32_t pane, const pebblegpu_display_pane *p);
    int display_next(int wait, pebblegpu_display_block *blocks);
    int display_release(uint64_t call_index);
    int display_dropped(uint64_t *blocks);
    // SpectrumWidget's auto-scale (recalcScale, spectrumwidget.cpp:693-734; kernels_display.h): the pull function -- the scale of frames
    // first + j * step of the last call's unprocessed spectrum, d_out [stream][n], queued where map_spectrum queues -- and the ring's
    // flags: host state consumed when the next call is queued, never a wait
    int spectrum_scale(uint32_t first, uint32_t n, uint32_t step, pebblegpu_display_scale *d_out);
    int display_set_auto_scale(uint32_t flags);
    int display_rescale();
    int display_scale(uint64_t call_index, pebblegpu_display_scale *out, uint32_t cap, uint32_t *n);
    int sync();
    int close_timing();  // records the end event a side-by-side call left out (no-op otherwise)
    const char *kernel_name(int which) const;  // the kernels behind pebblegpu_receiver_last_ms's groups, as last run

    int device = 0;
    double fs = 0;
    uint32_t nf = 2048, C = 1, S = 1, bins = 0, ff_n = 2048, ff_taps = 1025, max_sf = 1;
    bool shared_input = false, wfm = false;
    design::Chain chain;
    uint32_t demod_rate_int = 0;
    uint64_t superframe = 0;
    uint64_t last_audio_n = 0, last_spec_frames = 0;
    Timers tm;
    HistBuf audio;   // [C][k*nf]
    DevBuf<float> d_spec;
    // SignalSpectrum::zoomed (signalspectrum.cpp:89-113): the display transform of every decimated frame of every channel
    uint32_t zoom_bins = 0;
    DevBuf<float> d_zoom;             // [C][max_sf * superframe / (D * nf)][zoom_bins]
    uint64_t last_zoom_frames = 0;
    // the update timer (set_spectrum_updates): -1 no gate; with a gate last_spec_frames / last_zoom_frames count the COMPUTED rows of
    // the last call (compact in d_spec / d_zoom) and sel_spec_ / sel_zoom_ say which frames they are
    int spec_ups_ = -1;
    uint64_t spec_period_ms_ = 100;   // 1000 / m_updatesPerSec of the last rate above 0 (the reference's default: 10 per second)
    UpdateTimer ut_spec_, ut_zoom_;
    std::vector<uint32_t> sel_spec_, sel_zoom_;
    // what the S-meter and the squelch read between two updates (getUnprocessed(), receiver.cpp:891-897, 959-965): the latest computed
    // row per stream, carried across calls, and its S-meter per channel (refreshed with the channel's current band at every call)
    DevBuf<float> d_spec_carry;       // [S][bins]
    DevBuf<float4> d_sm_carry;        // [C]
    bool have_carry_ = false;
    // SignalStrength::fdEstimate per frame (S-meter): enabled on request, needs the spectrum
    bool smeter_on = false;
    DevBuf<float4> d_smeter;          // [C][max frames]
    DevBuf<SmBins> d_sm_bins;
    long long smeter_pitch = 0;
    int enable_smeter(bool on);
    double squelch_db_ = -120.0;      // DB::minDb: the gate never closes (receiverwidget.cpp:82); the one-channel, one-super-frame shape
    // banks (or calls of several super-frames): a per-channel threshold, decided on the device per (channel, super-frame)
    std::vector<float> squelch_;      // per channel, -120 = never closes
    bool bank_gate_ = false, squelch_dirty_ = false;
    DevBuf<float> d_squelch;
    DevBuf<unsigned char> d_gate;     // [C][max_sf]
    PinnedBuf<float4> h_gate_;        // pinned: the S-meter value the gate reads back
    uint64_t squelched_calls = 0;
    bool failed_ = false;             // a process call failed after it had started queueing work: the handle is refused from then on
    bool profile_detail = false;      // record the per-kernel events too (pebblegpu_receiver_set_profiling)
    uint32_t audio_rate = 0;          // 0: audio stays at the demod rate (the resampRate == 1 branch, receiver.cpp:1000-1003)
    DevBuf<float2> d_audio_rs;        // [C][rs_pitch] resampled audio
    long long rs_pitch = 0;
    const float2 *audio_ptr() const { return audio_rate ? d_audio_rs.get() : audio.data(0); }
    long long audio_pitch() const { return audio_rate ? rs_pitch : audio.pitch; }

private:
    struct ChanCtl {
        int mode = 0;
        double lo = 0, hi = 0, am_bw = 16000;  // Demod_AM ctor default (demod_am.cpp:9)
        bool bp_valid = false, bp_dirty = false, am_dirty = true;
    };
    int apply_controls(hipStream_t osc_stream);
    // One process call (receiver.hip): its route is planned once (call_route.h) from call_facts(), then its stages are queued in order.
    // What the stages hand to one another lives in one Call on the stack of process().
    struct Call {
        uint64_t n = 0;
        bool with_spectrum = false, with_chain = false;
        CallRoute rt;
        hipEvent_t *ev = nullptr;         // the call's timing slot (Timers::slot) ...
        int slot = 0;                     // ... and its number
        hipStream_t cs = nullptr;         // where the chain is being queued (the chain's stream from the fork or the hand-over on)
        const float2 *d_iq = nullptr;     // the input as the next stage reads it ...
        long long in_pitch = 0;           // ... and its row pitch
        const float2 *tap_iq = nullptr;   // the input before the conditioners (raw-IQ tap, recording)
        const RawSrc *raw = nullptr;      // raw source while the call's kernels convert in their own loads (null once staged)
        RawSrc rec_raw = {nullptr, 0, 0, 0.f, 0};  // what the recording ring reads of a raw call
        bool rec_from_raw = false;
        OscAdvance oa_pre = {};           // the oscillators' advance offered to the decimator (cleared when its kernel carried it)
        bool have_oa = false;
        DecFuse df;                       // the in-transform decimator's parameter block (CallRoute::fuse_dec)
        bool carry_before = false;        // a computed spectrum from before this call exists
        uint64_t disp_spec_rows = 0, disp_zoom_rows = 0;  // the display ring's block: the rows THIS call computes (never a carried one)
        long long nd = 0;                 // decimated samples per channel
        bool gate_closed = false;         // the call ends behind the band-pass: squelch read-back below the threshold, or tune-only mode
        bool tails_carried = false;       // the WFM kernel's launch carried the call's tail refresh
    };
    int refuse_call(const float2 *d_iq, uint64_t n, bool with_spectrum, bool with_chain, const RawSrc *raw) const;
    CallFacts call_facts(uint64_t n, bool with_spectrum, bool with_chain, bool raw) const;
    int join_and_apply(Call &c);
    int stage_input(Call &c);
    int start_call(Call &c);
    int run_display_transform(Call &c);
    int tap_and_record_input(Call &c);
    int end_without_chain(Call &c);
    int run_decimator(Call &c);
    int run_zoomed_transform(Call &c);
    int bandpass_and_gate(Call &c);
    int tail_closed(Call &c);
    int tail_bank_gated(Call &c);
    int tail_narrow(Call &c);
    int tail_wfm(Call &c);
    int finish_chain(Call &c);
    int end_call(Call &c);
    int join_streams();
    int raw_stage(float2 **p);
    int handover_event(hipEvent_t *e);
    int read_gate(hipStream_t cs, const float4 *src, bool *closed);
    int clear_tune_only_rows(hipStream_t cs, float2 *row0, long long pitch, long long n);
    int measure_carry(hipStream_t st);
    int process_slot(IngestRing &ring, uint32_t slot, int fmt, int order, double gain, uint64_t n);
    std::mutex mu_;
    hipStream_t stream_ = nullptr;
    // The display transform is arithmetic-bound and the front of the chain memory-bound: when the chain's first kernel
    // needs no LDS (the register front ends) the two run side by side, the chain on its own stream between a fork and a
    // join event.
    hipStream_t chain_stream_ = nullptr;
    // No events of its own: the chain stream waits for the call's start event, the call's end event is recorded on the chain
    // stream once it has also seen the transform's end event, and whatever next touches the main stream (the next call, a
    // synchronise) first waits for that end event.  Every event record costs the stream ~5 us, so none is spent on the fork/join.
    hipEvent_t spec_end_ = nullptr;   // pipelined calls: the last display transform queued on the main stream (for the chain's stream to wait on at a join)
    Tuning tun_;                      // the switches, read when the receiver is created
    bool touched_ = true;             // a setter ran since the last call
    bool bank_pipe_ok_ = false;       // no display transform: the call's two stages (decimator | band-pass .. resampler) on the two streams, stage 2 beside the next call's stage 1
    hipEvent_t f_end_[3] = {nullptr, nullptr, nullptr};  // where stage 2 of the last three such calls ended
    std::vector<std::pair<const void *, hipEvent_t>> out_reader_;  // per decimator output buffer: where the second stage that last read it ended
    hipEvent_t d_end_prev_ = nullptr;           // where the last call ended, if that was a two-stage call (the next one is timed from there)
    hipEvent_t sync_ev_[4] = {nullptr, nullptr, nullptr, nullptr};  // stage 1 -> stage 2 hand-over events (no timing), a ring
    hipEvent_t pipe_ev_ = nullptr;
    hipEvent_t chain_end_ = nullptr;  // set when a two-stream call failed half-way: what was queued on the chain stream, for the main stream to wait on
    hipStream_t zoom_stream_ = nullptr;  // where the last call's zoomed spectra were written (a map of them queues there)
    hipEvent_t map_ev_ = nullptr;     // behind a map queued on the chain's stream: what a join waits for instead of the call's end
    std::vector<ChanCtl> ctl_;
    bool am_list_dirty_ = true, sm_dirty_ = true;
    long long pll_cap_ = 0;
    OscBank osc_;
    DecimCore dec_;
    FastFirCore ff_;
    AmCore am_;
    PllCore nfm_, sam_;
    WfmCore wfmc_;
    AgcCore agc_;
    ConditionCore cond_;
    AnfCore anf_;
    MorseCore morse_;
    TestBenchCore tb_;
    uint64_t last_cond_n_ = 0;        // samples per stream the last call conditioned (0: it conditioned nothing, or was refused)
    bool last_tb_ = false;            // the last call ran the generator (kernel_name)
    bool last_tb_morse_ = false;      // ... with stations on: k_morsegen instead of k_testbench
    int last_input_ = -2;             // the last call's input route (kernel_name(6)): -2 no call yet, -1 float2, 0..4 raw of that format
                                      // converted in the kernels' loads, 5 raw staged through k_normalize_iq
    // taps: one buffer per enabled point (allocated when the point is first enabled), filled by a copy queued on the stream that has
    // just produced the signal; index = the point's number (PEBBLEGPU_TAP_*)
    static constexpr int kTapPoints = 17;
    static constexpr uint32_t kTapsBehindGate = 1u << PEBBLEGPU_TAP_MODEM | 1u << PEBBLEGPU_TAP_POST_DEMOD;  // points a closed squelch gate never reaches
    uint32_t taps_ = 0;
    DevBuf<float2> d_tap_[kTapPoints];
    uint64_t tap_n_[kTapPoints] = {};
    int copy_tap(hipStream_t s, int point, const float2 *src, long long src_pitch, long long n, uint32_t rows);
    ResampCore resamp_;
    SpectrumCore spec_, zoom_;
    DevBuf<float2> d_stage_in_;
    DevBuf<float2> d_raw_stage_;      // process_raw: the normalised copy of a raw device-format call (allocated on first use)
    IngestRing ingest_;               // the pinned double buffer of ingest_acquire / _submit / process_ingested (ingest.h)
    IngestRing ext_ingest_;           // device twins of somebody else's pinned slots (ingest_wait / _upload / process_uploaded)
    std::vector<float> h_frame_, h_out_;
    uint64_t acc_frames_ = 0;
    EgressRing aout_, rec_;           // the audio output ring and the recording ring (egress.h); closed: a call queues nothing for them
    int aout_format_ = 0;
    std::vector<uint32_t> aout_sel_;  // row r of a block is channel aout_sel_[r]
    struct Level { float gain = 100.f; bool mute = false; };  // Receiver::m_gain / m_mute defaults
    std::vector<Level> levels_;       // per channel (kept while the ring is closed)
    DevBuf<EgressRow> d_aout_tab_;    // [C] the selected rows' (g, mute, source row)
    bool aout_tab_dirty_ = false;
    int upload_audio_table();
    int queue_audio_block(hipStream_t s, uint64_t n);
    int queue_record_block(hipStream_t s, const float2 *iq, const RawSrc *raw, uint64_t n);
    EgressRing mout_;                 // the modem hook ring; closed: a call queues nothing for it
    std::vector<uint32_t> mout_sel_;  // row r of a block is channel mout_sel_[r]
    DevBuf<uint32_t> d_mout_tab_;     // [C] the selected rows: channel | kModemRowTuneOnly
    bool mout_tab_dirty_ = false;
    int upload_modem_table();
    int modem_out_open_plan(int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots, const ModemRatePlan *plan);
    bool mrate_on_ = false;           // the open ring decimates (set under mout_.mu at open; a plain ring, or an empty chain: false)
    ModemRatePlan mrate_;
    DevBuf<float> d_mrate_taps_;      // [stage][kMaxTaps]
    DevBuf<float2> d_mrate_carry_;    // [2][rows][H]: the last H delivered demodulator samples of every row, read at mrate_parity_
    int mrate_parity_ = 0;
    int queue_modem_block(hipStream_t s, long long spf, int n_sf, const unsigned char *gate);
    struct DisplayRing *disp_ = nullptr;  // allocated at the first open, kept until the receiver goes (a reader may hold it)
    bool disp_open_ = false;          // (under mu_: what a process call looks at)
    int upload_display_tables();
    int queue_display_block(hipStream_t spec_s, uint64_t spec_rows, hipStream_t zoom_s, uint64_t zoom_rows, bool rescale);
    bool display_scale_pending() const;  // the ring is open with an auto-scale flag on and a recalc requested (CallFacts::scale_pending)
    void display_destroy();
};

}  // namespace pg

// the handle of include/pebblegpu.h (pebblegpu_abi.hip has its entry points; multibank.hip owns one per shard)
struct pebblegpu_receiver {
    pg::Receiver rx;
};
