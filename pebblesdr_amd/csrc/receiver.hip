// receiver.hip -- the receiver bank: Receiver::processIQData's DSP (application/receiver.cpp:826-987)
// for C tuned channels, composed from the device cores in the reference's step order.
#include <cmath>
#include <map>
#include "receiver.h"

namespace pg {

int Receiver::create(const pebblegpu_config *cfg)
{
    device = cfg->device;
    fs = cfg->sample_rate;
    nf = cfg->frames_per_buffer ? cfg->frames_per_buffer : 2048;  // settings.cpp:57
    C = cfg->n_channels;
    shared_input = cfg->shared_input != 0;
    S = shared_input ? 1 : C;
    wfm = cfg->wfm != 0;
    bins = cfg->spectrum_bins;
    ff_n = cfg->fastfir_fft ? cfg->fastfir_fft : 2048;      // fastfir.cpp:65
    ff_taps = cfg->fastfir_taps ? cfg->fastfir_taps : 1025;  // fastfir.cpp:66
    max_sf = cfg->max_superframes ? cfg->max_superframes : 1;
    if (C == 0 || fs <= 0 || fs > 4.0e9 || fs != std::floor(fs)) return fail(PEBBLEGPU_E_INVALID, "bad channel count or sample rate");
    if (nf < 256 || nf > 65535) return fail(PEBBLEGPU_E_INVALID, "frames_per_buffer must be 256..65535 (quint16, device_interfaces.h:32)");
    // FastFirCore::init's rule, here in front of everything that is created: the super-frame below is computed from these sizes
    if (!wfm && (ff_taps < 2 || ff_taps > ff_n / 2 + 1)) return fail(PEBBLEGPU_E_INVALID, "FastFIR taps must be in [2, fft/2 + 1] (got %u for fft %u)", ff_taps, ff_n);
    PG_HIP(hipSetDevice(device));
    PG_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    PG_HIP(hipStreamCreateWithFlags(&chain_stream_, hipStreamNonBlocking));
    tun_ = read_tuning();
    for (auto &row : tm.ev)
        for (auto &e : row) PG_HIP(hipEventCreate(&e));

    chain = design::build_chain((uint32_t)fs, wfm ? 200000u : 30000u, 0);  // receiver.cpp:195,213
    // An empty chain is the reference's own case at its default rate (48000: no design has fs >= 30000 / wPass) and for WFM below 500 kHz:
    // Decimator::process copies (decimator.cpp:155-160), total = 1, no gain to restore, the demodulator runs at the input rate
    if (chain.stages.size() > (size_t)kMaxStages)
        return fail(PEBBLEGPU_E_UNSUPPORTED, "sample rate %.0f yields a decimation chain of %zu stages; at most %d are built", fs, chain.stages.size(), kMaxStages);
    demod_rate_int = (uint32_t)(int)chain.rate;  // int members, receiver.h:165-166
    superframe = design::superframe_len(chain, nf, ff_n, ff_taps, wfm);
    const long long max_n = (long long)max_sf * (long long)superframe;
    const long long nd_max = max_n / chain.total;

    ctl_.assign(C, ChanCtl());
    for (auto &c : ctl_) c.mode = wfm ? PEBBLEGPU_DM_FMM : PEBBLEGPU_DM_AM;  // Demod ctor default dmAM, demod.cpp:56
    if (int rc = osc_.init(C, fs)) return rc;
    osc_.allow_inline = true;
    osc_.device_advance = true;  // (banks of more than kOscInline channels: no per-call copy of the oscillators' phases)
    // "Restore gain lost in decimation" 10^(2*stages/20) only on the narrow branch (receiver.cpp:935-938 vs :854-901)
    const float gain = wfm ? 1.f : (float)std::pow(10.0, (double)(chain.dec_by2 * 2) / 20.0);
    if (int rc = dec_.init(C, chain, max_n, wfm ? 0 : (int)ff_taps - 1, gain, tun_)) return rc;
    if (int rc = audio.alloc((int)C, 0, nd_max)) return rc;
    if (!wfm) {
        // Two-stage calls (the band-pass and everything behind it on the chain's stream, beside the NEXT call's decimator): needs the
        // decimator's output twice (PEBBLEGPU_BANK_PIPELINE=0 keeps every call on one stream)
        bank_pipe_ok_ = tun_.bank_pipeline && chain.stages.size() > 1 && !bins;
        if (bank_pipe_ok_) {
            if (int rc = dec_.enable_double_out()) return rc;
            // The second stage runs in what the decimator leaves idle: its stream has the lower priority, so that when a call's decimator
            // and the previous call's band-pass become ready together (both wait for the same launch) the decimator's workgroups are placed
            // first -- the other way round the band-pass filled the CUs and the decimator, one 230-register wave per SIMD, took 112 us
            // instead of 65 waiting for room
            int lo = 0, hi = 0;
            PG_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
            (void)hipStreamDestroy(chain_stream_);
            chain_stream_ = nullptr;
            PG_HIP(hipStreamCreateWithPriority(&chain_stream_, hipStreamNonBlocking, lo));
        }
        if (int rc = ff_.init(C, ff_n, ff_taps, tun_)) return rc;
        // an empty chain under the 2048-point band-pass: the band-pass may mix in its own loads (PEBBLEGPU_NO_FUSED_DEC=1 keeps k_mixer)
        if (dec_.zero_stage && ff_.mix_ready() && !tun_.no_fused_dec) { if (int rc = dec_.enable_mix_in_consumer()) return rc; }
        if (int rc = am_.init(C, (double)demod_rate_int, nd_max)) return rc;  // Demod_AM(m_inputSampleRate), demod.cpp:62
        // Demod_SAM / Demod_NFM objects also exist in every Receiver (demod.cpp:63-64); their buffers are allocated on first use
        pll_cap_ = nd_max;
        if (int rc = agc_.init(C, (double)demod_rate_int)) return rc;  // AGC(m_demodSampleRate, m_demodFrames), receiver.cpp:264
        if (int rc = anf_.init(C)) return rc;
    } else {
        if (int rc = wfmc_.init(C, (double)demod_rate_int, nd_max, tun_)) return rc;  // Demod_WFM(m_inputWfmSampleRate), demod.cpp:65
        wfmc_.stereo_block = (int)nf;  // the reference demodulates one accumulated frame per call (receiver.cpp:896)
    }
    if (int rc = cond_.init(S, nf, fs, max_n)) return rc;
    if (int rc = tb_.init(fs, S)) return rc;
    audio_rate = cfg->audio_rate;
    if (audio_rate) {
        // resampRate = (m_demodSampleRate*1.0) / (m_audioOutRate*1.0), the int members (receiver.cpp:901,994)
        const double rr = ((double)demod_rate_int * 1.0) / ((double)audio_rate * 1.0);
        if (rr == 1.0) audio_rate = 0;  // copyCPX branch (receiver.cpp:1002-1003)
        else {
            // what each frame of the reference hands the resampler: the frame (WFM, receiver.cpp:901), or the blocks the band-pass released
            // at its end (receiver.cpp:950, 994) -- floor((k + 1) nf / L) - floor(k nf / L) of them, the frame itself wherever L divides nf
            std::vector<uint32_t> parts;
            const uint64_t per_sf = superframe / chain.total;
            if (wfm) parts.push_back(nf);
            else {
                const uint64_t L = (uint64_t)ff_.block_len();
                for (uint64_t k = 0; k < per_sf / nf; k++) {
                    const uint64_t r = ((k + 1) * nf) / L - (k * nf) / L;
                    if (r) parts.push_back((uint32_t)(r * L));
                }
            }
            if (int rc = resamp_.init(C, parts, rr, (uint32_t)(nd_max / (long long)per_sf))) return rc;
            rs_pitch = resamp_.max_out(nd_max);
            PG_TRY(d_audio_rs.alloc((size_t)rs_pitch * C));
        }
    }
    if (bins) {
        if (int rc = spec_.init(S, nf, bins, tun_)) return rc;
        bins = spec_.bins;
        PG_TRY(d_spec.alloc((size_t)(max_n / nf) * bins * S));
        if (tun_.fuse_dec && spec_.dec_ready() && nf == 2048) { if (int rc = dec_.set_fuse_window(spec_.d_window, spec_.h_window)) return rc; }  // (opt-in) the decimator may run inside the transform's kernel
    }
    zoom_bins = cfg->hires_bins;
    if (zoom_bins) {  // m_fftHiRes->fftParams(m_numHiResSpectrumBins, maxDb, m_hiResSampleRate, numSamples, BLACKMANHARRIS), signalspectrum.cpp:59
        if (nd_max % nf != 0) return fail(PEBBLEGPU_E_UNSUPPORTED, "the zoomed spectrum needs whole frames at the demodulator rate");
        if (int rc = zoom_.init(C, nf, zoom_bins, tun_)) return rc;
        zoom_bins = zoom_.bins;
        PG_TRY(d_zoom.alloc((size_t)(nd_max / nf) * zoom_bins * C));
    }
    return 0;
}

Receiver::~Receiver()
{
    (void)hipSetDevice(device);
    if (chain_stream_) (void)hipStreamSynchronize(chain_stream_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    // (what is released here holds events or host blocks; device memory goes with the members, behind this body: the streams have been waited for)
    osc_.release();
    dec_.release();
    for (hipEvent_t e : sync_ev_) if (e) (void)hipEventDestroy(e);
    ingest_.release();
    ext_ingest_.release();
    aout_.release();
    rec_.release();
    mout_.release();
    display_destroy();  // (closes an open display ring: waits for a reader that is inside _next)
    if (map_ev_) (void)hipEventDestroy(map_ev_);
    resamp_.release();
    morse_.release();
    tb_.release();
    for (auto &row : tm.ev)
        for (auto &e : row) if (e) (void)hipEventDestroy(e);
    if (chain_stream_) (void)hipStreamDestroy(chain_stream_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

int Receiver::set_mixer(uint32_t ch, double f)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    std::lock_guard<std::mutex> g(mu_);
    touched_ = true;  // the next call joins its two pipelines before the change is applied
    osc_.retune(ch, f);
    sm_dirty_ = true;
    return 0;
}

int Receiver::set_mode(uint32_t ch, int mode)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (wfm) {
        if (mode != PEBBLEGPU_DM_FMM && mode != PEBBLEGPU_DM_FMS) return fail(PEBBLEGPU_E_UNSUPPORTED, "a WFM bank demodulates FMM and FMS only");
        std::lock_guard<std::mutex> g(mu_);
        // refused (E_SIZE: the handle's frame against the RDS down-converter, RdsCore::check_frame): the channel stays as it was, nothing is
        // marked touched and the handle goes on
        if (int rc = wfmc_.set_stereo(ch, mode == PEBBLEGPU_DM_FMS)) return rc;
        touched_ = true;  // the next call joins its two pipelines before the change is applied
        ctl_[ch].mode = mode;
        return 0;
    } else if (mode == PEBBLEGPU_DM_FMM || mode == PEBBLEGPU_DM_FMS || mode < 0 || mode > PEBBLEGPU_DM_NONE) {
        return fail(PEBBLEGPU_E_UNSUPPORTED, "demod mode %d is not available in a narrow bank (FMM and FMS need a wfm bank)", mode);
    }
    std::lock_guard<std::mutex> g(mu_);
    touched_ = true;  // the next call joins its two pipelines before the change is applied
    if (ctl_[ch].mode != mode) am_list_dirty_ = true;
    if (ctl_[ch].mode != mode) mout_tab_dirty_ = true;  // (the modem ring's table says which rows are in dmNONE)
    ctl_[ch].mode = mode;
    if (!wfm) {  // "Tune only mode": the reference returns before NoiseFilter and AGC (receiver.cpp:968-971): their states stay frozen
        agc_.set_muted(ch, mode == PEBBLEGPU_DM_NONE);
        anf_.set_muted(ch, mode == PEBBLEGPU_DM_NONE);
    }
    // m_iDigitalModem->setDemodMode(_demodMode), receiver.cpp:653-654 (the dmNONE return, :968-971, leaves the channel's modem alone)
    if (morse_.C) {
        PG_HIP(hipSetDevice(device));
        if (int rc = morse_.set_mode(ch, mode)) return rc;
    }
    return 0;
}

int Receiver::set_morse(uint32_t ch, bool on)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (wfm) return fail(PEBBLEGPU_E_UNSUPPORTED, "the digital-modem hook is on the narrow branch (receiver.cpp:977-980): a WFM receiver has none");
    std::lock_guard<std::mutex> g(mu_);
    if (on && bank_gate_)
        return fail(PEBBLEGPU_E_UNSUPPORTED, "the per-channel squelch of a bank and the Morse modem do not run together (DESIGN.md section 7)");
    PG_HIP(hipSetDevice(device));
    if (!morse_.C) {
        if (!on) return 0;
        const long long per_sf = (long long)(superframe / chain.total);
        int rc = morse_.init(C, demod_rate_int, (long long)max_sf * per_sf, false);
        if (!rc) rc = morse_.check(per_sf);  // every call is a whole number of super-frames: one passing is all passing
        if (rc) { morse_.release(); return rc; }
    }
    touched_ = true;
    return morse_.enable(ch, on, ctl_[ch].mode);  // Receiver::setDigitalModem -> Morse::setSampleRate(m_demodSampleRate, m_demodFrames)
}

// (the getters take the receiver's lock like the setters: a host may read them from another thread than the one that calls process,
// whose calls drain the same logs when they could wrap)
int Receiver::morse_events(uint32_t ch, MorseEvent *ev, uint32_t cap, uint32_t *n)
{
    if (n) *n = 0;
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    std::lock_guard<std::mutex> g(mu_);
    if (!morse_.C) return 0;
    PG_HIP(hipSetDevice(device));
    return morse_.events(ch, ev, cap, n);
}

int Receiver::morse_status(uint32_t ch, MorseStatus *st)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    std::lock_guard<std::mutex> g(mu_);
    if (!morse_.C) return fail(PEBBLEGPU_E_INVALID, "the Morse modem of channel %u is off", ch);
    PG_HIP(hipSetDevice(device));
    return morse_.status(ch, st);
}

void UpdateTimer::advance(int ups, uint64_t period_ms, uint64_t n, uint64_t frame_len, uint64_t rate, std::vector<uint32_t> *sel)
{
    const uint64_t first = next, end = next + n;
    next = end;
    if (n == 0) return;
    if (ups < 0) {  // no gate: every frame is transformed and restarts the timer
        started = true;
        f_last = end - 1;
        return;
    }
    uint64_t f = first;
    if (!started) {  // "First time": the frame starts the timer and gets no spectrum (signalspectrum.cpp:65-68)
        started = true;
        f_last = f++;
    }
    if (ups == 0) return;  // m_updatesPerSec == 0: the timer runs on, nothing is made
    // floor(d * frame_len * 1000 / rate) >= period_ms  <=>  d >= ceil(period_ms * rate / (frame_len * 1000)); a frame never pairs with itself
    const uint64_t per = frame_len * 1000u;
    uint64_t d_min = (period_ms * rate + per - 1) / per;
    if (d_min < 1) d_min = 1;
    for (f = std::max(f, f_last + d_min); f < end; f = f_last + d_min) {
        sel->push_back((uint32_t)(f - first));
        f_last = f;
    }
}

int Receiver::set_spectrum_updates(int ups)
{
    if (ups < -1) return fail(PEBBLEGPU_E_INVALID, "updates per second: -1 (every frame), 0 (none) or a rate");
    std::lock_guard<std::mutex> g(mu_);
    PG_HIP(hipSetDevice(device));
    if (ups != -1) {
        if (bins) { if (int rc = spec_.init_list()) return rc; }
        if (zoom_bins) { if (int rc = zoom_.init_list()) return rc; }
        if (bins && !d_spec_carry) {
            PG_TRY(d_spec_carry.alloc((size_t)bins * S));
            PG_TRY(d_sm_carry.alloc(C));
        }
        if (spec_ups_ == -1 && bins && last_spec_frames) {
            // so far every frame had a spectrum: the one the S-meter and the squelch go on reading is the last call's last
            if (int rc = sync()) return rc;
            PG_HIP(hipMemcpy2D(d_spec_carry, sizeof(float) * bins, d_spec + (last_spec_frames - 1) * bins, sizeof(float) * last_spec_frames * bins,
                               sizeof(float) * bins, S, hipMemcpyDeviceToDevice));
            have_carry_ = true;
        }
    }
    if (ups > 0) spec_period_ms_ = (uint64_t)(1000 / ups);  // integer division, as the reference computes it
    spec_ups_ = ups;
    touched_ = true;  // the next call joins its two pipelines first
    return 0;
}
int Receiver::spectrum_frames(bool zoomed, uint32_t *idx, uint32_t cap, uint32_t *n) const
{
    if (!n) return fail(PEBBLEGPU_E_INVALID, "null argument");
    *n = 0;
    if (zoomed ? !zoom_bins : !bins) return fail(PEBBLEGPU_E_INVALID, zoomed ? "the receiver computes no zoomed spectrum (hires_bins = 0)" : "the receiver computes no spectrum (spectrum_bins = 0)");
    const uint64_t rows = zoomed ? last_zoom_frames : last_spec_frames;
    const std::vector<uint32_t> &sel = zoomed ? sel_zoom_ : sel_spec_;
    if (rows > cap) return fail(PEBBLEGPU_E_SIZE, "%llu frames do not fit %u entries", (unsigned long long)rows, cap);
    if (rows && !idx) return fail(PEBBLEGPU_E_INVALID, "null argument");
    // (without the gate every frame of the call has its row)
    for (uint64_t i = 0; i < rows; i++) idx[i] = gated() && sel.size() == rows ? sel[i] : (uint32_t)i;
    *n = (uint32_t)rows;
    return 0;
}

int Receiver::enable_smeter(bool on)
{
    std::lock_guard<std::mutex> g(mu_);
    if (on && !bins) return fail(PEBBLEGPU_E_INVALID, "signal strength is measured on the spectrum: create the bank with spectrum_bins");
    PG_HIP(hipSetDevice(device));
    if (on && !d_smeter) {
        smeter_pitch = (long long)max_sf * (long long)(superframe / nf);
        PG_TRY(d_smeter.alloc((size_t)smeter_pitch * C));
        PG_TRY(d_sm_bins.alloc(C));
        sm_dirty_ = true;
    }
    smeter_on = on;
    return 0;
}

int Receiver::rds_groups(uint32_t ch, RdsGroup *g, unsigned char *changed, uint32_t cap, uint32_t *n)
{
    if (n) *n = 0;
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (!wfm) return fail(PEBBLEGPU_E_UNSUPPORTED, "RDS groups come from the dmFMS channels of a WFM bank");
    if (int rc = sync()) return rc;
    return wfmc_.rds.groups(nullptr, ch, g, changed, cap, n);
}
int Receiver::stereo_lock(uint32_t ch, int *lock, int *changed)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (!wfm) return fail(PEBBLEGPU_E_UNSUPPORTED, "the stereo lock belongs to the dmFMS channels of a WFM bank");
    if (int rc = sync()) return rc;
    return wfmc_.stereo_lock(nullptr, ch, lock, changed);
}
int Receiver::set_squelch(uint32_t ch, double squelch_db)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u of %u", ch, C);
    if (squelch_db > -120.0) {
        std::lock_guard<std::mutex> g(mu_);
        if (taps_ & kTapsBehindGate)
            return fail(PEBBLEGPU_E_UNSUPPORTED, "a squelch gate ends the call before the modem hook and the demodulator: their taps are on (pebblegpu_receiver_set_taps)");
    }
    if (C != 1 || max_sf != 1) {
        // a bank, or calls of several super-frames: per-channel thresholds, the decision per (channel, super-frame) on the device
        if (wfm) {
            if (squelch_db <= -120.0) return 0;  // "never closes": nothing to set up
            return fail(PEBBLEGPU_E_UNSUPPORTED, "the per-channel gate of a bank is built for the narrow branch (a WFM receiver gates as one channel, one super-frame per call)");
        }
        const char *both = "the per-channel squelch of a bank and the Morse modem do not run together (DESIGN.md section 7)";
        {
            std::lock_guard<std::mutex> g(mu_);
            if (squelch_db > -120.0 && morse_.any()) return fail(PEBBLEGPU_E_UNSUPPORTED, "%s", both);
        }
        if (squelch_db > -120.0) {
            if (int rc = enable_smeter(true)) return rc;
        }
        std::lock_guard<std::mutex> g(mu_);
        if (squelch_db > -120.0 && morse_.any()) return fail(PEBBLEGPU_E_UNSUPPORTED, "%s", both);  // (a set_morse between the two locks)
        touched_ = true;  // the next call joins its two pipelines before the change is applied
        PG_HIP(hipSetDevice(device));
        if (squelch_.empty()) squelch_.assign(C, -120.f);
        if (!d_squelch) {
            PG_TRY(d_squelch.alloc(C));
            PG_TRY(d_gate.alloc((size_t)C * max_sf));
        }
        squelch_[ch] = (float)squelch_db;
        bank_gate_ = false;
        for (float v : squelch_) bank_gate_ = bank_gate_ || v > -120.f;
        squelch_dirty_ = true;
        return 0;
    }
    if (squelch_db > -120.0) {
        if (int rc = enable_smeter(true)) return rc;
    }
    std::lock_guard<std::mutex> g(mu_);
    touched_ = true;  // the next call joins its two pipelines before the change is applied
    if (squelch_db > -120.0 && !h_gate_) {
        PG_HIP(hipSetDevice(device));
        PG_TRY(h_gate_.alloc(1));
    }
    squelch_db_ = squelch_db;
    return 0;
}

// TestBench::reset() + the generator switches (testbench.cpp:550-566): the next call starts the sweep and the noise counter afresh
int Receiver::set_testbench_sweep(const pebblegpu_sweep *s)
{
    std::lock_guard<std::mutex> g(mu_);
    if (int rc = tb_.set_sweep(s)) return rc;
    touched_ = true;  // the next call joins its two pipelines before the change is applied
    return 0;
}

int Receiver::set_testbench_noise(double amplitude, uint64_t seed)
{
    std::lock_guard<std::mutex> g(mu_);
    if (int rc = tb_.set_noise(amplitude, seed)) return rc;
    touched_ = true;
    return 0;
}

// MorseGen stations (plugins/MorseGenDevice): replaces the set and restarts the stations; the sweep and the noise counter stay where they are
int Receiver::set_testbench_morse(const pebblegpu_morse_station *stations, uint32_t n_stations, int mix)
{
    std::lock_guard<std::mutex> g(mu_);
    if (int rc = tb_.set_morse(stations, n_stations, mix)) return rc;
    touched_ = true;
    return 0;
}

int Receiver::set_taps(uint32_t mask)
{
    const uint32_t known = 1u << PEBBLEGPU_TAP_RAW_IQ | 1u << PEBBLEGPU_TAP_POST_MIXER | 1u << PEBBLEGPU_TAP_POST_BP | 1u << PEBBLEGPU_TAP_POST_DEMOD | 1u << PEBBLEGPU_TAP_MODEM;
    if (mask & ~known) return fail(PEBBLEGPU_E_INVALID, "tap mask %#x names a point that does not exist", mask);
    if (wfm && (mask & (kTapsBehindGate | 1u << PEBBLEGPU_TAP_POST_BP)))
        return fail(PEBBLEGPU_E_UNSUPPORTED, "the WFM branch has no band-pass, modem hook or post-demodulator display point (receiver.cpp:854-901)");
    std::lock_guard<std::mutex> g(mu_);
    if ((mask & kTapsBehindGate) && (squelch_db_ > -120.0 || bank_gate_))
        return fail(PEBBLEGPU_E_UNSUPPORTED, "a squelch gate ends the call before the modem hook and the demodulator: no tap there while a threshold is set");
    PG_HIP(hipSetDevice(device));
    const size_t max_n = (size_t)max_sf * superframe;
    for (int pt = 0; pt < kTapPoints; pt++) {
        if (!(mask >> pt & 1u)) continue;
        if (!d_tap_[pt]) PG_TRY(d_tap_[pt].alloc(pt == PEBBLEGPU_TAP_RAW_IQ ? (size_t)S * max_n : (size_t)C * (max_n / chain.total)));
        if (!(taps_ >> pt & 1u)) tap_n_[pt] = 0;  // (nothing of this point yet)
    }
    taps_ = mask;
    touched_ = true;  // the next call joins its two pipelines first
    return 0;
}

const float2 *Receiver::tap(int point, uint64_t *n_per_row, uint64_t *pitch, double *rate) const
{
    if (point < 0 || point >= kTapPoints || !(taps_ >> point & 1u) || !tap_n_[point]) return nullptr;
    if (n_per_row) *n_per_row = tap_n_[point];
    if (pitch) *pitch = tap_n_[point];  // rows are compact
    if (rate) *rate = point == PEBBLEGPU_TAP_RAW_IQ ? fs : (double)demod_rate_int;
    return d_tap_[point];
}

// rows of n samples at src (pitched) -> the point's buffer, compact, behind whatever `s` has queued
int Receiver::copy_tap(hipStream_t s, int point, const float2 *src, long long src_pitch, long long n, uint32_t rows)
{
    if (!(taps_ >> point & 1u)) return 0;
    PG_HIP(hipMemcpy2DAsync(d_tap_[point], sizeof(float2) * (size_t)n, src, sizeof(float2) * (size_t)src_pitch, sizeof(float2) * (size_t)n, rows, hipMemcpyDeviceToDevice, s));
    tap_n_[point] = (uint64_t)n;
    return 0;
}

const float2 *Receiver::conditioned(uint64_t *n_per_stream, uint64_t *pitch) const
{
    if (n_per_stream) *n_per_stream = last_cond_n_;
    if (pitch) *pitch = last_cond_n_ ? (uint64_t)cond_.cap : 0;
    return last_cond_n_ ? (const float2 *)cond_.d_buf : nullptr;
}

int Receiver::set_conditioners(uint32_t stream, int flags, double iq_gain, double iq_phase)
{
    std::lock_guard<std::mutex> g(mu_);
    touched_ = true;  // the next call joins its two pipelines before the change is applied
    PG_HIP(hipSetDevice(device));
    return cond_.set(stream, flags, iq_gain, iq_phase);
}

int Receiver::set_noise_filter(uint32_t ch, bool on)
{
    if (wfm) return fail(PEBBLEGPU_E_UNSUPPORTED, "the WFM branch has no noise filter step (receiver.cpp:854-901)");
    std::lock_guard<std::mutex> g(mu_);
    touched_ = true;  // the next call joins its two pipelines before the change is applied
    PG_HIP(hipSetDevice(device));
    return anf_.set(ch, on);
}

int Receiver::set_agc(uint32_t ch, int mode, int threshold)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (wfm) return fail(PEBBLEGPU_E_UNSUPPORTED, "the WFM branch has no AGC (receiver.cpp:854-901)");
    std::lock_guard<std::mutex> g(mu_);
    touched_ = true;  // the next call joins its two pipelines before the change is applied
    return agc_.set_mode(ch, mode, threshold);
}

int Receiver::set_bandpass(uint32_t ch, double lo, double hi)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (wfm) return fail(PEBBLEGPU_E_UNSUPPORTED, "the WFM branch has no band-pass (receiver.cpp:854-901)");
    std::lock_guard<std::mutex> g(mu_);
    touched_ = true;  // the next call joins its two pipelines before the change is applied
    ChanCtl &c = ctl_[ch];
    const double flo = (double)(float)lo, fhi = (double)(float)hi;  // setBandPass(float, float), bandpassfilter.cpp:38
    if (c.mode == PEBBLEGPU_DM_AM) {  // Demod::setBandwidth only acts in AM (demod.cpp:230-239)
        c.am_bw = hi - lo;
        c.am_dirty = true;
    }
    if (c.bp_valid && flo == c.lo && fhi == c.hi) return 0;  // "return if no changes", fastfir.cpp:195-199
    c.lo = flo;  // stored before the sanity check, fastfir.cpp:200-203
    c.hi = fhi;
    sm_dirty_ = true;
    c.bp_valid = true;
    const double rate = (double)demod_rate_int;
    if (flo >= fhi || flo >= rate / 2.0 || flo <= -rate / 2.0 || fhi >= rate / 2.0 || fhi <= -rate / 2.0)
        return fail(PEBBLEGPU_E_FILTER_PARAM, "Filter Parameter error: lo %.1f hi %.1f rate %.1f", flo, fhi, rate);
    c.bp_dirty = true;
    return 0;
}

int Receiver::apply_controls(hipStream_t osc_stream)
{
    if (int rc = osc_.upload(osc_stream)) return rc;
    if (smeter_on && sm_dirty_) {
        // bin indices of fdEstimate (strength_windows, params.h)
        std::vector<SmBins> hb(C);
        for (uint32_t ch = 0; ch < C; ch++) {
            const float lo = wfm ? -100000.f : (float)ctl_[ch].lo, hi = wfm ? 100000.f : (float)ctl_[ch].hi;  // receiver.cpp:891-892,959-960
            hb[ch] = strength_windows((uint32_t)bins, (uint32_t)fs, lo, hi, osc_.ctl[ch].freq, shared_input ? 0 : (int)ch);
        }
        PG_HIP(hipMemcpyAsync(d_sm_bins, hb.data(), sizeof(SmBins) * C, hipMemcpyHostToDevice, stream_));
        PG_HIP(hipStreamSynchronize(stream_));
        sm_dirty_ = false;
    }
    if (squelch_dirty_) {
        PG_HIP(hipMemcpyAsync(d_squelch, squelch_.data(), sizeof(float) * C, hipMemcpyHostToDevice, stream_));
        PG_HIP(hipStreamSynchronize(stream_));
        squelch_dirty_ = false;
    }
    if (wfm) return 0;
    for (uint32_t ch = 0; ch < C; ch++) {
        ChanCtl &c = ctl_[ch];
        if (c.bp_dirty) {
            bool ok = false;
            if (int rc = ff_.design(stream_, ch, c.lo, c.hi, 0.0, (double)demod_rate_int, &ok)) return rc;
            c.bp_dirty = false;
        }
        if (c.am_dirty && c.mode == PEBBLEGPU_DM_AM) {
            if (int rc = am_.set_bandwidth(stream_, ch, c.am_bw)) return rc;
            c.am_dirty = false;
        }
    }
    if (int rc = agc_.apply(stream_)) return rc;
    if (int rc = anf_.apply(stream_)) return rc;
    if (am_list_dirty_) {
        std::vector<int> l, ls, ln;
        for (uint32_t ch = 0; ch < C; ch++) {
            if (ctl_[ch].mode == PEBBLEGPU_DM_AM) l.push_back((int)ch);
            else if (ctl_[ch].mode == PEBBLEGPU_DM_SAM) ls.push_back((int)ch);
            else if (ctl_[ch].mode == PEBBLEGPU_DM_FMN) ln.push_back((int)ch);
        }
        if (int rc = am_.set_list(stream_, l)) return rc;
        if (!ls.empty() && sam_.C == 0) { if (int rc = sam_.init(C, (double)demod_rate_int, pll_cap_, 1)) return rc; }
        if (!ln.empty() && nfm_.C == 0) { if (int rc = nfm_.init(C, (double)demod_rate_int, pll_cap_, 0)) return rc; }
        if (sam_.C) { if (int rc = sam_.set_list(stream_, ls)) return rc; }
        if (nfm_.C) { if (int rc = nfm_.set_list(stream_, ln)) return rc; }
        am_list_dirty_ = false;
    }
    return 0;
}

// ---- one process call: its refusals, its route (call_route.h), then its stages in queue order ----

// caller mistakes that leave the handle usable: refused before anything is queued
int Receiver::refuse_call(const float2 *d_iq, uint64_t n, bool with_spectrum, bool with_chain, const RawSrc *raw) const
{
    if (failed_) return fail(PEBBLEGPU_E_HIP, "an earlier call on this receiver failed half-way (its filter histories no longer match its oscillators): destroy it");
    if ((!d_iq && !raw) || n == 0) return fail(PEBBLEGPU_E_INVALID, "null input or zero samples");
    if (with_chain && (n % superframe != 0 || n / superframe > max_sf))
        return fail(PEBBLEGPU_E_SIZE, "n_samples %llu is not 1..%u super-frames of %llu", (unsigned long long)n, max_sf,
                    (unsigned long long)superframe);
    if (with_spectrum && (!bins || n % nf != 0 || n > (uint64_t)max_sf * superframe))
        return fail(PEBBLEGPU_E_SIZE, "spectrum needs whole frames of %u samples within capacity", nf);
    // caller mistakes around the squelch gate are refused HERE, before anything is queued: they leave the handle usable (a failure
    // behind this point has kernels in flight and histories half advanced, and closes the handle)
    if (with_chain && squelch_db_ > -120.0 && !with_spectrum && !last_spec_frames && !gated())  // (under the update timer the gate stays open until the first spectrum)
        return fail(PEBBLEGPU_E_INVALID, "the squelch gate needs a spectrum: none has been computed yet");
    if (with_chain && !wfm && bank_gate_ && !with_spectrum && !(squelch_db_ > -120.0) && !(C == 1 && ctl_[0].mode == PEBBLEGPU_DM_NONE))
        return fail(PEBBLEGPU_E_INVALID, "the squelch gate of a bank reads the spectra of the same call: create the bank with spectrum_bins");
    return 0;
}

// what plan_call_route() reads, as the handle stands before anything of the call is queued
CallFacts Receiver::call_facts(uint64_t n, bool with_spectrum, bool with_chain, bool raw) const
{
    CallFacts f;
    f.with_spectrum = with_spectrum;
    f.with_chain = with_chain;
    f.raw = raw;
    f.n = n;
    f.C = C;
    f.S = S;
    f.nf = nf;
    f.zoom_bins = zoom_bins;
    f.wfm = wfm;
    f.bank_pipe_ok = bank_pipe_ok_;
    f.profiling = profile_detail;
    f.squelch_set = squelch_db_ > -120.0;
    f.bank_gate = bank_gate_;
    f.gated = gated();
    f.touched = touched_;
    f.cond_any = cond_.any;
    f.cond_dirty = cond_.dirty;
    f.generator = tb_.any();
    f.taps = taps_ != 0;
    f.recording = rec_.open;
    f.ch0_tune_only = ctl_[0].mode == PEBBLEGPU_DM_NONE;
    f.scale_pending = display_scale_pending();
    f.dec_lds_free_front = dec_.front_is_lds_free();
    f.dec_raw_front = dec_.raw_front();
    f.dec_double_out = dec_.double_out();
    f.dec_triple_out = dec_.fin3.base != nullptr;
    f.dec_long_call = dec_.long_call((long long)n);
    f.dec_fuse_shape = dec_.fuse_shape();
    f.osc_transient = osc_.any_transient();
    f.spec_raw_ready = spec_.raw_ready();
    f.spec_dec_ready = spec_.dec_ready();
    f.pipeline = tun_.pipeline;
    f.fuse_dec = tun_.fuse_dec;
    f.bank_pipe_extev = tun_.bank_pipe_extev;
    f.bank_pipe_timed_ev = tun_.bank_pipe_timed_ev;
    f.dec_mix_in_consumer = dec_.mix_in_consumer_ready();
    f.tap_post_mixer = (taps_ >> PEBBLEGPU_TAP_POST_MIXER & 1u) != 0;
    return f;
}

int Receiver::join_streams()
{
    if (chain_end_) PG_HIP(hipStreamWaitEvent(stream_, chain_end_, 0));
    if (spec_end_) PG_HIP(hipStreamWaitEvent(chain_stream_, spec_end_, 0));
    chain_end_ = spec_end_ = nullptr;
    return 0;
}

// the staging buffer of raw and generated calls (allocated on first use)
int Receiver::raw_stage(float2 **p)
{
    if (!d_raw_stage_) PG_TRY(d_raw_stage_.alloc((size_t)S * max_sf * superframe));
    *p = d_raw_stage_;
    return 0;
}

// this call's stage 1 -> stage 2 hand-over event (no timing; the ring is created on first use)
int Receiver::handover_event(hipEvent_t *e)
{
    if (!sync_ev_[0]) for (hipEvent_t &ne : sync_ev_) PG_HIP(hipEventCreateWithFlags(&ne, hipEventDisableTiming));
    *e = sync_ev_[tm.calls % 4];
    return 0;
}

// the one-value squelch gate: the host reads one S-meter value back behind whatever `cs` has queued
int Receiver::read_gate(hipStream_t cs, const float4 *src, bool *closed)
{
    PG_HIP(hipMemcpyAsync(h_gate_, src, sizeof(float4), hipMemcpyDeviceToHost, cs));
    PG_HIP(hipStreamSynchronize(cs));
    *closed = (double)h_gate_->y < squelch_db_;  // m_avgDb < m_squelchDb
    return 0;
}

// clearCPX(m_audioBuf, ...) of a bank's tune-only channels: rows of n samples, `pitch` apart
int Receiver::clear_tune_only_rows(hipStream_t cs, float2 *row0, long long pitch, long long n)
{
    for (uint32_t ch = 0; ch < C; ch++)
        if (ctl_[ch].mode == PEBBLEGPU_DM_NONE) PG_HIP(hipMemsetAsync(row0 + (long long)ch * pitch, 0, sizeof(float2) * (size_t)n, cs));
    return 0;
}

// the carried row's S-meter with the channels' current bands (before this call's rows replace the row)
int Receiver::measure_carry(hipStream_t st)
{
    if (!(gated() && smeter_on && have_carry_)) return 0;
    return run_signal_strength(st, d_spec_carry, (long long)bins, (int)bins, 1, d_sm_bins, d_sm_carry, 1, C);
}

// join (unless the call is pipelined with its neighbours), apply the controls, upload the tables
int Receiver::join_and_apply(Call &c)
{
    for (uint64_t &tn : tap_n_) tn = 0;  // a tap holds the last call's signal: a point this call does not reach reads as "nothing" (NULL), never as an older call's
    if (!c.rt.plain) { if (int rc = join_streams()) return rc; }
    if (int rc = apply_controls(c.rt.plain ? chain_stream_ : stream_)) return rc;
    touched_ = false;
    if (int rc = cond_.apply(stream_)) return rc;
    if (aout_.open && aout_tab_dirty_) { if (int rc = upload_audio_table()) return rc; }
    if (mout_.open && mout_tab_dirty_) { if (int rc = upload_modem_table()) return rc; }
    if (disp_open_) { if (int rc = upload_display_tables()) return rc; }  // (only after open or set_pane)
    return 0;
}

// the input as the call's kernels read it: raw conversion, generator, conditioners
int Receiver::stage_input(Call &c)
{
    if (c.raw && !c.rt.raw_fused) {
        if (c.rt.plain && !c.rt.bank_pipe) { if (int rc = join_streams()) return rc; }  // the staging buffer is shared by successive calls (two-stage calls: only their first stage touches it)
        float2 *stage = nullptr;
        if (int rc = raw_stage(&stage)) return rc;
        // streams are stream-major in both layouts, so one pass over S * n pairs converts them all
        if (int rc = run_normalize_iq(c.raw->fmt, c.raw->order, 1.0, c.raw->base, (long long)(S * c.n), stage, stream_, false, &c.raw->scale)) return rc;
        c.d_iq = stage;
        c.raw = nullptr;
    }
    c.in_pitch = (long long)c.n;
    // TestBench::genSweep + genNoise, receiver.cpp:797-798: into the library's staging buffer (a raw call has been converted into it above:
    // generated in place; float2 input is read from the caller's buffer, which is never written)
    last_tb_ = tb_.any();
    last_tb_morse_ = tb_.morse_on();
    if (last_tb_) {
        float2 *stage = nullptr;
        if (int rc = raw_stage(&stage)) return rc;
        if (int rc = tb_.run(stream_, c.d_iq, c.in_pitch, stage, c.in_pitch, (long long)c.n, S, 0)) return rc;
        c.d_iq = stage;
    }
    c.tap_iq = c.d_iq;  // displayData(.., TB_RAW_IQ), receiver.cpp:803: before the conditioners
    // DCRemoval, IQBalance, NoiseBlanker 1/2 on the raw streams, ahead of the spectrum and the mixer (receiver.cpp:814-823)
    if (int rc = cond_.run(stream_, c.d_iq, c.in_pitch, (long long)c.n, &c.d_iq, &c.in_pitch)) return rc;
    if (cond_.any) last_cond_n_ = c.n;  // what pebblegpu_receiver_conditioned hands out
    return 0;
}

// the call's timing slot, its start record, the fork, and the wait for the last reader of the output buffer it writes
int Receiver::start_call(Call &c)
{
    c.ev = tm.slot();
    c.slot = (int)(tm.calls % Timers::kRing);
    tm.calls++;
    // Every event record is a packet of its own in the queue (~6 us of idle GPU between two kernels).  A side-by-side call therefore
    // records no end event: it ends where the next call's start event is recorded (same queue, nothing in between), or where
    // sync() / a timing query closes it (close_timing).
    hipEvent_t start = c.ev[0];
    if (c.rt.bank_pipe && c.rt.plain && d_end_prev_) start = d_end_prev_;  // (back to back, a two-stage call is timed from where the previous one ended: one queue packet less)
    else PG_HIP(hipEventRecord(c.ev[0], stream_));
    tm.start_ev[c.slot] = start;
    if (tm.open_slot >= 0) {
        tm.end_ev[tm.open_slot] = start;
        tm.open_slot = -1;
    }
    tm.end_ev[c.slot] = c.ev[6];
    c.cs = c.rt.side ? chain_stream_ : stream_;
    if (c.rt.side) {
        PG_HIP(hipStreamWaitEvent(chain_stream_, start, 0));  // fork: the input is ready where the call starts
    }
    // the output buffer this call writes was read three (two) calls ago (a wait is a queue packet: none when the host can see that it is over)
    hipEvent_t last_reader = nullptr;  // where the second stage that last read the buffer this call writes (dec_.fin2) ended
    for (const auto &pr : out_reader_) if (pr.first == (const void *)dec_.fin2.base) last_reader = pr.second;
    if (c.rt.bank_pipe && last_reader && hipEventQuery(last_reader) != hipSuccess) {
        // the host is more than two calls ahead of the device: it waits here (PEBBLEGPU_BANK_PIPE_HOSTWAIT=0: a wait in the queue instead,
        // one more packet between this decimator and the last)
        if (tun_.bank_pipe_hostwait) PG_HIP(hipEventSynchronize(last_reader));
        else PG_HIP(hipStreamWaitEvent(stream_, last_reader, 0));
    }
    return 0;
}

// the display transform, its S-meter and the carried row
int Receiver::run_display_transform(Call &c)
{
    if (c.rt.fuse_dec) { if (int rc = dec_.fill_dec_fuse(stream_, &c.df, osc_, (long long)c.n)) return rc; }
    c.carry_before = have_carry_;  // a computed spectrum from before this call exists (what its first super-frames' squelch reads)
    const uint64_t n = c.n;
    if (c.with_spectrum && gated()) {
        // SignalSpectrum::unprocessed behind its update timer (signalspectrum.cpp:63-86): the host has the frame list before anything is
        // queued; the transform runs over that list alone, rows compact, |X_prev| from listed frame to listed frame
        sel_spec_.clear();
        ut_spec_.advance(spec_ups_, spec_period_ms_, n / nf, nf, (uint64_t)fs, &sel_spec_);
        const long long ns = (long long)sel_spec_.size();
        if (int rc = measure_carry(stream_)) return rc;
        if (int rc = spec_.run_list(stream_, c.d_iq, c.in_pitch, sel_spec_.data(), ns, d_spec, c.raw)) return rc;
        last_spec_frames = (uint64_t)ns;
        if (ns) {
            if (smeter_on) { if (int rc = run_signal_strength(stream_, d_spec, ns * (long long)bins, (int)bins, ns, d_sm_bins, d_smeter, smeter_pitch, C)) return rc; }
            PG_HIP(hipMemcpy2DAsync(d_spec_carry, sizeof(float) * bins, d_spec + (ns - 1) * (long long)bins, sizeof(float) * (size_t)ns * bins, sizeof(float) * bins, S,
                                    hipMemcpyDeviceToDevice, stream_));
            have_carry_ = true;
        }
    } else if (c.with_spectrum) {  // SignalSpectrum::unprocessed on the raw frame, receiver.cpp:826
        ut_spec_.advance(-1, 0, n / nf, nf, (uint64_t)fs, nullptr);  // (every frame restarts the timer a later set_spectrum_updates goes on from)
        // (a call whose chain follows on the same stream, or that has none, leaves the GPU to the transform: its all-registers variant)
        if (int rc = spec_.run(stream_, c.d_iq, c.in_pitch, (long long)(n / nf), d_spec, c.raw, c.rt.fuse_dec ? &c.df : nullptr, !c.rt.side)) return rc;
        last_spec_frames = n / nf;
        if (smeter_on) {
            const long long F = (long long)(n / nf);
            if (int rc = run_signal_strength(stream_, d_spec, F * (long long)bins, (int)bins, F, d_sm_bins, d_smeter, smeter_pitch, C)) return rc;
        }
    }
    if (c.with_spectrum) c.disp_spec_rows = last_spec_frames;
    return 0;
}

// the raw-IQ tap, the record block and the record behind the display transform
int Receiver::tap_and_record_input(Call &c)
{
    const uint64_t n = c.n;
    if (taps_ >> PEBBLEGPU_TAP_RAW_IQ & 1u) {  // (behind the display transform on its stream: the chain's start does not wait for the copy)
        if (c.raw) { if (int rc = run_normalize_iq(c.raw->fmt, c.raw->order, 1.0, c.raw->base, (long long)(S * n), d_tap_[PEBBLEGPU_TAP_RAW_IQ], stream_, false, &c.raw->scale)) return rc; }
        else PG_HIP(hipMemcpyAsync(d_tap_[PEBBLEGPU_TAP_RAW_IQ], c.tap_iq, sizeof(float2) * (size_t)S * n, hipMemcpyDeviceToDevice, stream_));
        tap_n_[PEBBLEGPU_TAP_RAW_IQ] = n;
    }
    // WavFile::WriteSamples(nextStep, numSamples), receiver.cpp:800-801: the same samples, at the same place in the queue
    if (rec_.open && c.with_chain) { if (int rc = queue_record_block(stream_, c.tap_iq, c.rec_from_raw ? &c.rec_raw : nullptr, n)) return rc; }
    if (c.rt.mid) PG_HIP(hipEventRecord(c.ev[1], stream_));
    tm.detailed[(tm.calls - 1) % Timers::kRing] = profile_detail;
    tm.has_mid[(tm.calls - 1) % Timers::kRing] = c.rt.mid;
    return 0;
}

// the end of a call that has no chain
int Receiver::end_without_chain(Call &c)
{
    if (profile_detail) for (int i = 2; i <= 5; i++) PG_HIP(hipEventRecord(c.ev[i], stream_));
    PG_HIP(hipEventRecord(c.ev[6], stream_));
    return 0;
}

// Mixer::processBlock + Decimator::process, receiver.cpp:867-868 / :910-911, and for two-stage calls the hand-over to the chain's stream
int Receiver::run_decimator(Call &c)
{
    const CallRoute &rt = c.rt;
    const uint64_t n = c.n;
    // an event record costs the stream a ~5 us bubble: per-kernel events only when asked for (set_profiling)
    memset(&c.oa_pre, 0, sizeof(c.oa_pre));
    c.have_oa = false;
    DecimDone done;
    if (rt.fuse_dec) {
        if (int rc = dec_.run_beside_spectrum(c.cs, c.d_iq, c.in_pitch, shared_input, (long long)n, osc_, c.raw)) return rc;
        PG_HIP(hipStreamWaitEvent(c.cs, c.ev[1], 0));  // everything behind the decimator reads what the transform's kernel wrote
    } else {
        // (the oscillators' advance is offered to the decimator: the bank kernel carries it in its own launch, DecimDone::osc_advanced)
        if (!wfm) {
            if (int rc = osc_.advance_job(c.cs, n, &c.oa_pre)) return rc;
            c.have_oa = true;
        }
        DecimCall dc;
        dc.lds_free = rt.side;
        dc.rotate3 = rt.rot3;
        dc.mix_in_consumer = rt.mix_in_bandpass;
        // (PEBBLEGPU_BANK_PIPE_EXTEV=1, opt-in: measured 0.0695 / 0.0753 ms (configs[2] / configs[3] shard) against 0.0663 / 0.0774 without)
        // the hand-over event of a two-stage call: completed by the bank kernel's own dispatch when that ends the first stage
        if (rt.done_in_kernel) { if (int rc = handover_event(&dc.done_event)) return rc; }
        if (int rc = dec_.run(c.cs, c.d_iq, c.in_pitch, shared_input, (long long)n, osc_, profile_detail ? c.ev[2] : nullptr, c.raw, c.have_oa ? &c.oa_pre : nullptr, dc, &done)) return rc;
        if (c.have_oa && done.osc_advanced) memset(&c.oa_pre, 0, sizeof(c.oa_pre));
    }
    if (profile_detail) PG_HIP(hipEventRecord(c.ev[3], c.cs));
    if (rt.bank_pipe) {
        // the decimator's own histories and the oscillators' phases stay on its stream; the rest of the call moves over
        std::vector<TailJob> jobs;
        dec_.tail_jobs_dec(jobs);
        const bool nothing_behind = jobs.empty() && c.oa_pre.osc == nullptr;
        if (int rc = run_save_tails(stream_, jobs, C, &c.oa_pre)) return rc;  // (no launch at all behind the bank kernel: nothing left to do)
        // (an event without timing for the hand-over: PEBBLEGPU_BANK_PIPE_TIMED_EV=1 records the call's timing event instead -- A/B)
        hipEvent_t sync_ev = nullptr;
        if (int rc = handover_event(&sync_ev)) return rc;
        pipe_ev_ = rt.timed_handover ? c.ev[1] : sync_ev;
        if (!(done.done_recorded && nothing_behind && !rt.timed_handover)) PG_HIP(hipEventRecord(pipe_ev_, stream_));
        c.cs = chain_stream_;
        PG_HIP(hipStreamWaitEvent(c.cs, pipe_ev_, 0));
        // (with two output buffers the next call's decimator becomes ready with the same event as this band-pass: a short nap lets its
        // one-wave-per-SIMD workgroups be placed before the band-pass fills the CUs -- placed behind them it ran 112 us instead of 65.
        // With three the next decimator is already running when this point is reached: no nap)
        const int nap = tun_.bank_pipe_nap;
        if (int rc = run_nap(c.cs, nap >= 0 ? (unsigned)nap : (rt.rot3 ? 0u : 800u))) return rc;
    }
    c.nd = dec_.out_len();
    if (rt.mix_in_bandpass) return 0;  // (no mixed rows: the route is taken only while nothing reads them)
    return copy_tap(c.cs, PEBBLEGPU_TAP_POST_MIXER, dec_.out().data(), dec_.out().pitch, c.nd, C);  // receiver.cpp:945 (WFM: m_sampleBuf, :884)
}

// SignalSpectrum::zoomed(m_sampleBuf, numStepSamples), receiver.cpp:884 / :942 (its update timer: open by default)
int Receiver::run_zoomed_transform(Call &c)
{
    if (!zoom_bins) return 0;
    const long long nd = c.nd;
    if (gated()) {  // m_hiResTimer: the same period, counted in decimated frames at the demodulator rate (signalspectrum.cpp:94-100)
        sel_zoom_.clear();
        ut_zoom_.advance(spec_ups_, spec_period_ms_, (uint64_t)(nd / nf), nf, demod_rate_int, &sel_zoom_);
        if (int rc = zoom_.run_list(c.cs, dec_.out().data(), dec_.out().pitch, sel_zoom_.data(), (long long)sel_zoom_.size(), d_zoom)) return rc;
        last_zoom_frames = (uint64_t)sel_zoom_.size();
    } else {
        ut_zoom_.advance(-1, 0, (uint64_t)(nd / nf), nf, demod_rate_int, nullptr);
        if (int rc = zoom_.run(c.cs, dec_.out().data(), dec_.out().pitch, nd / nf, d_zoom)) return rc;
        last_zoom_frames = (uint64_t)(nd / nf);
    }
    zoom_stream_ = c.cs;
    c.disp_zoom_rows = last_zoom_frames;
    return 0;
}

// the band-pass, and whether the call ends behind it (c.gate_closed): the squelch gate's read-back, or tune-only mode
int Receiver::bandpass_and_gate(Call &c)
{
    hipStream_t cs = c.cs;
    if (!wfm) {
        if (c.rt.mix_in_bandpass) {  // Mixer::processBlock inside the band-pass's loads (an empty chain: the stream is at the demodulator rate)
            const DecimCore::MixTail &mt = dec_.mix_tail;
            if (int rc = ff_.run_mixing(cs, c.d_iq, c.in_pitch, shared_input, c.nd, audio.data(), audio.pitch, osc_, mt.tail, mt.tail_pitch, mt.tail_out)) return rc;
        } else if (int rc = ff_.run(cs, dec_.out(), c.nd, audio.data(), audio.pitch)) return rc;  // receiver.cpp:950
        if (profile_detail) PG_HIP(hipEventRecord(c.ev[4], cs));
        if (int rc = copy_tap(cs, PEBBLEGPU_TAP_POST_BP, audio.data(), audio.pitch, c.nd, C)) return rc;  // receiver.cpp:953
    }
    // Squelch, receiver.cpp:893-897 / :962-965: below the threshold the reference returns here -- nothing behind the gate
    // runs or changes state, and no audio leaves the call.
    bool gate_closed = false;
    if (squelch_db_ > -120.0) {
        const float4 *src = nullptr;
        if (!gated()) src = d_smeter + (last_spec_frames - 1);  // (refuse_call: a call without a spectrum of its own follows one that had one)
        // under the update timer the latest computed spectrum: a row of this call, else the carried one (m_unprocessedSpectrum between two
        // updates).  Before the first spectrum the reference compares against an uninitialised buffer (signalspectrum.cpp:13): the gate stays open
        else if (c.with_spectrum && last_spec_frames) src = d_smeter + (last_spec_frames - 1);
        else if (have_carry_) {
            if (!c.with_spectrum) { if (int rc = measure_carry(cs)) return rc; }
            src = d_sm_carry;
        }
        if (src) { if (int rc = read_gate(cs, src, &gate_closed)) return rc; }
    }
    if (gate_closed) squelched_calls++;
    // dmNONE, "Tune only mode, no demod or output" (receiver.cpp:968-971): for the reference's own shape (one channel) the call
    // ends here like a closed gate -- nothing behind the band-pass runs or changes state, no audio leaves; in a bank the
    // tune-only channels sit out the noise filter, AGC and demodulators (muted lists) and their audio rows are cleared
    c.gate_closed = gate_closed || c.rt.tune_only;
    return 0;
}

// a closed gate, or tune-only mode: nothing behind the band-pass runs
int Receiver::tail_closed(Call &c)
{
    last_audio_n = 0;
    if (profile_detail) { if (wfm) PG_HIP(hipEventRecord(c.ev[4], c.cs)); }
    if (mout_.open) { if (int rc = queue_modem_block(c.cs, 0, 0, nullptr)) return rc; }  // the reference returned before the hook: a block of 0 samples
    for (int pt : {PEBBLEGPU_TAP_MODEM, PEBBLEGPU_TAP_POST_DEMOD}) {  // "Tune only mode" returns before both points: their rows read zero
        if (!(taps_ >> pt & 1u)) continue;
        PG_HIP(hipMemsetAsync(d_tap_[pt], 0, sizeof(float2) * (size_t)c.nd * C, c.cs));
        tap_n_[pt] = (uint64_t)c.nd;
    }
    return 0;
}

// Per-channel squelch of a bank: the decision is made on the device from the S-meter of each super-frame's last raw frame
// (no read-back, no stream synchronisation); everything behind the band-pass then runs one super-frame at a time and
// leaves a closed channel alone -- no output, no state change: the reference's early return (receiver.cpp:962-965) per
// channel.  A closed (channel, super-frame) reads as silence in the bank's audio rows.
int Receiver::tail_bank_gated(Call &c)
{
    hipStream_t cs = c.cs;
    const long long nd = c.nd;
    if (!c.with_spectrum) return fail(PEBBLEGPU_E_INVALID, "the squelch gate of a bank reads the spectra of the same call: create the bank with spectrum_bins");
    const int k = (int)(c.n / superframe);
    const long long spf = nd / k;
    if (gated()) {
        // per super-frame the latest computed spectrum at or before its last raw frame: a compact row of this call, the carried row, or none yet
        const uint64_t fps = superframe / nf;
        std::vector<int> rows((size_t)k);
        size_t r = 0;
        for (int j = 0; j < k; j++) {
            while (r < sel_spec_.size() && (uint64_t)sel_spec_[r] <= (uint64_t)(j + 1) * fps - 1) r++;
            rows[(size_t)j] = r ? (int)r - 1 : (c.carry_before ? kGateRowCarried : kGateRowNone);
        }
        if (int rc = run_gate_eval_rows(cs, d_smeter, smeter_pitch, d_sm_carry, rows.data(), k, d_squelch, d_gate, (int)max_sf, C)) return rc;
    } else if (int rc = run_gate_eval(cs, d_smeter, smeter_pitch, (int)(superframe / nf), k, d_squelch, d_gate, (int)max_sf, C)) return rc;
    // The modem ring reads every super-frame's rows between the noise filter and the AGC, which works in place.  With the ring open the
    // noise filter's launches of all k super-frames are queued first (its state depends on nothing the AGC or a demodulator writes, and the
    // segments are disjoint: the same launches on the same data), then ONE packing launch, then the rest per super-frame
    const bool anf_first = mout_.open;
    if (anf_first) {
        for (int j = 0; j < k; j++) { if (int rc = anf_.run(cs, audio.data() + (long long)j * spf, audio.pitch, spf, Gate{d_gate, (int)max_sf, j})) return rc; }
        if (int rc = queue_modem_block(cs, spf, k, d_gate)) return rc;
    }
    for (int j = 0; j < k; j++) {
        const Gate gate{d_gate, (int)max_sf, j};
        float2 *seg = audio.data() + (long long)j * spf;
        if (!anf_first) { if (int rc = anf_.run(cs, seg, audio.pitch, spf, gate)) return rc; }
        if (int rc = agc_.run(cs, seg, audio.pitch, spf, gate)) return rc;
        if (int rc = am_.run(cs, seg, audio.pitch, seg, audio.pitch, spf, gate, false)) return rc;
        if (sam_.C) { if (int rc = sam_.run(cs, seg, audio.pitch, seg, audio.pitch, spf, gate)) return rc; }
        if (nfm_.C) { if (int rc = nfm_.run(cs, seg, audio.pitch, seg, audio.pitch, spf, gate, (int)ff_.block_len(), (int)nf)) return rc; }
    }
    if (int rc = run_gate_zero(cs, audio.data(), audio.pitch, spf, d_gate, (int)max_sf, C, k)) return rc;
    return clear_tune_only_rows(cs, audio.data(), audio.pitch, nd);
}

// noise filter, modem hook, AGC and demodulators of the narrow branch (receiver.cpp:974-992)
int Receiver::tail_narrow(Call &c)
{
    hipStream_t cs = c.cs;
    const long long nd = c.nd;
    if (int rc = anf_.run(cs, audio.data(), audio.pitch, nd)) return rc;  // NoiseFilter::ProcessBlock, receiver.cpp:974
    if (taps_ >> PEBBLEGPU_TAP_MODEM & 1u) {  // the frame m_iDigitalModem->processBlock receives (a dmNONE channel's call has returned before, :968-971)
        if (int rc = copy_tap(cs, PEBBLEGPU_TAP_MODEM, audio.data(), audio.pitch, nd, C)) return rc;
        if (int rc = clear_tune_only_rows(cs, d_tap_[PEBBLEGPU_TAP_MODEM], nd, nd)) return rc;
    }
    if (mout_.open) {  // the same rows, to the host's own modems: one launch per call
        const int k = (int)(c.n / superframe);
        if (int rc = queue_modem_block(cs, nd / k, k, nullptr)) return rc;
    }
    // m_iDigitalModem->processBlock, receiver.cpp:979-980: the Morse modem reads the rows before the AGC overwrites them
    if (morse_.any()) { if (int rc = morse_.run(cs, audio.data(), audio.pitch, nd)) return rc; }
    if (int rc = agc_.run(cs, audio.data(), audio.pitch, nd)) return rc;  // AGC::processBlock, receiver.cpp:983
    // Demod::processBlock, receiver.cpp:987: AM channels are demodulated in place; every other narrow mode returns its input
    // (a two-stage call's tail launch carries the AM demodulator's history refresh: one launch fewer)
    if (int rc = am_.run(cs, audio.data(), audio.pitch, audio.data(), audio.pitch, nd, Gate{nullptr, 0, 0}, c.rt.bank_pipe)) return rc;
    if (sam_.C) { if (int rc = sam_.run(cs, audio.data(), audio.pitch, audio.data(), audio.pitch, nd)) return rc; }
    if (nfm_.C) { if (int rc = nfm_.run(cs, audio.data(), audio.pitch, audio.data(), audio.pitch, nd, Gate{nullptr, 0, 0}, (int)ff_.block_len(), (int)nf)) return rc; }
    if (int rc = clear_tune_only_rows(cs, audio.data(), audio.pitch, nd)) return rc;
    return copy_tap(cs, PEBBLEGPU_TAP_POST_DEMOD, audio.data(), audio.pitch, nd, C);  // receiver.cpp:992, before the resampler
}

// Demod_WFM, receiver.cpp:896
int Receiver::tail_wfm(Call &c)
{
    if (profile_detail) PG_HIP(hipEventRecord(c.ev[4], c.cs));
    // (the call's tail refresh rides on the demodulator's launch: it is the last kernel of the call, run on an idle GPU)
    std::vector<TailJob> jobs;
    dec_.tail_jobs(jobs);
    OscAdvance oa;
    if (int rc = osc_.advance_job(c.cs, c.n, &oa)) return rc;
    return wfmc_.run(c.cs, dec_.out().data(), dec_.out().pitch, audio.data(), audio.pitch, c.nd, &jobs, &oa, &c.tails_carried);
}

// resampler, the audio ring's block, and the refresh of every history head-room for the next call
int Receiver::finish_chain(Call &c)
{
    hipStream_t cs = c.cs;
    if (!c.gate_closed) {
        last_audio_n = (uint64_t)c.nd;
        if (audio_rate) {  // CFractResampler::Resample into the audio buffer, receiver.cpp:1000-1001
            long long n_rs = 0;
            if (int rc = resamp_.run(cs, audio.data(), audio.pitch, c.nd, d_audio_rs, rs_pitch, &n_rs)) return rc;
            last_audio_n = (uint64_t)n_rs;
        }
    }
    // Audio::SendToOutput, receiver.cpp:1029-1035: behind the last writer of the audio buffer on whichever stream that was (the
    // resampler, the demodulators, the gate's clears); the next call's writers follow on the same stream or behind its end
    if (aout_.open) { if (int rc = queue_audio_block(cs, last_audio_n)) return rc; }
    if (profile_detail) PG_HIP(hipEventRecord(c.ev[5], cs));
    if (c.rt.bank_pipe) {
        std::vector<TailJob> jobs;
        dec_.tail_job_out(jobs);
        am_.tail_jobs(jobs);
        if (int rc = run_save_tails(cs, jobs, C, nullptr)) return rc;
    } else if (!c.tails_carried) {  // one launch refreshes every history head-room for the next call
        std::vector<TailJob> jobs;
        dec_.tail_jobs(jobs);
        if (wfm && !c.gate_closed) wfmc_.tail_jobs(jobs);  // a gated super-frame never reached the demodulator: its history stays
        OscAdvance oa = c.oa_pre;
        if (!c.have_oa) { if (int rc = osc_.advance_job(cs, c.n, &oa)) return rc; }
        if (int rc = run_save_tails(cs, jobs, C, &oa)) return rc;
    }
    return 0;
}

// the display ring's block and the call's end
int Receiver::end_call(Call &c)
{
    const CallRoute &rt = c.rt;
    hipStream_t cs = c.cs;
    hipEvent_t *ev = c.ev;
    // The display ring's block, where Receiver::map_spectrum would queue a map of each source: the zoomed spectra on the stream that wrote
    // them, the unprocessed spectrum on the main stream -- one stream, and one launch for both panes, unless the call's two pipelines end
    // separately (PEBBLEGPU_PIPELINE=1).  A call that joins its streams does so first.  Ahead of the call's end record, so that whoever
    // waits for the call (sync(), a join, the next call's transform on the same stream) waits for the launch too
    bool joined = false;
    if (disp_open_) {
        hipStream_t spec_s = stream_;
        if (rt.side && !tun_.pipeline) {
            if (!rt.fuse_dec) PG_HIP(hipStreamWaitEvent(cs, ev[1], 0));
            joined = true;
            spec_s = cs;
        }
        if (int rc = queue_display_block(spec_s, c.disp_spec_rows, cs, c.disp_zoom_rows, rt.rescale)) return rc;
    }
    if (!rt.bank_pipe) d_end_prev_ = nullptr;
    if (rt.bank_pipe) {
        PG_HIP(hipEventRecord(ev[6], cs));
        chain_end_ = ev[6];   // for whoever needs both stages over: sync(), a call after a setter, a call of another shape
        spec_end_ = pipe_ev_;
        f_end_[2] = f_end_[1];
        f_end_[1] = f_end_[0];
        f_end_[0] = ev[6];
        {   // this call's second stage reads the buffer the decimator has just written
            bool found = false;
            for (auto &pr : out_reader_) if (pr.first == (const void *)dec_.fin.base) { pr.second = ev[6]; found = true; }
            if (!found) out_reader_.push_back({(const void *)dec_.fin.base, ev[6]});
        }
        d_end_prev_ = ev[6];
    } else if (rt.side && tun_.pipeline) {
        // the call's two pipelines end separately: whoever needs both waits for both (sync(), the next call that is not plain)
        PG_HIP(hipEventRecord(ev[6], cs));
        chain_end_ = ev[6];
        spec_end_ = ev[1];
    } else if (rt.side) {
        // join: the call has ended once both pipelines have, and it ends on the chain's stream.  That stream is the main stream
        // of the next call (the two swap roles): its first kernel then follows this call's last in queue order, where a wait
        // on an event from the other queue cost ~25 us of idle GPU per call
        if (!rt.fuse_dec && !joined) PG_HIP(hipStreamWaitEvent(cs, ev[1], 0));
        if (tun_.end_records) PG_HIP(hipEventRecord(ev[6], cs));
        else tm.open_slot = c.slot;  // (closed by the next call's start record, by sync() or by a timing query)
        std::swap(stream_, chain_stream_);
    } else {
        PG_HIP(hipEventRecord(ev[6], stream_));
    }
    osc_.advance(c.n);
    return 0;
}

int Receiver::process(const float2 *d_iq, uint64_t n, bool with_spectrum, bool with_chain, const RawSrc *raw)
{
    std::lock_guard<std::mutex> g(mu_);
    PG_HIP(hipSetDevice(device));
    last_cond_n_ = 0;
    if (int rc = refuse_call(d_iq, n, with_spectrum, with_chain, raw)) return rc;
    Call c;
    c.rt = plan_call_route(call_facts(n, with_spectrum, with_chain, raw != nullptr));
    c.n = n;
    c.with_spectrum = with_spectrum;
    c.with_chain = with_chain;
    c.d_iq = d_iq;
    c.raw = raw;
    // recording (egress.h): with the generator off a raw call is recorded from the raw samples themselves, whichever way the chain takes
    // them in (the same loader and scale as the conversion pass: the same values, and the recording needs no float2 copy of its own)
    c.rec_raw = raw ? *raw : RawSrc{nullptr, 0, 0, 0.f, 0};
    c.rec_from_raw = raw != nullptr && !tb_.any();
    last_input_ = !raw ? -1 : c.rt.raw_fused ? (raw->fmt >= 0 && raw->fmt <= 4 ? raw->fmt : 4) : 5;
    if (int rc = join_and_apply(c)) return rc;
    if (int rc = stage_input(c)) return rc;
    if (int rc = start_call(c)) return rc;
    // From here on a failing step leaves kernels queued (on the chain stream too) and histories half advanced: whatever the
    // exit, join the two streams so later work is ordered behind what was queued, and refuse further calls on the handle.
    struct Guard {
        Receiver *r; hipEvent_t *ev; hipStream_t cs; bool side, armed;
        ~Guard()
        {
            if (!armed) return;
            r->failed_ = true;
            if (side && hipEventRecord(ev[6], cs) == hipSuccess) r->chain_end_ = ev[6];
        }
    } guard{this, c.ev, c.rt.bank_pipe ? chain_stream_ : c.cs, c.rt.side || c.rt.bank_pipe, true};
    if (int rc = run_display_transform(c)) return rc;
    if (int rc = tap_and_record_input(c)) return rc;
    if (!with_chain) {
        if (int rc = end_without_chain(c)) return rc;
        guard.armed = false;
        return 0;
    }
    if (int rc = run_decimator(c)) return rc;
    if (int rc = run_zoomed_transform(c)) return rc;
    if (int rc = bandpass_and_gate(c)) return rc;
    if (c.gate_closed) { if (int rc = tail_closed(c)) return rc; }
    else if (c.rt.tail == CallTail::BankGated) { if (int rc = tail_bank_gated(c)) return rc; }
    else if (c.rt.tail == CallTail::Narrow) { if (int rc = tail_narrow(c)) return rc; }
    else if (int rc = tail_wfm(c)) return rc;
    if (int rc = finish_chain(c)) return rc;
    if (int rc = end_call(c)) return rc;
    guard.armed = false;
    return 0;
}

int Receiver::process_raw(int fmt, int order, double gain, const void *d_raw, uint64_t n)
{
    if (!d_raw || n == 0) return fail(PEBBLEGPU_E_INVALID, "null input or zero samples");
    if (fmt < 0 || fmt > 4 || order < 0 || order > 3) return fail(PEBBLEGPU_E_INVALID, "unknown sample format %d / IQ order %d", fmt, order);
    if (n > (uint64_t)max_sf * superframe) return fail(PEBBLEGPU_E_SIZE, "%llu samples exceed this object's capacity", (unsigned long long)n);
    // (the converting loads read 8, 16 and 32 bytes at a time: raw_fetch4, raw_load4_even -- the stream bank's rule)
    if (reinterpret_cast<uintptr_t>(d_raw) % PEBBLEGPU_RAW_ALIGN) return fail(PEBBLEGPU_E_INVALID, "d_raw must be aligned to %d bytes", PEBBLEGPU_RAW_ALIGN);
    const RawSrc raw{d_raw, fmt, order, raw_scale(fmt, gain), 0};
    return process(nullptr, n, bins != 0, true, &raw);
}

// ---- host ingest: the pinned double buffer (ingest.h) ----
int Receiver::ingest_acquire(uint32_t slot, uint64_t bytes, void **host_ptr) { return ingest_.acquire(device, slot, bytes, host_ptr); }
int Receiver::ingest_submit(uint32_t slot, uint64_t bytes) { return ingest_.submit(device, slot, bytes); }
// a raw call on a slot of `ring`, ordered behind the slot's upload on the device
int Receiver::process_slot(IngestRing &ring, uint32_t slot, int fmt, int order, double gain, uint64_t n)
{
    IngestSlot *g = nullptr;
    if (int rc = ring.check(slot, fmt, (uint64_t)S * n, n, &g)) return rc;
    PG_HIP(hipSetDevice(device));
    // both of the call's streams read the raw samples (the display transform and the chain's first stage convert in their own loads)
    if (int rc = ring.wait_upload(*g, stream_, chain_stream_)) return rc;
    if (int rc = process_raw(fmt, order, gain, g->d, n)) return rc;
    return ring.mark_in_flight(*g, stream_, chain_stream_);
}
int Receiver::process_ingested(uint32_t slot, int fmt, int order, double gain, uint64_t n) { return process_slot(ingest_, slot, fmt, order, gain, n); }
// the twins of an outside owner's pinned slots (the multibank): same order of steps on the second ring
int Receiver::ingest_wait(uint32_t slot)
{
    PG_HIP(hipSetDevice(device));
    return ext_ingest_.wait_free(slot);
}
int Receiver::ingest_upload(uint32_t slot, const void *h_src, uint64_t bytes) { return ext_ingest_.submit_from(device, slot, h_src, bytes); }
int Receiver::process_uploaded(uint32_t slot, int fmt, int order, double gain, uint64_t n) { return process_slot(ext_ingest_, slot, fmt, order, gain, n); }

// "k_testbench + <front kernel>": one string per front-kernel name, kept for the life of the process like the literals the other groups
// return (the set of names is small and fixed)
// (with stations on the generator's kernel is k_morsegen)
static const char *testbench_label(const char *front, bool morse)
{
    static std::mutex mu;
    static std::map<std::string, std::string> labels[2];
    std::lock_guard<std::mutex> g(mu);
    auto it = labels[morse].find(front);
    if (it == labels[morse].end()) it = labels[morse].emplace(front, std::string(morse ? "k_morsegen + " : "k_testbench + ") + front).first;
    return it->second.c_str();
}

const char *Receiver::kernel_name(int which) const
{
    switch (which) {
    case 1: return !bins ? "" : gated() ? (spec_.any ? "k_spectrum_list_any" : "k_spectrum_list_q128") : spec_.big ? "k_big256_cols + k_big256_rows" : spec_.per_q ? "k_spectrum_q128" : bins == 8192 ? (spec_.use_w64 ? "k_spectrum_w64" : spec_.last_fullc ? "k_spectrum_t128 (twiddles held)" : "k_spectrum_t128") : bins == 4096 ? "k_spectrum<2>" : "k_spectrum_1to1";
    case 2:
        if (!last_tb_) return dec_.front_name();
        return testbench_label(dec_.front_name(), last_tb_morse_);
    case 3: return dec_.rest_name();
    case 4: return wfm ? "" : dec_.last_in_consumer() ? "k_fastfir_t128 (mixing)" : ff_n == 2048 ? "k_fastfir_t128" : "k_fastfir";
    case 5: return wfm ? (wfmc_.fused ? "k_wfm_fir" : "k_iir_scan + k_discrim + k_fir_dec") : "k_anf/k_agc/k_iir_scan/k_pll_demod + k_fir_dec (listed channels only)";
    case 6: {  // the input route of the last call; the format tags are the stream bank's
        static const char *const kIn[8] = {"", "float2", "raw s8", "raw u8", "raw s16", "raw f32", "raw wav16", "k_normalize_iq"};
        return kIn[last_input_ + 2];
    }
    default: return "";
    }
}

int Receiver::close_timing()
{
    if (tm.open_slot >= 0) {  // the last side-by-side call recorded no end event: it ended on what is now the main stream
        PG_HIP(hipEventRecord(tm.ev[tm.open_slot][6], stream_));
        tm.end_ev[tm.open_slot] = tm.ev[tm.open_slot][6];
        tm.open_slot = -1;
    }
    return 0;
}

// The map is queued where the spectrum it reads was written (or where that stream has been joined): the main stream for the
// unprocessed spectrum, the stream that ran the zoomed transform for the zoomed spectra.  The next call's transform of the same buffer
// follows on that stream, so it cannot overwrite the rows before they are read; no host wait.
int Receiver::map_spectrum(bool zoom, const int32_t *edges, bool per_stream, int32_t y_pixels, int32_t x_pixels, double max_db, double min_db,
                           uint32_t first, uint32_t n, uint32_t step, int32_t *d_out)
{
    std::lock_guard<std::mutex> g(mu_);
    if (!d_out || !edges) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (int rc = check_screen_map(y_pixels, x_pixels, max_db, min_db)) return rc;
    if (failed_) return fail(PEBBLEGPU_E_HIP, "an earlier call on this receiver failed half-way: its spectra are not defined");
    const uint32_t fft = zoom ? zoom_bins : bins;
    uint64_t frames = zoom ? last_zoom_frames : last_spec_frames;
    // behind the update timer a call may have made no spectrum: the display then maps the one it still holds (m_unprocessedSpectrum), as row 0
    const bool carried = !zoom && gated() && !frames && have_carry_;
    if (carried) frames = 1;
    if (!fft) return fail(PEBBLEGPU_E_INVALID, zoom ? "the receiver computes no zoomed spectrum (hires_bins = 0)" : "the receiver computes no spectrum (spectrum_bins = 0)");
    if (!frames) return fail(PEBBLEGPU_E_INVALID, "no call with a spectrum has been made yet");
    if (n == 0 || (uint64_t)first + (uint64_t)(n - 1) * step >= frames)
        return fail(PEBBLEGPU_E_INVALID, "frames %u + j * %u, j < %u, are not all within the last call's %llu", first, step, n, (unsigned long long)frames);
    PG_HIP(hipSetDevice(device));
    if (int rc = close_timing()) return rc;  // (a side-by-side call's time ends where it ended, not behind the map)
    const int rows = zoom ? (int)C : (int)S;
    const float *src = carried ? d_spec_carry : (zoom ? d_zoom : d_spec) + (long long)first * fft;
    hipStream_t ms = zoom && zoom_stream_ ? zoom_stream_ : stream_;
    if (int rc = run_screen_map(ms, src, (long long)frames * fft, (long long)step * fft, rows, (int)n, (int32_t)fft,
                                zoom ? (double)demod_rate_int : fs, edges, per_stream, y_pixels, x_pixels, max_db, min_db, d_out)) return rc;
    if (ms == chain_stream_ && chain_end_) {  // a join waits for the map too: the next call may write the zoomed spectra on the main stream
        if (!map_ev_) PG_HIP(hipEventCreateWithFlags(&map_ev_, hipEventDisableTiming));
        PG_HIP(hipEventRecord(map_ev_, chain_stream_));
        chain_end_ = map_ev_;
    }
    return 0;
}

int Receiver::sync()
{
    PG_HIP(hipSetDevice(device));
    if (int rc = close_timing()) return rc;
    PG_HIP(hipStreamSynchronize(stream_));
    PG_HIP(hipStreamSynchronize(chain_stream_));
    return 0;
}

// CB_ProcessIQData shape: one frame in; audio appears once a whole super-frame has been collected, exactly where
// the reference stops returning early (receiver.cpp:922-931).
int Receiver::process_iq(const double *iq, uint16_t n, double *audio_out, uint32_t *n_audio, double *spectrum_db, uint32_t *spectrum_updated)
{
    last_cond_n_ = 0;
    if (!iq || !n_audio) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (n != nf) return fail(PEBBLEGPU_E_SIZE, "process_iq takes frames of %u samples", nf);
    if (S != 1) return fail(PEBBLEGPU_E_UNSUPPORTED, "process_iq feeds one stream; this bank has %u", S);
    if (cond_.any || cond_.dirty)
        return fail(PEBBLEGPU_E_UNSUPPORTED, "the input conditioners run on the batched device path (pebblegpu_receiver_process) only");
    if (tb_.any() || taps_)  // (here `iq` is a host CPX *: the host injects and displays itself)
        return fail(PEBBLEGPU_E_UNSUPPORTED, "the test bench's generator and taps run on the batched device path (pebblegpu_receiver_process) only");
    if (aout_.open || rec_.open || mout_.open || disp_open_)  // (this entry point returns its audio and its spectrum itself, and the host holds the frame it passes in)
        return fail(PEBBLEGPU_E_UNSUPPORTED, "the audio, recording, modem and display rings follow the batched device path (pebblegpu_receiver_process) only: close them first");
    PG_HIP(hipSetDevice(device));
    if (!d_stage_in_) PG_TRY(d_stage_in_.alloc(superframe));
    h_frame_.resize((size_t)nf * 2);
    for (size_t i = 0; i < (size_t)nf * 2; i++) h_frame_[i] = (float)iq[i];
    float2 *dst = d_stage_in_ + acc_frames_ * nf;
    PG_HIP(hipMemcpy(dst, h_frame_.data(), sizeof(float2) * nf, hipMemcpyHostToDevice));
    *n_audio = 0;
    if (spectrum_updated) *spectrum_updated = 0;
    if ((spectrum_db || squelch_db_ > -120.0 || gated()) && bins) {  // the gate reads the latest frame's spectrum, wanted by the host or not (and the update timer counts every frame)
        if (int rc = process(dst, nf, true, false)) return rc;
        if (spectrum_updated) *spectrum_updated = last_spec_frames ? 1u : 0u;
    } else if (bins) {
        std::lock_guard<std::mutex> g(mu_);
        ut_spec_.advance(-1, 0, 1, nf, (uint64_t)fs, nullptr);
    }
    if (spectrum_db && bins && last_spec_frames) {  // (under the update timer only a frame that got a spectrum hands one out)
        if (int rc = sync()) return rc;
        h_out_.resize(bins);
        PG_HIP(hipMemcpy(h_out_.data(), d_spec, sizeof(float) * bins, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < bins; i++) spectrum_db[i] = (double)h_out_[i];
    }
    acc_frames_++;
    if (acc_frames_ * nf >= superframe) {
        acc_frames_ = 0;
        if (int rc = process(d_stage_in_, superframe, false, true)) return rc;
        if (int rc = sync()) return rc;
        const size_t na = (size_t)last_audio_n;
        h_out_.resize(na * 2);
        PG_HIP(hipMemcpy(h_out_.data(), audio_ptr(), sizeof(float2) * na, hipMemcpyDeviceToHost));
        if (audio_out)
            for (size_t i = 0; i < na * 2; i++) audio_out[i] = (double)h_out_[i];
        *n_audio = (uint32_t)na;
    }
    return 0;
}

}  // namespace pg
