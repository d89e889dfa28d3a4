// morse.hip -- MorseCore: the Morse digital modem (plugins/MorseDigitalModem/morse.cpp, Goertzel path) for the channels of a
// receiver or for the stand-alone step, and the step's C ABI (pebblegpu_morse_*).  Kernels: kernels_modem.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include "kernels_modem.h"
#include "receiver.h"

namespace pg {

static long long cdiv_ll(long long a, long long b) { return (a + b - 1) / b; }

// Morse::setSampleRate + init (morse.cpp:160-246, :566-601) for one channel, as the device state: a new GoertzelOOK (goertzel.cpp:351-373),
// a new dot-dash threshold filter, dmCWL, updateThresholds(1200000 / wpm, true), setMinMaxMark(10, 50), the filter reset, IDLE
static MorseState fresh_state(int32_t wpm)
{
    MorseState s;
    memset(&s, 0, sizeof(s));
    s.minp = 1.0;  // m_minPower = 1.0 while its filter starts at 0: the first result always reads as a tone
    s.neg = 1;     // m_demodMode = dmCWL whatever the receiver's mode (morse.cpp:181)
    const uint32_t w = wpm < 5 ? 5u : (uint32_t)wpm;
    s.wpm = (int32_t)w;
    morse_update_thresholds(s, kMorseDotMagic / w, true);
    s.shortest = (uint32_t)(kMorseDotMagic / ((int)kMorseWpmHigh * 1.10));
    s.sma_primed = 0; s.sma_idx = 0; s.sma_sum = 0; s.sma_avg = 0;  // m_dotDashThresholdFilter->reset()
    morse_reset_clock(s);
    s.state = kMsIdle;
    return s;
}

int MorseCore::init(uint32_t channels, uint32_t demod_rate, long long max_n, bool keep_tone)
{
    C = channels;
    in_rate = demod_rate;
    cap_in = max_n;
    chain = design::build_chain(demod_rate, 1000, 8000);
    if (chain.stages.size() > (size_t)kMaxStages) return fail(PEBBLEGPU_E_UNSUPPORTED, "modem chain of %zu stages", chain.stages.size());
    pp.rate = (uint32_t)(int)chain.rate;  // int actualModemRate (morse.cpp:193)
    if (pp.rate == 0) return fail(PEBBLEGPU_E_UNSUPPORTED, "no modem rate below %u", demod_rate);
    // findBestGoertzelN(10, 50), morse.cpp:396-446 (#else branch): quint32 arithmetic throughout
    const uint32_t usec_per_sample = (uint32_t)(1.0e6 / (int)pp.rate);
    pp.N = usec_per_sample ? ((kMorseDotMagic / ((kMorseWpmLow + kMorseWpmHigh) / 2)) / 4u) / usec_per_sample : 0;
    if (pp.N < 1) return fail(PEBBLEGPU_E_UNSUPPORTED, "modem rate %u gives no Goertzel block", pp.rate);
    // Goertzel::setFreq(+-1000, N, rate), goertzel.cpp:154-219: negative tones move up by the rate; only the coefficients change
    for (int q = 0; q < 2; q++) {
        int32_t f = q ? -1000 : 1000;
        if (f < 0) f = f + (int32_t)pp.rate;
        const double nfq = (double)f / (double)pp.rate;
        const double k = nfq * pp.N;
        const double A = design::kTwoPi * k / pp.N;
        pp.B[q] = 2 * std::cos(A);
        // c_C = exp(-c_j * c_A), c_D = exp(-c_j * c_A * (N - 1)) with pebblelib's c_j = {6.123233995736766e-17, 1} (cpx.h:158), not {0, 1}:
        // the modulus is exp(-6.1e-17 A (N - 1)), up to 3e-14 under 1
        const double cj_re = 6.123233995736766e-17;
        const double eC = std::exp(-cj_re * A);
        pp.Cr[q] = eC * std::cos(A);
        pp.Ci[q] = -(eC * std::sin(A));
        const double AD = A * ((double)pp.N - 1.0);
        const double eD = std::exp((-cj_re * A) * ((double)pp.N - 1.0));
        pp.Dr[q] = eD * std::cos(AD);
        pp.Di[q] = -(eD * std::sin(AD));
    }
    long long len = max_n;
    for (const design::Stage &st : chain.stages) {
        if (st.ntaps < 1 || st.ntaps > kMaxTaps) return fail(PEBBLEGPU_E_UNSUPPORTED, "modem stage of %d taps", st.ntaps);
        std::vector<float> h(kMaxTaps, 0.f);
        for (int p = 0; p < st.ntaps; p++) h[p] = (float)design::halfband_taps(st.design)[p];
        DevBuf<float> t;
        PG_TRY(t.upload(h.data(), kMaxTaps));
        d_taps.push_back(std::move(t));
        DevBuf<float2> hb;
        PG_TRY(hb.alloc_zero((size_t)kMaxTaps * C));
        d_hist.push_back(std::move(hb));
        len /= st.stride;
        const long long pitch = (len + 1) & ~1LL;
        DevBuf<float2> o;
        PG_TRY(o.alloc((size_t)pitch * C));
        d_out.push_back(std::move(o));
        out_pitch.push_back(pitch);
    }
    rpitch = len / pp.N + 2;
    log_cap = (int)std::max<long long>(1024, 2 * rpitch);
    PG_TRY(d_power.alloc((size_t)rpitch * C));
    if (keep_tone) PG_TRY(d_tone.alloc((size_t)rpitch * C));
    PG_TRY(d_state.alloc_zero(C));
    PG_TRY(d_log.alloc((size_t)log_cap * C));
    PG_TRY(d_list.alloc(C));
    PG_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    on.assign(C, 0);
    tune_only.assign(C, 0);
    wpm.assign(C, 20);  // "Initially 20 WPM" (morse.h:223): the member is read before anything sets it
    host.assign(C, Host());
    return 0;
}

void MorseCore::release()
{
    d_taps.clear(); d_hist.clear(); d_out.clear(); out_pitch.clear();
    d_power.release(); d_tone.release(); d_state.release(); d_log.release(); d_list.release();
    if (done) (void)hipEventDestroy(done);
    done = nullptr;
    C = 0;
    n_on = 0;
    list.clear();
    recorded = false;
    since_drain = 0;
}

int MorseCore::check(long long n) const
{
    if (n > cap_in) return fail(PEBBLEGPU_E_SIZE, "%lld samples exceed the modem's capacity", n);
    if (n % (long long)chain.total != 0)
        return fail(PEBBLEGPU_E_SIZE, "the Morse modem decimates by %u: calls must be multiples of that", chain.total);
    long long len = n;
    for (const design::Stage &st : chain.stages) {
        if (len < st.ntaps)  // Decimator::process's fallback for short frames (decimator.cpp:602-625) would drop samples unfiltered
            return fail(PEBBLEGPU_E_SIZE, "a call of %lld samples is shorter than the Morse modem's %d-tap stage needs", n, st.ntaps);
        len /= st.stride;
    }
    return 0;
}

int MorseCore::upload_list()
{
    list.clear();
    n_on = 0;
    for (uint32_t c = 0; c < C; c++) {
        if (on[c]) n_on++;
        if (on[c] && !tune_only[c]) list.push_back((int)c);
    }
    if (!list.empty()) PG_HIP(hipMemcpy(d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
    return 0;
}

int MorseCore::enable(uint32_t ch, bool en, int mode)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (recorded) PG_HIP(hipEventSynchronize(done));
    if (int rc = drain()) return rc;  // what the channel has decided so far reaches its host queue
    if (on[ch]) {
        // the plugin object outlives setSampleRate and setDigitalModem(NULL): its m_wpmSpeedCurrent is where the next init starts
        MorseState s;
        PG_HIP(hipMemcpy(&s, d_state + ch, sizeof(s), hipMemcpyDeviceToHost));
        wpm[ch] = s.wpm;
    }
    if (!en) {
        host[ch] = Host();  // setDigitalModem(NULL): the decoder's state goes, and what it decided that was not read
    } else {
        // setDigitalModem -> setSampleRate (morse.cpp:160-246), on a channel whose modem is off or already on: a fresh decoder in dmCWL
        // (a new Decimator, GoertzelOOK and threshold filter) from the current WPM estimate; events decided before stay readable
        const MorseState s = fresh_state(wpm[ch]);
        PG_HIP(hipMemcpy(d_state + ch, &s, sizeof(s), hipMemcpyHostToDevice));
        float2 z[kMaxTaps] = {};
        for (const DevBuf<float2> &hb : d_hist) PG_HIP(hipMemcpy(hb + (size_t)ch * kMaxTaps, z, sizeof(z), hipMemcpyHostToDevice));
        if (!on[ch]) host[ch] = Host();
        host[ch].seen = 0;  // the new decoder's log count starts at 0
    }
    on[ch] = en ? 1 : 0;
    tune_only[ch] = mode == PEBBLEGPU_DM_NONE ? 1 : 0;
    return upload_list();
}

int MorseCore::set_mode(uint32_t ch, int mode)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    tune_only[ch] = mode == PEBBLEGPU_DM_NONE ? 1 : 0;
    if (!on[ch]) return 0;
    if (recorded) PG_HIP(hipEventSynchronize(done));
    // Morse::updateGoertzel (morse.cpp:345-373): -1000 Hz for CWL and LSB, +1000 Hz otherwise; a block under way keeps its sums
    const uint32_t neg = (mode == PEBBLEGPU_DM_CWL || mode == PEBBLEGPU_DM_LSB) ? 1u : 0u;
    PG_HIP(hipMemcpy(reinterpret_cast<char *>(d_state + ch) + offsetof(MorseState, neg), &neg, sizeof(neg), hipMemcpyHostToDevice));
    return upload_list();
}

int MorseCore::run(hipStream_t s, const float2 *in, long long in_pitch, long long n)
{
    if (list.empty() || n <= 0) return 0;
    if (int rc = check(n)) return rc;
    const long long m = n / (long long)chain.total;
    const long long rmax = m / pp.N + 1;
    if (since_drain + rmax > log_cap) {  // the logs could wrap before the host reads them: move what they hold to the host first
        if (int rc = drain()) return rc;
    }
    since_drain += rmax;
    const int nl = (int)list.size();
    MorseTails tj;
    memset(&tj, 0, sizeof(tj));
    const float2 *x = in;
    long long xp = in_pitch, len = n;
    for (size_t j = 0; j < chain.stages.size(); j++) {
        const design::Stage &st = chain.stages[j];
        const long long n_out = len / st.stride;
        launch(k_morse_fir, dim3((unsigned)cdiv_ll(n_out, 256), nl), dim3(256), s, x, xp, (const float2 *)d_hist[j], kMaxTaps, d_out[j], out_pitch[j],
               n_out, (int)st.stride, (const float *)d_taps[j], st.ntaps, (const int *)d_list);
        tj.in[j] = x; tj.in_pitch[j] = xp; tj.n[j] = len; tj.hist[j] = d_hist[j]; tj.keep[j] = st.ntaps - 1;
        x = d_out[j]; xp = out_pitch[j]; len = n_out;
    }
    if (!chain.stages.empty())  // a demodulator rate of 8000 Hz or less has no stage, and a grid of no blocks is no launch
        launch(k_morse_tails, dim3((unsigned)chain.stages.size(), nl), dim3(64), s, tj, kMaxTaps, (const int *)d_list);
    launch(k_morse_goertzel, dim3(nl), dim3(64), s, x, xp, m, pp, d_state, d_power, rpitch, (const int *)d_list);
    launch(k_morse_decide, dim3((unsigned)cdiv_ll(nl, 64)), dim3(64), s, (const double *)d_power, rpitch, m, pp.N, pp.rate, d_state, d_log, log_cap,
           d_tone, (const int *)d_list, nl);
    PG_HIP(hipGetLastError());
    PG_HIP(hipEventRecord(done, s));
    recorded = true;
    return 0;
}

int MorseCore::drain()
{
    since_drain = 0;
    if (!recorded || n_on == 0) return 0;
    PG_HIP(hipEventSynchronize(done));
    h_state.resize(C);
    PG_HIP(hipMemcpy(h_state.data(), d_state, sizeof(MorseState) * C, hipMemcpyDeviceToHost));
    bool any_new = false;
    for (uint32_t c = 0; c < C; c++) any_new = any_new || (on[c] && h_state[c].n_events > host[c].seen);
    if (!any_new) return 0;
    h_log.resize((size_t)log_cap * C);
    PG_HIP(hipMemcpy(h_log.data(), d_log, sizeof(MorseEvent) * (size_t)log_cap * C, hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < C; c++) {
        if (!on[c]) continue;
        Host &h = host[c];
        const uint64_t total = h_state[c].n_events;
        for (uint64_t e = h.seen; e < total; e++) h.q.push_back(h_log[(size_t)c * log_cap + (size_t)(e % (uint64_t)log_cap)]);
        h.seen = total;
    }
    return 0;
}

int MorseCore::events(uint32_t ch, MorseEvent *ev, uint32_t cap, uint32_t *n)
{
    if (n) *n = 0;
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (int rc = drain()) return rc;
    Host &h = host[ch];
    const uint32_t k = (uint32_t)std::min<size_t>(h.q.size(), cap);
    if (ev) std::copy(h.q.begin(), h.q.begin() + k, ev);
    h.q.erase(h.q.begin(), h.q.begin() + k);
    if (n) *n = k;
    return 0;
}

int MorseCore::status(uint32_t ch, MorseStatus *st)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (!on[ch]) return fail(PEBBLEGPU_E_INVALID, "the Morse modem of channel %u is off", ch);
    if (recorded) PG_HIP(hipEventSynchronize(done));
    MorseState s;
    PG_HIP(hipMemcpy(&s, d_state + ch, sizeof(s), hipMemcpyDeviceToHost));
    st->wpm = s.wpm;
    st->above = s.above;
    st->below = s.below;
    st->rate = pp.rate;
    st->samples_per_result = pp.N;
    return 0;
}

}  // namespace pg

using pg::fail;

// DigitalModemInterface for the Morse plugin on one stream of host frames: setSampleRate(sample_rate, sample_count), processBlock(CPX *)
struct pebblegpu_morse {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t count = 0;
    pg::MorseCore core;
    pg::DevBuf<float2> d_in;
    std::vector<float> hf;
    std::vector<pg::MorseEvent> carried;  // events of the decoder a setSampleRate replaced, not read yet (handed out first)
    bool keep = false;                // pebblegpu_morse_keep_results: collect the parity read-out
    std::vector<double> pw;           // per-result powers and decisions since the last pebblegpu_morse_results
    std::vector<unsigned char> tone, th;
};

// Morse::setSampleRate(sample_rate, sample_count) on the step: everything new but the WPM estimate the plugin object keeps (wpm < 0: 20)
static int morse_open(pebblegpu_morse *m, uint32_t sample_rate, uint32_t sample_count, int32_t wpm)
{
    {   // what init or check refuses is refused before the handle is touched: the decoder that runs keeps running as it was
        pg::MorseCore probe;
        int rc = probe.init(1, sample_rate, sample_count, true);
        if (!rc) rc = probe.check(sample_count);
        probe.release();
        if (rc) return rc;
    }
    m->core.release();
    m->d_in.release();
    m->count = sample_count;
    m->pw.clear();
    m->tone.clear();
    if (int rc = m->core.init(1, sample_rate, sample_count, true)) return rc;
    if (int rc = m->core.check(sample_count)) return rc;
    PG_TRY(m->d_in.alloc(sample_count));
    if (wpm >= 0) m->core.wpm[0] = wpm;
    return m->core.enable(0, true, PEBBLEGPU_DM_CWL);
}

extern "C" {

int pebblegpu_morse_destroy(pebblegpu_morse *m)
{
    if (!m) return 0;
    (void)hipSetDevice(m->device);
    if (m->stream) { (void)hipStreamSynchronize(m->stream); (void)hipStreamDestroy(m->stream); }
    m->core.release();
    delete m;
    return 0;
}

int pebblegpu_morse_create(int device, uint32_t sample_rate, uint32_t sample_count, pebblegpu_morse **out)
{
    if (!out) return fail(PEBBLEGPU_E_INVALID, "null argument");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return fail(PEBBLEGPU_E_NO_DEVICE, "no HIP device visible: libpebblegpu has no CPU path");
    if (device < 0 || device >= nd) return fail(PEBBLEGPU_E_INVALID, "device %d out of range", device);
    if (sample_rate == 0 || sample_count == 0 || sample_rate > 0x7fffffffu) return fail(PEBBLEGPU_E_INVALID, "bad sample rate or count");
    pebblegpu_morse *m = new (std::nothrow) pebblegpu_morse();
    if (!m) return fail(PEBBLEGPU_E_INVALID, "out of host memory");
    m->device = device;
    int rc = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) == hipSuccess ? 0 : fail(PEBBLEGPU_E_HIP, "stream");
    if (!rc) rc = morse_open(m, sample_rate, sample_count, -1);
    if (rc) { pebblegpu_morse_destroy(m); return rc; }
    *out = m;
    return 0;
}

int pebblegpu_morse_set_sample_rate(pebblegpu_morse *m, uint32_t sample_rate, uint32_t sample_count)
{
    if (!m) return fail(PEBBLEGPU_E_INVALID, "null handle");
    if (sample_rate == 0 || sample_count == 0 || sample_rate > 0x7fffffffu) return fail(PEBBLEGPU_E_INVALID, "bad sample rate or count");
    PG_HIP(hipSetDevice(m->device));
    PG_HIP(hipStreamSynchronize(m->stream));
    int32_t wpm = -1;
    if (m->core.C) {
        pg::MorseStatus st;
        if (int rc = m->core.status(0, &st)) return rc;
        wpm = st.wpm;
        uint32_t k = 0;
        do {  // what the old decoder decided stays readable
            pg::MorseEvent ev[256];
            if (int rc = m->core.events(0, ev, 256, &k)) return rc;
            m->carried.insert(m->carried.end(), ev, ev + k);
        } while (k == 256);
    }
    return morse_open(m, sample_rate, sample_count, wpm);
}

int pebblegpu_morse_keep_results(pebblegpu_morse *m, int on)
{
    if (!m) return fail(PEBBLEGPU_E_INVALID, "null handle");
    m->keep = on != 0;
    if (!m->keep) { m->pw.clear(); m->tone.clear(); }
    return 0;
}

int pebblegpu_morse_set_demod_mode(pebblegpu_morse *m, int mode)
{
    if (!m) return fail(PEBBLEGPU_E_INVALID, "null handle");
    if (mode < 0 || mode > PEBBLEGPU_DM_NONE) return fail(PEBBLEGPU_E_INVALID, "demod mode %d", mode);
    PG_HIP(hipSetDevice(m->device));
    // the step is processBlock alone: dmNONE only moves the tone (the receiver's dmNONE return is not part of the modem)
    if (int rc = m->core.set_mode(0, mode == PEBBLEGPU_DM_NONE ? PEBBLEGPU_DM_USB : mode)) return rc;
    return 0;
}

int pebblegpu_morse_process(pebblegpu_morse *m, const double *in)
{
    if (!m || !in) return fail(PEBBLEGPU_E_INVALID, "null argument");
    PG_HIP(hipSetDevice(m->device));
    const size_t n = m->count;
    m->hf.resize(n * 2);
    for (size_t i = 0; i < n * 2; i++) m->hf[i] = (float)in[i];
    PG_HIP(hipMemcpyAsync(m->d_in, m->hf.data(), sizeof(float2) * n, hipMemcpyHostToDevice, m->stream));
    if (int rc = m->core.run(m->stream, m->d_in, (long long)n, (long long)n)) return rc;
    if (!m->keep) {
        PG_HIP(hipStreamSynchronize(m->stream));  // (returns with the frame consumed, as every host-buffer step does)
        return 0;
    }
    // the parity read-out, when asked for: this call's results (k_morse_goertzel's count, then the powers and decisions)
    pg::MorseState s;
    PG_HIP(hipMemcpyAsync(&s, m->core.d_state, sizeof(s), hipMemcpyDeviceToHost, m->stream));
    PG_HIP(hipStreamSynchronize(m->stream));
    if (s.nres) {
        const size_t k = s.nres;
        std::vector<double> p(k);
        m->th.resize(k);
        PG_HIP(hipMemcpy(p.data(), m->core.d_power, sizeof(double) * k, hipMemcpyDeviceToHost));
        PG_HIP(hipMemcpy(m->th.data(), m->core.d_tone, k, hipMemcpyDeviceToHost));
        m->pw.insert(m->pw.end(), p.begin(), p.end());
        m->tone.insert(m->tone.end(), m->th.begin(), m->th.end());
    }
    return 0;
}

int pebblegpu_morse_events(pebblegpu_morse *m, pebblegpu_morse_event *ev, uint32_t cap, uint32_t *n)
{
    if (!m || !n) return fail(PEBBLEGPU_E_INVALID, "null argument");
    static_assert(sizeof(pebblegpu_morse_event) == sizeof(pg::MorseEvent), "event layout");
    PG_HIP(hipSetDevice(m->device));
    if (!ev) cap = 0;
    const uint32_t k = (uint32_t)std::min<size_t>(m->carried.size(), cap);
    std::copy(m->carried.begin(), m->carried.begin() + k, reinterpret_cast<pg::MorseEvent *>(ev));
    m->carried.erase(m->carried.begin(), m->carried.begin() + k);
    uint32_t more = 0;
    if (int rc = m->core.events(0, k < cap ? reinterpret_cast<pg::MorseEvent *>(ev) + k : nullptr, cap - k, &more)) return rc;
    *n = k + more;
    return 0;
}

int pebblegpu_morse_status(pebblegpu_morse *m, pebblegpu_morse_report *st)
{
    if (!m || !st) return fail(PEBBLEGPU_E_INVALID, "null argument");
    static_assert(sizeof(pebblegpu_morse_report) == sizeof(pg::MorseStatus), "status layout");
    PG_HIP(hipSetDevice(m->device));
    return m->core.status(0, reinterpret_cast<pg::MorseStatus *>(st));
}

int pebblegpu_morse_results(pebblegpu_morse *m, double *power, uint8_t *tone, uint32_t cap, uint32_t *n)
{
    if (!m || !n) return fail(PEBBLEGPU_E_INVALID, "null argument");
    const uint32_t k = (uint32_t)std::min<size_t>(m->pw.size(), cap);
    if (power) std::copy(m->pw.begin(), m->pw.begin() + k, power);
    if (tone) std::copy(m->tone.begin(), m->tone.begin() + k, tone);
    m->pw.erase(m->pw.begin(), m->pw.begin() + k);
    m->tone.erase(m->tone.begin(), m->tone.begin() + k);
    *n = k;
    return 0;
}

}  // extern "C"
