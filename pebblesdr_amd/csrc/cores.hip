// cores.hip -- the device cores (see receiver.h): state allocation, parameter design upload, kernel launches.
// This is the only translation unit that instantiates kernels.
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <hip/hip_ext.h>
#include "kernels_demod.h"
#include "kernels_fastfir.h"
#include "kernels_frontend.h"
#include <algorithm>
#include "bank_geom.h"
#include "spectrum_geom.h"
#include "kernels_fused_dec.h"
#include "kernels_bank_dec.h"
#include "kernels_spectrum.h"
#include "receiver.h"

namespace pg {

std::string &last_error()
{
    static thread_local std::string e;
    return e;
}
int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}

static inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

int HistBuf::alloc(int channels, int hist_len, long long capacity)
{
    hist = (hist_len + 1) & ~1;  // keep data 16-byte aligned
    cap = capacity;
    chans = channels;
    pitch = (hist + capacity + 1) & ~1LL;
    return base.alloc_zero((size_t)pitch * channels);
}

static design::M2 section_matrix(const ScanSection &s)
{
    if (s.type == kBiquadDf2) return design::M2{-s.c[3], -s.c[4], 1.0, 0.0};
    return design::M2{s.type == kOnePoleDiff ? s.c[0] : 1.0 - s.c[0], 0, 0, 0};
}

void fill_scan_section(ScanSection &s, int type, const double *c)
{
    memset(&s, 0, sizeof(s));
    s.type = type;
    for (int i = 0; i < (type == kBiquadDf2 ? 5 : 1); i++) s.c[i] = c[i];
    const design::M2 m = section_matrix(s);
    for (int k = 0; k < 6; k++) {
        const design::M2 p = design::m2_pow(m, (uint64_t)kSeg << k);
        s.P[k][0] = p.a; s.P[k][1] = p.b; s.P[k][2] = p.c; s.P[k][3] = p.d;
    }
}

int make_twiddles(int n, DevBuf<float2> &tw)
{
    // per-pass tables in the layout fft_lds.h reads (fft_tw_off)
    if (!(n == 2048 || n == 4096 || n == 8192)) return fail(PEBBLEGPU_E_UNSUPPORTED, "no FFT plan for %d points", n);
    std::vector<float2> h((size_t)fft_tw_off(n, n));
    int P = 1;
    for (int pass = 0; pass < fft_passes(n); pass++) {
        const int R = fft_radix(n, pass);
        if (P > 1) {
            float2 *t = h.data() + fft_tw_off(n, P);
            for (int k = 0; k < P; k++)
                for (int e = 0; e < 3; e++) {
                    const long long idx = ((long long)k * (n / (P * R)) << e) % n;
                    const double a = -design::kTwoPi * (double)idx / (double)n;
                    t[e * P + k] = make_float2((float)std::cos(a), (float)std::sin(a));
                }
        }
        P *= R;
    }
    return tw.upload(h.data(), h.size());
}

int make_twiddles_t128(DevBuf<float2> &tw)
{
    // fft_t128.h: pass B W^{16k}, W^{32k}, W^{64k} (k < 16); pass C W^{k}, W^{2k}, W^{4k}, W^{8k} (k < 128); W = exp(-2 pi i / 2048)
    std::vector<float2> t2((size_t)kTw128Count);
    auto W = [](long long idx) {
        const double a = -design::kTwoPi * (double)(idx % 2048) / 2048.0;
        return make_float2((float)std::cos(a), (float)std::sin(a));
    };
    for (int k = 0; k < 16; k++)
        for (int e = 0; e < 3; e++) t2[kTw128B + e * 16 + k] = W((long long)(16 * k) << e);
    for (int k = 0; k < 128; k++)
        for (int e = 0; e < 4; e++) t2[kTw128C + e * 128 + k] = W((long long)k << e);
    return tw.upload(t2.data(), t2.size());
}

// k_spectrum_t128 (8192 bins = four transforms x[n] W_8192^{n q} of a 2048-sample frame): one such table per q with the per-work-item
// part of that factor, W_8192^{t q}, folded in -- pass B's entries times W_8192^{16 q << e}, pass C's times W_8192^{q << e}
int make_twiddles_t128q(DevBuf<float2> &tw)
{
    std::vector<float2> t2((size_t)4 * kTw128Count);
    auto W = [](long long idx) {
        const double a = -design::kTwoPi * (double)(idx % 8192) / 8192.0;
        return make_float2((float)std::cos(a), (float)std::sin(a));
    };
    for (int q = 0; q < 4; q++) {
        float2 *t = t2.data() + (size_t)q * kTw128Count;
        for (int k = 0; k < 16; k++)
            for (int e = 0; e < 3; e++) t[kTw128B + e * 16 + k] = W((long long)(64 * k + 16 * q) << e);
        for (int k = 0; k < 128; k++)
            for (int e = 0; e < 4; e++) t[kTw128C + e * 128 + k] = W((long long)(4 * k + q) << e);
    }
    return tw.upload(t2.data(), t2.size());
}

// ------------------------------------------------------------------------------------------------
// OscBank
// ------------------------------------------------------------------------------------------------
int OscBank::init(uint32_t channels, double sample_rate)
{
    static_assert(sizeof(OscBank::Dyn) == kChanOscDynBytes && offsetof(ChanOsc, inc) == kChanOscDynBytes, "ChanOsc layout");
    C = channels;
    fs = sample_rate;
    ctl.assign(C, Ctl());
    h_osc.assign(C, ChanOsc());
    for (int i = 0; i < 2; i++) {
        PG_TRY(h_dyn[i].alloc(C));
        PG_HIP(hipEventCreate(&h_done[i]));
    }
    PG_TRY(d_osc.alloc_zero(C));
    std::vector<float> amp(kAmpTab);
    design::mixer_amplitudes(amp.data(), kAmpTab, &a_inf);
    return d_amp.upload(amp.data(), kAmpTab);
}
void OscBank::release()
{
    for (int i = 0; i < 2; i++) {
        if (h_done[i]) (void)hipEventDestroy(h_done[i]);
        h_done[i] = nullptr;
        h_dyn[i].release();
    }
    d_osc.release();
    d_amp.release();
    d_adv.release();
}
void OscBank::retune(uint32_t ch, double f)
{
    Ctl &c = ctl[ch];
    c.freq = f;
    c.inc = (-f) / fs;  // m_frequency = -f; m_oscInc = TWOPI*m_frequency/m_sampleRate  (mixer.cpp:31-34)
    c.phase0 = 0;       // m_lastOsc = (1, 0)  (mixer.cpp:37-38)
    c.n0 = 0;
    c.dirty = true;
    adv_stale = true;
}
// CDownConvert::SetFrequency (pebblelib/downconvert.cpp:100-112): a new increment for the oscillator as it stands -- phase and amplitude
// recurrence go on (m_Osc1 is not touched), where Mixer::setFrequency starts over
void OscBank::retune_keep(uint32_t ch, double f)
{
    Ctl &c = ctl[ch];
    c.freq = f;
    c.inc = (-f) / fs;
    c.dirty = true;
    adv_stale = true;
}
int OscBank::upload(hipStream_t s)
{
    // retuned channels: rebuild the constant part (phasor step tables) and upload the whole block, synchronously (rare)
    for (uint32_t ch = 0; ch < C; ch++) {
        Ctl &c = ctl[ch];
        if (!c.dirty) continue;
        ChanOsc &o = h_osc[ch];
        for (int d = 0; d < kMaxTaps; d++) {
            double ph = (double)d * c.inc;
            ph -= std::floor(ph);
            o.step[d] = make_float2((float)std::cos(design::kTwoPi * ph), (float)std::sin(design::kTwoPi * ph));
        }
        double ph = 512.0 * c.inc;
        ph -= std::floor(ph);
        o.step512 = make_float2((float)std::cos(design::kTwoPi * ph), (float)std::sin(design::kTwoPi * ph));
        o.inc = c.inc;
        o.mix_on = (force_mix || (-c.freq) != 0) ? 1u : 0u;  // if (m_frequency == 0) return in;  (mixer.cpp:51-53; CDownConvert has no such exit)
        o.phase0 = c.phase0;
        o.n0 = 0;
        PG_HIP(hipMemcpyAsync(d_osc + ch, &o, sizeof(ChanOsc), hipMemcpyHostToDevice, s));
        PG_HIP(hipStreamSynchronize(s));
        c.dirty = false;
        dyn_epoch++;
    }
    if (device_advance && dev_dyn_valid && C > (uint32_t)kOscInline) return 0;  // the previous call's tail launch advanced them on the device
    dyn_epoch++;
    // every call: phase and amplitude-transient position, 16 bytes per channel, from pinned ping-pong staging
    const int cur = h_idx;
    h_idx ^= 1;
    PG_HIP(hipEventSynchronize(h_done[cur]));  // copy issued two uploads ago: finished long since, never waits in steady state
    Dyn *hd = h_dyn[cur];
    for (uint32_t ch = 0; ch < C; ch++) {
        hd[ch].phase0 = ctl[ch].phase0;
        hd[ch].n0 = (uint32_t)(ctl[ch].n0 > (uint64_t)kAmpTab ? (uint64_t)kAmpTab : ctl[ch].n0);
        hd[ch].mix_on = h_osc[ch].mix_on;
    }
    inline_dyn.use = 0;
    if (allow_inline && C <= (uint32_t)kOscInline) {  // small bank: the consumer takes these 16 bytes per channel as kernel arguments
        for (uint32_t ch = 0; ch < C; ch++) {
            inline_dyn.d[ch].phase0 = hd[ch].phase0;
            inline_dyn.d[ch].n0 = hd[ch].n0;
            inline_dyn.d[ch].mix_on = hd[ch].mix_on;
        }
        inline_dyn.use = 1;
        return 0;
    }
    PG_HIP(hipMemcpy2DAsync(d_osc, sizeof(ChanOsc), hd, sizeof(Dyn), sizeof(Dyn), C, hipMemcpyHostToDevice, s));
    PG_HIP(hipEventRecord(h_done[cur], s));
    return 0;
}
int OscBank::advance_job(hipStream_t s, uint64_t n, OscAdvance *oa)
{
    memset(oa, 0, sizeof(*oa));
    dev_dyn_valid = false;
    if (!device_advance || C <= (uint32_t)kOscInline) return 0;
    if (!d_adv) PG_TRY(d_adv.alloc(C));
    if (adv_stale || adv_n != n) {  // (rare: a retune or another call length)
        std::vector<double> a(C);
        for (uint32_t ch = 0; ch < C; ch++) {
            long double p = (long double)n * (long double)ctl[ch].inc;
            p -= floorl(p);
            a[ch] = (double)p;
        }
        PG_HIP(hipMemcpyAsync(d_adv, a.data(), sizeof(double) * C, hipMemcpyHostToDevice, s));
        PG_HIP(hipStreamSynchronize(s));
        adv_n = n;
        adv_stale = false;
    }
    oa->osc = d_osc;
    oa->adv = d_adv;
    oa->adv_n = (uint32_t)(n > 0xffffffffull ? 0xffffffffull : n);
    oa->osc_count = C;
    dev_dyn_valid = true;
    return 0;
}
bool OscBank::any_transient() const
{
    for (const auto &c : ctl)
        if (c.n0 < (uint64_t)kAmpTab) return true;
    return false;
}
void OscBank::advance(uint64_t n)
{
    for (auto &c : ctl) {
        long double p = (long double)c.phase0 + (long double)n * (long double)c.inc;
        p -= floorl(p);
        c.phase0 = (double)p;
        if (c.phase0 >= 1.0) c.phase0 = 0.0;
        c.n0 += n;
    }
}

int run_normalize_iq(int fmt, int order, double gain, const void *d_src, long long n, float2 *d_dst, hipStream_t s, bool wait, const float *final_scale)
{
    // (a final_scale: the caller has already folded the format's constant in, a gain of 0 included)
    const float scale = final_scale != nullptr ? *final_scale : raw_scale(fmt, gain);
    long long blocks = (n + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    launch(k_normalize_iq, dim3((unsigned)blocks), dim3(256), s, d_src, d_dst, n, fmt, order, scale);
    PG_HIP(hipGetLastError());
    if (wait) PG_HIP(hipStreamSynchronize(s));
    return 0;
}

// ---- IngestRing (ingest.h) ----
int IngestRing::acquire(int device, uint32_t s, uint64_t bytes, void **host_ptr)
{
    if (s > 1 || !host_ptr || bytes == 0) return fail(PEBBLEGPU_E_INVALID, "ingest slot is 0 or 1, bytes > 0");
    PG_HIP(hipSetDevice(device));
    IngestSlot &g = slot[s];
    if (g.in_flight) {  // the call that read this slot's device copy (and the upload before it) must be over before the host refills it
        PG_HIP(hipEventSynchronize(g.done_main));
        PG_HIP(hipEventSynchronize(g.done_chain));
        g.in_flight = false;
    }
    if (!copy_stream) PG_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    if (!g.uploaded) {
        PG_HIP(hipEventCreateWithFlags(&g.uploaded, hipEventDisableTiming));
        PG_HIP(hipEventCreateWithFlags(&g.done_main, hipEventDisableTiming));
        PG_HIP(hipEventCreateWithFlags(&g.done_chain, hipEventDisableTiming));
    }
    if (g.cap < bytes) {
        PG_HIP(hipStreamSynchronize(copy_stream));
        g.cap = 0;
        PG_TRY(g.h.alloc(bytes));
        PG_TRY(g.d.alloc(bytes));
        g.cap = bytes;
    }
    g.submitted = 0;
    *host_ptr = g.h;
    return 0;
}
int IngestRing::submit(int device, uint32_t s, uint64_t bytes)
{
    if (s > 1) return fail(PEBBLEGPU_E_INVALID, "ingest slot is 0 or 1");
    IngestSlot &g = slot[s];
    if (!g.h || bytes == 0 || bytes > g.cap) return fail(PEBBLEGPU_E_SIZE, "%llu bytes do not fit the slot acquired (%zu)", (unsigned long long)bytes, g.cap);
    if (g.in_flight) return fail(PEBBLEGPU_E_INVALID, "the slot's previous call is still in flight: acquire it again first");
    PG_HIP(hipSetDevice(device));
    PG_HIP(hipMemcpyAsync(g.d, g.h, bytes, hipMemcpyHostToDevice, copy_stream));
    PG_HIP(hipEventRecord(g.uploaded, copy_stream));
    g.submitted = bytes;
    return 0;
}
int IngestRing::check(uint32_t s, int fmt, uint64_t pairs, uint64_t n_for_message, IngestSlot **out)
{
    if (s > 1) return fail(PEBBLEGPU_E_INVALID, "ingest slot is 0 or 1");
    IngestSlot &g = slot[s];
    if (fmt < 0 || fmt > 4) return fail(PEBBLEGPU_E_INVALID, "unknown sample format %d", fmt);
    if (!g.submitted || pairs * kRawPairBytes[fmt] > g.submitted)
        return fail(PEBBLEGPU_E_SIZE, "the slot holds %zu submitted bytes; %llu samples of this format need more", g.submitted, (unsigned long long)n_for_message);
    *out = &g;
    return 0;
}
int IngestRing::wait_upload(IngestSlot &g, hipStream_t main, hipStream_t chain)
{
    PG_HIP(hipStreamWaitEvent(main, g.uploaded, 0));
    PG_HIP(hipStreamWaitEvent(chain, g.uploaded, 0));
    return 0;
}
int IngestRing::mark_in_flight(IngestSlot &g, hipStream_t main, hipStream_t chain)
{
    PG_HIP(hipEventRecord(g.done_main, main));
    PG_HIP(hipEventRecord(g.done_chain, chain));
    g.in_flight = true;
    return 0;
}
int IngestRing::wait_free(uint32_t s)
{
    if (s > 1) return fail(PEBBLEGPU_E_INVALID, "ingest slot is 0 or 1");
    IngestSlot &g = slot[s];
    if (g.in_flight) {
        PG_HIP(hipEventSynchronize(g.done_main));
        PG_HIP(hipEventSynchronize(g.done_chain));
        g.in_flight = false;
    }
    if (copy_stream) PG_HIP(hipStreamSynchronize(copy_stream));  // (an upload nobody processed: the host buffer is about to be refilled)
    g.submitted = 0;
    return 0;
}
int IngestRing::submit_from(int device, uint32_t s, const void *h_src, uint64_t bytes)
{
    if (s > 1 || !h_src || bytes == 0) return fail(PEBBLEGPU_E_INVALID, "ingest slot is 0 or 1, a host buffer, bytes > 0");
    IngestSlot &g = slot[s];
    if (g.in_flight) return fail(PEBBLEGPU_E_INVALID, "the slot's previous call is still in flight: acquire it again first");
    PG_HIP(hipSetDevice(device));
    if (!copy_stream) PG_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    if (!g.uploaded) {
        PG_HIP(hipEventCreateWithFlags(&g.uploaded, hipEventDisableTiming));
        PG_HIP(hipEventCreateWithFlags(&g.done_main, hipEventDisableTiming));
        PG_HIP(hipEventCreateWithFlags(&g.done_chain, hipEventDisableTiming));
    }
    if (g.cap < bytes) {
        PG_HIP(hipStreamSynchronize(copy_stream));
        g.cap = 0;
        PG_TRY(g.d.alloc(bytes));
        g.cap = bytes;
    }
    PG_HIP(hipMemcpyAsync(g.d, h_src, bytes, hipMemcpyHostToDevice, copy_stream));
    PG_HIP(hipEventRecord(g.uploaded, copy_stream));
    g.submitted = bytes;
    return 0;
}
void IngestRing::release()
{
    if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); }
    copy_stream = nullptr;
    for (IngestSlot &g : slot) {
        for (hipEvent_t e : {g.uploaded, g.done_main, g.done_chain}) if (e) (void)hipEventDestroy(e);
        g = IngestSlot();
    }
}

// streaming-copy probe: the chip's practical HBM ceiling next to which the kernels are priced
int probe_copy(int lane_bytes, size_t bytes, int iters, float *gbps)
{
    hipStream_t s;
    hipEvent_t e0, e1;
    DevBuf<unsigned char> a, b;
    PG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    PG_HIP(hipEventCreate(&e0));
    PG_HIP(hipEventCreate(&e1));
    PG_TRY(a.alloc(bytes));
    PG_TRY(b.alloc(bytes));
    PG_HIP(hipMemsetAsync(a, 1, bytes, s));
    const dim3 grid(256 * 8), block(256);
    for (int it = -1; it < iters; it++) {
        if (it == 0) PG_HIP(hipEventRecord(e0, s));
        if (lane_bytes == 16) launch(k_probe_copy16, grid, block, s, (const float4 *)a.get(), (float4 *)b.get(), (long long)(bytes / 16));
        else launch(k_probe_copy8, grid, block, s, (const float2 *)a.get(), (float2 *)b.get(), (long long)(bytes / 8));
    }
    PG_HIP(hipEventRecord(e1, s));
    PG_HIP(hipEventSynchronize(e1));
    float ms = 0;
    PG_HIP(hipEventElapsedTime(&ms, e0, e1));
    *gbps = (float)(2.0 * (double)bytes * iters / (ms * 1e-3) / 1e9);  // read + write
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(s);
    return 0;
}

// stand-alone mixer launch (Mixer::processBlock), used by the Mixer step
int run_mixer(hipStream_t s, const float2 *d_in, float2 *d_out, long long n, const OscBank &osc)
{
    launch(k_mixer, dim3(cdiv(n, 1024), osc.C), dim3(256), s, d_in, n, 0, d_out, n, n, (const ChanOsc *)osc.d_osc,
           (const float *)osc.d_amp, osc.a_inf, osc.inline_dyn);
    PG_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// DecimCore: k_mix_dec1 (mixer + first merged stage) -> buf0 -> k_cascade (every later stage, fused) -> final
// ------------------------------------------------------------------------------------------------
static size_t mixdec_lds_bytes(const FirTaps &t)
{
    const int H = t.cic3 ? t.stride : t.ntaps - 1;
    const int span = 256 * t.stride + H;
    return (size_t)(span + span / t.stride + 2) * sizeof(float2);
}

// ---- k_mix_dec_mfma's instantiations: one per entry of PG_BANK_DEC_INSTANCES (decim_route.h), in the list's order ----
struct BankVariant {
    int np, t1, t2, t3;
    void *kern;
};
template <int NP, int T1, int T2, int T3, int MINW>
static BankVariant bank_variant_of()
{
    return BankVariant{NP, T1, T2, T3, (void *)k_mix_dec_mfma<NP, T1, T2, T3, 0, MINW>};
}
static const std::vector<BankVariant> &bank_variants()
{
#define PG_X(NP, T1, T2, T3, MINW) bank_variant_of<NP, T1, T2, T3, MINW>(),
    static const std::vector<BankVariant> v = {PG_BANK_DEC_INSTANCES(PG_X)};
#undef PG_X
    return v;
}
static void *bank_kernel(const DecimShape &s)
{
    for (const BankVariant &b : bank_variants())
        if (b.np == s.bank_np && b.t1 == s.casc_ntaps[0] && b.t2 == s.casc_ntaps[1] && b.t3 == s.casc_ntaps[2]) return b.kern;
    return nullptr;
}

template <int NP>
static int launch_bank(void *kern, unsigned n_wg, hipStream_t s, const float2 *d_in, float2 *out, const ChanOsc *osc, const OscDynInline &dyn, const float2 *xh,
                       float2 *xh_out, const float2 *y0h, float2 *y0s, float2 *mixed, const BankDecParams<NP> &bp, hipEvent_t stop = nullptr)
{
    using K = void (*)(const float2 *, float2 *, const ChanOsc *, OscDynInline, const float2 *, float2 *, const float2 *, float2 *, float2 *, BankDecParams<NP>);
    // stop: an event that completes with THIS dispatch (the packet's own completion signal) -- recorded afterwards it would be a packet
    // of its own in the queue, ~6 us of idle GPU in front of the next call's decimator
    if (stop) hipExtLaunchKernelGGL(reinterpret_cast<K>(kern), dim3(n_wg), dim3(256), 0, s, nullptr, stop, 0, d_in, out, osc, dyn, xh, xh_out, y0h, y0s, mixed, bp);
    else launch(reinterpret_cast<K>(kern), dim3(n_wg), dim3(256), s, d_in, out, osc, dyn, xh, xh_out, y0h, y0s, mixed, bp);
    PG_HIP(hipGetLastError());
    return 0;
}

// the call's decimator as one launch of k_mix_dec_mfma (the caller has checked the sizes)
int DecimCore::run_bank_mfma(hipStream_t s, const float2 *d_in, long long n, const OscBank &osc, const OscAdvance *oa, hipEvent_t done_event, DecimDone *done)
{
    const bool cic = fused_front;
    const HistBuf &y0b = y0_buf();
    void *kern = bank_kernel(*this);
    if (!kern) return fail(PEBBLEGPU_E_UNSUPPORTED, "no k_mix_dec_mfma instance for this chain");
    const long long g32 = cdiv(C, 32);
    const int warm = (fused_hy - 8) / 8;
    const bool had_state = st.bank_state_valid;  // the previous call took this route: the halfbands' running sums are handed over
    // The first-stage outputs in front of the call's start (block 0 needs seven of them even with the running sums handed over; the whole
    // look-back without): from the stage-0 head-room when the previous call took another route, else straight from what the previous
    // launch staged (two staging buffers, written alternately: this launch's history waves write the other one)
    const float2 *y0_hist = st.y0_pending ? (const float2 *)(d_y0stage2[st.y0_cur] + fused_hy) : (const float2 *)y0b.data();
    const long long y0_hist_pitch = st.y0_pending ? (long long)fused_hy : y0b.pitch;
    // the oscillators' advance rides on the launch when the caller handed it over (banks whose oscillators live on the device)
    const bool adv = tun.bank_osc_adv != 0 && oa != nullptr && oa->osc != nullptr && oa->osc_count == C;
    if (adv && !d_dyn[0]) {
        for (int i = 0; i < 2; i++) PG_TRY(d_dyn[i].alloc(C));
    }
    if (osc.dyn_epoch != st.dyn_epoch_seen) st.dyn_valid = false;
    st.dyn_epoch_seen = osc.dyn_epoch;
    // waves per SIMD, outputs per chunk, chunk pairs and workgroups: bank_geom.h
    const BankGeom geo = bank_geometry(len_out, C, cic, warm, bank_minw, fin2.base != nullptr, tun.bank_waves, tun.fused_l, tun.bank_hsplit);
    const long long L = geo.L;
    const int S0 = first.stride, Sfs = cic ? S0 * wide_stride : S0;  // input samples per first-stage (hb11) output
    const int hist_split = tun.bank_hsplit;
    const unsigned n_wg = geo.n_wg;
    if (tun.bank_clk) PG_TRY(d_clk.grow(s, (size_t)n_wg * 16));
    if (tun.bank_clk) PG_HIP(hipMemsetAsync(d_clk, 0, sizeof(unsigned long long) * n_wg * 16, s));
    auto common = [&](auto &bp) {
        bp.n_out = len_out;
        bp.out_pitch = fin.pitch;
        bp.y0_pitch = y0_hist_pitch;
        bp.n_in = n;
        bp.S = Sfs;
        bp.L = (int)L;
        bp.n_chan = (int)C;
        bp.n_chunks = (int)cdiv(len_out, L);
        bp.n_groups = (int)g32;
        bp.hist_pitch = kMaxTaps;
        bp.xh = xh_depth;
        bp.a_inf = osc.a_inf;
        bp.gain = casc.gain;  // (the first stage's own gain is 1 in a chain of several stages)
        bp.hist_split = hist_split;
        bp.cic_s0 = cic ? S0 : 0;
        bp.state_in = had_state ? d_bank_state[st.bank_state_parity] : nullptr;
        bp.state_out = d_bank_state[st.bank_state_parity ^ 1];
        bp.clk = tun.bank_clk ? d_clk : nullptr;
        bp.dyn_in = adv && st.dyn_valid ? d_dyn[st.dyn_parity] : nullptr;
        bp.dyn_out = adv ? d_dyn[st.dyn_parity ^ 1] : nullptr;
        bp.osc_rw = adv ? oa->osc : nullptr;
        bp.adv = adv ? oa->adv : nullptr;
        bp.adv_n = adv ? oa->adv_n : 0;
    };
    const float2 *xh = d_xhist[st.hist_parity];
    float2 *xh_out = d_xhist[st.hist_parity ^ 1], *mixed = d_hist_mixed[st.hist_parity ^ 1];
    if (!cic) {
        BankDecParams<4> bp;
        memset(&bp, 0, sizeof(bp));
        common(bp);
        bp.min_off = -10;
        bp.max_off = 0;
        bp.ctr1 = -4.0;  // the hb11's centre tap sits on sample S j - 5; the oscillator of sample i is e^{j 2 pi (phase0 + (i + 1) inc)}
        static const int kE[4] = {0, 1, 3, 5};
        for (int p = 0; p < 4; p++) {
            bp.oa[p] = -5 + kE[p];
            bp.ob[p] = -5 - kE[p];
            bp.e[p] = (float)kE[p];
            bp.g[p] = p == 0 ? 0.5f * bank_taps.h[5] : bank_taps.h[5 + kE[p]];
        }
        if (int rc = launch_bank<4>(kern, n_wg, s, d_in, fin.data(), (const ChanOsc *)osc.d_osc, osc.inline_dyn, xh, xh_out, y0_hist, d_y0stage2[st.y0_cur ^ 1], mixed, bp, done_event)) return rc;
    } else {
        // CIC3 at stride S0 in the reference's merged form (decimator.cpp:719-737: output k = .125 (od_k + ev_{k-1} + 3 (od_{k-1} + ev_k)) of the
        // sample pairs (ev, od)_P = x[S0 P], x[S0 P + 1]) under the hb11 at stride 16: relative to sample S j, pair q = -11 .. 0 carries
        // We[q] = (3 h[q+10] + h[q+11]) / 8 on its even and Wo[q] = (h[q+10] + 3 h[q+11]) / 8 on its odd sample; the response is symmetric about
        // (-11 S0 + 1) / 2 (We[q] = Wo[-11-q]), which makes twelve (later, earlier) sample pairs with one weight each
        BankDecParams<12> bp;
        memset(&bp, 0, sizeof(bp));
        common(bp);
        bp.min_off = -11 * S0;
        bp.max_off = 1;
        bp.ctr1 = 0.5 * (-11.0 * S0 + 1.0) + 1.0;
        auto h = [&](int d) { return d >= 0 && d <= 10 ? wide_fir.h[d] : 0.f; };
        for (int i = 0; i < 6; i++) {
            const int q = -11 + i;
            bp.oa[2 * i] = S0 * (-11 - q) + 1;  bp.ob[2 * i] = S0 * q;          bp.g[2 * i] = (3.f * h(q + 10) + h(q + 11)) * 0.125f;
            bp.oa[2 * i + 1] = S0 * (-11 - q);  bp.ob[2 * i + 1] = S0 * q + 1;  bp.g[2 * i + 1] = (h(q + 10) + 3.f * h(q + 11)) * 0.125f;
        }
        for (int p = 0; p < 12; p++) bp.e[p] = 0.5f * (float)(bp.oa[p] - bp.ob[p]);
        if (int rc = launch_bank<12>(kern, n_wg, s, d_in, fin.data(), (const ChanOsc *)osc.d_osc, osc.inline_dyn, xh, xh_out, y0_hist, d_y0stage2[st.y0_cur ^ 1], mixed, bp, done_event)) return rc;
    }
    done->done_recorded = done_event != nullptr;
    if (tun.bank_clk) { if (int rc = report_clk(s, n_wg, L)) return rc; }
    st.hist_parity ^= 1;
    st.bank_state_parity ^= 1;
    st.bank_state_valid = true;
    st.y0_cur ^= 1;
    st.y0_pending = true;
    // (with dyn_in the launch advanced the device blocks too; without, the caller's tail launch does and the next call finds dyn_out current)
    done->osc_advanced = adv && st.dyn_valid;
    if (adv) st.dyn_parity ^= 1;
    st.dyn_valid = adv;
    return 0;
}

// Tuning::bank_clk: the clock counts k_mix_dec_mfma's waves left in d_clk (four per wave: shader clocks, 100 MHz ticks, blocks, pair)
int DecimCore::report_clk(hipStream_t s, unsigned n_wg, long long L)
{
    std::vector<unsigned long long> h((size_t)n_wg * 16);
    PG_HIP(hipStreamSynchronize(s));
    PG_HIP(hipMemcpy(h.data(), d_clk, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    std::vector<double> per, ghz;
    std::vector<std::pair<double, size_t>> slow;
    double mx = 0;
    for (size_t w = 0; w < (size_t)n_wg * 4; w++)
        if (h[4 * w + 2]) {
            per.push_back((double)h[4 * w] / (double)h[4 * w + 2]);
            ghz.push_back((double)h[4 * w] / ((double)h[4 * w + 1] * 10.0));
            slow.push_back({per.back(), w});
            if ((double)h[4 * w + 1] > mx) mx = (double)h[4 * w + 1];
        }
    std::sort(per.begin(), per.end());
    std::sort(ghz.begin(), ghz.end());
    std::sort(slow.begin(), slow.end());
    if (!per.empty()) {
        fprintf(stderr, "k_mix_dec_mfma: %zu waves, L %d, clocks per block min %.0f median %.0f max %.0f; shader clock median %.2f GHz; longest wave %.1f us\n", per.size(),
                (int)L, per.front(), per[per.size() / 2], per.back(), ghz[ghz.size() / 2], mx / 100.0);
        fprintf(stderr, "   slowest (clocks per block : workgroup.wave pair):");
        for (size_t i = slow.size() > 12 ? slow.size() - 12 : 0; i < slow.size(); i++)
            fprintf(stderr, " %.0f:%zu.%zu p%llu", slow[i].first, slow[i].second / 4, slow[i].second % 4, h[4 * slow[i].second + 3]);
        size_t over = 0;
        for (double v : per) over += v > 1.25 * per[per.size() / 2];
        fprintf(stderr, "\n   waves more than 25 %% over the median: %zu\n", over);
        fprintf(stderr, "   workgroups with a wave more than 8 %% over the median:");
        size_t last = (size_t)-1;
        for (size_t w = 0; w < (size_t)n_wg * 4; w++)
            if (h[4 * w + 2] && (double)h[4 * w] / (double)h[4 * w + 2] > 1.08 * per[per.size() / 2] && w / 4 != last) {
                fprintf(stderr, " %zu", w / 4);
                last = w / 4;
            }
        fprintf(stderr, "\n");
    }
    return 0;
}

// The first-stage history a k_mix_dec_mfma launch staged (d_y0stage) into the stage-0 head-room, where the other routes and a launch
// without the halfbands' running sums look for it.  Not needed between two such launches: queued only when a call wants it.
int DecimCore::flush_y0(hipStream_t s)
{
    if (!st.y0_pending) return 0;
    const HistBuf &y0b = y0_buf();
    std::vector<TailJob> jobs;
    jobs.push_back(TailJob{d_y0stage2[st.y0_cur], (long long)fused_hy, (long long)fused_hy, fused_hy, 0, y0b.base + (y0b.hist - fused_hy), y0b.pitch});
    st.y0_pending = false;
    return run_save_tails(s, jobs, C, nullptr);
}

int DecimCore::init(uint32_t channels, const design::Chain &c, long long max_in, int last_hist, float last_gain, const Tuning &t)
{
    release();
    tun = t;
    chain = c;
    const size_t ns = chain.stages.size();
    if (ns > (size_t)kMaxCascade + 1) return fail(PEBBLEGPU_E_UNSUPPORTED, "decimation chain has %zu stages; at most %d are built", ns, kMaxCascade + 1);
    DecimStageDesc sd[kMaxCascade + 1];
    for (size_t k = 0; k < ns; k++) sd[k] = DecimStageDesc{chain.stages[k].ntaps, (int)chain.stages[k].stride};
    DecimTuningFacts tf;
    tf.no_fused_dec = tun.no_fused_dec;
    tf.bank_dec = tun.bank_dec != 0;
    static_cast<DecimShape &>(*this) = plan_decim_shape(sd, (int)ns, channels, tf);
    if (total != (long long)chain.total) return fail(PEBBLEGPU_E_INVALID, "the chain's decimation %u is not the product of its strides %lld", chain.total, total);
    memset(&first, 0, sizeof(first));
    memset(&casc, 0, sizeof(casc));
    first.stride = first_stride;
    first.gain = ns <= 1 ? last_gain : 1.f;
    if (zero_stage) {
        // "No decimation, just return" (decimator.cpp:155-160): the mixer alone, into the row the consumer reads (its look-back in front)
        ovl_len = last_hist;
        return buf0.alloc((int)C, last_hist, max_in);
    }
    const design::Stage &s0 = chain.stages[0];
    first.ntaps = s0.ntaps;
    first.cic3 = first_cic3;
    for (int p = 0; p < s0.ntaps; p++) first.h[p] = (float)design::halfband_taps(s0.design)[p];
    if (mixdec_lds_bytes(first) > 150 * 1024) return fail(PEBBLEGPU_E_UNSUPPORTED, "first-stage stride %u too wide for the LDS tile", s0.stride);
    memset(&bank_taps, 0, sizeof(bank_taps));
    bank_taps.stride = first.stride;
    for (int p = 0; p < kFrontT1 && p < first.ntaps; p++) bank_taps.h[p] = first.h[p];
    if (wide) {  // a wide second stage is peeled off the fused cascade (see DecimShape)
        const design::Stage &w = chain.stages[1];
        std::vector<float> wt(kMaxTaps, 0.f);
        for (int p = 0; p < w.ntaps; p++) wt[p] = (float)design::halfband_taps(w.design)[p];
        PG_TRY(d_wide_taps.upload(wt.data(), kMaxTaps));
        memset(&wide_fir, 0, sizeof(wide_fir));
        wide_fir.stride = (int)w.stride;
        for (int p = 0; p < w.ntaps && p < kFrontT1; p++) wide_fir.h[p] = wt[p];
    }
    // the fused later stages
    casc.nst = nst;
    casc.gain = last_gain;
    casc.outb = outb;
    casc.lds_half = lds_half;
    for (int k = 0; k < nst; k++) {
        const design::Stage &stg = chain.stages[ns - nst + k];
        casc.ntaps[k] = stg.ntaps;
        casc.stride[k] = (int)stg.stride;
        for (int p = 0; p < stg.ntaps; p++) casc.h[k][p] = (float)design::halfband_taps(stg.design)[p];
    }
    if (casc_lds_bytes > 150 * 1024) return fail(PEBBLEGPU_E_UNSUPPORTED, "decimation cascade does not fit LDS");
    if (one_kernel()) {  // the histories of the one-kernel routes (DecimShape::fused_all, bank_mfma)
        if (fused_all) {
            fused_p = new FusedDecParams();
            memset(fused_p, 0, sizeof(*fused_p));
            fused_p->S = first.stride;
            fused_p->n_chan = (int)C;
            fused_p->hist_pitch = kMaxTaps;
            fused_p->gain0 = first.gain;
            fused_p->gain = casc.gain;
        }
        for (int i = 0; i < 2; i++) PG_TRY(d_xhist[i].alloc_zero(xh_depth));
        for (int i = 0; i < 2; i++) PG_TRY(d_y0stage2[i].alloc_zero((size_t)fused_hy * C + 64));  // (64 entries of slack: the kernel requests a block ahead of what it uses)
        d_y0stage = d_y0stage2[0];
        if (bank_mfma) {
            for (int i = 0; i < 2; i++) PG_TRY(d_bank_state[i].alloc_zero((size_t)bank_nstate * C));
        }
    }
    const long long len0 = max_in / s0.stride;
    if (ns == 1) {
        if (int rc = buf0.alloc((int)C, last_hist, len0)) return rc;
    } else {
        if (halo0 > 256 * 32) return fail(PEBBLEGPU_E_UNSUPPORTED, "cascade look-back %lld too deep", halo0);
        if (wide) {
            if (!fused_front) { if (int rc = buf0.alloc((int)C, wide_taps - 1, len0)) return rc; }
            if (int rc = buf1.alloc((int)C, (int)halo0, len0 / wide_stride)) return rc;
            if (int rc = fin.alloc((int)C, last_hist, len0 / wide_stride / later)) return rc;
        } else {
            if (int rc = buf0.alloc((int)C, (int)halo0, len0)) return rc;
            if (int rc = fin.alloc((int)C, last_hist, len0 / later)) return rc;
        }
    }
    for (int i = 0; i < 2; i++) {
        PG_TRY(d_hist_mixed[i].alloc_zero((size_t)kMaxTaps * C));
        if (C == 1) PG_TRY(d_xtail_w[i].alloc_zero(2048));
    }
    return 0;
}
// everything init() derived and every field one call hands to the next go back to their defaults with the buffers
void DecimCore::release()
{
    delete fused_p;
    fused_p = nullptr;
    static_cast<DecimShape &>(*this) = DecimShape{};
    st = Carried{};
    d_y0stage = nullptr;
    for (int i = 0; i < 2; i++) {
        d_ovl[i].release();
        d_xhist[i].release();
        d_y0stage2[i].release();
        d_bank_state[i].release();
        d_dyn[i].release();
        d_hist_mixed[i].release();
        d_xtail_w[i].release();
    }
    for (HistBuf *b : {&buf0, &buf1, &fin, &fin2, &fin3}) b->release();
    d_wide_taps.release();
    d_c0tab.release();
    d_ph_scratch.release();
    d_clk.release();
}
int DecimCore::set_fuse_window(const float *d_window, const std::vector<float> &w)
{
    fuse_window = nullptr;
    if (C != 1 || w.size() != 2048 || !bank_front) return 0;
    static const int kD[7] = {0, 2, 4, 5, 6, 8, 10};
    std::vector<float> t(7 * 256);
    for (int i = 0; i < 7; i++)
        for (int jf = 0; jf < 256; jf++) t[256 * i + jf] = bank_taps.h[kD[i]] / w[(8 * jf - 10 + kD[i]) & 2047];
    h_r0 = t;
    h_c0.assign(t.size(), make_float2(0.f, 0.f));
    c0_valid = false;
    if (!d_c0tab) PG_TRY(d_c0tab.alloc(t.size()));
    fuse_window = d_window;
    return 0;
}
bool DecimCore::shape_for_spectrum() const
{
    return C == 1 && bank_front && !fused_all && !fused_front && !wide && first.stride == 8 && casc.nst == 3 && casc.stride[0] == 2 && casc.stride[1] == 2 &&
           casc.stride[2] == 2 && casc.ntaps[0] == 15 && casc.ntaps[1] == 23 && casc.ntaps[2] == 47 && buf0.hist <= 256 && d_xtail_w[0] != nullptr && d_c0tab != nullptr;
}
int DecimCore::fill_dec_fuse(hipStream_t s, DecFuse *df, const OscBank &osc, long long n)
{
    if (n <= 0 || n % 2048 != 0) return fail(PEBBLEGPU_E_SIZE, "%lld samples is not a whole number of 2048-sample frames", n);
    len0 = n / first.stride;
    len_out = n / (long long)chain.total;
    if (len0 > buf0.cap) return fail(PEBBLEGPU_E_SIZE, "%lld samples exceed this object's capacity", n);
    memset(df, 0, sizeof(*df));
    df->y = fin.data();
    df->y0_tail = buf0.data() + (len0 - 256);
    df->xtail = d_xtail_w[st.xtail_parity];
    df->xtail_next = d_xtail_w[st.xtail_parity ^ 1];
    const ChanOsc &o = osc.h_osc[0];
    df->phase0 = osc.inline_dyn.use ? osc.inline_dyn.d[0].phase0 : osc.ctl[0].phase0;
    df->inc = o.inc;
    df->a_inf = osc.a_inf;
    df->gain0 = first.gain;
    df->gain_last = casc.gain;
    df->mix_on = (int)o.mix_on;
    if (!c0_valid || c0_inc != o.inc || c0_mix != (int)o.mix_on) {
        // (rare: the first such call and the first after a retune.)  The copy is queued on the call's main stream, which follows
        // everything earlier calls queued on either stream, and waited for: the host table is free to change afterwards
        static const int kD[7] = {0, 2, 4, 5, 6, 8, 10};
        for (int i = 0; i < 7; i++)
            for (int jf = 0; jf < 256; jf++) {
                const float r = h_r0[256 * i + jf];
                const float2 st = o.mix_on ? o.step[kD[i]] : make_float2(1.f, 0.f);
                h_c0[256 * i + jf] = make_float2(r * st.x, r * st.y);
            }
        PG_HIP(hipMemcpyAsync(d_c0tab, h_c0.data(), sizeof(float2) * h_c0.size(), hipMemcpyHostToDevice, s));
        PG_HIP(hipStreamSynchronize(s));
        c0_valid = true;
        c0_inc = o.inc;
        c0_mix = (int)o.mix_on;
    }
    {
        double ph = 2048.0 * o.inc;
        ph -= std::floor(ph);
        df->wfr = make_float2((float)std::cos(design::kTwoPi * ph), (float)std::sin(design::kTwoPi * ph));
    }
    df->c0tab = d_c0tab;
    {
        // one 2 KiB row per frame chain of the transform's launch (chains of at most 32 frames, at least 512 of them)
        PG_TRY(d_ph_scratch.grow(s, (size_t)(n / 2048 + 1024) * 256));
        df->ph_scratch = d_ph_scratch;
    }
    return 0;
}
// the call's last 2048 samples, windowed: the look-back of a later call whose decimator runs inside the display transform
static __global__ __launch_bounds__(256) void k_window_tail(const float2 *__restrict__ in, long long n, const float *__restrict__ window, float2 *__restrict__ out,
                                                            RawSrc raw)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const long long src = n - 2048 + i;
    const float2 v = raw.base ? raw_load(raw, src) : in[src];
    out[i] = cscale(v, window[i]);
}
static RawSrc raw_or_none(const RawSrc *raw) { return raw ? *raw : RawSrc{nullptr, 0, 0, 0.f, 0}; }
// LDS of the kernels plan_channel_lanes() lays out: one transposing tile per wave unless a lane holds one channel's outputs only
static size_t lanes_lds_bytes(const DecimRoute &r) { return r.cl_log2 ? 4 * (size_t)front_tile_slots(r.cl_log2, r.R) * sizeof(float2) : 0; }

// Two workgroups of the general register front beside a kernel that computes a call's inner outputs (k_mix_hb11_lean, the display
// transform): the first outputs, whose windows reach back into the mixed history, and the call's own mixed history
int DecimCore::run_edges(const Launch &l, int R)
{
    const long long j_first = (10 + first.stride - 1) / first.stride;
    launch(l.raw ? k_mix_hb11_bank<false, false, true> : k_mix_hb11_bank<false, false, false>, dim3(len0 / (4LL * R * 64) != 0 ? 2 : 1, 1), dim3(256), l.s, l.in, l.in_pitch,
           (int)l.shared_input, buf0.data(), buf0.pitch, len0, (const ChanOsc *)l.osc.d_osc, (const float2 *)d_hist_mixed[st.hist_parity], d_hist_mixed[st.hist_parity ^ 1],
           (int)kMaxTaps, (const float *)l.osc.d_amp, l.osc.a_inf, bank_taps, first.gain, l.osc.inline_dyn, 0, (int)C, R, j_first, raw_or_none(l.raw));
    return 0;
}
int DecimCore::run_beside_spectrum(hipStream_t s, const float2 *d_in, long long in_pitch, bool shared_input, long long n, const OscBank &osc, const RawSrc *raw)
{
    // (fill_dec_fuse has set the lengths.)  The general kernels keep the mixed samples of the call's end as their history: left by the
    // same two-workgroup launch that serves k_mix_hb11_lean, so the next call may take either route
    if (int rc = run_edges(Launch{s, d_in, in_pitch, shared_input, n, osc, raw}, 8)) return rc;
    PG_HIP(hipGetLastError());
    st.hist_parity ^= 1;
    st.xtail_parity ^= 1;  // the transform's last workgroup writes the next call's look-back
    st.last = DecimRoute{};
    st.last.front = DecimFront::InSpectrum;
    return 0;
}
// An empty chain whose consumer mixes: nothing to launch, the consumer reads the stream.  Its block 0 looks back at the previous call's
// mixed samples -- its own row, or the head-room a k_mixer call's tail job refreshed
int DecimCore::run_in_consumer(const DecimRoute &r)
{
    if (!mix_in_consumer_ready()) return fail(PEBBLEGPU_E_INVALID, "the consumer's overlap rows were not enabled");
    mix_tail.tail = r.ovl_from_row ? d_ovl[st.ovl_parity] : buf0.base + (buf0.hist - ovl_len);
    mix_tail.tail_pitch = r.ovl_from_row ? (long long)ovl_len : buf0.pitch;
    mix_tail.tail_out = d_ovl[st.ovl_parity ^ 1];
    st.ovl_parity ^= 1;
    return 0;
}
int DecimCore::run_mixer_only(const Launch &l, const DecimRoute &r)
{
    if (r.ovl_from_row) {  // the first k_mixer call behind calls that mixed in the band-pass: their overlap row becomes the head-room
        std::vector<TailJob> jobs;
        jobs.push_back(TailJob{d_ovl[st.ovl_parity], (long long)ovl_len, (long long)ovl_len, ovl_len, 0, buf0.base + (buf0.hist - ovl_len), buf0.pitch});
        if (int rc = run_save_tails(l.s, jobs, C, nullptr)) return rc;
    }
    launch(k_mixer, dim3(r.grid_x, r.grid_y), dim3(256), l.s, l.in, l.in_pitch, (int)l.shared_input, buf0.data(), buf0.pitch, l.n, (const ChanOsc *)l.osc.d_osc,
           (const float *)l.osc.d_amp, l.osc.a_inf, l.osc.inline_dyn);
    PG_HIP(hipGetLastError());
    return 0;
}
int DecimCore::run_fused(const Launch &l, const DecimRoute &r)
{
    long long L = tun.fused_l > 0 ? tun.fused_l : ((len_out * r.grid_y / 704 + 15) & ~15LL);  // ~700 four-wave workgroups (measured best on 256 CUs: 96 for configs[2]); every chunk pays a 21-block warm-up
    if (L < 32) L = 32;
    fused_p->n_out = len_out;
    fused_p->out_pitch = fin.pitch;
    fused_p->y0_pitch = buf0.pitch;
    fused_p->L = (int)L;
    fused_p->a_inf = l.osc.a_inf;
    launch(k_mix_dec_fused<15, 19, 31>, dim3(cdiv(len_out, L), r.grid_y), dim3(256), l.s, l.in, fin.data(), (const ChanOsc *)l.osc.d_osc, l.osc.inline_dyn,
           (const float2 *)d_xhist[st.hist_parity], d_xhist[st.hist_parity ^ 1], (const float2 *)buf0.data(), d_y0stage, d_hist_mixed[st.hist_parity ^ 1], *fused_p);
    PG_HIP(hipGetLastError());
    return 0;
}
int DecimCore::run_cic_hb(const Launch &l, const DecimRoute &r)
{
    auto kern = r.transient ? (r.uniform ? k_mix_cic_hb<true, true> : k_mix_cic_hb<true, false>) : (r.uniform ? k_mix_cic_hb<false, true> : k_mix_cic_hb<false, false>);
    launch_lds(kern, dim3(r.grid_x, r.grid_y), dim3(256), lanes_lds_bytes(r), l.s, l.in, l.in_pitch, (int)l.shared_input, buf1.data(), buf1.pitch,
               len1, (const ChanOsc *)l.osc.d_osc, (const float2 *)d_hist_mixed[st.hist_parity], d_hist_mixed[st.hist_parity ^ 1], (int)kMaxTaps,
               (const float *)l.osc.d_amp, l.osc.a_inf, wide_fir, first.stride, 1.0f, l.osc.inline_dyn, r.cl_log2, (int)C, r.R);
    return 0;
}
int DecimCore::run_lean(const Launch &l, const DecimRoute &r)
{
    const long long j_first = (10 + first.stride - 1) / first.stride;
    auto lean = r.raw_fmt < 0 ? k_mix_hb11_lean<-1> : r.raw_fmt == 0 ? k_mix_hb11_lean<0> : r.raw_fmt == 1 ? k_mix_hb11_lean<1> : r.raw_fmt == 2 ? k_mix_hb11_lean<2>
                             : r.raw_fmt == 3 ? k_mix_hb11_lean<3> : k_mix_hb11_lean<4>;
    launch(lean, dim3(r.grid_x), dim3(256), l.s, l.in, buf0.data(), len0, (const ChanOsc *)l.osc.d_osc, l.osc.a_inf, bank_taps, first.gain, l.osc.inline_dyn, r.R,
           r.edge_launch ? -j_first : j_first, raw_or_none(l.raw), (const float2 *)d_hist_mixed[st.hist_parity], d_hist_mixed[st.hist_parity ^ 1]);
    return r.edge_launch ? run_edges(l, r.R) : 0;  // (A/B: the edges as a launch of their own)
}
int DecimCore::run_hb11_bank(const Launch &l, const DecimRoute &r)
{
    auto kern = r.transient ? (r.uniform ? k_mix_hb11_bank<true, true> : k_mix_hb11_bank<true, false>)
                            : (r.uniform ? k_mix_hb11_bank<false, true> : k_mix_hb11_bank<false, false>);
    launch_lds(kern, dim3(r.grid_x, r.grid_y), dim3(256), lanes_lds_bytes(r), l.s, l.in, l.in_pitch, (int)l.shared_input, buf0.data(),
               buf0.pitch, len0, (const ChanOsc *)l.osc.d_osc, (const float2 *)d_hist_mixed[st.hist_parity], d_hist_mixed[st.hist_parity ^ 1], (int)kMaxTaps,
               (const float *)l.osc.d_amp, l.osc.a_inf, bank_taps, first.gain, l.osc.inline_dyn, r.cl_log2, (int)C, r.R, -1LL, RawSrc{nullptr, 0, 0, 0.f, 0});
    return 0;
}
int DecimCore::run_dec1(const Launch &l, const DecimRoute &r)
{
    size_t lds = mixdec_lds_bytes(first);
    if (r.cg > 1 && lds < (size_t)r.cg * 258 * sizeof(float4)) lds = (size_t)r.cg * 258 * sizeof(float4);
    launch_lds(k_mix_dec1, dim3(r.grid_x, r.grid_y), dim3(256), lds, l.s, l.in, l.in_pitch, (int)l.shared_input, buf0.data(),
               buf0.pitch, len0, (const ChanOsc *)l.osc.d_osc, (const float2 *)d_hist_mixed[st.hist_parity], (int)kMaxTaps, (const float *)l.osc.d_amp,
               l.osc.a_inf, first, d_hist_mixed[st.hist_parity ^ 1], l.osc.inline_dyn, r.cg, (int)C);  // its last block leaves the next call's mixed history
    return 0;
}
// the stages behind a general front: the peeled wide stage from buf0 into buf1, the fused cascade into fin
int DecimCore::run_rest(const Launch &l, const DecimRoute &r)
{
    if (r.fir_dec())
        launch(k_fir_dec, dim3(cdiv(len1, 256), C), dim3(256), l.s, (const float2 *)buf0.data(), buf0.pitch, buf1.data(), buf1.pitch, len1, wide_stride,
               (const float *)d_wide_taps, (const float *)nullptr, 0, (const int *)nullptr, wide_taps, 1.0f, 0, (const int *)nullptr, Gate{nullptr, 0, 0});
    if (r.cascade()) {
        const HistBuf &src = wide ? buf1 : buf0;
        // (this ladder, not a conditional expression: the compiler emits the three in the order they are first named, and so does the
        // order of the launchers in this file for every other instance -- reordering either moves the kernels inside the code object)
        auto kern = k_cascade<0, 0, 0>;
        if (r.cascade_inst == 1) kern = k_cascade<15, 23, 47>;
        else if (r.cascade_inst == 2) kern = k_cascade<15, 19, 31>;
        launch_lds(kern, dim3(r.tiles, C), dim3(256), r.cascade_inst ? casc_fixed_lds_bytes : casc_lds_bytes, l.s, (const float2 *)src.data(), src.pitch, fin.data(), fin.pitch, len_out, casc);
    }
    return 0;
}
int DecimCore::hand_over(const Launch &l)
{
    if (one_kernel() && l.shared_input && l.n >= xh_depth)  // the next call may take a one-kernel route: it wants this call's raw tail (hist_parity already flipped)
        PG_HIP(hipMemcpyAsync(d_xhist[st.hist_parity], l.in + (l.n - xh_depth), sizeof(float2) * xh_depth, hipMemcpyDeviceToDevice, l.s));
    if (fuse_window && l.n >= 2048 && shape_for_spectrum()) {  // the next call's decimator may run inside the display transform
        launch(k_window_tail, dim3(8), dim3(256), l.s, l.in, l.n, fuse_window, d_xtail_w[st.xtail_parity ^ 1], raw_or_none(l.raw));
        st.xtail_parity ^= 1;
    }
    return 0;
}
DecimCallFacts DecimCore::call_facts(const Launch &l, const DecimCall &call) const
{
    DecimCallFacts f;
    f.n = l.n;
    f.shared_input = l.shared_input;
    f.transient = l.osc.any_transient();
    f.lds_free = call.lds_free;
    f.raw_fmt = l.raw ? l.raw->fmt : -1;
    f.mix_in_consumer = call.mix_in_consumer;
    f.in_aligned = (reinterpret_cast<uintptr_t>(l.in) & 7) == 0;
    f.out_pitch = fin.pitch;
    f.lean_edge_launch = tun.lean_edge_launch;
    f.ovl_pending = st.ovl_pending;
    return f;
}
// refusals, the route (decim_route.h), its launcher, what it hands to the next call
int DecimCore::run(hipStream_t s, const float2 *d_in, long long in_pitch, bool shared_input, long long n, const OscBank &osc,
                   hipEvent_t after_first, const RawSrc *raw, const OscAdvance *oa, DecimCall call, DecimDone *done)
{
    DecimDone unread;
    if (!done) done = &unread;
    *done = DecimDone{};
    if (raw && !raw_ready(osc, call.lds_free)) return fail(PEBBLEGPU_E_INVALID, "raw-format input reached a decimator path that has no converting loads");
    if (n <= 0 || n % (long long)chain.total != 0)
        return fail(PEBBLEGPU_E_SIZE, "%lld samples is not a multiple of the decimation %u", n, chain.total);
    // (the buffer at the hb11's rate, or the only one: the first the call writes, and the one whose head-room the one-kernel routes keep)
    if (n / ((long long)first.stride * (fused_front ? wide_stride : 1)) > y0_buf().cap) return fail(PEBBLEGPU_E_SIZE, "%lld samples exceed this object's capacity", n);
    // successive calls write successive output buffers (tail_job_out carries the consumer's look-back into the next one's head-room)
    if (fin3.base && call.rotate3) { std::swap(fin, fin2); std::swap(fin2, fin3); }  // (fin, fin2, fin3) <- (fin2, fin3, fin)
    else if (fin2.base) std::swap(fin, fin2);  // (either way the call writes what was fin2, whose head-room the last call's consumer filled)
    const Launch l{s, d_in, in_pitch, shared_input, n, osc, raw};
    const DecimRoute r = plan_decim_route(*this, call_facts(l, call));
    len0 = r.len0;
    len1 = r.len1;
    len_out = r.len_out;
    if (r.front != DecimFront::BankMfma) {
        // the running sums and the oscillator fields k_mix_dec_mfma hands from call to call end here; its staged first-stage history
        // goes where every other route looks for it
        st.bank_state_valid = st.dyn_valid = false;
        if (int rc = flush_y0(s)) return rc;
    }
    int rc = 0;
    switch (r.front) {
    case DecimFront::InConsumer: rc = run_in_consumer(r); break;
    case DecimFront::Mixer: rc = run_mixer_only(l, r); break;
    case DecimFront::BankMfma: rc = run_bank_mfma(s, d_in, n, osc, oa, call.done_event, done); break;
    case DecimFront::Fused: rc = run_fused(l, r); break;
    case DecimFront::CicHb: rc = run_cic_hb(l, r); break;
    case DecimFront::Lean: rc = run_lean(l, r); break;
    case DecimFront::Hb11Bank: rc = run_hb11_bank(l, r); break;
    case DecimFront::Dec1: rc = run_dec1(l, r); break;
    case DecimFront::None: case DecimFront::InSpectrum: break;  // (never planned)
    }
    if (rc) {
        st.bank_state_valid = st.dyn_valid = false;
        return rc;
    }
    st.last = r;
    st.ovl_pending = r.ovl_pending;
    if (r.front == DecimFront::Fused || r.general()) st.hist_parity ^= 1;  // (k_mix_dec_mfma's launcher turns its own parities)
    if (after_first) PG_HIP(hipEventRecord(after_first, s));
    if (!r.general()) return 0;
    if (int rc2 = run_rest(l, r)) return rc2;
    PG_HIP(hipGetLastError());
    return hand_over(l);
}
void DecimCore::tail_jobs_dec(std::vector<TailJob> &jobs) const
{
    if (st.last.one_kernel()) {
        // the call's last first-stage outputs (staged by the kernel) become the stage-0 head-room, as if the buffer had been written
        // (behind k_mix_dec_mfma only when a later call asks for them there: flush_y0)
        const HistBuf &y0b = y0_buf();
        if (st.last.front == DecimFront::Fused) jobs.push_back(TailJob{d_y0stage, (long long)fused_hy, (long long)fused_hy, fused_hy, 0, y0b.base + (y0b.hist - fused_hy), y0b.pitch});
        return;
    }
    if (!fused_front && buf0.hist > 0 && casc.nst > 0) jobs.push_back(TailJob{buf0.data(), buf0.pitch, len0, buf0.hist, 0, nullptr, 0});
    if (wide && buf1.hist > 0) jobs.push_back(TailJob{buf1.data(), buf1.pitch, len1, buf1.hist, 0, nullptr, 0});
}
void DecimCore::tail_job_out(std::vector<TailJob> &jobs) const
{
    if (casc.nst == 0) {  // a single stage (or none: the mixer's row): its buffer is the output
        if (last_in_consumer()) return;  // (the consumer mixed in its own loads and kept its overlap itself: buf0 was not written)
        if (!fused_front && buf0.hist > 0) jobs.push_back(TailJob{buf0.data(), buf0.pitch, len0, buf0.hist, 0, nullptr, 0});
        return;
    }
    if (fin.hist <= 0) return;
    // (two output buffers: the next call writes the other one, whose head-room row starts at its base)
    if (fin2.base) jobs.push_back(TailJob{fin.data(), fin.pitch, len_out, fin.hist, 0, fin2.base, fin2.pitch});
    else jobs.push_back(TailJob{fin.data(), fin.pitch, len_out, fin.hist, 0, nullptr, 0});
}
void DecimCore::tail_jobs(std::vector<TailJob> &jobs) const
{
    tail_jobs_dec(jobs);
    tail_job_out(jobs);
}
int DecimCore::enable_mix_in_consumer()
{
    if (!zero_stage || buf0.hist <= 0) return fail(PEBBLEGPU_E_UNSUPPORTED, "only the consumer of an empty chain mixes in its own loads");
    if (d_ovl[0]) return 0;
    for (int i = 0; i < 2; i++) PG_TRY(d_ovl[i].alloc_zero((size_t)ovl_len * C));
    return 0;
}
int DecimCore::enable_double_out()
{
    if (casc.nst == 0 || !fin.base) return fail(PEBBLEGPU_E_UNSUPPORTED, "a single-stage chain has no separate output buffer to double");
    if (fin2.base) return 0;
    if (int rc = fin2.alloc(fin.chans, fin.hist, fin.cap)) return rc;
    if (tun.bank_pipe_bufs2) return 0;  // the decimator waits for the consumer of the call before the last
    return fin3.alloc(fin.chans, fin.hist, fin.cap);
}

int fill_tail_jobs(TailJobs &tj, const std::vector<TailJob> &jobs, const OscAdvance *oa)
{
    if (jobs.size() > (size_t)kMaxTailJobs) return fail(PEBBLEGPU_E_INVALID, "too many history buffers");
    memset(&tj, 0, sizeof(tj));
    tj.count = (int)jobs.size();
    if (oa != nullptr && oa->osc != nullptr) tj.oa = *oa;
    int maxh = 1;
    for (size_t i = 0; i < jobs.size(); i++) {
        tj.job[i] = jobs[i];
        if (jobs[i].hist > maxh) maxh = jobs[i].hist;
    }
    if (maxh > 256 * 32) return fail(PEBBLEGPU_E_UNSUPPORTED, "history of %d samples too deep for the tail refresh", maxh);
    return 0;
}
// one strided real-tap FIR over `channels` rows (k_fir_dec with one tap set for all rows): y[o] = sum_p in[o stride + p - (ntaps - 1)] taps[p]
int run_fir_dec(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n_out, int stride,
                const float *d_taps, int ntaps, uint32_t channels)
{
    if (n_out <= 0) return 0;
    if (ntaps < 1 || ntaps > kMaxTaps) return fail(PEBBLEGPU_E_UNSUPPORTED, "%d taps: k_fir_dec holds at most %d", ntaps, kMaxTaps);
    launch(k_fir_dec, dim3(cdiv(n_out, 256), channels), dim3(256), s, in, in_pitch, out, out_pitch, n_out, stride, d_taps, (const float *)nullptr, 0,
           (const int *)nullptr, ntaps, 1.0f, 0, (const int *)nullptr, Gate{nullptr, 0, 0});
    PG_HIP(hipGetLastError());
    return 0;
}
int run_nap(hipStream_t s, unsigned ticks_100mhz)
{
    if (ticks_100mhz == 0) return 0;
    launch(k_nap, dim3(1), dim3(64), s, ticks_100mhz);
    PG_HIP(hipGetLastError());
    return 0;
}
int run_save_tails(hipStream_t s, const std::vector<TailJob> &jobs, uint32_t channels, const OscAdvance *oa)
{
    const bool adv = oa != nullptr && oa->osc != nullptr;
    if (jobs.empty() && !adv) return 0;
    TailJobs tj;
    if (int rc = fill_tail_jobs(tj, jobs, oa)) return rc;
    launch(k_save_tails, dim3(1, channels, (unsigned)(jobs.empty() ? 1 : jobs.size())), dim3(256), s, tj);
    PG_HIP(hipGetLastError());
    return 0;
}
int run_save_tails_listed(hipStream_t s, const std::vector<TailJob> &jobs, const int *d_list, int n_list)
{
    if (jobs.empty() || n_list <= 0) return 0;
    TailJobs tj;
    if (int rc = fill_tail_jobs(tj, jobs, nullptr)) return rc;
    launch(k_save_tails_listed, dim3(1, (unsigned)n_list, (unsigned)jobs.size()), dim3(256), s, tj, d_list);
    PG_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// FastFirCore
// ------------------------------------------------------------------------------------------------
int FastFirCore::init(uint32_t channels, uint32_t fft_size, uint32_t fir_size, const Tuning &t)
{
    tun = t;
    C = channels;
    fft_n = fft_size;
    taps = fir_size;
    if (!(fft_n == 2048 || fft_n == 4096 || fft_n == 8192)) return fail(PEBBLEGPU_E_UNSUPPORTED, "FastFIR FFT size %u not built", fft_n);
    // overlap = taps-1 <= L = fft-overlap: one block back always reaches the whole overlap.  Longer filters have no reference semantics
    // (CFastFIR refills only the last L samples of m_pFFTOverlapBuf per block) and cost more than the next FFT size with the same taps
    if (taps < 2 || taps > fft_n / 2 + 1) return fail(PEBBLEGPU_E_INVALID, "FastFIR taps must be in [2, fft/2 + 1] (got %u for fft %u)", taps, fft_n);
    PG_TRY(d_H.alloc_zero((size_t)fft_n * C));
    if (fft_n == 2048) { if (int rc = make_twiddles_t128(d_tw128)) return rc; }
    return make_twiddles((int)fft_n, d_tw);
}
int FastFirCore::design(hipStream_t s, uint32_t ch, double lo, double hi, double offset, double rate, bool *ok)
{
    std::vector<std::complex<double>> H;
    *ok = design::fastfir_design(fft_n, taps, lo, hi, offset, rate, H);
    if (!*ok) return 0;
    std::vector<float2> hf(fft_n);
    for (uint32_t i = 0; i < fft_n; i++) hf[i] = make_float2((float)H[i].real(), (float)H[i].imag());
    PG_HIP(hipMemcpyAsync(d_H + (size_t)ch * fft_n, hf.data(), sizeof(float2) * fft_n, hipMemcpyHostToDevice, s));
    PG_HIP(hipStreamSynchronize(s));
    return 0;
}
// k_fastfir_t128's grid: one-dimensional with the XCD-aware order (kernels_fastfir.h) unless PEBBLEGPU_FF_XCD=0 asks for (block, channel)
struct FfGrid { dim3 grid; int nb, nchan; };
static FfGrid ff_grid(long long nb, uint32_t channels, bool xcd)
{
    const long long total = nb * (long long)channels;
    if (!xcd || total >= (1LL << 31) - 8) return FfGrid{dim3((unsigned)nb, channels), (int)nb, 0};
    return FfGrid{dim3((unsigned)(8 * ((total + 7) / 8))), (int)nb, (int)channels};
}
int FastFirCore::run(hipStream_t s, const HistBuf &in, long long n, float2 *out, long long out_pitch)
{
    const int overlap = (int)taps - 1;
    const long long L = block_len();
    if (n % L != 0) return fail(PEBBLEGPU_E_SIZE, "FastFIR input %lld is not a multiple of its block %lld", n, L);
    const dim3 grid((unsigned)(n / L), C), block(256);
    const float2 *no_tail = nullptr;
    // (twiddles from the workgroup's LDS copy here: beside a bank's decimator -- two-stage calls -- the variant that reads them through the
    // vector cache measured 0.0833 ms per configs[2] call against 0.0820; alone, in the stream bank, it is the faster one: run_ext)
    const bool tw_lds = tun.ff_twlds != 0;
    const FfGrid fg = ff_grid(n / L, C, tun.ff_xcd);
    if (fft_n == 2048 && !tw_lds) launch(k_fastfir_t128<false>, fg.grid, dim3(128), s, (const float2 *)in.data(), in.pitch, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw128, overlap, no_tail, (float2 *)nullptr, fg.nb, fg.nchan);
    else if (fft_n == 2048) launch(k_fastfir_t128<true>, fg.grid, dim3(128), s, (const float2 *)in.data(), in.pitch, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw128, overlap, no_tail, (float2 *)nullptr, fg.nb, fg.nchan);
    else if (fft_n == 4096) launch(k_fastfir<4096>, grid, block, s, (const float2 *)in.data(), in.pitch, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw, overlap, no_tail);
    else launch(k_fastfir<8192>, grid, block, s, (const float2 *)in.data(), in.pitch, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw, overlap, no_tail);
    PG_HIP(hipGetLastError());
    return 0;
}
int FastFirCore::run_mixing(hipStream_t s, const float2 *in, long long in_pitch, bool shared_input, long long n, float2 *out, long long out_pitch,
                            const OscBank &osc, const float2 *tail, long long tail_pitch, float2 *tail_out)
{
    if (!mix_ready() || !tail || !tail_out) return fail(PEBBLEGPU_E_INVALID, "the mixing band-pass is the 2048-point plan with both overlap rows");
    const int overlap = (int)taps - 1;
    const long long L = block_len();
    if (n <= 0 || n % L != 0) return fail(PEBBLEGPU_E_SIZE, "FastFIR input %lld is not a multiple of its block %lld", n, L);
    const FfGrid fg = ff_grid(n / L, C, tun.ff_xcd);
    launch(k_fastfir_t128_mix, fg.grid, dim3(128), s, in, in_pitch, (int)shared_input, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw128, overlap, tail,
           tail_pitch, tail_out, fg.nb, fg.nchan, (const ChanOsc *)osc.d_osc, (const float *)osc.d_amp, osc.a_inf, osc.inline_dyn);
    PG_HIP(hipGetLastError());
    return 0;
}
int FastFirCore::run_ext(hipStream_t s, const float2 *in, long long in_pitch, float2 *d_tail, long long n, float2 *out, long long out_pitch, float2 *d_tail_next, const RawSrc *raw)
{
    if (raw && !(raw_ready() && d_tail && d_tail_next)) return fail(PEBBLEGPU_E_INVALID, "raw-format input reached a band-pass kernel that has no converting loads");
    const int overlap = (int)taps - 1;
    const long long L = block_len();
    if (n % L != 0) return fail(PEBBLEGPU_E_SIZE, "FastFIR input %lld is not a multiple of its block %lld", n, L);
    if (n == 0) return 0;
    // (init: overlap <= L <= n, so only block 0 reaches in front of its row -- served from d_tail -- and the row holds a whole overlap for the next call)
    const dim3 grid((unsigned)(n / L), C), block(256);
    const float2 *tail = d_tail;
    if (fft_n == 2048) {
        const size_t pad = tun.ff_padlds;  // A/B: extra LDS per workgroup (lowers its occupancy)
        // twiddles through the vector cache: without the 4.5 KB copy per workgroup eight workgroups fit a CU's LDS instead of six -- configs[4]'s
        // band-pass 0.222 / 0.227 -> 0.215 / 0.211 ms in alternating runs (PEBBLEGPU_FF_TWLDS=1 brings the copy back)
        const bool twg = tun.ff_twlds != 1;
        const FfGrid fg = ff_grid(n / L, C, tun.ff_xcd);
        if (raw) {  // the stream bank's raw calls: converted in the loads (twiddles through the vector cache, as the float2 default below)
            auto go = [&](auto kern) { launch_lds(kern, fg.grid, dim3(128), pad, s, in_pitch, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw128, overlap, tail, d_tail_next, fg.nb, fg.nchan, *raw); };
            with_raw_fmt(raw->fmt, [&](auto F) { go(k_fastfir_t128_raw<F.value>); });
        }
        else if (twg) launch_lds(k_fastfir_t128<false>, fg.grid, dim3(128), pad, s, in, in_pitch, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw128, overlap, tail, d_tail_next, fg.nb, fg.nchan);
        else launch_lds(k_fastfir_t128<true>, fg.grid, dim3(128), pad, s, in, in_pitch, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw128, overlap, tail, d_tail_next, fg.nb, fg.nchan);
        if (d_tail_next) {  // the kernel's last block has written the next call's overlap into the caller's other buffer
            PG_HIP(hipGetLastError());
            return 0;
        }
    }
    else if (fft_n == 4096) launch(k_fastfir<4096>, grid, block, s, in, in_pitch, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw, overlap, tail);
    else launch(k_fastfir<8192>, grid, block, s, in, in_pitch, out, out_pitch, (const float2 *)d_H, (const float2 *)d_tw, overlap, tail);
    PG_HIP(hipGetLastError());
    // m_pFFTOverlapBuf <- last taps-1 input samples of every row (fastfir.cpp:312-316); ordered after the kernel on s
    PG_HIP(hipMemcpy2DAsync(d_tail, sizeof(float2) * (size_t)overlap, in + (n - overlap), sizeof(float2) * (size_t)in_pitch,
                            sizeof(float2) * (size_t)overlap, C, hipMemcpyDeviceToDevice, s));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// AmCore
// ------------------------------------------------------------------------------------------------
int AmCore::init(uint32_t channels, double demod_rate, long long max_n)
{
    C = channels;
    rate = demod_rate;
    if (int rc = tmp.alloc((int)C, kMaxTaps, max_n)) return rc;
    PG_TRY(d_taps.alloc_zero((size_t)kMaxTaps * C));
    PG_TRY(d_ntaps.alloc_zero(C));
    PG_TRY(d_list.alloc(C));
    PG_TRY(d_state.alloc_zero((size_t)4 * C));
    const double alpha = (double)0.9999f;  // DC_ALPHA is a float literal, demod_am.cpp:36
    fill_scan_section(scan.sec[0], kOnePoleDiff, &alpha);
    return 0;
}
int AmCore::set_bandwidth(hipStream_t s, uint32_t ch, double bw)
{
    // InitLPFilter(0, 1.0, 50.0, bw, bw*1.8, rate); it also clears the FIR delay line (fir.cpp:297-303)
    const std::vector<double> h = design::fir_lowpass(0, 1.0, 50.0, bw, bw * 1.8, rate);
    std::vector<float> hf(kMaxTaps, 0.f);
    for (size_t i = 0; i < h.size(); i++) hf[i] = (float)h[i];
    const int nt = (int)h.size();
    PG_HIP(hipMemcpyAsync(d_taps + (size_t)ch * kMaxTaps, hf.data(), sizeof(float) * kMaxTaps, hipMemcpyHostToDevice, s));
    PG_HIP(hipMemcpyAsync(d_ntaps + ch, &nt, sizeof(int), hipMemcpyHostToDevice, s));
    PG_HIP(hipMemsetAsync(tmp.base + (size_t)ch * tmp.pitch, 0, sizeof(float2) * tmp.hist, s));
    PG_HIP(hipStreamSynchronize(s));
    return 0;
}
int AmCore::set_list(hipStream_t s, const std::vector<int> &am_channels)
{
    list = am_channels;
    if (!list.empty()) {
        PG_HIP(hipMemcpyAsync(d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, s));
        PG_HIP(hipStreamSynchronize(s));
    }
    return 0;
}
int AmCore::run(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n, Gate gate, bool defer_tail)
{
    deferred_n = 0;
    if (list.empty()) return 0;
    if (n > tmp.cap) return fail(PEBBLEGPU_E_SIZE, "%lld samples exceed this object's capacity", n);
    if (n < tmp.hist) return fail(PEBBLEGPU_E_SIZE, "AM demod needs at least %d samples per call", tmp.hist);
    const unsigned na = (unsigned)list.size();
    const long long nsub = (n + kSub - 1) / kSub;
    // One workgroup per channel walks the call sequentially (the 0.9999 pole forbids a warm-up), so it may read
    // and write the same state slot; a channel that leaves AM keeps its stale state like the idle Demod_AM object.
    launch(k_iir_scan<2, 1>, dim3(1, na), dim3(64), s, in, in_pitch, tmp.data(), tmp.pitch, n, scan, (const double *)d_state, d_state,
           (int)nsub, -1, (const int *)d_list, gate);
    launch(k_fir_dec, dim3(cdiv(n, 256), na), dim3(256), s, (const float2 *)tmp.data(), tmp.pitch, out, out_pitch, n, 1,
           (const float *)d_taps, (const float *)nullptr, (int)kMaxTaps, (const int *)d_ntaps, 0, 1.0f, 0, (const int *)d_list, gate);
    if (defer_tail) deferred_n = n;
    else launch(k_save_tail, dim3(cdiv(tmp.hist, 256), na), dim3(256), s, tmp.data(), tmp.pitch, n, tmp.hist, (const int *)d_list, gate);
    PG_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// PllCore: Demod_NFM (mode 0) or Demod_SAM (mode 1) for the listed channels
// ------------------------------------------------------------------------------------------------
int PllCore::init(uint32_t channels, double demod_rate, long long max_n, int which)
{
    C = channels;
    rate = demod_rate;
    mode = which;
    memset(&pp, 0, sizeof(pp));
    pp.mode = mode;
    std::vector<double> h;
    std::vector<float> hi(kMaxTaps, 0.f), hq(kMaxTaps, 0.f);
    if (mode == 0) {  // Demod_NFM::init, demod_nfm.cpp:44-66 (float members, demod_nfm.h:27-40)
        const double norm = design::kTwoPi / rate;
        pp.lo = (float)(-15000.0 * norm);  // FMPLL_RANGE
        pp.hi = (float)(15000.0 * norm);
        pp.alpha = (float)(2.0 * .707 * 3000.0 * norm);  // FMPLL_ZETA, FMPLL_BW
        pp.beta = (float)((double)(pp.alpha * pp.alpha) / (4.0 * .707 * .707));
        pp.out_gain = 1.0f;
        pp.dc_alpha = (float)(1.0 - std::exp(-1.0 / (rate * 0.001)));  // FMDC_ALPHA
        h = design::fir_lowpass(0, 1.0, 50.0, 3000.0, 1.6 * 3000.0, rate);
        for (size_t i = 0; i < h.size(); i++) hi[i] = hq[i] = (float)h[i];
    } else {          // Demod_SAM ctor, demod_sam.cpp:5-32
        const float zeta = 0.707f;
        pp.alpha = (float)(2.0 * zeta * 100 * design::kTwoPi / rate);
        pp.beta = (float)((double)(pp.alpha * pp.alpha) / (4.0 * zeta * zeta));
        pp.lo = (float)(-1000 * design::kTwoPi / rate);
        pp.hi = (float)(1000 * design::kTwoPi / rate);
        h = design::fir_lowpass(0, 1.0, 40.0, 4500, 5500, rate);
        const int nt = (int)h.size();
        for (int n = 0; n < nt; n++) {  // GenerateHBFilter(5000.0), fir.cpp:454-468
            const double a = (design::kTwoPi * 5000.0 / rate) * ((double)n - ((double)(nt - 1) / 2.0));
            hi[n] = (float)(2.0 * h[n] * std::cos(a));
            hq[n] = (float)(2.0 * h[n] * std::sin(a));
        }
    }
    ntaps = (int)h.size();
    // k_fir_dec computes sum_p x[i-(T-1)+p] h[p]; CFir computes sum_k coef[k] x[i-k]: store the taps reversed
    std::vector<float> ri(kMaxTaps, 0.f), rq(kMaxTaps, 0.f);
    for (int p = 0; p < ntaps; p++) { ri[p] = hi[ntaps - 1 - p]; rq[p] = hq[ntaps - 1 - p]; }
    PG_TRY(d_taps_i.upload(ri.data(), kMaxTaps));
    PG_TRY(d_taps_q.upload(rq.data(), kMaxTaps));
    if (int rc = tmp.alloc((int)C, kMaxTaps, max_n)) return rc;
    PG_TRY(d_state.alloc_zero(C));
    return d_list.alloc(C);
}
int PllCore::set_list(hipStream_t s, const std::vector<int> &channels)
{
    list = channels;
    if (!list.empty()) {
        PG_HIP(hipMemcpyAsync(d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, s));
        PG_HIP(hipStreamSynchronize(s));
    }
    return 0;
}
int PllCore::run(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n, Gate gate, int blk_len, int blk_frame)
{
    if (list.empty()) return 0;
    if (n > tmp.cap) return fail(PEBBLEGPU_E_SIZE, "%lld samples exceed this object's capacity", n);
    if (n < tmp.hist) return fail(PEBBLEGPU_E_SIZE, "PLL demod needs at least %d samples per call", tmp.hist);  // k_save_tail reads tmp[n - hist .. n)
    const unsigned nl = (unsigned)list.size();
    launch(k_pll_demod, dim3(cdiv(nl, 64)), dim3(64), s, in, in_pitch, tmp.data(), tmp.pitch, n, pp, d_state, (const int *)d_list,
           (int)nl, gate, blk_frame > 0 ? blk_len : 0, blk_frame);
    launch(k_fir_dec, dim3(cdiv(n, 256), nl), dim3(256), s, (const float2 *)tmp.data(), tmp.pitch, out, out_pitch, n, 1, (const float *)d_taps_i,
           (const float *)d_taps_q, 0, (const int *)nullptr, ntaps, 1.0f, mode == 1 ? 1 : 0, (const int *)d_list, gate);
    // the listed channels' FIR history (a gated channel keeps its own)
    launch(k_save_tail, dim3(cdiv(tmp.hist, 256), nl), dim3(256), s, tmp.data(), tmp.pitch, n, tmp.hist, (const int *)d_list, gate);
    PG_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// WfmCore
// ------------------------------------------------------------------------------------------------
int WfmCore::init(uint32_t channels, double demod_rate, long long max_n, const Tuning &t)
{
    tun = t;
    C = channels;
    rate = demod_rate;
    max_n_ = max_n;
    stereo.assign(C, 0);
    lp_on = rate >= 150000;  // demod_wfm.cpp:210
    const design::Biquad l = design::biquad_lowpass(75000, 1.0, rate);   // demod_wfm.cpp:164
    const double lpc[5] = {l.b0, l.b1, l.b2, l.a1, l.a2};
    fill_scan_section(lp.sec[0], kBiquadDf2, lpc);
    const double da = 1.0 - std::exp(-1.0 / (rate * 75E-6));            // demod_wfm.cpp:181-183,454
    fill_scan_section(dn.sec[0], kOnePoleAvg, &da);
    const design::Biquad br = design::biquad_notch(19000.0, 5, rate);    // demod_wfm.cpp:178
    const double brc[5] = {br.b0, br.b1, br.b2, br.a1, br.a2};
    fill_scan_section(dn.sec[1], kBiquadDf2, brc);
    const std::vector<double> h = design::fir_lowpass(0, 1.0, 60.0, 15000.0, 1.4 * 15000.0, rate);  // demod_wfm.cpp:175
    ntaps = (int)h.size();
    std::vector<float> hf(kMaxTaps, 0.f);
    for (size_t i = 0; i < h.size(); i++) hf[i] = (float)h[i];
    PG_TRY(d_taps.upload(hf.data(), kMaxTaps));
    // One kernel with no carried state when the cascades decay fast enough to be folded into FIRs (they do at every rate
    // the WFM chain produces: pole radii <= ~0.97); otherwise the exact sequential multi-kernel path below.
    {
        std::vector<double> hl(1, 1.0), ha;
        bool ok = true;
        if (lp_on) ok = design::cascade_impulse(std::vector<double>(), nullptr, std::vector<design::Biquad>(1, l), 1e-11, kWfmLpMax, hl);
        if (ok) ok = design::cascade_impulse(h, &da, std::vector<design::Biquad>(1, br), 1e-11, kWfmIrMax, ha);
        fused = ok && wfm_fir_lds_bytes((int)((ha.size() + 15) & ~(size_t)15), (int)hl.size()) <= 64 * 1024;
        if (fused) {
            L4 = (int)((ha.size() + 15) & ~(size_t)15);
            Llp = (int)hl.size();
            ha.resize((size_t)L4 + 16, 0.0);  // the kernel fetches its taps one chunk of 16 ahead
            std::vector<float> hlf(hl.begin(), hl.end()), haf(ha.begin(), ha.end());
            PG_TRY(d_h.upload(haf.data(), (size_t)L4 + 16));
            std::vector<float> hm((size_t)wfm_mx_table_floats(L4));
            wfm_mx_fill_taps(haf.data(), L4, hm.data());
            PG_TRY(d_hm.upload(hm.data(), hm.size()));
            PG_TRY(d_hlp.upload(hlf.data(), (size_t)Llp));
            for (int i = 0; i < 2; i++) PG_TRY(d_xtail[i].alloc_zero((size_t)(L4 + Llp) * C));
            return 0;
        }
    }
    if (int rc = a.alloc((int)C, 2, max_n)) return rc;
    if (int rc = b.alloc((int)C, kMaxTaps, max_n)) return rc;
    if (int rc = c.alloc((int)C, 0, max_n)) return rc;
    for (int i = 0; i < 2; i++) {
        PG_TRY(d_lp_state[i].alloc_zero((size_t)4 * C));
        PG_TRY(d_dn_state[i].alloc_zero((size_t)8 * C));
    }
    return 0;
}
int WfmCore::set_stereo(uint32_t ch, bool on)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (on && !fused) return fail(PEBBLEGPU_E_UNSUPPORTED, "dmFMS needs the single-kernel WFM path (this demodulator rate runs the sequential one)");
    if (on && !d_pilot) {  // first dmFMS channel of this object: the pilot loop's constants, state and the (L - R) rows
        const design::WfmPilotDesign pd = design::wfm_pilot_design(rate);
        memset(&pilot, 0, sizeof(pilot));
        pilot.b0 = pd.bp.b0; pilot.b2 = pd.bp.b2; pilot.a1 = pd.bp.a1; pilot.a2 = pd.bp.a2;
        pilot.nco_lo = pd.nco_lo; pilot.nco_hi = pd.nco_hi; pilot.alpha = pd.alpha; pilot.beta = pd.beta;
        pilot.err_alpha = pd.err_alpha; pilot.phase_adjust = pd.phase_adjust;
        pilot.L4 = L4;
        PG_TRY(d_hilb.upload(pd.hilb, 122));
        PG_TRY(d_stereo_list.alloc(C));
        if (int rc = lm.alloc((int)C, L4 + 16, max_n_)) return rc;
        // initPilotPll (demod_wfm.cpp:371-386), once per object as in the reference: a channel that leaves dmFMS and comes back finds its
        // loop where it left it (its lock average still high: it stays dropped)
        std::vector<WfmPilotState> z(C);
        memset(z.data(), 0, sizeof(WfmPilotState) * C);
        for (auto &q : z) { q.nco_freq = pd.nco_freq0; q.quiet = 1LL << 40; }
        PG_TRY(d_pilot.upload(z.data(), C));
        // the RDS members, initialised with the rest of setSampleRate (demod_wfm.cpp:187-191)
        if (tun.rds) { if (int rc = rds.init(C, rate, max_n_)) return rc; }
    }
    // An owner with a fixed frame (a receiver: stereo_block = frames_per_buffer) is refused here, where nothing of a call is queued yet and
    // the channel simply stays dmFMM; every call of such an owner is whole frames, so one frame passing is all calls passing.  The
    // stand-alone step (stereo_block = 0: a call is a block) has no frame to ask about and is checked per call in run().
    if (on && stereo_block > 0) { if (int rc = rds.check_frame(stereo_block, true)) return rc; }
    if (stereo[ch] != (unsigned char)on) stereo_dirty = true;
    stereo[ch] = on;
    return 0;
}
int WfmCore::stereo_lock(hipStream_t s, uint32_t ch, int *lock, int *changed)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (last_lock.size() != C) { last_lock.assign(C, 1); stereo_ran.assign(C, 0); }
    int now = 0;
    if (d_pilot && stereo_ran[ch]) {  // a block of processDataStereo has run: locked until the first block that ended without lock
        WfmPilotState st;
        PG_HIP(hipStreamSynchronize(s));
        PG_HIP(hipMemcpy(&st, d_pilot + ch, sizeof(st), hipMemcpyDeviceToHost));
        now = st.dropped ? 0 : 1;
    }
    if (lock) *lock = now;
    if (changed) *changed = now != last_lock[ch] ? 1 : 0;
    last_lock[ch] = (char)now;
    return 0;
}
int WfmCore::run(hipStream_t s, const float2 *in, long long in_pitch, float2 *out, long long out_pitch, long long n,
                 const std::vector<TailJob> *more_tails, const OscAdvance *oa, bool *carried)
{
    if (carried) *carried = false;
    if (n < kMaxTaps) return fail(PEBBLEGPU_E_SIZE, "WFM demod needs at least %d samples per call", kMaxTaps);
    last_n = n;
    if (stereo_dirty) {  // (rare: a mode change)
        if (!d_stereo) PG_TRY(d_stereo.alloc(C));
        PG_HIP(hipMemcpyAsync(d_stereo, stereo.data(), C, hipMemcpyHostToDevice, s));
        std::vector<int> list;
        for (uint32_t ch = 0; ch < C; ch++) if (stereo[ch]) list.push_back((int)ch);
        n_stereo = (int)list.size();
        if (n_stereo) PG_HIP(hipMemcpyAsync(d_stereo_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, s));
        PG_HIP(hipStreamSynchronize(s));
        stereo_dirty = false;
    }
    // Before anything of THIS object's call is queued: that protects pebblegpu_demod_process, whose call starts here.  A receiver has queued
    // its mixer and decimator by now and would fail for good, which is why its frame is checked in set_stereo(); for it this is the last
    // line of defence (a frame that passed there passes here: every call is whole frames within the capacity).
    if (n_stereo) { if (int rc = rds.check(n, stereo_block)) return rc; }
    if (fused) {
        WfmFirParams wp;
        memset(&wp, 0, sizeof(wp));
        wp.L4 = L4;
        wp.Llp = Llp;
        wp.gain = 0.25f;  // FMDEMOD_GAIN, demod_wfm.cpp:51
        const long long Lx = (long long)L4 + Llp;
        // next call's history = the last Lx samples of (old history | this call's input), into the other buffer; when the
        // call alone covers it the copy is a tail-refresh job (tail_jobs): carried by this launch when the caller hands over
        // its own jobs, else left to the caller's tail-refresh launch
        float2 *nt = d_xtail[parity ^ 1];
        deferred_in = nullptr;
        if (n >= Lx) {
            deferred_in = in;
            deferred_pitch = in_pitch;
        }
        const int groups = (int)cdiv(n, kWfmOutB);
        TailJobs tj;
        memset(&tj, 0, sizeof(tj));
        int extra = 0;
        if (more_tails != nullptr && n >= Lx) {
            std::vector<TailJob> jobs(*more_tails);
            jobs.push_back(TailJob{const_cast<float2 *>(in), in_pitch, n, (int)Lx, 0, nt, Lx});
            if (fill_tail_jobs(tj, jobs, oa) == 0) {
                extra = (int)jobs.size();
                if (carried) *carried = true;
                deferred_in = nullptr;  // (done here)
            } else {
                memset(&tj, 0, sizeof(tj));
            }
        }
        launch_lds(k_wfm_fir, dim3(groups + extra, C), dim3(512), wfm_fir_lds_bytes(L4, Llp), s, in, in_pitch, (const float2 *)d_xtail[parity],
                   out, out_pitch, n, wp, (const float *)d_hm, (const float *)d_hlp, (const unsigned char *)d_stereo, groups, tj);
        PG_HIP(hipGetLastError());
        if (n < Lx) {
            PG_HIP(hipMemcpy2DAsync(nt, sizeof(float2) * Lx, d_xtail[parity] + n, sizeof(float2) * Lx, sizeof(float2) * (Lx - n), C, hipMemcpyDeviceToDevice, s));
            PG_HIP(hipMemcpy2DAsync(nt + (Lx - n), sizeof(float2) * Lx, in, sizeof(float2) * in_pitch, sizeof(float2) * n, C, hipMemcpyDeviceToDevice, s));
        }
        parity ^= 1;
        if (n_stereo) {
            if (last_lock.size() != C) { last_lock.assign(C, 1); stereo_ran.assign(C, 0); }
            for (uint32_t ch = 0; ch < C; ch++) if (stereo[ch]) stereo_ran[ch] = 1;
            // dmFMS before the pilot PLL's drop-out: the (L - R) part of the blocks that end locked, through the same audio response
            if (n > lm.cap) return fail(PEBBLEGPU_E_SIZE, "%lld samples exceed this object's capacity", n);
            PG_HIP(hipMemset2DAsync(lm.data(), sizeof(float2) * (size_t)lm.pitch, 0, sizeof(float2) * (size_t)n, C, s));
            WfmPilotParams pp = pilot;
            pp.block = stereo_block > 0 ? stereo_block : (int)n;
            launch(k_wfm_pilot, dim3(cdiv(n_stereo, 64)), dim3(64), s, in, in_pitch, n, pp, (const double *)d_hilb, d_pilot, lm.data(), lm.pitch,
                   (const int *)d_stereo_list, n_stereo);
            launch(k_wfm_lmr_fir, dim3(cdiv(n, 256), n_stereo), dim3(256), s, (const float2 *)lm.data(), lm.pitch, (const float *)d_h, L4, out, out_pitch, n,
                   (const WfmPilotState *)d_pilot, (const int *)d_stereo_list);
            // ALL rows, unlike the RDS rows (RdsCore::run): `lm` is what a channel adds to the input of the audio filter the reference
            // shares between processDataMono and processDataStereo (m_LPFilter, demod_wfm.cpp:359-361), and a channel in dmFMM adds
            // nothing.  The memset above zeroes [0, n) of every row, k_wfm_pilot writes the listed ones only, so an unlisted row's
            // refresh shifts n zeros into its head-room: the (L - R) part it left with rings out of the filter while it is away, as
            // in the reference.  A row never holds stale data, whatever the call lengths: [0, n) is rewritten on every call.
            std::vector<TailJob> lj(1, TailJob{lm.data(), lm.pitch, n, lm.hist, 0, nullptr, 0});
            if (int rc = run_save_tails(s, lj, C)) return rc;
            PG_HIP(hipGetLastError());
            // the RDS branch (demod_wfm.cpp:296-357) runs whether the pilot is locked or not
            if (int rc = rds.run(s, in, in_pitch, n, (const double *)d_hilb, (const int *)d_stereo_list, n_stereo, stereo_block)) return rc;
            lm_pending = lm.hist;
        } else if (lm_pending > 0) {
            // the last dmFMS channel has left: the same n zeros go into every row, as they would with another channel still listed
            const long long m = n < lm.cap ? n : lm.cap;
            PG_HIP(hipMemset2DAsync(lm.data(), sizeof(float2) * (size_t)lm.pitch, 0, sizeof(float2) * (size_t)m, C, s));
            std::vector<TailJob> lj(1, TailJob{lm.data(), lm.pitch, m, lm.hist, 0, nullptr, 0});
            if (int rc = run_save_tails(s, lj, C)) return rc;
            lm_pending -= m < lm_pending ? m : lm_pending;
        }
        return 0;
    }
    if (n > a.cap) return fail(PEBBLEGPU_E_SIZE, "%lld samples exceed this object's capacity", n);
    const long long nsub = (n + kSub - 1) / kSub;
    // slow poles: one workgroup per channel walks the call sequentially with the exact carried state
    if (lp_on)
        launch(k_iir_scan<0, 1>, dim3(1, C), dim3(64), s, in, in_pitch, a.data(), a.pitch, n, lp, (const double *)d_lp_state[0], d_lp_state[0],
               (int)nsub, -1, (const int *)nullptr, Gate{nullptr, 0, 0});
    else
        launch(k_copy, dim3(cdiv(n, 256), C), dim3(256), s, in, in_pitch, a.data(), a.pitch, n);
    launch(k_discrim, dim3(cdiv(n, 256), C), dim3(256), s, (const float2 *)a.data(), a.pitch, b.data(), b.pitch, n, 0.25f);  // FMDEMOD_GAIN
    launch(k_fir_dec, dim3(cdiv(n, 256), C), dim3(256), s, (const float2 *)b.data(), b.pitch, c.data(), c.pitch, n, 1, (const float *)d_taps,
           (const float *)nullptr, 0, (const int *)nullptr, ntaps, 1.0f, 0, (const int *)nullptr, Gate{nullptr, 0, 0});
    launch(k_iir_scan<1, 2>, dim3(1, C), dim3(64), s, (const float2 *)c.data(), c.pitch, out, out_pitch, n, dn, (const double *)d_dn_state[0],
           d_dn_state[0], (int)nsub, -1, (const int *)nullptr, Gate{nullptr, 0, 0});
    PG_HIP(hipGetLastError());
    return 0;
}
void WfmCore::tail_jobs(std::vector<TailJob> &jobs) const
{
    if (fused) {
        if (deferred_in) jobs.push_back(TailJob{const_cast<float2 *>(deferred_in), deferred_pitch, last_n, L4 + Llp, 0, d_xtail[parity], (long long)(L4 + Llp)});
        return;
    }
    jobs.push_back(TailJob{a.data(), a.pitch, last_n, a.hist, 0, nullptr, 0});
    jobs.push_back(TailJob{b.data(), b.pitch, last_n, b.hist, 0, nullptr, 0});
}

int run_gate_eval(hipStream_t s, const float4 *d_smeter, long long smeter_pitch, int frames_per_sf, int k, const float *d_squelch, unsigned char *d_gate,
                  int stride, uint32_t channels)
{
    launch(k_gate_eval, dim3((unsigned)((channels * (unsigned)k + 255) / 256)), dim3(256), s, d_smeter, smeter_pitch, frames_per_sf, k, d_squelch, d_gate, stride, (int)channels);
    PG_HIP(hipGetLastError());
    return 0;
}
// rows[j], j < k: the compact S-meter row super-frame j reads, kGateRowCarried or kGateRowNone (k_gate_eval_rows)
int run_gate_eval_rows(hipStream_t s, const float4 *d_smeter, long long smeter_pitch, const float4 *d_carried, const int *rows, int k, const float *d_squelch,
                       unsigned char *d_gate, int stride, uint32_t channels)
{
    for (int j0 = 0; j0 < k; j0 += kListMax) {
        GateRows gr;
        memset(&gr, 0, sizeof(gr));
        gr.n = k - j0 < kListMax ? k - j0 : kListMax;
        gr.j0 = j0;
        for (int j = 0; j < gr.n; j++) gr.row[j] = rows[j0 + j];
        launch(k_gate_eval_rows, dim3((unsigned)((channels * (unsigned)gr.n + 255) / 256)), dim3(256), s, d_smeter, smeter_pitch, d_carried, d_squelch, d_gate, stride,
               (int)channels, gr);
    }
    PG_HIP(hipGetLastError());
    return 0;
}
int run_gate_zero(hipStream_t s, float2 *audio, long long pitch, long long spf, const unsigned char *d_gate, int stride, uint32_t channels, int k)
{
    launch(k_gate_zero, dim3((unsigned)((spf + 1023) / 1024), channels, (unsigned)k), dim3(256), s, audio, pitch, spf, d_gate, stride);
    PG_HIP(hipGetLastError());
    return 0;
}

int run_signal_strength(hipStream_t s, const float *d_spec, long long stream_pitch, int bins, long long n_frames, const SmBins *d_bins,
                        float4 *d_out, long long out_pitch, uint32_t channels)
{
    if (n_frames <= 0) return 0;
    launch(k_signal_strength, dim3((unsigned)n_frames, channels), dim3(64), s, d_spec, stream_pitch, bins, n_frames, d_bins, d_out, out_pitch);
    PG_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// AgcCore
// ------------------------------------------------------------------------------------------------
int AgcCore::init(uint32_t channels, double demod_rate)
{
    C = channels;
    rate = demod_rate;
    host.assign(C, Host());
    PG_TRY(d_state.alloc_zero(C));
    PG_TRY(d_list.alloc(C));
    std::vector<AgcState> init(1);
    memset(&init[0], 0, sizeof(AgcState));
    init[0].manual_gain = 1.0;  // AGC::AGC -> setAgcMode(AGC_OFF, 1): dBToAmplitude(1 / 5) = 1 (agc.cpp:29,241-245)
    for (uint32_t c = 0; c < C; c++) PG_HIP(hipMemcpy(d_state + c, &init[0], offsetof(AgcState, sig), hipMemcpyHostToDevice));
    return 0;
}
int AgcCore::set_mode(uint32_t ch, int mode, int threshold)
{
    if (ch >= C || mode < 0 || mode > 4) return fail(PEBBLEGPU_E_INVALID, "bad AGC channel or mode");
    Host &h = host[ch];
    h.mode = mode;
    h.threshold = threshold;
    h.dirty = true;
    list_dirty = true;
    return 0;
}
int AgcCore::apply(hipStream_t s)
{
    if (!list_dirty) return 0;
    for (uint32_t c = 0; c < C; c++) {
        Host &h = host[c];
        if (!h.dirty) continue;
        h.dirty = false;
        // setAgcMode picks the decay for the mode, then setParameters (agc.cpp:53-82, 237-300)
        int decay = 200;
        if (h.mode == 1) decay = 100; else if (h.mode == 3) decay = 500; else if (h.mode == 2) decay = 250; else if (h.mode == 4) decay = 2000;
        AgcState st;
        PG_HIP(hipStreamSynchronize(s));
        PG_HIP(hipMemcpy(&st, d_state + c, offsetof(AgcState, sig), hipMemcpyDeviceToHost));  // running averages survive a parameter change
        st.mode = h.mode;
        if (h.mode == 0) {
            st.manual_gain = std::pow(10, (double)(h.threshold / 5) / 20.0);  // integer division as written
            h.manual = st.manual_gain;
            PG_HIP(hipMemcpy(d_state + c, &st, offsetof(AgcState, sig), hipMemcpyHostToDevice));
            continue;
        }
        const int thr = -h.threshold;
        st.manual_gain = 1;
        h.manual = 1;
        if (!(h.use_hang == 0 && thr == h.thr && h.slope == 0.0 && decay == h.decay && h.sample_rate == rate)) {
            h.use_hang = 0; h.thr = thr; h.slope = 0; h.decay = decay;
            if (h.sample_rate != rate) {  // first set-up: clear the delay line and the averagers (agc.cpp:262-277)
                h.sample_rate = rate;
                std::vector<AgcState> full(1);
                memset(&full[0], 0, sizeof(AgcState));
                for (int i = 0; i < kAgcMaxDelayBuf; i++) full[0].mag[i] = -16.0;
                PG_HIP(hipMemcpy(d_state + c, &full[0], sizeof(AgcState), hipMemcpyHostToDevice));
                st.sig_ptr = 0; st.hang_timer = 0; st.peak = -16.0; st.decay_avg = -5.0; st.attack_avg = -5.0; st.mag_pos = 0;
            }
            const float kDelayTc = .015f, kWindowTc = .018f, kAttackRiseTc = .002f, kAttackFallTc = .005f, kDecayRatio = .3f, kOutScale = 0.7f;
            st.use_hang = 0;
            st.knee = (double)thr / 20.0;
            st.gain_slope = h.slope / 100.0;
            st.fixed_gain = kOutScale * std::pow(10.0, st.knee * (st.gain_slope - 1.0));
            st.attack_rise = 1.0 - std::exp(-1.0 / (rate * kAttackRiseTc));
            st.attack_fall = 1.0 - std::exp(-1.0 / (rate * kAttackFallTc));
            st.decay_rise = 1.0 - std::exp(-1.0 / (rate * (double)decay * .001 * kDecayRatio));
            st.hang_time = (int)(rate * (double)decay * .001);
            st.decay_fall = 1.0 - std::exp(-1.0 / (rate * (double)decay * .001));
            st.delay_samples = (int)(rate * kDelayTc);
            st.window_samples = (int)(rate * kWindowTc);
            if (st.delay_samples >= kAgcMaxDelayBuf - 1) st.delay_samples = kAgcMaxDelayBuf - 1;
            if (st.window_samples > kAgcMaxDelayBuf) return fail(PEBBLEGPU_E_UNSUPPORTED, "AGC window of %d samples exceeds the reference's own buffer", st.window_samples);
        }
        PG_HIP(hipMemcpy(d_state + c, &st, offsetof(AgcState, sig), hipMemcpyHostToDevice));
    }
    list.clear();
    for (uint32_t c = 0; c < C; c++)
        if ((host[c].mode != 0 || host[c].manual != 1.0) && !(c < muted.size() && muted[c])) list.push_back((int)c);
    if (!list.empty()) PG_HIP(hipMemcpyAsync(d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, s));
    PG_HIP(hipStreamSynchronize(s));
    list_dirty = false;
    return 0;
}
int AgcCore::run(hipStream_t s, float2 *buf, long long pitch, long long n, Gate gate)
{
    if (list.empty()) return 0;  // AGC_OFF with unit manual gain: out = 1.0 * in
    launch(k_agc, dim3(cdiv((long long)list.size(), 64)), dim3(64), s, buf, pitch, n, d_state, (const int *)d_list, (int)list.size(), gate);
    PG_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// ConditionCore, AnfCore
// ------------------------------------------------------------------------------------------------
int ConditionCore::init(uint32_t streams, uint32_t frame, double sample_rate, long long max_n)
{
    S = streams;
    nf = frame;
    fs = sample_rate;
    cap = max_n;
    host.assign(S, Host());
    const design::Biquad h = design::biquad_highpass(10, 0.7071, fs);  // DCRemoval ctor, dcremoval.cpp:5-9
    const double c[5] = {h.b0, h.b1, h.b2, h.a1, h.a2};
    fill_scan_section(dc.sec[0], kBiquadDf2, c);
    return 0;
}
int ConditionCore::set(uint32_t stream, int flags, double gain, double phase)
{
    if (stream >= S || flags < 0 || flags > 15) return fail(PEBBLEGPU_E_INVALID, "bad stream or conditioner flags");
    if (!std::isfinite(gain) || !std::isfinite(phase)) return fail(PEBBLEGPU_E_INVALID, "the IQ gain and phase factors must be finite");
    Host &h = host[stream];
    if (!d_buf) {  // first use: the conditioned copy and the per-stream state
        PG_TRY(d_buf.alloc((size_t)cap * S));
        PG_TRY(d_dc_state.alloc_zero((size_t)4 * S));
        PG_TRY(d_dc_list.alloc(S));
        PG_TRY(d_iq.alloc(S));
        std::vector<NbState> nb(S);
        memset(nb.data(), 0, sizeof(NbState) * S);
        for (auto &b : nb) { b.nb_avg_mag = 1; b.nb2_avg_mag = 1; }  // NoiseBlanker ctor, noiseblanker.cpp:9-15
        PG_TRY(d_nb.upload(nb.data(), S));
    }
    // setNbEnabled(true) / setNb2Enabled(true) reset their averages (noiseblanker.cpp:20-37)
    const int turned_on = flags & ~h.flags;
    if (turned_on & 12) {
        NbState b;
        PG_HIP(hipDeviceSynchronize());
        PG_HIP(hipMemcpy(&b, d_nb + stream, sizeof(b), hipMemcpyDeviceToHost));
        if (turned_on & 4) { b.spike_count = 0; b.nb_avg_mag = 0; }
        if (turned_on & 8) { b.nb2_avg_mag = 0; b.nb2_avg[0] = b.nb2_avg[1] = 0; }
        PG_HIP(hipMemcpy(d_nb + stream, &b, sizeof(b), hipMemcpyHostToDevice));
    }
    h.flags = flags;
    h.gain = gain;
    h.phase = phase;
    dirty = true;
    return 0;
}
int ConditionCore::apply(hipStream_t s)
{
    if (!dirty) return 0;
    PG_HIP(hipStreamSynchronize(s));
    any = iq_any = nb_any = false;
    dc_list.clear();
    std::vector<IqFactors> iq(S);
    for (uint32_t i = 0; i < S; i++) {
        const Host &h = host[i];
        if (h.flags) any = true;
        if (h.flags & 1) dc_list.push_back((int)i);
        iq[i] = IqFactors{h.gain, h.phase, (h.flags & 2) ? 1 : 0, 0};
        if (h.flags & 2) iq_any = true;
        if (h.flags & 12) nb_any = true;
        const int nbf = (h.flags >> 2) & 3;
        PG_HIP(hipMemcpy(&d_nb[i].flags, &nbf, sizeof(int), hipMemcpyHostToDevice));
    }
    if (!dc_list.empty()) PG_HIP(hipMemcpy(d_dc_list, dc_list.data(), sizeof(int) * dc_list.size(), hipMemcpyHostToDevice));
    PG_HIP(hipMemcpy(d_iq, iq.data(), sizeof(IqFactors) * S, hipMemcpyHostToDevice));
    dirty = false;
    return 0;
}
int ConditionCore::run(hipStream_t s, const float2 *d_in, long long in_pitch, long long n, const float2 **out, long long *out_pitch)
{
    *out = d_in;
    *out_pitch = in_pitch;
    if (!any) return 0;
    if (n > cap || n % nf != 0) return fail(PEBBLEGPU_E_SIZE, "conditioners take whole frames within the bank's capacity");
    PG_HIP(hipMemcpy2DAsync(d_buf, sizeof(float2) * (size_t)cap, d_in, sizeof(float2) * (size_t)in_pitch, sizeof(float2) * (size_t)n, S, hipMemcpyDeviceToDevice, s));
    if (!dc_list.empty()) {  // DCRemoval::process: CIir high-pass 10 Hz, exact carried state (its pole sits at 1 - 3e-6 .. 3e-5)
        const long long nsub = (n + kSub - 1) / kSub;
        launch(k_iir_scan<0, 1>, dim3(1, (unsigned)dc_list.size()), dim3(64), s, (const float2 *)d_buf, cap, d_buf, cap, n, dc, (const double *)d_dc_state,
               d_dc_state, (int)nsub, -1, (const int *)d_dc_list, Gate{nullptr, 0, 0});
    }
    if (iq_any) launch(k_iq_balance, dim3(cdiv(n / nf, 64), S), dim3(64), s, d_buf, cap, (int)nf, n / nf, (const IqFactors *)d_iq);
    if (nb_any) launch(k_noise_blank, dim3(cdiv(S, 64)), dim3(64), s, d_buf, cap, n, d_nb, (int)S);
    PG_HIP(hipGetLastError());
    *out = d_buf;
    *out_pitch = cap;
    return 0;
}

int AnfCore::init(uint32_t channels)
{
    C = channels;
    on.assign(C, 0);
    return 0;
}
int AnfCore::set(uint32_t ch, bool enable)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (!d_state) {
        PG_TRY(d_state.alloc_zero(C));  // new CPX[] coefficients and the delay line start at zero
        PG_TRY(d_list.alloc(C));
    }
    on[ch] = enable ? 1 : 0;
    dirty = true;
    return 0;
}
int AnfCore::apply(hipStream_t s)
{
    if (!dirty) return 0;
    list.clear();
    for (uint32_t c = 0; c < C; c++) if (on[c] && !(c < muted.size() && muted[c])) list.push_back((int)c);
    PG_HIP(hipStreamSynchronize(s));
    if (!list.empty()) PG_HIP(hipMemcpy(d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
    dirty = false;
    return 0;
}
int AnfCore::run(hipStream_t s, float2 *buf, long long pitch, long long n, Gate gate)
{
    if (list.empty()) return 0;
    launch(k_anf, dim3((unsigned)list.size()), dim3(64), s, buf, pitch, n, d_state, (const int *)d_list, gate);
    PG_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// ResampCore
// ------------------------------------------------------------------------------------------------
int ResampCore::init(uint32_t channels, const std::vector<uint32_t> &parts_per_superframe, double rate, uint32_t superframes_per_call)
{
    C = channels;
    parts = parts_per_superframe;
    period = 0;
    nf = 0;
    for (uint32_t p : parts) {
        if (p < (uint32_t)kSincPeriods) return fail(PEBBLEGPU_E_SIZE, "resampler needs at least %d samples per frame", kSincPeriods);
        period += p;
        nf = nf ? std::min(nf, p) : p;
    }
    if (parts.empty()) return fail(PEBBLEGPU_E_INVALID, "resampler without a frame");
    dt = rate;
    max_frames = superframes_per_call * (uint32_t)parts.size();
    if (!(dt > 0) || dt > 1e6) return fail(PEBBLEGPU_E_INVALID, "bad resampling ratio");
    std::vector<float> t((size_t)kSincLength);
    for (int i = 0; i < kSincLength; i++) {  // fractresampler.cpp:104-118
        const double window = (0.35875 - 0.48829 * std::cos((design::kTwoPi * i) / (kSincLength - 1)) +
                               0.14128 * std::cos((2.0 * design::kTwoPi * i) / (kSincLength - 1)) -
                               0.01168 * std::cos((3.0 * design::kTwoPi * i) / (kSincLength - 1)));
        const double fi = (design::kTwoPi / 2.0) * (double)(i - kSincLength / 2) / (double)kSincPeriodPts;
        t[i] = (float)(i != kSincLength / 2 ? window * std::sin(fi) / fi : 1.0);
    }
    PG_TRY(d_sinc.upload(t.data(), (size_t)kSincLength));
    for (int i = 0; i < 2; i++) {
        PG_TRY(d_hist[i].alloc_zero((size_t)kSincPeriods * C));  // Init zeroes m_pInputBuf
        PG_TRY(h_frames[i].alloc(max_frames));
        PG_HIP(hipEventCreateWithFlags(&h_done[i], hipEventDisableTiming));
    }
    return d_frames.alloc(max_frames);
}
void ResampCore::release()
{
    for (hipEvent_t &e : h_done) {  // (the memory goes with the object)
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}
int ResampCore::run(hipStream_t s, const float2 *in, long long in_pitch, long long n, float2 *out, long long out_pitch, long long *n_out)
{
    if (n <= 0 || n % (long long)period != 0 || n / (long long)period * (long long)parts.size() > (long long)max_frames)
        return fail(PEBBLEGPU_E_SIZE, "resampler input %lld is not 1..%zu super-frames of %llu", n, (size_t)max_frames / parts.size(), (unsigned long long)period);
    const int F = (int)(n / (long long)period * (long long)parts.size());
    PG_HIP(hipEventSynchronize(h_done[pin]));  // the copy that last used this staging buffer has run
    ResampFrame *hf = h_frames[pin];
    // replay of the reference's time arithmetic, frame by frame (fractresampler.cpp:155-187)
    double t = float_time;
    int total = 0, max_per_frame = 0;
    long long at = 0;
    for (int f = 0; f < F; f++) {
        const int len = (int)parts[(size_t)f % parts.size()];
        hf[f].t_start = t;
        hf[f].out_offset = total;
        hf[f].in_offset = (int)at;
        hf[f].pad_ = 0;
        at += len;
        int it = (int)t, cnt = 0;
        while (it < len) {
            cnt++;
            t += dt;
            it = (int)t;
        }
        t -= (double)len;
        hf[f].nout = cnt;
        total += cnt;
        if (cnt > max_per_frame) max_per_frame = cnt;
    }
    float_time = t;
    *n_out = total;
    if (total > out_pitch) return fail(PEBBLEGPU_E_SIZE, "resampler output %d exceeds its buffer", total);
    PG_HIP(hipMemcpyAsync(d_frames, hf, sizeof(ResampFrame) * F, hipMemcpyHostToDevice, s));
    PG_HIP(hipEventRecord(h_done[pin], s));
    pin ^= 1;
    if (total > 0) {
        const int sub = (int)cdiv(max_per_frame, 256);
        launch(k_resample, dim3((unsigned)(F * sub), C), dim3(256), s, in, in_pitch, (const float2 *)d_hist[parity], out, out_pitch, sub, dt,
               (const ResampFrame *)d_frames, (const float *)d_sinc);
        PG_HIP(hipGetLastError());
    }
    // m_pInputBuf[0..27] <- the last 28 inputs (fractresampler.cpp:189-193)
    PG_HIP(hipMemcpy2DAsync(d_hist[parity ^ 1], sizeof(float2) * kSincPeriods, in + (n - kSincPeriods), sizeof(float2) * in_pitch,
                            sizeof(float2) * kSincPeriods, C, hipMemcpyDeviceToDevice, s));
    parity ^= 1;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// SpectrumCore
// ------------------------------------------------------------------------------------------------
// [bins/nf][nf] w[n] * W_bins^{n q}: the one factor per point of k_spectrum_q128 and k_spectrum_list_q128
static std::vector<float2> factor_table(const std::vector<double> &w, uint32_t nf, uint32_t bins)
{
    const uint32_t zp = bins / nf;
    std::vector<float2> ft((size_t)zp * nf);
    for (uint32_t q = 0; q < zp; q++)
        for (uint32_t n = 0; n < nf; n++) {
            const double a = -design::kTwoPi * (double)(((uint64_t)n * q) % bins) / (double)bins;
            ft[(size_t)q * nf + n] = make_float2((float)(w[n] * std::cos(a)), (float)(w[n] * std::sin(a)));
        }
    return ft;
}
int SpectrumCore::init(uint32_t streams, uint32_t frame, uint32_t fft_size, const Tuning &t)
{
    tun = t;
    S = streams;
    nf = frame;
    bins = fft_size;
    if (bins < 2048) bins = 2048;    // fft.cpp:74-75
    if (bins > 65535) bins = 65535;  // fft.cpp:76-77 (and then not a power of two)
    big = frame == (uint32_t)kBigN && fft_size == (uint32_t)kBigN;  // BASELINE config 5: past the fft.h:21 clamp on purpose
    if (big) bins = kBigN;
    const bool pow2_zp = nf == 2048 && (bins == 2048 || bins == 4096 || bins == 8192 || bins == 16384 || bins == 32768);
    // every other frame length (settings.cpp:57) goes through the general kernel: the frame rounded up to a power of two M <= 16384,
    // bins a power of two >= M (Accelerate's radix-2 transform takes no other sizes either)
    {
        int M = 256, lg = 8;
        while ((uint32_t)M < nf) { M *= 2; lg++; }
        int zl = 0;
        while (((uint32_t)M << zl) < bins) zl++;
        const bool ok = !big && M <= 16384 && ((uint32_t)M << zl) == bins && bins <= 32768;
        any = !big && !pow2_zp;
        if (any && !ok)
            return fail(PEBBLEGPU_E_UNSUPPORTED, "spectrum needs frames of at most 16384 samples and a power-of-two bin count of at least the frame length, at most 32768 (asked %u/%u)", nf, bins);
        if (ok) {
            any_M = M; any_logM = lg; any_zp_log2 = zl;
            std::vector<float2> tw((size_t)M / 2);
            for (int k = 0; k < M / 2; k++) tw[k] = make_float2((float)std::cos(-design::kTwoPi * k / M), (float)std::sin(-design::kTwoPi * k / M));
            PG_TRY(d_twM.upload(tw.data(), tw.size()));
        }
    }
    // One transform per 128-item workgroup (k_spectrum_q128) serves every power-of-two zero-padding; measured against the
    // shared-frame kernels on the bench batch it wins at 2048 bins (0.098 vs 0.105 ms) and loses at 4096 (0.198 vs 0.185) and
    // 8192 (0.44 vs 0.28: its ZP workgroups each re-read the frame and store 4-byte bins ZP*4 bytes apart), so it runs where
    // it wins and where nothing else exists (16384, 32768).  PEBBLEGPU_SPECTRUM_PERQ=1 forces it everywhere (A/B runs).
    use_w64 = tun.spectrum_w64;  // the one-wave 8192-bin kernel (measured equal: opt-in)
    per_q = !big && !any && (bins == 2048 || bins > 8192 || tun.spectrum_perq);
    std::vector<double> w;
    const double cg = design::blackman_harris(nf, w);
    std::vector<float> wf(nf);
    for (uint32_t i = 0; i < nf; i++) wf[i] = (float)w[i];
    PG_TRY(d_window.upload(wf.data(), nf));
    h_window = wf;
    // btab[q][m] = exp(-2*pi*i*(64*m*q)/bins): the wave-uniform factor of the pruned-FFT pre-twiddle W_bins^{n q},
    // n = lane + 64 m (the per-lane factor W_bins^{lane q} is computed in the kernel)
    const uint32_t zp = bins / nf;
    std::vector<float2> bt((size_t)zp * 32);
    for (uint32_t q = 0; q < zp; q++)
        for (uint32_t m = 0; m < 32; m++) {
            const uint64_t k = ((uint64_t)64 * m * q) % bins;
            const double a = -design::kTwoPi * (double)k / (double)bins;
            bt[(size_t)q * 32 + m] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    PG_TRY(d_btab.upload(bt.data(), bt.size()));
    if (per_q) {
        const std::vector<float2> ft = factor_table(w, nf, bins);
        PG_TRY(d_ftab.upload(ft.data(), ft.size()));
        if (int rc = make_twiddles_t128(d_tw128)) return rc;
    }
    if (bins == 8192 && !big && !per_q) {
        stagger = tun.t128_stagger;  // measured on the bench batch: 0.300 ms as two 512-item workgroups per CU, 0.278 with the halves three intervals apart
        pad_lds = tun.t128_padlds;
        std::vector<float2> b2(4 * 16);
        for (int q = 0; q < 4; q++)
            for (int m = 0; m < 16; m++) {
                const double a = -design::kTwoPi * (double)((128 * m * q) % 8192) / 8192.0;
                b2[q * 16 + m] = make_float2((float)std::cos(a), (float)std::sin(a));
            }
        PG_TRY(d_btab128.upload(b2.data(), b2.size()));
        if (int rc = make_twiddles_t128q(d_tw128)) return rc;  // (k_spectrum_t128's own: one table per q)
    }
    scale = (float)(1.0 / (cg * (double)nf));  // /coherentGain then /maxBinPower, fft.cpp:347,355
    if (int rc = make_twiddles(2048, d_tw_nf)) return rc;
    for (int i = 0; i < 2; i++) PG_TRY(d_prev[i].alloc_zero((size_t)bins * S));  // the reference leaves these uninitialised (fft.cpp:107-115)
    return 0;
}
// The 65536-point transform's intermediate Y (8 bytes per point, written by pass A, read by pass B) for a call of per_stream points per
// stream: streams are processed in batches (*bs streams each) whose Y fits well inside the 256 MiB Infinity Cache together with the
// batch's own input and output (one buffer reused by every batch), instead of a call-sized Y that went out to HBM and back (28 B moved
// per 12 B of algorithmic traffic).
int SpectrumCore::size_Y(hipStream_t s, long long per_stream, long long *bs)
{
    const long long batch_mb = tun.big_batch_mb;  // 0: the whole call in one pair of launches (measured: 16 / 32 / 64 / 128 MiB batches 0.61 / 0.48 / 0.39 / 0.34 ms against 0.34 whole: the kernels are not bound by that traffic)
    long long b = batch_mb > 0 ? (batch_mb << 20) / (long long)sizeof(float2) / per_stream : (long long)S;  // streams per batch
    *bs = b = b < 1 ? 1 : (b > (long long)S ? (long long)S : b);
    return d_Y.grow(s, (size_t)b * (size_t)per_stream);
}
// FFT::fftSpectrum for any frame length (and for fewer samples than samplesPerBuffer: copied, zero-padded, not windowed, fft.cpp:129-157)
int SpectrumCore::run_any(hipStream_t s, const float2 *d_in, long long in_pitch, long long F, float *d_out, int n_in, bool windowed)
{
    if (!d_twM) return fail(PEBBLEGPU_E_UNSUPPORTED, "no general display transform for %u-sample frames and %u bins", nf, bins);
    if (n_in <= 0 || n_in > any_M || (uint32_t)n_in > nf) return fail(PEBBLEGPU_E_SIZE, "%d samples do not fit a frame of %u", n_in, nf);
    if (F == 0) return 0;
    SpectrumParams sp;
    sp.in_pitch = in_pitch;
    sp.n_frames = F;
    const SpectrumGeom geo = spectrum_geometry(SpecFamily::any, F, S, bins, nf, S);  // chain length and workgroups: spectrum_geom.h
    sp.frames_per_group = geo.G;
    sp.scale = scale;
    sp.out_pitch = F * (long long)bins;
    AnySpecParams ap;
    ap.n_in = n_in;
    ap.frame = (int)nf;
    ap.M = any_M;
    ap.logM = any_logM;
    ap.zp_log2 = any_zp_log2;
    ap.windowed = windowed ? 1 : 0;
    launch_lds(k_spectrum_any, dim3(geo.wgs, S), dim3(256), sizeof(float2) * (size_t)any_M, s, d_in, d_out, (const float *)d_window, (const float2 *)d_twM,
               (const float *)d_prev[parity], d_prev[parity ^ 1], sp, ap);
    parity ^= 1;
    PG_HIP(hipGetLastError());
    return 0;
}
int SpectrumCore::run(hipStream_t s, const float2 *d_in, long long in_pitch, long long F, float *d_out, const RawSrc *raw, const DecFuse *df, bool nothing_beside)
{
    if (df && !dec_ready()) return fail(PEBBLEGPU_E_INVALID, "the decimator was handed to a display transform that cannot run it");
    last_fullc = nothing_beside && !df && dec_ready();
    if (raw && !(raw_ready() || raw_ready_big())) return fail(PEBBLEGPU_E_INVALID, "raw-format input reached a spectrum kernel that has no converting loads");
    if (any) {
        if (raw || df) return fail(PEBBLEGPU_E_INVALID, "the general display transform takes float2 input and runs no decimator");
        return run_any(s, d_in, in_pitch, F, d_out, (int)nf, true);
    }
    SpectrumParams sp;
    sp.in_pitch = in_pitch;
    sp.n_frames = F;
    if (big) {
        if (F == 0) return 0;
        long long bs = 0;  // streams per batch
        PG_TRY(size_Y(s, (long long)F * kBigN, &bs));
        // a chain that does not start at frame 0 recomputes one frame: chains sized by the batch (spectrum_geom.h)
        const SpectrumGeom geo = spectrum_geometry(SpecFamily::big, F, S, bins, nf, bs);
        sp.frames_per_group = geo.G;
        sp.scale = scale;
        sp.out_pitch = F * (long long)bins;
        for (long long s0 = 0; s0 < (long long)S; s0 += bs) {
            const unsigned nb = (unsigned)((long long)S - s0 < bs ? (long long)S - s0 : bs);
            if (tun.big_split32) {  // A/B: the 32 x 2048 split
                launch(k_big_cols, dim3((unsigned)(F * 8), nb), dim3(256), s, d_in + s0 * in_pitch, (long long)in_pitch, d_Y, (const float *)d_window, (long long)F);
                launch(k_big_rows, dim3(geo.wgs, nb), dim3(256), s, (const float2 *)d_Y, d_out + s0 * sp.out_pitch, (const float2 *)d_tw_nf,
                       (const float *)d_prev[parity] + s0 * kBigN, d_prev[parity ^ 1] + s0 * kBigN, sp);
            } else {
                if (raw) {  // (the stream offset is in IQ pairs of the raw format: the kernel gets the batch's base)
                    RawSrc rs = *raw;
                    rs.base = static_cast<const char *>(raw->base) + (size_t)(s0 * in_pitch) * kRawPairBytes[raw->fmt];
                    const bool b8 = raw->fmt == 0 || raw->fmt == 1;  // 8-bit pairs: the paired tile order (kernels_spectrum.h)
                    const dim3 grid(b8 ? (unsigned)(16 * cdiv(F, 2)) : (unsigned)(F * 8), nb);
                    auto go = [&](auto kern) { launch(kern, grid, dim3(256), s, (long long)in_pitch, d_Y, (const float *)d_window, (long long)F, rs); };
                    with_raw_fmt(raw->fmt, [&](auto F) { go(k_big256_cols_raw<F.value>); });
                } else
                launch(k_big256_cols, dim3((unsigned)(F * 8), nb), dim3(256), s, d_in + s0 * in_pitch, (long long)in_pitch, d_Y, (const float *)d_window, (long long)F);
                launch(k_big256_rows, dim3(geo.wgs, nb), dim3(256), s, (const float2 *)d_Y, d_out + s0 * sp.out_pitch,
                       (const float *)d_prev[parity] + s0 * kBigN, d_prev[parity ^ 1] + s0 * kBigN, sp);
            }
        }
        parity ^= 1;
        PG_HIP(hipGetLastError());
        return 0;
    }
    if (per_q) {
        // one (chain, q) per 128-item workgroup, in stretches of eight chains (spectrum_geom.h)
        const int zp = (int)(bins / nf);
        int zl = 0;
        while ((1 << zl) < zp) zl++;
        const SpectrumGeom geo = spectrum_geometry(SpecFamily::q128, F, S, bins, nf, S);
        sp.frames_per_group = geo.G;
        sp.scale = scale;
        sp.out_pitch = F * (long long)bins;
        launch(tun.spectrum_fregs ? k_spectrum_q128<true> : k_spectrum_q128<false>, dim3(geo.wgs, S), dim3(128), s, d_in, d_out, (const float2 *)d_ftab, (const float2 *)d_tw128,
               (const float *)d_prev[parity], d_prev[parity ^ 1], sp, zl);
        parity ^= 1;
        PG_HIP(hipGetLastError());
        return 0;
    }
    if (bins == 8192 && use_w64) {
        // one-wave transforms (fft_w64.h), one frame chain per 256-item workgroup, two workgroups per CU: chains as long as
        // keeps every workgroup resident at once (every chain recomputes one frame)
        const SpectrumGeom geo = spectrum_geometry(SpecFamily::w64, F, S, bins, nf, S);
        sp.frames_per_group = geo.G;
        sp.scale = scale;
        sp.out_pitch = F * (long long)bins;
        const RawSrc rs = raw ? *raw : RawSrc{nullptr, 0, 0, 0.f, 0};
        const dim3 grid(geo.wgs, S), block(256);
        auto go = [&](auto kern) { launch(kern, grid, block, s, d_in, d_out, (const float *)d_window, (const float2 *)d_btab, (const float *)d_prev[parity], d_prev[parity ^ 1], sp, rs); };
        with_sample_fmt(raw, [&](auto F) { go(k_spectrum_w64<F.value>); });
        parity ^= 1;
        PG_HIP(hipGetLastError());
        return 0;
    }
    if (bins == 8192) {
        // two-wave transforms, one frame chain per 512 work-items, two chains per workgroup but for the T128_STAGGER=0 launch (spectrum_geom.h)
        const bool one_chain = !df && !last_fullc && !raw && stagger <= 0;
        const SpectrumGeom geo = spectrum_geometry(one_chain ? SpecFamily::t128_one : SpecFamily::t128, F, S, bins, nf, S);
        sp.frames_per_group = geo.G;
        sp.scale = scale;
        sp.out_pitch = F * (long long)bins;
        const RawSrc rs = raw ? *raw : RawSrc{nullptr, 0, 0, 0.f, 0};
        const float *pin = d_prev[parity];
        float *pout = d_prev[parity ^ 1];
        DecFuse none;
        memset(&none, 0, sizeof(none));
        const DecFuse &dfv = df ? *df : none;
        // two chains per 1024-item workgroup, the second `st` barrier intervals behind the first
        auto go = [&](auto kern, int st) {
            launch(kern, dim3(geo.wgs, S), dim3(1024), s, d_in, d_out, (const float *)d_window, (const float2 *)d_btab128, (const float2 *)d_tw128, pin, pout, sp, st, rs, dfv);
        };
        if (df)  // the one-channel decimator rides in the transform's workgroups (every sample format)
            with_sample_fmt(raw, [&](auto F) { go(k_spectrum_t128<2, F.value, true>, stagger > 0 ? stagger : 3); });
        else if (last_fullc)
            // nothing is to run beside this launch: pass C's fifteen twiddles per work-item formed once and held (126 registers: four such
            // waves fill a SIMD's register file) -- 0.200 ms for the bench batch against 0.224
            with_sample_fmt(raw, [&](auto F) { go(k_spectrum_t128<2, F.value, false, true>, stagger > 0 ? stagger : 3); });
        else if (raw)  // raw-format frames take the two-chain kernel (one instantiation per sample format)
            with_raw_fmt(raw->fmt, [&](auto F) { go(k_spectrum_t128<2, F.value>, stagger > 0 ? stagger : 7); });
        else if (stagger > 0)
            go(k_spectrum_t128<2, -1>, stagger);
        else
            launch_lds(k_spectrum_t128<1, -1>, dim3(geo.wgs, S), dim3(512), (size_t)pad_lds, s, d_in, d_out, (const float *)d_window,
                       (const float2 *)d_btab128, (const float2 *)d_tw128, pin, pout, sp, 0, rs, dfv);
        parity ^= 1;
        PG_HIP(hipGetLastError());
        return 0;
    }
    const SpectrumGeom geo = spectrum_geometry(SpecFamily::waves, F, S, bins, nf, S);  // 4 / ZP wave groups (frames in flight) per workgroup
    sp.frames_per_group = geo.G;
    sp.scale = scale;
    sp.out_pitch = F * (long long)bins;
    const dim3 grid(geo.wgs, S), block(256);
    const float *pin = d_prev[parity];
    float *pout = d_prev[parity ^ 1];
    if (bins == 2048) launch(k_spectrum_1to1, grid, block, s, d_in, d_out, (const float *)d_window, (const float2 *)d_tw_nf, pin, pout, sp);
    else if (bins == 4096) launch(k_spectrum<2>, grid, block, s, d_in, d_out, (const float *)d_window, (const float2 *)d_btab, (const float2 *)d_tw_nf, pin, pout, sp);
    else return fail(PEBBLEGPU_E_UNSUPPORTED, "no spectrum kernel for %u bins", bins);
    parity ^= 1;
    PG_HIP(hipGetLastError());
    return 0;
}

// The tables of k_spectrum_list_q128 for a plan whose own kernels use others (4096 and 8192 bins); synchronous, once, from the setter
int SpectrumCore::init_list()
{
    if (big || any || d_list_ftab) return 0;  // (the 65536-point listed transform needs no table of its own)
    if (per_q) {  // k_spectrum_q128's own
        d_list_ftab = d_ftab;
        d_list_tw128 = d_tw128;
        return 0;
    }
    const std::vector<float2> ft = factor_table(std::vector<double>(h_window.begin(), h_window.end()), nf, bins);
    PG_TRY(own_list_ftab.upload(ft.data(), ft.size()));
    PG_TRY(make_twiddles_t128(own_list_tw128));
    d_list_ftab = own_list_ftab;
    d_list_tw128 = own_list_tw128;
    return 0;
}
// The 65536-point transform of the listed frames: pass A reads the listed frames and leaves COMPACT rows in Y ([stream][n_sel][k1][n2],
// k_big256_cols_list, kListMax frames per launch), pass B is run()'s k_big256_rows over those n_sel rows -- its chains take a row's
// predecessor from the row in front or from the carried amplitudes, and the last row leaves its own there.  Y, the stream batches and
// the chain length follow run()'s rules with n_sel in place of the call's frame count.  Under PEBBLEGPU_BIG_SPLIT32 these kernels run
// all the same.
int SpectrumCore::run_list_big(hipStream_t s, const float2 *d_in, long long in_pitch, const uint32_t *idx, long long n_sel, float *d_out, const RawSrc *raw)
{
    if (raw && !raw_ready_big()) return fail(PEBBLEGPU_E_INVALID, "raw-format input reached a spectrum kernel that has no converting loads");
    long long bs = 0;  // streams per batch
    PG_TRY(size_Y(s, n_sel * kBigN, &bs));
    const SpectrumGeom geo = spectrum_geometry(SpecFamily::big, n_sel, S, bins, nf, bs);
    SpectrumParams sp;
    sp.in_pitch = in_pitch;
    sp.n_frames = n_sel;
    sp.frames_per_group = geo.G;
    sp.scale = scale;
    sp.out_pitch = n_sel * (long long)bins;
    const bool b8 = raw && (raw->fmt == 0 || raw->fmt == 1);  // 8-bit pairs: the paired tile order (kernels_spectrum.h)
    for (long long s0 = 0; s0 < (long long)S; s0 += bs) {
        const unsigned nb = (unsigned)((long long)S - s0 < bs ? (long long)S - s0 : bs);
        RawSrc rs = raw ? *raw : RawSrc{nullptr, 0, 0, 0.f, 0};
        if (raw) rs.base = static_cast<const char *>(raw->base) + (size_t)(s0 * in_pitch) * kRawPairBytes[raw->fmt];
        const float2 *in0 = raw ? nullptr : d_in + s0 * in_pitch;
        for (long long r0 = 0; r0 < n_sel; r0 += kListMax) {
            FrameList fl;
            memset(&fl, 0, sizeof(fl));
            fl.n = (int)(n_sel - r0 < kListMax ? n_sel - r0 : kListMax);
            fl.row0 = (int)r0;
            fl.pred = -1;  // (pass B finds the predecessors)
            for (int i = 0; i < fl.n; i++) fl.idx[i] = idx[r0 + i];
            const dim3 grid(b8 ? (unsigned)(16 * cdiv(fl.n, 2)) : (unsigned)(fl.n * 8), nb);
            auto go = [&](auto kern) { launch(kern, grid, dim3(256), s, in0, (long long)in_pitch, d_Y, (const float *)d_window, (long long)n_sel, fl, rs); };
            with_sample_fmt(raw, [&](auto F) { go(k_big256_cols_list<F.value>); });
        }
        launch(k_big256_rows, dim3(geo.wgs, nb), dim3(256), s, (const float2 *)d_Y, d_out + s0 * sp.out_pitch,
               (const float *)d_prev[parity] + s0 * kBigN, d_prev[parity ^ 1] + s0 * kBigN, sp);
    }
    parity ^= 1;
    PG_HIP(hipGetLastError());
    return 0;
}
// FFT::fftSpectrum of the listed frames only (ascending, relative to d_in's first frame), rows compact in d_out: [stream][n_sel][bins]
int SpectrumCore::run_list(hipStream_t s, const float2 *d_in, long long in_pitch, const uint32_t *idx, long long n_sel, float *d_out, const RawSrc *raw)
{
    if (n_sel <= 0) return 0;  // nothing is queued and the carried amplitudes stay
    if (big) return run_list_big(s, d_in, in_pitch, idx, n_sel, d_out, raw);
    if (any && raw) return fail(PEBBLEGPU_E_INVALID, "the general display transform takes float2 input");
    if (!any && !d_list_ftab) return fail(PEBBLEGPU_E_INVALID, "the frame-list transform was not set up");
    SpectrumParams sp;
    sp.in_pitch = in_pitch;
    sp.n_frames = n_sel;
    sp.frames_per_group = 1;
    sp.scale = scale;
    sp.out_pitch = n_sel * (long long)bins;
    const RawSrc rs = raw ? *raw : RawSrc{nullptr, 0, 0, 0.f, 0};
    const float *pin = d_prev[parity];
    float *pout = d_prev[parity ^ 1];
    for (long long r0 = 0; r0 < n_sel; r0 += kListMax) {
        FrameList fl;
        memset(&fl, 0, sizeof(fl));
        fl.n = (int)(n_sel - r0 < kListMax ? n_sel - r0 : kListMax);
        fl.row0 = (int)r0;
        fl.pred = r0 ? (long long)idx[r0 - 1] : -1;
        fl.last = r0 + fl.n == n_sel ? 1 : 0;
        for (int i = 0; i < fl.n; i++) fl.idx[i] = idx[r0 + i];
        if (any) {
            AnySpecParams ap;
            ap.n_in = (int)nf;
            ap.frame = (int)nf;
            ap.M = any_M;
            ap.logM = any_logM;
            ap.zp_log2 = any_zp_log2;
            ap.windowed = 1;
            launch_lds(k_spectrum_list_any, dim3((unsigned)fl.n << any_zp_log2, S), dim3(256), sizeof(float2) * (size_t)any_M, s, d_in, d_out, (const float *)d_window,
                       (const float2 *)d_twM, pin, pout, sp, ap, fl);
        } else {
            int zl = 0;
            while (((uint32_t)nf << zl) < bins) zl++;
            const dim3 grid((unsigned)fl.n << zl, S), block(128);
            if (raw) launch(k_spectrum_list_q128<true>, grid, block, s, d_in, d_out, (const float2 *)d_list_ftab, (const float2 *)d_list_tw128, pin, pout, sp, zl, fl, rs);
            else launch(k_spectrum_list_q128<false>, grid, block, s, d_in, d_out, (const float2 *)d_list_ftab, (const float2 *)d_list_tw128, pin, pout, sp, zl, fl, rs);
        }
    }
    parity ^= 1;
    PG_HIP(hipGetLastError());
    return 0;
}

}  // namespace pg
