// streambank.hip -- S full-rate streams through CFastFIR + fftSpectrum (include/pebblegpu.h, "Stream bank").
#include <new>
#include <cmath>
#include "receiver.h"

using pg::fail;

struct pebblegpu_streambank {
    pebblegpu_streambank_config cfg{};
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // the band-pass of a call that also asks for the spectrum runs here, beside the transform
    bool side_ok = true, side = false;
    pg::FastFirCore ff;
    pg::SpectrumCore sp;
    float2 *d_tail = nullptr, *d_tail_alt = nullptr, *d_filt = nullptr;  // (the two overlap buffers swap after every band-pass call)
    float *d_spec = nullptr;
    uint64_t cap = 0, last_n = 0, last_frames = 0;
    hipEvent_t ev[4] = {};
    bool timed = false;
    float2 *d_raw_stage = nullptr;   // raw calls of a geometry without converting loads: the normalised copy (allocated on first use)
    pg::IngestRing ingest;           // the pinned double buffer of pebblegpu_streambank_ingest_* (ingest.h)
    int last_fmt = -1;               // the last call's route, for pebblegpu_streambank_kernel_name: -1 float2 input, else the raw format
    bool last_staged = false, last_bp = false, last_sp = false;
    // the spectrum's update gate (pebblegpu_streambank_set_spectrum_updates): one timer on the bank's sample clock, all streams select
    // the same frames.  With a gate last_frames counts the COMPUTED rows of the last call, d_spec holds them compact.
    int ups = -1;
    uint64_t period_ms = 100;        // 1000 / updates_per_sec of the last rate above 0 (the reference's default: 10 per second)
    pg::UpdateTimer ut;
    std::vector<uint32_t> sel;       // the last call's selection, relative to its first frame
    bool last_listed = false;        // the last call's transform went through the frame-list kernels (or, sel empty, through none)
    uint64_t spec_rows = 0;          // rows per stream of what d_spec holds (the last call that computed any): its last row is the latest spectrum
};

// every kernel a raw call would run converts in its own loads (else the call is staged through k_normalize_iq as a whole)
static bool sb_converts(const pebblegpu_streambank *sb) { return sb->ff.raw_ready() && (sb->sp.raw_ready() || sb->sp.raw_ready_big()); }

extern "C" {

int pebblegpu_streambank_destroy(pebblegpu_streambank *sb)
{
    if (!sb) return 0;
    (void)hipSetDevice(sb->cfg.device);
    if (sb->stream2) {
        (void)hipStreamSynchronize(sb->stream2);
        (void)hipStreamDestroy(sb->stream2);
    }
    if (sb->stream) {
        (void)hipStreamSynchronize(sb->stream);
        (void)hipStreamDestroy(sb->stream);
    }
    sb->ff.release();
    sb->sp.release();
    sb->ingest.release();
    void *p[] = {sb->d_tail, sb->d_tail_alt, sb->d_filt, sb->d_spec, sb->d_raw_stage};
    for (void *q : p) if (q) (void)hipFree(q);
    for (hipEvent_t e : sb->ev) if (e) (void)hipEventDestroy(e);
    delete sb;
    return 0;
}

int pebblegpu_streambank_create(const pebblegpu_streambank_config *cfg, pebblegpu_streambank **out)
{
    if (!cfg || !out) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (cfg->struct_size != sizeof(pebblegpu_streambank_config)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_streambank_config size mismatch");
    if (!cfg->n_streams || !cfg->frame || !cfg->max_frames || !(cfg->sample_rate > 0)) return fail(PEBBLEGPU_E_INVALID, "bad stream bank configuration");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PEBBLEGPU_E_NO_DEVICE, "no HIP device");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(PEBBLEGPU_E_INVALID, "device %d out of range", cfg->device);
    pebblegpu_streambank *sb = new (std::nothrow) pebblegpu_streambank();
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "out of host memory");
    sb->cfg = *cfg;
    if (!sb->cfg.fastfir_fft) sb->cfg.fastfir_fft = 2048;
    if (!sb->cfg.fastfir_taps) sb->cfg.fastfir_taps = 1025;
    const uint32_t S = cfg->n_streams;
    sb->cap = (uint64_t)cfg->frame * cfg->max_frames;
    int rc = 0;
    auto body = [&]() -> int {
        PG_HIP(hipSetDevice(cfg->device));
        PG_HIP(hipStreamCreateWithFlags(&sb->stream, hipStreamNonBlocking));
        PG_HIP(hipStreamCreateWithFlags(&sb->stream2, hipStreamNonBlocking));
        const pg::Tuning tun = pg::read_tuning();
        sb->side_ok = tun.sb_side;  // opt-in: measured equal (below)
        if (int r = sb->ff.init(S, sb->cfg.fastfir_fft, sb->cfg.fastfir_taps, tun)) return r;
        if (int r = sb->sp.init(S, cfg->frame, cfg->spectrum_bins, tun)) return r;
        if (cfg->frame % (uint64_t)sb->ff.block_len()) return fail(PEBBLEGPU_E_SIZE, "frame %u is not a multiple of the band-pass block %lld", cfg->frame, sb->ff.block_len());
        const size_t ov = sb->cfg.fastfir_taps - 1;
        PG_HIP(hipMalloc((void **)&sb->d_tail, sizeof(float2) * ov * S));
        PG_HIP(hipMemset(sb->d_tail, 0, sizeof(float2) * ov * S));  // m_pFFTOverlapBuf starts at zero, fastfir.cpp:104-105
        PG_HIP(hipMalloc((void **)&sb->d_tail_alt, sizeof(float2) * ov * S));
        PG_HIP(hipMemset(sb->d_tail_alt, 0, sizeof(float2) * ov * S));
        PG_HIP(hipMalloc((void **)&sb->d_filt, sizeof(float2) * sb->cap * S));
        PG_HIP(hipMalloc((void **)&sb->d_spec, sizeof(float) * (size_t)sb->sp.bins * cfg->max_frames * S));
        for (hipEvent_t &e : sb->ev) PG_HIP(hipEventCreate(&e));
        // CFastFIR's constructor state: lo -1, hi 1, offset 1, rate 1 -> an all-zero filter until the first setup
        return 0;
    };
    rc = body();
    if (rc) { pebblegpu_streambank_destroy(sb); return rc; }
    *out = sb;
    return 0;
}

int pebblegpu_streambank_set_bandpass(pebblegpu_streambank *sb, uint32_t stream, double lo, double hi)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (stream >= sb->cfg.n_streams) return fail(PEBBLEGPU_E_INVALID, "stream %u out of range", stream);
    PG_HIP(hipSetDevice(sb->cfg.device));
    bool ok = false;
    if (int rc = sb->ff.design(sb->stream, stream, lo, hi, 0.0, sb->cfg.sample_rate, &ok)) return rc;
    if (!ok) return fail(PEBBLEGPU_E_FILTER_PARAM, "Filter Parameter error (lo %g hi %g rate %g)", lo, hi, sb->cfg.sample_rate);
    return 0;
}

int pebblegpu_streambank_set_spectrum_updates(pebblegpu_streambank *sb, int updates_per_sec)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (updates_per_sec < -1) return fail(PEBBLEGPU_E_INVALID, "updates per second: -1 (every frame), 0 (none) or a rate");
    PG_HIP(hipSetDevice(sb->cfg.device));
    if (updates_per_sec != -1) { if (int rc = sb->sp.init_list()) return rc; }
    if (updates_per_sec > 0) sb->period_ms = (uint64_t)(1000 / updates_per_sec);  // integer division, as the reference computes it
    sb->ups = updates_per_sec;
    return 0;
}
int pebblegpu_streambank_spectrum_frames(const pebblegpu_streambank *sb, uint32_t *idx, uint32_t cap, uint32_t *n)
{
    if (!sb || !n) return fail(PEBBLEGPU_E_INVALID, "null argument");
    *n = 0;
    const uint64_t rows = sb->last_frames;
    if (rows > cap) return fail(PEBBLEGPU_E_SIZE, "%llu frames do not fit %u entries", (unsigned long long)rows, cap);
    if (rows && !idx) return fail(PEBBLEGPU_E_INVALID, "null argument");
    for (uint64_t i = 0; i < rows; i++) idx[i] = sb->last_listed ? sb->sel[i] : (uint32_t)i;  // (without the gate every frame of the call has its row)
    *n = (uint32_t)rows;
    return 0;
}

// the checks every process call makes before anything is queued
static int sb_check_n(const pebblegpu_streambank *sb, uint64_t n)
{
    if (n % sb->cfg.frame) return fail(PEBBLEGPU_E_SIZE, "n_samples %llu is not a multiple of the frame %u", (unsigned long long)n, sb->cfg.frame);
    if (n > sb->cap) return fail(PEBBLEGPU_E_SIZE, "n_samples %llu above the capacity %llu", (unsigned long long)n, (unsigned long long)sb->cap);
    return 0;
}
// one call: float2 rows `in`, or (raw != nullptr) rows still in the device's sample format that the kernels convert in their loads
static int sb_run(pebblegpu_streambank *sb, const float2 *in, const pg::RawSrc *raw, uint64_t n, uint32_t what)
{
    sb->last_n = 0;
    sb->last_frames = 0;
    if (n == 0) return 0;
    // The update timer, on the host before anything is queued.  A call without the spectrum advances the sample clock and nothing else:
    // it selects no frame and neither starts nor restarts the timer.
    const uint64_t F = n / sb->cfg.frame;
    sb->sel.clear();
    sb->last_listed = (what & 2u) && sb->ups != -1;
    if (what & 2u) sb->ut.advance(sb->ups, sb->period_ms, F, sb->cfg.frame, (uint64_t)std::llround(sb->cfg.sample_rate), &sb->sel);
    else sb->ut.next += F;
    PG_HIP(hipEventRecord(sb->ev[0], sb->stream));
    // Both asked for: the band-pass (bound by its two transforms per block: vector units + LDS) and the display transform (the 65536-point
    // one is bound by what it moves through HBM) read the same input and share nothing else.  Side by side on two streams (fork at the
    // call's start event, join at its end; PEBBLEGPU_SB_SIDE=1 when the bank is created) they do NOT overlap: 0.4345 / 0.4368 ms per
    // configs[4] call against 0.4346 / 0.4422 one after the other -- the band-pass's 32768 small workgroups fill every CU's LDS first and the
    // transform's workgroups wait for them; with the band-pass's occupancy cut (8 / 16 / 30 kB of extra LDS per workgroup) both get slower
    // (0.46 / 0.48 / 0.52).  Opt-in, not the default.
    const bool side = sb->side_ok && (what & 3u) == 3u;
    sb->side = side;
    hipStream_t fs = side ? sb->stream2 : sb->stream;
    if (side) PG_HIP(hipStreamWaitEvent(fs, sb->ev[0], 0));
    sb->last_bp = (what & 1u) != 0;
    sb->last_sp = (what & 2u) != 0;
    if (what & 1u) {
        float2 *next = sb->ff.fft_n == 2048 ? sb->d_tail_alt : nullptr;
        if (int rc = sb->ff.run_ext(fs, in, (long long)n, sb->d_tail, (long long)n, sb->d_filt, (long long)n, next, raw)) return rc;
        if (next) std::swap(sb->d_tail, sb->d_tail_alt);
        sb->last_n = n;
    }
    PG_HIP(hipEventRecord(sb->ev[1], fs));
    if (sb->last_listed) {  // the listed frames only, rows compact (an empty list queues nothing and leaves d_spec and the carried amplitudes alone)
        if (int rc = sb->sp.run_list(sb->stream, in, (long long)n, sb->sel.data(), (long long)sb->sel.size(), sb->d_spec, raw)) return rc;
        sb->last_frames = sb->sel.size();
    } else if (what & 2u) {
        if (int rc = sb->sp.run(sb->stream, in, (long long)n, (long long)F, sb->d_spec, raw, nullptr, !side)) return rc;
        sb->last_frames = F;
    }
    if (sb->last_frames) sb->spec_rows = sb->last_frames;
    if (side) {
        PG_HIP(hipEventRecord(sb->ev[3], sb->stream));       // where the transform ended
        PG_HIP(hipStreamWaitEvent(sb->stream, sb->ev[1], 0));  // join
    }
    PG_HIP(hipEventRecord(sb->ev[2], sb->stream));
    sb->timed = true;
    return 0;
}

int pebblegpu_streambank_process(pebblegpu_streambank *sb, const void *d_iq, uint64_t n, uint32_t what)
{
    if (!sb || (!d_iq && n)) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (int rc = sb_check_n(sb, n)) return rc;
    PG_HIP(hipSetDevice(sb->cfg.device));
    sb->last_fmt = -1;
    sb->last_staged = false;
    return sb_run(sb, static_cast<const float2 *>(d_iq), nullptr, n, what);
}

// the argument checks of a raw call, before anything is queued
static int sb_check_raw(const pebblegpu_streambank *sb, int fmt, int order, const void *d_raw, uint64_t n)
{
    if (!d_raw && n) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (fmt < 0 || fmt > 4 || order < 0 || order > 3) return fail(PEBBLEGPU_E_INVALID, "unknown sample format %d / IQ order %d", fmt, order);
    if (int rc = sb_check_n(sb, n)) return rc;
    if (reinterpret_cast<uintptr_t>(d_raw) % PEBBLEGPU_RAW_ALIGN) return fail(PEBBLEGPU_E_INVALID, "d_raw must be aligned to %d bytes", PEBBLEGPU_RAW_ALIGN);
    return 0;
}
// a raw call behind its checks.  Where every kernel converts in its loads no float2 copy of the streams exists; every other geometry is
// staged as a whole: k_normalize_iq on the bank's stream into a float2 buffer of the bank's capacity, then the ordinary call.
// Either way the band-pass's overlap buffers hold CONVERTED samples, so raw and float2 calls continue each other.
static int sb_run_raw(pebblegpu_streambank *sb, int fmt, int order, double gain, const void *d_raw, uint64_t n, uint32_t what)
{
    const pg::RawSrc raw{d_raw, fmt, order, pg::raw_scale(fmt, gain), 0};
    sb->last_fmt = fmt;
    sb->last_staged = !sb_converts(sb);
    if (!sb->last_staged || n == 0) return sb_run(sb, nullptr, &raw, n, what);
    const size_t S = sb->cfg.n_streams;
    if (!sb->d_raw_stage) PG_HIP(hipMalloc((void **)&sb->d_raw_stage, sizeof(float2) * S * sb->cap));
    // (the rows of d_raw are n pairs apart, so S * n pairs are one run; the side stream forks behind it, at the call's start event)
    if (int rc = pg::run_normalize_iq(fmt, order, 1.0, d_raw, (long long)(S * n), sb->d_raw_stage, sb->stream, false, &raw.scale)) return rc;
    return sb_run(sb, sb->d_raw_stage, nullptr, n, what);
}

int pebblegpu_streambank_process_raw(pebblegpu_streambank *sb, int format, int iq_order, double gain, const void *d_raw, uint64_t n, uint32_t what)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (int rc = sb_check_raw(sb, format, iq_order, d_raw, n)) return rc;
    PG_HIP(hipSetDevice(sb->cfg.device));
    return sb_run_raw(sb, format, iq_order, gain, d_raw, n, what);
}

int pebblegpu_streambank_ingest_acquire(pebblegpu_streambank *sb, uint32_t slot, uint64_t bytes, void **host_ptr)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    return sb->ingest.acquire(sb->cfg.device, slot, bytes, host_ptr);
}
int pebblegpu_streambank_ingest_submit(pebblegpu_streambank *sb, uint32_t slot, uint64_t bytes)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    return sb->ingest.submit(sb->cfg.device, slot, bytes);
}
int pebblegpu_streambank_process_ingested(pebblegpu_streambank *sb, uint32_t slot, int format, int iq_order, double gain, uint64_t n, uint32_t what)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    pg::IngestSlot *g = nullptr;
    if (int rc = sb->ingest.check(slot, format, (uint64_t)sb->cfg.n_streams * n, n, &g)) return rc;
    if (int rc = sb_check_raw(sb, format, iq_order, g->d, n)) return rc;
    PG_HIP(hipSetDevice(sb->cfg.device));
    // both streams may read the raw samples (PEBBLEGPU_SB_SIDE=1: the band-pass runs on the second one)
    if (int rc = sb->ingest.wait_upload(*g, sb->stream, sb->stream2)) return rc;
    if (int rc = sb_run_raw(sb, format, iq_order, gain, g->d, n, what)) return rc;
    return sb->ingest.mark_in_flight(*g, sb->stream, sb->stream2);
}

const char *pebblegpu_streambank_kernel_name(const pebblegpu_streambank *sb, int which)
{
    if (!sb || !sb->timed) return "";
    static const char *const kFf[6] = {"k_fastfir_t128", "k_fastfir_t128 (raw s8)", "k_fastfir_t128 (raw u8)", "k_fastfir_t128 (raw s16)",
                                       "k_fastfir_t128 (raw f32)", "k_fastfir_t128 (raw wav16)"};
    static const char *const kBig[6] = {"k_big256_cols + k_big256_rows", "k_big256_cols (raw s8) + k_big256_rows", "k_big256_cols (raw u8) + k_big256_rows",
                                        "k_big256_cols (raw s16) + k_big256_rows", "k_big256_cols (raw f32) + k_big256_rows",
                                        "k_big256_cols (raw wav16) + k_big256_rows"};
    static const char *const kT128[6] = {"k_spectrum_t128", "k_spectrum_t128 (raw s8)", "k_spectrum_t128 (raw u8)", "k_spectrum_t128 (raw s16)",
                                         "k_spectrum_t128 (raw f32)", "k_spectrum_t128 (raw wav16)"};
    static const char *const kW64[6] = {"k_spectrum_w64", "k_spectrum_w64 (raw s8)", "k_spectrum_w64 (raw u8)", "k_spectrum_w64 (raw s16)",
                                        "k_spectrum_w64 (raw f32)", "k_spectrum_w64 (raw wav16)"};
    const int r = sb->last_fmt >= 0 && !sb->last_staged ? sb->last_fmt + 1 : 0;  // 0: the float2 instances
    const pg::SpectrumCore &sp = sb->sp;
    if (which == 1) {
        if (!sb->last_bp) return "";
        if (sb->ff.fft_n == 2048) return sb->last_staged ? "k_normalize_iq + k_fastfir_t128" : kFf[r];
        return sb->last_staged ? "k_normalize_iq + k_fastfir" : "k_fastfir";
    }
    if (which == 2 && sb->last_sp && sb->last_listed) {  // a gated call: the frame-list kernels, or none
        static const char *const kBigL[6] = {"k_big256_cols_list + k_big256_rows", "k_big256_cols_list (raw s8) + k_big256_rows",
                                             "k_big256_cols_list (raw u8) + k_big256_rows", "k_big256_cols_list (raw s16) + k_big256_rows",
                                             "k_big256_cols_list (raw f32) + k_big256_rows", "k_big256_cols_list (raw wav16) + k_big256_rows"};
        static const char *const kQ128L[6] = {"k_spectrum_list_q128", "k_spectrum_list_q128 (raw s8)", "k_spectrum_list_q128 (raw u8)",
                                              "k_spectrum_list_q128 (raw s16)", "k_spectrum_list_q128 (raw f32)", "k_spectrum_list_q128 (raw wav16)"};
        if (!sb->last_frames) return "";
        if (sp.big) return sb->last_staged ? "k_normalize_iq + k_big256_cols_list + k_big256_rows" : kBigL[r];
        if (sp.any) return sb->last_staged ? "k_normalize_iq + k_spectrum_list_any" : "k_spectrum_list_any";
        return sb->last_staged ? "k_normalize_iq + k_spectrum_list_q128" : kQ128L[r];
    }
    if (which == 2) {
        if (!sb->last_sp) return "";
        if (sp.big && sp.tun.big_split32) return sb->last_staged ? "k_normalize_iq + k_big_cols + k_big_rows" : "k_big_cols + k_big_rows";
        if (sp.big) return sb->last_staged ? "k_normalize_iq + k_big256_cols + k_big256_rows" : kBig[r];
        if (sp.any) return sb->last_staged ? "k_normalize_iq + k_spectrum_any" : "k_spectrum_any";
        if (sp.per_q) return sb->last_staged ? "k_normalize_iq + k_spectrum_q128" : "k_spectrum_q128";
        if (sp.bins == 8192) return sb->last_staged ? (sp.use_w64 ? "k_normalize_iq + k_spectrum_w64" : "k_normalize_iq + k_spectrum_t128") : sp.use_w64 ? kW64[r] : kT128[r];
        if (sp.bins == 4096) return sb->last_staged ? "k_normalize_iq + k_spectrum<2>" : "k_spectrum<2>";
        return sb->last_staged ? "k_normalize_iq + k_spectrum_1to1" : "k_spectrum_1to1";
    }
    return "";
}

const void *pebblegpu_streambank_filtered(const pebblegpu_streambank *sb, uint64_t *n, uint64_t *pitch)
{
    if (!sb) return nullptr;
    if (n) *n = sb->last_n;
    if (pitch) *pitch = sb->last_n;
    return sb->d_filt;
}
const void *pebblegpu_streambank_spectrum(const pebblegpu_streambank *sb, uint64_t *frames, uint32_t *bins)
{
    if (!sb) return nullptr;
    if (frames) *frames = sb->last_frames;
    if (bins) *bins = sb->sp.bins;
    return sb->d_spec;
}
int pebblegpu_streambank_last_ms(const pebblegpu_streambank *sb, int which, float *ms)
{
    if (!sb || !ms) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (!sb->timed) return fail(PEBBLEGPU_E_INVALID, "no process call yet");
    if (which < 0 || which > 2) return fail(PEBBLEGPU_E_INVALID, "which must be 0..2");
    PG_HIP(hipSetDevice(sb->cfg.device));
    PG_HIP(hipEventSynchronize(sb->ev[2]));
    // side by side both groups start at the call's start event; the transform's own end is ev[3]
    const int a = (which == 2 && !sb->side) ? 1 : 0, b = which == 1 ? 1 : (which == 2 && sb->side ? 3 : 2);
    PG_HIP(hipEventElapsedTime(ms, sb->ev[a], sb->ev[b]));
    return 0;
}
int pebblegpu_streambank_map_spectrum(pebblegpu_streambank *sb, const pebblegpu_screen_map *map, uint32_t first_frame, uint32_t n_frames,
                                      uint32_t frame_step, int32_t *d_out)
{
    if (!sb || !map || !d_out) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (map->struct_size != sizeof(pebblegpu_screen_map)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_screen_map size mismatch");
    if (int rc = pg::check_screen_map(map->y_pixels, map->x_pixels, map->max_db, map->min_db)) return rc;
    // a gated call that asked for the spectrum and selected nothing left d_spec alone: the latest row computed before it (the last of
    // the spec_rows it holds) is mapped as frame 0 -- what the display still shows
    const bool latest = !sb->last_frames && sb->last_sp && sb->last_listed && sb->spec_rows;
    const uint64_t rows = latest ? 1 : sb->last_frames, pitch_rows = latest ? sb->spec_rows : sb->last_frames;
    if (!rows) return fail(PEBBLEGPU_E_INVALID, "the last call computed no spectrum (or no call has been made yet)");
    if (n_frames == 0 || (uint64_t)first_frame + (uint64_t)(n_frames - 1) * frame_step >= rows)
        return fail(PEBBLEGPU_E_INVALID, "frames %u + j * %u, j < %u, are not all within the last call's %llu", first_frame, frame_step, n_frames,
                    (unsigned long long)rows);
    PG_HIP(hipSetDevice(sb->cfg.device));
    const long long bins = sb->sp.bins;
    const int32_t edges[2] = {map->start_freq, map->stop_freq};
    if (latest) first_frame = (uint32_t)(sb->spec_rows - 1);
    // on the bank's stream, behind the call's transform (and its join) and ahead of the next call's
    return pg::run_screen_map(sb->stream, sb->d_spec + (long long)first_frame * bins, (long long)pitch_rows * bins, (long long)frame_step * bins,
                              (int)sb->cfg.n_streams, (int)n_frames, (int32_t)bins, sb->cfg.sample_rate, edges, false, map->y_pixels, map->x_pixels,
                              map->max_db, map->min_db, d_out);
}
int pebblegpu_streambank_synchronize(pebblegpu_streambank *sb)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    PG_HIP(hipSetDevice(sb->cfg.device));
    PG_HIP(hipStreamSynchronize(sb->stream));
    PG_HIP(hipStreamSynchronize(sb->stream2));
    return 0;
}

}  // extern "C"
