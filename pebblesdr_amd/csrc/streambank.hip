// streambank.hip -- S full-rate streams through CFastFIR + fftSpectrum (include/pebblegpu.h, "Stream bank").
#include <new>
#include <cmath>
#include "kernels_display.h"
#include "kernels_strength.h"
#include "kernels_condition.h"
#include "receiver.h"
#include "design.h"
#include <string>

using pg::fail;

struct pebblegpu_streambank {
    pebblegpu_streambank_config cfg{};
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // the band-pass of a call that also asks for the spectrum runs here, beside the transform
    bool side_ok = true, side = false;
    pg::FastFirCore ff;
    pg::SpectrumCore sp;
    pg::DevBuf<float2> d_tail, d_tail_alt, d_filt;  // (the two overlap buffers swap after every band-pass call)
    pg::DevBuf<float> d_spec;
    uint64_t cap = 0, last_n = 0, last_frames = 0;
    hipEvent_t ev[5] = {};           // (ev[4]: behind the conditioners, where a side-by-side call forks)
    bool timed = false;
    pg::DevBuf<float2> d_raw_stage;  // raw calls of a geometry without converting loads: the normalised copy (allocated on first use)
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
    // host egress (egress.h): the band-passed IQ of selected streams and the display rows of a call's spectra, one block per call each
    pg::EgressRing iq_ring, disp_ring;
    pg::DevBuf<uint32_t> d_iq_tab;   // d_iq_tab[r] = the stream of block row r (written at open)
    int iq_fmt = 0;
    pg::DisplayPack disp;            // format, selection table, plot geometry of the display ring
    pg::DevBuf<uint32_t> d_disp_tab; // ... the table disp.d_tab looks at
    uint32_t disp_max_rows = 0;
    // the display ring's auto-scale (SpectrumWidget::recalcScale, kernels_display.h): host flags consumed when the next call is queued
    uint32_t scale_flags = 0, scale_live = 0;  // PEBBLEGPU_AUTO_SCALE_* as last set; those whose end a recalc has computed since
    bool scale_pending = false;      // m_scaleNeedsRecalc
    pg::DevBuf<pg::ScaleEntry> d_scale; // [n_streams] the ranges (allocated with the ring)
    uint64_t trailer_bytes = 0;      // per slot, behind the rows
    bool slot_scaled[pg::kEgressMaxSlots] = {};  // the slot's block carries a trailer
    // the S-meter and the squelch (kernels_strength.h): host state consumed when the next call is queued, like the auto-scale flags
    bool sm_on = false;
    std::vector<float> bp_lo, bp_hi;     // per stream, as the last accepted set_bandpass left them (CFastFIR's constructor state: -1, 1)
    std::vector<float> squelch;          // per stream; -120 and below never closes
    uint32_t n_squelch = 0;              // thresholds above -120: while there are any the IQ ring packs through the gated instance
    bool win_dirty = true, sq_dirty = true;
    pg::DevBuf<pg::SmBins> d_win;        // [n_streams] fdEstimate's windows
    pg::DevBuf<float> d_squelch;         // [n_streams]
    pg::DevBuf<float4> d_smeter;         // [n_streams][max_frames]: one entry per row the last call computed
    pg::DevBuf<float4> d_carry[2];       // [n_streams] each: the last computed entry per stream.  A call that computes rows writes the other
    int carry_cur = 0;                   // one, so its own gate still reads what earlier calls left; then they swap
    bool have_row = false;               // d_carry[carry_cur] holds a row (computed since the S-meter went on)
    uint64_t sm_rows = 0;                // entries per stream the last call wrote
    // table uploads that never wait for earlier calls: pinned staging slots, each reused once the copy queued from it has completed
    static constexpr int kStage = 4;
    pg::PinnedBuf<unsigned char> h_stage[kStage];
    hipEvent_t stage_ev[kStage] = {};
    int stage_next = 0;
    // the input conditioners (kernels_condition.h): host flags consumed when the next call is queued; the setter touches no device state
    struct CondHost { int flags = 0, reset = 0; double gain = 1.0, phase = 0.0; };
    std::vector<CondHost> cond;          // per stream
    uint32_t n_cond = 0;                 // streams with a flag set: while there are any every call conditions its samples first
    bool cond_dirty = false;             // a setter changed something since the last upload
    bool cond_ready = false;             // the state block holds the constructors' values (written on the stream by the first conditioned call)
    int cond_mask = 0;                   // the flags of all streams or'ed, as last uploaded
    pg::ScanParams<1> cond_dc;           // DCRemoval's high-pass
    pg::CondAvg cond_mag{}, cond_cpx{};  // the blankers' averages
    double cond_m[4] = {};               // the high-pass's transition matrix on (w1, w1 - w2) to the power of a chunk
    float2 *d_cond[2] = {};              // views, [n_streams][capacity] each: of d_cond0 and of d_raw_stage (allocated on first use, either way)
    pg::DevBuf<float2> d_cond0;
    pg::DevBuf<pg::CondPar> d_cond_par;
    pg::DevBuf<pg::CondState> d_cond_state;
    pg::DevBuf<double> d_cond_sum, d_cond_entry;  // [n_streams][chunks][4]
    pg::DevBuf<unsigned> d_cond_map;     // [n_streams][chunks]
    pg::DevBuf<int> d_cond_count;        // [n_streams][chunks]
    pg::DevBuf<float2> d_cond_prev;      // [n_streams][2]
    pg::PinnedBuf<pg::CondPar> h_cond[kStage];  // pinned staging of the parameter table, reused like h_stage
    hipEvent_t cond_ev[kStage] = {};
    int cond_next = 0;
    const float2 *last_cond = nullptr;   // the rows the last call's transforms read, if it conditioned any
    uint64_t last_cond_n = 0;
    std::string name_buf[3];             // pebblegpu_streambank_kernel_name of a conditioned call
    uint64_t gate_bytes = 0;             // per IQ slot, behind the rows: room for n_selected * max_frames entries
    bool slot_gated[pg::kEgressMaxSlots] = {};      // the IQ slot's block carries the gate trailer ...
    uint32_t slot_frames[pg::kEgressMaxSlots] = {}; // ... of this many frames per selected stream
};

static_assert(sizeof(pg::StreamGate) == sizeof(pebblegpu_stream_gate) && sizeof(pebblegpu_stream_gate) == 24, "the IQ block trailer's entry");
constexpr uint64_t kMaxRingBytes = 1ull << 30;  // pinned host memory one ring may hold, all slots together

// a ring's selection: `streams` checked against the bank (NULL: all, in order)
static int sb_selection(const pebblegpu_streambank *sb, const uint32_t *streams, uint32_t n_streams, std::vector<uint32_t> *sel)
{
    const uint32_t S = sb->cfg.n_streams;
    if (!streams) {
        for (uint32_t c = 0; c < S; c++) sel->push_back(c);
        return 0;
    }
    if (n_streams == 0) return fail(PEBBLEGPU_E_INVALID, "an empty stream list");
    std::vector<char> seen(S, 0);
    for (uint32_t i = 0; i < n_streams; i++) {
        if (streams[i] >= S) return fail(PEBBLEGPU_E_INVALID, "stream %u out of range", streams[i]);
        if (seen[streams[i]]) return fail(PEBBLEGPU_E_INVALID, "stream %u is listed twice", streams[i]);
        seen[streams[i]] = 1;
        sel->push_back(streams[i]);
    }
    return 0;
}

// allocates the ring and the selection's table; on failure everything it made is freed again and the handle is as it was
static int sb_open_ring(pebblegpu_streambank *sb, pg::EgressRing &ring, pg::DevBuf<uint32_t> &d_tab, const std::vector<uint32_t> &sel, uint32_t n_slots, uint32_t bps,
                        uint64_t max_n, uint32_t fmt, uint64_t extra_bytes = 0)
{
    const uint64_t slot = (uint64_t)sel.size() * pg::EgressRing::row_pitch(max_n, bps) + extra_bytes;
    if (slot * n_slots > kMaxRingBytes)
        return fail(PEBBLEGPU_E_SIZE, "%u slots of %llu bytes: a ring pins at most %llu bytes of host memory", n_slots, (unsigned long long)slot,
                    (unsigned long long)kMaxRingBytes);
    PG_HIP(hipSetDevice(sb->cfg.device));
    auto body = [&]() -> int {
        PG_TRY(d_tab.upload(sel.data(), sel.size()));
        if (int rc = ring.open_ring(n_slots, (uint32_t)sel.size(), bps, max_n, fmt, extra_bytes)) return rc;
        for (uint32_t i = 0; i < n_slots; i++) PG_HIP(hipMemset(ring.slot[i].d, 0, ring.slot_bytes));  // (the padding of a row is never written)
        return 0;
    };
    std::lock_guard<std::mutex> lk(ring.mu);
    const int rc = body();
    if (rc) {
        ring.release();
        d_tab.release();
    }
    return rc;
}

static int sb_close_ring(pebblegpu_streambank *sb, pg::EgressRing &ring, pg::DevBuf<uint32_t> &d_tab)
{
    PG_HIP(hipSetDevice(sb->cfg.device));
    PG_HIP(hipStreamSynchronize(sb->stream));
    PG_HIP(hipStreamSynchronize(sb->stream2));
    ring.close_ring();
    d_tab.release();
    return 0;
}

// `bytes` of host table `src` to d_dst, in stream order on the bank's stream: behind the kernels of earlier calls that read the table,
// ahead of this call's.  The host copies into a pinned staging slot and goes on; it waits only if the copy queued from that slot
// kStage uploads ago has not completed.
static int sb_upload(pebblegpu_streambank *sb, void *d_dst, const void *src, size_t bytes)
{
    const int i = sb->stage_next;
    sb->stage_next = (i + 1) % pebblegpu_streambank::kStage;
    PG_HIP(hipEventSynchronize(sb->stage_ev[i]));
    memcpy(sb->h_stage[i], src, bytes);
    PG_HIP(hipMemcpyAsync(d_dst, sb->h_stage[i], bytes, hipMemcpyHostToDevice, sb->stream));
    PG_HIP(hipEventRecord(sb->stage_ev[i], sb->stream));
    return 0;
}

// fdEstimate on every row the call computed: one launch behind the call's end, none when it computed no row
static int sb_queue_strength(pebblegpu_streambank *sb, uint64_t rows)
{
    sb->sm_rows = 0;
    if (!rows) return 0;
    const uint32_t S = sb->cfg.n_streams;
    const int bins = (int)sb->sp.bins;
    if (sb->win_dirty) {
        std::vector<pg::SmBins> w(S);
        for (uint32_t s = 0; s < S; s++)
            w[s] = pg::strength_windows((uint32_t)bins, (uint32_t)std::llround(sb->cfg.sample_rate), sb->bp_lo[s], sb->bp_hi[s], 0.0, (int)s);
        if (int rc = sb_upload(sb, sb->d_win, w.data(), sizeof(pg::SmBins) * S)) return rc;
        sb->win_dirty = false;
    }
    pg::launch(pg::k_stream_strength, dim3((unsigned)(S * rows)), dim3(256), sb->stream, sb->d_spec, (long long)rows * bins, bins, (int)rows, sb->d_win,
               sb->d_smeter, (long long)sb->cfg.max_frames, sb->d_carry[sb->carry_cur ^ 1]);
    PG_HIP(hipGetLastError());
    sb->sm_rows = rows;
    return 0;
}

// The gate of an IQ block of F frames into its trailer: per frame the S-meter row it reads (receiver.cpp:959-965, getUnprocessed()) -- its
// own when the call computed one for it, else the latest at or before it, carried from an earlier call if need be, none before any exists
static int sb_queue_gate(pebblegpu_streambank *sb, uint32_t F, uint32_t what, pg::StreamGate *gate)
{
    if (sb->sq_dirty) {
        if (int rc = sb_upload(sb, sb->d_squelch, sb->squelch.data(), sizeof(float) * sb->cfg.n_streams)) return rc;
        sb->sq_dirty = false;
    }
    const int before = sb->have_row ? pg::kGateRowCarried : pg::kGateRowNone;
    const bool every = (what & 2u) && !sb->last_listed && sb->sm_rows;
    size_t k = 0;  // listed frames at or before the current one
    for (uint32_t j0 = 0; j0 < F; j0 += pg::kListMax) {
        pg::GateRows gr;
        gr.j0 = (int)j0;
        gr.n = (int)std::min<uint32_t>(pg::kListMax, F - j0);
        for (int j = 0; j < gr.n; j++) {
            const uint32_t f = j0 + (uint32_t)j;
            if (every) { gr.row[j] = (int)f; continue; }
            while (sb->sm_rows && k < sb->sel.size() && sb->sel[k] <= f) k++;
            gr.row[j] = k ? (int)k - 1 : before;
        }
        const unsigned items = sb->iq_ring.rows * (unsigned)gr.n;
        pg::launch(pg::k_stream_gate_eval, dim3((items + 255) / 256), dim3(256), sb->stream, sb->d_smeter, (long long)sb->cfg.max_frames,
                   sb->d_carry[sb->carry_cur], sb->d_squelch, sb->d_iq_tab, (int)sb->iq_ring.rows, (int)F, gate, gr);
    }
    PG_HIP(hipGetLastError());
    return 0;
}

// The blocks of an accepted call, behind its end on the bank's stream (behind the join of a side-by-side call) and so ahead of the
// next call's kernels, which overwrite d_filt and d_spec: one launch and one event per open ring; a call that did not run a ring's
// producer gives that ring a block of 0 samples / 0 rows and queues nothing.
static int sb_queue_blocks(pebblegpu_streambank *sb, uint64_t n, uint32_t what)
{
    if (sb->sm_on) {
        if (int rc = sb_queue_strength(sb, n ? sb->last_frames : 0)) return rc;
    }
    if (sb->iq_ring.open) {
        if (pg::EgressSlot *g = sb->iq_ring.begin()) {
            const uint64_t m = (what & 1u) ? n : 0, pitch = pg::EgressRing::row_pitch(m, sb->iq_ring.bytes_per_sample);
            // S-meter on: the gate per (selected stream, frame) into a trailer behind the rows, inside the one copy; the rows go through the
            // gated instance only while some threshold can close (else the launch is the one a bank without S-meter queues)
            pg::StreamGate *gate = nullptr;
            const uint32_t F = (uint32_t)(m / sb->cfg.frame);
            if (sb->sm_on && m) {
                gate = reinterpret_cast<pg::StreamGate *>((unsigned char *)g->d + sb->iq_ring.rows * pitch);
                if (int rc = sb_queue_gate(sb, F, what, gate)) return rc;
            }
            sb->slot_gated[g - sb->iq_ring.slot] = gate != nullptr;
            sb->slot_frames[g - sb->iq_ring.slot] = F;
            if (int rc = pg::run_iq_pack(sb->stream, sb->d_filt, (long long)n, (long long)m, sb->d_iq_tab, sb->iq_ring.rows, sb->iq_fmt, g->d, pitch,
                                         sb->n_squelch ? gate : nullptr, (long long)sb->cfg.frame))
                return rc;
            g->aux = 0;
            const uint64_t extra = gate ? ((uint64_t)sb->iq_ring.rows * F * sizeof(pg::StreamGate) + 15) & ~(uint64_t)15 : 0;
            if (int rc = sb->iq_ring.commit(g, sb->stream, m, extra)) return rc;
        }
    }
    if (sb->sm_rows) {  // this call's last entry is what later calls carry
        sb->carry_cur ^= 1;
        sb->have_row = true;
    }
    if (sb->disp_ring.open) {
        // SpectrumWidget::recalcScale on this call's first computed row of every stream; a call that computed none leaves the request
        // pending.  Delivered or dropped: what later blocks look like never depends on the reader.  One stream orders everything
        const bool recalc = sb->scale_flags && sb->scale_pending && n && sb->last_frames;
        if (recalc) {
            const long long bins = sb->sp.bins;
            if (int rc = pg::run_scale_stats(sb->stream, sb->d_spec, (long long)sb->last_frames * bins, 0, (int)sb->cfg.n_streams, 1, (int)bins, sb->d_scale)) return rc;
            sb->scale_live = sb->scale_flags;
            sb->scale_pending = false;
        }
        if (pg::EgressSlot *g = sb->disp_ring.begin()) {
            // the rows THIS call computed (under a gate d_spec is compact: last_frames rows per stream); the last max_rows of them
            const uint64_t computed = n ? sb->last_frames : 0, k = std::min<uint64_t>(computed, sb->disp_max_rows), first = computed - k;
            // auto-scale: the ranges by value in the launch, the ranges used into a trailer behind the rows (inside the one copy)
            pg::ScaleUse su;
            const uint64_t samples = k * (sb->disp.row_pitch_bytes / 4);  // (a "sample" is 4 bytes of a row)
            if (sb->scale_flags && k) {  // (a block without rows stays what it was: nothing queued, no trailer)
                su.tab = sb->d_scale;
                su.use = sb->scale_flags & sb->scale_live;
                su.refreshed = recalc ? 1u : 0u;
                su.trailer = reinterpret_cast<pg::ScaleEntry *>((unsigned char *)g->d + sb->disp_ring.rows * pg::EgressRing::row_pitch(samples, 4));
                su.n_trailer = sb->disp_ring.rows;
                su.fixed_max = sb->disp.sh.max_db;
                su.fixed_min = sb->disp.min_db;
            }
            sb->slot_scaled[g - sb->disp_ring.slot] = su.trailer != nullptr;
            if (int rc = pg::run_display_pack(sb->stream, sb->disp, sb->d_spec, (long long)computed, (int)first, (int)k, g->d, su)) return rc;
            g->aux = (uint32_t)first;
            if (int rc = sb->disp_ring.commit(g, sb->stream, samples, su.trailer ? sb->trailer_bytes : 0)) return rc;
        }
    }
    return 0;
}


// every kernel THIS raw call would run converts in its own loads (else the call is staged through k_normalize_iq as a whole): a call that
// asks for the band-pass alone does not depend on the display transform's kernels, and the other way round
static bool sb_converts(const pebblegpu_streambank *sb, uint32_t what)
{
    return (!(what & 1u) || sb->ff.raw_ready()) && (!(what & 2u) || sb->sp.raw_ready() || sb->sp.raw_ready_big());
}


// The conditioners of one call, queued on the bank's stream: *in (the caller's rows, or with `owned` the normalised copy of a raw call in
// d_cond[1]; rows n apart) becomes the bank-owned rows the call's transforms read.  The caller's rows are never written: the first pass
// over them is out of place.  DC removal, IQ balance and NB2 may run in place on rows the bank owns; NB1 never (its output is its input
// two samples earlier), it goes from one of the two buffers to the other.
static int sb_condition(pebblegpu_streambank *sb, const float2 **in, bool owned, uint64_t n)
{
    const uint32_t S = sb->cfg.n_streams;
    const size_t ncmax = (size_t)((sb->cap + pg::kCondChunk - 1) / pg::kCondChunk);
    if (!sb->cond_ready) {  // first use: the design, the state and the scans' scratch
        const pg::design::Biquad h = pg::design::biquad_highpass(10, 0.7071, sb->cfg.sample_rate);  // DCRemoval ctor, dcremoval.cpp:5-9
        const double c[5] = {h.b0, h.b1, h.b2, h.a1, h.a2};
        pg::fill_scan_section(sb->cond_dc.sec[0], pg::kBiquadDf2, c);
        // the chunk-to-chunk transition on (w1, w1 - w2) (k_cond_dc_combine): -a1 - a2 - 1 is 1e-11 at 20 Msps, formed in long double
        const double a12 = (double)(-(long double)h.a1 - (long double)h.a2), a121 = (double)(-(long double)h.a1 - (long double)h.a2 - 1.0L);
        const pg::design::M2 m = pg::design::m2_pow(pg::design::M2{a12, h.a2, a121, h.a2}, (uint64_t)pg::kCondChunk);
        sb->cond_m[0] = m.a; sb->cond_m[1] = m.b; sb->cond_m[2] = m.c; sb->cond_m[3] = m.d;
        auto avg = [](pg::CondAvg &a, double d, double g) {
            a.d = d;
            a.g = g;
            for (int k = 0; k < 6; k++) a.P[k] = std::pow(d, (double)(pg::kSeg << k));
            a.chunk = std::pow(d, (double)pg::kCondChunk);
        };
        avg(sb->cond_mag, 0.999, 0.001);
        avg(sb->cond_cpx, 0.75, 0.25);
        if (!sb->d_cond_par) PG_TRY(sb->d_cond_par.alloc(S));
        if (!sb->d_cond_state) PG_TRY(sb->d_cond_state.alloc(S));
        if (!sb->d_cond_sum) PG_TRY(sb->d_cond_sum.alloc(4 * ncmax * S));
        if (!sb->d_cond_entry) PG_TRY(sb->d_cond_entry.alloc(4 * ncmax * S));
        if (!sb->d_cond_map) PG_TRY(sb->d_cond_map.alloc(ncmax * S));
        if (!sb->d_cond_count) PG_TRY(sb->d_cond_count.alloc(ncmax * S));
        if (!sb->d_cond_prev) PG_TRY(sb->d_cond_prev.alloc((size_t)2 * S));
        for (int i = 0; i < pebblegpu_streambank::kStage; i++) {
            if (!sb->h_cond[i]) PG_TRY(sb->h_cond[i].alloc(S));
            if (!sb->cond_ev[i]) PG_HIP(hipEventCreateWithFlags(&sb->cond_ev[i], hipEventDisableTiming));
        }
    }
    hipStream_t st = sb->stream;
    if (sb->cond_dirty || !sb->cond_ready) {
        // the table in stream order: behind the kernels of earlier calls that read it, ahead of this call's.  The host waits only if the
        // copy queued from this pinned slot kStage uploads ago has not completed.
        const int i = sb->cond_next;
        sb->cond_next = (i + 1) % pebblegpu_streambank::kStage;
        PG_HIP(hipEventSynchronize(sb->cond_ev[i]));
        pg::CondPar *t = sb->h_cond[i];
        sb->cond_mask = 0;
        for (uint32_t s = 0; s < S; s++) {
            const auto &h = sb->cond[s];
            t[s] = pg::CondPar{h.flags, h.reset, h.gain, h.phase};
            sb->cond_mask |= h.flags;
        }
        PG_HIP(hipMemcpyAsync(sb->d_cond_par, t, sizeof(pg::CondPar) * S, hipMemcpyHostToDevice, st));
        PG_HIP(hipEventRecord(sb->cond_ev[i], st));
        pg::launch(pg::k_cond_reset, dim3((S + 63) / 64), dim3(64), st, sb->d_cond_state, (const pg::CondPar *)sb->d_cond_par, (int)S, sb->cond_ready ? 0 : 1);
        PG_HIP(hipGetLastError());
        for (auto &h : sb->cond) h.reset = 0;
        sb->cond_dirty = false;
        sb->cond_ready = true;
    }
    const int mask = sb->cond_mask;
    auto buffer = [&](int i) -> int {
        if (sb->d_cond[i]) return 0;
        pg::DevBuf<float2> &own = i ? sb->d_raw_stage : sb->d_cond0;
        if (!own) PG_TRY(own.alloc((size_t)S * sb->cap));
        sb->d_cond[i] = own;
        return 0;
    };
    const long long N = (long long)n;
    const int nc = (int)((n + pg::kCondChunk - 1) / pg::kCondChunk);
    const dim3 all((unsigned)nc, S), but_last((unsigned)(nc - 1), S), per_stream(S), wave(64);
    const pg::CondPar *par = sb->d_cond_par;
    const float2 *cur = *in;
    bool mine = owned;
    if (mask & 3) {  // DC removal; IQ balance alone needs rows it may write, and gets them from the same pass (it copies a stream without DC)
        if (!mine) { if (int rc = buffer(0)) return rc; }
        float2 *dst = mine ? const_cast<float2 *>(cur) : sb->d_cond[0];
        if (mask & 1) {
            if (nc > 1) pg::launch(pg::k_cond_dc_sum, but_last, wave, st, cur, N, sb->cond_dc, par, sb->d_cond_sum, nc);
            pg::launch(pg::k_cond_dc_combine, per_stream, wave, st, (const double *)sb->d_cond_sum, sb->d_cond_entry, (const pg::CondState *)sb->d_cond_state, par,
                       sb->cond_m[0], sb->cond_m[1], sb->cond_m[2], sb->cond_m[3], nc);
        }
        if ((mask & 1) || !mine)
            pg::launch(pg::k_cond_dc_apply, all, wave, st, cur, N, dst, N, N, sb->cond_dc, par, (const double *)sb->d_cond_entry, sb->d_cond_state, nc);
        cur = dst;
        mine = true;
    }
    if (mask & 2) pg::launch(pg::k_cond_iq, dim3((unsigned)(n / sb->cfg.frame), S), wave, st, const_cast<float2 *>(cur), N, (int)sb->cfg.frame, par);
    if (mask & 4) {
        const int to = cur == sb->d_cond[0] ? 1 : 0;
        if (int rc = buffer(to)) return rc;
        float2 *dst = sb->d_cond[to];
        if (nc > 1) pg::launch(pg::k_cond_nb_sum<1>, but_last, wave, st, cur, N, sb->cond_mag, sb->cond_cpx, par, sb->d_cond_sum, nc);
        pg::launch(pg::k_cond_nb_combine<1>, per_stream, wave, st, (const double *)sb->d_cond_sum, sb->d_cond_entry, (const pg::CondState *)sb->d_cond_state, par,
                   sb->cond_mag.chunk, sb->cond_cpx.chunk, nc);
        if (nc > 1) pg::launch(pg::k_cond_nb1_map, but_last, wave, st, cur, N, sb->cond_mag, par, (const double *)sb->d_cond_entry, sb->d_cond_map, nc);
        pg::launch(pg::k_cond_nb1_map_combine, per_stream, wave, st, (const unsigned *)sb->d_cond_map, sb->d_cond_count, sb->d_cond_prev, sb->d_cond_state, par, cur,
                   N, N, nc);
        pg::launch(pg::k_cond_nb1_apply, all, wave, st, cur, N, dst, N, N, sb->cond_mag, par, (const double *)sb->d_cond_entry, (const int *)sb->d_cond_count,
                   (const float2 *)sb->d_cond_prev, sb->d_cond_state, nc);
        cur = dst;
        mine = true;
    }
    if (mask & 8) {
        if (!mine) { if (int rc = buffer(0)) return rc; }
        float2 *dst = mine ? const_cast<float2 *>(cur) : sb->d_cond[0];
        if (nc > 1) pg::launch(pg::k_cond_nb_sum<2>, but_last, wave, st, cur, N, sb->cond_mag, sb->cond_cpx, par, sb->d_cond_sum, nc);
        pg::launch(pg::k_cond_nb_combine<2>, per_stream, wave, st, (const double *)sb->d_cond_sum, sb->d_cond_entry, (const pg::CondState *)sb->d_cond_state, par,
                   sb->cond_mag.chunk, sb->cond_cpx.chunk, nc);
        pg::launch(pg::k_cond_nb2_apply, all, wave, st, cur, N, dst, N, N, sb->cond_mag, sb->cond_cpx, par, (const double *)sb->d_cond_entry, sb->d_cond_state, nc);
        cur = dst;
    }
    PG_HIP(hipGetLastError());
    *in = cur;
    sb->last_cond = cur;
    sb->last_cond_n = n;
    return 0;
}

extern "C" {

int pebblegpu_streambank_destroy(pebblegpu_streambank *sb)
{
    if (!sb) return 0;
    (void)hipSetDevice(sb->cfg.device);
    if (sb->stream2) (void)hipStreamSynchronize(sb->stream2);
    if (sb->stream) (void)hipStreamSynchronize(sb->stream);
    if (sb->iq_ring.open) sb->iq_ring.close_ring();  // (waits for a reader that is inside _next)
    if (sb->disp_ring.open) sb->disp_ring.close_ring();
    if (sb->stream2) {
        (void)hipStreamSynchronize(sb->stream2);
        (void)hipStreamDestroy(sb->stream2);
    }
    if (sb->stream) {
        (void)hipStreamSynchronize(sb->stream);
        (void)hipStreamDestroy(sb->stream);
    }
    sb->ingest.release();
    for (hipEvent_t e : sb->stage_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : sb->cond_ev) if (e) (void)hipEventDestroy(e);
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
    sb->bp_lo.assign(cfg->n_streams, -1.f);
    sb->bp_hi.assign(cfg->n_streams, 1.f);
    sb->squelch.assign(cfg->n_streams, -120.f);
    sb->cond.assign(cfg->n_streams, pebblegpu_streambank::CondHost());
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
        PG_TRY(sb->d_tail.alloc_zero(ov * S));  // m_pFFTOverlapBuf starts at zero, fastfir.cpp:104-105
        PG_TRY(sb->d_tail_alt.alloc_zero(ov * S));
        PG_TRY(sb->d_filt.alloc(sb->cap * S));
        PG_TRY(sb->d_spec.alloc((size_t)sb->sp.bins * cfg->max_frames * S));
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
    sb->bp_lo[stream] = (float)lo;  // the S-meter's window (fdEstimate takes floats)
    sb->bp_hi[stream] = (float)hi;
    sb->win_dirty = true;
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
// (owned: `in` is the bank's own normalised copy, which the conditioners may write)
static int sb_run(pebblegpu_streambank *sb, const float2 *in, const pg::RawSrc *raw, uint64_t n, uint32_t what, bool owned = false)
{
    sb->last_n = 0;
    sb->last_frames = 0;
    sb->last_cond = nullptr;
    sb->last_cond_n = 0;
    if (n == 0) return sb_queue_blocks(sb, 0, what);
    // The update timer, on the host before anything is queued.  A call without the spectrum advances the sample clock and nothing else:
    // it selects no frame and neither starts nor restarts the timer.
    const uint64_t F = n / sb->cfg.frame;
    sb->sel.clear();
    sb->last_listed = (what & 2u) && sb->ups != -1;
    if (what & 2u) sb->ut.advance(sb->ups, sb->period_ms, F, sb->cfg.frame, (uint64_t)std::llround(sb->cfg.sample_rate), &sb->sel);
    else sb->ut.next += F;
    PG_HIP(hipEventRecord(sb->ev[0], sb->stream));
    // While any stream has a conditioner flag set every call conditions its samples first, whatever it asks for: the state advances
    // with the sample stream (receiver.cpp:814-823 run ahead of everything else)
    const bool conditioned = sb->n_cond != 0;
    if (conditioned) {
        if (int rc = sb_condition(sb, &in, owned, n)) return rc;
    }
    // Both asked for: the band-pass (bound by its two transforms per block: vector units + LDS) and the display transform (the 65536-point
    // one is bound by what it moves through HBM) read the same input and share nothing else.  Side by side on two streams (fork at the
    // call's start event, join at its end; PEBBLEGPU_SB_SIDE=1 when the bank is created) they do NOT overlap: 0.4345 / 0.4368 ms per
    // configs[4] call against 0.4346 / 0.4422 one after the other -- the band-pass's 32768 small workgroups fill every CU's LDS first and the
    // transform's workgroups wait for them; with the band-pass's occupancy cut (8 / 16 / 30 kB of extra LDS per workgroup) both get slower
    // (0.46 / 0.48 / 0.52).  Opt-in, not the default.
    const bool side = sb->side_ok && (what & 3u) == 3u;
    sb->side = side;
    hipStream_t fs = side ? sb->stream2 : sb->stream;
    if (side && conditioned) PG_HIP(hipEventRecord(sb->ev[4], sb->stream));
    if (side) PG_HIP(hipStreamWaitEvent(fs, sb->ev[conditioned ? 4 : 0], 0));
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
    return sb_queue_blocks(sb, n, what);
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
    sb->last_staged = !sb_converts(sb, what) || (sb->n_cond && n);  // (the conditioners read and write float2 rows)
    if (!sb->last_staged || n == 0) return sb_run(sb, nullptr, &raw, n, what);
    const size_t S = sb->cfg.n_streams;
    if (!sb->d_raw_stage) PG_TRY(sb->d_raw_stage.alloc(S * sb->cap));
    sb->d_cond[1] = sb->d_raw_stage;
    // (the rows of d_raw are n pairs apart, so S * n pairs are one run; the side stream forks behind it, at the call's start event)
    if (int rc = pg::run_normalize_iq(fmt, order, 1.0, d_raw, (long long)(S * n), sb->d_raw_stage, sb->stream, false, &raw.scale)) return rc;
    return sb_run(sb, sb->d_raw_stage, nullptr, n, what, true);
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

// the route of a call: last_fmt -1 float2 input, else the raw format; last_staged: through k_normalize_iq as a whole
static const char *sb_route_name(const pebblegpu_streambank *sb, int which, int last_fmt, bool last_staged)
{
    static const char *const kFf[6] = {"k_fastfir_t128", "k_fastfir_t128 (raw s8)", "k_fastfir_t128 (raw u8)", "k_fastfir_t128 (raw s16)",
                                       "k_fastfir_t128 (raw f32)", "k_fastfir_t128 (raw wav16)"};
    static const char *const kBig[6] = {"k_big256_cols + k_big256_rows", "k_big256_cols (raw s8) + k_big256_rows", "k_big256_cols (raw u8) + k_big256_rows",
                                        "k_big256_cols (raw s16) + k_big256_rows", "k_big256_cols (raw f32) + k_big256_rows",
                                        "k_big256_cols (raw wav16) + k_big256_rows"};
    static const char *const kT128[6] = {"k_spectrum_t128", "k_spectrum_t128 (raw s8)", "k_spectrum_t128 (raw u8)", "k_spectrum_t128 (raw s16)",
                                         "k_spectrum_t128 (raw f32)", "k_spectrum_t128 (raw wav16)"};
    static const char *const kW64[6] = {"k_spectrum_w64", "k_spectrum_w64 (raw s8)", "k_spectrum_w64 (raw u8)", "k_spectrum_w64 (raw s16)",
                                        "k_spectrum_w64 (raw f32)", "k_spectrum_w64 (raw wav16)"};
    const int r = last_fmt >= 0 && !last_staged ? last_fmt + 1 : 0;  // 0: the float2 instances
    const pg::SpectrumCore &sp = sb->sp;
    if (which == 1) {
        if (!sb->last_bp) return "";
        if (sb->ff.fft_n == 2048) return last_staged ? "k_normalize_iq + k_fastfir_t128" : kFf[r];
        return last_staged ? "k_normalize_iq + k_fastfir" : "k_fastfir";
    }
    if (which == 2 && sb->last_sp && sb->last_listed) {  // a gated call: the frame-list kernels, or none
        static const char *const kBigL[6] = {"k_big256_cols_list + k_big256_rows", "k_big256_cols_list (raw s8) + k_big256_rows",
                                             "k_big256_cols_list (raw u8) + k_big256_rows", "k_big256_cols_list (raw s16) + k_big256_rows",
                                             "k_big256_cols_list (raw f32) + k_big256_rows", "k_big256_cols_list (raw wav16) + k_big256_rows"};
        static const char *const kQ128L[6] = {"k_spectrum_list_q128", "k_spectrum_list_q128 (raw s8)", "k_spectrum_list_q128 (raw u8)",
                                              "k_spectrum_list_q128 (raw s16)", "k_spectrum_list_q128 (raw f32)", "k_spectrum_list_q128 (raw wav16)"};
        if (!sb->last_frames) return "";
        if (sp.big) return last_staged ? "k_normalize_iq + k_big256_cols_list + k_big256_rows" : kBigL[r];
        if (sp.any) return last_staged ? "k_normalize_iq + k_spectrum_list_any" : "k_spectrum_list_any";
        return last_staged ? "k_normalize_iq + k_spectrum_list_q128" : kQ128L[r];
    }
    if (which == 2) {
        if (!sb->last_sp) return "";
        if (sp.big && sp.tun.big_split32) return last_staged ? "k_normalize_iq + k_big_cols + k_big_rows" : "k_big_cols + k_big_rows";
        if (sp.big) return last_staged ? "k_normalize_iq + k_big256_cols + k_big256_rows" : kBig[r];
        if (sp.any) return last_staged ? "k_normalize_iq + k_spectrum_any" : "k_spectrum_any";
        if (sp.per_q) return last_staged ? "k_normalize_iq + k_spectrum_q128" : "k_spectrum_q128";
        if (sp.bins == 8192) return last_staged ? (sp.use_w64 ? "k_normalize_iq + k_spectrum_w64" : "k_normalize_iq + k_spectrum_t128") : sp.use_w64 ? kW64[r] : kT128[r];
        if (sp.bins == 4096) return last_staged ? "k_normalize_iq + k_spectrum<2>" : "k_spectrum<2>";
        return last_staged ? "k_normalize_iq + k_spectrum_1to1" : "k_spectrum_1to1";
    }
    return "";
}

const char *pebblegpu_streambank_kernel_name(const pebblegpu_streambank *sb, int which)
{
    if (!sb || !sb->timed) return "";
    if (!sb->last_cond) return sb_route_name(sb, which, sb->last_fmt, sb->last_staged);
    // a conditioned call: [k_normalize_iq +] k_condition + the float2 instances
    if (which < 1 || which > 2) return "";
    const char *base = sb_route_name(sb, which, -1, false);
    if (!*base) return "";
    std::string &b = const_cast<pebblegpu_streambank *>(sb)->name_buf[which];
    b = std::string(sb->last_fmt >= 0 ? "k_normalize_iq + " : "") + "k_condition + " + base;
    return b.c_str();
}

const void *pebblegpu_streambank_conditioned(const pebblegpu_streambank *sb, uint64_t *samples_per_stream, uint64_t *pitch_samples)
{
    if (samples_per_stream) *samples_per_stream = 0;
    if (pitch_samples) *pitch_samples = 0;
    if (!sb || !sb->last_cond) return nullptr;
    if (samples_per_stream) *samples_per_stream = sb->last_cond_n;
    if (pitch_samples) *pitch_samples = sb->last_cond_n;
    return sb->last_cond;
}
int pebblegpu_streambank_set_conditioners(pebblegpu_streambank *sb, uint32_t stream, int flags, double iq_gain, double iq_phase)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (stream >= sb->cfg.n_streams) return fail(PEBBLEGPU_E_INVALID, "stream %u out of range", stream);
    if (flags < 0 || flags > 15) return fail(PEBBLEGPU_E_INVALID, "conditioner flags %d: PEBBLEGPU_COND_* or'ed, 0..15", flags);
    if (!std::isfinite(iq_gain) || !std::isfinite(iq_phase)) return fail(PEBBLEGPU_E_INVALID, "the IQ gain and phase factors must be finite");
    // host state only: the next call uploads the table and resets what was switched on, in stream order
    auto &h = sb->cond[stream];
    h.reset |= (flags & ~h.flags) & (PEBBLEGPU_COND_NB1 | PEBBLEGPU_COND_NB2);  // setNbEnabled(true) / setNb2Enabled(true), noiseblanker.cpp:20-37
    sb->n_cond += (flags ? 1u : 0u) - (h.flags ? 1u : 0u);
    h.flags = flags;
    h.gain = iq_gain;
    h.phase = iq_phase;
    sb->cond_dirty = true;
    return 0;
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

// ---- host egress: the IQ ring ----
int pebblegpu_streambank_iq_out_open(pebblegpu_streambank *sb, int format, const uint32_t *streams, uint32_t n_streams, uint32_t n_slots)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (format != PEBBLEGPU_AUDIO_F32 && format != PEBBLEGPU_AUDIO_S16)
        return fail(PEBBLEGPU_E_INVALID, "IQ format %d: PEBBLEGPU_AUDIO_F32 or PEBBLEGPU_AUDIO_S16", format);
    if (int rc = pg::check_egress_slots(n_slots)) return rc;
    std::vector<uint32_t> sel;
    if (int rc = sb_selection(sb, streams, n_streams, &sel)) return rc;
    if (sb->iq_ring.open) return fail(PEBBLEGPU_E_INVALID, "the IQ ring is already open");
    // (room behind the rows for the gate trailer, reserved whether or not the S-meter is on: a slot's size is fixed here)
    const uint64_t trailer = ((uint64_t)sel.size() * sb->cfg.max_frames * sizeof(pg::StreamGate) + 15) & ~(uint64_t)15;
    if (int rc = sb_open_ring(sb, sb->iq_ring, sb->d_iq_tab, sel, n_slots, pg::kAudioBytes[format], sb->cap, (uint32_t)format, trailer)) return rc;
    sb->iq_fmt = format;
    sb->gate_bytes = trailer;
    for (bool &b : sb->slot_gated) b = false;
    return 0;
}
int pebblegpu_streambank_iq_out_close(pebblegpu_streambank *sb)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (!sb->iq_ring.open) return fail(PEBBLEGPU_E_INVALID, "the IQ ring is not open");
    return sb_close_ring(sb, sb->iq_ring, sb->d_iq_tab);
}
int pebblegpu_streambank_iq_out_next(pebblegpu_streambank *sb, int wait, pebblegpu_audio_block *b)
{
    if (!sb || !b) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (b->struct_size != sizeof(pebblegpu_audio_block)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_audio_block size mismatch");
    pg::EgressBlock e;
    if (int rc = sb->iq_ring.next(sb->cfg.device, wait, &e)) return rc;
    b->format = e.format;
    b->call_index = e.call;
    b->host = e.host;
    b->samples_per_channel = e.host ? e.samples : 0;
    b->pitch_bytes = e.host ? e.pitch_bytes : 0;
    b->n_channels = e.rows;
    b->dropped_before = e.host ? e.dropped_before : 0;
    return 0;
}
int pebblegpu_streambank_iq_out_release(pebblegpu_streambank *sb, uint64_t call_index)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    return sb->iq_ring.finish(call_index);
}
static int sb_dropped(pg::EgressRing &ring, uint64_t *blocks)
{
    std::lock_guard<std::mutex> lk(ring.mu);
    if (!ring.open) return fail(PEBBLEGPU_E_INVALID, "the ring is not open");
    *blocks = ring.dropped;
    return 0;
}
int pebblegpu_streambank_iq_out_dropped(const pebblegpu_streambank *sb, uint64_t *blocks)
{
    if (!sb || !blocks) return fail(PEBBLEGPU_E_INVALID, "null argument");
    return sb_dropped(const_cast<pebblegpu_streambank *>(sb)->iq_ring, blocks);
}

// ---- host egress: the display ring ----
int pebblegpu_streambank_display_open(pebblegpu_streambank *sb, int format, const pebblegpu_screen_map *map, const uint32_t *streams, uint32_t n_streams,
                                      uint32_t max_rows, uint32_t n_slots)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (format != PEBBLEGPU_DISPLAY_DB_F32 && format != PEBBLEGPU_DISPLAY_PIXELS_I32 && format != PEBBLEGPU_DISPLAY_WATERFALL_ARGB32)
        return fail(PEBBLEGPU_E_INVALID, "unknown display format %d", format);
    if (int rc = pg::check_egress_slots(n_slots)) return rc;
    if (!sb->cfg.spectrum_bins) return fail(PEBBLEGPU_E_INVALID, "the bank was created without a spectrum (spectrum_bins 0)");
    if (format != PEBBLEGPU_DISPLAY_DB_F32) {
        if (!map) return fail(PEBBLEGPU_E_INVALID, "display format %d needs a pebblegpu_screen_map", format);
        if (map->struct_size != sizeof(pebblegpu_screen_map)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_screen_map size mismatch");
        if (int rc = pg::check_screen_map(map->y_pixels, map->x_pixels, map->max_db, map->min_db)) return rc;
        if (format == PEBBLEGPU_DISPLAY_WATERFALL_ARGB32 && map->y_pixels != 255)
            return fail(PEBBLEGPU_E_INVALID, "the waterfall's palette is indexed by pixels of a 255-pixel plot, not %d (spectrumwidget.cpp:1285-1293)", map->y_pixels);
    }
    std::vector<uint32_t> sel;
    if (int rc = sb_selection(sb, streams, n_streams, &sel)) return rc;
    if (sb->disp_ring.open) return fail(PEBBLEGPU_E_INVALID, "the display ring is already open");
    pg::DisplayPack plan;
    plan.format = format;
    plan.n_streams = (uint32_t)sel.size();
    pg::display_pack_plan(&plan, (int32_t)sb->sp.bins, sb->cfg.sample_rate, map);
    const uint32_t rows = max_rows && max_rows < sb->cfg.max_frames ? max_rows : sb->cfg.max_frames;  // (no call computes more than max_frames)
    // (room behind the rows for the auto-scale trailer, and the ranges' table: one entry per stream of the bank)
    const uint64_t trailer = ((uint64_t)sel.size() * sizeof(pg::ScaleEntry) + 15) & ~(uint64_t)15;
    PG_HIP(hipSetDevice(sb->cfg.device));
    if (!sb->d_scale) {
        PG_TRY(sb->d_scale.alloc_zero(sb->cfg.n_streams));
    }
    if (int rc = sb_open_ring(sb, sb->disp_ring, sb->d_disp_tab, sel, n_slots, 4, (uint64_t)rows * (plan.row_pitch_bytes / 4), (uint32_t)format, trailer)) return rc;
    plan.d_tab = sb->d_disp_tab;
    sb->disp = plan;
    sb->disp_max_rows = rows;
    sb->trailer_bytes = trailer;
    sb->scale_flags = sb->scale_live = 0;
    sb->scale_pending = false;
    return 0;
}
int pebblegpu_streambank_display_close(pebblegpu_streambank *sb)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (!sb->disp_ring.open) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    sb->disp.d_tab = nullptr;
    return sb_close_ring(sb, sb->disp_ring, sb->d_disp_tab);
}
int pebblegpu_streambank_display_next(pebblegpu_streambank *sb, int wait, pebblegpu_display_block *b)
{
    if (!sb || !b) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (b->struct_size != sizeof(pebblegpu_display_block)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_display_block size mismatch");
    pg::EgressBlock e;
    if (int rc = sb->disp_ring.next(sb->cfg.device, wait, &e)) return rc;
    // (disp is written at open only, and a reader has no business in _next before open has returned)
    const uint64_t row_pitch = sb->disp.row_pitch_bytes;
    b->format = e.format;
    b->call_index = e.call;
    b->host = e.host;
    b->rows_per_stream = e.host && row_pitch ? (uint32_t)(e.pitch_bytes / row_pitch) : 0;
    b->first_row = e.host ? e.aux : 0;
    b->row_elems = sb->disp.row_elems;
    b->n_streams = e.rows;
    b->dropped_before = e.host ? e.dropped_before : 0;
    b->reserved = 0;
    b->row_pitch_bytes = row_pitch;
    b->stream_pitch_bytes = e.host ? e.pitch_bytes : 0;
    return 0;
}
int pebblegpu_streambank_display_release(pebblegpu_streambank *sb, uint64_t call_index)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    return sb->disp_ring.finish(call_index);
}
int pebblegpu_streambank_display_dropped(const pebblegpu_streambank *sb, uint64_t *blocks)
{
    if (!sb || !blocks) return fail(PEBBLEGPU_E_INVALID, "null argument");
    return sb_dropped(const_cast<pebblegpu_streambank *>(sb)->disp_ring, blocks);
}
int pebblegpu_auto_scale_row(const float *db, uint32_t bins, pebblegpu_display_scale *out)
{
    if (!db || !out) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (!bins) return fail(PEBBLEGPU_E_INVALID, "a row of 0 bins");
    const pg::ScaleEntry e = pg::auto_scale_row(db, bins);
    out->max_db = e.max_db;
    out->min_db = e.min_db;
    out->avg_power = e.avg_power;
    out->peak_power = e.peak_power;
    return 0;
}
int pebblegpu_streambank_spectrum_scale(pebblegpu_streambank *sb, uint32_t first_frame, uint32_t n_frames, uint32_t frame_step, pebblegpu_display_scale *d_out)
{
    if (!sb || !d_out) return fail(PEBBLEGPU_E_INVALID, "null argument");
    // (the frame rules of pebblegpu_streambank_map_spectrum, the latest row after a gated call that selected nothing included)
    const bool latest = !sb->last_frames && sb->last_sp && sb->last_listed && sb->spec_rows;
    const uint64_t rows = latest ? 1 : sb->last_frames, pitch_rows = latest ? sb->spec_rows : sb->last_frames;
    if (!rows) return fail(PEBBLEGPU_E_INVALID, "the last call computed no spectrum (or no call has been made yet)");
    if (n_frames == 0 || (uint64_t)first_frame + (uint64_t)(n_frames - 1) * frame_step >= rows)
        return fail(PEBBLEGPU_E_INVALID, "frames %u + j * %u, j < %u, are not all within the last call's %llu", first_frame, frame_step, n_frames,
                    (unsigned long long)rows);
    PG_HIP(hipSetDevice(sb->cfg.device));
    const long long bins = sb->sp.bins;
    if (latest) first_frame = (uint32_t)(sb->spec_rows - 1);
    return pg::run_scale_stats(sb->stream, sb->d_spec + (long long)first_frame * bins, (long long)pitch_rows * bins, (long long)frame_step * bins,
                               (int)sb->cfg.n_streams, (int)n_frames, (int)bins, reinterpret_cast<pg::ScaleEntry *>(d_out));
}
int pebblegpu_streambank_display_set_auto_scale(pebblegpu_streambank *sb, uint32_t flags)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (!sb->disp_ring.open) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    if (int rc = pg::check_auto_scale(flags, 0.0, -120.0)) return rc;  // (the flag bits)
    if (sb->disp.format == PEBBLEGPU_DISPLAY_DB_F32) return fail(PEBBLEGPU_E_INVALID, "a DB_F32 ring maps nothing: there is no range to scale");
    if (int rc = pg::check_auto_scale(flags, sb->disp.sh.max_db, sb->disp.min_db)) return rc;
    if (int rc = pg::check_auto_scale(flags & sb->scale_live, sb->disp.sh.max_db, sb->disp.min_db)) return rc;  // (the ends the table supplies until the recalc lands)
    if (flags & ~sb->scale_flags) sb->scale_pending = true;  // "Auto" chosen: m_scaleNeedsRecalc = true (spectrumwidget.cpp:942, :960)
    sb->scale_live &= flags;                                 // a flag that goes off returns its end to the map (m_plotMaxDb = db)
    sb->scale_flags = flags;
    if (!flags) sb->scale_pending = false;
    return 0;
}
int pebblegpu_streambank_display_rescale(pebblegpu_streambank *sb)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (!sb->disp_ring.open) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    sb->scale_pending = sb->scale_flags != 0;  // (recalcScale returns at once with neither flag on)
    return 0;
}
int pebblegpu_streambank_display_scale(pebblegpu_streambank *sb, uint64_t call_index, pebblegpu_display_scale *out, uint32_t cap, uint32_t *n)
{
    if (!sb || !n) return fail(PEBBLEGPU_E_INVALID, "null argument");
    *n = 0;
    pg::EgressRing &ring = sb->disp_ring;
    std::lock_guard<std::mutex> lk(ring.mu);
    if (!ring.open) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    for (uint64_t q = ring.tail; q < ring.read; q++) {
        const uint32_t si = (uint32_t)(q % ring.n_slots);
        const pg::EgressSlot &g = ring.slot[si];
        if (g.call != call_index) continue;
        if (!sb->slot_scaled[si]) return fail(PEBBLEGPU_E_INVALID, "the block of call %llu carries no ranges: no auto-scale flag was on when it was queued, or it has no rows", (unsigned long long)call_index);
        if (ring.rows > cap) return fail(PEBBLEGPU_E_SIZE, "%u ranges do not fit %u entries", ring.rows, cap);
        if (!out) return fail(PEBBLEGPU_E_INVALID, "null argument");
        memcpy(out, (const unsigned char *)g.h + ring.rows * g.pitch_bytes, sizeof(pebblegpu_display_scale) * ring.rows);
        *n = ring.rows;
        return 0;
    }
    return fail(PEBBLEGPU_E_INVALID, "call %llu is not handed out", (unsigned long long)call_index);
}
// ---- the S-meter and the squelch ----
int pebblegpu_signal_strength_row(const float *db, uint32_t bins, uint32_t sample_rate, float bp_lo, float bp_hi, double mixer_freq, float out[4])
{
#pragma clang fp contract(off)
    if (!db || !out) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (!bins || bins > 0x7FFFFFFFu) return fail(PEBBLEGPU_E_INVALID, "a row of %u bins", bins);
    if (sample_rate / bins == 0) return fail(PEBBLEGPU_E_INVALID, "sample rate %u below %u bins: the reference's integer bin width is 0", sample_rate, bins);
    // the loop of signalstrength.cpp:339-353 as written, one bin after the other
    const pg::SmBins b = pg::strength_windows(bins, sample_rate, bp_lo, bp_hi, mixer_freq, 0);
    double total = 0.0, peak = 0.0, noise = 0.0;
    int nn = 0;
    for (int i = 0; i < (int)bins; i++) {
        if (i < b.nlo) continue;
        const double pwr = std::pow(10, (double)db[i] / 10.0);  // DB::dBToPower
        if (i >= b.lo && i <= b.hi) {
            total += pwr;
            if (pwr > peak) peak = pwr;
        } else if (i >= b.nlo && i <= b.nhi) {
            noise += pwr;
            nn++;
        }
        if (i >= b.nhi) break;
    }
    const float4 r = pg::strength_finish(total, peak, noise, nn, b.bp_bins);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
    return 0;
}
int pebblegpu_streambank_enable_signal_strength(pebblegpu_streambank *sb, int on)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (!on) {
        if (sb->n_squelch) return fail(PEBBLEGPU_E_INVALID, "%u streams have a squelch threshold above -120: the squelch reads the S-meter", sb->n_squelch);
        sb->sm_on = false;
        sb->sm_rows = 0;
        return 0;
    }
    if (sb->sm_on) return 0;
    const uint32_t S = sb->cfg.n_streams, bins = (uint32_t)sb->sp.bins;
    if (!sb->cfg.spectrum_bins || !bins) return fail(PEBBLEGPU_E_INVALID, "the bank was created without a spectrum (spectrum_bins 0)");
    if (bins % 4) return fail(PEBBLEGPU_E_UNSUPPORTED, "%u bins: spectrum rows are read in 16-byte vectors", bins);
    const long long rate = std::llround(sb->cfg.sample_rate);
    if (rate > 0xFFFFFFFFLL || (uint32_t)rate / bins == 0)
        return fail(PEBBLEGPU_E_INVALID, "sample rate %g with %u bins: the reference's integer bin width would be 0 (or the rate does not fit 32 bits)", sb->cfg.sample_rate, bins);
    PG_HIP(hipSetDevice(sb->cfg.device));
    if (!sb->d_smeter) {  // (kept until destroy; nothing here waits for queued calls)
        const size_t stage = std::max(sizeof(pg::SmBins), sizeof(float)) * S;
        for (int i = 0; i < pebblegpu_streambank::kStage; i++) {
            if (!sb->h_stage[i]) PG_TRY(sb->h_stage[i].alloc(stage));
            if (!sb->stage_ev[i]) PG_HIP(hipEventCreateWithFlags(&sb->stage_ev[i], hipEventDisableTiming));
        }
        if (!sb->d_win) PG_TRY(sb->d_win.alloc(S));
        if (!sb->d_squelch) PG_TRY(sb->d_squelch.alloc(S));
        for (pg::DevBuf<float4> &c : sb->d_carry) if (!c) PG_TRY(c.alloc(S));
        PG_TRY(sb->d_smeter.alloc((size_t)S * sb->cfg.max_frames));
    }
    sb->sm_on = true;
    sb->win_dirty = sb->sq_dirty = true;
    sb->have_row = false;  // rows computed while the S-meter was off are not carried
    sb->sm_rows = 0;
    return 0;
}
const void *pebblegpu_streambank_signal_strength(const pebblegpu_streambank *sb, uint64_t *rows_per_stream, uint64_t *pitch)
{
    if (rows_per_stream) *rows_per_stream = 0;
    if (pitch) *pitch = 0;
    if (!sb || !sb->sm_on) return nullptr;
    if (rows_per_stream) *rows_per_stream = sb->sm_rows;
    if (pitch) *pitch = sb->cfg.max_frames;
    return sb->d_smeter;
}
int pebblegpu_streambank_set_squelch(pebblegpu_streambank *sb, uint32_t stream, double squelch_db)
{
    if (!sb) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (stream >= sb->cfg.n_streams) return fail(PEBBLEGPU_E_INVALID, "stream %u out of range", stream);
    if (!std::isfinite(squelch_db)) return fail(PEBBLEGPU_E_INVALID, "the squelch threshold must be finite");
    const float v = (float)squelch_db;  // (what the device compares the S-meter's float with)
    if (v > -120.f) {
        if (int rc = pebblegpu_streambank_enable_signal_strength(sb, 1)) return rc;
    }
    sb->n_squelch += (v > -120.f ? 1u : 0u) - (sb->squelch[stream] > -120.f ? 1u : 0u);
    sb->squelch[stream] = v;
    sb->sq_dirty = true;
    return 0;
}
int pebblegpu_streambank_iq_out_gate(pebblegpu_streambank *sb, uint64_t call_index, pebblegpu_stream_gate *out, uint32_t cap, uint32_t *n_frames)
{
    if (!sb || !n_frames) return fail(PEBBLEGPU_E_INVALID, "null argument");
    *n_frames = 0;
    pg::EgressRing &ring = sb->iq_ring;
    std::lock_guard<std::mutex> lk(ring.mu);
    if (!ring.open) return fail(PEBBLEGPU_E_INVALID, "the IQ ring is not open");
    for (uint64_t q = ring.tail; q < ring.read; q++) {
        const uint32_t si = (uint32_t)(q % ring.n_slots);
        const pg::EgressSlot &g = ring.slot[si];
        if (g.call != call_index) continue;
        if (!sb->slot_gated[si]) return fail(PEBBLEGPU_E_INVALID, "the block of call %llu carries no gate: the S-meter was off when it was queued, or it has no samples", (unsigned long long)call_index);
        const uint64_t entries = (uint64_t)ring.rows * sb->slot_frames[si];
        if (entries > cap) return fail(PEBBLEGPU_E_SIZE, "%llu gate entries do not fit %u", (unsigned long long)entries, cap);
        if (!out) return fail(PEBBLEGPU_E_INVALID, "null argument");
        memcpy(out, (const unsigned char *)g.h + ring.rows * g.pitch_bytes, sizeof(pebblegpu_stream_gate) * entries);
        *n_frames = sb->slot_frames[si];
        return 0;
    }
    return fail(PEBBLEGPU_E_INVALID, "call %llu is not handed out", (unsigned long long)call_index);
}
int pebblegpu_waterfall_colors(const int32_t *pixels, uint64_t n, uint32_t *argb)
{
    if (n && (!pixels || !argb)) return fail(PEBBLEGPU_E_INVALID, "null argument");
    return pg::waterfall_colors(pixels, n, argb);
}

}  // extern "C"
