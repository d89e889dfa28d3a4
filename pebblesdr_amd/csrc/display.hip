// display.hip -- launcher of k_screen_map (FFT::mapFFTToScreen, kernels_display.h) for the receiver, the stream bank and the
// stand-alone spectrum step, and of the stream bank's display-ring packing kernels; the receiver's display ring (k_display_panes).
#include <algorithm>
#include <cmath>
#include <new>
#include "kernels_display.h"
#include "receiver.h"

namespace pg {

template <int G>
static void launch_map(hipStream_t s, const float *in, long long stream_pitch, long long frame_pitch, int n_frames, long long n_items,
                       const MapGeoms &geoms, const MapShared &sh, int32_t *out)
{
    constexpr long long kGroups = 256 / G;
    const long long blocks = std::min<long long>((n_items + kGroups - 1) / kGroups, 1LL << 20);
    launch(k_screen_map<G>, dim3((unsigned)blocks), dim3(256), s, in, stream_pitch, frame_pitch, n_frames, n_items, geoms, sh, out);
}

// (the lane group of a launch and of each stream's rows: map_lane_group / map_chunk_plan / map_row_plan, screen_geom.h)
int run_screen_map(hipStream_t s, const float *in, long long stream_pitch, long long frame_pitch, int n_streams, int n_frames, int32_t fft_size,
                   double sample_rate, const int32_t *edges, bool per_stream, int32_t y_pixels, int32_t x_pixels, double max_db, double min_db,
                   int32_t *out)
{
    if (n_streams <= 0 || n_frames <= 0 || x_pixels <= 0) return 0;
    MapShared sh;
    sh.fft_size = fft_size;
    sh.x_pixels = x_pixels;
    sh.y_pixels = y_pixels;
    sh.y_scale = map_y_scale(y_pixels, max_db, min_db);
    sh.max_db = max_db;
    const int chunk = per_stream ? kMapMaxGeom : n_streams;
    for (int s0 = 0; s0 < n_streams; s0 += chunk) {
        const int ns = std::min(chunk, n_streams - s0);
        MapGeoms geoms;
        memset(&geoms, 0, sizeof(geoms));
        geoms.n = per_stream ? ns : 1;
        const int G = map_chunk_plan(fft_size, sample_rate, edges, per_stream, s0, ns, x_pixels, geoms.g);
        const long long n_items = (long long)ns * n_frames * x_pixels;
        const float *rin = in + (long long)s0 * stream_pitch;
        int32_t *rout = out + (long long)s0 * n_frames * x_pixels;
        switch (G) {
        case 1: launch_map<1>(s, rin, stream_pitch, frame_pitch, n_frames, n_items, geoms, sh, rout); break;
        case 2: launch_map<2>(s, rin, stream_pitch, frame_pitch, n_frames, n_items, geoms, sh, rout); break;
        case 4: launch_map<4>(s, rin, stream_pitch, frame_pitch, n_frames, n_items, geoms, sh, rout); break;
        case 8: launch_map<8>(s, rin, stream_pitch, frame_pitch, n_frames, n_items, geoms, sh, rout); break;
        case 16: launch_map<16>(s, rin, stream_pitch, frame_pitch, n_frames, n_items, geoms, sh, rout); break;
        case 32: launch_map<32>(s, rin, stream_pitch, frame_pitch, n_frames, n_items, geoms, sh, rout); break;
        default: launch_map<64>(s, rin, stream_pitch, frame_pitch, n_frames, n_items, geoms, sh, rout); break;
        }
        PG_HIP(hipGetLastError());
    }
    return 0;
}

// DB_F32: the dB rows themselves, a gather in 16-byte vectors.  Every bin count SpectrumCore accepts is a power of two >= 2048, so rows
// are 16-byte aligned on both sides.  grid (x, rows): row = r * n_rows + j, strided over grid.y
static __global__ __launch_bounds__(256) void k_display_rows(const float *__restrict__ in, long long stream_pitch, long long frame_pitch, int first_row,
                                                             int n_rows, long long total_rows, int bins, const uint32_t *__restrict__ tab,
                                                             unsigned char *__restrict__ out, unsigned long long out_row_pitch,
                                                             unsigned long long out_stream_pitch)
{
    const int t = (int)(blockIdx.x * 256 + threadIdx.x), step = (int)gridDim.x * 256;
    for (long long row = blockIdx.y; row < total_rows; row += gridDim.y) {
        const int r = (int)(row / n_rows), j = (int)(row - (long long)r * n_rows);
        const float4 *x = reinterpret_cast<const float4 *>(in + (long long)tab[r] * stream_pitch + (long long)(first_row + j) * frame_pitch);
        float4 *o = reinterpret_cast<float4 *>(out + (unsigned long long)r * out_stream_pitch + (unsigned long long)j * out_row_pitch);
        for (int k = t; k < bins / 4; k += step) o[k] = x[k];
    }
}

template <int G>
static void launch_display_map(hipStream_t s, const DisplayPack &p, const float *in, long long stream_pitch, int first_row, int n_rows, unsigned char *out,
                               unsigned long long stream_bytes, const ScaleUse &su)
{
    constexpr long long kGroups = 256 / G;
    const long long n_items = (long long)p.n_streams * n_rows * p.sh.x_pixels;
    const dim3 grid((unsigned)std::min<long long>((n_items + kGroups - 1) / kGroups, 1LL << 20));
    if (p.format == PEBBLEGPU_DISPLAY_WATERFALL_ARGB32)
        launch(k_display_map<G, true>, grid, dim3(256), s, in, stream_pitch, (long long)p.sh.fft_size, first_row, n_rows, n_items, p.geom, p.sh, p.d_tab, out,
               (unsigned long long)p.row_pitch_bytes, stream_bytes, su);
    else
        launch(k_display_map<G, false>, grid, dim3(256), s, in, stream_pitch, (long long)p.sh.fft_size, first_row, n_rows, n_items, p.geom, p.sh, p.d_tab, out,
               (unsigned long long)p.row_pitch_bytes, stream_bytes, su);
}

int run_scale_stats(hipStream_t s, const float *in, long long stream_pitch, long long frame_pitch, int n_streams, int n_frames, int bins, ScaleEntry *out)
{
    if (n_streams <= 0 || n_frames <= 0) return 0;
    if (bins < 4 || bins % 4) return fail(PEBBLEGPU_E_UNSUPPORTED, "%d bins: spectrum rows are read in 16-byte vectors", bins);
    launch(k_scale_stats, dim3((unsigned)((long long)n_streams * n_frames)), dim3(256), s, in, stream_pitch, frame_pitch, n_frames, bins, out);
    PG_HIP(hipGetLastError());
    return 0;
}

// SpectrumWidget::recalcScale on the host: the loop of spectrumwidget.cpp:705-710 as written, one bin after the other
ScaleEntry auto_scale_row(const float *db, uint32_t bins)
{
#pragma clang fp contract(off)
    double total = 0.0, peak = 0.0;
    for (uint32_t i = 0; i < bins; i++) {
        const double pwr = std::pow(10, (double)db[i] / 10.0);  // DB::dBToPower
        total += pwr;
        if (pwr > peak) peak = pwr;
    }
    return auto_scale_finish(total, peak, (int32_t)bins);
}

int check_auto_scale(uint32_t flags, double fixed_max_db, double fixed_min_db)
{
    if (flags & ~(uint32_t)(PEBBLEGPU_AUTO_SCALE_MAX | PEBBLEGPU_AUTO_SCALE_MIN)) return fail(PEBBLEGPU_E_INVALID, "unknown auto-scale flags 0x%x", flags);
    if (flags == PEBBLEGPU_AUTO_SCALE_MAX && fixed_min_db >= (double)kAutoMaxDbLimit)
        return fail(PEBBLEGPU_E_INVALID, "auto-scaled max_db may come out %d: a fixed min_db of %g leaves no range", kAutoMaxDbLimit, fixed_min_db);
    if (flags == PEBBLEGPU_AUTO_SCALE_MIN && fixed_max_db <= (double)kAutoMinDbLimit)
        return fail(PEBBLEGPU_E_INVALID, "auto-scaled min_db may come out %d: a fixed max_db of %g leaves no range", kAutoMinDbLimit, fixed_max_db);
    return 0;
}

void display_pack_plan(DisplayPack *p, int32_t bins, double sample_rate, const pebblegpu_screen_map *map)
{
    memset(&p->sh, 0, sizeof(p->sh));
    memset(&p->geom, 0, sizeof(p->geom));
    p->sh.fft_size = bins;
    p->group = 1;
    if (p->format == PEBBLEGPU_DISPLAY_DB_F32) {
        p->row_elems = (uint32_t)bins;
    } else {
        p->sh.x_pixels = map->x_pixels;
        p->sh.y_pixels = map->y_pixels;
        p->sh.y_scale = map_y_scale(map->y_pixels, map->max_db, map->min_db);
        p->sh.max_db = map->max_db;
        p->min_db = map->min_db;
        p->geom = map_geom(bins, sample_rate, map->start_freq, map->stop_freq, map->x_pixels);
        p->group = map_lane_group(p->geom.bins_to_plot > map->x_pixels ? p->geom.bins_per_pixel : 0.0f);  // as run_screen_map sizes it
        p->row_elems = (uint32_t)map->x_pixels;
    }
    p->row_pitch_bytes = ((uint64_t)p->row_elems * 4 + 15) & ~(uint64_t)15;
}

int run_display_pack(hipStream_t s, const DisplayPack &p, const float *spec, long long pitch_rows, int first_row, int n_rows, void *dst, const ScaleUse &su)
{
    if (n_rows <= 0 || p.n_streams == 0) return 0;
    const long long bins = p.sh.fft_size, stream_pitch = pitch_rows * bins;
    const unsigned long long stream_bytes = (unsigned long long)n_rows * p.row_pitch_bytes;
    unsigned char *out = (unsigned char *)dst;
    if (p.format == PEBBLEGPU_DISPLAY_DB_F32) {
        const long long total = (long long)p.n_streams * n_rows;
        const dim3 grid((unsigned)std::min<long long>((bins / 4 + 255) / 256 + 1, 64), (unsigned)std::min<long long>(total, 65535));
        if (bins % 4) return fail(PEBBLEGPU_E_UNSUPPORTED, "%lld bins: display rows are copied in 16-byte vectors", bins);
        launch(k_display_rows, grid, dim3(256), s, spec, stream_pitch, bins, first_row, n_rows, total, (int)bins, p.d_tab, out,
               (unsigned long long)p.row_pitch_bytes, stream_bytes);
    } else {
        switch (p.group) {
        case 1: launch_display_map<1>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes, su); break;
        case 2: launch_display_map<2>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes, su); break;
        case 4: launch_display_map<4>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes, su); break;
        case 8: launch_display_map<8>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes, su); break;
        case 16: launch_display_map<16>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes, su); break;
        case 32: launch_display_map<32>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes, su); break;
        default: launch_display_map<64>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes, su); break;
        }
    }
    PG_HIP(hipGetLastError());
    return 0;
}

int run_display_panes(hipStream_t s, const DisplayPaneArgs *panes, int n_panes, const ScaleUse &su, const DisplayRow *trailer_tab)
{
    DisplayPaneArgs a[2];
    int n = 0;
    for (int k = 0; k < n_panes && k < 2; k++)
        if (panes[k].total_rows > 0) a[n++] = panes[k];
    if (!n) return 0;
    if (n == 1) {
        a[1] = a[0];
        a[1].total_rows = 0;
    }
    unsigned gx = 1;
    long long gy = 1;
    for (int k = 0; k < n; k++) {
        gx = std::max(gx, a[k].x_blocks);
        gy = std::max(gy, a[k].total_rows);
    }
    launch(k_display_panes, dim3(gx, (unsigned)std::min<long long>(gy, 4096), (unsigned)n), dim3(256), s, a[0], a[1], su, trailer_tab);
    PG_HIP(hipGetLastError());
    return 0;
}

// the host twin of the waterfall's colour rule (no device)
int waterfall_colors(const int32_t *pixels, uint64_t n, uint32_t *argb)
{
    for (uint64_t i = 0; i < n; i++) {
        if (pixels[i] < 0 || pixels[i] > 255) return fail(PEBBLEGPU_E_INVALID, "pixel %llu is %d: a waterfall pixel is 0..255", (unsigned long long)i, pixels[i]);
        argb[i] = waterfall_color(pixels[i]);
    }
    return 0;
}

int check_screen_map(int32_t y_pixels, int32_t x_pixels, double max_db, double min_db)
{
    if (x_pixels <= 0 || y_pixels <= 0) return fail(PEBBLEGPU_E_INVALID, "plot of %d x %d pixels", x_pixels, y_pixels);
    if (max_db == min_db) return fail(PEBBLEGPU_E_INVALID, "max_db == min_db (%g): no dB range to scale", max_db);
    return 0;
}

// SignalSpectrum::mapFFTZoomedToScreen (application/signalspectrum.cpp:151-167): quint16 span = hiResSampleRate * zoom, then
// (-span/2 - modeOffset, span/2 - modeOffset) in int.  A product of 65536 or more does not fit the quint16: the conversion is
// undefined in C; x86-64 truncates to int32 (INT_MIN when that overflows too) and keeps the low 16 bits, and so does this.
void zoom_span_edges(uint32_t hires_rate, double zoom, int32_t mode_offset, int32_t *start, int32_t *stop)
{
#pragma clang fp contract(off)
    const uint16_t span = (uint16_t)(uint32_t)x86_trunc((double)hires_rate * zoom);
    *start = (int32_t)((uint32_t)(-(int32_t)span / 2) - (uint32_t)mode_offset);  // (int arithmetic that wraps as on x86-64)
    *stop = (int32_t)((uint32_t)((int32_t)span / 2) - (uint32_t)mode_offset);
}

// ---- the receiver's display ring: one or two panes per block (include/pebblegpu.h, "The receiver's display ring") ----
// One EgressRing whose "row" is a whole slot: the panes of a call lie behind one another in it, compact, so one copy and one event carry
// them all; what each pane of a slot holds is kept beside the ring (written between begin() and commit(), read behind next(): the
// ring's lock orders the two).
constexpr uint64_t kMaxDisplayRingBytes = 1ull << 30;  // pinned host memory the ring may hold, all slots together (the stream bank's limit)

struct DisplayRing {
    struct Pane {
        uint32_t source = 0, format = 0, max_rows = 0;
        std::vector<uint32_t> sel;       // row r of the pane is stream / channel sel[r]
        uint32_t row_elems = 0;          // bins (DB_F32) or x_pixels
        uint64_t row_pitch = 0;          // bytes, a multiple of 16
        uint64_t cap_pitch = 0;          // ... what the slots were sized for at open
        MapShared sh{};
        double min_db = 0;               // the map's lower end (sh has the upper one)
        unsigned x_blocks = 1;
        std::vector<DisplayRow> tab;     // the device table's host copy
        DevBuf<DisplayRow> d_tab;
    };
    struct SlotPane { uint32_t rows, first_row, row_elems; uint64_t row_pitch, offset; };
    EgressRing ring;
    uint32_t n_panes = 0;                // 0: closed
    uint32_t fmt[PEBBLEGPU_DISPLAY_MAX_PANES] = {}, n_sel[PEBBLEGPU_DISPLAY_MAX_PANES] = {};  // fixed at open (what the reader may look at)
    Pane pane[PEBBLEGPU_DISPLAY_MAX_PANES];
    SlotPane info[kEgressMaxSlots][PEBBLEGPU_DISPLAY_MAX_PANES] = {};
    hipEvent_t packed2[kEgressMaxSlots] = {};  // behind the first pane's launch when the two panes are packed on different streams
    bool dirty = false;                  // a table changed: uploaded at the next call's boundary
    // auto-scale (SpectrumWidget::recalcScale): host flags consumed when the next call is queued -- never a wait
    uint32_t scale_flags = 0;            // PEBBLEGPU_AUTO_SCALE_* as last set
    uint32_t scale_live = 0;             // ... those whose end of the range a recalc has computed since the flag went on
    bool scale_pending = false;          // m_scaleNeedsRecalc
    DevBuf<ScaleEntry> d_scale;          // [streams] the ranges, written by k_scale_stats in a recalc call
    hipEvent_t scale_ev = nullptr;       // behind that launch, for the panes packed on the other stream (the recalc call only)
    hipEvent_t scale_rd_ev = nullptr;    // ... and in front of it: behind everything queued on the other stream so far (the table's readers there)
    uint64_t trailer_cap = 0;            // bytes of a slot kept for the trailer
    struct SlotScale { bool on; uint32_t n; uint64_t offset; };
    SlotScale scale_info[kEgressMaxSlots] = {};

    void free_device()
    {
        d_scale.release();
        if (scale_ev) (void)hipEventDestroy(scale_ev);
        scale_ev = nullptr;
        if (scale_rd_ev) (void)hipEventDestroy(scale_rd_ev);
        scale_rd_ev = nullptr;
        scale_flags = scale_live = 0;
        scale_pending = false;
        for (Pane &p : pane) p.d_tab.release();
        for (hipEvent_t &e : packed2) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
};

// a pane's request checked against the receiver and turned into its table and launch geometry (no device call)
static int plan_pane(const Receiver &rx, const pebblegpu_display_pane *p, DisplayRing::Pane *out)
{
    if (p->struct_size != sizeof(pebblegpu_display_pane)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_display_pane size mismatch");
    if (p->source != PEBBLEGPU_PANE_SPECTRUM && p->source != PEBBLEGPU_PANE_ZOOM) return fail(PEBBLEGPU_E_INVALID, "unknown pane source %u", p->source);
    if (p->format != PEBBLEGPU_DISPLAY_DB_F32 && p->format != PEBBLEGPU_DISPLAY_PIXELS_I32 && p->format != PEBBLEGPU_DISPLAY_WATERFALL_ARGB32)
        return fail(PEBBLEGPU_E_INVALID, "unknown display format %u", p->format);
    const bool zoom = p->source == PEBBLEGPU_PANE_ZOOM;
    const uint32_t fft = zoom ? rx.zoom_bins : rx.bins, n_src = zoom ? rx.C : rx.S;
    if (!fft) return fail(PEBBLEGPU_E_INVALID, zoom ? "the receiver computes no zoomed spectrum (hires_bins = 0)" : "the receiver computes no spectrum (spectrum_bins = 0)");
    out->source = p->source;
    out->format = p->format;
    out->sel.clear();
    if (!p->rows) {
        for (uint32_t c = 0; c < n_src; c++) out->sel.push_back(c);
    } else {
        if (p->n_rows == 0) return fail(PEBBLEGPU_E_INVALID, "an empty row selection");
        std::vector<char> seen(n_src, 0);
        for (uint32_t i = 0; i < p->n_rows; i++) {
            if (p->rows[i] >= n_src) return fail(PEBBLEGPU_E_INVALID, "%s %u out of range", zoom ? "channel" : "stream", p->rows[i]);
            if (seen[p->rows[i]]) return fail(PEBBLEGPU_E_INVALID, "%s %u is listed twice", zoom ? "channel" : "stream", p->rows[i]);
            seen[p->rows[i]] = 1;
            out->sel.push_back(p->rows[i]);
        }
    }
    // no call computes more rows than its capacity holds frames (the zoomed transform: decimated frames)
    const uint64_t cap = (uint64_t)rx.max_sf * rx.superframe, maxr = std::max<uint64_t>(1, zoom ? cap / ((uint64_t)rx.chain.total * rx.nf) : cap / rx.nf);
    out->max_rows = (uint32_t)(p->max_rows && p->max_rows < maxr ? p->max_rows : maxr);
    memset(&out->sh, 0, sizeof(out->sh));
    out->sh.fft_size = (int32_t)fft;
    out->tab.assign(out->sel.size(), DisplayRow{});
    for (size_t r = 0; r < out->sel.size(); r++) {
        out->tab[r].src = out->sel[r];
        out->tab[r].group = 1;
        out->tab[r].scale_src = zoom ? (rx.shared_input ? 0u : out->sel[r]) : out->sel[r];  // m_plotMaxDb / m_plotMinDb are the widget's: the zoomed panel takes its stream's range
    }
    if (p->format == PEBBLEGPU_DISPLAY_DB_F32) {
        if (fft % 4) return fail(PEBBLEGPU_E_UNSUPPORTED, "%u bins: display rows are copied in 16-byte vectors", fft);
        out->row_elems = fft;
        out->x_blocks = std::min<unsigned>((fft / 4 + 255) / 256, 16);
    } else {
        const pebblegpu_screen_map &m = p->map;
        if (m.struct_size != sizeof(pebblegpu_screen_map)) return fail(PEBBLEGPU_E_INVALID, "display format %u needs a pebblegpu_screen_map (struct_size set)", p->format);
        if (int rc = check_screen_map(m.y_pixels, m.x_pixels, m.max_db, m.min_db)) return rc;
        if (p->format == PEBBLEGPU_DISPLAY_WATERFALL_ARGB32 && m.y_pixels != 255)
            return fail(PEBBLEGPU_E_INVALID, "the waterfall's palette is indexed by pixels of a 255-pixel plot, not %d (spectrumwidget.cpp:1285-1293)", m.y_pixels);
        if (zoom && !std::isfinite(p->zoom)) return fail(PEBBLEGPU_E_INVALID, "zoom must be finite");
        // the edges and the per_stream decision of pebblegpu_receiver_map_spectrum / _map_zoom_spectrum, then run_screen_map's plan for every row
        std::vector<int32_t> edges(2 * (size_t)n_src);
        bool same = true;
        if (zoom) {
            for (uint32_t c = 0; c < n_src; c++) {
                zoom_span_edges(rx.demod_rate_int, p->zoom, p->mode_offset ? p->mode_offset[c] : 0, &edges[2 * c], &edges[2 * c + 1]);
                same = same && edges[2 * c] == edges[0] && edges[2 * c + 1] == edges[1];
            }
        } else {
            edges[0] = m.start_freq;
            edges[1] = m.stop_freq;
        }
        std::vector<MapGeom> geoms(n_src);
        std::vector<int> groups(n_src);
        map_row_plan((int32_t)fft, zoom ? (double)rx.demod_rate_int : rx.fs, edges.data(), zoom && !same, (int)n_src, m.x_pixels, geoms.data(), groups.data());
        int gmax = 1;
        for (size_t r = 0; r < out->sel.size(); r++) {
            out->tab[r].geom = geoms[out->sel[r]];
            out->tab[r].group = groups[out->sel[r]];
            gmax = std::max(gmax, groups[out->sel[r]]);
        }
        out->sh.x_pixels = m.x_pixels;
        out->sh.y_pixels = m.y_pixels;
        out->sh.y_scale = map_y_scale(m.y_pixels, m.max_db, m.min_db);
        out->sh.max_db = m.max_db;
        out->min_db = m.min_db;
        out->row_elems = (uint32_t)m.x_pixels;
        const long long per_wg = 256 / gmax;
        out->x_blocks = (unsigned)std::min<long long>(((long long)m.x_pixels + per_wg - 1) / per_wg, 64);
    }
    out->row_pitch = ((uint64_t)out->row_elems * 4 + 15) & ~(uint64_t)15;
    return 0;
}

int Receiver::display_open(const pebblegpu_display_pane *panes, uint32_t n_panes, uint32_t n_slots)
{
    if (!panes) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (n_panes < 1 || n_panes > PEBBLEGPU_DISPLAY_MAX_PANES) return fail(PEBBLEGPU_E_INVALID, "n_panes %u: a block has 1..%d panes", n_panes, PEBBLEGPU_DISPLAY_MAX_PANES);
    if (int rc = check_egress_slots(n_slots)) return rc;
    DisplayRing::Pane plan[PEBBLEGPU_DISPLAY_MAX_PANES];
    uint64_t slot_bytes = 0;
    for (uint32_t k = 0; k < n_panes; k++) {
        if (int rc = plan_pane(*this, &panes[k], &plan[k])) return rc;
        plan[k].cap_pitch = plan[k].row_pitch;
        const uint64_t rows = (uint64_t)plan[k].sel.size() * plan[k].max_rows;
        if (rows > kMaxDisplayRingBytes / plan[k].row_pitch) slot_bytes = kMaxDisplayRingBytes + 1;  // (and no overflow)
        else slot_bytes += rows * plan[k].row_pitch;
    }
    const uint64_t trailer_cap = ((uint64_t)plan[0].sel.size() * sizeof(ScaleEntry) + 15) & ~(uint64_t)15;  // room behind the panes for the auto-scale trailer
    if (slot_bytes <= kMaxDisplayRingBytes) slot_bytes += trailer_cap;
    std::lock_guard<std::mutex> g(mu_);
    if (disp_open_) return fail(PEBBLEGPU_E_INVALID, "the display ring is already open");
    if (slot_bytes > kMaxDisplayRingBytes || slot_bytes * n_slots > kMaxDisplayRingBytes)
        return fail(PEBBLEGPU_E_SIZE, "%u slots of %llu bytes: a ring pins at most %llu bytes of host memory", n_slots, (unsigned long long)slot_bytes,
                    (unsigned long long)kMaxDisplayRingBytes);
    PG_HIP(hipSetDevice(device));
    if (!disp_) disp_ = new (std::nothrow) DisplayRing();
    if (!disp_) return fail(PEBBLEGPU_E_INVALID, "out of host memory");
    DisplayRing &d = *disp_;
    std::lock_guard<std::mutex> lk(d.ring.mu);
    auto body = [&]() -> int {
        for (uint32_t k = 0; k < n_panes; k++) PG_TRY(plan[k].d_tab.alloc(plan[k].tab.size()));
        // the auto-scale trailer holds pane 0's selected rows; the ranges' table one entry per stream
        d.trailer_cap = trailer_cap;
        PG_TRY(d.d_scale.alloc_zero(S));
        PG_HIP(hipEventCreateWithFlags(&d.scale_ev, hipEventDisableTiming));
        PG_HIP(hipEventCreateWithFlags(&d.scale_rd_ev, hipEventDisableTiming));
        if (int rc = d.ring.open_ring(n_slots, 1, 4, (slot_bytes - trailer_cap) / 4, 0, trailer_cap)) return rc;
        for (uint32_t i = 0; i < n_slots; i++) {
            PG_HIP(hipMemset(d.ring.slot[i].d, 0, d.ring.slot_bytes));  // (the padding of a row is never written)
            PG_HIP(hipEventCreateWithFlags(&d.packed2[i], hipEventDisableTiming));
        }
        PG_HIP(hipStreamSynchronize(nullptr));  // (the clears are over before a packing kernel on the receiver's own streams can run)
        return 0;
    };
    if (int rc = body()) {
        d.ring.release();
        d.free_device();
        return rc;  // (the planned panes' tables go with `plan`)
    }
    for (uint32_t k = 0; k < n_panes; k++) {
        d.fmt[k] = plan[k].format;
        d.n_sel[k] = (uint32_t)plan[k].sel.size();
        d.pane[k] = std::move(plan[k]);
    }
    d.n_panes = n_panes;
    d.dirty = true;
    disp_open_ = true;
    return 0;
}

int Receiver::display_close()
{
    std::lock_guard<std::mutex> g(mu_);
    if (!disp_open_) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    if (int rc = sync()) return rc;
    disp_->ring.close_ring();  // (waits for a reader that is inside _next)
    disp_->n_panes = 0;
    disp_->free_device();
    disp_open_ = false;
    return 0;
}

// ~Receiver, behind the synchronisation of both streams
void Receiver::display_destroy()
{
    if (!disp_) return;
    if (disp_->ring.open) disp_->ring.close_ring();
    else disp_->ring.release();
    disp_->free_device();
    delete disp_;
    disp_ = nullptr;
    disp_open_ = false;
}

int Receiver::display_set_pane(uint32_t pane, const pebblegpu_display_pane *p)
{
    if (!p) return fail(PEBBLEGPU_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(mu_);
    if (!disp_open_) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    if (pane >= disp_->n_panes) return fail(PEBBLEGPU_E_INVALID, "pane %u: the ring has %u", pane, disp_->n_panes);
    DisplayRing::Pane &cur = disp_->pane[pane];
    if (p->source != cur.source || p->format != cur.format)
        return fail(PEBBLEGPU_E_INVALID, "a pane keeps the source and the format it was opened with: close and open the ring to change them");
    pebblegpu_display_pane q = *p;  // ... and its selection and max_rows
    q.rows = cur.sel.data();
    q.n_rows = (uint32_t)cur.sel.size();
    q.max_rows = cur.max_rows;
    DisplayRing::Pane next;
    if (int rc = plan_pane(*this, &q, &next)) return rc;
    if (next.row_pitch > cur.cap_pitch)
        return fail(PEBBLEGPU_E_SIZE, "rows of %llu bytes: the slots were sized for %llu at open", (unsigned long long)next.row_pitch, (unsigned long long)cur.cap_pitch);
    if (next.format != PEBBLEGPU_DISPLAY_DB_F32) {  // (against the flags, and against the ends the table supplies until a pending recalc lands)
        if (int rc = check_auto_scale(disp_->scale_flags, next.sh.max_db, next.min_db)) return rc;
        if (int rc = check_auto_scale(disp_->scale_flags & disp_->scale_live, next.sh.max_db, next.min_db)) return rc;
    }
    next.cap_pitch = cur.cap_pitch;
    next.d_tab = std::move(cur.d_tab);
    cur = std::move(next);
    disp_->dirty = true;
    return 0;
}

// the panes' tables for the coming call.  Rare (open, set_pane): both streams are drained first, since the packing kernel of an earlier
// call may still be reading a table -- as the audio ring's table is refreshed
int Receiver::upload_display_tables()
{
    if (!disp_->dirty) return 0;
    PG_HIP(hipStreamSynchronize(stream_));
    PG_HIP(hipStreamSynchronize(chain_stream_));
    for (uint32_t k = 0; k < disp_->n_panes; k++) {
        const DisplayRing::Pane &p = disp_->pane[k];
        PG_HIP(hipMemcpy(p.d_tab, p.tab.data(), sizeof(DisplayRow) * p.tab.size(), hipMemcpyHostToDevice));
    }
    disp_->dirty = false;
    return 0;
}

// The block of an accepted call.  spec_rows / zoom_rows: the rows THIS call computed (compact in d_spec / d_zoom), complete on spec_s /
// zoom_s -- where Receiver::map_spectrum would queue its map, and where the next call's transform of the same buffer follows.  Both
// panes on one stream: one launch; else one per pane, and the slot's copy waits for both.
int Receiver::queue_display_block(hipStream_t spec_s, uint64_t spec_rows, hipStream_t zoom_s, uint64_t zoom_rows, bool rescale)
{
    DisplayRing &d = *disp_;
    // SpectrumWidget::recalcScale on this call's first computed row of every stream (spectrumwidget.cpp:1184-1187: "wait for next fft to
    // have new data" -- a call that computed none leaves the request pending).  Whether the block is delivered or dropped: what later
    // blocks look like never depends on the reader
    const bool recalc = rescale && d.scale_flags && d.scale_pending && spec_rows > 0;
    if (recalc) {
        // The table's readers are the packing launches of earlier calls.  Those on spec_s precede the write in stream order.  A call whose two
        // pipelines are not joined (PEBBLEGPU_PIPELINE=1) may have zoomed-pane launches of ANY earlier call still queued on the other stream,
        // which the main stream never waits for: the write waits for everything queued there so far, and that stream -- this call's zoomed
        // pane and every later one -- is ordered behind the write.  Two records and two waits, in the recalc call only
        const bool two = zoom_s != spec_s;
        if (two) {
            PG_HIP(hipEventRecord(d.scale_rd_ev, zoom_s));
            PG_HIP(hipStreamWaitEvent(spec_s, d.scale_rd_ev, 0));
        }
        if (int rc = run_scale_stats(spec_s, d_spec, (long long)spec_rows * bins, 0, (int)S, 1, (int)bins, d.d_scale)) return rc;
        if (two) {
            PG_HIP(hipEventRecord(d.scale_ev, spec_s));
            PG_HIP(hipStreamWaitEvent(zoom_s, d.scale_ev, 0));
        }
        d.scale_live = d.scale_flags;
        d.scale_pending = false;
    }
    EgressSlot *g = d.ring.begin();
    if (!g) return 0;
    const int si = (int)(g - d.ring.slot);
    DisplayPaneArgs a[PEBBLEGPU_DISPLAY_MAX_PANES];
    hipStream_t st[PEBBLEGPU_DISPLAY_MAX_PANES] = {};
    uint64_t off = 0;
    for (uint32_t k = 0; k < d.n_panes; k++) {
        const DisplayRing::Pane &p = d.pane[k];
        const bool zoom = p.source == PEBBLEGPU_PANE_ZOOM;
        const uint64_t computed = zoom ? zoom_rows : spec_rows, n = std::min<uint64_t>(computed, p.max_rows), first = computed - n;
        d.info[si][k] = DisplayRing::SlotPane{(uint32_t)n, (uint32_t)first, p.row_elems, p.row_pitch, off};
        DisplayPaneArgs &q = a[k];
        q.in = zoom ? d_zoom : d_spec;
        q.stream_pitch = (long long)computed * p.sh.fft_size;
        q.first_row = (int)first;
        q.n_rows = (int)n;
        q.total_rows = (long long)p.sel.size() * (long long)n;
        q.tab = p.d_tab;
        q.format = (int)p.format;
        q.x_blocks = p.x_blocks;
        q.sh = p.sh;
        q.out = (unsigned char *)g->d + off;
        q.out_row_pitch = p.row_pitch;
        q.min_db = p.min_db;
        st[k] = zoom ? zoom_s : spec_s;
        off += (uint64_t)q.total_rows * p.row_pitch;
    }
    g->aux = (uint32_t)si;
    // auto-scale: the ranges by value in the launch, the ranges used into a trailer behind the panes (inside the one copy).  A block
    // without a row of any pane stays what it was: nothing queued, no trailer
    ScaleUse su, su_rest;
    uint64_t trailer = 0;
    d.scale_info[si] = DisplayRing::SlotScale{false, 0, 0};
    if (d.scale_flags && off) {
        su.tab = d.d_scale;
        su.use = d.scale_flags & d.scale_live;
        su.refreshed = recalc ? 1u : 0u;
        su_rest = su;
        su.trailer = reinterpret_cast<ScaleEntry *>((unsigned char *)g->d + off);
        su.n_trailer = (uint32_t)d.pane[0].sel.size();
        su.fixed_max = d.pane[0].sh.max_db;
        su.fixed_min = d.pane[0].min_db;
        d.scale_info[si] = DisplayRing::SlotScale{true, su.n_trailer, off};
        trailer = d.trailer_cap;
    }
    hipStream_t last = st[0];
    if (d.n_panes == 2 && st[0] != st[1] && a[0].total_rows && a[1].total_rows) {
        if (int rc = run_display_panes(st[0], &a[0], 1, su, d.pane[0].d_tab)) return rc;
        PG_HIP(hipEventRecord(d.packed2[si], st[0]));
        PG_HIP(hipStreamWaitEvent(d.ring.copy_stream, d.packed2[si], 0));
        if (int rc = run_display_panes(st[1], &a[1], 1, su_rest, nullptr)) return rc;
        last = st[1];
    } else {
        if (d.n_panes == 2 && !a[0].total_rows) last = st[1];
        if (int rc = run_display_panes(last, a, (int)d.n_panes, su, d.pane[0].d_tab)) return rc;
    }
    return d.ring.commit(g, last, off / 4, trailer);  // (a "sample" is 4 bytes; 0: nothing is queued at all)
}

// ---- auto-scale: the pull function and the ring's flags ----
bool Receiver::display_scale_pending() const { return disp_open_ && disp_->scale_flags && disp_->scale_pending; }

int Receiver::spectrum_scale(uint32_t first, uint32_t n, uint32_t step, pebblegpu_display_scale *d_out)
{
    std::lock_guard<std::mutex> g(mu_);
    if (!d_out) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (failed_) return fail(PEBBLEGPU_E_HIP, "an earlier call on this receiver failed half-way: its spectra are not defined");
    if (!bins) return fail(PEBBLEGPU_E_INVALID, "the receiver computes no spectrum (spectrum_bins = 0)");
    uint64_t frames = last_spec_frames;
    const bool carried = gated() && !frames && have_carry_;  // as pebblegpu_receiver_map_spectrum: the spectrum the display still holds, as row 0
    if (carried) frames = 1;
    if (!frames) return fail(PEBBLEGPU_E_INVALID, "no call with a spectrum has been made yet");
    if (n == 0 || (uint64_t)first + (uint64_t)(n - 1) * step >= frames)
        return fail(PEBBLEGPU_E_INVALID, "frames %u + j * %u, j < %u, are not all within the last call's %llu", first, step, n, (unsigned long long)frames);
    PG_HIP(hipSetDevice(device));
    if (int rc = close_timing()) return rc;
    const float *src = carried ? d_spec_carry : d_spec + (long long)first * bins;
    return run_scale_stats(stream_, src, (long long)frames * bins, (long long)step * bins, (int)S, (int)n, (int)bins, reinterpret_cast<ScaleEntry *>(d_out));
}

int Receiver::display_set_auto_scale(uint32_t flags)
{
    std::lock_guard<std::mutex> g(mu_);
    if (!disp_open_) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    if (!bins) return fail(PEBBLEGPU_E_INVALID, "the range comes from the unprocessed spectrum: the receiver computes none (spectrum_bins = 0)");
    DisplayRing &d = *disp_;
    if (int rc = check_auto_scale(flags, 0.0, -120.0)) return rc;  // (the flag bits)
    // (the one-flag refusals hold for the flags and for the ends the table supplies until the recalc lands: flags & live)
    for (uint32_t k = 0; k < d.n_panes; k++)
        if (d.pane[k].format != PEBBLEGPU_DISPLAY_DB_F32) {
            if (int rc = check_auto_scale(flags, d.pane[k].sh.max_db, d.pane[k].min_db)) return rc;
            if (int rc = check_auto_scale(flags & d.scale_live, d.pane[k].sh.max_db, d.pane[k].min_db)) return rc;
        }
    if (flags & ~d.scale_flags) d.scale_pending = true;  // maxDbChanged / minDbChanged with "Auto": m_scaleNeedsRecalc = true (spectrumwidget.cpp:942, :960)
    d.scale_live &= flags;                               // a flag that goes off returns its end to the pane's map (m_plotMaxDb = db)
    d.scale_flags = flags;
    if (!flags) d.scale_pending = false;
    return 0;
}
int Receiver::display_rescale()
{
    std::lock_guard<std::mutex> g(mu_);
    if (!disp_open_) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    disp_->scale_pending = disp_->scale_flags != 0;  // (recalcScale returns at once with neither flag on)
    return 0;
}
int Receiver::display_scale(uint64_t call_index, pebblegpu_display_scale *out, uint32_t cap, uint32_t *n)
{
    if (!n) return fail(PEBBLEGPU_E_INVALID, "null argument");
    *n = 0;
    if (!disp_) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    DisplayRing &d = *disp_;
    std::lock_guard<std::mutex> lk(d.ring.mu);
    if (!d.ring.open) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    for (uint64_t q = d.ring.tail; q < d.ring.read; q++) {
        const uint32_t si = (uint32_t)(q % d.ring.n_slots);
        const EgressSlot &g = d.ring.slot[si];
        if (g.call != call_index) continue;
        const DisplayRing::SlotScale &z = d.scale_info[si];
        if (!z.on) return fail(PEBBLEGPU_E_INVALID, "the block of call %llu carries no ranges: no auto-scale flag was on when it was queued, or it has no rows", (unsigned long long)call_index);
        if (z.n > cap) return fail(PEBBLEGPU_E_SIZE, "%u ranges do not fit %u entries", z.n, cap);
        if (z.n && !out) return fail(PEBBLEGPU_E_INVALID, "null argument");
        memcpy(out, (const unsigned char *)g.h + z.offset, sizeof(pebblegpu_display_scale) * z.n);
        *n = z.n;
        return 0;
    }
    return fail(PEBBLEGPU_E_INVALID, "call %llu is not handed out", (unsigned long long)call_index);
}

int Receiver::display_next(int wait, pebblegpu_display_block *b)
{
    if (!b) return fail(PEBBLEGPU_E_INVALID, "null argument");
    const uint32_t n = disp_ ? disp_->n_panes : 0;
    if (!n) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    for (uint32_t k = 0; k < n; k++)
        if (b[k].struct_size != sizeof(pebblegpu_display_block)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_display_block size mismatch (pane %u)", k);
    EgressBlock e;
    if (int rc = disp_->ring.next(device, wait, &e)) return rc;
    for (uint32_t k = 0; k < n; k++) {
        pebblegpu_display_block &o = b[k];
        const DisplayRing::SlotPane z{}, &q = e.host ? disp_->info[e.aux % kEgressMaxSlots][k] : z;
        o.format = disp_->fmt[k];
        o.call_index = e.call;
        o.host = e.host ? (const unsigned char *)e.host + q.offset : nullptr;
        o.rows_per_stream = q.rows;
        o.first_row = q.first_row;
        o.row_elems = q.row_elems;
        o.n_streams = disp_->n_sel[k];
        o.dropped_before = e.host ? e.dropped_before : 0;
        o.reserved = 0;
        o.row_pitch_bytes = q.row_pitch;
        o.stream_pitch_bytes = (uint64_t)q.rows * q.row_pitch;
    }
    return 0;
}
int Receiver::display_release(uint64_t call_index)
{
    if (!disp_) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    return disp_->ring.finish(call_index);
}
int Receiver::display_dropped(uint64_t *blocks)
{
    if (!disp_) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    std::lock_guard<std::mutex> lk(disp_->ring.mu);
    if (!disp_->ring.open) return fail(PEBBLEGPU_E_INVALID, "the display ring is not open");
    *blocks = disp_->ring.dropped;
    return 0;
}

}  // namespace pg
