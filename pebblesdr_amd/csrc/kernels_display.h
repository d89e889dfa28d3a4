// kernels_display.h -- FFT::mapFFTToScreen (pebblelib/fft.cpp:400-534) on the device: rows of float dB (-f..+f, as the display
// transforms leave them) to rows of x_pixels int32 plot heights, the last step of the spectrum path before SpectrumWidget draws.
//
// What the reference computes, restated (fft.cpp:411-534, x86-64 arithmetic):
//   binsPerHz    = (float)fftSize / (float)sampleRate                                       float
//   binLow       = (int)((float)startFreq * binsPerHz) + fftSize/2, binHigh the same with stopFreq    (float -> int truncates)
//   fftBinsToPlot = binHigh - binLow;  pixelsPerBin = (float)xPixels / (float)fftBinsToPlot;  binsPerPixel its inverse   float
//   yScaleFactor = (float)(-yPixels / (maxdB - mindB))                                      double, then float
//   fftBinsToPlot > xPixels (:470-508): pixel i reads bin = (int)((float)binLow + (float)i * binsPerPixel);
//       out of [0, fftSize): powerdB = DB::minDb = -120 (no maxdB offset);
//       else if lastFftBin > 0 (strictly) and bin != lastFftBin + 1, lastFftBin being pixel i-1's bin (-1 for pixel 0):
//           powerdB = (int)(powerTodB(sum_{b in [lastFftBin, bin)} pow(10, dB[b] / 10.0) / (bin - lastFftBin)) - maxdB)
//           with powerTodB(0) = -120 and 10 log10(p) otherwise -- the window holds the previous pixel's bin, not its own;
//       else powerdB = (int)(dB[bin] - maxdB)
//   otherwise (:510-527): bin = (int)((float)binLow + (float)i / pixelsPerBin), never averaged
//   yPixel = qBound(0, (int)(yScaleFactor * (float)powerdB - 1.0f), yPixels - 1)
// lastFftBin is the previous pixel's bin in closed form, so every pixel is independent: no scan.  Float and double expressions
// are evaluated without contraction (hipcc would fuse a*b+c into an FMA on the device and move the truncation boundaries), and
// every float -> int conversion is x86-64's cvtts*2si: toward zero, INT_MIN for NaN and out of range (C leaves those undefined;
// the host the reference runs on does this).  Int sums that may wrap (binLow + fftSize/2, binHigh - binLow) wrap as on x86-64.
//
// Layout (the hot case is many bins per pixel): a group of G lanes (a power of two near binsPerPixel, up to a wave) owns one pixel;
// its lanes walk the pixel's bins, so a wave's loads cover one contiguous stretch of the row; the per-bin power is double; one
// shuffle reduction per pixel segment.  Items are (row, pixel) pairs, grid-strided, so rows spread over all workgroups.
#pragma once
#include <climits>
#include "common.h"
#include "screen_geom.h"

struct pebblegpu_screen_map;  // include/pebblegpu.h

namespace pg {

constexpr int kMinDb = -120;     // DB::minDb (pebblelib/db.cpp)

// x86_trunc, MapGeom, MapShared, map_geom, map_y_scale, map_bin, map_y and the lane-group plan (map_lane_group, map_chunk_plan,
// map_row_plan): screen_geom.h, the part of the map a host evaluates too
struct MapGeoms {
    int n;  // 1: every row uses g[0]; else row stream s (relative to the launch) uses g[s]
    MapGeom g[kMapMaxGeom];
};

// powerdB of pixel i of the dB row x (fft.cpp:470-527), for the G lanes that own the pixel: every lane of the group calls it with the
// same arguments and gets the same value.  Shared by k_screen_map and the display ring's packing kernel (k_display_map), so a block's
// pixels and pebblegpu_*_map_spectrum's are one computation.
template <int G>
__device__ inline int32_t map_power_db(const float *__restrict__ x, const MapGeom &g, const MapShared &sh, int32_t i, int lane)
{
#pragma clang fp contract(off)
    const bool averaged = g.bins_to_plot > sh.x_pixels;
    const int32_t bin = map_bin(g, averaged, i);
    if (bin < 0 || bin >= sh.fft_size) return kMinDb;
    const int32_t last = i == 0 ? -1 : map_bin(g, averaged, i - 1);
    if (averaged && last > 0 && bin != last + 1) {
        // bins [last, bin): 1 <= last, bin < fft_size, and last <= bin (the per-pixel bin never decreases)
        const int32_t skipped = bin - last;
        double acc = 0.0;
        for (int32_t k = lane; k < skipped; k += G) acc += exp10((double)x[last + k] / 10.0);  // DB::dBToPower
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, G);
        const double p = acc / (double)skipped;
        const double db = p == 0.0 ? (double)kMinDb : 10.0 * log10(p);  // DB::powerTodB
        return x86_trunc(db - sh.max_db);
    }
    return x86_trunc((double)x[bin] - sh.max_db);
}

// rows = streams x frames: row (s, j) reads in + s * stream_pitch + j * frame_pitch and writes out + (s * n_frames + j) * x_pixels
template <int G>
static __global__ __launch_bounds__(256) void k_screen_map(const float *__restrict__ in, long long stream_pitch, long long frame_pitch,
                                                           int n_frames, long long n_items, MapGeoms geoms, MapShared sh,
                                                           int32_t *__restrict__ out)
{
#pragma clang fp contract(off)
    constexpr int kGroups = 256 / G;
    const int lane = (int)threadIdx.x % G;
    const long long stride = (long long)gridDim.x * kGroups;
    for (long long item = (long long)blockIdx.x * kGroups + (int)threadIdx.x / G; item < n_items; item += stride) {
        const long long row = item / sh.x_pixels;
        const int32_t i = (int32_t)(item - row * sh.x_pixels);
        const int s = (int)(row / n_frames), j = (int)(row - (long long)s * n_frames);
        const MapGeom g = geoms.g[geoms.n == 1 ? 0 : s];
        const float *x = in + (long long)s * stream_pitch + (long long)j * frame_pitch;
        const int32_t power_db = map_power_db<G>(x, g, sh, i, lane);
        if (lane == 0) out[row * sh.x_pixels + i] = map_y(sh.y_scale, power_db, sh.y_pixels);
    }
}

// ---- SpectrumWidget::recalcScale (application/spectrumwidget.cpp:693-734): the plot range of AutoScaleMax / AutoScaleMin ----
// (both default true, application/settings.cpp:70-71).  One spectrum row of `bins` dB values, each widened to double:
//   pwr_i   = pow(10, dB_i / 10.0)                               DB::dBToPower, db.h:72-75                            (:706)
//   total  += pwr_i; if (pwr_i > peak) peak = pwr_i  (peak starts at 0);  avg = total / bins                          (:707-711)
//   newAvg  = (int)(powerTodB(avg) - 10)       powerTodB(0) = -120, else 10 * log10 (db.h:78-82); double -> int truncates   (:715)
//   newAvg  = (newAvg / 5) * 5                 C int division, toward zero                                            (:716)
//   min_db  = qBound(-120, newAvg, -70)        m_minDbScaleLimit, spectrumwidget.h:154                                (:717)
//   newPeak = (int)(powerTodB(peak) + 10); (newPeak / 5) * 5; max_db = qBound(-50, newPeak, 0)   m_maxDbScaleLimit, :153   (:723-725)
// The range comes from the unprocessed spectrum and applies to every pane (m_plotMaxDb / m_plotMinDb are the widget's).
constexpr int kAutoMinDbLimit = -70, kAutoMaxDbLimit = -50;
struct ScaleEntry {  // = pebblegpu_display_scale
    int32_t max_db, min_db;
    double avg_power, peak_power;
};
__host__ __device__ inline ScaleEntry auto_scale_finish(double total, double peak, int32_t bins)
{
#pragma clang fp contract(off)
    ScaleEntry e;
    e.avg_power = total / (double)bins;
    e.peak_power = peak;
    int32_t a = x86_trunc((e.avg_power == 0.0 ? (double)kMinDb : 10.0 * log10(e.avg_power)) - 10.0);
    a = (a / 5) * 5;
    e.min_db = a > kAutoMinDbLimit ? kAutoMinDbLimit : (a < kMinDb ? kMinDb : a);  // qBound(lo, v, hi) = max(lo, min(hi, v))
    int32_t p = x86_trunc((peak == 0.0 ? (double)kMinDb : 10.0 * log10(peak)) + 10.0);
    p = (p / 5) * 5;
    e.max_db = p > 0 ? 0 : (p < kAutoMaxDbLimit ? kAutoMaxDbLimit : p);
    return e;
}

// One 256-lane workgroup per row (grid = rows; row = s * n_frames + j reads in + s * stream_pitch + j * frame_pitch and writes out[row]).
// Rows are powers of two >= 2048 floats and 16-byte aligned (as the DB_F32 gather relies on): float4 loads, bins / 1024 per lane.  Each
// lane keeps a double sum and a double peak; xor-shuffle tree inside the wave, then the four waves' values through LDS, added in wave
// order by lane 0 -- no atomics, one fixed order, the same bits on every run.  Lane 0 finishes the integer rule.  A 65536-bin row is
// 256 KiB for one workgroup: the kernel runs when a recalc is pending or the pull function asks, never per call.
static __global__ __launch_bounds__(256) void k_scale_stats(const float *__restrict__ in, long long stream_pitch, long long frame_pitch, int n_frames,
                                                            int bins, ScaleEntry *__restrict__ out)
{
#pragma clang fp contract(off)
    const long long row = blockIdx.x;
    const long long s = row / n_frames, j = row - s * n_frames;
    const float4 *x = reinterpret_cast<const float4 *>(in + s * stream_pitch + j * frame_pitch);
    double sum = 0.0, peak = 0.0;
    for (int k = (int)threadIdx.x; k < bins / 4; k += 256) {
        const float4 v = x[k];
        const double p0 = exp10((double)v.x / 10.0), p1 = exp10((double)v.y / 10.0), p2 = exp10((double)v.z / 10.0), p3 = exp10((double)v.w / 10.0);
        sum += p0; sum += p1; sum += p2; sum += p3;
        if (p0 > peak) peak = p0;
        if (p1 > peak) peak = p1;
        if (p2 > peak) peak = p2;
        if (p3 > peak) peak = p3;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sum += __shfl_xor(sum, m, 64);
        const double o = __shfl_xor(peak, m, 64);
        if (o > peak) peak = o;
    }
    __shared__ double w_sum[4], w_peak[4];
    if ((threadIdx.x & 63) == 0) {
        w_sum[threadIdx.x >> 6] = sum;
        w_peak[threadIdx.x >> 6] = peak;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = w_sum[0], pk = w_peak[0];
        for (int w = 1; w < 4; w++) {
            total += w_sum[w];
            if (w_peak[w] > pk) pk = w_peak[w];
        }
        out[row] = auto_scale_finish(total, pk, bins);
    }
}
// the launch; rows = n_streams x n_frames
int run_scale_stats(hipStream_t s, const float *in, long long stream_pitch, long long frame_pitch, int n_streams, int n_frames, int bins, ScaleEntry *out);
// the host twin of one row, serial as the reference (no device)
ScaleEntry auto_scale_row(const float *db, uint32_t bins);
// the refusals a flag word shares: unknown bits; MAX alone against a fixed min_db >= -50 / MIN alone against a fixed max_db <= -70 (a range
// that could come out empty or upside down: the reference would divide by zero or flip the plot)
int check_auto_scale(uint32_t flags, double fixed_max_db, double fixed_min_db);

// A ring's ranges on the device: tab[stream] is the stream's range as the last recalc left it; `use` (the AUTO_SCALE bits whose end of the
// range has been computed since the flag went on) says which ends the packing kernel takes from it, the others stay the pane's map's.
// Carried by value in the packing launch: flags never wait for earlier calls.  use == 0: the kernels run exactly as without the table.
struct ScaleUse {
    const ScaleEntry *tab = nullptr;
    uint32_t use = 0;
    uint32_t refreshed = 0;           // this call's launch was preceded by the recalc: the trailer carries avg_power / peak_power
    ScaleEntry *trailer = nullptr;    // [n_trailer] the ranges used, per selected stream (nullptr: none)
    uint32_t n_trailer = 0;
    double fixed_max = 0, fixed_min = 0;  // the trailer's pane's own range
};
// max_db / y_scale of a row whose range is stream `src`'s
__device__ inline void scale_row_shared(const ScaleUse &u, uint32_t src, double fixed_min, MapShared *sh)
{
    const ScaleEntry e = u.tab[src];
    const double mx = (u.use & 1u) ? (double)e.max_db : sh->max_db, mn = (u.use & 2u) ? (double)e.min_db : fixed_min;
    sh->max_db = mx;
    sh->y_scale = map_y_scale(sh->y_pixels, mx, mn);
}
__device__ inline void scale_write_trailer(const ScaleUse &u, uint32_t r, uint32_t src)
{
    const ScaleEntry e = u.tab[src];
    ScaleEntry o;
    o.max_db = (u.use & 1u) ? e.max_db : (int32_t)u.fixed_max;
    o.min_db = (u.use & 2u) ? e.min_db : (int32_t)u.fixed_min;
    o.avg_power = u.refreshed ? e.avg_power : 0.0;
    o.peak_power = u.refreshed ? e.peak_power : 0.0;
    u.trailer[r] = o;
}

// ---- the waterfall's colours ----
// SpectrumWidget's palette (application/spectrumwidget.cpp:97-113), the constructor's loop in its own integer arithmetic, entry i as
// QColor::setRgb(r, g, b) leaves it: alpha 255, QRgb layout 0xFFRRGGBB.  The reference allocates 255 entries, writes entry 255 and
// reads it for a pixel value of 0, both out of bounds; here the table has 256 entries and entry 255 is what the loop computes for it.
__host__ __device__ inline uint32_t waterfall_palette(int i)
{
    int r, g, b;
    if (i < 43) { r = 0; g = 0; b = 255 * i / 43; }
    else if (i < 87) { r = 0; g = 255 * (i - 43) / 43; b = 255; }
    else if (i < 120) { r = 0; g = 255; b = 255 - (255 * (i - 87) / 32); }
    else if (i < 154) { r = 255 * (i - 120) / 33; g = 255; b = 0; }
    else if (i < 217) { r = 255; g = 255 - (255 * (i - 154) / 62); b = 0; }
    else { r = 255; g = 0; b = 128 * (i - 217) / 38; }
    return 0xFF000000u | ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b;
}
// SpectrumWidget::drawWaterfall, spectrumwidget.cpp:1111-1113: plotColor = m_spectrumColors[255 - _fftMap[i]]; v in 0..255
__host__ __device__ inline uint32_t waterfall_color(int32_t v) { return waterfall_palette(255 - v); }

// ---- the display ring's packing kernels (streambank.hip) ----
// what a display ring fixes at open: the format, the selection's table on the device, the plot geometry and its lane group
struct DisplayPack {
    int format = 0;                  // pebblegpu_display_format
    uint32_t n_streams = 0;          // selected streams: rows of d_tab
    uint32_t *d_tab = nullptr;       // a view of the owner's table: d_tab[r] = the stream of block row r
    uint32_t row_elems = 0;          // bins (DB_F32) or x_pixels
    uint64_t row_pitch_bytes = 0;    // row_elems * 4 rounded up to 16
    int group = 1;                   // the lane group run_screen_map picks for geom
    MapGeom geom;
    MapShared sh;                    // (DB_F32: fft_size only)
    double min_db = 0;               // the map's lower end (auto-scale with one flag on)
};
// fills everything but n_streams and d_tab from the format and (mapped formats) the checked map
void display_pack_plan(DisplayPack *p, int32_t bins, double sample_rate, const ::pebblegpu_screen_map *map);
// rows first_row .. first_row + n_rows - 1 of spec ([stream][pitch_rows][bins]) -> dst [selected][n_rows][row_pitch_bytes]; one launch
// su: the ring's ranges (ScaleUse{}: none, the launch as without auto-scale)
int run_display_pack(hipStream_t s, const DisplayPack &p, const float *spec, long long pitch_rows, int first_row, int n_rows, void *dst, const ScaleUse &su = ScaleUse{});
int waterfall_colors(const int32_t *pixels, uint64_t n, uint32_t *argb);

// Rows first_row .. first_row + n_rows - 1 of the selected streams of a compact spectrum buffer ([stream][pitch_rows][bins] float dB,
// tab[r] = the stream of block row r) into a block: row j of selected stream r at out + r * out_stream_pitch + j * out_row_pitch
// (bytes, multiples of 16).  ARGB false: FFT::mapFFTToScreen pixels, as k_screen_map writes them; true: drawWaterfall's colour of
// each pixel, with no int32 intermediate.  One geometry for all rows; G is the lane group run_screen_map picks for it, so the
// reduction adds in the same order.
template <int G, bool ARGB>
static __global__ __launch_bounds__(256) void k_display_map(const float *__restrict__ in, long long stream_pitch, long long frame_pitch, int first_row,
                                                            int n_rows, long long n_items, MapGeom g, MapShared sh, const uint32_t *__restrict__ tab,
                                                            unsigned char *__restrict__ out, unsigned long long out_row_pitch,
                                                            unsigned long long out_stream_pitch, ScaleUse su)
{
#pragma clang fp contract(off)
    constexpr int kGroups = 256 / G;
    const int lane = (int)threadIdx.x % G;
    const long long stride = (long long)gridDim.x * kGroups;
    // auto-scale: stream tab[r]'s range from the ring's table; the ranges used go into the slot's trailer (first workgroup).  The range of
    // a row -- a table read and a double division -- is made once per row a workgroup's kGroups consecutive items touch (at most kGroups
    // rows), by its first lanes, and handed to the items through LDS; su is uniform, so are the barriers
    __shared__ float row_y_scale[kGroups];
    __shared__ double row_max_db[kGroups];
    if (su.trailer && blockIdx.x == 0)
        for (uint32_t r = threadIdx.x; r < su.n_trailer; r += 256) scale_write_trailer(su, r, tab[r]);
    for (long long base = (long long)blockIdx.x * kGroups; base < n_items; base += stride) {
        const long long item = base + (int)threadIdx.x / G;
        const long long row0 = base / sh.x_pixels;
        if (su.use) {
            const long long last = base + kGroups - 1 < n_items ? base + kGroups - 1 : n_items - 1;
            const int rows_here = (int)(last / sh.x_pixels - row0) + 1;
            __syncthreads();  // (the previous round's readers)
            if ((int)threadIdx.x < rows_here) {
                MapShared t = sh;
                scale_row_shared(su, tab[(row0 + (int)threadIdx.x) / n_rows], su.fixed_min, &t);
                row_y_scale[threadIdx.x] = t.y_scale;
                row_max_db[threadIdx.x] = t.max_db;
            }
            __syncthreads();
        }
        if (item >= n_items) continue;
        const long long row = item / sh.x_pixels;
        const int32_t i = (int32_t)(item - row * sh.x_pixels);
        const int r = (int)(row / n_rows), j = (int)(row - (long long)r * n_rows);
        const float *x = in + (long long)tab[r] * stream_pitch + (long long)(first_row + j) * frame_pitch;
        MapShared rs = sh;
        if (su.use) {
            rs.y_scale = row_y_scale[row - row0];
            rs.max_db = row_max_db[row - row0];
        }
        const int32_t y = map_y(rs.y_scale, map_power_db<G>(x, g, rs, i, lane), rs.y_pixels);
        if (lane == 0) {
            unsigned char *o = out + (unsigned long long)r * out_stream_pitch + (unsigned long long)j * out_row_pitch;
            if (ARGB) reinterpret_cast<uint32_t *>(o)[i] = waterfall_color(y);
            else reinterpret_cast<int32_t *>(o)[i] = y;
        }
    }
}

// ---- the receiver's display ring (egress.hip): one or two panes per block, per-row geometry from a table on the device ----
// k_display_map carries ONE geometry by value; a zoomed pane needs one per channel, for any number of channels, and run_screen_map's
// answer -- a launch per kMapMaxGeom streams -- would make the ring's launches grow with the bank.  Here the geometry lives in device
// memory, one entry per block row, written at open and at set_pane (call boundaries, like the audio ring's EgressRow table), together
// with the source row (the selection) and the lane group run_screen_map gives THAT row, so the reduction adds in the same order.
struct DisplayRow {
    MapGeom geom;
    uint32_t src;    // the stream / channel of this block row
    int32_t group;   // lanes per pixel, a power of two <= 64
    uint32_t scale_src;  // auto-scale: the stream whose range maps this row (a zoomed row: its channel's stream, 0 off a shared input)
    uint32_t pad_;
};
// one pane of one call, by value
struct DisplayPaneArgs {
    const float *in;                 // [source row][pitch rows][fft_size] float dB
    long long stream_pitch;          // floats between two source rows
    int first_row, n_rows;           // rows first_row .. first_row + n_rows - 1 of each selected source row
    long long total_rows;            // selected rows x n_rows
    const DisplayRow *tab;
    int format;                      // pebblegpu_display_format
    unsigned x_blocks;               // workgroups along x this pane uses (the grid has the larger of the two panes')
    MapShared sh;
    unsigned char *out;              // [selected][n_rows][out_row_pitch bytes]
    unsigned long long out_row_pitch;
    double min_db;                   // the pane's own lower end (auto-scale with one flag: the other end stays the pane's)
};

template <int G>
__device__ inline void display_map_row(const float *__restrict__ x, const MapGeom &g, const MapShared &sh, bool argb, unsigned char *__restrict__ o, unsigned x_blocks)
{
#pragma clang fp contract(off)
    constexpr int kGroups = 256 / G;
    const int lane = (int)threadIdx.x % G;
    for (int32_t i = (int32_t)blockIdx.x * kGroups + (int)threadIdx.x / G; i < sh.x_pixels; i += (int32_t)x_blocks * kGroups) {
        const int32_t y = map_y(sh.y_scale, map_power_db<G>(x, g, sh, i, lane), sh.y_pixels);
        if (lane == 0) {
            if (argb) reinterpret_cast<uint32_t *>(o)[i] = waterfall_color(y);
            else reinterpret_cast<int32_t *>(o)[i] = y;
        }
    }
}

// grid (x, rows, panes): a workgroup takes whole block rows (strided over grid.y), so the row's lane group is uniform in it.  DB_F32 is
// k_display_rows' 16-byte gather (rows are powers of two >= 2048 floats: 16-byte aligned on both sides); the mapped formats run
// map_power_db<G> / map_y / waterfall_color, the one computation of k_screen_map and k_display_map.
// su (auto-scale, ScaleUse): use != 0 takes each mapped row's range from the ring's table, once per row; the workgroup (0, 0, 0) copies
// the ranges used into the slot's trailer (trailer_tab: the table of the pane the trailer speaks for).  DB_F32 panes ignore the range.
static __global__ __launch_bounds__(256) void k_display_panes(DisplayPaneArgs p0, DisplayPaneArgs p1, ScaleUse su, const DisplayRow *__restrict__ trailer_tab)
{
    if (su.trailer && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (uint32_t r = threadIdx.x; r < su.n_trailer; r += 256) scale_write_trailer(su, r, trailer_tab[r].scale_src);
    const DisplayPaneArgs &p = blockIdx.z ? p1 : p0;
    if (blockIdx.x >= p.x_blocks) return;
    for (long long row = blockIdx.y; row < p.total_rows; row += gridDim.y) {
        const int r = (int)(row / p.n_rows), j = (int)(row - (long long)r * p.n_rows);
        const DisplayRow e = p.tab[r];
        const float *x = p.in + (long long)e.src * p.stream_pitch + (long long)(p.first_row + j) * p.sh.fft_size;
        unsigned char *o = p.out + (unsigned long long)row * p.out_row_pitch;
        if (p.format == 0) {  // PEBBLEGPU_DISPLAY_DB_F32
            const float4 *xv = reinterpret_cast<const float4 *>(x);
            float4 *ov = reinterpret_cast<float4 *>(o);
            for (int k = (int)(blockIdx.x * 256 + threadIdx.x); k < p.sh.fft_size / 4; k += (int)p.x_blocks * 256) ov[k] = xv[k];
            continue;
        }
        const bool argb = p.format == 2;  // PEBBLEGPU_DISPLAY_WATERFALL_ARGB32
        MapShared sh = p.sh;
        if (su.use) scale_row_shared(su, e.scale_src, p.min_db, &sh);
        switch (e.group) {
        case 1: display_map_row<1>(x, e.geom, sh, argb, o, p.x_blocks); break;
        case 2: display_map_row<2>(x, e.geom, sh, argb, o, p.x_blocks); break;
        case 4: display_map_row<4>(x, e.geom, sh, argb, o, p.x_blocks); break;
        case 8: display_map_row<8>(x, e.geom, sh, argb, o, p.x_blocks); break;
        case 16: display_map_row<16>(x, e.geom, sh, argb, o, p.x_blocks); break;
        case 32: display_map_row<32>(x, e.geom, sh, argb, o, p.x_blocks); break;
        default: display_map_row<64>(x, e.geom, sh, argb, o, p.x_blocks); break;
        }
    }
}

// up to two panes in one launch on `s` (n_panes 1 or 2; a pane of 0 rows is left out, none left: no launch)
// su / trailer_tab (auto-scale): the ranges' table and where the launch's first workgroup writes the trailer
int run_display_panes(hipStream_t s, const DisplayPaneArgs *panes, int n_panes, const ScaleUse &su = ScaleUse{}, const DisplayRow *trailer_tab = nullptr);

}  // namespace pg
