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

struct pebblegpu_screen_map;  // include/pebblegpu.h

namespace pg {

constexpr int kMapMaxGeom = 64;  // per-stream geometries carried in one launch's arguments (zoomed spectra with per-channel offsets)
constexpr int kMinDb = -120;     // DB::minDb (pebblelib/db.cpp)

__host__ __device__ inline int32_t x86_trunc(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : INT32_MIN; }
__host__ __device__ inline int32_t x86_trunc(double d) { return (d > -2147483649.0 && d < 2147483648.0) ? (int32_t)d : INT32_MIN; }

// one (startFreq, stopFreq) against one transform size and rate
struct MapGeom {
    int32_t bin_low, bins_to_plot;
    float pixels_per_bin, bins_per_pixel;
};
struct MapGeoms {
    int n;  // 1: every row uses g[0]; else row stream s (relative to the launch) uses g[s]
    MapGeom g[kMapMaxGeom];
};
struct MapShared {
    int32_t fft_size, x_pixels, y_pixels;
    float y_scale;
    double max_db;
};

inline MapGeom map_geom(int32_t fft_size, double sample_rate, int32_t start_freq, int32_t stop_freq, int32_t x_pixels)
{
#pragma clang fp contract(off)
    const float bins_per_hz = (float)fft_size / (float)sample_rate;
    const int32_t lo = x86_trunc((float)start_freq * bins_per_hz), hi = x86_trunc((float)stop_freq * bins_per_hz);
    MapGeom g;
    g.bin_low = (int32_t)((uint32_t)lo + (uint32_t)(fft_size / 2));
    const int32_t bin_high = (int32_t)((uint32_t)hi + (uint32_t)(fft_size / 2));
    g.bins_to_plot = (int32_t)((uint32_t)bin_high - (uint32_t)g.bin_low);
    g.pixels_per_bin = (float)x_pixels / (float)g.bins_to_plot;
    g.bins_per_pixel = (float)g.bins_to_plot / (float)x_pixels;
    return g;
}

inline float map_y_scale(int32_t y_pixels, double max_db, double min_db)
{
    const double db_range = max_db - min_db;
    return (float)(-y_pixels / db_range);
}

// the bin pixel i reads (fft.cpp:474 / :513)
__host__ __device__ inline int32_t map_bin(const MapGeom &g, bool averaged, int32_t i)
{
#pragma clang fp contract(off)
    const float fi = (float)i;
    float off;
    if (averaged) {
        off = fi * g.bins_per_pixel;
    } else {
#ifdef __HIP_DEVICE_COMPILE__
        off = __fdiv_rn(fi, g.pixels_per_bin);
#else
        off = fi / g.pixels_per_bin;
#endif
    }
    return x86_trunc((float)g.bin_low + off);
}

__host__ __device__ inline int32_t map_y(float y_scale, int32_t power_db, int32_t y_pixels)
{
#pragma clang fp contract(off)
    const int32_t y = x86_trunc(y_scale * (float)power_db - 1.0f);
    return y < 0 ? 0 : (y > y_pixels - 1 ? y_pixels - 1 : y);  // qBound(0, y, yPixels - 1)
}

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
    uint32_t *d_tab = nullptr;       // d_tab[r] = the stream of block row r
    uint32_t row_elems = 0;          // bins (DB_F32) or x_pixels
    uint64_t row_pitch_bytes = 0;    // row_elems * 4 rounded up to 16
    int group = 1;                   // the lane group run_screen_map picks for geom
    MapGeom geom;
    MapShared sh;                    // (DB_F32: fft_size only)
};
// fills everything but n_streams and d_tab from the format and (mapped formats) the checked map
void display_pack_plan(DisplayPack *p, int32_t bins, double sample_rate, const ::pebblegpu_screen_map *map);
// rows first_row .. first_row + n_rows - 1 of spec ([stream][pitch_rows][bins]) -> dst [selected][n_rows][row_pitch_bytes]; one launch
int run_display_pack(hipStream_t s, const DisplayPack &p, const float *spec, long long pitch_rows, int first_row, int n_rows, void *dst);
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
                                                            unsigned long long out_stream_pitch)
{
#pragma clang fp contract(off)
    constexpr int kGroups = 256 / G;
    const int lane = (int)threadIdx.x % G;
    const long long stride = (long long)gridDim.x * kGroups;
    for (long long item = (long long)blockIdx.x * kGroups + (int)threadIdx.x / G; item < n_items; item += stride) {
        const long long row = item / sh.x_pixels;
        const int32_t i = (int32_t)(item - row * sh.x_pixels);
        const int r = (int)(row / n_rows), j = (int)(row - (long long)r * n_rows);
        const float *x = in + (long long)tab[r] * stream_pitch + (long long)(first_row + j) * frame_pitch;
        const int32_t y = map_y(sh.y_scale, map_power_db<G>(x, g, sh, i, lane), sh.y_pixels);
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
    uint32_t pad_[2];
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
static __global__ __launch_bounds__(256) void k_display_panes(DisplayPaneArgs p0, DisplayPaneArgs p1)
{
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
        switch (e.group) {
        case 1: display_map_row<1>(x, e.geom, p.sh, argb, o, p.x_blocks); break;
        case 2: display_map_row<2>(x, e.geom, p.sh, argb, o, p.x_blocks); break;
        case 4: display_map_row<4>(x, e.geom, p.sh, argb, o, p.x_blocks); break;
        case 8: display_map_row<8>(x, e.geom, p.sh, argb, o, p.x_blocks); break;
        case 16: display_map_row<16>(x, e.geom, p.sh, argb, o, p.x_blocks); break;
        case 32: display_map_row<32>(x, e.geom, p.sh, argb, o, p.x_blocks); break;
        default: display_map_row<64>(x, e.geom, p.sh, argb, o, p.x_blocks); break;
        }
    }
}

// the lane group run_screen_map gives each of n_streams rows: per chunk of kMapMaxGeom streams by the chunk's widest averaged pixel
// (per_stream), one for all otherwise.  geoms / groups: n_streams entries each
void map_row_plan(int32_t fft_size, double sample_rate, const int32_t *edges, bool per_stream, int n_streams, int32_t x_pixels, MapGeom *geoms, int *groups);
// up to two panes in one launch on `s` (n_panes 1 or 2; a pane of 0 rows is left out, none left: no launch)
int run_display_panes(hipStream_t s, const DisplayPaneArgs *panes, int n_panes);

}  // namespace pg
