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
        const bool averaged = g.bins_to_plot > sh.x_pixels;
        const int32_t bin = map_bin(g, averaged, i);
        int32_t power_db;
        if (bin < 0 || bin >= sh.fft_size) {
            power_db = kMinDb;
        } else {
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
                power_db = x86_trunc(db - sh.max_db);
            } else {
                power_db = x86_trunc((double)x[bin] - sh.max_db);
            }
        }
        if (lane == 0) out[row * sh.x_pixels + i] = map_y(sh.y_scale, power_db, sh.y_pixels);
    }
}

}  // namespace pg
