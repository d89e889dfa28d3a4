// screen_geom.h -- the host-evaluable part of FFT::mapFFTToScreen (pebblelib/fft.cpp:411-534) on the device: the per-call geometry, the
// bin a pixel reads, the y rule, and the lane group run_screen_map gives a launch.  What the reference computes is restated at the top of
// kernels_display.h; the kernels (map_power_db<G> there) and the launchers (display.hip) call these functions, nothing else decides a
// pixel's bin or a launch's lane group.  Plain C++ (no HIP): tests/test_screen_cases_host.py compiles it on the host with
// -ffp-contract=off and holds it, row by row of tests/screen_cases.py, to the table's plain-integer planner.
//
// Float and double expressions are evaluated without contraction (hipcc would fuse a*b+c into an FMA on the device and move the
// truncation boundaries), and every float -> int conversion is x86-64's cvtts*2si: toward zero, INT_MIN for NaN and out of range (C
// leaves those undefined; the host the reference runs on does this).  Int sums that may wrap (binLow + fftSize/2, binHigh - binLow) wrap
// as on x86-64.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>

#if defined(__HIPCC__)
#define PG_SCREEN_GEOM_FN __host__ __device__ inline
#else
#define PG_SCREEN_GEOM_FN inline
#endif
#if defined(__clang__)
#define PG_SCREEN_GEOM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PG_SCREEN_GEOM_NO_CONTRACT  // (g++: -ffp-contract=off on the command line)
#endif

namespace pg {

constexpr int kMapMaxGeom = 64;  // per-stream geometries carried in one launch's arguments (zoomed spectra with per-channel offsets)

PG_SCREEN_GEOM_FN int32_t x86_trunc(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : INT32_MIN; }
PG_SCREEN_GEOM_FN int32_t x86_trunc(double d) { return (d > -2147483649.0 && d < 2147483648.0) ? (int32_t)d : INT32_MIN; }

// one (startFreq, stopFreq) against one transform size and rate
struct MapGeom {
    int32_t bin_low, bins_to_plot;
    float pixels_per_bin, bins_per_pixel;
};
struct MapShared {
    int32_t fft_size, x_pixels, y_pixels;
    float y_scale;
    double max_db;
};

inline MapGeom map_geom(int32_t fft_size, double sample_rate, int32_t start_freq, int32_t stop_freq, int32_t x_pixels)
{
    PG_SCREEN_GEOM_NO_CONTRACT
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

// (a double division, correctly rounded on the device too: the packing kernels of a ring with auto-scale on call it per row and get the host's bits)
PG_SCREEN_GEOM_FN float map_y_scale(int32_t y_pixels, double max_db, double min_db)
{
    PG_SCREEN_GEOM_NO_CONTRACT
    const double db_range = max_db - min_db;
    return (float)(-y_pixels / db_range);
}

// the bin pixel i reads (fft.cpp:474 / :513)
PG_SCREEN_GEOM_FN int32_t map_bin(const MapGeom &g, bool averaged, int32_t i)
{
    PG_SCREEN_GEOM_NO_CONTRACT
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

PG_SCREEN_GEOM_FN int32_t map_y(float y_scale, int32_t power_db, int32_t y_pixels)
{
    PG_SCREEN_GEOM_NO_CONTRACT
    const int32_t y = x86_trunc(y_scale * (float)power_db - 1.0f);
    return y < 0 ? 0 : (y > y_pixels - 1 ? y_pixels - 1 : y);  // qBound(0, y, yPixels - 1)
}

// the lane group of a launch whose widest averaged pixel covers bpp bins (0: no averaged pixel)
inline int map_lane_group(float bpp)
{
    int G = 1;
    while (G < 64 && (float)(2 * G) <= bpp) G *= 2;
    return G;
}

// one chunk of run_screen_map: the geometries of streams s0 .. s0 + ns - 1 into g (per_stream; else the one geometry every stream uses)
// and the lane group of the chunk's launch: the widest averaged pixel sizes it
inline int map_chunk_plan(int32_t fft_size, double sample_rate, const int32_t *edges, bool per_stream, int s0, int ns, int32_t x_pixels, MapGeom *g)
{
    const int n = per_stream ? ns : 1;
    float bpp = 0.0f;
    for (int k = 0; k < n; k++) {
        const int32_t *e = edges + 2 * (per_stream ? s0 + k : 0);
        g[k] = map_geom(fft_size, sample_rate, e[0], e[1], x_pixels);
        if (g[k].bins_to_plot > x_pixels) bpp = std::max(bpp, g[k].bins_per_pixel);
    }
    return map_lane_group(bpp);
}

// the lane group run_screen_map gives each of n_streams rows: per chunk of kMapMaxGeom streams by the chunk's widest averaged pixel
// (per_stream), one for all otherwise.  geoms / groups: n_streams entries each.  What run_screen_map does with each stream's rows, as a
// table: the receiver's display ring packs with it (k_display_panes)
inline void map_row_plan(int32_t fft_size, double sample_rate, const int32_t *edges, bool per_stream, int n_streams, int32_t x_pixels, MapGeom *geoms, int *groups)
{
    const int chunk = per_stream ? kMapMaxGeom : n_streams;
    for (int s0 = 0; s0 < n_streams; s0 += chunk) {
        const int ns = std::min(chunk, n_streams - s0);
        MapGeom g[kMapMaxGeom];
        const int G = map_chunk_plan(fft_size, sample_rate, edges, per_stream, s0, ns, x_pixels, g);
        for (int k = 0; k < ns; k++) {
            geoms[s0 + k] = g[per_stream ? k : 0];
            groups[s0 + k] = G;
        }
    }
}

}  // namespace pg
