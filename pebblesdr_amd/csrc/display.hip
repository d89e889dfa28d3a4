// display.hip -- launcher of k_screen_map (FFT::mapFFTToScreen, kernels_display.h) for the receiver, the stream bank and the
// stand-alone spectrum step.
#include <algorithm>
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
        float bpp = 0.0f;  // the widest pixel of the launch sizes its lane groups
        for (int k = 0; k < geoms.n; k++) {
            const int32_t *e = edges + 2 * (per_stream ? s0 + k : 0);
            geoms.g[k] = map_geom(fft_size, sample_rate, e[0], e[1], x_pixels);
            if (geoms.g[k].bins_to_plot > x_pixels) bpp = std::max(bpp, geoms.g[k].bins_per_pixel);
        }
        int G = 1;
        while (G < 64 && (float)(2 * G) <= bpp) G *= 2;
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

}  // namespace pg
