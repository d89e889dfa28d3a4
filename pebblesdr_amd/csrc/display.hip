// display.hip -- launcher of k_screen_map (FFT::mapFFTToScreen, kernels_display.h) for the receiver, the stream bank and the
// stand-alone spectrum step, and of the stream bank's display-ring packing kernels.
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

// the lane group of a launch whose widest averaged pixel covers bpp bins (0: no averaged pixel)
static int map_lane_group(float bpp)
{
    int G = 1;
    while (G < 64 && (float)(2 * G) <= bpp) G *= 2;
    return G;
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
        const int G = map_lane_group(bpp);
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
                               unsigned long long stream_bytes)
{
    constexpr long long kGroups = 256 / G;
    const long long n_items = (long long)p.n_streams * n_rows * p.sh.x_pixels;
    const dim3 grid((unsigned)std::min<long long>((n_items + kGroups - 1) / kGroups, 1LL << 20));
    if (p.format == PEBBLEGPU_DISPLAY_WATERFALL_ARGB32)
        launch(k_display_map<G, true>, grid, dim3(256), s, in, stream_pitch, (long long)p.sh.fft_size, first_row, n_rows, n_items, p.geom, p.sh, p.d_tab, out,
               (unsigned long long)p.row_pitch_bytes, stream_bytes);
    else
        launch(k_display_map<G, false>, grid, dim3(256), s, in, stream_pitch, (long long)p.sh.fft_size, first_row, n_rows, n_items, p.geom, p.sh, p.d_tab, out,
               (unsigned long long)p.row_pitch_bytes, stream_bytes);
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
        p->geom = map_geom(bins, sample_rate, map->start_freq, map->stop_freq, map->x_pixels);
        p->group = map_lane_group(p->geom.bins_to_plot > map->x_pixels ? p->geom.bins_per_pixel : 0.0f);  // as run_screen_map sizes it
        p->row_elems = (uint32_t)map->x_pixels;
    }
    p->row_pitch_bytes = ((uint64_t)p->row_elems * 4 + 15) & ~(uint64_t)15;
}

int run_display_pack(hipStream_t s, const DisplayPack &p, const float *spec, long long pitch_rows, int first_row, int n_rows, void *dst)
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
        case 1: launch_display_map<1>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes); break;
        case 2: launch_display_map<2>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes); break;
        case 4: launch_display_map<4>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes); break;
        case 8: launch_display_map<8>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes); break;
        case 16: launch_display_map<16>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes); break;
        case 32: launch_display_map<32>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes); break;
        default: launch_display_map<64>(s, p, spec, stream_pitch, first_row, n_rows, out, stream_bytes); break;
        }
    }
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

}  // namespace pg
