/* receiver_display_host.c -- a receiver that listens and watches without ever waiting for the device, in plain C through the C ABI
 * (include/pebblegpu.h): one WFM channel at 20 Msps; raw int8 pairs go in through the two pinned ingest
 * slots, PCM16 audio comes out through the audio ring and the two panels of SpectrumWidget::newFftData through the display ring --
 * top: the zoomed spectrum as plot heights, bottom: one waterfall line of the whole band per call as 0xFFRRGGBB.  A reader thread takes
 * both rings' blocks, each time waiting for ONE slot's copy; the producer's loop holds no pebblegpu_receiver_synchronize.  The two
 * threads talk through two counters on the host: the reader asks for block k once call k has been queued, and the producer stays at
 * most N_SLOTS calls ahead of the reader, so nothing is dropped (a host that would rather lose a line than wait leaves that out and
 * reads dropped_before).  Half-way the "user" changes the plot's dB range: pebblegpu_receiver_display_set_pane.
 * With --auto both dB boxes are on "Auto" (the reference's default, SpectrumWidget::recalcScale): pebblegpu_receiver_display_set_auto_scale
 * after the open -- a host flag, no wait -- the range of every block is printed from its trailer (pebblegpu_receiver_display_scale), and
 * half-way the "user" moves the LO instead: pebblegpu_receiver_display_rescale, the next call's first spectrum gives the new range.
 * Exit status 0 on success; otherwise the failing call and pebblegpu_last_error() on stderr.
 * Build: gcc -O2 -Wall -pthread -Iinclude examples/receiver_display_host.c -Lpebblesdr_amd -lpebblegpu -Wl,-rpath,$PWD/pebblesdr_amd -lm */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include "pebblegpu.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, pebblegpu_last_error()); return 1; } } while (0)
#define N_SLOTS 4u
#define N_CALLS 12
#define TOP_X 700
#define BOTTOM_X 1024

static pebblegpu_receiver *rx;
static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t cv = PTHREAD_COND_INITIALIZER;
static int queued = 0;      /* calls the producer has queued (N_CALLS + 1: it gave up) */
static int taken = 0;       /* calls whose blocks the reader has released */
static int reader_rc = 0;
static uint32_t audio_sum = 0, plot_sum = 0, line_sum = 0;
static uint64_t audio_samples = 0, plots = 0, lines = 0;
static int auto_scale = 0;  /* --auto */

static int read_call(uint64_t call)
{
    pebblegpu_audio_block a;
    pebblegpu_display_block d[2];
    memset(&a, 0, sizeof a);
    memset(d, 0, sizeof d);
    a.struct_size = sizeof a;
    d[0].struct_size = d[1].struct_size = sizeof d[0];
    CHECK(pebblegpu_receiver_audio_out_next(rx, 1, &a));          /* blocks on this slot's copy only */
    if (!a.host || a.call_index != call || a.dropped_before) { fprintf(stderr, "audio block %llu missing\n", (unsigned long long)call); return 1; }
    const int16_t *pcm = (const int16_t *)a.host;                 /* the "sound device": a checksum */
    for (uint64_t i = 0; i < a.samples_per_channel; i++) audio_sum = audio_sum * 31u + (uint16_t)pcm[i];
    audio_samples += a.samples_per_channel;
    CHECK(pebblegpu_receiver_audio_out_release(rx, a.call_index));
    CHECK(pebblegpu_receiver_display_next(rx, 1, d));             /* both panes of the same call */
    if (!d[0].host || d[0].call_index != call || d[1].call_index != call || d[0].dropped_before) {
        fprintf(stderr, "display block %llu missing\n", (unsigned long long)call);
        return 1;
    }
    if (d[0].rows_per_stream) {                                   /* the top panel draws the latest zoomed plot */
        const int32_t *y = (const int32_t *)((const char *)d[0].host + (d[0].rows_per_stream - 1) * d[0].row_pitch_bytes);
        for (uint32_t i = 0; i < d[0].row_elems; i++) plot_sum = plot_sum * 31u + (uint32_t)y[i];
        plots++;
    }
    for (uint32_t j = 0; j < d[1].rows_per_stream; j++) {         /* the bottom panel scrolls by one line (max_rows = 1) */
        const uint32_t *line = (const uint32_t *)((const char *)d[1].host + j * d[1].row_pitch_bytes);
        for (uint32_t i = 0; i < d[1].row_elems; i++) line_sum = line_sum * 31u + line[i];
        lines++;
    }
    if (auto_scale) {                                             /* the range this block was mapped with (one channel: one entry) */
        pebblegpu_display_scale sc;
        uint32_t n_sc = 0;
        CHECK(pebblegpu_receiver_display_scale(rx, call, &sc, 1, &n_sc));
        printf("call %llu: %d .. %d dB%s\n", (unsigned long long)call, sc.min_db, sc.max_db, sc.peak_power > 0.0 ? " (recalculated)" : "");
    }
    CHECK(pebblegpu_receiver_display_release(rx, call));
    return 0;
}

static void *reader(void *arg)
{
    (void)arg;
    for (int call = 0; call < N_CALLS; call++) {
        pthread_mutex_lock(&mu);
        while (queued <= call) pthread_cond_wait(&cv, &mu);
        const int stop = queued > N_CALLS;
        pthread_mutex_unlock(&mu);
        if (stop) break;
        const int rc = read_call((uint64_t)call);
        pthread_mutex_lock(&mu);
        if (rc) reader_rc = rc;
        taken = call + 1;
        pthread_cond_broadcast(&cv);
        pthread_mutex_unlock(&mu);
        if (rc) break;
    }
    return NULL;
}

static void plot_geometry(pebblegpu_screen_map *m, int32_t y, int32_t x, double max_db, int32_t start, int32_t stop)
{
    memset(m, 0, sizeof *m);
    m->struct_size = sizeof *m;
    m->y_pixels = y;
    m->x_pixels = x;
    m->max_db = max_db;
    m->min_db = -120.0;
    m->start_freq = start;
    m->stop_freq = stop;
}

int main(int argc, char **argv)
{
    auto_scale = argc > 1 && !strcmp(argv[1], "--auto");
    pebblegpu_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.sample_rate = 20.0e6;
    cfg.frames_per_buffer = 2048;
    cfg.n_channels = 1;
    cfg.shared_input = 1;
    cfg.wfm = 1;
    cfg.spectrum_bins = 8192;
    cfg.hires_bins = 2048;
    cfg.max_superframes = 2;
    CHECK(pebblegpu_receiver_create(&cfg, &rx));
    CHECK(pebblegpu_set_mixer_freq(rx, 0, 1.0e6));
    pebblegpu_info info;
    CHECK(pebblegpu_receiver_info(rx, &info));
    CHECK(pebblegpu_receiver_audio_out_open(rx, PEBBLEGPU_AUDIO_S16_MONO, NULL, 0, N_SLOTS));

    pebblegpu_display_pane pane[2];
    memset(pane, 0, sizeof pane);
    pane[0].struct_size = pane[1].struct_size = sizeof pane[0];
    pane[0].source = PEBBLEGPU_PANE_ZOOM;                         /* top: the zoomed spectrum around the tuned channel, as plot heights */
    pane[0].format = PEBBLEGPU_DISPLAY_PIXELS_I32;
    pane[0].zoom = 0.5;
    plot_geometry(&pane[0].map, 400, TOP_X, 0.0, 0, 0);
    pane[1].source = PEBBLEGPU_PANE_SPECTRUM;                     /* bottom: the whole band's waterfall, the latest line of each call */
    pane[1].format = PEBBLEGPU_DISPLAY_WATERFALL_ARGB32;
    pane[1].max_rows = 1;
    plot_geometry(&pane[1].map, 255, BOTTOM_X, 0.0, -10000000, 10000000);
    CHECK(pebblegpu_receiver_display_open(rx, pane, 2, N_SLOTS));
    if (auto_scale) CHECK(pebblegpu_receiver_display_set_auto_scale(rx, PEBBLEGPU_AUTO_SCALE_MAX | PEBBLEGPU_AUTO_SCALE_MIN));

    pthread_t th;
    if (pthread_create(&th, NULL, reader, NULL)) { fprintf(stderr, "pthread_create failed\n"); return 1; }

    const uint64_t n = 2 * info.superframe, bytes = 2 * n;
    const double two_pi = 6.283185307179586;
    unsigned lcg = 12345u;
    uint64_t t0 = 0;
    int rc = 0;
    for (int call = 0; call < N_CALLS && !rc; call++) {
        pthread_mutex_lock(&mu);                                  /* at most N_SLOTS calls ahead of the reader: host bookkeeping, no device wait */
        while (!reader_rc && call - taken >= (int)N_SLOTS) pthread_cond_wait(&cv, &mu);
        rc = reader_rc;
        pthread_mutex_unlock(&mu);
        if (rc) break;
        if (call == N_CALLS / 2 && auto_scale) {                  /* the user moves the LO: m_scaleNeedsRecalc (a host flag, no wait) */
            CHECK(pebblegpu_receiver_display_rescale(rx));
        } else if (call == N_CALLS / 2) {                         /* the user drags the plot's top down to -20 dB: from this call on */
            plot_geometry(&pane[0].map, 400, TOP_X, -20.0, 0, 0);
            CHECK(pebblegpu_receiver_display_set_pane(rx, 0, &pane[0]));
        }
        const uint32_t slot = (uint32_t)(call & 1);
        int8_t *dst = NULL;
        CHECK(pebblegpu_receiver_ingest_acquire(rx, slot, bytes, (void **)&dst));  /* blocks only while the slot's last call runs */
        for (uint64_t i = 0; i < n; i++) {                        /* the radio's side: an FM carrier at the tuned frequency over a little noise */
            const double t = (double)(t0 + i) / cfg.sample_rate;
            const double ph = two_pi * fmod(1.0e6 * t, 1.0) + 5.0 * sin(two_pi * fmod(1000.0 * t, 1.0));
            lcg = lcg * 1664525u + 1013904223u;
            dst[2 * i] = (int8_t)lrint(40.0 * cos(ph) + (double)((lcg >> 16) & 3) - 1.5);
            dst[2 * i + 1] = (int8_t)lrint(40.0 * sin(ph) + (double)((lcg >> 20) & 3) - 1.5);
        }
        t0 += n;
        CHECK(pebblegpu_receiver_ingest_submit(rx, slot, bytes));
        CHECK(pebblegpu_receiver_process_ingested(rx, slot, PEBBLEGPU_IQ_S8, PEBBLEGPU_IQO_IQ, 1.0, n));  /* queues and returns */
        pthread_mutex_lock(&mu);
        queued = call + 1;                                        /* block `call` of both rings exists from here on */
        pthread_cond_broadcast(&cv);
        pthread_mutex_unlock(&mu);
    }
    pthread_mutex_lock(&mu);
    if (rc) queued = N_CALLS + 1;                                 /* the reader failed and has left, or leaves now */
    pthread_cond_broadcast(&cv);
    pthread_mutex_unlock(&mu);
    pthread_join(th, NULL);
    if (rc || reader_rc) return 1;
    uint64_t d_audio = 0, d_disp = 0;
    CHECK(pebblegpu_receiver_audio_out_dropped(rx, &d_audio));
    CHECK(pebblegpu_receiver_display_dropped(rx, &d_disp));
    CHECK(pebblegpu_receiver_audio_out_close(rx));
    CHECK(pebblegpu_receiver_display_close(rx));
    CHECK(pebblegpu_receiver_destroy(rx));
    if (d_audio || d_disp || !audio_samples || plots != N_CALLS || lines != N_CALLS) {
        fprintf(stderr, "%llu + %llu blocks dropped, %llu samples, %llu plots, %llu lines\n", (unsigned long long)d_audio, (unsigned long long)d_disp,
                (unsigned long long)audio_samples, (unsigned long long)plots, (unsigned long long)lines);
        return 1;
    }
    printf("%llu audio samples (checksum %08x), %llu zoomed plots (checksum %08x), %llu waterfall lines (checksum %08x), none dropped\n",
           (unsigned long long)audio_samples, audio_sum, (unsigned long long)plots, plot_sum, (unsigned long long)lines, line_sum);
    return 0;
}
