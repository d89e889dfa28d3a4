/* streambank_host.c -- a stream bank run from pinned slots in to pinned slots out, in plain C through the C ABI (include/pebblegpu.h,
 * INTEGRATION.md section 4): raw int8 pairs of 8 streams go in through the two pinned ingest slots; the band-passed IQ of two of the
 * streams (PCM16) and one waterfall line per stream and call (0xFFRRGGBB) come out through the bank's two egress rings.  A reader
 * thread takes the blocks, each time waiting for ONE slot's copy; the producer's loop holds no pebblegpu_streambank_synchronize.  The
 * two threads talk through two counters on the host: the reader asks for block k once call k has been queued (_next returns no
 * block, rather than waiting, while no call has queued one), and the producer stays at most N_SLOTS calls ahead of the reader, so
 * nothing is dropped (a host that would rather lose a line than wait leaves that out and reads dropped_before).
 * The two recorded streams carry a squelch threshold each; the S-meter runs on the device and every IQ block brings, in a trailer inside
 * its one copy, the values and the decision per (stream, frame): the reader prints which streams were open and would skip closed frames.
 * Exit status 0 on success; otherwise the failing call and pebblegpu_last_error() on stderr.
 * Build: gcc -O2 -Wall -pthread -Iinclude examples/streambank_host.c -Lpebblesdr_amd -lpebblegpu -Wl,-rpath,$PWD/pebblesdr_amd -lm */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include "pebblegpu.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, pebblegpu_last_error()); return 1; } } while (0)
#define N_SLOTS 4u
#define N_CALLS 12
#define N_STREAMS 8u
#define FRAME 2048u
#define FRAMES_PER_CALL 4u
#define X_PIXELS 301

static pebblegpu_streambank *sb;
static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t cv = PTHREAD_COND_INITIALIZER;
static int queued = 0;      /* calls the producer has queued (N_CALLS + 1: it gave up) */
static int taken = 0;       /* calls whose two blocks the reader has released */
static int reader_rc = 0;
static uint32_t iq_sum = 0, line_sum = 0;
static uint64_t iq_samples = 0, lines = 0;
static const uint32_t recorded[2] = {5, 2};                  /* row 0 of every IQ block is stream 5, row 1 stream 2 */

static int read_call(uint64_t call)
{
    pebblegpu_audio_block a;
    pebblegpu_display_block d;
    memset(&a, 0, sizeof a);
    memset(&d, 0, sizeof d);
    a.struct_size = sizeof a;
    d.struct_size = sizeof d;
    CHECK(pebblegpu_streambank_iq_out_next(sb, 1, &a));      /* blocks on this slot's copy only */
    if (!a.host || a.call_index != call || a.dropped_before) { fprintf(stderr, "IQ block %llu missing\n", (unsigned long long)call); return 1; }
    for (uint32_t r = 0; r < a.n_channels; r++) {            /* the "recorder": a checksum over every selected stream's pairs */
        const int16_t *row = (const int16_t *)((const char *)a.host + r * a.pitch_bytes);
        for (uint64_t i = 0; i < 2 * a.samples_per_channel; i++) iq_sum = iq_sum * 31u + (uint16_t)row[i];
    }
    iq_samples += a.samples_per_channel;
    pebblegpu_stream_gate gate[2 * FRAMES_PER_CALL];         /* entry r * frames + j: selected stream r, frame j of the call */
    uint32_t frames = 0;
    CHECK(pebblegpu_streambank_iq_out_gate(sb, a.call_index, gate, 2 * FRAMES_PER_CALL, &frames));
    printf("block %llu:", (unsigned long long)call);
    for (uint32_t r = 0; r < a.n_channels && frames; r++) {
        uint32_t open = 0;
        for (uint32_t j = 0; j < frames; j++) open += gate[r * frames + j].open;
        printf("  stream %u open in %u of %u frames (avg %.1f dB, snr %.1f dB)", recorded[r], open, frames, gate[r * frames + frames - 1].avg_db,
               gate[r * frames + frames - 1].snr_db);
    }
    printf("\n");
    CHECK(pebblegpu_streambank_iq_out_release(sb, a.call_index));
    CHECK(pebblegpu_streambank_display_next(sb, 1, &d));
    if (!d.host || d.call_index != call || d.dropped_before) { fprintf(stderr, "display block %llu missing\n", (unsigned long long)call); return 1; }
    for (uint32_t r = 0; r < d.n_streams; r++)               /* the "waterfall": one new line per stream (max_rows = 1) */
        for (uint32_t j = 0; j < d.rows_per_stream; j++) {
            const uint32_t *line = (const uint32_t *)((const char *)d.host + r * d.stream_pitch_bytes + j * d.row_pitch_bytes);
            for (uint32_t i = 0; i < d.row_elems; i++) line_sum = line_sum * 31u + line[i];
            lines++;
        }
    CHECK(pebblegpu_streambank_display_release(sb, d.call_index));
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

int main(void)
{
    pebblegpu_streambank_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.sample_rate = 2.0e6;
    cfg.n_streams = N_STREAMS;
    cfg.frame = FRAME;
    cfg.spectrum_bins = 4096;
    cfg.max_frames = FRAMES_PER_CALL;
    CHECK(pebblegpu_streambank_create(&cfg, &sb));
    for (uint32_t s = 0; s < N_STREAMS; s++) CHECK(pebblegpu_streambank_set_bandpass(sb, s, -60e3, 60e3));
    /* real front ends: DCRemoval and the first noise blanker ahead of both transforms, on every stream (a host flag, no wait) */
    for (uint32_t s = 0; s < N_STREAMS; s++) CHECK(pebblegpu_streambank_set_conditioners(sb, s, PEBBLEGPU_COND_DC | PEBBLEGPU_COND_NB1, 1.0, 0.0));

    CHECK(pebblegpu_streambank_set_squelch(sb, 5, -20.0));   /* above what the tone averages over the pass band: closed, zeros in the block */
    CHECK(pebblegpu_streambank_set_squelch(sb, 2, -60.0));   /* (a threshold above -120 turns the S-meter on) */
    CHECK(pebblegpu_streambank_iq_out_open(sb, PEBBLEGPU_AUDIO_S16, recorded, 2, N_SLOTS));
    pebblegpu_screen_map map;
    memset(&map, 0, sizeof map);
    map.struct_size = sizeof map;
    map.y_pixels = 255;                                      /* the waterfall's palette is indexed by a 255-pixel plot */
    map.x_pixels = X_PIXELS;
    map.max_db = 0.0;
    map.min_db = -120.0;
    map.start_freq = -1000000;
    map.stop_freq = 1000000;
    CHECK(pebblegpu_streambank_display_open(sb, PEBBLEGPU_DISPLAY_WATERFALL_ARGB32, &map, NULL, 0, 1, N_SLOTS));

    pthread_t th;
    if (pthread_create(&th, NULL, reader, NULL)) { fprintf(stderr, "pthread_create failed\n"); return 1; }

    const uint64_t n = (uint64_t)FRAME * FRAMES_PER_CALL, bytes = 2 * n * N_STREAMS;
    const double two_pi = 6.283185307179586;
    unsigned lcg = 12345u;
    uint64_t t0 = 0;
    int rc = 0;
    for (int call = 0; call < N_CALLS && !rc; call++) {
        pthread_mutex_lock(&mu);                             /* at most N_SLOTS calls ahead of the reader: host bookkeeping, no device wait */
        while (!reader_rc && call - taken >= (int)N_SLOTS) pthread_cond_wait(&cv, &mu);
        rc = reader_rc;
        pthread_mutex_unlock(&mu);
        if (rc) break;
        const uint32_t slot = (uint32_t)(call & 1);
        int8_t *dst = NULL;
        CHECK(pebblegpu_streambank_ingest_acquire(sb, slot, bytes, (void **)&dst));  /* blocks only while the slot's last call runs */
        for (uint32_t s = 0; s < N_STREAMS; s++)             /* the radios' side: a tone per stream, inside its pass band, over noise */
            for (uint64_t i = 0; i < n; i++) {
                const double ph = two_pi * fmod((5e3 + 6e3 * s) * (double)(t0 + i) / cfg.sample_rate, 1.0);
                lcg = lcg * 1664525u + 1013904223u;
                dst[2 * (s * n + i)] = (int8_t)lrint(40.0 * cos(ph) + (double)((lcg >> 16) & 3) - 1.5);
                dst[2 * (s * n + i) + 1] = (int8_t)lrint(40.0 * sin(ph) + (double)((lcg >> 20) & 3) - 1.5);
            }
        t0 += n;
        CHECK(pebblegpu_streambank_ingest_submit(sb, slot, bytes));
        CHECK(pebblegpu_streambank_process_ingested(sb, slot, PEBBLEGPU_IQ_S8, PEBBLEGPU_IQO_IQ, 1.0, n, 3));  /* queues and returns */
        pthread_mutex_lock(&mu);
        queued = call + 1;                                   /* block `call` of both rings exists from here on */
        pthread_cond_broadcast(&cv);
        pthread_mutex_unlock(&mu);
    }
    pthread_mutex_lock(&mu);
    if (rc) queued = N_CALLS + 1;                            /* the reader failed and has left, or leaves now */
    pthread_cond_broadcast(&cv);
    pthread_mutex_unlock(&mu);
    pthread_join(th, NULL);
    if (rc || reader_rc) return 1;
    uint64_t d_iq = 0, d_disp = 0;
    CHECK(pebblegpu_streambank_iq_out_dropped(sb, &d_iq));
    CHECK(pebblegpu_streambank_display_dropped(sb, &d_disp));
    CHECK(pebblegpu_streambank_iq_out_close(sb));
    CHECK(pebblegpu_streambank_display_close(sb));
    CHECK(pebblegpu_streambank_destroy(sb));
    if (d_iq || d_disp || iq_samples != n * N_CALLS || lines != (uint64_t)N_STREAMS * N_CALLS) {
        fprintf(stderr, "%llu + %llu blocks dropped, %llu samples, %llu lines\n", (unsigned long long)d_iq, (unsigned long long)d_disp,
                (unsigned long long)iq_samples, (unsigned long long)lines);
        return 1;
    }
    printf("%llu recorded samples per stream (checksum %08x), %llu waterfall lines (checksum %08x), none dropped\n", (unsigned long long)iq_samples,
           iq_sum, (unsigned long long)lines, line_sum);
    return 0;
}
