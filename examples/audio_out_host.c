/* audio_out_host.c -- the steady state of a host-to-host loop in plain C through the C ABI (include/pebblegpu.h, INTEGRATION.md
 * section 10): raw int8 samples go in through the two pinned ingest slots, PCM16 audio comes out through the pinned audio blocks, and
 * nothing in the loop waits for the device -- the host reads the block of the call N_SLOTS - 1 calls back, whose copy has long
 * completed, while the newer calls are still queued or running.  A 16-channel SSB bank off one 2.048 Msps stream; the "sound
 * device" here is a checksum over channel 3's samples.
 * Exit status 0 on success; otherwise the failing call and pebblegpu_last_error() on stderr.
 * Build: gcc -O2 -Wall -Iinclude examples/audio_out_host.c -Lpebblesdr_amd -lpebblegpu -Wl,-rpath,$PWD/pebblesdr_amd -lm */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "pebblegpu.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, pebblegpu_last_error()); return 1; } } while (0)
#define N_SLOTS 4u  /* covers the run-ahead of three calls */
#define N_CALLS 12

static uint32_t sum = 0;
static uint64_t total = 0;

/* the consumer: takes the oldest block (blocking on ITS copy only), "plays" one row, gives the slot back */
static int take_block(pebblegpu_receiver *rx, uint64_t expect_call)
{
    pebblegpu_audio_block b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b;
    CHECK(pebblegpu_receiver_audio_out_next(rx, 1, &b));
    if (!b.host || b.call_index != expect_call || b.dropped_before) { fprintf(stderr, "block %llu missing\n", (unsigned long long)expect_call); return 1; }
    const int16_t *row = (const int16_t *)((const char *)b.host + 3 * b.pitch_bytes);  /* row r = the r-th selected channel */
    for (uint64_t i = 0; i < b.samples_per_channel; i++) sum = sum * 31u + (uint16_t)row[i];
    total += b.samples_per_channel;
    CHECK(pebblegpu_receiver_audio_out_release(rx, b.call_index));
    return 0;
}

int main(void)
{
    pebblegpu_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.sample_rate = 2048000.0;
    cfg.frames_per_buffer = 2048;
    cfg.n_channels = 16;
    cfg.shared_input = 1;
    cfg.max_superframes = 2;
    pebblegpu_receiver *rx = NULL;
    CHECK(pebblegpu_receiver_create(&cfg, &rx));
    for (uint32_t ch = 0; ch < cfg.n_channels; ch++) {
        CHECK(pebblegpu_set_demod_mode(rx, ch, PEBBLEGPU_DM_USB));
        CHECK(pebblegpu_set_mixer_freq(rx, ch, -400e3 + 50e3 * ch));
        CHECK(pebblegpu_set_bandpass(rx, ch, 300, 3000));
        CHECK(pebblegpu_set_audio_level(rx, ch, 80.f, 0));  /* the volume slider */
    }
    pebblegpu_info info;
    CHECK(pebblegpu_receiver_info(rx, &info));
    CHECK(pebblegpu_receiver_audio_out_open(rx, PEBBLEGPU_AUDIO_S16_MONO, NULL, 0, N_SLOTS));

    const uint64_t n = 2 * info.superframe, bytes = 2 * n;
    const double two_pi = 6.283185307179586;
    unsigned s = 12345u;
    uint64_t t0 = 0;
    for (int call = 0; call < N_CALLS; call++) {
        const uint32_t slot = (uint32_t)(call & 1);
        int8_t *dst = NULL;
        CHECK(pebblegpu_receiver_ingest_acquire(rx, slot, bytes, (void **)&dst));  /* blocks only while the slot's last call runs */
        for (uint64_t i = 0; i < n; i++) {  /* the radio's side: a tone 1 kHz above channel 3's centre over a little noise */
            const double ph = two_pi * fmod((-400e3 + 50e3 * 3 + 1000.0) * (double)(t0 + i) / cfg.sample_rate, 1.0);
            s = s * 1664525u + 1013904223u;
            dst[2 * i] = (int8_t)lrint(40.0 * cos(ph) + (double)((s >> 16) & 3) - 1.5);
            dst[2 * i + 1] = (int8_t)lrint(40.0 * sin(ph) + (double)((s >> 20) & 3) - 1.5);
        }
        t0 += n;
        CHECK(pebblegpu_receiver_ingest_submit(rx, slot, bytes));
        CHECK(pebblegpu_receiver_process_ingested(rx, slot, PEBBLEGPU_IQ_S8, PEBBLEGPU_IQO_IQ, 1.0, n));  /* queues and returns */
        /* lagging by N_SLOTS - 1: the block taken here belongs to a call the device finished while the host was filling slots */
        if (call >= (int)N_SLOTS - 1 && take_block(rx, (uint64_t)(call - ((int)N_SLOTS - 1)))) return 1;
    }
    for (int call = N_CALLS - ((int)N_SLOTS - 1); call < N_CALLS; call++)  /* the end of the stream: drain what is still queued */
        if (take_block(rx, (uint64_t)call)) return 1;
    uint64_t dropped = 0;
    CHECK(pebblegpu_receiver_audio_out_dropped(rx, &dropped));
    CHECK(pebblegpu_receiver_audio_out_close(rx));
    CHECK(pebblegpu_receiver_destroy(rx));
    if (dropped || total == 0) { fprintf(stderr, "%llu blocks dropped, %llu samples\n", (unsigned long long)dropped, (unsigned long long)total); return 1; }
    printf("channel 3: %llu samples in %d blocks, checksum %08x, none dropped\n", (unsigned long long)total, N_CALLS, sum);
    return 0;
}
