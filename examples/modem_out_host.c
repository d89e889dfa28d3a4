/* modem_out_host.c -- a host digital-modem "plugin" bound to a bank through the modem hook ring, in plain C through the C ABI
 * (include/pebblegpu.h): the process thread feeds raw int8 samples through the two pinned ingest slots and
 * never waits for the device; a READER THREAD takes the modem blocks -- the rows DigitalModemInterface::processBlock would receive,
 * behind the noise filter and ahead of the AGC -- and runs its "decoder" on them: a zero-crossing counter per channel, which for a
 * channel that hears one tone reads twice the tone's offset from the channel's centre.  A 16-channel USB bank off one 2.048 Msps
 * stream, channel 5 in tune-only mode (dmNONE: the reference returns before the hook, its pairs are absent and the decoder skips
 * them); a tone 1 kHz above channel 3's centre.  No pebblegpu_receiver_synchronize in either loop: the reader waits for ITS slot's
 * copy, and the two threads wait for each other on a host counter (the reader for a queued call, the producer for a free slot, so
 * that nothing is dropped).
 * Exit status 0 on success; otherwise the failing call and pebblegpu_last_error() on stderr.
 * Build: gcc -O2 -Wall -Iinclude examples/modem_out_host.c -Lpebblesdr_amd -lpebblegpu -Wl,-rpath,$PWD/pebblesdr_amd -lm -lpthread */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include "pebblegpu.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, pebblegpu_last_error()); return 1; } } while (0)
#define N_SLOTS 4u  /* covers the run-ahead of three calls */
#define N_CALLS 12
#define N_CH 16u
#define NONE_CH 5u
#define TONE_CH 3u

static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t cv = PTHREAD_COND_INITIALIZER;
static int produced = 0, consumed = 0, failed = 0;  /* calls queued, blocks released, either side gave up */

static uint64_t crossings[N_CH], samples[N_CH], absent[N_CH];
static float last_i[N_CH];
static uint32_t rate = 0;

/* the plugin's processBlock for one present (channel, super-frame): n float I, Q pairs */
static void count_crossings(uint32_t ch, const float *iq, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) {
        const float v = iq[2 * i];
        if ((v >= 0.f) != (last_i[ch] >= 0.f)) crossings[ch]++;
        last_i[ch] = v;
    }
    samples[ch] += n;
}

static int take_block(pebblegpu_receiver *rx, uint64_t expect_call)
{
    pebblegpu_modem_block b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b;
    CHECK(pebblegpu_receiver_modem_out_next(rx, 1, &b));  /* blocks on this slot's copy only */
    if (!b.host || b.call_index != expect_call || b.dropped_before) { fprintf(stderr, "block %llu missing\n", (unsigned long long)expect_call); return 1; }
    rate = b.rate;
    for (uint32_t r = 0; r < b.n_channels; r++) {  /* row r = the r-th selected channel: here all of them, in order */
        const float *row = (const float *)((const char *)b.host + r * b.pitch_bytes);
        for (uint32_t j = 0; j < b.n_superframes; j++) {
            if (!b.present[r * b.n_superframes + j]) { absent[r]++; continue; }  /* the reference never called the hook here */
            count_crossings(r, row + 2 * j * b.samples_per_superframe, b.samples_per_superframe);
        }
    }
    CHECK(pebblegpu_receiver_modem_out_release(rx, b.call_index));
    return 0;
}

static void *reader(void *arg)
{
    pebblegpu_receiver *rx = (pebblegpu_receiver *)arg;
    for (int call = 0; call < N_CALLS; call++) {
        pthread_mutex_lock(&mu);
        while (produced <= call && !failed) pthread_cond_wait(&cv, &mu);  /* (_next reports "nothing queued" instead of waiting for a call) */
        const int stop = failed;
        pthread_mutex_unlock(&mu);
        if (stop) break;
        const int rc = take_block(rx, (uint64_t)call);
        pthread_mutex_lock(&mu);
        if (rc) failed = 1;
        else consumed = call + 1;
        pthread_cond_broadcast(&cv);
        pthread_mutex_unlock(&mu);
        if (rc) break;
    }
    return NULL;
}

static int give_up(void)
{
    pthread_mutex_lock(&mu);
    failed = 1;
    pthread_cond_broadcast(&cv);
    pthread_mutex_unlock(&mu);
    return 1;
}

static int produce(pebblegpu_receiver *rx, const pebblegpu_config *cfg, uint64_t n)
{
    const uint64_t bytes = 2 * n;
    const double two_pi = 6.283185307179586;
    unsigned s = 12345u;
    uint64_t t0 = 0;
    for (int call = 0; call < N_CALLS; call++) {
        pthread_mutex_lock(&mu);
        while (call - consumed >= (int)N_SLOTS && !failed) pthread_cond_wait(&cv, &mu);  /* a free slot for this call's block */
        const int stop = failed;
        pthread_mutex_unlock(&mu);
        if (stop) return 1;
        const uint32_t slot = (uint32_t)(call & 1);
        int8_t *dst = NULL;
        CHECK(pebblegpu_receiver_ingest_acquire(rx, slot, bytes, (void **)&dst));  /* blocks only while the slot's last call runs */
        for (uint64_t i = 0; i < n; i++) {  /* the radio's side: a tone 1 kHz above channel 3's centre over a little noise */
            const double ph = two_pi * fmod((-400e3 + 50e3 * TONE_CH + 1000.0) * (double)(t0 + i) / cfg->sample_rate, 1.0);
            s = s * 1664525u + 1013904223u;
            dst[2 * i] = (int8_t)lrint(40.0 * cos(ph) + (double)((s >> 16) & 3) - 1.5);
            dst[2 * i + 1] = (int8_t)lrint(40.0 * sin(ph) + (double)((s >> 20) & 3) - 1.5);
        }
        t0 += n;
        CHECK(pebblegpu_receiver_ingest_submit(rx, slot, bytes));
        CHECK(pebblegpu_receiver_process_ingested(rx, slot, PEBBLEGPU_IQ_S8, PEBBLEGPU_IQO_IQ, 1.0, n));  /* queues and returns */
        pthread_mutex_lock(&mu);
        produced = call + 1;
        pthread_cond_broadcast(&cv);
        pthread_mutex_unlock(&mu);
    }
    return 0;
}

int main(void)
{
    pebblegpu_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.sample_rate = 2048000.0;
    cfg.frames_per_buffer = 2048;
    cfg.n_channels = N_CH;
    cfg.shared_input = 1;
    cfg.max_superframes = 2;
    pebblegpu_receiver *rx = NULL;
    CHECK(pebblegpu_receiver_create(&cfg, &rx));
    for (uint32_t ch = 0; ch < cfg.n_channels; ch++) {
        CHECK(pebblegpu_set_demod_mode(rx, ch, ch == NONE_CH ? PEBBLEGPU_DM_NONE : PEBBLEGPU_DM_USB));
        CHECK(pebblegpu_set_mixer_freq(rx, ch, -400e3 + 50e3 * ch));
        CHECK(pebblegpu_set_bandpass(rx, ch, 300, 3000));
    }
    pebblegpu_info info;
    CHECK(pebblegpu_receiver_info(rx, &info));
    CHECK(pebblegpu_receiver_modem_out_open(rx, PEBBLEGPU_AUDIO_F32, NULL, 0, N_SLOTS));

    pthread_t th;
    if (pthread_create(&th, NULL, reader, rx)) { fprintf(stderr, "pthread_create failed\n"); return 1; }
    const int rc = produce(rx, &cfg, 2 * info.superframe);
    if (rc) give_up();
    pthread_join(th, NULL);
    if (rc || failed) return 1;

    uint64_t dropped = 0;
    CHECK(pebblegpu_receiver_modem_out_dropped(rx, &dropped));
    CHECK(pebblegpu_receiver_modem_out_close(rx));
    CHECK(pebblegpu_receiver_destroy(rx));
    if (dropped || samples[TONE_CH] == 0) { fprintf(stderr, "%llu blocks dropped, %llu samples\n", (unsigned long long)dropped, (unsigned long long)samples[TONE_CH]); return 1; }
    printf("channel %u: %llu crossings in %llu samples at %u Hz, %llu absent pairs\n", TONE_CH, (unsigned long long)crossings[TONE_CH],
           (unsigned long long)samples[TONE_CH], rate, (unsigned long long)absent[TONE_CH]);
    printf("channel %u: %llu crossings in %llu samples at %u Hz, %llu absent pairs\n", NONE_CH, (unsigned long long)crossings[NONE_CH],
           (unsigned long long)samples[NONE_CH], rate, (unsigned long long)absent[NONE_CH]);
    return 0;
}
