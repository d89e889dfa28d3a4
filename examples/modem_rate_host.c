/* modem_rate_host.c -- a host digital-modem "plugin" bound to a bank through the modem hook ring AT A MODEM RATE, in plain C through the
 * C ABI (include/pebblegpu.h).  As examples/modem_out_host.c, but the ring is opened with
 * pebblegpu_receiver_modem_out_open_rate(..., 1000, 8000): every block row has already been through the reference's own Decimator chain
 * for a 1 kHz modem at 8 kHz or more (what Morse::setSampleRate builds and runs at the head of processBlock) on the device, so an eighth
 * of the bytes cross the link and the READER THREAD starts where a modem's detector starts: a tone detector per channel, the power of
 * the row at +1000 Hz and at -1000 Hz (two single-bin transforms over everything the channel delivered).  A 16-channel USB bank off one
 * 2.048 Msps stream (64 kHz rows, 8 kHz blocks), channel 5 in tune-only mode (dmNONE: its pairs are absent and the detector skips them),
 * a tone 1 kHz above channel 3's centre.  No pebblegpu_receiver_synchronize in either loop.
 * Exit status 0 on success; otherwise the failing call and pebblegpu_last_error() on stderr.
 * Build: gcc -O2 -Wall -Iinclude examples/modem_rate_host.c -Lpebblesdr_amd -lpebblegpu -Wl,-rpath,$PWD/pebblesdr_amd -lm -lpthread */
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

static uint64_t samples[N_CH], absent[N_CH];
static double up_re[N_CH], up_im[N_CH], dn_re[N_CH], dn_im[N_CH];  /* sum x e^{-+j 2 pi 1000 t}: the detector's two bins */
static uint32_t rate = 0;

/* the plugin's processBlock for one present (channel, super-frame): n float I, Q pairs at the modem's rate */
static void detect_tone(uint32_t ch, const float *iq, uint64_t n)
{
    const double two_pi = 6.283185307179586;
    for (uint64_t i = 0; i < n; i++) {
        const double ph = two_pi * fmod(1000.0 * (double)(samples[ch] + i) / (double)rate, 1.0), c = cos(ph), s = sin(ph);
        const double re = iq[2 * i], im = iq[2 * i + 1];
        up_re[ch] += re * c + im * s; up_im[ch] += im * c - re * s;
        dn_re[ch] += re * c - im * s; dn_im[ch] += im * c + re * s;
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
            detect_tone(r, row + 2 * j * b.samples_per_superframe, b.samples_per_superframe);
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
    CHECK(pebblegpu_receiver_modem_out_open_rate(rx, PEBBLEGPU_AUDIO_F32, NULL, 0, N_SLOTS, 1000, 8000));

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
    const uint32_t show[2] = {TONE_CH, NONE_CH};
    for (int k = 0; k < 2; k++) {
        const uint32_t ch = show[k];
        const double n = samples[ch] ? (double)samples[ch] : 1.0;
        printf("channel %u: +1000 Hz %.6e -1000 Hz %.6e in %llu samples at %u Hz, %llu absent pairs\n", ch,
               (up_re[ch] * up_re[ch] + up_im[ch] * up_im[ch]) / (n * n), (dn_re[ch] * dn_re[ch] + dn_im[ch] * dn_im[ch]) / (n * n),
               (unsigned long long)samples[ch], rate, (unsigned long long)absent[ch]);
    }
    return 0;
}
