/* multibank_host.c -- a plain-C, one-process, one-thread host that drives a bank sharded across several devices through the C ABI
 * (pebblegpu_multibank_*, include/pebblegpu.h): the call sequence a Qt host makes from its consumer thread.
 * It creates a multibank on the device list given as argv[1] (comma separated; default "0,0": two shards on one device, the rig for a
 * one-GPU machine), tunes every channel through the shards' borrowed receiver handles, pushes a few super-frames of a synthetic int8
 * stream through the two pinned ingest slots, reads one channel's audio from each shard and prints one checksum line per shard.
 * Exit status 0 on success; otherwise the failing call and pebblegpu_last_error() on stderr.
 * Build: gcc -O2 -Wall -Iinclude examples/multibank_host.c -Lpebblesdr_amd -lpebblegpu -Wl,-rpath,$PWD/pebblesdr_amd -lm */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pebblegpu.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, pebblegpu_last_error()); return 1; } } while (0)

int main(int argc, char **argv)
{
    int32_t devices[PEBBLEGPU_MULTIBANK_MAX_SHARDS];
    uint32_t n_shards = 0;
    char list[256];
    strncpy(list, argc > 1 ? argv[1] : "0,0", sizeof list - 1);
    list[sizeof list - 1] = 0;
    for (char *tok = strtok(list, ","); tok && n_shards < PEBBLEGPU_MULTIBANK_MAX_SHARDS; tok = strtok(NULL, ","))
        devices[n_shards++] = (int32_t)atoi(tok);

    pebblegpu_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.sample_rate = 2048000.0;
    cfg.frames_per_buffer = 2048;
    cfg.n_channels = 16 * (n_shards ? n_shards : 1);  /* the total: every shard gets 16 */
    cfg.shared_input = 1;
    cfg.max_superframes = 2;
    pebblegpu_multibank *mb = NULL;
    CHECK(pebblegpu_multibank_create(&cfg, devices, n_shards, 0, &mb));

    /* tuning goes through the shard's receiver handle with the channel's index inside the shard */
    for (uint32_t ch = 0; ch < cfg.n_channels; ch++) {
        uint32_t g, c;
        pebblegpu_receiver *rx = NULL;
        CHECK(pebblegpu_multibank_locate(mb, ch, &g, &c));
        CHECK(pebblegpu_multibank_shard(mb, g, &rx, NULL, NULL, NULL));
        CHECK(pebblegpu_set_demod_mode(rx, c, PEBBLEGPU_DM_USB));
        CHECK(pebblegpu_set_mixer_freq(rx, c, -400e3 + 25e3 * ch));
        CHECK(pebblegpu_set_bandpass(rx, c, 300, 3000));
    }
    pebblegpu_receiver *rx0 = NULL;
    pebblegpu_info info;
    CHECK(pebblegpu_multibank_shard(mb, 0, &rx0, NULL, NULL, NULL));
    CHECK(pebblegpu_receiver_info(rx0, &info));

    /* the radio's side: int8 I,Q pairs (a tone 1 kHz above every channel's centre over a little noise) written straight into the
     * pinned slots, two super-frames per call, the slots in turn */
    const uint64_t n = 2 * info.superframe, bytes = 2 * n;
    const double two_pi = 6.283185307179586;
    unsigned s = 12345u;
    uint64_t t0 = 0;
    for (int call = 0; call < 4; call++) {
        const uint32_t slot = (uint32_t)(call & 1);
        int8_t *dst = NULL;
        CHECK(pebblegpu_multibank_ingest_acquire(mb, slot, bytes, (void **)&dst));  /* blocks only while the slot's last call runs */
        for (uint64_t i = 0; i < n; i++) {
            double re = 0, im = 0;
            for (uint32_t ch = 0; ch < cfg.n_channels; ch += 5) {  /* a few of the channels carry a tone */
                const double ph = two_pi * fmod((-400e3 + 25e3 * ch + 1000.0) * (double)(t0 + i) / cfg.sample_rate, 1.0);
                re += 8.0 * cos(ph);
                im += 8.0 * sin(ph);
            }
            s = s * 1664525u + 1013904223u;
            dst[2 * i] = (int8_t)lrint(re + (double)((s >> 16) & 3) - 1.5);
            dst[2 * i + 1] = (int8_t)lrint(im + (double)((s >> 20) & 3) - 1.5);
        }
        t0 += n;
        CHECK(pebblegpu_multibank_ingest_submit(mb, slot, bytes));  /* one upload per shard */
        CHECK(pebblegpu_multibank_process_ingested(mb, slot, PEBBLEGPU_IQ_S8, PEBBLEGPU_IQO_IQ, 1.0, n));  /* queued on every shard */
    }
    CHECK(pebblegpu_multibank_synchronize(mb));

    /* outputs stay sharded: each shard's audio is on its own device */
    uint32_t shards = 0;
    CHECK(pebblegpu_multibank_shards(mb, &shards));
    for (uint32_t g = 0; g < shards; g++) {
        pebblegpu_receiver *rx = NULL;
        int32_t dev = 0;
        uint32_t first = 0, count = 0;
        uint64_t na = 0, pitch = 0;
        CHECK(pebblegpu_multibank_shard(mb, g, &rx, &dev, &first, &count));
        const void *d_audio = pebblegpu_receiver_audio(rx, &na, &pitch);
        /* the first channel of the shard that carries a tone (global channels 0, 5, 10, ...) */
        const uint32_t ch = (first + 4) / 5 * 5;
        if (!d_audio || na == 0 || ch >= first + count) { fprintf(stderr, "shard %u has no audio\n", g); return 1; }
        float *a = (float *)malloc(sizeof(float) * 2 * (size_t)na);
        if (!a) return 1;
        CHECK(pebblegpu_memcpy_d2h(dev, a, (const char *)d_audio + sizeof(float) * 2 * pitch * (ch - first), sizeof(float) * 2 * (size_t)na));
        double power = 0;
        uint32_t sum = 0;
        for (uint64_t i = 0; i < 2 * na; i++) {
            uint32_t bits;
            memcpy(&bits, &a[i], sizeof bits);
            sum = sum * 31u + bits;
            power += (double)a[i] * a[i];
        }
        free(a);
        if (!(power > 0)) { fprintf(stderr, "shard %u: channel %u is silent\n", g, ch); return 1; }
        printf("shard %u device %d channels %u..%u: channel %u, %llu samples, checksum %08x, power %.6e\n", g, (int)dev, first,
               first + count - 1, ch, (unsigned long long)na, sum, power / (double)na);
    }
    float ms = 0;
    CHECK(pebblegpu_multibank_last_ms(mb, &ms));
    CHECK(pebblegpu_multibank_destroy(mb));
    return 0;
}
