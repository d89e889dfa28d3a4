"""What the two tiers of the modem hook ring (pebblegpu_receiver_modem_out_*) share: the block layout restated, the drivers that run a
tests/tail_cases.py row with the ring open, the references for a gated bank's present pairs, and the C++ program that holds
pebblegpu::feedModemBlock to a block's own samples.

Geometry: tail_cases' own -- one shared stream at 1 024 000 samples/s, D = 16, demodulator rate 64 000, super-frames of 32 768 samples,
2048 demodulator samples each (FRAME 2048: 128 demodulator samples per frame).  Rows of 2048 float2 are 16-byte multiples in both formats,
so the ungated cases add a bank whose selection is odd (5 of 6, 70 of 70) for the trailer's padding, and the host tier walks the layout
through odd row and super-frame counts.

Bars (none of them taken from what the library delivers):
  - ring rows against the MODEM tap, and S16 rows against the host twin of those: exact (np.array_equal) -- the packing kernel copies or
    converts, there is no arithmetic that could justify a tolerance;
  - present pairs of a channel without the noise filter against the oracle's band-passed rows: TOL, the project's bar (1e-5 relative RMS),
    per pair (one super-frame of 2048 samples);
  - present pairs of a noise-filter channel against oracle.Anf over the opened super-frames of a twin bank's band-passed rows (identical
    input): tail_cases.TOL_ANF (1e-6), the figure tail_cases.chan_bar gives a channel behind the noise filter alone."""
import numpy as np

from tests import tail_cases as TC
from tests.test_parity_gpu import TOL

F32, S16, S16_MONO = 0, 1, 2          # PEBBLEGPU_AUDIO_*
BYTES = {F32: 8, S16: 4}              # per sample and row
E_INVALID, E_UNSUPPORTED = -1, -6
DEMOD_FRAME = TC.FRAME // TC.D        # demodulator samples per processBlock call: 128


def layout_ref(fmt, rows, n, k):
    """(pitch_bytes, trailer_offset, trailer_bytes) of a block of `rows` rows of n samples over k super-frames: rows padded to 16 bytes, the
    trailer of rows * k flags right behind them, padded to 16 bytes (include/pebblegpu.h)"""
    pitch = -(-(n * BYTES[fmt]) // 16) * 16
    return pitch, rows * pitch, -(-(rows * k) // 16) * 16


def rel_rms(a, b):
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / np.sqrt(np.mean(np.abs(b) ** 2)))


def as_complex(rows):
    """a block's float rows [rows, n, 2] -> complex64 [rows, n]"""
    return np.ascontiguousarray(rows, dtype=np.float32).view(np.complex64)[..., 0]


def drain(rx, K):
    """K blocks, oldest first, each released once copied: [(call_index, dropped_before, rows, present, rate)]"""
    out = []
    for _ in range(K):
        blk = rx.modem_out_next(True)
        assert blk is not None
        out.append(blk)
        rx.modem_out_release(blk[0])
    return out


# ------------------------------------------------------------------------------------------------
# ungated banks: tones in USB channels, some behind the noise filter
# ------------------------------------------------------------------------------------------------
def usb_centres(C):
    return [(-0.45 + 0.9 * (c + 0.5) / C) * TC.FS for c in range(C)]


def usb_stream(C, n_sf, seed, fs=TC.FS, sf=TC.SF, centres=None):
    """two tones in every channel's pass-band over LCG noise, no two channels or super-frames alike"""
    n = n_sf * sf
    t = np.arange(n) / float(fs)
    x = TC.lcg_noise(n, seed, 1e-4)
    fcs = usb_centres(C) if centres is None else centres
    for c, fc in enumerate(fcs):
        x = x + (0.4 / C) * (np.exp(2j * np.pi * (fc + 700.0 + 13.0 * (c % 37)) * t) + 0.5 * np.exp(2j * np.pi * (fc + 1900.0 - 7.0 * (c % 11)) * t + 0.3j * c))
    return x


def usb_bank(P, C, bins, max_sf, anf=(), fs=TC.FS, centres=None):
    rx = P.ReceiverBank(fs, C, True, False, bins, max_superframes=max_sf)
    fcs = usb_centres(C) if centres is None else centres
    for c in range(C):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000)
        if c in anf:
            rx.set_noise_filter(c, True)
    return rx


def expected_from_tap(P, fmt, tap, sel, none, k):
    """what a block must hold, from the MODEM tap's rows of a twin's call: (rows [len(sel), n, 2], present [len(sel), k]); channels in `none`
    sit the call out in dmNONE: zeros, flags 0"""
    rows, present = [], np.ones((len(sel), k), dtype=np.uint8)
    for r, ch in enumerate(sel):
        row = np.zeros_like(tap[ch]) if ch in none else tap[ch]
        if ch in none:
            present[r, :] = 0
        rows.append(P.modem_out_convert(fmt, row))
    return np.stack(rows), present


# ------------------------------------------------------------------------------------------------
# gated banks: tail_cases' rows `gate` and `gate-thr`, unchanged
# ------------------------------------------------------------------------------------------------
def row_bank(P, row, twin=False, squelch=True):
    """tests/test_narrow_tail_gpu.py::_bank: the row's bank.  twin: the channels behind the noise filter deliver their band-passed rows
    (USB, filter and AGC off)"""
    rx = P.ReceiverBank(TC.FS, len(row.chans), True, False, row.bins, max_superframes=row.max_sf, audio_rate=row.audio_rate)
    assert rx.superframe == TC.SF and int(rx.info.demod_rate_int) == TC.RATE and rx.D == TC.D
    for c, ch in enumerate(row.chans):
        via = twin and ch.anf
        rx.set_mode(c, TC.MODE["USB" if via else ch.modes[0]]); rx.set_mixer(c, ch.fc); rx.set_bandpass(c, *ch.band)
        if not via:
            if ch.agc is not None:
                rx.set_agc(c, *ch.agc)
            if ch.anf:
                rx.set_noise_filter(c, True)
        if ch.squelch is not None and squelch:
            rx.set_squelch(c, ch.squelch)
    return rx


def run_row(rx, row, twin=False, squelch=True, ring=False):
    """the row's calls with its mode changes and setters -> ([call] audio [C, n], [call] ring block or None); the handle stays open"""
    x, audio, blocks = TC.row_input(row.name), [], []
    for k, (s0, ns) in enumerate(TC.call_offsets(row)):
        for c, ch in enumerate(row.chans):
            if k and ch.modes[k] != ch.modes[k - 1] and not (twin and ch.anf):
                rx.set_mode(c, TC.MODE[ch.modes[k]])
            for what, args in TC.actions_before(row, k, c):
                if what == "bandpass":
                    rx.set_bandpass(c, *args)
                elif what == "squelch" and squelch:
                    rx.set_squelch(c, *args)
        audio.append(rx.process(x[s0 * TC.SF:(s0 + ns) * TC.SF])[0])
        if ring:
            blocks += drain(rx, 1)
    return audio, blocks


def anf_reference(O, bp, opened, through_closed=False):
    """oracle.Anf over a channel's band-passed rows bp[call][sf] (never gated), run on the opened super-frames only, its state standing still
    over the closed ones -> [call][sf] arrays (None where closed).  through_closed: the wrong model -- the filter kept running (and adapting)
    through the closed super-frames, as a kernel that ignored the Gate would"""
    f, out = O.Anf(), []
    for call, op in zip(bp, opened):
        res = []
        for y, o in zip(call, op):
            if o:
                res.append(f.process(np.asarray(y, dtype=np.complex128)))
            else:
                if through_closed:
                    f.process(np.asarray(y, dtype=np.complex128))
                res.append(None)
        out.append(res)
    return out


def split_sf(rows_per_call, ch, row):
    """[call] arrays [C, ns * SPF] -> [call][sf] rows of channel ch"""
    return [[a[ch][j * TC.SPF:(j + 1) * TC.SPF] for j in range(ns)] for a, (_, ns) in zip(rows_per_call, TC.call_offsets(row))]


GATE_ROWS = ("gate", "gate-thr")
PAIR_BAR = TOL


# ------------------------------------------------------------------------------------------------
# the C++ feeder, held to the block it is fed (compiled and run by the GPU tier)
# ------------------------------------------------------------------------------------------------
FEEDER_CPP = r"""
// a three-channel bank on tail_cases' geometry: channel 1 behind a threshold no signal reaches (its pairs are absent), channel 2 in dmNONE
// during the second call; every block through pebblegpu::feedModemBlock, whose callbacks must be the present (row, super-frame, frame)
// triples, in order, with the block's own samples
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "pebblegpu_steps.hpp"
#define CHECK(x) do { int rc_ = (x); if (rc_) { std::fprintf(stderr, "%s -> %d: %s\n", #x, rc_, pebblegpu_last_error()); return 1; } } while (0)
int main(int argc, char **argv)
{
    const int format = argc > 1 && !std::strcmp(argv[1], "s16") ? PEBBLEGPU_AUDIO_S16 : PEBBLEGPU_AUDIO_F32;
    pebblegpu_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.sample_rate = 1024000.0;
    cfg.frames_per_buffer = 2048;
    cfg.n_channels = 3;
    cfg.shared_input = 1;
    cfg.spectrum_bins = 4096;
    cfg.max_superframes = 2;
    pebblegpu_receiver *rx = nullptr;
    CHECK(pebblegpu_receiver_create(&cfg, &rx));
    const double fc[3] = {-200e3, 50e3, 300e3};
    for (uint32_t ch = 0; ch < 3; ch++) {
        CHECK(pebblegpu_set_demod_mode(rx, ch, PEBBLEGPU_DM_USB));
        CHECK(pebblegpu_set_mixer_freq(rx, ch, fc[ch]));
        CHECK(pebblegpu_set_bandpass(rx, ch, 300, 3000));
    }
    CHECK(pebblegpu_set_squelch(rx, 1, 50.0));
    pebblegpu_info info;
    CHECK(pebblegpu_receiver_info(rx, &info));
    const uint32_t demodFrames = (uint32_t)(cfg.frames_per_buffer / info.total_decimation);
    CHECK(pebblegpu_receiver_modem_out_open(rx, format, nullptr, 0, 4));
    const uint64_t n = 2 * info.superframe;
    std::vector<float> x(2 * n);
    void *d = nullptr;
    CHECK(pebblegpu_malloc(0, sizeof(float) * x.size(), &d));
    unsigned long long callbacks = 0, expected = 0, mismatches = 0, absent = 0, order = 0;
    for (int call = 0; call < 2; call++) {
        for (uint64_t i = 0; i < n; i++) {
            const double t = (double)(call * n + i) / cfg.sample_rate;
            double re = 0, im = 0;
            for (int ch = 0; ch < 3; ch++) {
                const double ph = 6.283185307179586 * std::fmod((fc[ch] + 900.0 + 200.0 * ch) * t, 1.0);
                re += 0.1 * std::cos(ph);
                im += 0.1 * std::sin(ph);
            }
            x[2 * i] = (float)re;
            x[2 * i + 1] = (float)im;
        }
        if (call == 1) CHECK(pebblegpu_set_demod_mode(rx, 2, PEBBLEGPU_DM_NONE));
        CHECK(pebblegpu_memcpy_h2d(0, d, x.data(), sizeof(float) * x.size()));
        CHECK(pebblegpu_receiver_process(rx, d, n));
        pebblegpu_modem_block b;
        std::memset(&b, 0, sizeof b);
        b.struct_size = sizeof b;
        CHECK(pebblegpu_receiver_modem_out_next(rx, 1, &b));
        if (!b.host || b.n_superframes != 2 || b.n_channels != 3 || b.samples_per_superframe % demodFrames) { std::fprintf(stderr, "unexpected block\n"); return 1; }
        const uint64_t perPair = b.samples_per_superframe / demodFrames;
        std::vector<unsigned long long> seen(3 * 2, 0);
        for (uint32_t r = 0; r < 3; r++)
            for (uint32_t j = 0; j < 2; j++) {
                if (b.present[r * 2 + j]) expected += perPair;
                else absent++;
            }
        long long lastKey = -1;
        callbacks += pebblegpu::feedModemBlock(b, demodFrames, [&](uint32_t r, pebblegpu::CPX *in, uint32_t m) {
            // which frame of row r this is: the frames of a row arrive in stream order, skipping absent super-frames
            uint64_t f = seen[r * 2] + seen[r * 2 + 1];
            uint32_t j = 0;
            uint64_t left = f;
            for (j = 0; j < 2; j++) {
                if (!b.present[r * 2 + j]) continue;
                if (left < perPair) break;
                left -= perPair;
            }
            if (j >= 2 || m != demodFrames) { mismatches++; return; }
            seen[r * 2 + j]++;
            const long long key = ((long long)r * 2 + j) * (long long)perPair + (long long)left;
            if (key <= lastKey) order++;
            lastKey = key;
            const uint64_t at = j * b.samples_per_superframe + left * demodFrames;
            const char *row = (const char *)b.host + r * b.pitch_bytes;
            for (uint32_t i = 0; i < m; i++) {
                double re, im;
                if (b.format == PEBBLEGPU_AUDIO_F32) { const float *p = (const float *)row + 2 * (at + i); re = p[0]; im = p[1]; }
                else { const int16_t *p = (const int16_t *)row + 2 * (at + i); re = p[0] / 32767.0; im = p[1] / 32767.0; }
                if (in[i].real() != re || in[i].imag() != im) mismatches++;
            }
        });
        CHECK(pebblegpu_receiver_modem_out_release(rx, b.call_index));
    }
    CHECK(pebblegpu_receiver_modem_out_close(rx));
    CHECK(pebblegpu_free(0, d));
    CHECK(pebblegpu_receiver_destroy(rx));
    std::printf("callbacks %llu expected %llu absent %llu mismatches %llu order %llu\n", callbacks, expected, absent, mismatches, order);
    return 0;
}
"""
