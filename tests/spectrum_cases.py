"""The coverage statement for the frame chains of the display transforms (csrc/kernels_spectrum.h): one table of stream-bank shapes,
used by the CPU tier (tests/test_spectrum_chains_host.py: which kernel family and which chain geometry every row reaches, through
spectrum_geometry() of csrc/spectrum_geom.h, and how sensitive the input is to a wrong predecessor) and by the GPU tier
(tests/test_spectrum_chains_gpu.py: the same rows against the oracle, and against a second bank fed another partition into calls).
No row sets an environment switch.

A workgroup walks G consecutive frames of a stream.  Every row is the smallest shape that makes its kernel walk chains of G >= 2
frames under today's thresholds, with the ragged / dead / surplus chain the row is named for.  A row's bank runs three calls:
F frames (chains of G), 5 frames (G = 1: its frame 0 averages with what the ragged last chain of call 1 left), F frames again (chain
0 of a G > 1 launch reads what a G = 1 launch carried).

Input: frame g (numbered from the stream's first, across calls) of stream s is one tone plus LCG noise.  The tone's level is
-6 * ((3 g) mod 5) dB under 0.5 -- 0, -18, -6, -24, -12: at least 12 dB from one frame to the next -- and it sits on a bin of the
frame-length transform that moves by 37 steps per frame and 101 per stream, modulo 251 (prime: coprime to every chain length).  So
frames g, g - 1 and g - 2 have their peaks in three different places, and an average taken with the wrong predecessor (g - 2, g
itself, nothing) is off by 6 dB or more at the peak of g or of g - 1: the CPU tier asserts 1 dB on the oracle for every compared frame.
The phase starts again with every frame, so any frame can be made on its own; the noise is one LCG run per stream, entered anywhere by
jumping the generator ahead.
"""
from collections import namedtuple
import functools

import numpy as np

from tests.signals import lcg_noise, lcg_uniform
from tests.streambank_gate_ref import BankGateTimer

FS = 2_000_000
SHORT = 5            # frames of the short call between the two long ones
A0, SIGMA = 0.5, 1e-2
PERIOD = 251         # of the tone's position, in frames (prime)

# family: the SpecFamily of csrc/spectrum_geom.h the row's kernel belongs to.  kernel: what the bank reports (kernel_name(2)).
# fmt: None float2 input, 0 int8 pairs through process_raw.  ups: the update rate of a gated row (None: every frame).
# G, chains, last_live, surplus: chain length, chains per stream, frames in the last chain and wholly dead chain slots of the LONG calls
# (for a gated row: of the first call's listed frames).  chunk: frames per call of the second bank (G = 1 there).
Row = namedtuple("Row", "name family kernel frame bins S F fmt ups taps chunk G chains last_live surplus why")


def _row(name, family, kernel, frame, bins, S, F, G, chains, last_live, surplus, why, fmt=None, ups=None, taps=0, chunk=64):
    return Row(name, family, kernel, frame, bins, S, F, fmt, ups, taps, chunk, G, chains, last_live, surplus, why)


ROWS = [
    _row("q128-32768", "q128", "k_spectrum_q128", 2048, 32768, 3, 87, 2, 44, 1, 4, "one live frame in the last chain; four surplus chain slots (ZP = 16)"),
    _row("q128-16384", "q128", "k_spectrum_q128", 2048, 16384, 2, 385, 3, 129, 1, 7, "chains of three, the last with one live frame of three"),
    _row("q128-2048", "q128", "k_spectrum_q128", 2048, 2048, 8, 513, 2, 257, 1, 7, "seven surplus chain slots, no zero-padding"),
    _row("waves-4096", "waves", "k_spectrum<2>", 2048, 4096, 8, 515, 2, 258, 1, 0,
         "the last workgroup: one chain of two live frames beside one of a live and a dead frame"),
    _row("t128-float", "t128", "k_spectrum_t128", 2048, 8192, 4, 257, 2, 129, 1, 1,
         "an odd number of chains: the last workgroup's second chain wholly dead, the last live chain one frame"),
    _row("t128-s8", "t128", "k_spectrum_t128 (raw s8)", 2048, 8192, 4, 257, 2, 129, 1, 1, "the same in the converting-loads instance", fmt=0),
    _row("any-1024-8192", "any", "k_spectrum_any", 1024, 8192, 3, 87, 2, 44, 1, 0, "ZP = 8"),
    # (a frame of 3000 samples is no multiple of the band-pass's default block of 1024: 549 taps make it 1500 -- overlap 548, two blocks a
    # frame; the band-pass never runs)
    _row("any-3000-4096", "any", "k_spectrum_any", 3000, 4096, 4, 513, 2, 257, 1, 0, "a frame that is no power of two (M = 4096)", taps=549),
    _row("any-4096-16384", "any", "k_spectrum_any", 4096, 16384, 2, 257, 2, 129, 1, 0, "ZP = 4"),
    _row("big", "big", "k_big256_cols + k_big256_rows", 65536, 65536, 16, 9, 2, 5, 1, 0, "five chains per stream, the last ragged", chunk=2),
    _row("big-listed-s8", "big", "k_big256_cols_list (raw s8) + k_big256_rows", 65536, 65536, 16, 19, 2, 5, 1, 0,
         "several chains of LISTED frames (every second frame at 20 per second)", fmt=0, ups=20, chunk=3),
]


def calls(row):
    return (row.F, SHORT, row.F)


def chain_length(row, k):
    """G of call k (the CPU tier holds it to spectrum_geometry())"""
    return 1 if k == 1 else row.G


def computed_frames(row, split=None):
    """per call (lengths `split`, default the row's three) the frames that get a spectrum, numbered from the stream's first"""
    split = calls(row) if split is None else split
    t = BankGateTimer(row.frame, FS)
    if row.ups is not None:
        t.set_updates(row.ups)
    out, lo = [], 0
    for n in split:
        out.append([lo + i for i in t.call(n)])
        lo += n
    return out


def chunks(row):
    """the second bank's partition of the same frames: calls of row.chunk frames, the last one shorter"""
    total = sum(calls(row))
    return [min(row.chunk, total - lo) for lo in range(0, total, row.chunk)]


def streams(row):
    return sorted({0, row.S - 1, int(lcg_uniform(1, 77 + row.S)[0] * row.S)})


def compared_rows(row, k, n, G):
    """which of call k's n computed rows are compared: 0 and 1, both sides of the first chain boundary, of two boundaries picked by the
    LCG and the last two.  Row 0 of a fresh bank has no predecessor (the reference's buffer is uninitialised there)."""
    want = {0, 1, G - 1, G, G + 1, n - 2, n - 1}
    nch = (n + G - 1) // G
    if nch > 1:
        for u in lcg_uniform(2, 1000 * (k + 1) + n):
            b = 1 + int(u * (nch - 1))
            want |= {b * G - 1, b * G, b * G + 1}
    return sorted(f for f in want if 0 <= f < n and (k or f))


# ---- the input ----
def level_db(g):
    return -6.0 * ((3 * np.asarray(g)) % 5)


def tone_index(row, s, g):
    """the tone of frame g of stream s in bins of the frame-length transform, signed"""
    return (((37 * np.asarray(g) + 101 * s) % PERIOD) - PERIOD // 2) * (row.frame // 256)


def tone_bin(row, s, g):
    """where the oracle puts that tone: bin of the unfolded, zero-padded spectrum (for a frame of 3000 samples: the nearest)"""
    return int(round(row.bins / 2 + tone_index(row, s, g) * row.bins / row.frame))


def lcg_jump(seed, k):
    """the LCG's state after k draws from `seed`: lcg_uniform(n, lcg_jump(seed, k)) == lcg_uniform(k + n, seed)[k:]"""
    m = 1 << 32
    a_k, c_k, a, c = 1, 0, 1664525, 1013904223
    while k:
        if k & 1:
            a_k, c_k = (a * a_k) % m, (a * c_k + c) % m
        a, c = (a * a) % m, (a * c + c) % m
        k >>= 1
    return (a_k * (seed & 0xFFFFFFFF) + c_k) % m


def _seed(row, s):
    return 9000 + 100 * [r.name for r in ROWS].index(row.name) + s


def _frames(row, s, g0, n):
    """frames g0 .. g0 + n - 1 of stream s in double precision"""
    g = np.arange(g0, g0 + n)
    table = np.exp(2j * np.pi * np.arange(row.frame) / row.frame)
    ph = (tone_index(row, s, g)[:, None] * np.arange(row.frame)[None, :]) % row.frame
    x = (A0 * 10.0 ** (level_db(g) / 20.0))[:, None] * table[ph]
    return x.reshape(-1) + lcg_noise(n * row.frame, lcg_jump(_seed(row, s), 2 * g0 * row.frame), SIGMA)


def raw_of(x):
    """HackRF / RTL shape: int8 pairs [..., 2]"""
    return np.stack([np.round(x.real * 127.0), np.round(x.imag * 127.0)], axis=-1).astype(np.int8)


def convert(raw):
    """DeviceInterfaceBase::normalizeIQ at gain 1: component / 128 (exact in fp32)"""
    c = raw.astype(np.float32) * np.float32(1.0 / 128.0)
    return (c[..., 0] + 1j * c[..., 1]).astype(np.complex64)


def frames_input(row, s, g0, n):
    """those frames as the bank's kernels and the oracle see them: complex64, for an int8 row what the device's samples convert to"""
    x = _frames(row, s, g0, n)
    return convert(raw_of(x)) if row.fmt == 0 else x.astype(np.complex64)


def bank_input(row, g0, n):
    """what the bank is fed: [S, n * frame] complex64, or for an int8 row [S, n * frame, 2] int8 -- frames g0 .. g0 + n - 1 of every stream"""
    if row.fmt == 0:
        return np.stack([raw_of(_frames(row, s, g0, n)) for s in range(row.S)])
    return np.stack([frames_input(row, s, g0, n) for s in range(row.S)])


@functools.lru_cache(maxsize=64)
def frame_input(row, s, g):
    x = frames_input(row, s, g, 1)
    x.setflags(write=False)
    return x


def new_oracle(oracle_mod, row):
    return oracle_mod.Spectrum(row.bins, row.frame, lift_clamp=True) if row.frame == 65536 else oracle_mod.Spectrum(row.bins, row.frame)


def oracle_pair(oracle_mod, row, s, pred, g):
    """FFT::fftSpectrum of frame g averaged with frame `pred` (fft.cpp:378-386): the oracle transforms the pair, its first output
    (averaged with the start-up zeros) is discarded"""
    sp = new_oracle(oracle_mod, row)
    sp.process(frame_input(row, s, pred).astype(np.complex128))
    return sp.process(frame_input(row, s, g).astype(np.complex128))
