"""The coverage statement for the geometry of the modem ring at a modem rate (k_modem_rate_pack, csrc/egress.hip; the tile rule
modem_rate_geometry, csrc/modem_rate_geom.h): one table of rows, their streams and seeds, a plain fp64 model of the kernel's algorithm and
its six deliberately wrong variants, shared by the CPU tier (tests/test_modem_geom_host.py) and the GPU tier
(tests/test_modem_geom_gpu.py).  Nothing is stored: every row is a recipe.

tests/modem_rate_cases.py runs on one geometry (super-frames of 2048 demodulator samples, D = 4 or 8, H <= 142): there every launch
has tile 256, m = spf / D a multiple of the tile, a span that is nearly all its own samples, at most three stages and 16-byte stores.
The rows here are the launches that geometry never makes.  The columns of ROWS (nf: frames_per_buffer; the band-pass as fft / taps,
its block L = fft - taps + 1; spf = lcm(nf, L) demodulator samples per super-frame; m = spf / D; ragged = m % tile) are asserted by
the CPU tier against pebblegpu_modem_rate_plan, oracle.Decimator(...).chain() and the compiled header, none is taken on trust:

  d4-l1792         ragged last tile (192 of 256)
  d8-ragged        ragged last tile (128 of 256)
  d16-t64          the tile halved by out_spf (64 outputs per super-frame: one tile of 64)
  d32-ragged       the tile halved by the LDS span (64 * 32 + 10 <= 4096 < 128 * 32 + 10), ragged (32 of 64)
  d64-one-tile     one tile per super-frame (16), H = 586 over half of the tile's own 1024 samples
  d64-four         four stages; tile 32, ragged (16); the last tile's own samples (16 * 64 = 1024) are fewer than H = 1498, so the carry's
                   H samples begin in the look-back
  d128             tile 8: every tile's span is mostly look-back (8 * 128 = 1024 own samples, H = 2250), p0 < 0 in all three tiles
  d128-l1792       the same, ragged (4 of 8)
  d128-s16-scalar  the same with m = 42: m % 4 == 2, the S16 instance stores sample by sample (and zeroes absent pairs so), F32 by pairs
  d64-48k          a 48 kHz receiver without a decimator (behind k_fastfir_t128_mix): the 59-tap stage last, tile 16, tile * D < H = 2330

Every row but the last is a bank at 1 024 000 samples/s (front decimation 16, demodulator rate 64 000) of three to five channels in USB
with a band-pass of (-1000, 2000) Hz -- the hook sits in front of the demodulator, the mode only names the branch -- and a permuted
subset selected; calls of 1, 3, 2 and max_superframes = 3 super-frames.  No receiver refused a row's (nf, band-pass): none was replaced.

THE SIGNAL.  A decimation by 128 that protects 200 Hz leaves nothing of a voice channel, and a relative bar on a near-silent pair
measures nothing: every channel hears a carrier within +-60 Hz of its centre (OFFSETS) at 0.4 / C over LCG noise of 1e-4, and both
tiers assert that the oracle's output RMS of every compared pair is at least MIN_GAIN = 0.05 of the pair's input RMS.

THE SCALAR PATHS, which of the four can be reached and why (read from the code, the CPU tier pins the arithmetic facts):
  - The source row is always 16-byte aligned: Receiver::audio is HistBuf::alloc(C, 0, nd_max) (csrc/cores.hip), hist = 0 and pitch =
    (capacity + 1) & ~1 -- even -- on a hipMalloc'ed base, so iq + channel * pitch is a multiple of 16 bytes for every channel.  A
    misaligned `src` is the kernels' guard for a caller that does not exist.
  - k_modem_rate_pack, vec_in == false: NOT reachable.  It needs one of spf, p0, H, n0 odd.  Every stage has an odd tap count (the design
    table has no even one; the CIC3 is refused), so H = sum (T_j - 1) * scale_j is even; a non-empty chain has D even and the plan refuses
    spf % D != 0, so spf is even; p0 = o0 * D - H and n0 = tn * D + H are even with them.
  - k_modem_rate_pack, the S16 sample-by-sample store (m % 4 != 0): row d128-s16-scalar, in its present and its absent pairs.
  - k_modem_rate_pack, the F32 sample-by-sample store (m odd), and both scalar loops of k_modem_pack (spf % 2 != 0 for F32, spf % 4 != 0
    for S16): NOT reachable with the three band-pass sizes the project builds hosts and tests for (2048 / 1025, 4096 / 2049, 2048 / 257:
    L = 1024, 2048, 1792, all multiples of 256).  spf = lcm(nf, L) is then a multiple of 256, so spf % 4 == 0 for the plain ring; and
    wherever the plan accepts a chain at a receiver's rate D <= 128 (the CPU tier sweeps this), so m = spf / D is even.  pebblegpu_
    receiver_create also accepts an even tap count (taps in [2, fft / 2 + 1]), whose block L is odd: such a band-pass is outside what this
    table covers, and no row is invented for it.

Bars: the device against oracle.Decimator fed the twin's present pairs: modem_out_cases.PAIR_BAR (1e-5 relative RMS per pair); the
model against the oracle: MODEL_BAR = 1e-12 (fp64 sums of at most 59 products in another order); S16 rows against the host twin of the
F32 ring's rows: exact."""
from collections import namedtuple
import functools
import math

import numpy as np

from tests import decim_cases as DC
from tests import tail_cases as TC
from tests.signals import lcg_noise

E_INVALID, E_SIZE, E_UNSUPPORTED = -1, -5, -6
MODEL_BAR = 1e-12
MIN_GAIN = 0.05
CALLS, RECUT, MAX_SF = (1, 3, 2, 3), (3, 1, 3, 2), 3
BAND = (-1000.0, 2000.0)
OFFSETS = (-55.0, 35.0, -20.0, 50.0, 10.0)      # the carrier of channel c, in Hz from its centre
RECEIVER_RATES = (64000, 62500, 48828, 48000, 39062, 37500)   # demodulator rates Receiver's (fs, 30000, 0) chain gives
BLOCKS = (1024, 2048, 1792)                     # L of the three band-pass sizes

# name; (max_bw, min_rate); fs; nf, fft, taps; spf; chain; D; H; m; tile; ragged (m % tile); channels, selection; seed
Row = namedtuple("Row", "name bw mn fs nf fft taps spf chain D H m tile ragged C sel seed")
_D128 = [(11, 32), (19, 2), (27, 2)]
ROWS = {r.name: r for r in (
    Row("d4-l1792", 200, 16000, 1024000, 256, 2048, 257, 1792, [(11, 4)], 4, 10, 448, 256, 192, 5, [3, 0, 4, 1], 61),
    Row("d8-ragged", 200, 8000, 1024000, 1536, 2048, 1025, 3072, [(11, 8)], 8, 10, 384, 256, 128, 4, [2, 0, 3], 62),
    Row("d16-t64", 200, 4000, 1024000, 512, 2048, 1025, 1024, [(11, 16)], 16, 10, 64, 64, 0, 3, [2, 0], 63),
    Row("d32-ragged", 200, 2000, 1024000, 1536, 2048, 1025, 3072, [(11, 32)], 32, 10, 96, 64, 32, 5, [4, 1, 0, 2], 64),
    Row("d64-one-tile", 200, 1000, 1024000, 512, 2048, 1025, 1024, [(11, 32), (19, 2)], 64, 586, 16, 16, 0, 4, [1, 3, 0], 65),
    Row("d64-four", 500, 125, 1024000, 1536, 2048, 1025, 3072, [(11, 8), (15, 2), (19, 2), (35, 2)], 64, 1498, 48, 32, 16, 5, [3, 0, 4, 1], 66),
    Row("d128", 200, 500, 1024000, 1536, 2048, 1025, 3072, _D128, 128, 2250, 24, 8, 0, 4, [2, 0, 3], 67),
    Row("d128-l1792", 200, 500, 1024000, 512, 2048, 257, 3584, _D128, 128, 2250, 28, 8, 4, 3, [2, 0], 68),
    Row("d128-s16-scalar", 200, 500, 1024000, 768, 2048, 257, 5376, _D128, 128, 2250, 42, 8, 2, 5, [4, 1, 0, 2], 69),
    Row("d64-48k", 500, 125, 48000, 1536, 2048, 1025, 3072, [(11, 8), (15, 2), (23, 2), (59, 2)], 64, 2330, 48, 16, 0, 3, [2, 0], 70),
)}
STATE_ROWS = ("d64-four", "d128", "d128-s16-scalar")
# the chain a state row's ring is reopened with, mid-stream, on another selection: (max_bw, min_rate), selection
REOPEN = {"d64-four": ((200, 2000), [1, 2]), "d128": ((500, 125), [3, 1]), "d128-s16-scalar": ((200, 8000), [0, 3, 2])}

# refusals at a receiver rate: (demodulator rate, spf, max_bw, min_rate, code, a word of the message)
REFUSALS = (
    (64000, 3072, 300, 500, E_SIZE, "3626"),         # the look-back of 3626 samples exceeds the super-frame
    (64000, 1024, 200, 500, E_SIZE, "27-tap"),       # H = 2250 exceeds 1024 as well, but the 27-tap stage's 16 inputs are refused first
    (37500, 5376, 200, 500, E_UNSUPPORTED, "LDS"),   # every stage is fed and H fits, but the smallest tile's span exceeds the LDS buffer
)


def demod_rate(row):
    return 64000 if row.fs == 1024000 else row.fs


def front(row):
    """the receiver's own decimation in front of the band-pass"""
    return row.fs // demod_rate(row)


def lookback(chain):
    h, scale = 0, 1
    for taps, stride in chain:
        h += (taps - 1) * scale
        scale *= stride
    return h


def tile_rule(D, H, out_spf, taps0, stride0):
    """modem_rate_geometry restated -> (tile, lds_a, lds_b) or None"""
    tile = 256
    while tile > 4 and tile // 2 >= out_spf:
        tile //= 2
    while tile > 4 and tile * D + H > 4096:
        tile //= 2
    a = (tile * D + H + 1) & ~1
    if a > 4096:
        return None
    return tile, a, ((a - taps0) // stride0 + 2) & ~1


def centres(row):
    if row.fs == 48000:
        return [-9000.0, 0.0, 9000.0]
    return [(-0.45 + 0.9 * (c + 0.5) / row.C) * row.fs for c in range(row.C)]


def wide_stream(row, n_sf):
    """the bank's input: a carrier OFFSETS[c] from every channel's centre over LCG noise"""
    n = n_sf * row.spf * front(row)
    t = np.arange(n) / float(row.fs)
    x = lcg_noise(n, row.seed, 1e-4)
    for c, fc in enumerate(centres(row)):
        x = x + (0.4 / row.C) * np.exp(1j * (2 * np.pi * (fc + OFFSETS[c]) * t + 0.3 * c))
    return x


def bank(P, row, max_sf=MAX_SF, bins=0):
    rx = P.ReceiverBank(row.fs, row.C, True, False, bins, frames_per_buffer=row.nf, fastfir_fft=row.fft, fastfir_taps=row.taps, max_superframes=max_sf)
    for c, fc in enumerate(centres(row)):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fc); rx.set_bandpass(c, *BAND)
    return rx


@functools.lru_cache(maxsize=None)
def host_stream(name, ch):
    """what the CPU tier feeds the model and the oracle for channel ch of a row, at the demodulator rate: the same carrier over LCG noise,
    one array of sum(CALLS) super-frames (no two super-frames alike: an absent pair's samples are not the present ones')"""
    row = ROWS[name]
    n = sum(CALLS) * row.spf
    t = np.arange(n) / float(demod_rate(row))
    x = (0.4 / row.C) * np.exp(1j * (2 * np.pi * OFFSETS[ch] * t + 0.3 * ch)) + lcg_noise(n, 100 * row.seed + ch, 1e-4)
    x.setflags(write=False)
    return x


# presence patterns over CALLS: [call][super-frame]
PATTERNS = {
    "all": [[1], [1, 1, 1], [1, 1], [1, 1, 1]],
    "gap": [[1], [1, 0, 1], [1, 1], [0, 1, 1]],          # present-absent-present inside a call; a call that starts absent
    "absent-call": [[1], [1, 1, 1], [0, 0], [1, 1, 1]],  # a whole call with nothing present
}


def rel_rms(a, b):
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / np.sqrt(np.mean(np.abs(b) ** 2)))


def rms(a):
    return float(np.sqrt(np.mean(np.abs(np.asarray(a, dtype=np.complex128)) ** 2)))


# ------------------------------------------------------------------------------------------------
# the kernel's algorithm in fp64, from the comment above k_modem_rate_pack -- and its wrong variants, each one line of it
# ------------------------------------------------------------------------------------------------
WRONG = ("a", "b", "c", "d", "e", "f")


def model(row, x, present, calls=CALLS, wrong=None):
    """one block row through the launches of `calls`: x the row's demodulator-rate samples of every super-frame (absent ones included: the
    audio buffer holds something there), present[call][super-frame] -> [call][super-frame] arrays of m outputs (zeros where absent).
    grid (tile, row, super-frame); the span of a tile is tn * D + H samples from o0 * D - H; `back` is the tail of the nearest present
    super-frame in front of j in this call, else the carry; the stages run in local indices; the carry comes from the owner of the last
    tile of the row's last present super-frame and is copied where nothing is present; the parity flips with every launch.
    wrong: None, or
      "a"  a look-back of H - 1: the span's oldest sample is not loaded
      "b"  the ragged last tile computed as a full one: it reads past the super-frame (and, owning no `last tile`, writes no carry)
      "c"  the carry taken as the last min(H, tn * D) samples of the tile, the rest left stale
      "d"  `back` always from super-frame j - 1, present or not
      "e"  the carry not copied through a launch with nothing present
      "f"  the parity not flipped"""
    D, H, spf, m, tile = row.D, row.H, row.spf, row.m, row.tile
    taps = [DC.halfband_taps()[T] for T, _ in row.chain]
    carry, parity = [np.zeros(H, dtype=np.complex128), np.zeros(H, dtype=np.complex128)], 0
    out, at = [], 0
    for k, ns in enumerate(calls):
        src = np.concatenate([x[at * spf:(at + ns) * spf], np.zeros(tile * D, dtype=np.complex128)])   # (room for model b's over-read)
        at += ns
        cin, cout = carry[parity], carry[parity ^ 1]
        pres = [bool(p) for p in present[k]]
        res = []
        for j in range(ns):
            if not pres[j]:
                res.append(np.zeros(m, dtype=np.complex128))
                continue
            before = [q for q in range(j) if pres[q]]
            jprev = (j - 1 if j else -1) if wrong == "d" else (before[-1] if before else -1)
            back = src[(jprev + 1) * spf - H:(jprev + 1) * spf] if jprev >= 0 else cin
            later = any(pres[j + 1:])
            y = np.zeros(m + tile, dtype=np.complex128)
            for o0 in range(0, m, tile):
                tn = tile if wrong == "b" else min(tile, m - o0)
                n0, p0 = tn * D + H, o0 * D - H
                p = p0 + np.arange(n0)
                span = np.where(p >= 0, src[j * spf + np.maximum(p, 0)], back[np.minimum(p, -1) + H])
                if wrong == "a":
                    span[0] = 0.0
                if not later and o0 + tn == m:
                    keep = min(H, tn * D) if wrong == "c" else H
                    cout[H - keep:] = span[n0 - keep:]
                v = span
                for (T, st), h in zip(row.chain, taps):
                    v = np.lib.stride_tricks.sliding_window_view(v, T)[::st] @ h
                y[o0:o0 + tn] = v[:tn]
            res.append(y[:m])
        if not any(pres) and wrong != "e":
            cout[:] = cin
        if wrong != "f":
            parity ^= 1
        out.append(res)
    return out


def oracle_pairs(O, row, x, present, calls=CALLS):
    """one fresh oracle.Decimator fed the present pairs, whole super-frames, in order -> ([call][super-frame] arrays or None, gains)"""
    dec = O.Decimator(demod_rate(row), row.bw, row.mn)
    out, gains, at = [], [], 0
    for k, ns in enumerate(calls):
        res = []
        for j in range(ns):
            seg = x[(at + j) * row.spf:(at + j + 1) * row.spf]
            if present[k][j]:
                res.append(dec.process(seg))
                gains.append(rms(res[-1]) / rms(seg))
            else:
                res.append(None)
        at += ns
        out.append(res)
    return out, gains


def worst(got, want):
    """-> (the worst rel-RMS over the present pairs, call, super-frame)"""
    figs = [(rel_rms(g, w), k, j) for k, (gc, wc) in enumerate(zip(got, want)) for j, (g, w) in enumerate(zip(gc, wc)) if w is not None]
    return max(figs)


# where each wrong model must miss MODEL's bar for the device -- PAIR_BAR -- tenfold at least: (row, pattern); the CPU tier asserts it,
# and says for the others on which rows they cannot be told apart
MISSES = {
    "a": ("d8-ragged", "all"),
    "b": ("d8-ragged", "all"),
    "c": ("d64-four", "all"),
    "d": ("d128", "gap"),
    "e": ("d64-four", "absent-call"),
    "f": ("d128-s16-scalar", "all"),
}


def lcm(a, b):
    return a // math.gcd(a, b) * b


# ------------------------------------------------------------------------------------------------
# the gated row: tail_cases' `gate` -- its channels, carriers, keys, thresholds and calls -- on the d64-four geometry (frames of 1536)
# ------------------------------------------------------------------------------------------------
GATE_NF = 1536
GATE_SFW = TC.D * lcm(GATE_NF, 1024)     # 49 152 samples: 3072 at the demodulator rate
# the FMN, the plain AM and the SAM channel, permuted: each hears a carrier at its centre, which the (500 Hz, 125 Hz) chain keeps; the
# two USB channels' tones (1100 Hz and more above the centre) are not in what a decimation to 1 kHz leaves
GATE_SEL = [3, 0, 2]


@functools.lru_cache(maxsize=None)
def gate_input():
    """tail_cases.row_input("gate") with super-frames of GATE_SFW samples: one key per super-frame"""
    row = TC.ROWS["gate"]
    n = sum(row.calls) * GATE_SFW
    t = np.arange(n) / float(TC.FS)
    x = lcg_noise(n, row.seed, row.noise)
    for fc, sig, key in row.carriers:
        level = TC.HI if key is None else np.repeat(np.where(np.asarray(key) > 0, TC.HI, TC.LO), GATE_SFW)
        x = x + TC._carrier(sig, fc, t, level)
    x.setflags(write=False)
    return x


def gate_bank(P):
    """tests/modem_out_cases.py::row_bank for the row `gate`, on frames of GATE_NF"""
    row = TC.ROWS["gate"]
    rx = P.ReceiverBank(TC.FS, len(row.chans), True, False, row.bins, frames_per_buffer=GATE_NF, max_superframes=row.max_sf)
    for c, ch in enumerate(row.chans):
        rx.set_mode(c, TC.MODE[ch.modes[0]]); rx.set_mixer(c, ch.fc); rx.set_bandpass(c, *ch.band)
        if ch.agc is not None:
            rx.set_agc(c, *ch.agc)
        if ch.anf:
            rx.set_noise_filter(c, True)
        if ch.squelch is not None:
            rx.set_squelch(c, ch.squelch)
    return rx
