"""The coverage statement for k_mix_dec_mfma (csrc/kernels_bank_dec.h): one table of bank shapes, used by the CPU tier
(tests/test_bank_decimator_host.py: which instance and which chunk geometry every row reaches) and by the GPU tier
(tests/test_bank_decimator_gpu.py: the same rows against the oracle).  No row sets an environment switch.

A row's calls are given in super-frames.  The first call of a handle lies inside the oscillators' amplitude transient and the
call after a retune does too: both take the two-kernel route, so their geometry entry is None.  Every other call is one launch
of k_mix_dec_mfma, expected at (waves per SIMD, outputs per chunk) as bank_geometry() of csrc/bank_geom.h says.

The input of every row is periodic in three super-frames (every frequency is a multiple of fs / (3 * 2048 * D)), so that
 - a call's input is synthesised on its own by inverse FFTs of the call's length (2080 tones, or 8.4 M samples at 200 Msps),
 - the tone of channel c falls exactly on bin `bins[c]` of the 6144-point FFT of the run's last 3 * 2048 output samples.
"""
from collections import namedtuple

import numpy as np

from tests.signals import lcg_noise, lcg_uniform

Row = namedtuple("Row", "name fs C wfm spectrum_bins max_superframes calls instance geometry retune_before")
FRAME = 2048  # outputs per super-frame (narrow: lcm(2048, 2048 - 1024); WFM: the frame itself)


def _row(name, fs, C, instance, geometry, calls=(1, 1, 1), wfm=False, spectrum_bins=0, max_superframes=None, retune_before=None):
    return Row(name, fs, C, wfm, spectrum_bins, max_superframes or max(calls), tuple(calls), instance, tuple(geometry), retune_before)


_ = None
ROWS = [
    # ---- every instance with a ragged bank of five channel groups (a second quad of one live wave, 5 live lanes in the last group) ----
    _row("inst-4-15-23-43", 3_200_000, 133, (4, 15, 23, 43), [_, (1, 16), (1, 16)]),
    _row("inst-4-15-23-47", 3_000_000, 133, (4, 15, 23, 47), [_, (1, 16), (1, 16)]),
    _row("inst-4-15-19-35", 3_840_000, 133, (4, 15, 19, 35), [_, (1, 16), (1, 16)]),
    _row("inst-4-19-27-59", 2_400_000, 133, (4, 19, 27, 59), [_, (1, 32), (1, 32)]),
    # (five calls, a channel retuned before the third: it takes the two-kernel route, the fourth comes back without running sums)
    _row("inst-4-15-27-59-retune", 5_000_000, 133, (4, 15, 27, 59), [_, (1, 32), _, (1, 32), (1, 32)], calls=(1, 1, 1, 1, 1), retune_before=2),
    _row("inst-4-15-19-31", 4_000_000, 133, (4, 15, 19, 31), [_, (1, 16), (1, 16)]),
    _row("inst-12-15-19-35-s0x8", 61_440_000, 133, (12, 15, 19, 35), [_, (1, 16), (1, 16)]),
    _row("inst-12-15-27-59-s0x8-retune", 40_000_000, 133, (12, 15, 27, 59), [_, (1, 32), _, (1, 32), (1, 32)], calls=(1, 1, 1, 1, 1), retune_before=2),
    _row("inst-12-15-23-47-s0x8", 50_000_000, 133, (12, 15, 23, 47), [_, (1, 16), (1, 16)]),
    # ---- front strides: hb11 x 2 and x 16 with a second group of one live lane; CIC3 at stride 32 (353 samples in front of the call) ----
    _row("hb11x2", 1_024_000, 33, (4, 15, 19, 31), [_, (1, 16), (1, 16)]),
    _row("hb11x16", 6_400_000, 33, (4, 15, 23, 43), [_, (1, 16), (1, 16)]),
    _row("cic3x32", 200_000_000, 17, (12, 15, 23, 47), [_, (1, 16), (1, 16)]),
    # ---- longer chunks; L changing between the calls of one handle ----
    _row("long-hb-544", 2_500_000, 544, (4, 15, 27, 59), [_, (1, 32), (1, 32)]),
    _row("long-cic-544", 12_500_000, 544, (12, 15, 23, 47), [_, (1, 64), (1, 64)]),
    _row("mixed-lengths-hb", 2_400_000, 224, (4, 19, 27, 59), [_, (1, 64), (1, 32), (1, 64)], calls=(1, 8, 2, 8)),
    _row("mixed-lengths-cic", 10_000_000, 96, (12, 15, 27, 59), [_, (1, 64), (1, 32), (1, 64)], calls=(1, 8, 2, 8)),
    # ---- two waves per SIMD: no two-stage calls with a display transform, a call long against its warm-up ----
    _row("two-waves-4-15-23-43", 3_200_000, 256, (4, 15, 23, 43), [_, (2, 64), (2, 64)], calls=(1, 16, 16), spectrum_bins=2048),
    _row("two-waves-4-15-19-31", 2_048_000, 256, (4, 15, 19, 31), [_, (2, 64), (2, 64)], calls=(1, 16, 16), spectrum_bins=2048),
    # ---- WFM through the bank kernel: gain 1, an output without look-back ----
    _row("wfm-20M", 20_000_000, 33, (4, 15, 23, 47), [_, (1, 16), (1, 16)], calls=(2, 2, 2), wfm=True),
    # ---- fewer chunk pairs than a stretch of eight workgroups holds ----
    _row("pairs-below-8", 12_500_000, 2080, (12, 15, 23, 47), [_, (1, 256), (1, 256)]),
]
del _


def instance_of(chain):
    """(NP, T1, T2, T3) of the k_mix_dec_mfma instance a bank of >= 16 channels with this chain takes (DecimCore::init): hb11 x S
    (S <= 16) gives NP = 4, CIC3 x S0 + hb11 x 16 gives NP = 12, three stride-2 halfbands behind either.  None: another route."""
    chain = [tuple(s) for s in chain]
    if len(chain) == 4 and chain[0][0] == 11 and chain[0][1] <= 16:
        np_, rest = 4, chain[1:]
    elif len(chain) == 5 and chain[0][0] == 0 and chain[1] == (11, 16):
        np_, rest = 12, chain[2:]
    else:
        return None
    if [s for _, s in rest] != [2, 2, 2]:
        return None
    return (np_,) + tuple(t for t, _ in rest)


def front_stride(chain):
    """S of hb11 x S, or S0 of the CIC3 in front of hb11 x 16"""
    return int(chain[0][1])


def warm_blocks(instance):
    """FusedDecGeom<T1, T2, T3>::warm: the halfbands' look-back in blocks of eight first-stage outputs"""
    _, t1, t2, t3 = instance
    return ((t1 - 1) + 2 * (t2 - 1) + 4 * (t3 - 1)) // 8


def has_two_stage_calls(row):
    """Receiver::create: a narrow receiver without a display transform doubles the decimator's output (fin2)"""
    return not row.wfm and row.spectrum_bins == 0


def protect_bw(row):
    return 200000 if row.wfm else 30000


def mfma_calls(row):
    return [k for k, g in enumerate(row.geometry) if g is not None]


def _largest_prime_up_to(n):
    for p in range(n, 1, -1):
        if all(p % q for q in range(2, int(p ** 0.5) + 1)):
            return p
    raise ValueError(n)


Plan = namedtuple("Plan", "D period df zero retuned extra fc_idx fc tone_idx bins band extra_fc extra_tone_idx extra_bin amp compare")
DENSE = 133  # channels above which a row's band-passes are narrowed onto the channels' own tones (see plan())


def decimation(chain):
    return int(np.prod([s for _, s in chain]))


def plan(row, chain):
    """Tunings, tones and band-passes of a row with this decimation chain.

    Channel c is tuned to fc[c] = (c - zero) * spacing: channel `zero`, in the middle of a channel group, sits at exactly 0.0 Hz
    (the mixer's pass-through).  Its tone lies bins[c] grid steps above, 200 Hz or more inside the USB band-pass 300 .. 3000 Hz.
    A row with a retune carries one more carrier above the last channel: channel `retuned` moves there before call retune_before.

    Up to DENSE channels every channel has a bin of its own and the band-pass is 300 .. 3000 Hz: the channels lie 12 kHz or more
    apart, and what the merged first stage (one 11-tap halfband at stride S: no stop band at the multiples of fs / S beyond the
    first few) folds into a channel from the others misses its band-pass (the host tier checks it on the oracle).  A denser bank
    cannot be lit like that: channels fs / S apart fold into each other at full level, and the reference itself shows a
    neighbour's tone as large as the channel's own.  There the spacing divides fs / S, so that channel c folds exactly onto the
    channels c +- j M; the tones of channels 1, 2 and 3 M apart are kept 400 Hz or more apart, and every channel's band-pass is
    300 Hz wide around its own tone (still inside 300 .. 3000 Hz)."""
    C, D = row.C, decimation(chain)
    period = 3 * FRAME * D
    df = row.fs / period
    b_lo, b_hi = int(np.ceil(500.0 / df)), int(np.floor(2800.0 / df))
    avail = b_hi - b_lo + 1
    zero = (C // 2) // 32 * 32 + 13
    if zero >= C or C < 32:
        zero = C // 2
    spacing = int(round(0.7 * row.fs / C / df))
    if C <= DENSE or row.wfm:
        assert C + 1 <= avail
        bins = [b_lo + c for c in range(C)]
        extra_bin = b_lo + C
        band = [(300.0, 3000.0)] * C
    else:
        fold = period // (chain[0][1] * (chain[1][1] if chain[0][0] == 0 else 1))  # fs / S in grid steps: 3 * 2 ** k
        m = min(v for v in [2 ** b for b in range(12)] + [3 * 2 ** b for b in range(12)] if v * spacing >= fold)
        assert fold % m == 0
        spacing = fold // m
        slot = avail // 4
        bins = [b_lo + (c // m) % 4 * slot + (c % m) % (slot // 4) for c in range(C)]
        assert (slot - slot // 4) * df >= 400.0
        extra_bin = b_lo
        band = [(b * df - 150.0, b * df + 150.0) for b in bins]
    fc_idx = [(c - zero) * spacing for c in range(C)]
    extra_idx = (C + 1 - zero) * spacing
    assert extra_idx * df < 0.47 * row.fs and -fc_idx[0] * df < 0.47 * row.fs
    retuned = None
    if row.retune_before is not None:
        retuned = (zero + 32 + 5) % C  # (another group than the 0 Hz channel's, mid-group)
        band[retuned] = (300.0, 3000.0)
    pick = [int(u * C) for u in lcg_uniform(3, C)]
    edges = {0, 1, 30, 31, 32, 33, 63, 64, 127, 128, C - 2, C - 1, 2047, 2048, zero}
    compare = sorted({c for c in edges | set(pick) | ({retuned} if retuned is not None else set()) if 0 <= c < C})
    return Plan(D, period, df, zero, retuned, row.retune_before is not None, fc_idx, [i * df for i in fc_idx], [i + b for i, b in zip(fc_idx, bins)], bins, band,
                extra_idx * df, extra_idx + extra_bin, extra_bin, min(0.05, 0.5 / np.sqrt(C)), compare)


def final_bins(row, p):
    """bin of the 6144-point FFT of the run's last three output frames in which every channel's peak lies"""
    b = list(p.bins)
    if p.retuned is not None:
        b[p.retuned] = p.extra_bin
    return b


def _carriers(row, p):
    idx = list(p.tone_idx)
    if p.extra:
        idx.append(p.extra_tone_idx)
    return idx


def call_start(row, p, k):
    return sum(row.calls[:k]) * FRAME * p.D


def call_input(row, p, k):
    """the input of call k alone: the row's periodic carriers over the call's samples + LCG noise of the call's own seed"""
    n, start = row.calls[k] * FRAME * p.D, call_start(row, p, k)
    if row.wfm:
        x = _fm_carriers(row, p, start, n)
    else:
        x = synth_tones(_carriers(row, p), p.period, start, n) * p.amp
    return x + lcg_noise(n, 5 + k, 1e-3)


def synth_tones(idx, period, start, n):
    """sum over m in idx of exp(2j pi m (start + i) / period), i = 0 .. n - 1, where period divides 3 n: the tones whose
    3 n m / period is r mod 3 are bins of an n-point inverse FFT, turned by the slow ramp exp(2j pi r i / (3 n))"""
    assert (3 * n) % period == 0
    j = 3 * n // period
    spec = np.zeros((3, n), dtype=np.complex128)
    for m in idx:
        q, r = divmod(m * j, 3)
        spec[r, q % n] += np.exp(2j * np.pi * ((m * start) % period) / period)
    x = np.zeros(n, dtype=np.complex128)
    i = np.arange(n, dtype=np.float64)
    for r in range(3):
        if spec[r].any():
            y = np.fft.ifft(spec[r]) * n
            x += y * np.exp(2j * np.pi * r * i / (3.0 * n)) if r else y
    return x


def direct_tones(idx, period, start, n):
    """synth_tones() evaluated tone by tone (the host tier compares the two)"""
    t = (np.arange(n, dtype=np.int64) + start)
    x = np.zeros(n, dtype=np.complex128)
    for m in idx:
        x += np.exp(2j * np.pi * ((m * t) % period) / period)
    return x


def _fm_carriers(row, p, start, n):
    """WFM rows: one FM carrier per channel, 50 kHz deviation, modulated by the channel's own audio tone bins[c] * df"""
    t = (np.arange(n, dtype=np.int64) + start)
    x = np.zeros(n, dtype=np.complex128)
    for c in range(row.C):
        fa = p.bins[c]
        car = 2 * np.pi * ((p.fc_idx[c] * t) % p.period) / p.period
        x += p.amp * np.exp(1j * (car + (50e3 / (fa * p.df)) * np.sin(2 * np.pi * ((fa * t) % p.period) / p.period)))
    return x


def peak_bins(y):
    """y: [channels, >= 6144] outputs -> the largest bin of the last 6144 samples' FFT, bin 0 left out (complex USB audio: the
    whole circle; WFM audio is real: the lower half of its real part's)"""
    z = np.asarray(y)[..., -3 * FRAME:]
    s = np.abs(np.fft.fft(z, axis=-1))
    return np.argmax(s[..., 1:], axis=-1) + 1


def peak_bins_wfm(y):
    z = np.asarray(y)[..., -3 * FRAME:].real
    s = np.abs(np.fft.rfft(z, axis=-1))
    return np.argmax(s[..., 1:-1], axis=-1) + 1


class OracleChannel:
    """Mixer -> Decimator -> gain restore -> FastFIR (narrow USB, the channel's band-pass) or Mixer -> Decimator -> DemodWFM of channel c, fed
    whole super-frames, call by call"""

    def __init__(self, oracle_mod, row, p, c, chain=None):
        self.row, self.p, self.c = row, p, c
        self.mix = oracle_mod.Mixer(row.fs)
        self.mix.set_frequency(p.fc[c])
        self.dec = oracle_mod.Decimator(row.fs, protect_bw(row))
        if chain is not None:
            assert self.dec.chain() == chain
        rate = int(row.fs / p.D)
        if row.wfm:
            self.gain = 1.0
            self.last = oracle_mod.DemodWFM(rate)
        else:
            self.gain = 10 ** (2 * int(round(np.log2(p.D))) / 20.0)  # "restore gain lost in decimation", 2 dB per halving
            self.last = oracle_mod.FastFIR()
            self.last.setup(p.band[c][0], p.band[c][1], 0, rate)

    def call(self, k, x):
        """the output of call k (input x), every call of the run given in order"""
        sf = FRAME * self.p.D
        if k == self.row.retune_before and self.c == self.p.retuned:
            self.mix.set_frequency(self.p.extra_fc)  # (Mixer::setFrequency starts the oscillator again)
        z = np.concatenate([self.dec.process(self.mix.process(x[i:i + sf])) for i in range(0, len(x), sf)]) * self.gain
        return np.concatenate([self.last.process(z[i:i + FRAME]) for i in range(0, len(z), FRAME)])


def oracle_channel(oracle_mod, row, p, c, inputs, chain=None):
    """-> the whole run's output of channel c; `inputs` yields the calls' inputs in order"""
    o = OracleChannel(oracle_mod, row, p, c, chain)
    return np.concatenate([o.call(k, x) for k, x in enumerate(inputs)])
