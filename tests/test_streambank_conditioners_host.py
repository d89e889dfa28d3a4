"""Host tier of the stream bank's input conditioners (pebblegpu_streambank_set_conditioners / _conditioned): what needs no device,
and what tests/test_streambank_conditioners_gpu.py shares -- the test input, the oracle's side of the chain and the MARGIN CONDITION.

The oracle's side is composed from what oracle/__init__.py has, each pinned to the reference by tests/test_reference_pins.py: Iir
high-pass 10 Hz / Q 0.7071 (DCRemoval), iq_balance per frame, NoiseBlanker with enable(1 | 2) and process(which=), in the reference's
order (receiver.cpp:814-823).

The margin condition.  A blanker's decision is the comparison mag > 3.3 avg.  The device gives every run of 8 samples its average from
an fp64 scan and rounds to float per step from there; the serial form rounds to float all the way: the two averages differ in the last
bits (2e-6 relative, measured on the serial chain).  So the inputs here leave every decision room, and that is asserted on the CPU from
a double restatement of the averages: for every sample of every blanker's input, |mag - 3.3 avg| >= 1e-4 * 3.3 avg.  It is a
condition on the INPUT; failing it fails the test.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import scipy.signal as ss

from tests.signals import lcg_noise, tones

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-4
CHUNK, SUB, SEG = 2048, 512, 8   # kernels_condition.h: samples per workgroup, per wave step, per lane
E_INVALID = -1


def spiky(fs, n, seed, edges, runs, f_tone=101e3, level=1.0):
    """the _spiky recipe of tests/test_conditioners_gpu.py (tones 0.05 and 0.02, LCG noise 1e-3, DC 0.01) with spikes of 1.5 .. 3.0 at
    offsets -3, +2 and +5 around every edge and a run of 40 consecutive spikes from every position in runs"""
    x = tones(fs, n, [(0.05, f_tone), (0.02, -0.122 * fs)]) + lcg_noise(n, seed, 1e-3) + 0.01
    amps = (1.5, -3.0, 2.0j)
    for e in edges:
        for off, a in zip((-3, 2, 5), amps):
            if 0 <= e + off < n:
                x[e + off] += a
    for r in runs:
        x[r:r + 40] += 2.0
    return x * level


def edges_for(n, frame, calls):
    """sample positions whose neighbourhoods get spikes: every workgroup (chunk) boundary of every call -- with it every frame and call
    boundary, both multiples of it or equal to it here -- a wave-step and two lane boundaries inside the first chunk of every call, and
    64 and 1000"""
    out, at = {64, 1000}, 0
    for c in calls:
        m = c * frame
        out.update(range(at + CHUNK, at + m, CHUNK))
        out.update((at, at + SUB, at + 3 * SUB, at + 5 * SEG, at + SUB + 9 * SEG))
        at += m
    assert at == n
    return sorted(e for e in out if 0 < e < n)


class Chain:
    """one stream's conditioners on the oracle: set(flags, gain, phase) as pebblegpu_streambank_set_conditioners, process(x) frame by
    frame; nb_in collects every blanker's input (for the margin condition), with the average it entered with"""

    def __init__(self, oracle_mod, fs, frame):
        self.O, self.frame, self.flags, self.gain, self.phase = oracle_mod, frame, 0, 1.0, 0.0
        self.dc = oracle_mod.Iir("hp", 10, 0.7071, fs)
        self.nb = oracle_mod.NoiseBlanker()
        self.nb_in = []

    def set(self, flags, gain=1.0, phase=0.0):
        for bit, which in ((4, 1), (8, 2)):
            if flags & bit and not self.flags & bit:
                self.nb.enable(which)
        self.flags, self.gain, self.phase = flags, gain, phase

    def process(self, x):
        out = []
        for f in range(len(x) // self.frame):
            v = np.asarray(x[f * self.frame:(f + 1) * self.frame], dtype=np.complex128)
            if self.flags & 1:
                v = self.dc.process(v)
            if self.flags & 2:
                v = self.O.iq_balance(v, self.gain, self.phase)
            if self.flags & 4:
                self.nb_in.append((float(self.nb.s.nb_avg_mag), v))
                v = self.nb.process(v, which=1)
            if self.flags & 8:
                self.nb_in.append((float(self.nb.s.nb2_avg_mag), v))
                v = self.nb.process(v, which=2)
            out.append(v)
        return np.concatenate(out)


def smallest_margin(nb_in):
    """min over every sample of every recorded blanker input of |mag - 3.3 avg| / (3.3 avg), the averages restated in double from the
    value each block entered with"""
    worst = np.inf
    for a0, v in nb_in:
        mag = np.abs(v)
        avg, _ = ss.lfilter([0.001], [1.0, -0.999], mag, zi=[0.999 * a0])
        with np.errstate(divide="ignore", invalid="ignore"):  # (avg 0, before anything came in: |mag - 0| >= 0 holds)
            worst = min(worst, float(np.min(np.where(avg > 0, np.abs(mag - 3.3 * avg) / (3.3 * avg), np.inf))))
    return worst


def assert_margin(chains, what):
    m = min(smallest_margin(c.nb_in) for c in chains if c.nb_in)
    print("%s: smallest decision margin %.3e (needs %.0e)" % (what, m, MARGIN))
    assert m >= MARGIN, "the test INPUT leaves a blanker decision no room: %.3e" % m


def fastfir_and_spectrum(oracle_mod, v, fs, frame, bins, lo, hi):
    """the bank's two transforms on the oracle, as the existing stream-bank tests build them -> (filtered, dB rows [frames, bins])"""
    f = oracle_mod.FastFIR(2048, 1025)
    f.setup(lo, hi, 0.0, fs)
    sp = oracle_mod.Spectrum(bins, frame, lift_clamp=True) if frame == 65536 else oracle_mod.Spectrum(bins, frame)
    y = np.concatenate([f.process(v[k:k + frame]) for k in range(0, len(v), frame)])
    return y, np.array([sp.process(v[k:k + frame]) for k in range(0, len(v), frame)])


# ---- 8: what needs no device ----
def test_null_handle_returns():
    import pebblesdr_amd as P
    L = P.load_library()
    assert L.pebblegpu_streambank_set_conditioners(None, 0, 1, 1.0, 0.0) == E_INVALID
    assert b"null" in L.pebblegpu_last_error()
    n, pitch = C.c_uint64(7), C.c_uint64(7)
    assert L.pebblegpu_streambank_conditioned(None, C.byref(n), C.byref(pitch)) is None
    assert (n.value, pitch.value) == (0, 0)
    assert L.pebblegpu_streambank_conditioned(None, None, None) is None


def test_both_functions_are_declared_bound_and_exported():
    import pebblesdr_amd as P
    from pebblesdr_amd.binding import SYMBOLS
    header = open(os.path.join(ROOT, "include", "pebblegpu.h")).read()
    mine = sorted(set(re.findall(r"\b(pebblegpu_streambank_(?:set_conditioners|conditioned))\s*\(", header)))
    assert mine == ["pebblegpu_streambank_conditioned", "pebblegpu_streambank_set_conditioners"]
    L = P.load_library()
    for name in mine:
        assert name in SYMBOLS and SYMBOLS.count(name) == 1
        assert getattr(L, name).argtypes is not None
    assert hasattr(P.StreamBank, "set_conditioners") and hasattr(P.StreamBank, "conditioned")


# ---- the oracle's side and the inputs of the GPU tier ----
def test_chain_is_the_oracle_receivers_conditioner_block(oracle_mod):
    """Chain against oracle.Receiver.set_conditioners on the same samples, through what both feed: the unprocessed spectrum"""
    fs, n, bins = 2048000, 2048, 2048
    x = spiky(fs, 4 * n, 20, edges_for(4 * n, n, [4]), [5000])
    ref = oracle_mod.Receiver(fs, n, bins)
    ref.set_conditioners(15, 1.02, 0.03)
    ch = Chain(oracle_mod, fs, n)
    ch.set(15, 1.02, 0.03)
    v = ch.process(x)
    sp = oracle_mod.Spectrum(bins, n)
    for f in range(4):
        want = ref.process(x[f * n:(f + 1) * n])[1]
        got = sp.process(v[f * n:(f + 1) * n])
        assert np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def margin_of(seed, level):
    import oracle
    oracle.build()
    fs, n = 2048000, 3 * 16384
    x = spiky(fs, n, seed, [64, 512, 4096, 8192, 16384, 32768], [20000], level=level)
    ch = Chain(oracle, fs, 2048)
    ch.set(15, 1.02, 0.03)
    ch.process(x)
    return smallest_margin(ch.nb_in)


def test_the_recipe_meets_the_margin_condition(oracle_mod):
    got = [margin_of(seed, 1.0) for seed in (20, 21, 22)]
    print("smallest margins, seeds 20 / 21 / 22: %s" % got)
    assert min(got) >= MARGIN


def test_margin_restatement_follows_the_oracles_float_average(oracle_mod):
    """the double restatement against the float average the oracle's blanker ends with: within 1e-5 relative (measured 2e-6)"""
    fs, n = 2048000, 16384
    x = spiky(fs, n, 20, [64, 512, 4096, 8192], [6000])
    nb = oracle_mod.NoiseBlanker()
    nb.enable(1)
    nb.process(x, which=1)
    avg, _ = ss.lfilter([0.001], [1.0, -0.999], np.abs(x), zi=[0.0])
    rel = abs(float(nb.s.nb_avg_mag) - avg[-1]) / avg[-1]
    print("float average against its double restatement after %d samples: %.2e relative" % (n, rel))
    assert rel <= 1e-5
