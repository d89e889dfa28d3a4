"""The coverage statement for the overlap-save band-pass (csrc/kernels_fastfir.h: k_fastfir<4096|8192>, k_fastfir_t128<..>,
k_fastfir_t128_raw<0..4>): one table of (fft, taps) geometries, used by the CPU tier (tests/test_fastfir_geometry_host.py: the oracle
is the convolution at every row, the rows satisfy the library's size rules, and the input is one on which a lost overlap or an
off-by-one overlap cannot pass) and by the GPU tier (tests/test_fastfir_geometry_gpu.py: the same rows against the oracle).  No row
sets an environment switch.

overlap = taps - 1, L = fft - overlap.  The library accepts 2 <= taps <= fft/2 + 1, i.e. overlap <= L: beyond that the reference's
bookkeeping (which the oracle restates) is no convolution any more (test_fastfir_geometry_host.py pins that), so every row here is
one where the oracle is the truth.  At the three stock pairs overlap == L == fft/2 and `i >= overlap` is the same test as `i >= L`;
every other row tells them apart.

Three entry points:
 - STEP_ROWS: P.FastFIR (pebblegpu_fastfir_*, one channel, head-room buffer, the 64-block device loop) against oracle.FastFIR at 64 kHz;
 - RX_ROWS:   P.ReceiverBank at 2.048 Msps (three channels, FastFirCore::run behind the decimator, the lcm(frame, L) super-frame)
              against oracle.Receiver fed 2048-sample frames;
 - SB_ROWS:   P.StreamBank at 64 kHz (three streams, FastFirCore::run_ext: `tail` / `tail_out`, float2 and raw input) against a
              per-stream oracle.FastFIR fed oracle.normalize_iq of the same samples.
"""
from collections import namedtuple
import functools
import math

import numpy as np

from tests.signals import lcg_noise, tones

TOL = 1e-5          # BASELINE.json north_star, as tests/test_parity_gpu.py
FS = 64000.0
# tests/test_parity_gpu.py::test_fastfir_step's tones: one inside every pass-band below plus a strong out-of-band one
TONES = [(0.4873, 1000.0), (0.3, -12000.0), (0.2, 1250.0), (0.25, -1700.0)]
SIGMA = 1e-3
# (lo, hi, offset, rate): SetupParameters' arguments.  With its offset the first passes 1000 .. 3700 Hz, the second -3700 .. -1000 Hz
BANDS = [(300.0, 3000.0, 700.0, FS), (-3000.0, -300.0, -700.0, FS), (-5000.0, 5000.0, 0.0, FS)]
INVALID = (3000.0, 300.0, 0.0, FS)   # "Filter Parameter error": the previous taps stay (fastfir.cpp:208-216)
CTOR = (-1.0, 1.0, 1.0, 1.0)         # the constructor's own members (fastfir.cpp:141-144): SetupParameters returns early, the taps stay zero


def geometry(fft, taps):
    """-> (overlap, L)"""
    return taps - 1, fft - (taps - 1)


def accepted(fft, taps):
    """FastFirCore::init's rule"""
    return fft in (2048, 4096, 8192) and 2 <= taps <= fft // 2 + 1


# ---- comparison: rel-RMS over consecutive chunks of max(L, 1024) output samples, the first included ----
def chunk_bounds(n, L):
    """[(lo, hi)] covering n output samples; a remainder shorter than a chunk joins the last one (never its own denominator)"""
    size = max(L, 1024)
    k = max(1, n // size)
    return [(i * size, (i + 1) * size if i < k - 1 else n) for i in range(k)] if n else []


def rel_rms(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / max(np.sqrt(np.mean(np.abs(b) ** 2)), 1e-12))


def chunk_errors(got, ref, L):
    """rel-RMS of every chunk of one call's output; the lengths must agree exactly"""
    assert len(got) == len(ref), (len(got), len(ref))
    return [rel_rms(got[lo:hi], ref[lo:hi]) for lo, hi in chunk_bounds(len(ref), L)]


# ------------------------------------------------------------------------------------------------
# the stand-alone step
# ------------------------------------------------------------------------------------------------
StepRow = namedtuple("StepRow", "name fft taps L ctor why")


def _step(fft, taps, why, ctor=False):
    return StepRow("%d-%d%s" % (fft, taps, "-ctor" if ctor else ""), fft, taps, geometry(fft, taps)[1], ctor, why)


STEP_ROWS = [
    _step(2048, 2, "overlap 1: `i >= overlap` and `i >= L` are as different as they get"),
    _step(2048, 129, "L = 1920 is no power of two"),
    _step(2048, 1024, "odd overlap 1023, odd L 1025, one short of the stock pair"),
    _step(2048, 1025, "stock"),
    _step(4096, 1025, "k_fastfir<4096> with L = 3072 = 3 overlap"),
    _step(4096, 2049, "stock"),
    _step(8192, 1025, "k_fastfir<8192> with L = 7168 = 7 overlap"),
    _step(8192, 4097, "stock"),
    _step(2048, 1025, "a fresh object given the constructor's own parameters: no design, all-zero taps", ctor=True),
]


def step_calls(row):
    """1, L-1, L, L+1, 3L, then 66L+5: more than the step's 64-block device buffer holds, so its loop runs twice and leaves a ragged rest"""
    L = row.L
    return [1, L - 1, L, L + 1, 3 * L, 66 * L + 5]


def step_cases():
    """(row, band index) pairs: every band on every row (the constructor row has no band)"""
    return [(r, b) for r in STEP_ROWS for b in (range(len(BANDS)) if not r.ctor else (None,))]


def step_script(row, b):
    """[("setup", (lo, hi, offset, rate), accepted) | ("call", n)]: band b; the same parameters again (no redesign); the invalid pair
    (refused, the taps stay); then a real redesign to the next band, in force for the two long calls"""
    n = step_calls(row)
    if row.ctor:
        return [("setup", CTOR, True)] + [("call", k) for k in n[2:5]]
    A, B = BANDS[b], BANDS[(b + 1) % len(BANDS)]
    return [("setup", A, True), ("call", n[0]), ("call", n[1]), ("setup", A, True), ("call", n[2]), ("setup", INVALID, False), ("call", n[3]),
            ("setup", B, True), ("call", n[4]), ("call", n[5])]


def script_samples(script):
    return sum(e[1] for e in script if e[0] == "call")


@functools.lru_cache(maxsize=None)
def step_input(row):
    n = script_samples(step_script(row, 0 if not row.ctor else None))
    x = tones(FS, n, TONES) + lcg_noise(n, 40 + STEP_ROWS.index(row), SIGMA)
    x.setflags(write=False)
    return x


def run_script(script, x, setup, process):
    """setup(lo, hi, offset, rate) -> accepted?; process(samples) -> output.  -> one output per call"""
    outs, at = [], 0
    for e in script:
        if e[0] == "setup":
            assert bool(setup(*e[1])) == e[2], e
        else:
            outs.append(process(x[at:at + e[1]]))
            at += e[1]
    assert at == len(x)
    return outs


# ------------------------------------------------------------------------------------------------
# the receiver bank
# ------------------------------------------------------------------------------------------------
RX_FS, RX_FRAME, RX_D = 2_048_000, 2048, 32   # hb chain to 64 kHz
RX_CALLS = (1, 2, 1)                          # super-frames per call
# (mode, lo, hi, mixer frequency)
RX_CHANNELS = [("USB", 300.0, 3000.0, 100.0e3), ("AM", -5000.0, 5000.0, -250.0e3), ("USB", 500.0, 2600.0, 400.5e3)]
RxRow = namedtuple("RxRow", "name fft taps L why")
RX_ROWS = [
    RxRow("rx-2048-513", 2048, 513, 1536, "the XCD-ordered grid with nb * C = 12 blocks in a one-super-frame call: no multiple of 8"),
    RxRow("rx-4096-1025", 4096, 1025, 3072, "k_fastfir<4096> on the decimator's head-room buffer, L = 3 overlap"),
    RxRow("rx-8192-2049", 8192, 2049, 6144, "k_fastfir<8192>, one block per frame group"),
]


def rx_superframe(row):
    """Receiver::create: total decimation times lcm(frame, L), in input samples"""
    return RX_D * (RX_FRAME * row.L // math.gcd(RX_FRAME, row.L))


def rx_blocks(row, superframes):
    """band-pass blocks per channel in a call"""
    return superframes * rx_superframe(row) // RX_D // row.L


@functools.lru_cache(maxsize=None)
def rx_input(n):
    """every channel: tones inside its pass-band and one outside, AM as a carrier with two sidebands"""
    (_, _, _, f0), (_, _, _, f1), (_, _, _, f2) = RX_CHANNELS
    x = tones(RX_FS, n, [(0.1, f0 + 1000.0), (0.04, f0 + 2200.0, 0.7), (0.06, f0 - 2000.0),
                         (0.2, f1), (0.05, f1 + 1000.0, 0.3), (0.05, f1 - 1000.0, -0.3), (0.03, f1 + 9000.0),
                         (0.1, f2 + 1500.0, 1.1), (0.07, f2 + 4000.0)]) + lcg_noise(n, 61, SIGMA)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------
# the stream bank
# ------------------------------------------------------------------------------------------------
SB_S, SB_CALLS, SB_FRAMES = 3, 3, 2           # streams, calls, frames per call
SB_BANDS = [(300.0, 3000.0), (-3000.0, -300.0), (-5000.0, 5000.0)]   # per stream (the bank's design has no offset)
# pebblegpu_iq_format -> (name in kernel_name, numpy type of a component, offset, full scale used, gain)
FORMATS = {0: ("s8", np.int8, 0.0, 127.0, 0.7), 1: ("u8", np.uint8, 128.0, 127.0, 1.0), 2: ("s16", np.int16, 0.0, 32000.0, 1.3),
           3: ("f32", np.float32, 0.0, 1.0, 0.9), 4: ("wav16", np.int16, 0.0, 32000.0, 0.5)}
# fmts: None float2 input, else a pebblegpu_iq_format.  kernel: what kernel_name(1) says for float2 input
SbRow = namedtuple("SbRow", "name fft taps L frame bins fmts kernel why")
SB_ROWS = [
    SbRow("sb-2048-513", 2048, 513, 1536, 3072, 4096, (None, 0, 1, 2, 3, 4), "k_fastfir_t128",
          "the one-dimensional grid with nb * S = 12 and `tail_out` written from i >= L = 1536 != overlap, in every instance"),
    SbRow("sb-2048-129", 2048, 129, 1920, 1920, 2048, (None, 0), "k_fastfir_t128", "nb * S = 6: fewer blocks than XCDs; `tail_out` is 128 samples"),
    SbRow("sb-4096-1025", 4096, 1025, 3072, 3072, 4096, (None,), "k_fastfir", "the two-dimensional k_fastfir<4096> and the hipMemcpy2DAsync tail"),
    SbRow("sb-8192-2049", 8192, 2049, 6144, 6144, 8192, (None,), "k_fastfir", "the same with k_fastfir<8192>"),
]


def sb_cases():
    return [(r, f) for r in SB_ROWS for f in r.fmts]


def sb_call_samples(row):
    return SB_FRAMES * row.frame


def sb_blocks(row):
    return sb_call_samples(row) // row.L


def sb_kernel(row, fmt, what=1):
    """kernel_name(1) of a call: the converting instance where the call asks for the band-pass alone (what = 1) on the 2048-point plan;
    with the display transform in the same call (what = 3) these frame lengths have no converting display kernel and the call is staged"""
    if fmt is None:
        return row.kernel
    if row.fft == 2048 and what == 1:
        return "%s (raw %s)" % (row.kernel, FORMATS[fmt][0])
    return "k_normalize_iq + " + row.kernel


@functools.lru_cache(maxsize=None)
def _sb_signal(row):
    """[S, n] in double precision, |component| <= 0.93: the step's tones moved and turned per stream (a kernel that reads a neighbour's
    row reads something else) plus noise of the stream's own seed"""
    n = SB_CALLS * sb_call_samples(row)
    x = np.stack([0.75 * (tones(FS, n, [(a, f + 37.0 * s, 1.3 * s) for a, f in TONES]) + lcg_noise(n, 80 + 10 * SB_ROWS.index(row) + s, SIGMA))
                  for s in range(SB_S)])
    x.setflags(write=False)
    return x


def sb_raw(row, fmt):
    """[S, n, 2] components of `fmt`"""
    _, dtype, off, full, _ = FORMATS[fmt]
    x = _sb_signal(row)
    comp = np.stack([x.real, x.imag], axis=-1)
    if dtype == np.float32:
        return comp.astype(np.float32)
    return (np.round(comp * full) + off).astype(dtype)


def sb_input(row, fmt, oracle_mod=None):
    """-> (what the bank is fed [S, n] complex64 or [S, n, 2] raw, what the oracle is fed [S, n] complex128, gain)"""
    if fmt is None:
        x = _sb_signal(row).astype(np.complex64)
        return x, x.astype(np.complex128), 1.0
    raw, gain = sb_raw(row, fmt), FORMATS[fmt][4]
    return raw, np.stack([oracle_mod.normalize_iq(raw[s].reshape(-1), fmt, 0, gain) for s in range(SB_S)]), gain
