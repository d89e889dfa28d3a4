"""The coverage statement for WHOLE RECEIVERS at frame sizes other than 2048 (pebblegpu_receiver_create takes frames_per_buffer 256 .. 65535
and three band-pass sizes).  The frame size reaches into a call's tail in these places: the super-frame is total * lcm(nf, L); the band-pass
releases 0, 1, 2 or 3 blocks per demodulator-rate frame; k_pll_demod places Demod_NFM's phase wrap from (blk_len, blk_frame); the resampler
works in frames of nf; the S-meter and the bank gate count superframe / nf raw frames; a WFM receiver's call is shorter than k_wfm_fir's
history (Lx = L4 + Llp, 593 at 256 kHz) as soon as nf < Lx; and WfmCore::stereo_block = nf sets the pilot block, the RDS block and how often
the group queue is polled.  Every other table of this suite runs at frames of 2048 with the stock 2048/1025 band-pass.

One table of rows, their inputs (recipes with the seeds written here; nothing is stored), the oracle drivers and the comparison, used by the
CPU tier (tests/test_receiver_frames_host.py) and by the GPU tier (tests/test_receiver_frames_gpu.py: every row through P.ReceiverBank
against oracle.Receiver(fs, nf, bins, fft, taps) fed frame by frame).  No row sets an environment switch, no kernel is launched directly.
Call scripts are given in super-frames.

Bars, all imported, none new: TOL, TOL_AGC_STARTUP, tail_cases.TOL_SAM, TOL_NFM_WRAP for the narrow rows per chunk of 512 outputs of the
stream (every call is a whole number of such chunks), 256 behind the resampler (k_resample's block); demod_cases.TOL per chunk of 1024 for
WFM mono; rds_cases.AUDIO_TOL and call_errors for dmFMS audio; lengths, groups and `changed` flags exact.

Where a narrow stream starts the rule is tail_cases.compared_chunks', restated on stream positions because a super-frame is not 2048 outputs
here (stream_chunks): the chunks inside the band-pass's rise join the chunk behind them (joined_at_start: AM's chunk 0 at the stock sizes,
SAM's at 2049 taps); behind a running AGC chunk 0 is the delay line's zeros and chunk 1 joins chunk 2; an FMN channel is compared from
the first wrap at or behind FMN_SKIP outputs (fmn_first_compared), and the chunk that starts there is held to TOL_NFM_WRAP.  The CPU tier
holds all of it to what the oracle's own parts do under the band-pass's fp32 floor.  The FMN carriers sit 100 .. 400 Hz off tune (the
rows' _fmn offsets), so that Demod_NFM's float phase counts up to 30 .. 40 rad between two wraps: a wrap put elsewhere then changes the
output (the CPU tier's wrong models, 9e-7 .. 2e-4 against a bar of 1e-9), while the phase's resolution (4e-6 rad there) keeps the
reference algorithm's own sensitivity to fp32 input under a third of TOL.  With offsets five times as large (150 .. 200 rad, 1.5e-5 .. 3e-5
rad) the oracle fed its own input rounded to fp32 moved by up to 7e-6 in steady state, and by 5e-5 in front of a late first wrap.

A stereo block as long as the call instead of nf CANNOT be told apart by any row here (the pilot loop drops out in its first block and the
group queue never holds two groups): tests/test_receiver_frames_host.py says so in a test of its own.

NOT covered: frames whose super-frame is too long to test (65535 under a narrow band-pass: lcm(65535, 1024) demodulator-rate samples), and
the 8192-point band-pass under the tail.
"""
from collections import namedtuple
import functools
from math import gcd

import numpy as np

from tests import rds_cases as RC
from tests import rds_signal as rs
from tests import tail_cases as TC
from tests.demod_cases import chunk_bounds, rel_rms  # noqa: F401
from tests.signals import lcg_noise
from tests.test_parity_gpu import TOL, TOL_AGC_STARTUP

CHUNK = 512
RS_CHUNK = 256            # k_resample's block
WFM_CHUNK = 1024          # kWfmOutB
FMN_SKIP = 2048           # outputs of an FMN channel's acquisition that are not compared (tail_cases: the stream's first super-frame of 2048)
MODE = dict(TC.MODE, FMM=3, FMS=4)
WFM_LX_256K = 593         # L4 + Llp at 256 000 (asserted by the CPU tier against demod_cases.wfm_design)


def lcm(a, b):
    return a * b // gcd(a, b)


# ------------------------------------------------------------------------------------------------
# narrow rows
# ------------------------------------------------------------------------------------------------
# mode; fc: mixer frequency; off: the carrier sits fc + off; sig: tail_cases' signal tuple; agc: (mode, threshold) or None; key: None or
# one 0 / 1 per super-frame (tail_cases.LO / HI); squelch: dB or None
NChan = namedtuple("NChan", "mode fc off sig agc key squelch")
# total: the decimation in front (1: none); rate: demodulator rate; L: the band-pass's block; spf: demodulator-rate samples per super-frame;
# release: the blocks the band-pass releases at the end of each demodulator-rate frame of one super-frame (the `why`, asserted by the CPU tier)
NRow = namedtuple("NRow", "name fs nf fft taps bins audio_rate total rate chans calls release seed noise why")


def _nrow(name, fs, nf, fft, taps, chans, calls, release, seed, why, bins=0, audio_rate=0, total=16, noise=1e-4):
    return NRow(name, fs, nf, fft, taps, bins, audio_rate, total, fs // total, chans, calls, release, seed, noise, why)


def _fmn(fc, off, fm=800.0, beta=2.0):
    return NChan("FMN", fc, off, ("fm", fm, beta), None, None, None)


def _am(fc, f1=700.0, f2=1900.0, ph=0.4, agc=None, key=None, squelch=None):
    return NChan("AM", fc, 0.0, ("am", f1, f2, ph), agc, key, squelch)


def _sam(fc):
    return NChan("SAM", fc, 0.0, ("am", 900.0, 2100.0, 0.2), None, None, None)


def _usb(fc, agc=None):
    return NChan("USB", fc, 0.0, ("tones", 1100.0, 2300.0), agc, None, None)


GATE_KEY = TC.GATE_KEYS[1]     # closed where the stream starts: the AGC behind it first runs on a band-pass that has filled
GATE_THR = -44.0               # midway between the keyed levels as the oracle's fdEstimate reads them at 512-sample frames in 2048 bins (CPU tier)

NARROW = [
    _nrow("n-512", 1024000, 512, 2048, 1025,
          [_fmn(-400e3, 400.0), _am(-150e3), _sam(100e3), _usb(350e3, (TC.AGC_MED, 30))], (1, 2, 1, 3), (0, 1), 51,
          "a frame releases nothing, then one block (1024 every second frame); blk_frame < blk_len: NFM wraps at every block"),
    _nrow("n-1536", 1024000, 1536, 2048, 1025, [_fmn(-300e3, 200.0), _sam(200e3)], (1, 2), (1, 2), 52,
          "releases alternate 1024, 2048; one wrap per frame, none inside the double release"),
    _nrow("n-3072", 1024000, 3072, 2048, 1025, [_fmn(-300e3, 130.0), _usb(200e3)], (1, 2), (3,), 53,
          "three blocks per frame, one processBlock"),
    _nrow("n-2048-t257", 1024000, 2048, 2048, 257, [_fmn(-300e3, 110.0), _am(200e3)], (1, 1), (1, 1, 1, 1, 1, 1, 2), 54,
          "L = 1792: six frames release one block, the seventh two (3584) in one processBlock: the rule's p + blk_len == frame end edge"),
    _nrow("n-4096-f4096", 1024000, 4096, 4096, 2049, [_fmn(-300e3, 100.0), _sam(200e3)], (1, 2), (2,), 55,
          "the 4096-point band-pass under the tail, two blocks per frame"),
    _nrow("n-300-48k", 48000, 300, 2048, 1025, [_fmn(-15e3, 300.0), _am(0.0), _usb(12e3)], (1, 2), None, 56,
          "a frame that is no power of two and does not divide L, k_fastfir_t128_mix in front; 48000 / 11025 = 640 / 147 puts an output time "
          "on a whole sample every 147 outputs, so the resampler's count per call follows the partition of its time sum: the 75 blocks of "
          "1024 the reference's frames release per super-frame (235 or 236 outputs each), not 256 frames of 300", audio_rate=11025, total=1),
    _nrow("n-512-gate", 1024000, 512, 2048, 1025,
          [_am(-150e3, agc=(TC.AGC_FAST, 20), key=GATE_KEY, squelch=GATE_THR), _usb(350e3)], TC.GATE_CALLS, (0, 1), 57,
          "superframe / nf = 32 raw frames per super-frame; the gate reads the last of them, zero-padded k_spectrum_any", bins=2048, noise=1e-5),
]
NARROW_BY_NAME = {r.name: r for r in NARROW}


def n_block(row):
    return row.fft - row.taps + 1


def n_spf(row):
    return lcm(row.nf, n_block(row))


def n_superframe(row):
    return row.total * n_spf(row)


def expected_release(row):
    """blocks released at the end of each demodulator-rate frame of a super-frame: floor((k + 1) nf / L) - floor(k nf / L)"""
    L, nf = n_block(row), row.nf
    return [((k + 1) * nf) // L - (k * nf) // L for k in range(n_spf(row) // nf)]


def wrap_points(row, n):
    """k_pll_demod's rule restated: over n demodulator-rate samples from a super-frame border, the positions p (multiples of the block) at
    which the phase is wrapped: those released by a frame that ends before the next block is full, ceil(p / nf) nf < p + L"""
    L, nf = n_block(row), row.nf
    return [p for p in range(L, n + 1, L) if -(-p // nf) * nf < p + L]


def fmn_first_compared(row):
    """the first wrap at or behind FMN_SKIP outputs: the acquisition's run-up leaves the float phase in the hundreds until a wrap takes it
    down, and until then it resolves 3e-5 rad and more (tail_cases.chunk_bar); the chunk behind that wrap is the one held to TOL_NFM_WRAP"""
    return min(p for p in wrap_points(row, FMN_SKIP + 2 * n_spf(row)) if p >= FMN_SKIP)


@functools.lru_cache(maxsize=None)
def n_input(name):
    row = NARROW_BY_NAME[name]
    sf = n_superframe(row)
    n = sum(row.calls) * sf
    t = np.arange(n) / float(row.fs)
    x = lcg_noise(n, row.seed, row.noise)
    for ch in row.chans:
        level = TC.HI if ch.key is None else np.repeat(np.where(np.asarray(ch.key) > 0, TC.HI, TC.LO), sf)
        x = x + TC._carrier(ch.sig, ch.fc + ch.off, t, level)
    x.setflags(write=False)
    return x


def n_calls(row):
    """[(first input sample, input samples)] of every call"""
    sf, out, at = n_superframe(row), [], 0
    for k in row.calls:
        out.append((at * sf, k * sf))
        at += k
    return out


def n_oracle_receiver(O, row, c, resample=True):
    ch = row.chans[c]
    r = O.Receiver(row.fs, row.nf, row.bins, row.fft, row.taps)
    r.set_mode(MODE[ch.mode]); r.set_mixer(ch.fc); r.set_filter(*TC.BAND[ch.mode])
    if ch.agc is not None:
        r.set_agc(*ch.agc)
    if row.audio_rate and resample:
        r.set_audio_rate(row.audio_rate)
    if ch.squelch is not None:
        r.set_squelch(ch.squelch)
    return r


_N_CACHE = {}


def n_oracle(O, name, c, resample=True):
    """-> (per call: the audio the Receiver delivered, concatenated; per call: per super-frame whether it delivered anything;
    the outputs of every frame of the stream).  resample = False: the row's receiver without its audio_rate"""
    if (name, c, resample) not in _N_CACHE:
        row = NARROW_BY_NAME[name]
        x, r, sf = n_input(name), n_oracle_receiver(O, row, c, resample), n_superframe(row)
        calls, opened, lens = [], [], []
        for o, n in n_calls(row):
            parts, op = [], []
            for s in range(o, o + n, sf):
                fr = [r.process(x[i:i + row.nf], want_spectrum=bool(row.bins))[0] for i in range(s, s + sf, row.nf)]
                lens += [len(a) for a in fr]
                op.append(any(len(a) for a in fr))
                parts += fr
            calls.append(np.concatenate(parts)); opened.append(op)
        _N_CACHE[(name, c, resample)] = (calls, opened, lens)
    return _N_CACHE[(name, c, resample)]


# ------------------------------------------------------------------------------------------------
# a plain model of the LIBRARY's partition of a call, from the oracle's parts -- and the wrong models, each one change to it
# ------------------------------------------------------------------------------------------------
WRAP_MODELS = ("every_nf", "every_block", "call_end")


def model_wraps(row, n, wrong=None):
    """where the model wraps Demod_NFM's phase inside a call of n demodulator-rate samples (the call's end always wraps).  None: k_pll_demod's
    rule; "every_nf": every nf samples; "every_block": at every block of the band-pass; "call_end": at the call's end only"""
    L, nf = n_block(row), row.nf
    if wrong is None:
        w = wrap_points(row, n)
    elif wrong == "every_nf":
        w = list(range(nf, n + 1, nf))
    elif wrong == "every_block":
        w = list(range(L, n + 1, L))
    else:
        assert wrong == "call_end"
        w = []
    return sorted(set(w) | {n})


def n_model(O, name, c, wrong=None, floor_seed=None, resample=True, rs_partition="released"):
    """oracle.Mixer -> Decimator -> gain -> FastFIR over each whole call, the AGC and the demodulator once per call -- Demod_NFM in pieces that
    end where model_wraps says -- and, with an audio_rate, the resampler over the whole call in the parts resampler_parts names
    (ResampCore's partition).  Never-gated channels only.  floor_seed: white noise of tail_cases.FLOOR rms on I and on Q added behind the
    band-pass, what the fp32 overlap-save leaves there.  -> per call the audio"""
    row = NARROW_BY_NAME[name]
    ch, x = row.chans[c], n_input(name)
    assert ch.key is None and ch.squelch is None
    mixer = O.Mixer(row.fs); mixer.set_frequency(ch.fc)
    dec = O.Decimator(row.fs, 30000)
    gain = 10 ** ((dec.dec_by2_stages * 2) / 20.0)                  # receiver.cpp:935-938
    bp = O.FastFIR(row.fft, row.taps)
    lo, hi = TC.BAND[ch.mode]
    bp.setup(np.float32(lo), np.float32(hi), 0, float(row.rate))
    agc = None
    if ch.agc is not None:
        agc = O.Agc(row.rate); agc.set_mode(*ch.agc)
    dem = {"AM": O.DemodAM, "SAM": O.DemodSAM, "FMN": O.DemodNFM}.get(ch.mode)
    dem = dem(row.rate) if dem else None
    if ch.mode == "AM":
        dem.set_bandwidth(hi - lo)
    rs_ = O.Resampler(row.nf + row.fft) if (row.audio_rate and resample) else None
    out = []
    for k, (o, n) in enumerate(n_calls(row)):
        y = bp.process(dec.process(mixer.process(x[o:o + n])) * gain)
        assert len(y) == n // row.total, (len(y), n)
        if floor_seed is not None:
            y = y + lcg_noise(len(y), 1000 * floor_seed + k, TC.FLOOR * 12 ** 0.5)
        if agc is not None:
            y = agc.process(y)
        if ch.mode == "FMN":
            at, parts = 0, []
            for w in model_wraps(row, len(y), wrong):
                parts.append(dem.process(y[at:w])); at = w
            y = np.concatenate(parts)
        elif dem is not None:
            y = dem.process(y)
        if rs_ is not None:
            parts, at = [], 0
            while at < len(y):
                for ln in resampler_parts(row, rs_partition):
                    parts.append(rs_.process(y[at:at + ln], row.rate / float(row.audio_rate))); at += ln
            assert at == len(y)
            y = np.concatenate(parts)
        out.append(y)
    return out


def resampler_parts(row, partition="released"):
    """the lengths ResampCore takes off its running time sum over one super-frame.  "released": what each reference frame released (the
    non-empty entries of expected_release, in blocks): Receiver::init's rule; "frames": frames of nf, the partition the library had"""
    if partition == "frames":
        return [row.nf] * (n_spf(row) // row.nf)
    return [r * n_block(row) for r in expected_release(row) if r]


def n_bar(ch):
    bar = TOL
    if ch.agc is not None and ch.agc[0] != TC.AGC_OFF:
        bar = max(bar, TOL_AGC_STARTUP)
    if ch.mode == "SAM":
        bar = max(bar, TC.TOL_SAM)
    return bar


def stream_chunks(row, c, n_out):
    """the chunks of a never-gated channel's stream of n_out outputs that are compared -> [(lo, hi, bar)], on stream positions.  chunk: 512,
    or 256 behind the resampler, whose stream is 1 / dt as long (positions below are scaled by it and rounded up to whole chunks)"""
    ch = row.chans[c]
    size = RS_CHUNK if row.audio_rate else CHUNK
    scale = (row.audio_rate / float(row.rate)) if row.audio_rate else 1.0
    up = lambda p: -(-int(np.ceil(p * scale)) // size) * size  # noqa: E731
    bar = n_bar(ch)
    b = [(lo, hi, bar) for lo, hi in chunk_bounds(n_out, size)]
    running = ch.agc is not None and ch.agc[0] != TC.AGC_OFF
    if ch.mode == "FMN":
        skip = up(fmn_first_compared(row))
        b = [(lo, hi, TC.TOL_NFM_WRAP if lo == skip else v) for lo, hi, v in b if lo >= skip]
    elif running:       # chunk 0: zeros of the 960-sample delay line; the chunk that holds its end joins the one behind it
        assert row.taps == 1025
        j = up(TC.AGC_DELAY) // size - 1
        b = b[:j] + [(b[j][0], b[j + 1][1], bar)] + b[j + 2:]
    else:
        j = joined_at_start(row, ch)
        if j:   # the first j chunks are joined to the one behind them
            b = [(0, b[j][1], bar)] + b[j + 1:]
    return b


def joined_at_start(row, ch):
    """how many chunks of 512 outputs at the stream's start are joined to the chunk behind them.  The band-pass's response rises over its
    first (taps - 1) / 2 outputs (512 of the stock 1025 taps, 1024 of 2049, 128 of 257), and what it delivers before lies under the fp32
    floor of the overlap-save block it comes from.  AM loses its bar on every chunk inside that rise; SAM (at 1e-4) and USB hold it on the
    last of them (tail_cases.compared_chunks: the stock sizes, where that leaves AM's chunk 0 joined and SAM's and USB's compared).  The CPU
    tier holds this to what the oracle's own parts do under that floor."""
    per_chunk = CHUNK if not row.audio_rate else RS_CHUNK * row.rate / float(row.audio_rate)   # demodulator-rate samples a chunk covers
    rise = int(((row.taps - 1) // 2) / per_chunk)      # (behind the resampler a chunk of 256 outputs covers the rise and as much again: none)
    return rise if ch.mode == "AM" else max(rise - 1, 0)


def form(ch, a):
    return TC.sam_form(a) if ch.mode == "SAM" else np.asarray(a)


# ------------------------------------------------------------------------------------------------
# WFM rows
# ------------------------------------------------------------------------------------------------
# chans: (mode, (f1, f2) audio tones of the channel's own FM signal); shared: one stream for all channels (the dmFMS rows: a broadcast multiplex)
WRow = namedtuple("WRow", "name fs nf total chans calls fc seed why")


def fms_edge_nf(rate):
    """the smallest frame a dmFMS receiver at this demodulator rate accepts (RdsCore::check_frame with the in-place rule), from the design program"""
    des = RC.rds_design(float(rate))
    D = 1 << len(des.stages)
    nf = D
    while fms_verdict(rate, nf) is not None:
        nf += D
    return nf


def fms_verdict(rate, nf):
    """RdsCore::check_frame(nf, true) restated over design::rds_design's chain -> None (accepted) or the reason"""
    des = RC.rds_design(float(rate))
    D = 1 << len(des.stages)
    if nf % D:
        return "not a multiple of D"
    for j, (design, T) in enumerate(zip(des.stages, des.stage_taps)):
        if (nf >> j) < T:
            return "stage shorter than its taps"
    for j, (design, T) in enumerate(zip(des.stages, des.stage_taps)):
        if ((nf >> j) <= 18) if design == 1 else ((nf >> j) < 2 * (T - 1)):
            return "below 2 (T - 1)"
    return None


_TONES = ((1000.0, 3300.0), (700.0, 5200.0), (2400.0, 9100.0))


@functools.lru_cache(maxsize=None)
def wfm_rows():
    return [
        WRow("w-256", 256000, 256, 1, [("FMM", _TONES[0]), ("FMM", _TONES[1]), ("FMM", _TONES[2])], (1, 2, 3, 1, 2), 20e3, 61,
             "256 and 512 are below Lx = 593: the history merge (hipMemcpy2DAsync pair) over three rows; 768 is above it: the tail job is "
             "carried by the launch; short after long, and long after short"),
        WRow("w-600", 256000, 600, 1, [("FMM", _TONES[0]), ("FMM", _TONES[1])], (1, 1, 2), 20e3, 62, "seven samples over Lx"),
        WRow("w-65535", 256000, 65535, 1, [("FMM", _TONES[0])], (1, 1), 20e3, 63, "the largest frame, and odd: 64 workgroups, the last one output short"),
        WRow("w-dec-512", 1024000, 512, 4, [("FMM", _TONES[0]), ("FMM", _TONES[1])], (1, 3, 2), 250e3, 64,
             "a decimator in front delivering 512 outputs per super-frame, below Lx at 1"),
        WRow("w-1024-fms", 256000, 1024, 1, [("FMS", None), ("FMM", None)], (1, 2, 3), 10e3, 65,
             "stereo_block = 1024: one to three pilot / RDS blocks per call, the group queue polled once per 1024; at least ten groups"),
        WRow("w-384k-fms", 384000, fms_edge_nf(384000), 1, [("FMS", None)], (1, 2), 20e3, 66,
             "the accepted edge of the size rule at the four-stage chain (11, 15, 23, 51 taps), rds_cases.A_LEVELS' 384 000 levels"),
    ]


def w_shared(row):
    return row.chans[0][0] == "FMS"


FMS_GROUPS = 18
# w-256: the deviation drops to W_QUIET_LEVEL during the call of 256 behind the call of 768 and during the call of 512 behind that one
# (demod_cases.WFM_QUIET_CALLS' reasoning: a short call leaves [end of the old history | its input] as history, and what a wrong merge
# loses is the old part, 256 and more samples back, where the folded response has almost ended: with these calls quiet and the samples in
# front of them loud, the last call's first outputs are little else than the response to that part)
W_QUIET = {"w-256": (3, 4)}
W_QUIET_LEVEL = 0.015


@functools.lru_cache(maxsize=None)
def w_input(name):
    """-> (x [streams, n], [(offset, n)] of the calls)"""
    row = {r.name: r for r in wfm_rows()}[name]
    sf = row.total * row.nf
    if w_shared(row):
        n = int(row.fs * (FMS_GROUPS * 104 + 60) / 1187.5)
        cyc = sum(row.calls) * sf
        n -= n % cyc
        reps = n // cyc
        t = np.arange(n) / float(row.fs)
        x = rs.fm_multiplex(rs.make_groups(FMS_GROUPS, seed=row.seed), float(row.fs), n, subcarrier_offset_hz=-14.0, **RC.A_LEVELS.get(row.fs, {})) \
            * np.exp(2j * np.pi * row.fc * t)
        x = x[None, :]
    else:
        reps = 1
        n = sum(row.calls) * sf
        t = np.arange(n) / float(row.fs)
        level, at = np.ones(n), 0
        for k, m in enumerate(row.calls):
            if k in W_QUIET.get(name, ()):
                level[at:at + m * sf] = W_QUIET_LEVEL
            at += m * sf
        xs = []
        for c, (_, (f1, f2)) in enumerate(row.chans):
            f = level * 60000.0 * (np.cos(2 * np.pi * f1 * t + 0.9 + c) + 0.3 * np.cos(2 * np.pi * f2 * t + 0.2))
            xs.append(0.5 * np.exp(1j * (2 * np.pi * np.cumsum(f) / row.fs + 2 * np.pi * row.fc * t)) + lcg_noise(n, row.seed + 10 * c, 1e-4))
        x = np.array(xs)
    calls, at = [], 0
    for _ in range(reps):
        for k in row.calls:
            calls.append((at, k * sf)); at += k * sf
    assert at == x.shape[1]
    x.setflags(write=False)
    return x, calls


_W_CACHE = {}


def w_oracle(O, name, c):
    """oracle.Receiver fed frame by frame -> (per call the audio delivered, (groups, changed) polled over the whole script)"""
    if (name, c) not in _W_CACHE:
        row = {r.name: r for r in wfm_rows()}[name]
        x, calls = w_input(name)
        xs = x[0 if w_shared(row) else c]
        r = O.Receiver(row.fs, row.nf, 0)
        r.set_mode(MODE[row.chans[c][0]]); r.set_mixer(row.fc)
        out = []
        for o, n in calls:
            out.append(np.concatenate([r.process(xs[i:i + row.nf], want_spectrum=False)[0] for i in range(o, o + n, row.nf)]))
        _W_CACHE[(name, c)] = (out, r.rds_polled() if row.chans[c][0] == "FMS" else None)
    return _W_CACHE[(name, c)]


# ------------------------------------------------------------------------------------------------
# refusal rows: (fs, nf, reason) -- a WFM receiver without a decimator whose set_mode(FMS) is refused with the size code
# ------------------------------------------------------------------------------------------------
REFUSALS = [
    (256000, 300, "not a multiple of D"),
    (384000, 256, "stage shorter than its taps"),
    (384000, 512, "below 2 (T - 1)"),
    (256000, 256, "below 2 (T - 1)"),          # 64 < 68 at the 35-tap stage
]
VERDICT_FRAMES = (256, 300, 512, 600, 768, 1024, 2048)


_L_CACHE = {}


def w_locks(O, name, with_audio=False):
    """the pilot's lock flag after the last frame of every call of a dmFMS row: oracle.Mixer and oracle.DemodWFM frame by frame, which a
    Receiver without a decimator is (oracle.Receiver does not hand the flag out; the CPU tier holds this chain's audio to the Receiver's,
    bit for bit) -> [bool], or ([bool], the audio per call)"""
    if name not in _L_CACHE:
        row = {r.name: r for r in wfm_rows()}[name]
        assert row.total == 1 and row.chans[0][0] == "FMS"
        x, calls = w_input(name)
        m, d = O.Mixer(row.fs), O.DemodWFM(float(row.fs))
        m.set_frequency(row.fc)
        locks, audio = [], []
        for o, n in calls:
            parts = []
            for i in range(o, o + n, row.nf):
                a, lk = d.process_stereo(m.process(x[0, i:i + row.nf]))
                parts.append(a)
            locks.append(bool(lk)); audio.append(np.concatenate(parts))
        _L_CACHE[name] = (locks, audio)
    return _L_CACHE[name] if with_audio else _L_CACHE[name][0]


# ------------------------------------------------------------------------------------------------
# the CDownConvert step at calls of a few samples: a plain fp64 streaming model
# ------------------------------------------------------------------------------------------------
DC_STEP = (2048000.0, 15000.0, 0.11 * 2048000.0, (11, 11, 15, 19, 31))     # rate, bandwidth, tuned frequency, the chain's taps (D = 32)

_DC_PROGRAM = r'''
#include <cstdio>
#include "design.h"
using namespace pg::design;
int main()
{
    double rate, bw;
    int simple;
    while (std::scanf("%lf %lf %d", &rate, &bw, &simple) == 3) {
        const DcChain c = downconvert_chain(rate, bw, simple != 0);
        for (int s : c.stages) {
            const std::vector<double> h = downconvert_stage_response(s);
            std::printf("stage %d", s);
            for (double v : h) std::printf(" %.17g", v);
            std::printf("\n");
        }
        double amp[1024];
        oscillator_amplitudes(amp, 1024);
        std::printf("amp 0");
        for (int i = 0; i < 1024; i++) std::printf(" %.17g", amp[i]);
        std::printf("\n");
    }
    return 0;
}
'''


@functools.lru_cache(maxsize=None)
def dc_design(rate, bw, simple=False):
    """design::downconvert_chain's stages (the taps each applies, oldest sample first) and design::oscillator_amplitudes, asked with g++
    as rds_cases asks for its designs -> ([h per stage], amp[1024])"""
    import atexit, os, shutil, subprocess, tempfile
    d = tempfile.mkdtemp(prefix="dc_design_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "dc_design.cpp"), os.path.join(d, "dc_design")
    with open(src, "w") as f:
        f.write(_DC_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + RC.CSRC, src, os.path.join(RC.CSRC, "design.cpp"), "-o", exe])
    lines = subprocess.run([exe], input=("%.17g %.17g %d\n" % (rate, bw, int(simple))).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    stages = [np.array([float(v) for v in ln.split()[2:]]) for ln in lines if ln.startswith("stage")]
    amp = [np.array([float(v) for v in ln.split()[2:]]) for ln in lines if ln.startswith("amp")][0]
    return stages, amp


def dc_step_calls():
    return [32, 64, 96] + [32] * 40 + [32]


@functools.lru_cache(maxsize=None)
def dc_step_input():
    fs, _, f0, _ = DC_STEP
    n = sum(dc_step_calls())
    t = np.arange(n) / fs
    x = 0.3 * np.exp(2j * np.pi * (f0 + 0.02 * fs / 32) * t) + 0.2 * np.exp(2j * np.pi * (f0 - 0.05 * fs / 32) * t + 0.5j) \
        + 0.3 * np.exp(2j * np.pi * (f0 + 0.37 * fs) * t) + lcg_noise(n, 4, 1e-3)
    x = x.astype(np.complex64).astype(np.complex128)     # both sides are handed the same single-precision samples, the step's upload format
    x.setflags(write=False)
    return x


def downconvert_model(fs, bw, f0, x):
    """CDownConvert::ProcessData over the whole stream at once, zero history in front: the oscillator in closed form (tests/rds_ref.py: the
    angle of the rounded (cos, sin) pair times the sample count, the length from design::oscillator_amplitudes), the product, and every
    decimate-by-2 stage as a strided FIR, output m from the inputs 2 m - (T - 1) .. 2 m"""
    stages, amp = dc_design(fs, bw)
    inc = 6.28318530717958647692528676656 * (-f0) / fs        # CDownConvert::SetFrequency negates (downconvert.cpp:100-112)
    inc_eff = np.arctan2(np.longdouble(np.sin(inc)), np.longdouble(np.cos(inc)))
    m = np.arange(len(x))
    ph = (m + 1).astype(np.longdouble) * inc_eff
    z = np.asarray(x, dtype=np.complex128) * (amp[np.minimum(m, len(amp) - 1)] * (np.cos(ph).astype(np.float64) + 1j * np.sin(ph).astype(np.float64)))
    for h in stages:
        T = len(h)
        full = np.convolve(np.concatenate([np.zeros(T - 1, dtype=np.complex128), z]), h[::-1])
        z = full[T - 1:T - 1 + len(z):2]
    return z
