"""The coverage statement for a receiver's input conditioners (pebblegpu_set_conditioners): DCRemoval, IQBalance, NB1 and NB2 as
ConditionCore runs them on a conditioned call (csrc/cores.hip: set / apply / run) -- a copy of all S streams at pitch `cap` (the handle's
capacity, not the call's n), k_iir_scan<0,1> over a host-rebuilt d_dc_list, k_iq_balance with one lane per (stream, frame of nf),
k_noise_blank with one lane per stream in cdiv(S, 64) workgroups, NbState carried from call to call and edited by the setter -- and the
route such a call takes (csrc/call_route.h: no side, no bank_pipe, no plain, no raw_fused while a flag is on or a change is pending).
Their arithmetic is pinned elsewhere (tests/test_reference_pins.py: nb1, nb2, iqbalance, dcremoval_*); the rows here pin their INDEXING,
their STATE HANDLING and what the rest of the call READS.

One table of rows, their inputs, the oracle driver and the deliberately wrong models, used by the CPU tier
(tests/test_receiver_conditioners_host.py: the rows are well formed and reach what their "why" says, the margin condition holds, every call
plans the route the table names, every wrong model misses the new comparison by a factor of WRONG_FACTOR or more, and the factor by which
it moves the OLD observables is recorded) and by the GPU tier (tests/test_receiver_conditioners_gpu.py: the same rows through
P.ReceiverBank, pebblegpu_receiver_conditioned() against the oracle chain sample by sample).

The oracle: one Chain per stream (tests/test_streambank_conditioners_host.py: Iir("hp", 10, 0.7071, fs), iq_balance per frame of nf,
NoiseBlanker with enable on the off -> on transition), restated here as Model, which is Chain when no wrong model is asked for (the CPU
tier holds the two to the same bits) and oracle.Receiver.set_conditioners for audio and spectrum.  The margin condition (assert_margin,
MARGIN) is the stream bank's: it is a condition on the INPUT.  The receivers' k_noise_blank rounds as the reference does, step by step, but
its input is the float the stage before it stored, where the oracle carries doubles: a decision within that rounding could fall the other
way, so the rows leave every decision the same room.

Inputs: the `spiky` recipe (tones 0.05 and 0.02, LCG noise 1e-3, DC 0.01) with another seed, tone and level per stream, spikes at -3, +2
and +5 around EVERY call boundary and EVERY frame boundary of the row's call script and a run of 40 consecutive spikes across one call
boundary.  One deviation, found by the wrong models: with the spike at -3 in front of every call boundary NB1 blanks the first four
outputs of every call, and those are the only outputs that show the two samples its delay line carried over.  So the streams listed in
Row.quiet leave the -3 spike out at CALL boundaries (frame boundaries keep all three); the other NB1 stream of the row keeps it and shows
the carried count.  Seeds are picked on the CPU so that the margin condition holds; the ones that do not are noted at the rows.

All rows but `wfm` run at 1 024 000 samples/s (the rate of tests/tail_cases.py): four stages, D = 16, a super-frame of 32 768 samples = 16
frames of 2048 (65 536 = 16 frames of 4096 for `frame4096`), 2048 outputs each.  Every channel is USB 300 .. 3000 Hz (no AGC: TOL is the
only audio bar), its mixer 1 kHz under its stream's 0.05 tone.

NOT covered, and why:
  - The environment-switch routes (PEBBLEGPU_PIPELINE, PEBBLEGPU_FUSE_DEC, PEBBLEGPU_BANK_PIPELINE ...): no row sets a switch.  A
    conditioned call plans side = plain = fuse_dec = 0 whatever they say (call_route.h; tests/test_call_route_host.py holds that).
  - pebblegpu_process_iq: refused while a conditioner is on or pending (the GPU tier checks the refusal, and that conditioned() is NULL
    behind it).
  - The multibank: its shards are receivers, reached through pebblegpu_multibank_shard; nothing of the conditioners is its own.
  - Which STREAM a call's kernels run on: pebblegpu_receiver_kernel_name names kernels, not streams.  The `two_stage` row holds the route
    facts on the CPU (bank_pipe and plain before the change and after it) and the results on the GPU (calls 0-1 bit for bit a twin that
    was never given a conditioner, every call against the oracle).
  - A blanker decision closer to its threshold than MARGIN: a condition on the input, see above.
"""
from collections import namedtuple
import functools

import numpy as np

from tests.demod_cases import chunk_errors
from tests.signals import lcg_noise, tones
from tests.test_parity_gpu import TOL, TOL_DB, db_err, rel_rms
from tests.test_streambank_conditioners_host import MARGIN, Chain, assert_margin, smallest_margin, spiky  # noqa: F401  (part of this module's interface)

FS, FRAME, SF, D = 1024000, 2048, 32768, 16
WFM_FS, WFM_SF, WFM_D = 20000000, 131072, 64
CHUNK = 512
WRONG_FACTOR = 100          # tests/tail_cases.py WRONG_FACTOR, tests/raw_cases.py MARGIN: the project's own
BAND = (300.0, 3000.0)
RAW_FMT, RAW_GAIN = 2, 4.0  # int16 pairs, I then Q; a power-of-two gain (tests/raw_cases.py on gains)
SPIKE_OFFS, SPIKE_AMPS = (-3, 2, 5), (1.5, -3.0, 2.0j)

# script: [(call, stream, flags, iq_gain, iq_phase)] setter calls issued before that call, in order.  levels: the input's level per call.
# quiet: streams whose input leaves the -3 spike out at call boundaries (module docstring).  kind: what else the row switches on.
Row = namedtuple("Row", "name fs nf sf S C shared wfm bins hires max_sf calls script levels seed quiet kind why")

GAINS6 = [1.0, 1.01, 1.02, 0.97, 1.03, 1.05]
PHASES6 = [0.0, 0.01, 0.03, -0.02, 0.02, 0.01]
LISTS_S = 66                 # the handle takes any channel count: 66 as asked
LISTS_FLAGS0 = {0: 12, 1: 3, 63: 6, 64: 15, 65: 9}
GEN_SWEEP = (-0.25e6, 0.3e6, 23456789.0, 0.03)   # start, stop, Hz per second, amplitude (mixed into the input)
GEN_NOISE = (0.002, 77)
GATE_UPS = 100               # a spectrum every 10 ms: every fifth frame of 2 ms


def _row(name, S, calls, script, why, C=None, shared=False, bins=2048, hires=0, max_sf=None, levels=None, seed=0, quiet=(), kind=None,
         fs=FS, nf=FRAME, sf=SF, wfm=False):
    return Row(name, fs, nf, sf, S, S if C is None else C, shared, wfm, bins, hires, max(calls) if max_sf is None else max_sf, tuple(calls), script,
               tuple(levels) if levels else (1.0,) * len(calls), seed, tuple(quiet), kind, why)


def _all(call, flags, gains=None, phases=None):
    return [(call, s, f, (gains or GAINS6)[s % 6], (phases or PHASES6)[s % 6]) for s, f in enumerate(flags)]


ROWS = {r.name: r for r in (
    _row("flags", 6, (1, 2, 1, 3), _all(0, [0, 1, 2, 4, 8, 15]), "every stage alone and together; three of four calls have n < cap", max_sf=3, seed=200, quiet=(3,)),
    _row("lists", LISTS_S, (1, 1), [(0, s, f, GAINS6[s % 6], PHASES6[s % 6]) for s, f in sorted(LISTS_FLAGS0.items())] +
         [(1, 1, 2, GAINS6[1], PHASES6[1]), (1, 63, 7, GAINS6[3], PHASES6[3])],
         "66 streams: k_noise_blank's second workgroup; DC list {1, 64, 65} then {63, 64, 65}: positions are not ids, the list is rebuilt, a DC state sleeps and another starts",
         seed=301),   # (seed 300 misses the margin condition on stream 64: 4.5e-6)
    _row("frame4096", 2, (1, 2), _all(0, [2, 15], GAINS6[2:], PHASES6[2:]), "k_iq_balance restarts per nf = 4096", nf=4096, sf=65536, bins=4096, seed=400),
    _row("switching", 2, (1, 1, 1, 1, 1), _all(0, [15, 13]) + _all(1, [0, 1]) + _all(2, [15, 15]) + _all(3, [15, 15], [0.95, 1.04], [0.02, -0.03]) + _all(4, [3, 0]),
         "blanker reset on off -> on only; a setter call with the flag already on; DC and IQ off and on; a gain change; NB1's delay line and count across calls",
         levels=(1.0, 0.5, 2.0, 1.0, 1.0), seed=500, quiet=(1,)),
    _row("negative_gain", 2, (1, 1), [(0, 0, 2, -0.97, 0.02), (0, 1, 15, -0.97, 0.02)], "a negative iq_gain with the flag on is applied, not taken for 'off'", seed=600),
    _row("two_stage", 1, (1,) * 6, [(2, 0, 15, 1.02, 0.03), (3, 0, 0, 1.0, 0.0)], "bank_pipe / plain -> conditioned -> cond_dirty -> two-stage again, without a display transform",
         C=3, shared=True, bins=0, seed=700),
    _row("raw", 3, (1, 2, 1), _all(0, [15, 0, 5]), "int16 process_raw: the staged conversion, then the copy at cap, with S > 1", max_sf=2, seed=800, quiet=(2,), kind="raw"),
    _row("generator", 1, (1, 2), [(0, 0, 15, 1.02, 0.03)], "the copy is taken from the generator's staging buffer", seed=900, kind="generator"),
    _row("gated", 2, (1, 2), _all(0, [5, 5]), "set_spectrum_updates on: run_list reads pitch cap", max_sf=3, seed=1000, kind="gated"),
    _row("downstream", 1, (1, 2), [(0, 0, 1, 1.0, 0.0)], "the zoomed transform, the S-meter and the chain all read the conditioned rows", hires=2048, seed=1100, kind="downstream"),
    _row("recording", 1, (1, 2), [(0, 0, 15, 1.02, 0.03)], "the ring records the unconditioned input; conditioned() is not that", levels=(0.25, 0.25), seed=1200,
         kind="recording"),
    _row("wfm", 1, (1, 2), [(0, 0, 15, 1.02, 0.03)], "20 Msps WFM, the rate of tests/test_conditioners_gpu.py, with the sample-exact view", fs=WFM_FS, sf=WFM_SF, wfm=True,
         bins=8192, seed=1300),
)}


# ------------------------------------------------------------------------------------------------
# scripts and inputs
# ------------------------------------------------------------------------------------------------
def call_bounds(row):
    """[(first sample, samples)] of every call"""
    out, at = [], 0
    for k in row.calls:
        out.append((at, k * row.sf))
        at += k * row.sf
    return out


def total(row):
    return sum(row.calls) * row.sf


def setters_before(row, k):
    return [(s, f, g, p) for c, s, f, g, p in row.script if c == k]


def flags_during(row):
    """[call][stream] -> the flags in force"""
    cur, out = [0] * row.S, []
    for k in range(len(row.calls)):
        for s, f, _, _ in setters_before(row, k):
            cur[s] = f
        out.append(list(cur))
    return out


def dc_list(row, k):
    return [s for s, f in enumerate(flags_during(row)[k]) if f & 1]


def tone_of(row, s):
    if row.kind == "downstream":
        return 2500.0
    return row.fs * (0.0493 + 0.0034 * s)


def mixer_of(row, c):
    """channel c's centre: 1 kHz under the 0.05 tone of its stream (shared input: the one stream's two tones and a third place)"""
    if row.wfm:
        return 1.0e6
    if row.kind == "downstream":
        return 1000.0
    if row.shared:
        return [tone_of(row, 0) - 1000.0, -0.122 * row.fs - 1500.0, tone_of(row, 0) - 2200.0][c]
    return tone_of(row, c) - 1000.0


def band_of(row):
    return (-5000.0, 5000.0) if row.kind == "downstream" else BAND


def spike_positions(row, s):
    """{position: amplitude} of stream s: -3, +2, +5 around every frame and call boundary (a quiet stream: no -3 at call boundaries)"""
    n, out = total(row), {}
    calls = {lo for lo, _ in call_bounds(row)} | {n}
    for e in range(0, n + 1, row.nf):
        for off, a in zip(SPIKE_OFFS, SPIKE_AMPS):
            if off == -3 and e in calls and s in row.quiet:
                continue
            if 0 <= e + off < n:
                out[e + off] = a
    return out


def run_start(row):
    """the run of 40 consecutive spikes: from 20 samples in front of the second call"""
    return call_bounds(row)[1][0] - 20


def _stream(row, s):
    n = total(row)
    if row.wfm:     # an FM carrier in the 0.05 tone's place
        t = np.arange(n) / float(row.fs)
        x = 0.05 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + tones(row.fs, n, [(0.02, -0.122 * row.fs)]) + lcg_noise(n, row.seed, 1e-3) + 0.01
    elif row.kind == "downstream":   # stream-bank test 6: a 0.01 offset under a 0.004 tone, inside a band-pass across 0 Hz
        x = tones(row.fs, n, [(0.004, tone_of(row, s))]) + lcg_noise(n, row.seed + s, 1e-4) + 0.01
        return x
    else:
        x = tones(row.fs, n, [(0.05, tone_of(row, s)), (0.02, -0.122 * row.fs)]) + lcg_noise(n, row.seed + s, 1e-3) + 0.01
    for p, a in spike_positions(row, s).items():
        x[p] += a
    r = run_start(row)
    x[r:r + 40] += 2.0
    lev = np.repeat(np.asarray(row.levels) * (1.0 + 0.07 * (s % 5)), [m for _, m in call_bounds(row)])
    return x * lev


@functools.lru_cache(maxsize=None)
def row_raw(name):
    """the `raw` row's int16 pairs [S, n, 2]"""
    row = ROWS[name]
    x = np.stack([_stream(row, s) for s in range(row.S)])
    raw = np.round(np.stack([x.real, x.imag], axis=-1) * (32768.0 / RAW_GAIN))
    assert np.abs(raw).max() < 32767
    raw = raw.astype(np.int16)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def row_input(name):
    """complex64 [S, n]: what the device is handed (the `raw` row: what its int16 pairs convert to); the oracle gets the same floats"""
    row = ROWS[name]
    if row.kind == "raw":
        from tests.raw_cases import host_convert
        x = host_convert(row_raw(name), RAW_FMT, 0, RAW_GAIN)
    else:
        x = np.stack([_stream(row, s) for s in range(row.S)]).astype(np.complex64)
    x.setflags(write=False)
    return x


def generator_adds(row, n):
    """what the test bench's generator adds to the `generator` row's stream (tests/testbench_ref.py): the CPU tier's stand-in for the
    RAW_IQ tap the GPU tier feeds the oracle"""
    from tests import testbench_ref as R
    a, b, rate, amp = GEN_SWEEP
    ref, _ = R.serial_sweep(row.fs, n, 2048, amp, start=a, stop=b, rate=rate, sweep_type=R.REPEAT)
    return ref + GEN_NOISE[0] * R.noise(GEN_NOISE[1], 0, 0, n)[0]


@functools.lru_cache(maxsize=None)
def oracle_input(name):
    """what the conditioners see on the CPU: the input, plus the generator's restated injection on the `generator` row"""
    row = ROWS[name]
    x = row_input(name).astype(np.complex128)
    if row.kind == "generator":
        x = (x + generator_adds(row, x.shape[1])[None, :]).astype(np.complex64).astype(np.complex128)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------
# the route of every call (csrc/call_route.h)
# ------------------------------------------------------------------------------------------------
def call_facts(row, k):
    """the CallFacts the table fixes for call k, as Receiver::call_facts captures them BEFORE the call applies anything: cond_any is what
    the last call applied, cond_dirty whether a conditioner setter ran since.  What the cores can do (dec_lds_free_front, dec_raw_front,
    spec_raw_ready ...) is the device's to say: the CPU tier plans every call under all of their values"""
    fl = flags_during(row)
    two_stage_handle = not row.wfm and not row.bins   # Receiver::create: bank_pipe_ok_ (the chain has four stages at this rate)
    return dict(with_spectrum=int(bool(row.bins)), with_chain=1, raw=int(row.kind == "raw"), n=call_bounds(row)[k][1], C=row.C, S=row.S, nf=row.nf,
                zoom_bins=row.hires, wfm=int(row.wfm), bank_pipe_ok=int(two_stage_handle), dec_double_out=int(two_stage_handle),
                gated=int(row.kind == "gated"), touched=int(k == 0 or bool(setters_before(row, k))),
                cond_any=int(k > 0 and any(fl[k - 1])), cond_dirty=int(bool(setters_before(row, k))),
                generator=int(row.kind == "generator"), taps=int(row.kind == "generator"), recording=int(row.kind == "recording"))


def route_of(row, k):
    """the route fields the table names for call k"""
    f = call_facts(row, k)
    cond = f["cond_any"] or f["cond_dirty"]
    if cond:
        return dict(side=0, bank_pipe=0, plain=0, raw_fused=0, staged=int(row.kind in ("raw", "generator")))
    assert row.name == "two_stage", "only that row has calls without a conditioner on or pending"
    return dict(side=0, bank_pipe=1, plain=int(not f["touched"]), raw_fused=0, staged=0)


# ------------------------------------------------------------------------------------------------
# the oracle chain, and the wrong models: each one change to it
# ------------------------------------------------------------------------------------------------
WRONG = {
    # model: (rows it is held to, what it is)
    "iq_2048": (("frame4096",), "IQ balance restarting every 2048 samples whatever nf is"),
    "iq_carried": (("flags",), "IQ balance's adaptive terms carried from frame to frame of a call"),
    "by_position": (("lists",), "the DC state taken by list position instead of stream id"),
    "dc_zeroed": (("flags", "switching"), "the DC state zeroed at the start of every call"),
    "dc_awake": (("lists", "switching"), "the DC state advanced while its flag is off"),
    "nb1_delay_cleared": (("flags", "switching", "raw"), "NB1's delay line cleared at the start of every call"),
    "nb1_count_dropped": (("flags", "switching"), "NB1's spike count not carried across a call boundary"),
    "nb1_six": (("flags",), "NB1 blanking 6 samples"),
    "no_reset": (("switching",), "no reset when a blanker is switched on"),
    "reset_when_on": (("switching",), "a reset on every setter call with the blanker's flag on"),
    "nb2_first": (("flags", "switching"), "NB2 ahead of NB1"),
    "iq_first": (("flags", "switching"), "IQ balance ahead of DC removal"),
    "pitch_n": (("flags", "raw"), "stream s read at s * n from the copy pitched at cap"),
    "spectrum_raw": (("flags", "gated"), "the spectrum taken from the unconditioned input"),
    "negative_off": (("negative_gain",), "a negative gain treated as 'IQ balance off'"),
}


class Model(Chain):
    """one stream's conditioners over whole calls: Chain (same bits, the CPU tier asserts it) when wrong is None, else Chain with that one
    change.  call(x) takes one call's samples; IQ balance restarts per frame, the other stages are serial in time and do not care how a
    call is cut"""

    def __init__(self, oracle_mod, fs, frame, wrong=None):
        Chain.__init__(self, oracle_mod, fs, frame)
        self.fs, self.wrong = fs, wrong
        self.dc_slot = self          # whose DC filter this stream runs on (by_position moves it)
        self.py = dict(avg=1.0, cnt=0, prev=[0j, 0j])   # nb1_six: NB1 restated in Python (noiseblanker.cpp:45-75), its own state

    def set(self, flags, gain=1.0, phase=0.0):
        for bit, which in ((4, 1), (8, 2)):
            on, was = bool(flags & bit), bool(self.flags & bit)
            reset = on and not was
            if self.wrong == "no_reset":
                reset = False
            elif self.wrong == "reset_when_on":
                reset = on
            if reset:
                self.nb.enable(which)
                if which == 1:
                    self.py.update(avg=0.0, cnt=0)
        self.flags, self.gain, self.phase = flags, gain, phase

    def _nb1_python(self, v, spike):
        mag = np.sqrt(v.real * v.real + v.imag * v.imag).astype(np.float32).astype(np.float64)
        out, a, cnt = np.empty_like(v), self.py["avg"], self.py["cnt"]
        d = self.py["prev"] + list(v)
        f32 = np.float32
        for i, m in enumerate(mag):
            a = float(f32((0.999 * a) + (0.001 * m)))
            if cnt == 0 and m > a * 3.3:
                cnt = spike
            if cnt > 0:
                out[i] = 0
                cnt -= 1
            else:
                out[i] = d[i]   # DelayLine(8, 2): the input two samples earlier
        self.py.update(avg=a, cnt=cnt, prev=d[-2:])
        return out

    def call(self, x):
        O, w, fl = self.O, self.wrong, self.flags
        v = np.asarray(x, dtype=np.complex128)
        if w == "dc_zeroed":
            self.dc = O.Iir("hp", 10, 0.7071, self.fs)
        if w == "nb1_delay_cleared":
            for i in range(16):
                self.nb.s.delay[i] = 0.0
        if w == "nb1_count_dropped":
            self.nb.s.spike_count = 0
        order = ["dc", "iq", "nb1", "nb2"]
        if w == "nb2_first":
            order = ["dc", "iq", "nb2", "nb1"]
        if w == "iq_first":
            order = ["iq", "dc", "nb1", "nb2"]
        for stage in order:
            if stage == "dc":
                if fl & 1:
                    v = self.dc_slot.dc.process(v)
                elif w == "dc_awake":
                    self.dc.process(v)
            elif stage == "iq" and fl & 2 and not (w == "negative_off" and self.gain < 0):
                fr = 2048 if w == "iq_2048" else len(v) if w == "iq_carried" else self.frame
                v = np.concatenate([O.iq_balance(v[i:i + fr], self.gain, self.phase) for i in range(0, len(v), fr)])
            elif stage == "nb1" and fl & 4:
                self.nb_in.append((float(self.nb.s.nb_avg_mag), v))
                v = self._nb1_python(v, 6) if w == "nb1_six" else self.nb.process(v, which=1)
            elif stage == "nb2" and fl & 8:
                self.nb_in.append((float(self.nb.s.nb2_avg_mag), v))
                v = self.nb.process(v, which=2)
        return v


def conditioned(O, row, wrong=None, x=None):
    """the row's script on the oracle chain -> ([call] -> complex128 [S, n], or None where no stream has a flag; the streams' Models).
    Rows of streams without a flag are the input.  wrong: None or a key of WRONG (spectrum_raw changes nothing here: see observables)"""
    x = oracle_input(row.name) if x is None else x
    per_stream = None if wrong in ("by_position", "pitch_n", "spectrum_raw") else wrong
    ms = [Model(O, row.fs, row.nf, per_stream) for _ in range(row.S)]
    cap, flat, out = row.max_sf * row.sf, None, []
    for k, (lo, n) in enumerate(call_bounds(row)):
        for s, f, g, p in setters_before(row, k):
            ms[s].set(f, g, p)
        if not any(m.flags for m in ms):
            out.append(None)
            continue
        if wrong == "by_position":
            for pos, s in enumerate(dc_list(row, k)):
                ms[s].dc_slot = ms[pos]
        y = np.stack([ms[s].call(x[s, lo:lo + n]) for s in range(row.S)])
        if wrong == "pitch_n":   # rows written at s * cap, read at s * n; the buffer keeps what earlier calls left
            flat = np.zeros(row.S * cap, dtype=np.complex128) if flat is None else flat
            for s in range(row.S):
                flat[s * cap:s * cap + n] = y[s]
            y = np.stack([flat[s * n:s * n + n] for s in range(row.S)])
        out.append(y)
    return out, ms


_CACHE = {}


def right(O, name):
    if name not in _CACHE:
        _CACHE[name] = conditioned(O, ROWS[name])
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------
# the comparisons
# ------------------------------------------------------------------------------------------------
def view_figures(got, want):
    """the GPU tier's comparison of one call's conditioned() with the oracle chain -> (worst rel-RMS of a chunk of 512 consecutive samples
    over all streams, (stream, chunk) there, whether the exact-zero positions are the same)"""
    assert got.shape == want.shape, (got.shape, want.shape)
    worst, at = 0.0, (0, 0)
    for s in range(want.shape[0]):
        e = chunk_errors(got[s], want[s], CHUNK)
        i = int(np.argmax(e))
        if e[i] > worst:
            worst, at = e[i], (s, i)
    return worst, at, bool(np.array_equal(got == 0, want == 0))


def new_factor(row, good, bad):
    """by how many bars (TOL per chunk of 512) a model's conditioned streams miss the right ones, over the calls that conditioned"""
    return max(view_figures(b, g)[0] for g, b in zip(good, bad) if g is not None) / TOL


def observables(O, row, cond, spectrum_raw=False):
    """what the suite observed before: the USB (WFM) audio of every channel and the spectrum rows of every stream, from oracle Receivers
    WITHOUT conditioners fed the given conditioned streams (the input where a call conditioned nothing) -> (audio [C][n], rows [S][frames,
    bins] or None).  spectrum_raw: the rows taken from the unconditioned input instead"""
    x = oracle_input(row.name)
    fed = np.concatenate([x[:, lo:lo + n] if c is None else c for (lo, n), c in zip(call_bounds(row), cond)], axis=1)
    audio, rows = [], []
    for c in range(row.C):
        s = 0 if row.shared else c
        r = O.Receiver(row.fs, row.nf, row.bins)
        r.set_mode(O.FMM if row.wfm else O.USB)
        r.set_mixer(mixer_of(row, c))
        if not row.wfm:
            r.set_filter(*band_of(row))
        outs = [r.process(fed[s, i:i + row.nf], want_spectrum=bool(row.bins)) for i in range(0, fed.shape[1], row.nf)]
        audio.append(np.concatenate([o[0] for o in outs]))
        if row.bins and (c < row.S):
            rows.append(np.array([o[1] for o in outs]))
    if spectrum_raw and row.bins:
        rows = []
        for s in range(row.S):
            sp = O.Spectrum(row.bins, row.nf)
            rows.append(np.array([sp.process(x[s, i:i + row.nf]) for i in range(0, x.shape[1], row.nf)]))
    return audio, (rows if row.bins else None)


def old_factor(good_obs, bad_obs):
    """by how many bars a model moves the old observables -> (audio rel-RMS over a channel's whole run / TOL, spectrum rows from the
    second on / TOL_DB), each the worst over channels and streams"""
    (ga, gs), (ba, bs) = good_obs, bad_obs
    fa = max(rel_rms(b, g) for g, b in zip(ga, ba)) / TOL
    fs_ = 0.0 if gs is None else max(db_err(b[f], g[f]) for g, b in zip(gs, bs) for f in range(1, len(g))) / TOL_DB
    return fa, fs_


def receiver_oracles(O, row, x=None):
    """one oracle.Receiver per channel, given the row's script through set_conditioners -> [call] of (audio [C][nd], rows [S][frames, bins] or None)"""
    x = oracle_input(row.name) if x is None else x
    rs = []
    for c in range(row.C):
        r = O.Receiver(row.fs, row.nf, row.bins)
        r.set_mode(O.FMM if row.wfm else O.USB)
        r.set_mixer(mixer_of(row, c))
        if not row.wfm:
            r.set_filter(*band_of(row))
        rs.append(r)
    out = []
    for k, (lo, n) in enumerate(call_bounds(row)):
        for s, f, g, p in setters_before(row, k):
            for c in range(row.C):
                if (0 if row.shared else c) == s:
                    rs[c].set_conditioners(f, g, p)
        audio, rows = [], []
        for c in range(row.C):
            s = 0 if row.shared else c
            outs = [rs[c].process(x[s, i:i + row.nf], want_spectrum=bool(row.bins)) for i in range(lo, lo + n, row.nf)]
            audio.append(np.concatenate([o[0] for o in outs]))
            if row.bins and c < row.S:
                rows.append(np.array([o[1] for o in outs]))
        out.append((audio, rows if row.bins else None))
    return out
