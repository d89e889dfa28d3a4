"""The cases of tests/test_reference_pins.py: for each, the input recipe, the reference driver's command line
(oracle/ref_build/ref_driver.cpp) and the oracle's counterpart, both returning the same list of records.

Shared by the test module and tools/record_reference_pins.py, which writes the fixtures tests/golden/refpin_*.npy.

A record is (kind, float64 array); complex samples are stored interleaved.  kind:
  "x"  compared exactly (counts, chain tables, flags, and every record of a case whose bar is 0)
  "v"  values: relative RMS error <= the case's bar
  "d"  decibels: max |difference| <= the case's dB bar
"""
import json
import os
import subprocess
import tempfile

import numpy as np

from tests.signals import lcg_noise, tones

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BINARY = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
TAIL = 512  # values of a case's last record kept in its fixture (256 complex samples)

# The ceilings the bars may never exceed: four orders under the 1e-5 / 0.1 dB the oracle is used to judge.
MAX_BAR = 1e-9
MAX_BAR_DB = 1e-6


def _il(z):
    """complex -> interleaved float64"""
    return np.ascontiguousarray(z, dtype=np.complex128).view(np.float64).copy()


def run_driver(stage, x, args):
    """-> list of float64 arrays, the driver's records.  A binary that does not run is an error."""
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "in.f64"), os.path.join(d, "out.f64")
        (np.ascontiguousarray(x, dtype=np.float64) if np.isrealobj(x) else _il(x)).tofile(fi)
        p = subprocess.run([BINARY, stage, fi, fo] + [repr(float(a)) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=120)
        assert p.returncode == 0, "ref_driver %s failed (%d): %s" % (stage, p.returncode, p.stdout[-500:])
        raw = np.fromfile(fo, dtype=np.float64)
    out, pos = [], 0
    while pos < len(raw):
        n = int(raw[pos])
        out.append(raw[pos + 1:pos + 1 + n].copy())
        pos += 1 + n
    assert pos == len(raw)
    return out


def compress(records):
    """what a fixture holds of a list of records: every length; short records (counts, state scalars, chain tables, taps) whole;
    the last TAIL values of the last long record and the last 16 of the long ones before it"""
    records = [np.asarray(r, dtype=np.float64) for r in records]
    big = [i for i, r in enumerate(records) if len(r) > 160]
    parts = []
    for i, r in enumerate(records):
        k = len(r) if len(r) <= 160 else min(len(r), TAIL if i == big[-1] else 16)
        parts += [np.array([len(r), k], dtype=np.float64), r[len(r) - k:]]
    return np.concatenate(parts) if parts else np.zeros(0)


def expand(flat):
    """fixture -> [(full length, tail)]"""
    out, pos = [], 0
    while pos < len(flat):
        n, k = int(flat[pos]), int(flat[pos + 1])
        out.append((n, flat[pos + 2:pos + 2 + k]))
        pos += 2 + k
    return out


def record_error(kind, got, want):
    """-> the error of one record in the unit of its kind (0.0 when identical)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0 or np.array_equal(got, want):
        return 0.0
    if kind == "d":
        return float(np.abs(got - want).max())
    den = float(np.sqrt(np.mean(want ** 2)))
    num = float(np.sqrt(np.mean((got - want) ** 2)))
    return num / den if den > 0 else float("inf")


class Case:
    """view: what of the records a fixture is made of, [(kind, array)] -> [(kind, array)] (default: all of them, as they are).
    meta: what the device tier (tests/test_demod_reference_gpu.py) needs to run the case: mode, rate, calls, why"""

    def __init__(self, name, stage, args, make_input, oracle, bar=0.0, bar_db=0.0, view=None, meta=None):
        self.name, self.stage, self.args, self.make_input, self.oracle = name, stage, list(args), make_input, oracle
        self.bar, self.bar_db = bar, bar_db
        self.view = view if view is not None else (lambda pairs: pairs)
        self.meta = meta
        assert bar <= MAX_BAR and bar_db <= MAX_BAR_DB

    @property
    def fixture(self):
        return os.path.join(GOLD, "refpin_%s.npy" % self.name)

    def reference(self, x):
        return run_driver(self.stage, x, self.args)

    def allowed(self, kind):
        return 0.0 if kind == "x" else (self.bar_db if kind == "d" else self.bar)


# ---------------------------------------------------------------------------------------------------------------
# inputs (seeds and tones written here; regenerated, never stored)
# ---------------------------------------------------------------------------------------------------------------
def _wide(fs, n, seed):
    return tones(fs, n, [(0.3, 0.0586 * fs), (0.1, -0.146 * fs), (0.05, 0.0012 * fs)]) + lcg_noise(n, seed, 1e-3)


def _audio(fs, n, seed):
    return tones(fs, n, [(0.3, 1000.0), (0.2, -2200.0), (0.1, 4500.0), (0.05, 12000.0)]) + lcg_noise(n, seed, 1e-2)


# ---------------------------------------------------------------------------------------------------------------
# oracle counterparts: each returns [(kind, array)] in the driver's record order
# ---------------------------------------------------------------------------------------------------------------
def _mixer(fs, n, f0, retune=None):
    def run(O, x):
        m = O.Mixer(fs)
        m.set_frequency(f0)
        out = []
        for f in range(len(x) // n):
            if retune and f == retune[0]:
                m.set_frequency(retune[1])
            out.append(("v", _il(m.process(x[f * n:(f + 1) * n]))))
        return out
    return run


def _decimator(fs, bw, n):
    def run(O, x):
        d = O.Decimator(fs, bw)
        out = [("x", np.array([d.rate])), ("x", np.array([float(d.dec_by2_stages)])),
               ("x", np.array([v for c in d.chain() for v in c], dtype=np.float64))]
        for f in range(len(x) // n):
            out.append(("v", _il(d.process(x[f * n:(f + 1) * n]))))
        return out
    return run


def _downconvert(fs, bw, simple, calls):
    def run(O, x):
        d = O.DownConvert()
        out = [("x", np.array([d.set_data_rate(fs, bw, simple)]))]
        pos, prev = 0, None
        for ln, f, cw in calls:
            if prev != (f, cw):
                d.set_cw_offset(cw)
                d.set_frequency(f)
            prev = (f, cw)
            out.append(("v", _il(d.process(x[pos:pos + ln]))))
            pos += ln
        return out
    return run


def _fastfir(lo, hi, fs, n):
    def run(O, x):
        f = O.FastFIR(2048, 1025)
        f.setup(lo, hi, 0.0, fs)
        out = [("v", _il(f.coef()))]
        for b in range(len(x) // n):
            out.append(("v", _il(f.process(x[b * n:(b + 1) * n]))))
        return out
    return run


def _fir(ntaps, scale, astop, fpass, fstop, fs):
    def run(O, x):
        f = O.Fir()
        nt = f.init_lp(ntaps, scale, astop, fpass, fstop, fs)
        return [("x", np.array([float(nt)])), ("v", f.taps()), ("v", _il(f.process(x)))]
    return run


def _iir(kind, f0, q, fs, n=None):
    def run(O, x):
        f = O.Iir(kind, f0, q, fs)
        if n is None:
            return [("v", np.array(f.coeffs())), ("v", _il(f.process(x)))]
        return [("v", _il(f.process(x[b * n:(b + 1) * n]))) for b in range(len(x) // n)]
    return run


def _resampler(maxin, rate, n):
    def run(O, x):
        r = O.Resampler(maxin)
        out = []
        for f in range(len(x) // n):
            out.append(("v", _il(r.process(x[f * n:(f + 1) * n], rate))))
            out.append(("v", np.array([r.float_time])))
        return out
    return run


def _spectrum(bins, spb, lens):
    def run(O, x):
        s = O.Spectrum(bins, spb)
        out, pos = [], 0
        for ln in lens:
            out.append(("d", s.process(x[pos:pos + ln])))
            out.append(("x", np.array([float(s.overload)])))
            pos += ln
        return out
    return run


def _agc(fs, n, plan):
    def run(O, x):
        a = O.Agc(fs)
        out, prev = [], None
        for b, mt in enumerate(plan):
            if mt != prev:
                a.set_mode(*mt)
            prev = mt
            out.append(("v", _il(a.process(x[b * n:(b + 1) * n]))))
        return out
    return run


def _nb(which, n, plan):
    def run(O, x):
        nb = O.NoiseBlanker()
        out, prev = [], 0
        for b, on in enumerate(plan):
            if on and not prev:
                nb.enable(which)
            prev = on
            blk = x[b * n:(b + 1) * n]
            out.append(("v", _il(nb.process(blk, which) if on else blk)))  # disabled: the reference hands its input back
        return out
    return run


def _anf(n):
    def run(O, x):
        a = O.Anf()
        return [("v", _il(a.process(x[b * n:(b + 1) * n]))) for b in range(len(x) // n)]
    return run


def _iqbalance(n, gain, phase):
    def run(O, x):
        return [("v", _il(O.iq_balance(x[b * n:(b + 1) * n], gain, phase))) for b in range(len(x) // n)]
    return run


def _fdestimate(rate, mixer, bands):
    def run(O, sp):
        out = []
        for lo, hi in bands:
            v = O.fd_estimate(sp, rate, lo, hi, mixer)
            out.append(("v", np.array([v[0], v[1], v[2], v[3], v[1]])))
        return out
    return run


def _mapscreen(r):
    def run(O, db):
        px = O.map_fft_to_screen(db, r.bins, r.fs, r.y, r.x, r.max_db, r.min_db, r.start, r.stop)
        return [("x", px.astype(np.float64))]
    return run


# ---- the Morse restatement (tests/morse_ref.py): its Goertzel, TH_PEAK, clock and threshold-filter arithmetic against the pebblelib
# classes; the decoder proper (Morse::init, updateThresholds, stateMachine, findBestGoertzelN, setSampleRate) against the plugin's own
# morse.cpp, compiled unmodified into the driver (stage morse, further down)
def _morse_goertzel(rate, n, freq, switch_at, freq2):
    def run(O, x):
        from tests import morse_ref as M

        class Rec(M.MorseRef):
            peaks = None

            def th_peak(self, p):
                tone = super().th_peak(p)
                self.peaks.append(self.peak)
                return tone

        r = Rec(rate, 1)                      # at 8000 Hz and below the modem's decimator has no stage: the modem rate is the rate
        r.peaks = []
        assert (r.rate, r.n) == (rate, n)
        mode = {-1000: M.DM_CWL, 1000: M.DM_CWU}
        r.set_demod_mode(mode[freq])
        r.process_modem(x[:switch_at])
        r.set_demod_mode(mode[freq2])
        r.process_modem(x[switch_at:])
        return [("v", np.array(r.powers)), ("x", np.array(r.tones, dtype=np.float64)), ("v", np.array(r.peaks)),
                ("x", np.array([float(r.count)]))]
    return run


def _morse_clock(rate, pairs):
    def run(O, x):
        from tests import morse_ref as M
        return [("x", np.array([float(M.usec_delta(a, b, rate)) for a, b in pairs]))]
    return run


def _morse_sma(reset_at):
    def run(O, x):
        from tests import morse_ref as M
        r = M.MorseRef(8000, 1)
        out = []
        for i, v in enumerate(x):
            if i == reset_at or i == 0:
                r.sma, r.sma_i = None, 0      # MovingAvgFilter::reset, as MorseRef.init does it
            out.append(r.sma_sample(v))
        return [("v", np.array(out))]
    return run


def _morse_keyed(rate, n, freq, switch_at, seed):
    from tests import morse_ref as M
    out = lcg_noise(n, seed, 2e-3)
    for text, f, start in (("TEST", freq, 0), ("EE", -freq, switch_at)):
        env = M.keying(text, 25, rate)[:n - start]
        t = (np.arange(len(env)) + start) / float(rate)
        out[start:start + len(env)] += 0.05 * env * np.exp(2j * np.pi * f * t)
    return out


def morse_view(pairs):
    """The fixture of a stage-morse case.  The driver's records are decisions, events (sample, token, kind), starred events, statuses,
    powers.  The fixture keeps the decisions whole, 32 to a value; the events, stars and statuses whole, cut into records of at most
    160 values with their count in front; and the powers last, of which compress() keeps the tail"""
    (kt, tn), (ke, ev), (ks, stars), (kq, st), pw = pairs
    bits = np.concatenate([np.asarray(tn, dtype=np.int64), np.zeros(-len(tn) % 32, dtype=np.int64)]).reshape(-1, 32)
    out = [(kt, np.array([float(len(tn))]))]
    out += _chunks(kt, (bits << np.arange(32)).sum(axis=1).astype(np.float64))
    for k, v in ((ke, ev), (ks, stars), (kq, st)):
        c = _chunks(k, v)
        out += [(k, np.array([float(len(c))]))] + c
    return out + [pw]


def _chunks(kind, v, step=160):
    v = np.asarray(v, dtype=np.float64)
    return [(kind, v[i:i + step]) for i in range(0, max(len(v), 1), step)]


def morse_fixture(case):
    """a stage-morse fixture taken apart again -> dict: decisions [results], events [(sample, token, kind)], stars, statuses [k, 10],
    powers (the kept tail), results (the count)"""
    recs = [t for _, t in expand(np.load(case.fixture))]
    nres, pos = int(recs[0][0]), 1
    nb = max(1, -(-(-(-nres // 32)) // 160))
    packed = np.concatenate(recs[pos:pos + nb]).astype(np.int64); pos += nb
    tones = ((packed[:, None] >> np.arange(32)) & 1).reshape(-1)[:nres]
    parts = []
    for _ in range(3):
        k = int(recs[pos][0])
        parts.append(np.concatenate(recs[pos + 1:pos + 1 + k])); pos += 1 + k
    assert pos + 1 == len(recs)
    return dict(results=nres, decisions=tones.astype(bool).tolist(),
                events=[tuple(int(v) for v in e) for e in parts[0].reshape(-1, 3)], stars=[int(v) for v in parts[1]],
                statuses=parts[2].reshape(-1, 10).astype(np.int64).tolist(), powers=recs[-1])


def _morse_records(name, ref, seen):
    from tests import morse_hard_cases as H
    return [("x", np.array(ref.tones, dtype=np.float64)), ("x", np.array(ref.events, dtype=np.float64).reshape(-1)),
            ("x", np.array(H.stars_of(name, ref.events), dtype=np.float64)), ("x", np.array([s for _, s in seen], dtype=np.float64).reshape(-1)),
            ("v", np.array(ref.powers))]


def _morse_hard(name, rate, frame):
    def run(O, x):
        from tests import morse_hard_cases as H
        ref = H.reference(name, rate, frame)
        assert min(ref.margins) > H.MARGIN, (name, rate, frame, min(ref.margins))   # the condition of every row, at every geometry
        return _morse_records(name, ref, ref.seen)
    return run


def _morse_stream(rate, frame):
    """the stream of tests/morse_cases.py (TEST at -1000 Hz, CWU and MORSE at +1000 Hz), with the readings of a hard row's plan"""
    def run(O, x):
        from tests import morse_cases as MC, morse_hard_cases as H
        ref = H.CountingRef(rate, frame)
        seen = H.feed(ref, x, morse_stream_plan(rate, frame), frame)
        assert min(ref.margins) > MC.MARGIN
        return _morse_records("", ref, seen)
    return run


def morse_stream_plan(rate, frame):
    n1 = -(-int(2.2 * rate) // frame) * frame          # tests/morse_cases.stream's two lengths
    n = n1 + -(-int(4.6 * rate) // frame) * frame
    return sorted([(n1, "cwu")] + [(((n // frame) * q // 4) * frame, "status") for q in (1, 2, 3)], key=lambda p: p[0])


# the hard rows at the other forms of the modem's decimator: no stage, one stage, a fractional modem rate (7812 of 7812.5); every hard
# row runs at 64 000 (the merged 11-tap stage).  The frame is morse_cases.frames()' third: the block phase moves a sample a call
MORSE_HARD_ELSEWHERE = (("spike2", 8000), ("mode_rate_midchar", 12000), ("speed_15_35_15", 31250))


# ---- the Morse sender (tests/morsegen_ref.py) against the reference's own MorseGen (stage morsegen): setParams, setTextOut, then
# nextOutputSample n times.  n is one pass through the text, the rise of the mark it starts over with and 256 samples more, so that
# a fixture's tail lies inside a mark
MORSEGEN_FS, MORSEGEN_F, MORSEGEN_DB = 64000, 1000.0, -6.0
# (wpm, ms rise, text): test_morsegen_host's mark-table rows and its pinned 25 WPM row; the last has samplesPerTcw = 1536 barely above
# the rise of 1472 samples (a dot's steady part is 64 samples)
MORSEGEN_ROWS = ((50, 5, "TEST "), (40, 0, "CQ DE K1ABC "), (13, 20, "E"), (25, 5, "PARIS "), (50, 23, "TEN "))


def _morsegen_ref(wpm, ms_rise, text):
    from tests import morsegen_ref as G
    g = G.MorseGenRef(MORSEGEN_FS)
    g.set_params(MORSEGEN_F, G.db_to_amplitude(MORSEGEN_DB), wpm, ms_rise)
    g.set_text_out(G.text_tokens(text))
    return g


def morsegen_samples(wpm, ms_rise, text):
    g = _morsegen_ref(wpm, ms_rise, text)
    return g.lengths()[4] + g.rise + 256


def _keyed_edges(il):
    """the samples at which an interleaved stream starts or stops being zero"""
    z = (il[0::2] != 0) | (il[1::2] != 0)
    return np.flatnonzero(np.diff(np.concatenate([[False], z]).astype(np.int8))).astype(np.float64)


def morsegen_view(pairs):
    """counts, samples -> counts, the mark boundaries read off the samples (records of at most 160 values, their number in front),
    samples"""
    (kc, counts), (kv, x) = pairs
    e = _chunks("x", _keyed_edges(x))
    return [(kc, counts), ("x", np.array([float(len(e))]))] + e + [(kv, x)]


def _morsegen(wpm, ms_rise, text, n):
    def run(O, x):
        g = _morsegen_ref(wpm, ms_rise, text)
        y, key = g.generate(n)
        # the restatement's own mark table says what the samples say (the last sample of a fall may come out as an exact zero)
        edges = _keyed_edges(_il(y))
        starts = [s for s, _ in g.mark_starts if s < n]
        assert [int(v) for v in edges[0::2]] == starts, (edges[:8], starts[:4])
        assert all(key[int(a)] and key[int(b) - 1] and b - a >= (g.n_dot_buf - 1) for a, b in zip(edges[0::2], edges[1::2]))
        counts = [g.rise, g.fall, g.n_dot, g.n_dot_buf, g.n_dash, g.n_dash_buf, g.n_element, g.n_char, g.n_word]
        return [("x", np.array(counts, dtype=np.float64)), ("v", _il(y))]
    return run


def _clock_pairs(n):
    """(earlier, later) clock pairs: marks and spaces of a few to a few thousand results, earlier >= later (0 by definition), and
    spans whose microseconds pass 2^32 (the quint64 is cut to quint32)"""
    pairs = [(0, 0), (5, 5), (7, 3), (0, 1), (0, n - 1), (0, n), (0, n + 1)]
    pairs += [(k * 37, k * 37 + k * n) for k in range(1, 40)]
    pairs += [(11, 11 + k * n + (k % n)) for k in (3, 13, 127, 1021, 8191)]
    pairs += [(1, 40000000), (0, 4294967295), (123456, 3123456789)]
    return pairs


# ---- the demodulators (application/demod/): the driver calls the reference's classes the way Demod::processBlock, fmMono and fmStereo
# do (demod.cpp:100-141, :169-226); every record is compared exactly.  A call script is a list of lengths, ragged on purpose
DEMOD_CALLS = (2048, 2048, 1000, 81, 2048, 2048)   # the last call is whole, so that a fixture's tail lies inside it
DEMOD_N = 2048                                       # the buffer size the classes are constructed with: no call is longer


def _split(x, calls):
    out, pos = [], 0
    for ln in calls:
        out.append(x[pos:pos + ln])
        pos += ln
    assert pos == len(x)
    return out


def am_fading(fs, n, seed):
    """tests/demod_cases.am_input's recipe: a carrier fading from 0.5 to 0.1 with two modulating tones, turned in phase, plus noise"""
    t = np.arange(n) / float(fs)
    carrier = 0.096 + 0.4 * np.exp(-np.arange(n) / 2500.0)
    return (carrier * (1 + 0.5 * np.cos(2 * np.pi * 1000 * t + 0.4) + 0.2 * np.cos(2 * np.pi * 3300 * t))) * np.exp(0.7j) + lcg_noise(n, seed, 1e-4)


def _demod_am(fs, calls):
    def run(O, x):
        d = O.DemodAM(fs)
        out = []
        for blk, (_, bw) in zip(_split(x, [c[0] for c in calls]), calls):
            if bw:
                d.set_bandwidth(bw)
            out.append(("v", _il(d.process(blk))))
        return out
    return run


SAM_OFFSETS = {"lock": 30.0, "down": -40.0, "slip": 1500.0}
SAM_KINDS = ("lock", "down", "slip", "clamp")


def sam_carrier(fs, n, which):
    """an AM-modulated carrier (800 Hz, depth 0.5) off tune by SAM_OFFSETS[which], plus noise.  "clamp": a stronger carrier (the loop's
    gain follows the level, demod_sam.cpp:57) whose offset runs from 0 up to +1200 Hz within the first third and down to -1200 Hz by the
    end, 25 kHz/s at most, which the 100 Hz loop follows: it is taken past pllLimit (1000 Hz) on either side"""
    t = np.arange(n) / float(fs)
    if which == "clamp":
        u = np.arange(n) / float(n)
        f = 1200.0 * np.where(u < 1 / 3.0, 3 * u, 1 - 3 * (u - 1 / 3.0))
        return 0.8 * (1 + 0.3 * np.cos(2 * np.pi * 800 * t)) * np.exp(2j * np.pi * np.cumsum(f) / fs) + lcg_noise(n, 8, 1e-3)
    return (0.3 * (1 + 0.5 * np.cos(2 * np.pi * 800 * t))) * np.exp(2j * np.pi * SAM_OFFSETS[which] * t) + lcg_noise(n, 8, 1e-3)


def sam_trace(O, fs, x):
    """(frequency, phase) of the oracle's loop behind every sample (a second instance, walked sample by sample)"""
    d = O.DemodSAM(fs)
    f, p = np.empty(len(x)), np.empty(len(x))
    for i in range(len(x)):
        d.process(x[i:i + 1])
        f[i], p[i] = d.s.freq, d.s.phase
    return f, p, float(d.s.lo), float(d.s.hi)


def _demod_sam(fs, calls, which):
    def run(O, x):
        # the branch the input is there for was reached, read from the oracle's own loop state
        f, p, lo, hi = sam_trace(O, fs, x)
        jump = np.diff(p)
        up, down = int((jump > np.pi).sum()), int((jump < -np.pi).sum())   # the second while added 2 pi / the first took 2 pi off
        hz = f * fs / (2 * np.pi)
        if which == "lock":       # the loop settles on the carrier (the NCO turns against it) and never touches a clamp
            assert np.abs(hz[-2048:] + SAM_OFFSETS[which]).max() < 5.0 and f.min() > lo and f.max() < hi, (hz[-1], lo, hi)
            assert up > down, (up, down)                                     # the phase runs below 0 again and again: demod_sam.cpp:73-74
        elif which == "down":     # the other way round: the phase runs over 2 pi, demod_sam.cpp:71-72
            assert np.abs(hz[-2048:] + SAM_OFFSETS[which]).max() < 5.0 and f.min() > lo and f.max() < hi, (hz[-1], lo, hi)
            assert down > up, (up, down)
        elif which == "slip":     # 1500 Hz off, beyond the limit: the 100 Hz loop never captures the carrier and never reaches a clamp;
            # the phase is dragged round by the beat, wrapping many times
            assert f.min() > lo and f.max() < hi, (f.min(), f.max(), lo, hi)
            assert up + down >= 10, (up, down)
        else:                     # both clamps engage (demod_sam.cpp:63-66): exactly the limit is what only their assignments leave
            assert (f == lo).sum() >= 100 and (f == hi).sum() >= 100, (f.min(), f.max(), lo, hi)
        d = O.DemodSAM(fs)
        return [("v", _il(d.process(blk))) for blk in _split(x, calls)]
    return run


NFM_KINDS = ("tone", "clamp", "offset")


NFM_CARRIER = {"tone": 0.0, "clamp": 16000.0, "offset": 700.0}


def nfm_signal(fs, n, which):
    """a 1 kHz tone at 3 kHz deviation on a carrier NFM_CARRIER[which] off tune, plus noise.  The static offset of "offset" carries the
    tone as well: behind the loop's DC removal a bare carrier leaves nothing but the loop's own noise floor (6e-5 rad / sample RMS), on
    which the reference algorithm fed single-precision samples misses itself by 1e-2 -- a relative error against that measures no kernel.
    With the offset the float phase counts up to 140 .. 240 rad inside a call, where its last bit is 1.5e-5 rad: fed single-precision
    samples the reference algorithm misses itself by 2e-7 to 5e-6 over the tail of these cases (by 1.1e-5 on one 8-sample snippet at
    48 000), against 7e-8 without the offset"""
    t = np.arange(n) / float(fs)
    return 0.3 * np.exp(1j * (3.0 * np.sin(2 * np.pi * 1000 * t) + 2 * np.pi * NFM_CARRIER[which] * t)) + lcg_noise(n, 7, 1e-3)


def _demod_nfm(fs, calls, which):
    def run(O, x):
        d = O.DemodNFM(fs)
        out, ends = [], []
        for blk in _split(x, calls):
            out.append(("v", _il(d.process(blk))))
            ends.append(float(d.s.err_dc))     # the loop's own running average of nco_freq (1 ms)
        if which == "clamp" and fs / 2.0 > 16000.0 + 3000.0:
            # the clamp (demod_nfm.cpp:242-245) replaced nco_freq on thousands of samples.  At 37 500 the carrier's swing passes half
            # the rate, the loop never settles on it and no sample is clamped: the row is pinned all the same, without this assertion
            assert d.s.n_clamped >= 1000, d.s.n_clamped
        if which == "offset":     # at that average the phase passes 2 pi several times inside a 2048-sample call, between the per-call fmods (:253)
            assert all(abs(f) * 2048 > 3 * 2 * np.pi for f in ends), ends
        return out
    return run


WFM_MONO_CALLS = (2048, 2048, 1000)


def wfm_fm(fs, n, seed):
    """tests/demod_cases.wfm_input's recipe at full level: 1 kHz and 3.3 kHz tones, peak deviation min(75 kHz, rate / 4) * 1.3"""
    t = np.arange(n) / float(fs)
    f = min(75000.0, fs / 4.0) * (np.cos(2 * np.pi * 1000.0 * t + 0.9) + 0.3 * np.cos(2 * np.pi * 3300.0 * t + 0.2))
    return 0.5 * np.exp(2j * np.pi * np.cumsum(f) / float(fs)) + lcg_noise(n, seed, 1e-4)


def _demod_wfm_mono(fs, calls):
    def run(O, x):
        d = O.DemodWFM(float(fs))
        out = []
        for blk in _split(x, calls):
            out += [("x", np.array([float(len(blk))])), ("v", _il(d.process(blk)))]
        return out
    return run


def fm_stereo_mpx(fs, n, pilot_phase):
    """the multiplex of tests/test_parity_gpu.py::test_wfm_stereo_mode_is_the_reference_from_the_first_block: 1 kHz left, 2.5 kHz right,
    the pilot, the 38 kHz difference signal, on a 75 kHz-deviation carrier, plus that test's noise"""
    t = np.arange(n) / float(fs)
    left, right = 0.9 * np.sin(2 * np.pi * 1000 * t), 0.9 * np.sin(2 * np.pi * 2500 * t)
    mpx = 0.45 * (left + right) + 0.1 * np.sin(2 * np.pi * 19000 * t + pilot_phase) \
        + 0.45 * (left - right) * np.sin(2 * (2 * np.pi * 19000 * t + pilot_phase))
    return 0.5 * np.exp(1j * 2 * np.pi * 75000 * np.cumsum(mpx) / fs) + lcg_noise(n, 9, 1e-4)


# the RDS rows: tests/rds_signal.py's multiplex of the groups test_rds_groups_of_a_multiplex_through_the_restated_decoder sends, the
# subcarrier 14 Hz low as there.  At 390 625 (24 414 Hz behind the chain) the decoder finds no block A at the default levels, as at
# 384 000 (tests/rds_cases.A_LEVELS): that row carries the stronger subcarrier under quieter audio that row uses.  The lengths are the
# shortest, in 2048-sample calls, at which the third group has been popped, and two calls more
RDS_PIN_ROWS = {256000: (84, {}), 390625: (110, dict(rds_level=0.2, audio_level=0.1))}


def rds_mpx(fs):
    from tests import rds_signal as rs
    calls, levels = RDS_PIN_ROWS[fs]
    return rs.fm_multiplex(rs.make_groups(30), float(fs), 2048 * calls, subcarrier_offset_hz=-14.0, **levels)


def _demod_wfm_stereo(fs, calls, rds):
    def run(O, x):
        d = O.DemodWFM(float(fs))
        out, last, popped = [], True, []      # getStereoLock: m_LastPilotLocked starts as !m_PilotLocked, demod_wfm.cpp:122-123
        for blk in _split(x, calls):
            y, lock = d.process_stereo(blk)
            g = d.next_rds_group()
            out += [("x", np.array([float(len(blk))])), ("v", _il(y)), ("x", np.array([float(lock != last), float(lock)])),
                    ("x", np.array([0.0] * 5 if g is None else [float(g[1])] + [float(v) for v in g[0]]))]
            last = lock
            if g is not None:
                popped.append(g[0])
        rest = []
        while True:
            g = d.next_rds_group()
            if g is None:
                break
            rest += [float(v) for v in g[0]]
        out.append(("x", np.array(rest)))
        if rds:                   # at least three groups came through, a popped group's BlockA is there, and the queue was never cleared
            assert len(popped) >= 3 and all(g[0] != 0 for g in popped), popped
            assert len(rest) == 0
        return out
    return run


HEAD = 256  # complex samples of the first call a head_view fixture keeps


def head_view(pairs):
    """The fixture of a case whose later output cannot be followed sample by sample (the SAM loop out of lock): every record, and then
    the first HEAD samples of the first call once more, as the last record, which compress() keeps whole"""
    return list(pairs) + [(pairs[0][0], pairs[0][1][:2 * HEAD])]


def stereo_view(audio_every):
    """The fixture of a demod_wfm_stereo case.  Its records are per call (count, output, (changed, lock), (got, four words)) and a drained
    queue at the end; the fixture regroups them so that a hundred calls fit: the counts of all calls, the lock pairs of all calls, one
    row (call, got, four words) per call that delivered a group, the drained queue -- each cut into records of at most 160 values,
    which compress() keeps whole, the numbers of group and queue records in front of them -- and then the outputs of every audio_every-th call and of the last one"""
    def chunks(kind, v, step):
        v = np.asarray(v, dtype=np.float64)
        return [(kind, v[i:i + step]) for i in range(0, max(len(v), 1), step)]

    def view(pairs):
        assert len(pairs) % 4 == 1
        calls = len(pairs) // 4
        rows = [[float(k)] + list(pairs[4 * k + 3][1]) for k in range(calls) if np.any(pairs[4 * k + 3][1] != 0)]
        out = chunks("x", np.concatenate([pairs[4 * k][1] for k in range(calls)]), 160)
        out += chunks("x", np.concatenate([pairs[4 * k + 2][1] for k in range(calls)]), 160)
        grp, rest = chunks("x", np.array(rows).reshape(-1), 156), chunks("x", pairs[-1][1], 160)
        out += [("x", np.array([float(len(grp)), float(len(rest))]))] + grp + rest
        out += [pairs[4 * k + 1] for k in stereo_audio_calls(calls, audio_every)]
        return out
    return view


def stereo_audio_calls(calls, audio_every):
    return [k for k in range(calls) if k % audio_every == 0 or k == calls - 1]


def stereo_fixture(case):
    """the fixture of a demod_wfm_stereo case, taken apart again -> dict: counts [calls], locks [calls, 2], groups {call: (got, a, b, c,
    d)}, rest [m, 4], audio {call: the kept tail, interleaved}"""
    calls, every = len(case.meta["calls"]), case.meta["audio_every"]
    recs = [t for _, t in expand(np.load(case.fixture))]
    n160 = lambda m: max(1, -(-m // 160))
    pos = 0
    counts = np.concatenate(recs[pos:pos + n160(calls)]); pos += n160(calls)
    locks = np.concatenate(recs[pos:pos + n160(2 * calls)]).reshape(-1, 2); pos += n160(2 * calls)
    audio_calls = stereo_audio_calls(calls, every)
    audio = dict(zip(audio_calls, recs[len(recs) - len(audio_calls):]))
    ngrp, nrest = int(recs[pos][0]), int(recs[pos][1])
    rows = np.concatenate(recs[pos + 1:pos + 1 + ngrp]).reshape(-1, 6)
    rest = np.concatenate(recs[pos + 1 + ngrp:pos + 1 + ngrp + nrest]).reshape(-1, 4)
    assert pos + 1 + ngrp + nrest + len(audio_calls) == len(recs)
    assert len(counts) == calls and len(locks) == calls
    return dict(counts=counts, locks=locks, groups={int(r[0]): tuple(int(v) for v in r[1:]) for r in rows}, rest=rest, audio=audio)


# ---------------------------------------------------------------------------------------------------------------
# the table of cases
# ---------------------------------------------------------------------------------------------------------------
def _levels(fs, n, nblocks, seed):
    """AGC input over about 2 s (the modes differ by decay constants of 100 ms .. 2 s, so nothing shorter tells them apart): a tone
    whose level starts in silence, steps to between the two knees (0.0316 and 0.1 for thresholds 30 and 20), under both, up by 30 dB
    (attack; the peak-window rescan runs at every step down), is held for a second so that the decay average charges (its rise takes
    0.3 of the mode's decay time), then drops by 9.5 dB to a level above both knees, where the decay average alone sets the gain until
    the end: the tail a fixture keeps lies there."""
    m = n * nblocks
    t = np.arange(m) / float(fs)
    env = np.full(m, 0.2)
    for t0, t1, v in ((0.0, 0.05, 0.001), (0.05, 0.15, 0.06), (0.15, 0.25, 0.02), (0.25, 1.25, 0.6)):
        env[(t >= t0) & (t < t1)] = v
    return env * tones(fs, m, [(1.0, 1000.0), (0.1, -2200.0)]) + lcg_noise(m, seed, 1e-3)


def _spiky(fs, n, seed):
    x = tones(fs, n, [(0.05, 101e3), (0.02, -250e3)]) + lcg_noise(n, seed, 1e-3) + 0.01
    x[5000 % n] += 2.0
    x[3000:3003] += 1.5j
    x[n - 1000] -= 3.0
    return x


def _toggled(fs, n, seed):
    """three blocks for a blanker that is on, off, on: the level drops to a quarter for the third block, and 150 samples before its end
    comes a spike of 0.19.  The average a blanker keeps has a time constant of 1000 samples: restarted from zero by the setter it
    stands near 0.043 there (the spike is over 3.3 times that and is blanked), carried over from the first block it would stand near
    0.072 (the spike would pass).  So the reset shows in the last 256 samples, the part of the output a fixture keeps."""
    x = tones(fs, 3 * n, [(1.0, 101e3)]) * np.repeat([0.2, 0.2, 0.05], n) + lcg_noise(3 * n, seed, 1e-3) + 0.001
    x[3 * n - 150] = 0.19
    return x


def _spectrum_input(n, seed, hot_frame=None, spb=2048):
    x = tones(2048000, n, [(10 ** (-10 / 20) * 0.9, 0.2305 * 2048000), (0.01, 0.4871 * 2048000), (0.003, -0.31 * 2048000)]) \
        + lcg_noise(n, seed, 1e-3)
    if hot_frame is not None:
        x[hot_frame * spb + 17] = 0.95 + 0.1j  # one sample over the 0.9 overload limit
    return x


def _dc_calls(D, f0, fs):
    # the call lengths of the device test, quartered where the first stage is a generic halfband: the reference copies a call
    # into a buffer of 32768 samples there (downconvert.cpp:60,345) and writes past it on a longer one
    q = 4 if D == 64 else 1
    lens = [D * 600 // q, D * 256 // q, D * 1024 // q, D * 300 // q]
    return [(lens[0], f0, 0.0), (lens[1], f0, 0.0), (lens[2], f0 + 0.01 * fs / D, 700.0), (lens[3], 0.0, 0.0)]


def _dc_input(fs, D, f0, n):
    return tones(fs, n, [(0.3, f0 + 0.02 * fs / D), (0.2, f0 - 0.05 * fs / D), (0.3, f0 + 0.37 * fs), (0.1, 0.013 * fs / D)]) \
        + lcg_noise(n, 4, 1e-3)


DC_BOUNDARY = ((384000.0, 1024), (256000.0, 512))     # chains 11, 15, 23, 51 and 15, 19, 35: 1024 >> 3 = 128 >= 100, 512 >> 2 = 128 >= 68
DC_INPLACE = ((384000.0, 512), (256000.0, 256))       # 512 >> 3 = 64 < 100, 256 >> 2 = 64 < 68: every stage still sees its taps
DC_RDS_BW, DC_RDS_F0, DC_EQUAL_CALLS = 8000.0, 57000.0, 6


def _dc_equal_calls_case(dfs, ln, prefix="downconvert"):
    """CDownConvert at the RDS branch's settings (SetDataRate(rate, 8000), 57 kHz) over six equal calls"""
    calls = [(ln, DC_RDS_F0, 0.0)] * DC_EQUAL_CALLS
    stages = {384000.0: 4, 256000.0: 3}[dfs]
    return Case("%s_%d_%d_x%d" % (prefix, dfs, DC_RDS_BW, ln), "downconvert", [dfs, DC_RDS_BW, 0] + [v for c in calls for v in c],
                lambda: _dc_input(dfs, 1 << stages, DC_RDS_F0, ln * DC_EQUAL_CALLS), _downconvert(dfs, DC_RDS_BW, False, calls))


def inplace_cases():
    """NOT in cases(): below 2 (T - 1) samples per stage the reference's in-place DecBy2 copies its next history out of samples its own
    outputs have overwritten, and the oracle (exact history, what the device streams) is NOT the reference there.  The fixtures
    tests/golden/refpin_inplace_*.npy hold the reference's outputs whole (32 outputs a call); tests/test_oracle_pins.py holds the oracle to
    them on the first call and asserts that it differs from the second call on."""
    return [_dc_equal_calls_case(dfs, ln, "inplace_downconvert") for dfs, ln in DC_INPLACE]


def _build_cases():
    C = []
    fs, n = 2048000, 2048
    # Mixer::processBlock
    C.append(Case("mixer_100k", "mixer", [fs, n, 100e3], lambda: _wide(fs, 4 * n, 11), _mixer(fs, n, 100e3)))
    C.append(Case("mixer_retune", "mixer", [fs, n, 100e3, 2, -250e3], lambda: _wide(fs, 4 * n, 12), _mixer(fs, n, 100e3, (2, -250e3))))
    C.append(Case("mixer_zero", "mixer", [fs, n, 0.0], lambda: _wide(fs, 2 * n, 13), _mixer(fs, n, 0.0)))
    # Decimator: chain builder and cascade (vDSP path, combined stages), then once through HalfbandFilter::process
    for dfs, bw, dn, frames in ((2048000, 30000, 2048, 4), (2048000, 200000, 2048, 4), (20000000, 200000, 2048, 4),
                                (100000000, 30000, 49152, 2), (100000000, 30000, 2048, 1), (20000000, 30000, 2048, 1)):
        C.append(Case("decimator_%d_%d_%d" % (dfs, bw, dn), "decimator", [dfs, bw, dn, 0],
                      lambda dfs=dfs, dn=dn, frames=frames: _wide(dfs, frames * dn, 21), _decimator(dfs, bw, dn)))
    C.append(Case("decimator_plain_2048000_30000", "decimator", [2048000, 30000, 2048, 1], lambda: _wide(2048000, 4 * 2048, 21),
                  _decimator(2048000, 30000, 2048)))
    # CDownConvert: the four cases of test_downconvert_step_against_the_oracle
    for dfs, bw, simple, stages in ((2048000.0, 15000.0, False, 5), (10e6, 15000.0, False, 7), (20e6, 200000.0, True, 6), (250000.0, 48000.0, False, 0)):
        D, f0 = 1 << stages, 0.11 * dfs
        calls = _dc_calls(D, f0, dfs)
        C.append(Case("downconvert_%d_%d" % (dfs, bw), "downconvert", [dfs, bw, int(simple)] + [v for c in calls for v in c],
                      lambda dfs=dfs, D=D, f0=f0, calls=calls: _dc_input(dfs, D, f0, sum(c[0] for c in calls)),
                      _downconvert(dfs, bw, simple, calls)))
    # ... and the RDS down-converter's chains (bw 8000) at the shortest equal calls whose every stage sees 2 (T - 1) samples or more:
    # from there up CHalfBandDecimateBy2's in-place history (downconvert.cpp:325, :389-390) is the stream's, and the oracle is bit for bit
    for dfs, ln in DC_BOUNDARY:
        C.append(_dc_equal_calls_case(dfs, ln))
    # CFastFIR 2048/1025 at 64 kHz: H and three blocks
    for lo, hi in ((300, 3000), (-5000, 5000), (-3000, -300), (1000, 1500)):
        C.append(Case("fastfir_%d_%d" % (lo, hi), "fastfir", [lo, hi, 0, 64000, 2048], lambda: _audio(64000, 3 * 2048, 31),
                      _fastfir(float(lo), float(hi), 64000.0, 2048)))
    # CFir Kaiser low-pass (the demodulators' audio filters) and CIir LP / HP
    for nm, a in (("am10k_64k", (0, 1.0, 50.0, 10000.0, 10000.0 * 1.8, 64000.0)), ("nfm_64k", (0, 1.0, 50.0, 3000.0, 1.6 * 3000.0, 64000.0)),
                  ("sam_64k", (0, 1.0, 40.0, 4500.0, 5500.0, 64000.0)), ("wfm_256k", (0, 1.0, 60.0, 15000.0, 21000.0, 256000.0)),
                  ("wfm_312k5", (0, 1.0, 60.0, 15000.0, 21000.0, 312500.0))):
        C.append(Case("fir_" + nm, "fir", a, lambda a=a: _audio(a[5], 4096, 41), _fir(*a)))
    for nm, kind, a in (("lp_15k_256k", "lp", (15000.0, 0.7071, 256000.0)), ("hp_10_64k", "hp", (10.0, 0.7071, 64000.0)),
                        ("lp_15k_312k5", "lp", (15000.0, 0.7071, 312500.0))):
        C.append(Case("iir_" + nm, "iir", [0 if kind == "lp" else 1] + list(a), lambda a=a: _audio(a[2], 4096, 42) + 0.01, _iir(kind, *a)))
    # CFractResampler (complex)
    for out_rate in (11025, 48000):
        C.append(Case("resampler_%d" % out_rate, "resampler", [4096, 64000.0 / out_rate, 2048], lambda: _audio(64000, 6 * 2048, 51),
                      _resampler(4096, 64000.0 / out_rate, 2048)))
    # FFT::fftParams / fftSpectrum with the Blackman-Harris window
    for bins in (2048, 4096, 8192):
        C.append(Case("spectrum_%d" % bins, "spectrum", [bins, 2048, 2048000, 0, 2048, 2048, 2048], lambda: _spectrum_input(3 * 2048, 61),
                      _spectrum(bins, 2048, [2048] * 3)))
    C.append(Case("spectrum_short_buffer", "spectrum", [4096, 2048, 2048000, 0, 2048, 1500, 2048], lambda: _spectrum_input(2048 + 1500 + 2048, 62),
                  _spectrum(4096, 2048, [2048, 1500, 2048])))
    C.append(Case("spectrum_overload_then_short", "spectrum", [2048, 2048, 2048000, 0, 2048, 2048, 1000, 2048],
                  lambda: _spectrum_input(3 * 2048 + 1000, 63, hot_frame=1), _spectrum(2048, 2048, [2048, 2048, 1000, 2048])))
    C.append(Case("spectrum_ooura_4096", "spectrum", [4096, 2048, 2048000, 1, 2048, 2048, 2048], lambda: _spectrum_input(3 * 2048, 61),
                  _spectrum(4096, 2048, [2048] * 3), bar_db=OOURA_BAR_DB))
    # AGC: five modes x two thresholds x two rates over 16 blocks of 8192 (2 s at 64 kHz); a change of mode and threshold between blocks,
    # just behind the drop, so that the new decay constant and the new knee both show in what follows
    an, ab = 8192, 16
    for afs in (64000, 48828):
        for mode, mname in ((0, "off"), (1, "fast"), (2, "med"), (3, "slow"), (4, "long")):
            for thr in (20, 30):
                plan = [(mode, thr)] * ab
                C.append(Case("agc_%s_%d_%d" % (mname, thr, afs), "agc", [afs, an] + [v for p in plan for v in p],
                              lambda afs=afs: _levels(afs, an, ab, 71), _agc(afs, an, plan)))
    plan = [(2, 30)] * 10 + [(3, 20)] * 6
    C.append(Case("agc_med_to_slow", "agc", [64000, an] + [v for p in plan for v in p], lambda: _levels(64000, an, ab, 72), _agc(64000, an, plan)))
    # conditioners: spikes and a DC offset, 3 blocks with state carried; each blanker disabled then enabled again
    bn = 8192
    for which in (1, 2):
        C.append(Case("nb%d" % which, "nb", [which, fs, bn, 1, 1, 1], lambda: _spiky(fs, 3 * bn, 81), _nb(which, bn, [1, 1, 1])))
        C.append(Case("nb%d_off_on" % which, "nb", [which, fs, 2048, 1, 0, 1], lambda: _toggled(fs, 2048, 82), _nb(which, 2048, [1, 0, 1])))
    C.append(Case("anf", "anf", [64000, 2048], lambda: tones(64000, 3 * 2048, [(0.05, 1000.0), (0.03, 2200.0)]) + lcg_noise(3 * 2048, 5, 1e-2),
                  _anf(2048)))
    C.append(Case("iqbalance", "iqbalance", [fs, bn, 1.02, 0.03], lambda: _spiky(fs, 3 * bn, 83), _iqbalance(bn, 1.02, 0.03)))
    for dfs in (2048000, 20000000):
        C.append(Case("dcremoval_%d" % dfs, "dcremoval", [dfs, bn], lambda dfs=dfs: _spiky(dfs, 3 * bn, 84),
                      _iir("hp", 10.0, 0.7071, float(dfs), n=bn)))
    # SignalStrength::fdEstimate: two bands over one spectrum
    bands = [(-4000.0, 4000.0), (300.0, 3000.0)]
    C.append(Case("fdestimate", "fdestimate", [2048000, 2048, 2048000, 100000.0] + [v for b in bands for v in b], _fd_spectrum,
                  _fdestimate(2048000, 100000.0, bands)))
    # ... and every window of tests/strength_cases.py: clipped at either end, bpBins == 0 with one bin and with none, no noise bin,
    # truncating bin widths, a refused (inverted) band-pass.  Where fdEstimate divides 0 by 0 its qBound returns the lower bound
    # (oracle/ref_build/standins/qt_standins.h words qMin as Qt does): every recorded value is finite
    from tests import strength_cases as S
    for name, rate, sbins, lo, hi, mixer, _ in S.ROWS:
        C.append(Case("fdestimate_" + name, "fdestimate", [rate, 2048, rate, mixer, lo, hi], lambda name=name: S.row_spectrum(name),
                      _fdestimate(rate, mixer, [(lo, hi)])))
    # FFT::mapFFTToScreen on every pinned row of tests/screen_cases.py (the rows whose float -> int conversions are all in range): one dB
    # row of float32 values in, the pixels out; the driver and the oracle run the same libm in the same order, so the bar is 0
    from tests import screen_cases as SC
    for r in SC.ROWS:
        if r.pinned:
            C.append(Case("mapscreen_" + r.name, "mapscreen", [r.bins, r.fs, r.y, r.x, r.max_db, r.min_db, r.start, r.stop],
                          lambda name=r.name: SC.row_input(name), _mapscreen(r)))
    # the Morse modem's pebblelib classes at its four modem rates (no stage; 6000; 4687 of 4687.5; 7812 of 7812.5), both tones, the
    # tone moved to the other side on a running filter (Morse::setDemodMode): GoertzelOOK TH_PEAK, SampleClock, MovingAvgFilter(8)
    from tests import morse_ref as M
    for mrate in (8000, 6000, 4687, 7812):
        mn = M.best_n(mrate)
        total = int(2.6 * mrate)
        sw = int(1.7 * mrate) + 7             # inside a block, not on its boundary
        for freq in (-1000, 1000):
            C.append(Case("morse_goertzel_%d_%s" % (mrate, "cwl" if freq < 0 else "cwu"), "goertzel", [mrate, 2048, mn, freq, sw, -freq],
                          lambda mrate=mrate, freq=freq, total=total, sw=sw: _morse_keyed(mrate, total, freq, sw, 95),
                          _morse_goertzel(mrate, mn, freq, sw, -freq), bar=MORSE_POWER_BAR))
        pairs = _clock_pairs(mn)
        C.append(Case("morse_clock_%d" % mrate, "sampleclock", [mrate] + [v for p in pairs for v in p], lambda: np.zeros(0),
                      _morse_clock(mrate, pairs)))
    C.append(Case("morse_threshold_filter", "movingavg", [8, 21], _sma_input, _morse_sma(21)))
    # the plugin's decoder itself on the hard rows of tests/morse_hard_cases.py and on the stream of tests/morse_cases.py: decisions,
    # events, starred events and statuses (estimate, range flags, modem rate, N, the five thresholds) exact, powers to MORSE_POWER_BAR
    from tests import morse_cases as MC, morse_hard_cases as H
    where = [(nm, H.RATE, H.FRAME) for nm in H.NAMES] + [(nm, r, MC.frames(r)[2]) for nm, r in MORSE_HARD_ELSEWHERE]
    for nm, rate, frame in where:
        C.append(Case("morse_hard_%s_%d" % (nm, rate), "morse", H.driver_args(rate, frame, H.plan(nm, rate, frame)[1]),
                      lambda nm=nm, rate=rate, frame=frame: H.stream(nm, rate, frame)[0], _morse_hard(nm, rate, frame),
                      bar=MORSE_POWER_BAR, view=morse_view, meta=dict(row=nm, rate=rate, frame=frame)))
    for wpm, ms_rise, text in MORSEGEN_ROWS:
        total = morsegen_samples(wpm, ms_rise, text)
        C.append(Case("morsegen_%d_%d" % (wpm, ms_rise), "morsegen", [MORSEGEN_FS, MORSEGEN_F, MORSEGEN_DB, wpm, ms_rise, total] + [ord(c) for c in text],
                      lambda: np.zeros(0), _morsegen(wpm, ms_rise, text, total), bar=MORSEGEN_BAR, view=morsegen_view))
    C.append(Case("morse_stream_64000", "morse", H.driver_args(64000, 2048, morse_stream_plan(64000, 2048)),
                  lambda: MC.stream(64000, 2048)[0], _morse_stream(64000, 2048), bar=MORSE_POWER_BAR, view=morse_view))
    C += _demod_rows()
    return C


def _demod_rows():
    """the demodulators at the rates the library runs them: 64 000 (2.048 Msps receivers), 37 500 (2.4 Msps), 48 000 (no decimator)"""
    C = []
    N = DEMOD_N
    # AM: setBandwidth before the first call and before the third (CFir::InitLPFilter clears the delay line)
    am_calls = [(2048, 10000.0), (2048, 0.0), (1000, 6000.0), (81, 0.0), (2048, 0.0)]
    for fs in (64000, 37500):
        C.append(Case("demod_am_%d" % fs, "demod_am", [fs, N] + [v for c in am_calls for v in c],
                      lambda fs=fs: am_fading(fs, sum(c[0] for c in am_calls), 90), _demod_am(fs, am_calls),
                      meta=dict(mode="AM", rate=fs, calls=[c[0] for c in am_calls], bw=[c[1] for c in am_calls], why="")))
    n = sum(DEMOD_CALLS)
    for fs in (64000, 37500, 48000):
        for which in SAM_KINDS:
            # out of lock the float loop is chaotic: the oracle fed the same samples rounded to single precision, the device's input
            # format, misses 1e-4 against itself within the first call ("slip": 1e-3 to 3e-3 over the first call, 0.7 to 2 over the
            # tail) and, where the loop is driven along a clamp, in the later calls ("clamp": 1e-4 to 1.6e-3 over the tail).  Over the
            # first 256 samples it stays at 2e-8.  Those are what the device tier compares of these cases, so their fixtures keep them
            head = which in ("slip", "clamp")
            C.append(Case("demod_sam_%s_%d" % (which, fs), "demod_sam", [fs, N] + list(DEMOD_CALLS),
                          lambda fs=fs, which=which: sam_carrier(fs, n, which), _demod_sam(fs, DEMOD_CALLS, which),
                          view=head_view if head else None,
                          meta=dict(mode="SAM", rate=fs, calls=list(DEMOD_CALLS), which=which, head=head,
                                    why="the first %d samples of the first call: behind them the loop's float trajectory cannot be "
                                        "followed from single-precision input" % HEAD if head else "")))
        for which in NFM_KINDS:
            # 16 kHz off at 37 500: the carrier's swing passes half the rate and the loop never settles; like the SAM loop out of lock,
            # the reference algorithm fed single-precision samples misses itself there (2.7e-5 over the tail, 1e-5 over the first call,
            # 9e-7 over its first 256 samples), so the device tier compares that stretch
            head = which == "clamp" and fs == 37500
            C.append(Case("demod_nfm_%s_%d" % (which, fs), "demod_nfm", [fs, N] + list(DEMOD_CALLS),
                          lambda fs=fs, which=which: nfm_signal(fs, n, which), _demod_nfm(fs, DEMOD_CALLS, which),
                          view=head_view if head else None,
                          meta=dict(mode="FMN", rate=fs, calls=list(DEMOD_CALLS), which=which, head=head,
                                    why="the first %d samples of the first call: the loop is out of lock" % HEAD if head else "")))
    # WFM mono: one row per path decision of the device's WfmCore::init (low-pass off; sequential; one kernel; longest responses)
    for fs in (100000, 192000, 256000, 512000):
        C.append(Case("demod_wfm_mono_%d" % fs, "demod_wfm_mono", [fs, N] + list(WFM_MONO_CALLS),
                      lambda fs=fs: wfm_fm(fs, sum(WFM_MONO_CALLS), 70), _demod_wfm_mono(fs, WFM_MONO_CALLS),
                      meta=dict(mode="FMM", rate=fs, calls=list(WFM_MONO_CALLS), why="")))
    # WFM stereo: the lock sequence of the pilot loop itself, ten blocks
    for fs in (256000, 312500):
        for pp in (1.0, 2.5):
            calls = [2048] * 10
            C.append(Case("demod_wfm_stereo_%d_%s" % (fs, str(pp).replace(".", "p")), "demod_wfm_stereo", [fs, N] + calls,
                          lambda fs=fs, pp=pp: fm_stereo_mpx(fs, 2048 * 10, pp), _demod_wfm_stereo(fs, calls, False), view=stereo_view(1),
                          meta=dict(mode="FMS", rate=fs, calls=calls, audio_every=1, rds=False, why="")))
    # the RDS branch up to the group queue; 390 625 is where the device's decimation goes from 8 to 16
    for fs, (ncalls, _) in RDS_PIN_ROWS.items():
        calls = [2048] * ncalls
        C.append(Case("demod_wfm_rds_%d" % fs, "demod_wfm_stereo", [fs, N] + calls, lambda fs=fs: rds_mpx(fs),
                      _demod_wfm_stereo(fs, calls, True), view=stereo_view(8),
                      meta=dict(mode="FMS", rate=fs, calls=calls, audio_every=8, rds=True, why="")))
    return C


def _sma_input():
    """dot-dash thresholds as updateThresholds feeds them: whole microseconds, (dash + dot) / 2 for speeds of 10 to 50 WPM"""
    from tests.signals import lcg_uniform
    u = lcg_uniform(40, 97)
    return np.floor(2 * 1200000 / (10 + 40 * u))


def _fd_spectrum():
    """a dB spectrum of 4096 bins: a ragged floor near -100 dB and a ragged plateau around the mixer's bin"""
    from tests.signals import lcg_uniform
    u = lcg_uniform(4096, 91)
    sp = -100.0 + 6.0 * u
    sp[2248 - 3:2248 + 4] = -30.0 - 3.0 * u[:7]
    return sp


# Every stage comes out bit for bit against the reference binary and is asserted equal (bar 0).  The one bar is for the cross-check
# of the spectrum through the reference's in-tree Ooura transform, a different FFT: measured 1.01e-10 dB on the CPU, times ten.
OOURA_BAR_DB = 1.1e-9
# The Goertzel powers and peak averages of the Morse restatement against the reference's GoertzelOOK: measured bit for bit as well
MORSE_POWER_BAR = 0.0
# The sender's samples, the restatement's serial sums against the reference's MorseGen: counts and mark boundaries exact; of the
# samples 13 to 234 in 50 000 to 500 000 values differ, by one unit in the last place, at the same sample numbers whatever the rise
# (so in cos / sin of the phase sum: the compiler pairs the reference's cos(acc), sin(acc) into one sincos call, whose last place is
# not always cos's and sin's own).  Measured 3.4e-18 to 4.0e-18 relative RMS; the bar is ten times the largest
MORSEGEN_BAR = 4e-17

CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = _build_cases()
    return CASES


def chains_table():
    return json.load(open(os.path.join(GOLD, "chains.json")))
