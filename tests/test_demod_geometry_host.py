"""CPU tier of the demodulator-rate table (tests/demod_cases.py).

 - The path table: csrc/design.cpp, compiled here with g++ and asked with WfmCore::init's rule, puts every WFM row on the path it is
   there for (`fused`, Llp, L4 pinned), and the call-length scripts take Lx from that program.
 - At every WFM and AM row the oracle, fed the row's ragged calls, IS the plain fp64 chain run over the whole input in one piece
   (biquad -> 0.25 atan2 -> CFir -> de-emphasis -> notch; |x| -> DC block -> CFir), to 1e-12 per chunk: the oracle is split-invariant
   at exactly these lengths, so any difference the GPU tier sees at a call boundary is the library's.
 - The one-kernel design (both cascades folded into FIRs, taps rounded to fp32 as uploaded, history = the last Lx input samples)
   evaluated in fp64 stays 100x inside the bar at every one-kernel row.
 - The inputs are adequate: seven deliberately wrong models miss the bar by a factor of 100 on a chunk they reach, and are inside it
   on every chunk of the calls before the first they can affect.
 - The rows satisfy the size rules the library enforces, and every oracle chunk carries signal.
"""
import functools

import numpy as np
import pytest
from scipy.signal import lfilter

from tests import demod_cases as DC

EXACT = 1e-12
MARGIN = 100 * DC.TOL


# ------------------------------------------------------------------------------------------------
# the oracle over a row's script (computed once per row, never changed)
# ------------------------------------------------------------------------------------------------
_cache = {}


def oracle_wfm(oracle_mod, row):
    """[call] outputs of oracle.DemodWFM fed the row's valid calls"""
    if row.name not in _cache:
        ref, x = oracle_mod.DemodWFM(row.rate), DC.wfm_input(row)
        _cache[row.name] = [ref.process(x[o:o + n]) for o, n in DC.call_offsets(DC.wfm_script(row))]
        for y in _cache[row.name]:
            y.setflags(write=False)
    return _cache[row.name]


def oracle_am(oracle_mod, row):
    if row.name not in _cache:
        ref, x, outs = oracle_mod.DemodAM(row.rate, DC.AM_BW[0]), DC.am_input(row), []
        for k, (o, n) in enumerate(DC.call_offsets(DC.am_script(row))):
            if k == DC.AM_CHANGE_BEFORE:
                ref.set_bandwidth(DC.AM_BW[1])
            outs.append(ref.process(x[o:o + n]))
            outs[-1].setflags(write=False)
        _cache[row.name] = outs
    return _cache[row.name]


def split(y, script):
    return [y[o:o + n] for o, n in DC.call_offsets(script)]


def all_chunk_errors(got_calls, ref_calls, size):
    """[(call, chunk, rel-RMS)]"""
    return [(c, k, e) for c, (g, r) in enumerate(zip(got_calls, ref_calls)) for k, e in enumerate(DC.chunk_errors(g, r, size))]


def check_wrong(errs, first_affected, label):
    """a wrong model against the oracle: inside the bar on every chunk of the calls before `first_affected`, and at least 100 bars off
    on a chunk from there on"""
    before = [e for c, _, e in errs if c < first_affected]
    after = [e for c, _, e in errs if c >= first_affected]
    assert after, label
    assert all(e <= DC.TOL for e in before), (label, max(before))
    assert max(after) >= MARGIN, (label, max(after))
    return max(after)


# ------------------------------------------------------------------------------------------------
# plain fp64 chains
# ------------------------------------------------------------------------------------------------
def wfm_coeffs(oracle_mod, rate):
    lp = oracle_mod.Iir("lp", 75000, 1.0, rate).coeffs()
    br = oracle_mod.Iir("br", 19000.0, 5, rate).coeffs()
    f = oracle_mod.Fir()
    f.init_lp(0, 1.0, 60.0, 15000.0, 1.4 * 15000.0, float(rate))
    return lp, f.taps(), 1.0 - np.exp(-1.0 / (rate * 75E-6)), br


def discriminate(x, prev):
    """0.25 atan2(I1 Q0 - I0 Q1, I1 I0 + Q1 Q0): the angle of x[n] conj(x[n-1]) (atan2(0, 0) = 0 on the very first sample)"""
    d = x * np.conj(np.concatenate([[prev], x[:-1]]))
    return 0.25 * np.arctan2(d.imag, d.real)


def wfm_plain(oracle_mod, rate, x):
    """Demod_WFM::processDataMono over the whole input in one piece (demod_wfm.cpp:207-232)"""
    (b0, b1, b2, a1, a2), h, da, (n0, n1, n2, m1, m2) = wfm_coeffs(oracle_mod, rate)
    if rate >= 150000:
        x = lfilter([b0, b1, b2], [1.0, a1, a2], x)
    y = lfilter(h, [1.0], discriminate(x, 0.0))
    y = 2.0 * lfilter([da], [1.0, -(1.0 - da)], y)
    y = lfilter([n0, n1, n2], [1.0, m1, m2], y)
    return y + 1j * y


def dc_block(mag):
    """demod_am.cpp:52-57 as written: m_amDc = ALPHA * m_amDcLast + mag; out = m_amDc - m_amDcLast (ALPHA a float literal)"""
    alpha, last, out = float(np.float32(0.9999)), 0.0, np.empty(len(mag))
    for i, m in enumerate(mag.tolist()):
        dc = (alpha * last) + m
        out[i] = dc - last
        last = dc
    return out


def am_taps(oracle_mod, rate, bw):
    f = oracle_mod.Fir()
    f.init_lp(0, 1.0, 50.0, bw, bw * 1.8, float(rate))
    return f.taps()


def am_plain(oracle_mod, row):
    """Demod_AM::processBlockFiltered over the whole input in one piece; the FIR starts afresh where the bandwidth changes"""
    x = DC.am_input(row)
    y = dc_block(np.sqrt(x.real * x.real + x.imag * x.imag))
    cut = DC.call_offsets(DC.am_script(row))[DC.AM_CHANGE_BEFORE][0]
    y = np.concatenate([lfilter(am_taps(oracle_mod, row.rate, DC.AM_BW[0]), [1.0], y[:cut]), lfilter(am_taps(oracle_mod, row.rate, DC.AM_BW[1]), [1.0], y[cut:])])
    return y + 1j * y


# ------------------------------------------------------------------------------------------------
# call-by-call models with carried state, right or deliberately wrong
# ------------------------------------------------------------------------------------------------
class Section:
    """one recurrence of a scan (any realisation: only what later outputs see of the state matters).
    wrong = "pad": the carried state is taken at the end of the call's last 8-sample segment, the missing samples run as zero steps
    (k_iir_scan reading the scan's lane state instead of the state after the last valid sample);
    wrong = "zero": the carried state is zeroed at every call after the first"""

    def __init__(self, b, a, wrong=None):
        self.b, self.a, self.wrong, self.z, self.calls = np.asarray(b, float), np.asarray(a, float), wrong, None, 0

    def run(self, u):
        nz = max(len(self.a), len(self.b)) - 1
        if self.z is None or (self.wrong == "zero" and self.calls):
            self.z = np.zeros(nz, dtype=u.dtype)
        self.calls += 1
        pad = (-len(u)) % DC.K_SEG if self.wrong == "pad" else 0
        y, self.z = lfilter(self.b, self.a, np.concatenate([u, np.zeros(pad, dtype=u.dtype)]), zi=self.z.astype(u.dtype))
        return y[:len(u)]


class SequentialWfm:
    """WfmCore::run's sequential path call by call.  wrong: "pad" / "zero" in all three recurrences (models a, b), or "discrim": the
    discriminator's previous sample is zero at every call start (model e: a[-1] not refreshed)"""

    def __init__(self, oracle_mod, rate, wrong=None):
        (b0, b1, b2, a1, a2), h, da, (n0, n1, n2, m1, m2) = wfm_coeffs(oracle_mod, rate)
        scan = wrong if wrong in ("pad", "zero") else None
        self.lp = Section([b0, b1, b2], [1.0, a1, a2], scan) if rate >= 150000 else None
        self.fir = Section(h, [1.0])
        self.de = Section([2.0 * da], [1.0, -(1.0 - da)], scan)
        self.notch = Section([n0, n1, n2], [1.0, m1, m2], scan)
        self.prev, self.wrong = 0.0, wrong

    def process(self, x):
        a = self.lp.run(np.asarray(x, dtype=np.complex128)) if self.lp else np.asarray(x, dtype=np.complex128)
        d = discriminate(a, 0.0 if self.wrong == "discrim" else self.prev)
        self.prev = a[-1]
        y = self.notch.run(self.de.run(self.fir.run(d)))
        return y + 1j * y


class ScanAm:
    """AmCore::run call by call: |x| -> k_iir_scan<2,1> -> k_fir_dec"""

    def __init__(self, oracle_mod, rate, wrong=None):
        self.o, self.rate = oracle_mod, rate
        self.dc = Section([1.0, -1.0], [1.0, -float(np.float32(0.9999))], wrong)
        self.set_bandwidth(DC.AM_BW[0])

    def set_bandwidth(self, bw):
        self.fir = Section(am_taps(self.o, self.rate, bw), [1.0])

    def process(self, x):
        y = self.fir.run(self.dc.run(np.abs(np.asarray(x, dtype=np.complex128))))
        return y + 1j * y


class FoldedWfm:
    """k_wfm_fir in fp64: both cascades as FIRs with the taps rounded to fp32 as uploaded, no carried filter state, history = the last
    Lx input samples.  wrong = "shift": the history is read one sample off (model c); wrong = "merge": a call shorter than Lx leaves
    [zeros | its own input] as history instead of [the old history's end | its own input] (model d)"""

    def __init__(self, design, wrong=None):
        self.hlp = design.hlp.astype(np.float32).astype(np.float64)
        self.h = design.h.astype(np.float32).astype(np.float64)
        self.Lx, self.L4 = design.Llp + design.L4, design.L4
        self.hist, self.wrong = np.zeros(self.Lx, dtype=np.complex128), wrong
        # (the kernel rounds the low-pass off switch the same way: tap 1.0)

    def process(self, x):
        x = np.asarray(x, dtype=np.complex128)
        hist = np.concatenate([[0.0], self.hist[:-1]]) if self.wrong == "shift" else self.hist
        xx = np.concatenate([hist, x])
        lp = np.convolve(xx, self.hlp, mode="valid")          # positions -L4 - 1 .. n - 1
        d = discriminate(lp[1:], lp[0])                        # positions -L4 .. n - 1
        y = np.convolve(d, self.h, mode="valid")[-len(x):]     # positions 0 .. n - 1 (h has L4 taps: valid gives n + 1)
        if len(x) >= self.Lx:
            self.hist = x[len(x) - self.Lx:].copy()
        elif self.wrong == "merge":
            self.hist = np.concatenate([np.zeros(self.Lx - len(x), dtype=np.complex128), x])
        else:
            self.hist = np.concatenate([self.hist[len(x):], x])
        return y + 1j * y


def run_wfm(model, row):
    x = DC.wfm_input(row)
    return [model.process(x[o:o + n]) for o, n in DC.call_offsets(DC.wfm_script(row))]


def run_am(model, row):
    x, outs = DC.am_input(row), []
    for k, (o, n) in enumerate(DC.call_offsets(DC.am_script(row))):
        if k == DC.AM_CHANGE_BEFORE:
            model.set_bandwidth(DC.AM_BW[1])
        outs.append(model.process(x[o:o + n]))
    return outs


def first_call_after(script, pred):
    """index of the valid call that follows the first valid call with pred(n)"""
    for k, n in enumerate(DC.valid_calls(script)):
        if pred(n):
            return k + 1
    raise AssertionError("the script has no such call")


# ------------------------------------------------------------------------------------------------
# the path table
# ------------------------------------------------------------------------------------------------
def test_every_wfm_row_sits_on_the_path_it_is_there_for():
    """WfmCore::init's decision, asked of csrc/design.cpp: `fused`, Llp and L4 of every row as the table has them, so a change of a
    threshold (the fold's tolerance, kWfmIrMax, kWfmLpMax, the 64 KiB of LDS) cannot silently move a row onto the other path; the
    scripts' Lx is the program's.  The receiver's own WFM rates (250 000 .. 480 000) stay on the one-kernel path."""
    for row in DC.WFM_ROWS:
        d = DC.wfm_design(row.rate)
        assert (d.fused, d.Llp if d.fused else 0, d.L4 if d.fused else 0) == (row.fused, row.Llp, row.L4), (row.name, d[:4])
        assert DC.wfm_lx(row) == (row.L4 + row.Llp if row.fused else DC.MIN_CALL)
        assert row.chunk == (DC.K_WFM_OUTB if row.fused else DC.K_SUB)
        if d.fused:
            assert d.L4 % 16 == 0 and len(d.h) == d.L4 and len(d.hlp) == d.Llp and (d.Llp == 1) == (row.rate < 150000)
            if d.Llp == 1:
                assert d.hlp[0] == 1.0
    assert [r.rate for r in DC.WFM_ROWS if not r.fused] == [150000, 192000, 1000000]
    assert [(r.rate, r.Llp, r.L4) for r in DC.WFM_ROWS if r.fused] == [(100000, 1, 272), (125000, 1, 320), (256000, 49, 544), (512000, 62, 1024)]
    # the rest of the table the rows were chosen from
    others = {160000: False, 200000: False, 240000: (52, 512), 312500: (47, 656), 390625: (51, 800), 625000: False, 781250: False}
    for rate, want in others.items():
        d = DC.wfm_design(rate)
        assert (d.fused and (d.Llp, d.L4)) == want, (rate, d[:4])
    for rate in (250000, 480000):
        assert DC.wfm_design(rate).fused
    # every rate below 150 000 folds, so WfmCore::run's k_copy front (sequential path, low-pass off) has no caller
    for rate in list(range(40000, 150000, 2500)) + [44100, 48000, 96000, 149999]:
        d = DC.wfm_design(rate)
        assert d.fused and d.Llp == 1, rate
    k = DC._header_constants()
    assert k["kWfmOutB"] == DC.K_WFM_OUTB


def test_rows_and_scripts_satisfy_the_size_rules():
    """AmCore::run / WfmCore::run: n >= kMaxTaps = 80 and n <= the capacity given at create; the scripts have short after short, short
    after long, long after short, lengths that are no multiple of 4, 8, 512 or 1024, refused calls before and between valid ones, and
    stay under 20 000 samples a row.  The bank and resampler rows: whole super-frames, at most max_superframes a call."""
    names = [r.name for r in DC.WFM_ROWS + DC.AM_ROWS + DC.RS_ROWS]
    assert len(set(names)) == len(names)
    for row in DC.WFM_ROWS:
        s, Lx = DC.wfm_script(row), DC.wfm_lx(row)
        v = DC.valid_calls(s)
        assert s[0] == DC.REFUSED and DC.REFUSED in s[1:-1] and all(n == DC.REFUSED or n >= DC.MIN_CALL for n in s)
        assert sum(v) < 20000 and max(v) == 3 * 1024 + 2 and len(DC.wfm_input(row)) == sum(v)
        assert {80, 81, Lx, Lx + 1, 1023, 1024, 1025, 1027, 513, 519, 520, 521} <= set(v)
        if row.fused:
            # the quiet calls: each short call that follows another call directly in front of a loud stretch, and the call behind it
            assert DC.WFM_QUIET_CALLS == (1, 2, 7, 8) and [v[k] for k in (0, 1, 6, 7)] == [80, 81, 1023, 80] and 81 < Lx
            assert v.count(Lx - 1) == 2 and Lx - 1 >= DC.MIN_CALL
            short = [n < Lx for n in v]
            pairs = set(zip(short, short[1:]))
            assert pairs == {(True, True), (True, False), (False, True), (False, False)}, row.name
        else:
            assert s.count(DC.REFUSED) == 4
        assert any(n % 4 for n in v) and any(n % 8 for n in v) and any(n % 512 and n > 512 for n in v) and any(n % 1024 and n > 1024 for n in v)
    for row in DC.AM_ROWS:
        s = DC.am_script(row)
        v = DC.valid_calls(s)
        assert s[0] == DC.REFUSED and s.count(DC.REFUSED) == 2 and v == [80, 81, 87, 88, 89, 511, 512, 513, 519, 520, 521, 1025, 2568, 80]
        assert v[DC.AM_CHANGE_BEFORE] == 513 and sum(v) < 20000
        # every edge of scan_sub: nv <= kSeg never (n >= 80) but a last sub-chunk of 1 (513, 1025), 7, 8 (520, 2568), 9 samples; cnt < kSeg
        assert {n % DC.K_SUB for n in v if n > DC.K_SUB} == {1, 7, 8, 9}
        assert {n % DC.K_SEG for n in v} == {0, 1, 7}
    assert DC.BANK_CALLS == 6 and 0 < DC.BANK_AWAY_CALL < DC.BANK_CALLS - 2 and DC.BANK_AWAY in DC.BANK_AM
    assert [c for c, ch in enumerate(DC.BANK_CHANNELS) if ch[0] == "AM"] == list(DC.BANK_AM) and len(DC.BANK_CHANNELS) == DC.BANK_C
    assert max(DC.RS_CALLS) == 2 and sum(DC.RS_CALLS) == 4
    for row in DC.RS_ROWS:
        assert row.demod_rate != row.audio_rate  # (equal rates take the copy branch, receiver.cpp:1002-1003: no resampler)
    assert any(r.audio_rate > r.demod_rate for r in DC.RS_ROWS)


def test_am_bank_tap_counts_differ_and_one_is_the_clamp(oracle_mod):
    """AmCore::set_bandwidth's tap counts of the three AM channels (csrc/design.cpp) are three different ones, one of them CFir's
    75-tap clamp, and they are the oracle's"""
    counts = [DC.am_ntaps(DC.BANK_RATE, DC.BANK_CHANNELS[c][2] - DC.BANK_CHANNELS[c][1]) for c in DC.BANK_AM]
    assert len(set(counts)) == 3 and 75 in counts and all(3 <= n <= 75 for n in counts), counts
    for c, n in zip(DC.BANK_AM, counts):
        assert oracle_mod.DemodAM(DC.BANK_RATE, DC.BANK_CHANNELS[c][2] - DC.BANK_CHANNELS[c][1]).ntaps == n
    for row in DC.AM_ROWS:
        for bw in DC.AM_BW:
            assert DC.am_ntaps(row.rate, bw) == oracle_mod.DemodAM(row.rate, bw).ntaps
        assert DC.am_ntaps(row.rate, DC.AM_BW[0]) != DC.am_ntaps(row.rate, DC.AM_BW[1])
    print("AM bank tap counts of channels %s: %s" % (DC.BANK_AM, counts))


# ------------------------------------------------------------------------------------------------
# the oracle is the plain chain, and every chunk carries signal
# ------------------------------------------------------------------------------------------------
def signal_floor(calls, size):
    """the least chunk RMS of the oracle's output over the whole run's RMS"""
    whole = DC.rms(np.concatenate(calls))
    return min(DC.rms(y[lo:hi]) for y in calls for lo, hi in DC.chunk_bounds(len(y), size)) / whole


@pytest.mark.parametrize("name", [r.name for r in DC.WFM_ROWS])
def test_the_oracle_is_the_plain_wfm_chain_at_these_call_lengths(oracle_mod, name):
    """oracle.DemodWFM over the row's ragged calls against biquad -> 0.25 atan2 -> CFir -> de-emphasis -> notch (scipy.signal.lfilter,
    fp64) over the concatenated input, per chunk: 1e-12.  Every oracle chunk's RMS is at least 1 % of the run's."""
    row = {r.name: r for r in DC.WFM_ROWS}[name]
    calls = oracle_wfm(oracle_mod, row)
    plain = split(wfm_plain(oracle_mod, row.rate, DC.wfm_input(row)), DC.wfm_script(row))
    e, c, k = DC.worst_of(all_chunk_errors(calls, plain, row.chunk))
    floor = signal_floor(calls, row.chunk)
    print("%s: oracle against the plain chain, worst chunk %.2e (call %d chunk %d); least chunk RMS %.3f of the run's" % (name, e, c, k, floor))
    assert e <= EXACT
    assert floor >= 0.01
    # and the call-by-call model with true carried state is the same thing
    seq = run_wfm(SequentialWfm(oracle_mod, row.rate), row)
    assert DC.worst_of(all_chunk_errors(seq, calls, row.chunk))[0] <= EXACT


@pytest.mark.parametrize("name", [r.name for r in DC.AM_ROWS])
def test_the_oracle_is_the_plain_am_chain_at_these_call_lengths(oracle_mod, name):
    """oracle.DemodAM over the row's ragged calls, with the bandwidth change, against |x| -> DC block -> CFir over the concatenated
    input, per chunk: 1e-12"""
    row = {r.name: r for r in DC.AM_ROWS}[name]
    calls = oracle_am(oracle_mod, row)
    plain = split(am_plain(oracle_mod, row), DC.am_script(row))
    e, c, k = DC.worst_of(all_chunk_errors(calls, plain, row.chunk))
    floor = signal_floor(calls, row.chunk)
    print("%s: oracle against the plain chain, worst chunk %.2e (call %d chunk %d); least chunk RMS %.3f of the run's" % (name, e, c, k, floor))
    assert e <= EXACT
    assert floor >= 0.01
    model = run_am(ScanAm(oracle_mod, row.rate), row)
    assert DC.worst_of(all_chunk_errors(model, calls, row.chunk))[0] <= 1e-10  # (lfilter's DC block rounds at 3000 ulp(1): see dc_block)


# ------------------------------------------------------------------------------------------------
# the folded design
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in DC.WFM_ROWS if r.fused])
def test_the_folded_design_is_100_times_inside_the_bar(oracle_mod, name):
    """k_wfm_fir's design in fp64 (taps rounded to fp32) against the oracle, per chunk of 1024 outputs of every call: what truncating
    the cascades' responses at 1e-11 and rounding the taps costs.  Measured 6e-9 .. 1e-8 at the rows without the low-pass, 4e-9 .. 5e-9
    with it; the bar for the design is TOL / 100."""
    row = {r.name: r for r in DC.WFM_ROWS}[name]
    got = run_wfm(FoldedWfm(DC.wfm_design(row.rate)), row)
    e, c, k = DC.worst_of(all_chunk_errors(got, oracle_wfm(oracle_mod, row), row.chunk))
    print("%s: folded design against the oracle, worst chunk %.2e (call %d chunk %d)" % (name, e, c, k))
    assert e <= DC.TOL / 100


# ------------------------------------------------------------------------------------------------
# adequacy: wrong models a .. e on the step rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in DC.WFM_ROWS if not r.fused])
def test_wrong_sequential_paths_miss_the_bar_by_100(oracle_mod, name):
    """(a) the scans carry the state of the end of the last 8-sample segment, (b) they zero it at every call after the first,
    (e) k_discrim's previous sample is zero at every call start.  A row that fails this needs another input, not another margin."""
    row = {r.name: r for r in DC.WFM_ROWS}[name]
    ref, script = oracle_wfm(oracle_mod, row), DC.wfm_script(row)
    first = {"pad": first_call_after(script, lambda n: n % DC.K_SEG != 0), "zero": 1, "discrim": 1}
    assert first["pad"] == 2
    for wrong in ("pad", "zero", "discrim"):
        errs = all_chunk_errors(run_wfm(SequentialWfm(oracle_mod, row.rate, wrong), row), ref, row.chunk)
        print("%s, wrong model '%s': worst chunk %.2e (bar %.0e)" % (name, wrong, check_wrong(errs, first[wrong], (name, wrong)), MARGIN))


@pytest.mark.parametrize("name", [r.name for r in DC.AM_ROWS])
def test_wrong_am_scans_miss_the_bar_by_100(oracle_mod, name):
    """(a) and (b) on k_iir_scan<2,1>.  The DC block's pole is 0.9999: a zero step changes its state by 1e-4 of itself, so model (a)
    shows only because the state is hundreds of carrier amplitudes by the later ragged calls -- the input's carrier fades for that
    (demod_cases.am_input)."""
    row = {r.name: r for r in DC.AM_ROWS}[name]
    ref, script = oracle_am(oracle_mod, row), DC.am_script(row)
    first = {"pad": first_call_after(script, lambda n: n % DC.K_SEG != 0), "zero": 1}
    assert first["pad"] == 2
    for wrong in ("pad", "zero"):
        errs = all_chunk_errors(run_am(ScanAm(oracle_mod, row.rate, wrong), row), ref, row.chunk)
        print("%s, wrong model '%s': worst chunk %.2e (bar %.0e)" % (name, wrong, check_wrong(errs, first[wrong], (name, wrong)), MARGIN))


@pytest.mark.parametrize("name", [r.name for r in DC.WFM_ROWS if r.fused])
def test_wrong_one_kernel_histories_miss_the_bar_by_100(oracle_mod, name):
    """(c) the history read one sample off, (d) the short-call merge keeping only the new input.  (d) loses what is older than the
    short call itself, 80 samples and more, where the response has almost ended at the rows without the low-pass: the input is quiet
    during the short calls and the calls behind them for that (demod_cases.WFM_QUIET_CALLS), and the model misses by 100 bars at
    every row.  It first shows where the lost samples were not zero anyway: behind the second short call."""
    row = {r.name: r for r in DC.WFM_ROWS}[name]
    ref, script, d = oracle_wfm(oracle_mod, row), DC.wfm_script(row), DC.wfm_design(row.rate)
    first = {"shift": 1, "merge": first_call_after(script, lambda n: n < d.Llp + d.L4) + 1}
    assert first["merge"] == 2
    for wrong in ("shift", "merge"):
        errs = all_chunk_errors(run_wfm(FoldedWfm(d, wrong), row), ref, row.chunk)
        print("%s, wrong model '%s': worst chunk %.2e (bar %.0e)" % (name, wrong, check_wrong(errs, first[wrong], (name, wrong)), MARGIN))


# ------------------------------------------------------------------------------------------------
# the AM bank: (f) two channels with their tap sets swapped
# ------------------------------------------------------------------------------------------------
def test_swapped_am_tap_sets_miss_the_bar_by_100(oracle_mod):
    """the bank's oracle recipe with the bandwidths of two AM channels exchanged (every pair), against the recipe as it is, per
    2048-sample frame: both channels of the pair are off by 100 bars in some frame, the other channels are untouched"""
    dec = oracle_mod.Decimator(DC.BANK_FS, 30000)
    sf = DC.BANK_FRAME * dec.total_decimation
    x = DC.bank_input(DC.BANK_CALLS * sf)
    right = bank_oracle_cached(oracle_mod)
    bw = {c: DC.BANK_CHANNELS[c][2] - DC.BANK_CHANNELS[c][1] for c in DC.BANK_AM}
    for p, q in ((1, 3), (1, 4), (3, 4)):
        wrong = DC.bank_oracle(oracle_mod, x, sf, dec.dec_by2_stages, {p: bw[q], q: bw[p]})
        for c in range(DC.BANK_C):
            errs = [e for k in range(DC.BANK_CALLS) for e in DC.chunk_errors(wrong[c][k], right[c][k], DC.BANK_FRAME)]
            if c in (p, q):
                assert max(errs) >= MARGIN, (p, q, c, max(errs))
            else:
                assert max(errs) == 0.0
    # the away call: the channel's output is its band-pass output, and its Demod_AM object was not fed
    assert all(len(right[c][k]) == DC.BANK_FRAME for c in range(DC.BANK_C) for k in range(DC.BANK_CALLS))
    floor = min(DC.rms(right[c][k]) for c in range(DC.BANK_C) for k in range(DC.BANK_CALLS)) / max(DC.rms(np.concatenate(right[c])) for c in range(DC.BANK_C))
    assert floor >= 0.01, floor


@functools.lru_cache(maxsize=None)
def bank_oracle_cached(oracle_mod):
    dec = oracle_mod.Decimator(DC.BANK_FS, 30000)
    sf = DC.BANK_FRAME * dec.total_decimation
    return DC.bank_oracle(oracle_mod, DC.bank_input(DC.BANK_CALLS * sf), sf, dec.dec_by2_stages)


# ------------------------------------------------------------------------------------------------
# the resampler: the oracle's counts, a plain restatement, and (g) a time sum that restarts at every call
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sinc_table():
    """fractresampler.cpp:104-118"""
    n = 280001
    i = np.arange(n, dtype=np.float64)
    w = 0.35875 - 0.48829 * np.cos(2 * np.pi * i / (n - 1)) + 0.14128 * np.cos(4 * np.pi * i / (n - 1)) - 0.01168 * np.cos(6 * np.pi * i / (n - 1))
    fi = np.pi * (i - n // 2) / 10000.0
    fi[n // 2] = 1.0
    t = w * np.sin(fi) / fi
    t[n // 2] = 1.0
    return t


def resample(calls, dt, restart=False):
    """CFractResampler::Resample (fractresampler.cpp:149-195) frame by frame.  calls: [call][frame] arrays -> [call][frame] outputs.
    restart: the running time sum starts again at zero at every call (model g)"""
    sinc, hist, ft, outs = sinc_table(), np.zeros(28, dtype=np.complex128), 0.0, []
    for ci, frames in enumerate(calls):
        if restart and ci:
            ft = 0.0
        res = []
        for fr in frames:
            n, buf, times = len(fr), np.concatenate([hist, fr]), []
            while int(ft) < n:          # the running sum, in the reference's order
                times.append(ft)
                ft += dt
            ft -= float(n)
            hist = buf[n:n + 28]
            t = np.array(times)[:, None]
            j = t.astype(np.int64) + np.arange(1, 29)[None, :]
            res.append(np.sum(buf[j] * sinc[((j - t) * 10000.0).astype(np.int64)], axis=1))
        outs.append(res)
    return outs


def rs_oracle(oracle_mod, row, audio_rate):
    """[call][frame] outputs of oracle.Receiver (USB, manual gain) over the row's calls; audio_rate 0: at the demodulator rate"""
    return DC.rs_oracle(oracle_mod, row, audio_rate)[0]


@pytest.mark.parametrize("name", [r.name for r in DC.RS_ROWS])
def test_resampler_rows_on_the_oracle(oracle_mod, name):
    """oracle.Receiver with set_audio_rate against the plain restatement of CFractResampler::Resample run over the oracle's
    demodulator-rate frames (1e-12 per 256 outputs, counts exact); at 8000 from 64 000 every frame gives exactly 256 outputs; a time
    sum that restarts at every call (g) misses the bar by 100 from the second call on wherever the sum is not zero there anyway (dt = 8
    exactly at 8000, and 2/3 at 96 000 leaves 1e-13 of a sample: those two rows cannot tell, the other four must); at 8012 the
    two-frame call has a frame of 256 and one of 257 outputs"""
    row = {r.name: r for r in DC.RS_ROWS}[name]
    assert int(oracle_mod.Decimator(row.fs, 30000).rate) == row.demod_rate
    base, want = rs_oracle(oracle_mod, row, 0), rs_oracle(oracle_mod, row, row.audio_rate)
    sf = DC.rs_superframe(oracle_mod, row) // (row.fs // row.demod_rate)
    assert [sum(len(f) for f in c) for c in base] == [k * sf for k in DC.RS_CALLS] and sf % DC.RS_FRAME == 0
    L = 2048 - (row.taps - 1)
    assert all(len(f) in (L, 2 * L) for c in base for f in c)  # (what the band-pass hands on per frame)
    dt = (row.demod_rate * 1.0) / (row.audio_rate * 1.0)
    plain, wrong = resample(base, dt), resample(base, dt, restart=True)
    counts = [[len(f) for f in c] for c in want]
    assert [[len(f) for f in c] for c in plain] == counts
    if row.audio_rate == 8000:
        assert all(len(f) == DC.RS_FRAME for c in base for f in c) and all(n == 256 for c in counts for n in c)
    if row.audio_rate == 8012:
        # ResampCore::run launches cdiv(257, 256) = 2 sub-blocks per frame in the two-frame call; the 256-output frame's second returns
        # at `sb * 256 >= nout`, the 257-output frame's second holds one lane
        assert all(len(f) == DC.RS_FRAME for c in base for f in c) and counts == [[257], [256, 257], [256]]
    assert all(abs(n - len(b) / dt) < 1 for c, cb in zip(counts, base) for n, b in zip(c, cb))
    assert (row.audio_rate > row.demod_rate) == (sum(sum(c) for c in counts) > sum(DC.RS_CALLS) * sf)
    cat = lambda calls: [np.concatenate(c) for c in calls]
    e, c, k = DC.worst_of(all_chunk_errors(cat(plain), cat(want), DC.RS_CHUNK))
    floor = signal_floor(cat(want), DC.RS_CHUNK)
    print("%s: %s outputs per frame; oracle against the plain resampler, worst chunk %.2e; least chunk RMS %.3f of the run's" % (name, sorted({n for c in counts for n in c}), e, floor))
    assert e <= EXACT and floor >= 0.01
    # the library resamples frames of 2048 samples whatever the band-pass's block: the same stream cut that way gives the same counts
    # per call and the same samples (the time sum only has whole numbers taken off it at other moments)
    by_frame = resample([[w[i:i + DC.RS_FRAME] for i in range(0, len(w), DC.RS_FRAME)] for w in cat(base)], dt)
    assert [len(w) for w in cat(by_frame)] == [len(w) for w in cat(want)]
    assert DC.worst_of(all_chunk_errors(cat(by_frame), cat(want), DC.RS_CHUNK))[0] <= 1e-9
    same_counts = [len(f) for c in wrong for f in c] == [n for c in counts for n in c]
    # (a call of the wrong model may come out a sample longer or shorter, which the GPU tier refuses by itself: cut or padded here)
    fitted = [np.concatenate([w, np.zeros(max(0, len(r) - len(w)), dtype=np.complex128)])[:len(r)] for w, r in zip(cat(wrong), cat(want))]
    errs = all_chunk_errors(fitted, cat(want), DC.RS_CHUNK)
    if row.audio_rate in (8000, 96000):
        assert same_counts and max(e for _, _, e in errs) <= DC.TOL
    else:
        print("%s, wrong model 'restart': worst chunk %.2e (bar %.0e)" % (name, check_wrong(errs, 1, name), MARGIN))
