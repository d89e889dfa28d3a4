"""GPU tier (-m gpu): the demodulator kernels against what the reference's own demodulator classes delivered, with no oracle in between.

tests/golden/refpin_demod_*.npy hold what oracle/_ref/ref_driver -- Demod_AM, Demod_SAM, Demod_NFM and Demod_WFM compiled unmodified from the
reference tree -- wrote for the cases of tests/reference_cases.py (stages demod_*): of every call the count, of the last call the last 256
complex outputs, of each earlier call the last 8, the pilot-lock pair of every stereo call and every RDS group a call delivered.  Each test
here regenerates a case's input from its recipe, feeds it through P.Demod with the case's call script and compares those values.  Nothing
here reads the reference tree or the binary.

Bars, the suite's own (tests/test_parity_gpu.py): 1e-5 relative RMS for AM, NFM, WFM mono and WFM stereo.  The 8-sample snippets of earlier
calls are compared by the RMS of their absolute error against the RMS of the tail of the last call: a relative RMS over 8 samples of their
own level means nothing.  Counts, lock flags and RDS groups are compared exactly.

SAM: the in-phase form (re + im) / 2 at 1e-4 and at max(1e-5, 3 x own), as test_sam_pll_demod_step; the quadrature path is not compared
sample by sample.  One figure per case: the relative RMS over everything the fixture keeps (the tail and the snippets pooled).  own is
what the CPU oracle misses against itself over the same samples when its input is rounded to single precision, the device's input
format.  The loop is chaotic, so one such run is one draw: rounding alone gives 8e-6 on demod_sam_down_48000 where the same input scaled
by 1 + 3e-8 .. 1 + 2.1e-7 before rounding gives 4e-5 to 5.6e-5 (CPU, seven draws).  own is therefore the largest of eight draws, the plain
rounding and those seven.

A loop out of lock cannot be followed from single-precision input at all (the oracle misses itself by 1e-3 .. 2 there): the SAM cases
"slip" and "clamp", and NFM 16 kHz off at 37 500, are compared over the first 256 samples of the first call, which their fixtures keep
(reference_cases._demod_rows has the figures).
"""
import numpy as np
import pytest

from tests import reference_cases as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
SAM_BAR = 1e-4
CASES = [c for c in R.cases() if c.stage.startswith("demod_")]
NARROW = [c.name for c in CASES if c.stage in ("demod_am", "demod_nfm")]
SAM = [c.name for c in CASES if c.stage == "demod_sam"]
MONO = [c.name for c in CASES if c.stage == "demod_wfm_mono"]
STEREO = [c.name for c in CASES if c.stage == "demod_wfm_stereo"]


def _case(name):
    return next(c for c in CASES if c.name == name)


def _cpx(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.complex128)


def _rms(v):
    return float(np.sqrt(np.mean(np.abs(v) ** 2)))


def _rel(got, want):
    return _rms(np.asarray(got) - np.asarray(want)) / max(_rms(want), 1e-12)


def _run(case, wfm):
    """the case's input through P.Demod with its call script -> the device's output of every call"""
    import pebblesdr_amd as P
    m = case.meta
    d = P.Demod(64000, m["rate"], R.DEMOD_N) if wfm else P.Demod(m["rate"], 256000, R.DEMOD_N)
    d.setDemodMode({"AM": P.DM_AM, "SAM": P.DM_SAM, "FMN": P.DM_FMN, "FMM": P.DM_FMM, "FMS": P.DM_FMS}[m["mode"]])
    out = []
    for k, blk in enumerate(R._split(case.make_input(), m["calls"])):
        if m.get("bw") and m["bw"][k]:
            d.setBandwidth(m["bw"][k])
        out.append(np.array(d.processBlock(blk)))
    return d, out


def _compare_calls(name, got, want, form, bar_of):
    """got: the device's output per call; want: [(full length, kept tail)] per call, interleaved; form: what of a complex block is compared;
    bar_of(call, slice): the bar for that stretch.  The last call by relative RMS, the earlier ones by absolute RMS against the tail's"""
    assert [2 * len(g) for g in got] == [n for n, _ in want], name
    last = len(got) - 1
    tail = form(_cpx(want[last][1]))
    e = _rel(form(got[last][-len(tail):]), tail)
    print("%s: tail of call %d: %.3e (bar %.3e)" % (name, last, e, bar_of(last, len(tail))))
    worst = [(e, bar_of(last, len(tail)), last)]
    for k in range(last):
        w = form(_cpx(want[k][1]))
        e = _rms(form(got[k][-len(w):]) - w) / _rms(tail)
        print("%s: end of call %d: %.3e (bar %.3e)" % (name, k, e, bar_of(k, len(w))))
        worst.append((e, bar_of(k, len(w)), k))
    for e, bar, k in worst:
        assert e <= bar, (name, "call %d: %.3e over %.3e" % (k, e, bar))


def _compare_head(name, got, want, form, bar):
    """a head_view fixture: the counts of every call, and the first R.HEAD samples of the first call"""
    assert [2 * len(g) for g in got] == [n for n, _ in want[:-1]], name
    head = form(_cpx(want[-1][1]))
    assert len(head) == R.HEAD
    e = _rel(form(got[0][:R.HEAD]), head)
    print("%s: head of call 0: %.3e (bar %.3e)" % (name, e, bar))
    assert e <= bar, (name, e, bar)


@pytest.mark.parametrize("name", NARROW)
def test_am_and_nfm_against_the_recorded_reference(gpu_lib, name):
    case = _case(name)
    _, got = _run(case, wfm=False)
    want = R.expand(np.load(case.fixture))
    if case.stage == "demod_nfm":
        assert all(np.all(g.imag == 0) for g in got)     # out[i] = <real> assigns imag 0 and the CFir keeps it 0
    if case.meta.get("head"):
        _compare_head(name, got, want, lambda z: z, TOL)
    else:
        _compare_calls(name, got, want, lambda z: z, lambda k, n: TOL)


@pytest.mark.parametrize("name", SAM)
def test_sam_against_the_recorded_reference(gpu_lib, oracle_mod, name):
    case = _case(name)
    m = case.meta
    x = case.make_input()
    _, got = _run(case, wfm=False)
    want = R.expand(np.load(case.fixture))
    ip = lambda z: (z.real + z.imag) / 2

    def oracle_run(scale, single):
        d = oracle_mod.DemodSAM(m["rate"])
        return [d.process((blk * scale).astype(np.complex64) if single else blk) for blk in R._split(x, m["calls"])]
    if m["head"]:
        own = _rel(ip(oracle_run(1.0, True)[0][:R.HEAD]), ip(oracle_run(1.0, False)[0][:R.HEAD]))
        _compare_head(name, got, want, ip, min(SAM_BAR, max(TOL, 3 * own)))
        return
    assert [2 * len(g) for g in got] == [n for n, _ in want], name
    kept = lambda ys: np.concatenate([ip(np.asarray(y)[-len(t) // 2:]) for y, (_, t) in zip(ys, want)])
    ref = np.concatenate([ip(_cpx(t)) for _, t in want])
    # own is taken against the recorded reference itself (the oracle on the samples as they are equals it: tests/test_reference_pins.py)
    own =max(_rel(kept(oracle_run(1.0 + k * 3e-8, True)), ref) for k in range(8))
    e = _rel(kept(got), ref)
    print("%s: kept samples pooled: %.3e (own %.3e)" % (name, e, own))
    assert own > 1e-7                                      # (it IS sensitive: a linear demodulator would read ~3e-8 here)
    assert e <= max(TOL, 3 * own) and e <= SAM_BAR, (name, e, own)


@pytest.mark.parametrize("name", MONO)
def test_wfm_mono_against_the_recorded_reference(gpu_lib, name):
    case = _case(name)
    _, got = _run(case, wfm=True)
    recs = R.expand(np.load(case.fixture))
    counts, want = recs[0::2], recs[1::2]
    assert [len(g) for g in got] == [int(t[0]) for _, t in counts], name
    _compare_calls(name, got, want, lambda z: z, lambda k, n: TOL)


@pytest.mark.parametrize("name", STEREO)
def test_wfm_stereo_and_rds_against_the_recorded_reference(gpu_lib, name):
    """the lock pair Demod_WFM::getStereoLock delivered behind every call, the audio of the calls the fixture keeps (both channels), and
    the groups Demod::fmStereo's one getNextRdsGroupData per call took from the queue, with the function's return values"""
    import pebblesdr_amd as P
    case = _case(name)
    m = case.meta
    fx = R.stereo_fixture(case)
    d = P.Demod(64000, m["rate"], R.DEMOD_N)
    d.setDemodMode(P.DM_FMS)
    got, locks = {}, []
    for k, blk in enumerate(R._split(case.make_input(), m["calls"])):
        g = d.processBlock(blk)
        assert len(g) == int(fx["counts"][k]), (name, k)
        lock, changed = d.getStereoLock()
        locks.append((float(bool(changed)), float(bool(lock))))
        if k in fx["audio"]:
            got[k] = np.array(g)
    assert locks == [tuple(r) for r in fx["locks"].tolist()], (name, locks)
    last = len(m["calls"]) - 1
    tail = _cpx(fx["audio"][last])
    for ch, part in (("left", np.real), ("right", np.imag)):
        e = _rel(part(got[last][-len(tail):]), part(tail))
        print("%s: tail of call %d, %s: %.3e" % (name, last, ch, e))
        assert e <= TOL, (name, ch, e)
    for k in sorted(fx["audio"]):
        if k != last:
            w = _cpx(fx["audio"][k])
            e = _rms(got[k][-len(w):] - w) / _rms(tail)
            print("%s: end of call %d: %.3e" % (name, k, e))
            assert e <= TOL, (name, k, e)
    words, flags = d.getNextRdsGroupData()
    want = [fx["groups"][k] for k in sorted(fx["groups"])]
    assert [tuple(int(v) for v in row) for row in words] == [g[1:] for g in want], name
    assert [int(bool(f)) for f in flags] == [g[0] for g in want], name
    if m["rds"]:
        assert len(want) >= 3 and all(g[1] != 0 for g in want)
    else:
        assert want == []
