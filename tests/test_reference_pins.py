"""Pins the CPU oracle (oracle/pebble_oracle.c) to the reference's own code, stage by stage.

oracle/_ref/ref_driver is the reference's DSP classes compiled unmodified from the reference tree against stand-in Qt and
Accelerate headers (oracle/ref_build/).  Each case (tests/reference_cases.py) generates its input from a recipe, runs the
reference class and the oracle's counterpart on the same float64 samples and compares every output record: counts, chain
tables, coefficients, state scalars and samples.

With the binary present a test compares reference, oracle and the recorded fixture tests/golden/refpin_<case>.npy, all
three.  Without it and without a reference tree (a clean checkout elsewhere, the GPU machine) it compares oracle and
fixture.  A binary that is present but does not run fails the test.  tools/record_reference_pins.py rewrites the fixtures.

WHAT IS PINNED.  The Accelerate stand-in is this project's code (plain loops, left-to-right sums, a textbook radix-2 DFT),
so these tests pin the reference's code AROUND the DFT and the strided FIR, not those two primitives: the window, scaling,
unfold and dB averaging of the spectrum, the filter designs, the overlap-save bookkeeping of FastFIR, the decimator's chain
selection, delay lines and short-frame fallback, and every serial fp64 stage whole (mixer, CDownConvert, CFir, CIir, the
resampler, AGC, the blankers, ANF, IQBalance, DCRemoval, fdEstimate).  The Morse restatement (tests/morse_ref.py) is held to the
pebblelib classes the modem is made of, driven the way morse.cpp:160-246 and :761-894 drive them: GoertzelOOK with TH_PEAK at the four
modem rates of tests/morse_cases.py and both tones, the tone moved on a running filter (powers, decisions, peak averages, the count
left in the block), SampleClock::uSecDelta, MovingAvgFilter(8).  FFT::mapFFTToScreen is pinned on every row of tests/screen_cases.py whose
float -> int conversions are all in range (cases mapscreen_*, one dB row in, the pixels out, exact).  The two primitives are cross-checked once each through
reference code that does not use the stand-in: the decimator through HalfbandFilter::process (decimator.cpp:661-685) and the
spectrum through the in-tree Ooura transform (magnitudes only: FastFIR is mirrored on that back end).

MEASURED (CPU, both sides fp64, same libm, contraction off): every case is bit for bit, so equality is asserted, except
  spectrum through Ooura against the oracle: max 1.01e-10 dB, bar 1.1e-9 dB (ten times; the ceiling is 1e-6 dB).
  every demodulator case: bit for bit, bar 0 -- the two WFM loops too, where the reference runs x87 fsincos (demod_wfm.cpp:400, :550)
  and the oracle sin and cos of the C library.
No bar may exceed 1e-9 relative RMS or 1e-6 dB (reference_cases.MAX_BAR, MAX_BAR_DB).
Sensitivity of the demodulator pins, each a one-token change of the oracle on a scratch copy: 0.9999f -> 0.9999 in AM fails both AM
cases (3.7e-5, 7.4e-5); cosf / sinf -> cos / sin in SAM fails all twelve (8.6e-9 .. 4.0e-2); NFM's beta from the float product to a
double product fails all nine (2.4e-8 .. 1.6e-1).

The demodulators (application/demod/, cases demod_*): Demod_AM::processBlockFiltered with setBandwidth between calls, Demod_SAM::processBlock,
Demod_NFM::processBlockNCO, Demod_WFM::processDataMono and processDataStereo with getStereoLock and one getNextRdsGroupData behind each
call, driven as Demod::processBlock, fmMono and fmStereo drive them (demod.cpp:100-141, :169-226) with ragged call lengths, at the rates
the library runs: the float loop state of SAM and NFM sample for sample, the pilot loop's lock sequence, the RDS branch up to the group
queue (groups word for word).  Their base class Demod is two lines of this project's own in the driver; a SAM or NFM case's oracle
function asserts from the oracle's loop state that the branch its input is there for was reached.

The Morse decoder proper (plugins/MorseDigitalModem/morse.cpp and morsecode.cpp, compiled unmodified against stand-in widgets; cases
morse_hard_*, morse_stream_64000): Morse() + setSampleRate, then processBlock frame by frame, setDemodMode and setSampleRate again where
a row says so.  The plugin's signals are plain member calls whose bodies the driver defines: testbench() gives the power and decision of
every Goertzel result, newOutput() the sample and the dot-dash buffer of every output (the token, also where the plugin prints '*'),
and the members give the estimate, the range flags, the modem rate, N and the five thresholds at every reading.  The restatement
(init, updateThresholds, stateMachine, findBestGoertzelN, setSampleRate) is held to it on every row of tests/morse_hard_cases.py at
64 000 / 2048 (the merged 11-tap stage), on one row each at 8000 (no stage), 12 000 (one stage) and 31 250 (modem rate 7812 of 7812.5),
and on tests/morse_cases.py's stream: decisions, events, starred events and statuses exact, powers bit for bit (bar 0).  The constructor
leaves m_wpmSpeedCurrent, the range limits and the state unset and setSampleRate reads them; the driver builds the object over zeroed
memory and writes m_wpmSpeedCurrent = 20 and the class's default limits (10 / 50) into it: the first call is this project's choice, not
the reference's doing; every later setSampleRate, which finds what the plugin left there, is pinned (row mode_rate_midchar).
The Morse sender (plugins/MorseGenDevice/morsegen.cpp; cases morsegen_*): setParams, setTextOut, nextOutputSample at the speeds and rise
times of tests/test_morsegen_host.py and with samplesPerTcw barely above the rise: sample counts and mark boundaries exact, samples to
one unit in the last place (measured 4.0e-18 relative RMS: a handful of cos / sin values, see reference_cases.MORSEGEN_BAR).

NOT PINNED: CRdsDecode; Demod::processBlock's dispatch itself (demod.cpp brings the GUI; the driver restates it by its call sequence);
the Morse plugin's panel code (setupDataUi, refreshOutput, the slider slots: compiled, never run) and its C_FIR_filter path
(m_useGoertzel is true); the two vDSP primitives themselves; CFastFIR at 8192/4097 (its sizes are #defines inside fastfir.cpp, so the
variant cannot be built from the unmodified source).

FOUND BY THESE PINS: FFT::m_isOverload is a member that only whole buffers rewrite; the oracle returned 0 for a short
frame after an overloaded whole one (case spectrum_overload_then_short).  Fixed in the oracle and in the device's spectrum step.
pebblelib's c_j is {6.123233995736766e-17, 1} (cpx.h:158), so Goertzel's c_C and c_D have a modulus of exp(-6.1e-17 A (N - 1)), up to
3e-14 under 1; the Morse restatement had {0, 1} and its powers came out 5e-14 off (cases morse_goertzel_*).  Fixed in the restatement and
in MorseCore::init's coefficients; bit for bit since.
fdEstimate divides 0 by 0 where a window has no noise bin or no bin at all, and bounds the NaN with qBound, which Qt words so that a NaN
comes out as the LOWER bound (-120 dB; 0 for snr).  The oracle and the device let the NaN through, and the stand-in qMin, worded the
other way round, returned the UPPER bound (cases fdestimate_* of tests/strength_cases.py: bp0_one_bin, bp0_no_bin, all_in_band,
inverted).  Fixed in the stand-in, the oracle (po_db_clip, the snr bound) and the device's strength_finish; the 80 earlier pins did not
move.  The wording of qMin / qMax / qBound is Qt's published qglobal.h as remembered, not checked against an installed Qt.
The Morse decoder and sender pins (above) found no defect: restatement, recorded reference and device agree on every row.
Demod_NFM's DC average, m_pllFreqErrorDC = (1.0 - m_pllDcAlpha) * m_pllFreqErrorDC + m_pllDcAlpha * m_ncoFrequency (demod_nfm.cpp:249): the
first product has a double factor and is a double product, the second multiplies two floats and is a FLOAT product, rounded before the sum.
The oracle and k_pll_demod had a double product there: 1e-8 to 3e-7 of the output off the binary, first at sample 20 to 1734 (all nine
cases demod_nfm_*).  Fixed in both; the 144 earlier fixtures did not move.
"""
import os

import numpy as np
import pytest

from tests import reference_cases as R

NAMES = [c.name for c in R.cases()]


def _have_binary():
    return os.path.exists(R.BINARY)


def _check(case, kinds, got, want, what):
    """got / want: lists of arrays with equal record structure"""
    assert len(got) == len(want) == len(kinds), (case.name, what, len(got), len(want))
    worst = 0.0
    for i, (k, g, w) in enumerate(zip(kinds, got, want)):
        assert len(g) == len(w), (case.name, what, "record %d: %d values against %d" % (i, len(g), len(w)))
        e = R.record_error(k, g, w)
        worst = max(worst, e)
        assert e <= case.allowed(k), (case.name, what, "record %d kind %s: error %.3e over %.3e" % (i, k, e, case.allowed(k)))
    return worst


def _check_fixture(case, kinds, records, what):
    fixture = R.expand(np.load(case.fixture))
    kept = case.view(list(zip(kinds, records)))
    kinds, records = [k for k, _ in kept], [v for _, v in kept]
    mine = R.expand(R.compress(records))
    assert [n for n, _ in mine] == [n for n, _ in fixture], (case.name, what, "record lengths")
    return _check(case, kinds, [t for _, t in mine], [t for _, t in fixture], what)


@pytest.mark.parametrize("name", NAMES)
def test_reference_pin(oracle_mod, name):
    case = next(c for c in R.cases() if c.name == name)
    x = case.make_input()
    orc = case.oracle(oracle_mod, x)
    kinds = [k for k, _ in orc]
    orc = [np.asarray(v, dtype=np.float64) for _, v in orc]
    e_fix = _check_fixture(case, kinds, orc, "oracle against fixture")
    if _have_binary():
        ref = case.reference(x)
        e_ref = _check(case, kinds, orc, ref, "oracle against reference binary")
        _check_fixture(case, kinds, ref, "reference binary against fixture")
        print("%s: oracle against reference %.3e, against fixture %.3e" % (name, e_ref, e_fix))
    else:
        print("%s: oracle against fixture %.3e (no reference binary)" % (name, e_fix))


def test_every_stage_of_the_table_has_a_case():
    stages = {c.stage for c in R.cases()}
    assert stages == {"mixer", "decimator", "downconvert", "fastfir", "fir", "iir", "resampler", "spectrum", "agc", "nb", "anf",
                      "iqbalance", "dcremoval", "fdestimate", "goertzel", "sampleclock", "movingavg", "mapscreen", "demod_am", "demod_sam", "demod_nfm", "demod_wfm_mono",
                      "demod_wfm_stereo", "morse", "morsegen"}
    assert all(c.bar <= R.MAX_BAR and c.bar_db <= R.MAX_BAR_DB for c in R.cases())
    assert all(os.path.getsize(c.fixture) < 16384 for c in R.cases())


def test_every_recorded_signal_strength_is_finite(oracle_mod):
    """fdEstimate's qBound turns 0 / 0 into its lower bound: no fixture, no oracle value and no value of the binary is NaN or inf, and
    the rows whose class makes a value a bound hold exactly that bound"""
    from tests import strength_cases as S
    seen = 0
    for case in R.cases():
        if case.stage != "fdestimate":
            continue
        x = case.make_input()
        sets = [[t for _, t in R.expand(np.load(case.fixture))], [v for _, v in case.oracle(oracle_mod, x)]]
        if _have_binary():
            sets.append(case.reference(x))
        for records in sets:
            for rec in records:
                assert len(rec) == 5 and np.isfinite(rec).all(), (case.name, rec)
                if case.name.startswith("fdestimate_"):
                    for k, v in S.expected(S.row(case.name[len("fdestimate_"):])[6]).items():
                        assert rec[k] == v, (case.name, k, rec)
                    assert rec[4] == rec[1]
        seen += 1
    assert seen == 1 + len(S.ROWS)


def test_chain_tables_of_the_reference_equal_the_recorded_ones(oracle_mod):
    """Decimator::buildDecimationChain of the reference binary for every row of tests/golden/chains.json (the rows the oracle is held
    to by test_oracle_pins.test_decimation_chains_match_survey).  Needs the binary; without it the rows stay pinned to the oracle only."""
    rows = R.chains_table()
    for row in rows:
        d = oracle_mod.Decimator(row["fs"], row["bw"])
        assert [list(c) for c in d.chain()] == row["chain"] and d.rate == row["rate"] and d.dec_by2_stages == row["stages"]
        if _have_binary():
            rec = R.run_driver("decimator", np.zeros(0, dtype=np.complex128), [row["fs"], row["bw"], 2048, 0])
            assert rec[0][0] == row["rate"], row
            assert rec[1][0] == row["stages"], row
            assert rec[2].reshape(-1, 2).astype(int).tolist() == row["chain"], row
            assert int(np.prod(rec[2].reshape(-1, 2)[:, 1])) == row["D"], row


def test_short_frame_fallback_of_the_reference_passes_a_constant_through(oracle_mod):
    """The known answer of test_oracle_pins.test_decimator_short_frame_fallback_known_answer, on the reference binary: 20 Msps / 30 kHz
    with 2048-sample frames ends in two dropping stages, 4 samples out, a constant input passed through (first call: inside the filters'
    transient the value is not reached yet, so only count and agreement with the oracle are asserted there; the count is the answer)."""
    x = np.full(2048, 0.25 + 0.5j)
    d = oracle_mod.Decimator(20000000, 30000)
    y = d.process(x)
    assert len(y) == 4
    if _have_binary():
        rec = R.run_driver("decimator", x, [20000000, 30000, 2048, 0])
        assert len(rec) == 4 and len(rec[3]) == 8
        assert np.array_equal(rec[3], y.view(np.float64))
