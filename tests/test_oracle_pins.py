"""Pins the CPU oracle (oracle/pebble_oracle.c) to every known answer the reference offers.

The reference has no test suite and no golden files.  What exists:
  (1) the worked table in pebblelib/fft.cpp:363-369 (-10 dB test tone, 1 Msps, peak dB per FFT size);
  (2) outputs of the reference itself recorded when its sources were executed at survey time
      (SURVEY.md section 10): chain tables, stage counts, tap counts, oscillator fixed point, FastFIR gain;
  (3) closed forms and independent implementations (numpy.fft, scipy.signal) for everything else.
Stages pinned only by (3) say "parity unpinned" below: they are checked for self-consistency, not against
reference output.  Since then tests/test_reference_pins.py compares the time-domain stages with the reference's own
code, compiled with stand-ins; the docstrings below point at its cases.
"""
import json
import os

import numpy as np
import pytest
import scipy.signal as ss

from tests.signals import lcg_noise, tones

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_fft_cpp_known_answer_table(oracle_mod):
    """pebblelib/fft.cpp:363-369: '-10db testbench signal, 1msps': fftSize -> maxDB.
    The tone frequency is not recorded; the TestBench spin box is integer kHz (testbench.cpp:369).  A single
    integer-kHz tone must reproduce ALL FIVE rows, including the repeated -10.0096 at 8192 and 16384."""
    O = oracle_mod
    table = json.load(open(os.path.join(GOLD, "fft_cpp_table.json")))
    fs, n = 1e6, 2048
    rows = {int(k): v for k, v in table["rows"].items()}
    hits = []
    for fk in table["candidate_khz"]:
        x = tones(fs, 2 * n, [(10 ** (-10 / 20), fk * 1000.0)])
        worst = 0.0
        for bins, want in rows.items():
            s = O.Spectrum(bins, n)
            s.process(x[:n])                      # frame 0 averages with the (zeroed) previous buffer
            got = s.process(x[n:]).max()          # steady state from frame 1 on
            worst = max(worst, abs(got - want))
        if worst < 6e-5:                          # the table is printed to 4 decimals
            hits.append(fk)
    assert hits, "no integer-kHz tone reproduces the reference's table"
    assert 48 in hits and 77 in hits  # recorded when the oracle was first pinned


def test_decimation_chains_match_survey(oracle_mod):
    """chains replayed from Decimator::buildDecimationChain (decimator.cpp:64-149)."""
    O = oracle_mod
    exp = json.load(open(os.path.join(GOLD, "chains.json")))
    for row in exp:
        d = O.Decimator(row["fs"], row["bw"])
        assert d.rate == row["rate"], row
        assert d.dec_by2_stages == row["stages"], row
        assert d.total_decimation == row["D"], row
        assert [list(c) for c in d.chain()] == row["chain"], row


def test_decimator_frame_geometry(oracle_mod):
    """2.048 Msps / 30 kHz -> 64 kHz, 5 stages, 64 samples out per 2048 in."""
    d = oracle_mod.Decimator(2048000, 30000)
    y = d.process(np.ones(2048, dtype=complex))
    assert len(y) == 64 and d.rate == 64000.0 and d.dec_by2_stages == 5


def test_decimator_is_frame_invariant(oracle_mod):
    """With every stage seeing >= its tap count the cascade is a streaming multirate filter: frame size must not
    matter.  This is the property that lets the GPU process super-frames."""
    O = oracle_mod
    x = tones(2048000, 16 * 2048, [(0.5, 5000.0), (0.3, 700e3)]) + lcg_noise(16 * 2048, 9, 0.01)
    a = O.Decimator(2048000, 30000)
    b = O.Decimator(2048000, 30000)
    ya = np.concatenate([a.process(x[i * 2048:(i + 1) * 2048]) for i in range(16)])
    yb = np.concatenate([b.process(x[i * 8192:(i + 1) * 8192]) for i in range(4)])
    assert np.array_equal(ya, yb)


def test_decimator_matches_scipy_polyphase(oracle_mod):
    """(parity with the reference binary: tests/test_reference_pins.py, decimator_*)  Each halfband stage is y[n] = sum_p x[nS+p-(T-1)] h[p]; check the
    cascade against scipy.signal.lfilter + slicing in fp64."""
    O = oracle_mod
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "oracle", "hb_taps.h")).read()
    taps = {}
    for m in re.finditer(r'\{ "(\w+)", (\d+), ([0-9.]+), \{ ([^}]*) \} \}', txt):
        taps[int(m.group(2))] = np.array([float(v) for v in m.group(4).split(",")])
    d = O.Decimator(2048000, 30000)
    x = lcg_noise(8 * 2048, 4, 1.0)
    y = np.concatenate([d.process(x[i * 2048:(i + 1) * 2048]) for i in range(8)])
    z = x
    for nt, stride in d.chain():
        h = taps[nt]
        f = ss.lfilter(h[::-1], [1.0], z)  # sum_p x[i+p-(T-1)] h[p] = sum_k x[i-k] h[T-1-k]
        z = f[::stride]
    assert np.abs(y - z).max() < 1e-13


def test_decimator_short_frame_fallback_known_answer(oracle_mod):
    """decimator.cpp:602-625: a stage that sees fewer samples than taps stops filtering and drops samples.
    20 Msps / 30 kHz with 2048-sample frames: cic3 x4 -> 512, hb11 x16 -> 32, then 32 >= 15 taps ok -> 16,
    16 < 27 taps: dropping -> 8, 8 < 59: dropping -> 4.  Known answer: with a constant input the dropping stages
    pass the value through untouched."""
    d = oracle_mod.Decimator(20000000, 30000)
    assert d.chain() == [(0, 4), (11, 16), (15, 2), (27, 2), (59, 2)]
    y = None
    for _ in range(40):
        y = d.process(np.full(2048, 0.25 + 0.5j))
    assert len(y) == 4
    # CIC3 DC gain 1, halfband DC gain 1 (taps sum to ~1), dropping stages gain 1
    assert np.allclose(y, 0.25 + 0.5j, rtol=0, atol=2e-4)


def test_mixer_fixed_point_and_closed_form(oracle_mod):
    """a_inf = 0.974679434480897 = sqrt(0.95); osc_i = a_i exp(j(i+1)inc), max diff ~8e-13."""
    O = oracle_mod
    m = O.Mixer(2048000)
    m.set_frequency(100000.0)
    n = 8 * 2048
    y = m.process(np.ones(n, dtype=complex))
    assert abs(abs(y[-1]) - 0.974679434480897) < 2e-15
    a = np.empty(n)
    a[0] = 1.0
    for i in range(1, n):
        a[i] = a[i - 1] * (1.95 - a[i - 1] ** 2)
    cf = a * np.exp(1j * (np.arange(n) + 1) * (2 * np.pi * -100000.0 / 2048000))
    assert np.abs(y - cf).max() < 5e-12
    # retune resets phase and amplitude (mixer.cpp:37-38); f == 0 returns the input (mixer.cpp:51-53)
    m.set_frequency(-5000.0)
    y2 = m.process(np.ones(4, dtype=complex))
    assert abs(abs(y2[0]) - 1.0) < 1e-15 and abs(abs(y2[1]) - 0.95) < 1e-15
    m.set_frequency(0.0)
    x = lcg_noise(16, 1, 1.0)
    assert np.array_equal(m.process(x), x)


def test_fastfir_known_answers(oracle_mod):
    """ProcessData(2048) returns 2048; unity pass-band gain (0.4873 in -> 0.4873 out);
    per-sample phase step +0.09817 for a +1 kHz tone at 64 kHz (Accelerate semantics, not the mirrored Ooura/cute)."""
    O = oracle_mod
    f = O.FastFIR()
    assert f.setup(300, 3000, 0, 64000) == 0
    x = tones(64000, 4096, [(0.4873, 1000.0)])
    y0 = f.process(x[:2048])
    y1 = f.process(x[2048:])
    assert len(y0) == 2048 and len(y1) == 2048
    assert abs(abs(y1[-1]) - 0.4873) < 2e-5
    assert abs(np.angle(y1[-1] / y1[-2]) - 0.09817477) < 1e-7
    # "Filter Parameter error" keeps the previous taps (fastfir.cpp:208-216)
    H = f.coef()
    assert f.setup(3000, 300, 0, 64000) == -1
    assert np.array_equal(f.coef(), H)


def test_fastfir_equals_direct_convolution(oracle_mod):
    """(parity with the reference binary: tests/test_reference_pins.py, fastfir_*)  Overlap-save must equal y[n] = sum_k h[k] x[n-k] with h = IFFT(H)*N... i.e.
    the designed taps; checked with scipy in fp64."""
    O = oracle_mod
    f = O.FastFIR()
    f.setup(-5000, 5000, 0, 64000)
    h = np.fft.ifft(f.coef()) * 1.0  # H holds taps/2048 transformed unscaled: ifft gives taps/2048
    x = lcg_noise(3 * 2048, 7, 1.0)
    y = np.concatenate([f.process(x[i * 2048:(i + 1) * 2048]) for i in range(3)])
    z = ss.lfilter(h[:1025] * 2048, [1.0], x)
    assert np.abs(y - z).max() < 1e-11


def test_po_fft_matches_numpy(oracle_mod):
    x = lcg_noise(8192, 11, 1.0)
    assert np.abs(oracle_mod.fft(x) - np.fft.fft(x)).max() < 1e-10
    assert np.abs(oracle_mod.fft(x, inverse=True) - np.fft.ifft(x) * 8192).max() < 1e-10


def test_cfir_tap_counts_match_survey(oracle_mod):
    """AM bw 10k @ 64k -> 24 taps (ctor default 16k -> 15); WFM 15k/21k @ 256k or 312.5k -> 75."""
    O = oracle_mod
    assert O.DemodAM(64000, 10000).ntaps == 24
    assert O.DemodAM(64000).ntaps == 15
    assert O.DemodWFM(256000).ntaps == 75
    assert O.DemodWFM(312500).ntaps == 75


def test_cfir_and_ciir_match_scipy(oracle_mod):
    """(parity with the reference binary: tests/test_reference_pins.py, fir_* and iir_*)  CFir's circular delay line and CIir's DF2
    against scipy.signal.lfilter."""
    O = oracle_mod
    x = lcg_noise(5000, 5, 1.0)
    f = O.Fir()
    f.init_lp(0, 1.0, 50.0, 10000, 18000, 64000)
    y = np.concatenate([f.process(x[:1234]), f.process(x[1234:])])
    z = ss.lfilter(f.taps(), [1.0], x)
    assert np.abs(y - z).max() < 1e-13
    q = O.Iir("br", 19000, 5, 256000)
    b0, b1, b2, a1, a2 = q.coeffs()
    y = np.concatenate([q.process(x[:777]), q.process(x[777:])])
    z = ss.lfilter([b0, b1, b2], [1.0, a1, a2], x)
    assert np.abs(y - z).max() < 1e-12


def test_nfm_pll_recovers_the_modulation(oracle_mod):
    """closed-form check of Demod_NFM (pinned to the reference's class since: tests/test_reference_pins.py, cases demod_nfm_*) -- a 1 kHz tone with 3 kHz deviation comes out as a 1 kHz sine of
    amplitude 2*pi*3000/fs (the PLL output is NCO frequency in rad/sample) within the 75-tap CFir's pass-band ripple."""
    fs, n = 64000, 16384
    t = np.arange(n) / fs
    x = 0.3 * np.exp(1j * 3.0 * np.sin(2 * np.pi * 1000 * t))
    d = oracle_mod.DemodNFM(fs)
    assert d.ntaps == 75
    y = d.process(x)
    assert np.all(y.imag == 0)
    amp = np.abs(np.fft.rfft(y.real[8192:] * np.hanning(8192)))[128] / (8192 / 4)
    assert abs(amp - 2 * np.pi * 3000 / fs) / (2 * np.pi * 3000 / fs) < 0.06


def test_sam_reference_algorithm_is_chaotic(oracle_mod):
    """Demod_SAM keeps its PLL phase and frequency in `float` (demod_sam.h:19-25).  Its trajectory is chaotic at the
    last-bit level: perturbing the INPUT by 1e-9 (relative) moves the oracle's own in-phase output by > 1e-6 and
    decorrelates the quadrature path, while 1e-12 (below the float state's resolution) changes nothing.  This is why
    the GPU parity bar for SAM is looser than 1e-5 (tests/test_parity_gpu.py::test_sam_pll_demod_step)."""
    fs, n = 64000, 6 * 2048
    t = np.arange(n) / fs
    am = (0.3 * (1 + 0.5 * np.cos(2 * np.pi * 800 * t))) * np.exp(2j * np.pi * 30 * t) + lcg_noise(n, 8, 1e-3)
    a = oracle_mod.DemodSAM(fs).process(am)
    rr = lambda p, q: np.sqrt(np.mean(np.abs(p - q) ** 2)) / np.sqrt(np.mean(np.abs(q) ** 2))
    ip = lambda z: (z.real + z.imag) / 2
    qp = lambda z: (z.real - z.imag) / 2
    b = oracle_mod.DemodSAM(fs).process(am * (1 + 1e-12))
    assert rr(ip(b), ip(a)) < 1e-10 and rr(qp(b), qp(a)) < 1e-10
    c = oracle_mod.DemodSAM(fs).process(am * (1 + 1e-9))
    assert rr(ip(c), ip(a)) > 1e-6 and rr(qp(c), qp(a)) > 1e-2
    # the demodulated audio itself is there: 800 Hz at half the carrier level in the in-phase path
    spec = np.abs(np.fft.rfft(ip(a)[4096:4096 + 8192] * np.hanning(8192)))
    assert int(np.argmax(spec[10:])) + 10 in (102, 103)


def test_spectrum_window_and_gain(oracle_mod):
    """windowfunction.cpp:214-235: coherentGain ~ 0.35875 ("SB 0.36"); a bin-centred -10 dBFS tone reads -10.000 dB at any size."""
    O = oracle_mod
    s = O.Spectrum(4096, 2048)
    assert abs(s.coherent_gain - 0.35875) < 1e-6
    x = tones(2048000, 4096, [(10 ** (-10 / 20), 2048000 * 100 / 2048)])
    s.process(x[:2048])
    db = s.process(x[2048:])
    assert abs(db.max() + 10.0) < 1e-6
    assert int(np.argmax(db)) == 2048 + 200  # -f..+f order, fft.cpp:207-213
    assert db.min() >= -120.0 and db.max() <= 0.0


def test_receiver_chain_skeleton(oracle_mod):
    """processIQData bookkeeping: audio appears every D-th frame; gain restore 10^(2*5/20); USB is a pass-through of the band-pass."""
    O = oracle_mod
    r = O.Receiver(2048000, 2048, 4096)
    r.set_mode(O.USB)
    r.set_mixer(100e3)
    r.set_filter(300, 3000)
    assert r.demod_rate() == 64000 and r.dec_stages() == 5
    x = tones(2048000, 64 * 2048, [(0.1, 101e3)])
    outs = [r.process(x[i * 2048:(i + 1) * 2048])[0] for i in range(64)]
    lens = [len(o) for o in outs]
    assert lens == ([0] * 31 + [2048]) * 2
    y = outs[63]
    # tone at +1 kHz after mixing: amplitude 0.1 * sqrt(.95) (mixer) * halfband DC~1 * 10^(10/20) (gain restore)
    assert abs(abs(y[-1]) - 0.1 * np.sqrt(0.95) * 10 ** 0.5) < 2e-4
    assert abs(np.angle(y[-1] / y[-2]) - 2 * np.pi * 1000 / 64000) < 1e-6


# ------------------------------------------------------------------------------------------------
# AGC and CFractResampler restatements: the reference holds no recorded values for these two classes ("parity
# unpinned"), so these are closed-form properties of the algorithms as written.
# ------------------------------------------------------------------------------------------------
def test_resampler_reproduces_a_delayed_tone_and_carries_its_clock(oracle_mod):
    """Outputs are the input evaluated at t_k = k*rate - 14 input samples (the sinc table is centred on its 28 taps) to
    the table's resolution (10000 points per zero crossing -> ~1e-6); the fractional clock carries across calls, so the
    output counts of successive 2048-sample frames sum to floor-consistent totals."""
    O = oracle_mod
    fs, rate = 62500.0, 62500.0 / 11025.0
    t = np.arange(8 * 2048) / fs
    x = 0.1 * np.exp(2j * np.pi * 1000 * t)
    r = O.Resampler(2048)
    outs = [r.process(x[i * 2048:(i + 1) * 2048], rate) for i in range(8)]
    counts = [len(o) for o in outs]
    assert set(counts) <= {361, 362} and sum(counts) == int(np.ceil(8 * 2048 / rate))
    y = np.concatenate(outs)
    tt = (np.arange(len(y)) * rate - 14.0) / fs
    assert np.abs(y[40:] - 0.1 * np.exp(2j * np.pi * 1000 * tt[40:])).max() < 3e-6
    assert 0.0 <= r.float_time < rate


def test_agc_off_is_a_gain_and_on_settles_at_the_knee_curve(oracle_mod):
    """AGC_OFF: out = 10^((threshold/5)/20) * in with the integer division the reference writes (agc.cpp:241-245);
    the constructor's OFF/1 is unity.  AGC on, constant-envelope input above the knee: once the averagers settle the
    gain is 0.7 * 10^(mag*(slope-1)) = 0.7/|x|max, i.e. the larger of |re|,|im| leaves at 0.7 (agc.cpp:226-231)."""
    O = oracle_mod
    fs = 62500.0
    x = 0.05 * np.exp(2j * np.pi * 500 * np.arange(40000) / fs)
    a = O.Agc(fs)
    assert np.array_equal(a.process(x[:100]), x[:100])
    a.set_mode(0, 33)  # 33 / 5 = 6 dB
    assert np.allclose(a.process(x[:100]), x[:100] * 10 ** (6 / 20), rtol=1e-15)
    b = O.Agc(fs)
    b.set_mode(2, 60)  # knee -60 dB: 0.05 is far above it
    y = b.process(x)
    tail = y[-2000:]
    assert abs(max(np.abs(tail.real).max(), np.abs(tail.imag).max()) - 0.7) < 2e-3
    d = int(fs * np.float32(0.015))  # the output is the input delayed by delay_samples (agc.cpp:104-110)
    ph = np.angle(tail * np.conj(x[-2000 - d:-d]))
    assert np.abs(ph).max() < 1e-9


def test_fd_estimate_window_arithmetic(oracle_mod):
    """fdEstimate on a synthetic dB spectrum: a flat -100 dB floor with a 7-bin -30 dB plateau centred on the mixer bin.
    bin width 2048000/4096 = 500 Hz; band -4..4 kHz -> bins mixer-8 .. mixer+8 (17 bins inclusive, divided by bpBins = 16
    as the reference does); peak -30, average 10*log10((7e-3 + 10e-10)/16), floor -100, snr 70."""
    sp = np.full(4096, -100.0)
    mixer_bin = 2048 + 200
    sp[mixer_bin - 3:mixer_bin + 4] = -30.0
    peak, avg, snr, floor = oracle_mod.fd_estimate(sp, 2048000, -4000, 4000, 100000.0)
    assert peak == -30.0 and floor == -100.0 and abs(snr - 70.0) < 1e-9
    assert abs(avg - 10 * np.log10((7 * 1e-3 + 10 * 1e-10) / 16)) < 1e-9


def test_anf_is_ill_conditioned_on_band_limited_input(oracle_mod):
    """NoiseFilter (45-tap leaky NLMS) behind the band-pass: its input occupies a few per cent of the band, the input
    correlation matrix is nearly singular, and the reference's OWN output moves by ~1e-4 for a 1e-8 white perturbation
    of that input (amplification ~1e4) -- while on a full-band input the same perturbation stays at the 1e-7 level.
    This is why the in-chain GPU comparison for the ANF carries a looser bar (tests/test_parity_gpu.py)."""
    O = oracle_mod
    fs = 64000.0
    rng = np.random.RandomState(2)
    t = np.arange(6144) / fs
    narrow = 0.15 * np.exp(2j * np.pi * 1000 * t) + 0.09 * np.exp(2j * np.pi * 2200 * t)  # what a 300..3000 Hz band-pass leaves
    wide = narrow + 0.03 * (rng.standard_normal(len(t)) + 1j * rng.standard_normal(len(t)))
    pert = 1e-8 * (rng.standard_normal(len(t)) + 1j * rng.standard_normal(len(t)))

    def moved(x):
        y0, y1 = O.Anf().process(x), O.Anf().process(x + pert)
        return np.sqrt(np.mean(np.abs(y1 - y0) ** 2)) / np.sqrt(np.mean(np.abs(y0) ** 2))
    assert moved(narrow) > 1e-5
    assert moved(wide) < 1e-6


def test_conditioner_restatements_closed_forms(oracle_mod):
    """IQBalance with unit gain / zero phase on a clean tone leaves it untouched to first order (t2 stays ~mu*|x|^2);
    NoiseBlanker 1 zeroes exactly 7 samples from a spike on and otherwise delays by 2; NoiseBlanker 2 replaces a spike by
    the running average; DCRemoval (high-pass 10 Hz) removes a constant."""
    O = oracle_mod
    fs = 2048000.0
    t = np.arange(4096) / fs
    x = 0.1 * np.exp(2j * np.pi * 50e3 * t)
    y = O.iq_balance(x, 1.0, 0.0)
    assert np.abs(y - x).max() < 1e-3 and np.abs(y[:3] - x[:3]).max() < 1e-4
    nb = O.NoiseBlanker(); nb.enable(1)
    z = x.copy(); z[2000] += 5.0
    o = nb.process(z, 1)
    zeros = np.flatnonzero(o == 0)
    assert list(zeros[zeros >= 2000]) == list(range(2000, 2007))
    assert np.allclose(o[2100:2200], z[2098:2198])
    nb2 = O.NoiseBlanker(); nb2.enable(2)
    o2 = nb2.process(z, 2)
    assert abs(o2[2000]) < 2.0 and np.array_equal(o2[2500:2600], z[2500:2600])
    dc = O.Iir("hp", 10, 0.7071, fs)
    d = dc.process(np.full(2000000, 0.25 + 0.1j))
    assert abs(d[-1]) < 1e-3 and abs(d[0] - (0.25 + 0.1j)) < 1e-4



def test_squelch_is_an_early_return_that_freezes_the_demodulator(oracle_mod):
    """receiver.cpp:959-965: with avgDb of the latest spectrum under m_squelchDb the frame ends after the band-pass: no audio,
    and the demodulator behind the gate keeps its state.  -120 (the default) never gates."""
    fs, n, bins, fc = 2048000, 2048, 4096, 100e3
    sf = 32 * 2048
    t = np.arange(3 * sf) / fs
    carrier = 0.1 * (1 + 0.5 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * fc * t)
    rng = np.random.default_rng(3)
    noise = 1e-5 * (rng.standard_normal(3 * sf) + 1j * rng.standard_normal(3 * sf))
    x = carrier * np.repeat([1.0, 0.0, 1.0], sf) + noise

    def run(squelch):
        r = oracle_mod.Receiver(fs, n, bins)
        r.set_mode(oracle_mod.AM); r.set_mixer(fc); r.set_filter(-5000, 5000); r.set_squelch(squelch)
        return [r.process(x[f * n:(f + 1) * n], want_spectrum=False)[0] for f in range(3 * sf // n)]

    gated, plain = run(-60.0), run(-120.0)
    per_sf = sf // n
    counts = [sum(len(a) for a in gated[k * per_sf:(k + 1) * per_sf]) for k in range(3)]
    assert counts == [2048, 0, 2048]
    assert [sum(len(a) for a in plain[k * per_sf:(k + 1) * per_sf]) for k in range(3)] == [2048, 2048, 2048]
    first = np.concatenate(gated[:per_sf])
    assert np.array_equal(first, np.concatenate(plain[:per_sf]))  # the gate changes nothing while it is open
    # after the gate reopens the demodulator carries on from the state the first super-frame left (the ungated run's has
    # meanwhile seen 2048 samples of silence, so the two differ), and the modulation is there
    again, ungated = np.concatenate(gated[2 * per_sf:]).real, np.concatenate(plain[2 * per_sf:]).real
    assert np.abs(again[1100:]).max() > 0.01
    assert not np.allclose(again, ungated, rtol=0, atol=1e-6)
    assert sum(len(a) for a in run(-10.0)) == 0  # a threshold above the carrier's average: every super-frame is gated


@pytest.mark.parametrize("fs", [256000.0, 312500.0, 390625.0])
@pytest.mark.parametrize("pilot", ["clean", "noisy", "weak", "absent"])
def test_wfm_stereo_pilot_pll_of_the_reference_does_not_hold_lock(oracle_mod, fs, pilot):
    """Why FM-Stereo is not demultiplexed on the device path.  Restated line by line (processDataStereo,
    demod_wfm.cpp:255-297; processPilotPll :392-429; arctan2 :792-821), the pilot PLL steers its NCO onto 19 kHz but its
    phase detector -- Demod_WFM::arctan2 with 2*pi where the textbook approximation has pi/2 -- is discontinuous next to
    the loop's operating point, so the loop ends in a limit cycle, the lock average climbs past LOCK_MAG_THRESHOLD within the
    first blocks for every pilot phase, and from then on the block copies the mono signal to both channels.  What the
    reference's dmFMS produces is therefore its mono discriminator output without the 75 kHz pre-filter; there is no stereo
    separation to be bit-compatible with.  Pinned at the three demodulator rates the WFM chains of the ladder end on (256, 312.5
    and 390.625 kHz) with a 10 % pilot, the same under 2 % noise, a 3 % pilot and none; anything else: parity unpinned."""
    from tests.signals import lcg_noise
    n, blocks = 2048, 24
    t = np.arange(n * blocks) / fs
    left, right = 0.9 * np.sin(2 * np.pi * 1000 * t), 0.9 * np.sin(2 * np.pi * 2500 * t)
    amp = {"clean": 0.1, "noisy": 0.1, "weak": 0.03, "absent": 0.0}[pilot]
    for ph in (0.0, 1.0, 2.5, 3.67, 5.0):
        mpx = 0.45 * (left + right) + amp * np.sin(2 * np.pi * 19000 * t + ph) + 0.45 * (left - right) * np.sin(2 * (2 * np.pi * 19000 * t + ph))
        x = 0.5 * np.exp(1j * 2 * np.pi * 75000 * np.cumsum(mpx) / fs)
        if pilot == "noisy":
            x = x + lcg_noise(len(x), 7, 0.02)
        d = oracle_mod.DemodWFM(fs)
        locks, outs = [], []
        for k in range(blocks):
            o, lk = d.process_stereo(x[k * n:(k + 1) * n])
            locks.append(lk)
            outs.append(o)
        assert not any(locks[3:]), "pilot phase %.2f" % ph
        if pilot == "clean":
            assert abs(d.s.nco_freq - (-19000.0 * 2 * np.pi / fs)) < 1e-5  # the frequency IS found (to 0.6 Hz) ...
        assert d.s.err_ave > 1.0                                            # ... the phase detector never settles
        tail = np.concatenate(outs[8:])
        assert np.array_equal(tail.real, tail.imag)                         # mono in both channels


def test_uncompensated_bin_power_of_a_full_scale_tone(oracle_mod):
    """pebblelib/fft.cpp:282-290: "a BlackmanHarris window has a gain factor of 0.36 ... the expected uncompensated power in our
    1 bin should be 2048 * 0.36 = 737.28".  A full-scale bin-centred tone through the oracle's window and transform: the bin
    holds N * coherentGain = 2048 * 0.35875 = 734.72 (the comment rounds the gain to 0.36), everything else ~0."""
    O = oracle_mod
    n = 2048
    s = O.Spectrum(2048, n)
    w = s.window()
    x = np.exp(2j * np.pi * 200 * (np.arange(n)) / n)
    X = O.fft(x * w)
    assert abs(np.abs(X[200]) - 2048 * s.coherent_gain) < 1e-6 * 2048
    assert abs(np.abs(X[200]) - 737.28) / 737.28 < 4e-3          # the comment's figure, with its rounded 0.36
    # the (i + 0.5)/N phase of the reference's window leaves e^{j pi k/N}-modulated leakage on the four-term main lobe only
    assert np.abs(np.delete(X, [197, 198, 199, 200, 201, 202, 203])).max() < 1e-3 * np.abs(X[200])


def test_window_coherent_gains_should_be_comments():
    """pebblelib/windowfunction.cpp:74-233 annotates eight windows with the coherent gain they "SB" (should be): 1, 0.50, 0.67,
    0.69, 0.50, 0.54, 0.42, 0.36.  Restating the loops as written shows which of those the code produces.  RECTANGULAR and
    BLACKMANHARRIS (the only one on the receive path, signalspectrum.cpp:58) sum the whole window and give their figure;
    the symmetric windows sum i = 0 .. N/2 only (`i <= midn`) and divide by N, i.e. HALF the annotated gain; WELCH's argument
    is an integer division that is zero over that range (window = 1 -> 0.50), PARZEN's triangle halves to 0.25, and
    BLACKMAN's formula reads coherentGain before it is set.  Only the two full-sum windows are known answers of the code."""
    n = 2048
    midn, midp1, midm1 = n // 2, (n + 1) // 2, (n - 1) // 2
    two_pi = np.float32(2 * np.pi)
    freq = np.float32(two_pi / np.float32(n))
    i = np.arange(midn + 1)
    angle = np.cumsum(np.concatenate([[np.float32(0)], np.full(midn, freq, dtype=np.float32)])).astype(np.float32)  # angle += freq
    rect = np.ones(n).sum() / n                                                        # :68-74
    hann = (0.5 - 0.5 * np.cos(angle.astype(np.float64))).sum() / n                    # :79-85
    welch = (1.0 - np.sqrt(np.trunc((i - midm1) / midp1).clip(0).astype(np.float32))).sum() / n   # :91-97, int / int
    parzen = (1.0 - np.abs((i - midm1).astype(np.float32) / midp1)).sum() / n          # :103-109
    rate = np.float32(1.0 / midn)
    bart = np.cumsum(np.concatenate([[np.float32(0)], np.full(midn, rate, dtype=np.float32)])).astype(np.float64).sum() / n  # :115-121
    hamm = (0.54 - 0.46 * np.cos(angle.astype(np.float64))).sum() / n                  # :129-135
    a = [np.float32(v) for v in (0.35875, 0.48829, 0.14128, 0.01168)]                  # :214-233
    k = (np.arange(n) + 0.5) / n
    bh = (a[0] - a[1] * np.cos(float(two_pi) * k) + a[2] * np.cos(2.0 * float(two_pi) * k) - a[3] * np.cos(3.0 * float(two_pi) * k)).sum() / n
    assert rect == 1.0                                    # SB 1
    assert round(bh, 2) == 0.36 and abs(bh - 0.35875) < 1e-6   # SB 0.36
    assert abs(hann - 0.50 / 2) < 1e-3                    # SB 0.50: the loop covers half the window
    assert abs(hamm - 0.54 / 2) < 1e-3                    # SB 0.54
    assert abs(bart - 0.50 / 2) < 1e-3                    # SB 0.50
    assert abs(welch - 0.50) < 1e-3                       # SB 0.67: the square root's argument is an integer quotient, 0 here
    assert abs(parzen - 0.25) < 1e-3                      # SB 0.69


@pytest.mark.parametrize("amp,n", [(1.0, 2048), (1.0, 4096), (0.5, 4096)])
def test_noise_floor_formula(oracle_mod, amp, n):
    """application/signalstrength.cpp:124-131: "Expected FFT powerDb = 10*log10(Noise power / Number FFT bins)", tabulated as
    1.0 / 2048 -> -33.11 dB, 1.0 / 4096 -> -36.12 dB, 0.25 / 4096 -> -42.13 dB.  With the window off (gain 1) and one bin per
    sample the oracle's normalisation (|X| / N, fft.cpp:347-355) gives E[power per bin] = P / N exactly; fftSpectrum
    reports the dB of the two-frame AVERAGE AMPLITUDE, whose square for Rayleigh bins is (1 + pi/4)/2 of the power (-0.49 dB)."""
    O = oracle_mod
    want = {(1.0, 2048): -33.11, (1.0, 4096): -36.12, (0.5, 4096): -42.13}[(amp, n)]
    assert abs(10 * np.log10(amp * amp / n) - want) < 0.02   # the table rounds (its last row is 0.014 dB off its own formula)
    rng = np.random.default_rng(7)
    s = O.Spectrum(n, n, window=False)
    acc = []
    for f in range(12):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (amp / np.sqrt(2.0)) * 0.2   # power (0.2 amp)^2, |x| < 0.9
        db = s.process(x)
        if f:
            acc.append(np.mean(10 ** (db / 10)))
    got = 10 * np.log10(np.mean(acc)) - 20 * np.log10(0.2)
    assert abs(got - (want + 10 * np.log10((1 + np.pi / 4) / 2))) < 0.1


def test_agc_remembers_the_silence_it_started_in(oracle_mod):
    """Why the device tests that run an AGC use a 5e-5 bar for the first half second and 1e-5 after it.  The AGC's detector is
    log10(max(|re|, |im|) + 1e-8) (agc.cpp:119-121): while the band-pass is still filling, its output is ~1e-16..1e-9 and the
    detector reads about -8; an ABSOLUTE error of 3e-8 there -- the fp32 floor of an overlap-save block whose later samples are
    at full level -- reads -7.4 instead.  That start-up value seeds the decay average (time constants 30 / 100 ms), and its
    trace is what sets the gain once the envelope falls: the oracle's own output, 100-250 ms later, moves by > 3e-6 when
    nothing but the first 64 near-silent samples of its input are touched at the 3e-8 level.  Not chaos (cf. SAM): the trace
    decays, by a factor e every 100 ms."""
    O = oracle_mod
    fs, fc = 2048000, 100e3
    N = 16 * 32 * 2048
    t = np.arange(N) / fs
    x = 0.1 * (1 + 0.8 * np.sin(2 * np.pi * 3.0 * t)) * np.exp(2j * np.pi * (fc + 1000) * t) + lcg_noise(N, 9, 1e-4)
    mix = O.Mixer(fs); mix.set_frequency(fc)
    dec = O.Decimator(fs, 30000)
    z = np.concatenate([dec.process(mix.process(x[i:i + 8192])) for i in range(0, N, 8192)]) * 10 ** (2 * 5 / 20.0)
    ff = O.FastFIR(); ff.setup(300, 3000, 0, 64000)
    y = np.concatenate([ff.process(z[k:k + 2048]) for k in range(0, len(z), 2048)])
    assert np.abs(y[:8]).max() < 1e-9 and np.abs(y[600:700]).min() > 1e-2   # the filter fills within a few hundred samples

    def agc(v):
        a = O.Agc(64000); a.set_mode(1, 20)
        return np.concatenate([a.process(v[k:k + 2048]) for k in range(0, len(v), 2048)])

    base = agc(y)
    y2 = y.copy()
    y2[:64] += 3e-8 * np.exp(2j * np.pi * np.arange(64) / 7.0)
    pert = agc(y2)
    rr = lambda k: float(np.sqrt(np.mean(np.abs(pert[k * 2048:(k + 1) * 2048] - base[k * 2048:(k + 1) * 2048]) ** 2)) /
                         np.sqrt(np.mean(np.abs(base[k * 2048:(k + 1) * 2048]) ** 2)))
    assert rr(2) < 1e-7          # while the attack average rules the gain, nothing shows
    assert rr(5) > 3e-6          # 160-190 ms in: the decay average, seeded at start-up, now does
    assert rr(15) < rr(5) / 10   # and its trace fades (half a second in: below 1e-6)


def _dc_table():
    """(name, ntaps, limit, taps) rows of oracle/dc_taps.h -- the data table the oracle and the library both carry"""
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "dc_taps.h")).read()
    rows = []
    for m in re.finditer(r'\{"(\w+)",\s*(\d+),\s*([0-9.]+),\s*([0-9.]+),\s*\{([^}]*)\}\}', txt):
        vals = [float(v) for v in m.group(5).replace("\n", " ").split(",") if v.strip()]
        rows.append((m.group(1), int(m.group(2)), float(m.group(3)) - float(m.group(4)), vals[:int(m.group(2))]))
    assert len(rows) == 12
    return rows


def test_downconvert_stage_limits_are_the_reference_comments(oracle_mod):
    """CDownConvert (pebblelib/downconvert.cpp): the reference works the stage limits out in a comment above SetDataRate
    (:124-134, "Examples at 48k 10k"): CIC3 to 32,000,000, the 11-tap halfband to 1,920,000, HB15 979,592, HB19 666,666, HB23 527,472
    and, for HB51, 287,425 at 48 kHz and 59,880 at 10 kHz of wanted bandwidth.  The generated table (filtercoef.h:19-30 through
    tools/gen_dc_taps.py) reproduces every one of those figures, and the ladder picks a stage exactly at its limit."""
    rows = {r[0]: r for r in _dc_table()}
    for name, bw, want in (("cic3", 48000, 32000000), ("hb11", 48000, 1920000), ("hb15", 48000, 979592), ("hb19", 48000, 666666),
                           ("hb23", 48000, 527472), ("hb51", 48000, 287425), ("hb51", 10000, 59880)):
        assert abs(bw / rows[name][2] - want) < 1.0, (name, bw / rows[name][2])  # (the comment rounds some and truncates others)
    # the ladder: the FIRST design whose limit the rate clears; stops once the rate is at or under max_bw / HB51's limit or 15.8 kHz
    d = oracle_mod.DownConvert()
    assert d.set_data_rate(32000000.0, 48000) == 250000.0 and d.chain()[0] == 0 and len(d.chain()) == 7  # at CIC3's limit: CIC3; down to <= 287,425
    d = oracle_mod.DownConvert()
    assert d.set_data_rate(31999999.0, 48000) and d.chain()[0] == 11                            # just under: the 11-tap halfband
    d = oracle_mod.DownConvert()
    assert d.set_data_rate(2048000, 15000) == 64000.0 and d.chain() == [11, 11, 15, 19, 31]      # receiver.cpp:198 at the stock rate
    d = oracle_mod.DownConvert()
    assert d.set_data_rate(20e6, 200000, simple=True) == 312500.0 and d.chain() == [51] * 6      # receiver.cpp:217: HB51 down to <= 400 kHz
    d = oracle_mod.DownConvert()
    assert d.set_data_rate(40000, 15000) == 40000 and d.chain() == []                            # already under 15000 / 0.167: no stage


def test_downconvert_against_independent_filters(oracle_mod):
    """(parity with the reference binary: tests/test_reference_pins.py, downconvert_*)  The restatement against an independent model -- the
    oscillator in closed form (a_0 = 1, a_{n+1} = a_n (1.95 - a_n^2), phase (n + 1) inc: the recurrence of downconvert.cpp:288-293
    started from m_Osc1 = 1), every stage as a plain convolution at stride 2: the CIC3 as (1 3 3 1) / 8 ending on the pair's ODD sample
    (:524-526), the fixed 11-tap class with its table as it stands (:429-489), the generic class with tap 0 counted twice
    (:368-376: the accumulator starts from tap 0 and the loop adds it again).  Streaming: any split of the input into calls gives
    the same output (each stage keeps its last ntaps - 1 inputs)."""
    O = oracle_mod
    rows = _dc_table()
    by_taps = {r[1]: r for r in rows}
    fs, f0 = 10e6, 1.234e6
    d = O.DownConvert()
    rate = d.set_data_rate(fs, 15000)
    chain = d.chain()
    assert chain == [0, 11, 11, 11, 11, 15, 27] and rate == fs / 128
    d.set_frequency(f0)
    n = 128 * 600
    x = tones(fs, n, [(0.3, f0 + 2500.0), (0.2, f0 - 4000.0), (0.3, f0 + 900e3)]) + lcg_noise(n, 4, 1e-3)
    got = np.concatenate([d.process(x[:128 * 100]), d.process(x[128 * 100:128 * 140]), d.process(x[128 * 140:])])  # (every stage sees >= its tap count per call: below that the reference returns early, :361-362)
    one = O.DownConvert(); one.set_data_rate(fs, 15000); one.set_frequency(f0)
    assert np.array_equal(got, one.process(x))
    # the independent model
    a = np.empty(n)
    v = 1.0
    for i in range(n):
        a[i] = v
        v = v * (1.95 - v * v)
    inc = 2 * np.pi * (-f0) / fs
    y = x * a * np.exp(1j * inc * (np.arange(n) + 1))
    for taps in chain:
        if taps == 0:
            h = np.array([1, 3, 3, 1]) / 8.0
            full = np.convolve(np.concatenate([np.zeros(3), y]), h)[3:]   # full[m] = sum_t h[t] y[m - t]
            y = full[1::2][:len(y) // 2]                                  # ends on the odd sample 2 j + 1
        else:
            h = np.array(by_taps[taps][3])
            if taps != 11:
                h = h.copy(); h[0] *= 2.0
            full = np.convolve(y, h[::-1])      # out[k] = sum_j h[j] y[2 k + j - (T - 1)]  ==  conv(y, reversed h)[2 k]
            y = full[0:len(y):2]
    assert got.shape == y.shape
    assert np.sqrt(np.mean(np.abs(got - y) ** 2)) <= 1e-10 * np.sqrt(np.mean(np.abs(y) ** 2))  # (measured 2e-12: the recurrence against the closed form)
    assert np.abs(got[300:]).max() > 0.2


def test_downconvert_set_data_rate_flips_the_tuned_frequency(oracle_mod):
    """As written (downconvert.cpp:205, :232): SetDataRate ends with SetFrequency(m_NcoFreq) -- the STORED frequency, which
    SetFrequency negated when it stored it (:103-106), is negated again: a rate change after tuning mirrors the tuning.  The
    reference's own call order (rates at construction, frequency later: receiver.cpp:198, :718) never shows it; restated, not fixed."""
    O = oracle_mod
    fs, f0, n = 2048000.0, 100e3, 64 * 400
    x = tones(fs, n, [(0.5, f0 + 1000.0)])
    a = O.DownConvert(); a.set_data_rate(fs, 15000); a.set_frequency(f0)
    ya = a.process(x)
    b = O.DownConvert(); b.set_frequency(f0); b.set_data_rate(fs, 15000)     # the other order: tuned to -f0 afterwards
    yb = b.process(x)
    assert np.abs(ya[200:]).min() > 0.4 and np.abs(yb[200:]).max() < 1e-3


# the reference's own RDS tables (application/demod/rbdsconstants.h): the generator matrix rows, the offset words and their syndromes
_RDS_CHKWORDGEN = [0x077, 0x2E7, 0x3AF, 0x30B, 0x359, 0x370, 0x1B8, 0x0DC, 0x06E, 0x037, 0x2C7, 0x3BF, 0x303, 0x35D, 0x372, 0x1B9]
_RDS_PARCKH = [0x2DC, 0x16E, 0x0B7, 0x287, 0x39F, 0x313, 0x355, 0x376, 0x1BB, 0x201, 0x3DC, 0x1EE, 0x0F7, 0x2A7, 0x38F, 0x31B]
_RDS_OFFSET_SYNDROME = {"A": 0x3D8, "B": 0x3D4, "C": 0x25C, "Cp": 0x3CC, "D": 0x258}


def test_rds_block_coding_of_the_test_signal_against_the_reference_tables():
    """tests/rds_signal.py builds its blocks from the published generator polynomial; the reference holds the same code as tables
    (rbdsconstants.h): CHKWORDGEN row i is the checkword of information bit i, and the syndrome checkBlock forms (the top ten
    bits through an identity, the low sixteen through PARCKH, demod_wfm.cpp:711-721) of a block with offset word X is
    OFFSET_SYNDROME_BLOCK_X.  Both hold for the encoder the RDS tests transmit with."""
    from tests import rds_signal as rs
    assert [rs.checkword(1 << (15 - i), 0) for i in range(16)] == _RDS_CHKWORDGEN
    rng = np.random.default_rng(5)
    for key, want in _RDS_OFFSET_SYNDROME.items():
        for info in rng.integers(0, 65536, 50):
            blk = (int(info) << 10) | rs.checkword(int(info), rs.OFFSET[key])
            syn = blk >> 16
            for i in range(16):
                if blk & (0x8000 >> i):
                    syn ^= _RDS_PARCKH[i]
            assert syn == want


@pytest.mark.parametrize("fsw", [250000, 256000, 312500])
def test_rds_groups_of_a_multiplex_through_the_restated_decoder(oracle_mod, fsw):
    """The RDS branch of processDataStereo (demod_wfm.cpp:296-357, 488-786) restated in the oracle, on an FM multiplex carrying 30 known
    groups (0A / 2A / 2B).  As written the branch tunes the WRONG way -- CDownConvert::SetFrequency negates its argument
    (downconvert.cpp:103-108), so SetFrequency(-57000) moves the multiplex up and the decoder sees the subcarrier's image through the
    Hilbert pair's stop band -- and its PLL's phase detector (arctan2 with 2 pi where pi / 2 belongs, :792-821) pins the loop at its
    frequency limit with a constant lead; a subcarrier 14 Hz low stands nearly still in that loop and most groups come through, one
    on frequency turns at ~19 Hz through the detector and few do.  Pinned here: the groups the decoder queues are groups that were sent,
    in the order sent (the all-zero group marks a cleared queue; a miscorrected block now and then); getNextRdsGroupData pops them one per call and flags repeats.
    The branch itself is pinned to Demod_WFM::processDataStereo since: tests/test_reference_pins.py, cases demod_wfm_rds_*."""
    O = oracle_mod
    from tests import rds_signal as rs
    ng = 30
    groups = rs.make_groups(ng)
    n = int(fsw * (ng * 104 + 60) / 1187.5)
    n -= n % 2048
    for off, at_least in ((-14.0, 20), (0.0, 0)):
        x = rs.fm_multiplex(groups, float(fsw), n, subcarrier_offset_hz=off)
        d = O.DemodWFM(float(fsw))
        assert d.rds_rate in (fsw / 8.0, fsw / 16.0)
        pushed, popped = [], []
        for k in range(n // 2048):
            d.process_stereo(x[k * 2048:(k + 1) * 2048])
            pushed += [tuple(int(v) for v in r) for r in d.rds_pushed()]
            g = d.next_rds_group()                      # Demod::fmStereo: one per frame
            if g is not None:
                popped.append(g)
        sent = [tuple(g) for g in groups]
        real = [g for g in pushed if g != (0, 0, 0, 0)]
        idx = [sent.index(g) for g in real if g in sent]
        assert len(idx) >= at_least
        assert idx == sorted(idx) and len(set(idx)) == len(idx)  # queued once, in the order sent
        assert len(real) - len(idx) <= 3                # (the burst corrector "repairs" the odd damaged block into another valid one)
        assert [g for g, _ in popped] == pushed[:len(popped)] or (0, 0, 0, 0) in pushed
        assert all(ch for _, ch in popped[:1])
        bits = d.rds_bits()
        assert abs(len(bits) - n / fsw * 1187.5) < 30   # the resonator delivers the bit clock (a peak more or less where the signal nulls)


def test_downconvert_below_twice_a_stages_history_the_oracle_is_not_the_reference(oracle_mod):
    """CDownConvert::ProcessData runs its decimate-by-2 stages in place (downconvert.cpp:325), and CHalfBandDecimateBy2::DecBy2 copies its
    next history out of pInData after its outputs have overwritten the front of it (:389-390): with T <= InLength < 2 (T - 1) that
    history holds outputs.  The oracle (po_ DecBy2: the exact last T - 1 inputs) and the device stream exact history there, as
    pebblegpu.h promises for the stand-alone steps; a receiver refuses such frames for dmFMS (RdsCore::check_frame).  On the reference's
    recorded outputs (tests/golden/refpin_inplace_*.npy: six equal calls of 512 at 384 000 and of 256 at 256 000, whole) the first call
    is the oracle's -- its history is the zeros both start with -- and from the second call on the oracle differs by more than 1e-6
    (measured on this input: 7.1e-4 .. 1.7e-3 at 384 000, 1.9e-6 .. 9.2e-6 at 256 000).  The day someone makes the oracle restate the in-place copy,
    this test says so; tests/reference_cases.DC_BOUNDARY pins the shortest calls at which both are bit for bit."""
    from tests import reference_cases as R
    cases = R.inplace_cases()
    assert [c.name for c in cases] == ["inplace_downconvert_384000_8000_x512", "inplace_downconvert_256000_8000_x256"]
    for case in cases:
        assert os.path.getsize(case.fixture) < 16384
        want = R.expand(np.load(case.fixture))
        x = case.make_input()
        got = [np.asarray(v, dtype=np.float64) for _, v in case.oracle(oracle_mod, x)]
        assert len(got) == len(want) == 1 + R.DC_EQUAL_CALLS
        assert all(len(g) == n == len(t) for g, (n, t) in zip(got, want))            # the fixture holds every record whole
        assert np.array_equal(got[0], want[0][1])                                    # the output rate
        assert np.array_equal(got[1], want[1][1]), case.name                         # the first call
        later = [R.record_error("v", g, t) for g, (_, t) in zip(got[2:], want[2:])]
        print("%s: oracle against the reference's in-place history, calls 2..6: %s" % (case.name, " ".join("%.2e" % e for e in later)))
        assert min(later) > 1e-6, (case.name, later)
        if os.path.exists(R.BINARY):   # (and the fixture is what the binary gives today)
            ref = case.reference(x)
            assert all(np.array_equal(r, t) for r, (_, t) in zip(ref, want))
