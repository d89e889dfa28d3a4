"""The input conditioners and the AGC modes on the device, at the shapes the suite had not run them: several independent
streams with different flags, DCRemoval at 20 Msps, a blanker switched off and on again mid-stream, AGC SLOW / LONG and a
mode change between calls.  The oracle's side of each stage is held to the reference's own code by
tests/test_reference_pins.py (nb1/nb2 and their *_off_on cases, iqbalance, dcremoval_2048000 / dcremoval_20000000, agc_*),
so the bars here are the suite's own: TOL (1e-5 relative RMS), TOL_DB (0.1 dB) and, for an AGC that starts with its stream,
TOL_AGC_STARTUP (5e-5).

Every test prints its figures before it asserts.
"""
import numpy as np
import pytest

from tests.signals import lcg_noise, tones
from tests.test_parity_gpu import TOL, TOL_AGC_STARTUP, TOL_DB, db_err, rel_rms

pytestmark = pytest.mark.gpu


def _spiky(fs, n, f_tone, seed):
    x = tones(fs, n, [(0.05, f_tone), (0.02, -0.122 * fs)]) + lcg_noise(n, seed, 1e-3) + 0.01
    x[5000] += 2.0
    x[n // 3:n // 3 + 3] += 1.5j
    x[n - 4000] -= 3.0
    return x


def _oracle_frames(ref, x, n):
    outs = [ref.process(x[f * n:(f + 1) * n]) for f in range(len(x) // n)]
    return np.concatenate([o[0] for o in outs]), np.array([o[1] for o in outs])


def test_three_independent_streams_with_their_own_conditioners(gpu_lib, oracle_mod):
    """Three independent streams, conditioner flags 1 (DCRemoval), 6 (IQBalance + NB1) and 15 (all four), each with its own IQ gain and
    phase, USB, 3 super-frames in 2 calls: every stream against its own oracle chain.  The kernels index the factors, the blanker state
    and a list of the streams whose DC filter runs by stream; one stream alone cannot show a wrong index."""
    import pebblesdr_amd as P
    fs, n, S, bins = 2048000, 2048, 3, 2048
    flags, gains, phases = [1, 6, 15], [1.02, 0.97, 1.05], [0.03, -0.02, 0.01]
    f0 = [100e3, -200e3, 333e3]
    rx = P.ReceiverBank(fs, S, False, False, bins, max_superframes=2)
    refs = [oracle_mod.Receiver(fs, n, bins) for _ in range(S)]
    for s in range(S):
        refs[s].set_mode(oracle_mod.USB); refs[s].set_mixer(f0[s]); refs[s].set_filter(300, 3000)
        refs[s].set_conditioners(flags[s], gains[s], phases[s])
        rx.set_mode(s, P.DM_USB); rx.set_mixer(s, f0[s]); rx.set_bandpass(s, 300, 3000); rx.set_conditioners(s, flags[s], gains[s], phases[s])
    sf = rx.superframe
    xs = np.stack([_spiky(fs, 3 * sf, f0[s] + 1000.0, 20 + s) for s in range(S)])
    outs = [rx.process(xs[:, lo:hi]) for lo, hi in ((0, sf), (sf, 3 * sf))]
    g = np.concatenate([o[0] for o in outs], axis=1)
    gs = np.concatenate([o[1] for o in outs], axis=1)
    errs = []
    for s in range(S):
        r, rs = _oracle_frames(refs[s], xs[s], n)
        errs.append((rel_rms(g[s], r), max(db_err(gs[s][f], rs[f]) for f in range(1, len(rs)))))
    print("streams with flags %s: (audio rel RMS, spectrum dB) %s" % (flags, errs))
    for s in range(S):
        assert errs[s][0] <= TOL, (s, errs)
        assert errs[s][1] <= TOL_DB, (s, errs)


@pytest.mark.parametrize("flags", [1, 15])
def test_dc_removal_at_20_msps_on_the_wfm_receiver(gpu_lib, oracle_mod, flags):
    """DCRemoval where its 10 Hz high-pass pole lies at 1 - 2e-6 (20 Msps), alone and with the other three conditioners, in front of the
    WFM chain and the 8192-bin spectrum: 3 super-frames in 2 calls, a 0.01 DC offset and three spikes on an FM carrier.  The scan kernel
    stages its samples as floats; until now it had run at 2.048 Msps only."""
    import pebblesdr_amd as P
    fs, n, bins = 20000000, 2048, 8192
    rx = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=2)
    rx.set_mixer(0, 1.0e6); rx.set_conditioners(0, flags, 1.02, 0.03)
    ref = oracle_mod.Receiver(fs, n, bins); ref.set_mode(oracle_mod.FMM); ref.set_mixer(1.0e6); ref.set_conditioners(flags, 1.02, 0.03)
    sf = rx.superframe
    t = np.arange(3 * sf) / fs
    x = 0.5 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(3 * sf, 2, 1e-3) + 0.01
    x[5000] += 0.4; x[sf + 70000:sf + 70003] += 0.3j; x[2 * sf + 150] -= 0.4
    outs = [rx.process(x[lo:hi]) for lo, hi in ((0, sf), (sf, 3 * sf))]
    g = np.concatenate([o[0] for o in outs], axis=1)[0]
    gs = np.concatenate([o[1] for o in outs], axis=1)[0]
    r, rs = _oracle_frames(ref, x, n)
    e, ed = rel_rms(g, r), max(db_err(gs[f], rs[f]) for f in range(1, len(rs)))
    print("flags %d at 20 Msps: audio rel RMS %.3e, spectrum %.4f dB" % (flags, e, ed))
    assert g.shape == r.shape
    assert e <= TOL
    assert ed <= TOL_DB


def test_blankers_switched_off_and_on_again(gpu_lib, oracle_mod):
    """NB1 and NB2 on for one call, off for the next, on again for the third: switching a blanker on resets its averages (and NB1's
    spike count) in the reference's setters; the device does so in its conditioner setter.  Each call against the oracle chain given
    the same setter calls; the spikes fall into the first and the third call."""
    import pebblesdr_amd as P
    fs, n, bins = 2048000, 2048, 2048
    rx = P.ReceiverBank(fs, 1, True, False, bins, max_superframes=1)
    ref = oracle_mod.Receiver(fs, n, bins)
    ref.set_mode(oracle_mod.USB); ref.set_mixer(100e3); ref.set_filter(300, 3000)
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, 100e3); rx.set_bandpass(0, 300, 3000)
    sf = rx.superframe
    x = np.concatenate([_spiky(fs, sf, 101e3, 31 + k) * (1.0, 0.5, 2.0)[k] for k in range(3)])  # other levels: stale averages would show
    errs = []
    for k, fl in enumerate((12, 0, 12)):
        ref.set_conditioners(fl, 1.0, 0.0); rx.set_conditioners(0, fl, 1.0, 0.0)
        a, s = rx.process(x[k * sf:(k + 1) * sf])
        r, rs = _oracle_frames(ref, x[k * sf:(k + 1) * sf], n)
        errs.append((rel_rms(a[0], r), max(db_err(s[0][f], rs[f]) for f in range(1 if k == 0 else 0, len(rs)))))
    print("blankers on / off / on: (audio rel RMS, spectrum dB) per call %s" % errs)
    for e, ed in errs:
        assert e <= TOL
        assert ed <= TOL_DB


AGC_CALLS = (4, 8, 8)  # super-frames per call: 20 x 32 ms = 655 ms at 2.048 Msps
AGC_FCS = [-400e3, 300e3]


def _agc_input(fs, sf):
    """Two tones, one per channel, whose common level is held at 0.45 for 350 ms (the decay average charges: its rise takes 0.3 of the
    mode's decay time, 75 / 150 / 600 ms for MED / SLOW / LONG), drops by 10 dB to 0.14 -- above both knees (0.1 for threshold 20, 0.0316
    for 30), so the decay average alone sets the gain there -- and at 550 ms to 0.06, between the knees.  On the CPU the oracle's outputs
    for this input under MED / 30, SLOW / 30, LONG / 30 and MED / 30 then SLOW / 20 differ from one another by 0.057 (MED against MED then SLOW / 20) .. 0.44
    relative RMS (measured, channel 0), against the bar of 1e-5."""
    m = sum(AGC_CALLS) * sf
    t = np.arange(m) / fs
    env = np.where(t < 0.35, 0.45, np.where(t < 0.55, 0.14, 0.06))
    return env * (np.exp(2j * np.pi * (AGC_FCS[0] + 1000.0) * t) + np.exp(2j * np.pi * (AGC_FCS[1] + 1700.0) * t)) + lcg_noise(m, 3, 1e-4)


def _agc_oracle(oracle_mod, fs, n, sf, x, c, plan):
    """channel c of the oracle chain, frame by frame; plan: (mode, threshold) per call, None for manual gain throughout"""
    ref = oracle_mod.Receiver(fs, n, 0)
    ref.set_mode(oracle_mod.USB); ref.set_mixer(AGC_FCS[c]); ref.set_filter(300, 3000); ref.set_audio_rate(11025)
    if plan is None:
        ref.set_agc(0, 30)
    out, lo, prev = [], 0, None
    for k, nsf in enumerate(AGC_CALLS):
        if plan is not None and plan[k] != prev:
            ref.set_agc(*plan[k])
            prev = plan[k]
        out += [ref.process(x[f * n:(f + 1) * n])[0] for f in range(lo // n, (lo + nsf * sf) // n)]
        lo += nsf * sf
    return np.concatenate(out)


AGC_PLANS = {"slow": [(3, 30)] * 3, "long": [(4, 30)] * 3, "med_then_slow": [(2, 30), (3, 20), (3, 20)]}


@pytest.mark.parametrize("name", list(AGC_PLANS))
def test_audio_tail_usb_agc_slow_long_and_a_mode_change(gpu_lib, oracle_mod, name):
    """test_audio_tail_usb_agc_and_resampler with AGC SLOW, AGC LONG and a change from MED / 30 to SLOW / 20 before the second call, on an
    input long enough for the modes to differ (see _agc_input): two USB channels (the other on manual gain), the resampler to 11025 Hz,
    calls of 4, 8 and 8 super-frames.  Output count exact.  The oracle's output under MED / 30 throughout is computed too: the plan under
    test must lie a thousand bars or more from it, or the test could not tell the modes apart.

    Bars: TOL for the channel on manual gain; TOL_AGC_STARTUP (the suite's bar for an AGC that starts with its stream, see
    test_parity_gpu) for the AGC channel.  Here, unlike in the MED test, the decay average sets the gain, and the decay average remembers
    the band-pass output's first 14 samples, which lie under 1e-6 (the filter's onset): the device's fp32 overlap-save leaves a floor of
    3e-8 there where the oracle has 1e-15, and the log detector turns that into another start-up value.  The oracle's own sensitivity,
    measured on the CPU by adding a uniform floor of +-3e-8 to its AGC's input: SLOW 1.4e-5, MED then SLOW 8.6e-6, LONG 6.2e-8, MED
    1.2e-6 (with +-1e-8: 6.4e-6, 3.9e-6, 2.1e-8, 5.4e-7); rounding that input to fp32 instead, a relative error, moves it by 3e-8.
    The device measures 3.0e-5, 1.8e-5 and 1.2e-7 for the three plans: the same order and ranking."""
    import pebblesdr_amd as P
    plan = AGC_PLANS[name]
    fs, n, C = 2048000, 2048, 2
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=max(AGC_CALLS), audio_rate=11025)
    for c in range(C):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, AGC_FCS[c]); rx.set_bandpass(c, 300, 3000)
    rx.set_agc(1, 0, 30)
    sf = rx.superframe
    x = _agc_input(fs, sf)
    r = [_agc_oracle(oracle_mod, fs, n, sf, x, 0, plan), _agc_oracle(oracle_mod, fs, n, sf, x, 1, None)]
    med = _agc_oracle(oracle_mod, fs, n, sf, x, 0, [(2, 30)] * 3)
    apart = rel_rms(r[0], med)
    g, lo, prev = [], 0, None
    for k, nsf in enumerate(AGC_CALLS):
        if plan[k] != prev:
            rx.set_agc(0, *plan[k])
            prev = plan[k]
        g.append(rx.process(x[lo:lo + nsf * sf])[0])
        lo += nsf * sf
    g = np.concatenate(g, axis=1)
    errs = [rel_rms(g[c], r[c]) if g.shape[1] == len(r[c]) else None for c in range(C)]
    print("AGC plan %s: counts %d / %d, rel RMS %s; the oracle under MED / 30 lies %.3f away" % (name, g.shape[1], len(r[0]), errs, apart))
    assert apart > 1000 * TOL
    for c, bar in enumerate((TOL_AGC_STARTUP, TOL)):
        assert g.shape[1] == len(r[c])
        assert errs[c] <= bar
