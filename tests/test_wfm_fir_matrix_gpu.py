"""k_wfm_fir with its audio FIR on the fp32 matrix instruction (csrc/wfm_fir_geom.h), on the device: P.Demod in DM_FMM against
oracle.DemodWFM(rate) as tests/test_demod_geometry_gpu.py runs its rows, at four demodulator rates that table does not have or that
take another turn through the K loop, and a three-channel WFM bank at the 312 500 Hz the headline benchmark runs.

| rate    | Llp | L4   | groups of 16 k per K half | why                                                        |
| 312 500 | 47  | 656  | 21 + 21                   | the benchmark's rate                                       |
| 250 000 | 50  | 528  | 17 + 17 (odd turns)       | L4 an odd multiple of 16; a half ends on a lone group      |
| 512 000 | 62  | 1024 | 33 + 32                   | the longest response, Lx > 1024, unequal halves            |
| 100 000 | 1   | 272  | 9 + 9                     | low-pass off                                               |

Calls, in one handle so that the histories carry: 80, Lx - 1, Lx, Lx + 1, 1023, 1024, 1025, 2 * 1024 + 2 (n < Lx with the history
merged on the host side of the call, ragged last workgroups of 1 and 2 outputs, whole workgroups, several workgroups).  Bar and
error measure: tests/demod_cases.py (rel-RMS <= 1e-5 per chunk of 1024 consecutive outputs of every call, the first included).
The low-pass in front of the discriminator runs on the same instruction (Llp 47, 50, 62: four or five groups of 16 k; Llp 1: one).
Measured worst chunk on the MI355X: 1.04e-7 (100 000), 8.5e-8 (250 000), 7.7e-8 (312 500), 7.2e-8 (512 000), 6.9e-8 (the bank)."""
import numpy as np
import pytest

from tests import demod_cases as DC
from tests.signals import lcg_noise

pytestmark = pytest.mark.gpu

# rate -> (Llp, L4): what WfmCore::init designs there, asserted against the design program
RATES = {312500: (47, 656), 250000: (50, 528), 512000: (62, 1024), 100000: (1, 272)}
QUIET_CALLS = (1, 2)   # Lx - 1 after 80, and the call behind it: demod_cases.WFM_QUIET_CALLS' reason (a short call's merged history)


def _script(Lx):
    return [80, Lx - 1, Lx, Lx + 1, 1023, 1024, 1025, 2 * 1024 + 2]


def _input(rate, script, seed):
    """demod_cases.wfm_input's construction at this rate and script"""
    n = sum(script)
    t = np.arange(n) / float(rate)
    level = np.ones(n)
    for k, (o, m) in enumerate(DC.call_offsets(script)):
        if k in QUIET_CALLS:
            level[o:o + m] = DC.WFM_QUIET_LEVEL
    dev = min(75000.0, rate / 4.0)
    f = level * dev * (np.cos(2 * np.pi * 1000.0 * t + 0.9) + 0.3 * np.cos(2 * np.pi * 3300.0 * t + 0.2))
    return 0.5 * np.exp(2j * np.pi * np.cumsum(f) / float(rate)) + lcg_noise(n, seed, 1e-4)


@pytest.mark.parametrize("rate", sorted(RATES))
def test_wfm_mono_through_the_matrix_fir(gpu_lib, oracle_mod, rate):
    import pebblesdr_amd as P
    d = DC.wfm_design(rate)
    assert d.fused and (d.Llp, d.L4) == RATES[rate], (d.fused, d.Llp, d.L4)
    Lx = d.L4 + d.Llp
    script = _script(Lx)
    x = _input(rate, script, 60 + sorted(RATES).index(rate))
    ref = oracle_mod.DemodWFM(rate)
    dm = P.Demod(64000, rate, max(script))
    dm.setDemodMode(P.DM_FMM)
    errs, at = [], 0
    for k, n in enumerate(script):
        fr = x[at:at + n]
        g, r = dm.processBlock(fr), ref.process(fr)
        assert g.shape == r.shape == (n,)
        assert np.array_equal(g.real, g.imag), "mono: left = right"
        errs += [(k, c, e) for c, e in enumerate(DC.chunk_errors(g, r, DC.K_WFM_OUTB))]
        at += n
    dm.close()
    e, c, k = DC.worst_of(errs)
    print("wfm-%d (Llp %d, L4 %d, Lx %d): worst rel-RMS over %d chunks %.3e, call %d (%d samples) chunk %d" % (rate, d.Llp, d.L4, Lx, len(errs), e, c, script[c], k))
    assert e <= DC.TOL


def test_wfm_bank_of_three_channels_with_different_content(gpu_lib, oracle_mod):
    """Three independent 2.5 Msps streams (demodulator rate 312 500: Llp 47, L4 656), each its own FM signal, in one WFM bank: grid.y = 3,
    every channel's own history rows, the tail-refresh workgroups riding on the launch.  Each channel against the oracle's Receiver
    over three calls of one super-frame, per chunk of 1024 outputs."""
    import pebblesdr_amd as P
    fs, nf, K = 2_500_000, 2048, 3
    rx = P.ReceiverBank(fs, 3, False, True, 0, max_superframes=1)
    assert int(rx.info.demod_rate_int) == 312500
    sf = rx.superframe
    n = K * sf
    t = np.arange(n) / float(fs)
    tones = ((1000.0, 3300.0), (700.0, 5200.0), (2400.0, 9100.0))
    xs, refs = [], []
    for c, (f1, f2) in enumerate(tones):
        rx.set_mode(c, P.DM_FMM); rx.set_mixer(c, 250e3)
        f = 60000.0 * (np.cos(2 * np.pi * f1 * t + 0.9 + c) + 0.3 * np.cos(2 * np.pi * f2 * t + 0.2))
        xs.append(0.5 * np.exp(1j * (2 * np.pi * np.cumsum(f) / fs + 2 * np.pi * 250e3 * t)) + lcg_noise(n, 80 + c, 1e-4))
        r = oracle_mod.Receiver(fs, nf, 0)
        r.set_mode(oracle_mod.FMM); r.set_mixer(250e3)
        refs.append(r)
    x = np.array(xs)
    errs = []
    for k in range(K):
        g = rx.process(x[:, k * sf:(k + 1) * sf])[0]
        for c in range(3):
            want = np.concatenate([a for a in (refs[c].process(x[c, i:i + nf], want_spectrum=False)[0] for i in range(k * sf, (k + 1) * sf, nf)) if len(a)])
            assert g[c].shape == want.shape
            errs += [((c, k), j, e) for j, e in enumerate(DC.chunk_errors(g[c], want, DC.K_WFM_OUTB))]
    rx.close()
    assert DC.rel_rms(g[0], g[1]) > 1e-2 and DC.rel_rms(g[1], g[2]) > 1e-2, "the channels carry different content"
    e, (c, k), j = DC.worst_of(errs)
    print("WFM bank, three channels: worst rel-RMS over %d chunks %.3e, channel %d call %d chunk %d" % (len(errs), e, c, k, j))
    assert e <= DC.TOL
