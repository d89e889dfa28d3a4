"""GPU tier (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on identical inputs.

Bars (BASELINE.json north_star): time-domain rel-RMS <= 1e-5 on >= 3 output frames including the first
(transients); spectrum max |dB| <= 0.1 over bins the oracle puts above -110 dB, from frame 1 on (frame 0
averages with an uninitialised buffer in the reference, fft.cpp:107-115; both sides here start it at zero).
The device computes in fp32 (fp64 only in recurrences and the oscillator phase); typical error is ~1e-7.
"""
import numpy as np
import pytest

from tests.signals import lcg_noise, tones

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_DB = 0.1
# Paths through a running AGC, during the first half second of a stream: the AGC's log detector turns the fp32 floor of the
# band-pass output's first, near-silent samples (3e-8 absolute, under full-level samples of the same overlap-save block) into a
# different start-up value of its decay average, whose trace (100 ms time constant) sets the gain later on.  The oracle does
# the same to itself: tests/test_oracle_pins.py::test_agc_remembers_the_silence_it_started_in.  The AGC kernel itself matches
# the oracle's AGC to 3e-8 on identical input (tools/diag/agc_iso.py).
TOL_AGC_STARTUP = 5e-5


def rel_rms(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / max(np.sqrt(np.mean(np.abs(b) ** 2)), 1e-12))


def db_err(g, r):
    m = r > -110
    return float(np.abs(g - r)[m].max())


# ------------------------------------------------------------------------------------------------
# stand-alone steps (reference class shapes)
# ------------------------------------------------------------------------------------------------
def test_mixer_step_with_retune(gpu_lib, oracle_mod):
    """Mixer::processBlock incl. the start-up amplitude transient, state across frames and a mid-stream retune."""
    import pebblesdr_amd as P
    fs = 2.048e6
    x = tones(fs, 6 * 2048, [(0.5, 100e3), (0.2, -300e3)]) + lcg_noise(6 * 2048, 2, 1e-3)
    ref, mx = oracle_mod.Mixer(fs), P.Mixer(fs, 2048)
    for f in range(6):
        if f == 0:
            ref.set_frequency(100e3); mx.setFrequency(100e3)
        if f == 3:
            ref.set_frequency(-250e3); mx.setFrequency(-250e3)
        fr = x[f * 2048:(f + 1) * 2048]
        assert rel_rms(mx.processBlock(fr), ref.process(fr)) <= TOL
    # f == 0 returns the input untouched (mixer.cpp:51-53)
    mx.setFrequency(0)
    fr = x[:2048].copy()
    assert mx.processBlock(fr) is fr


@pytest.mark.parametrize("fs,bw,n", [(2048000, 30000, 2048), (2048000, 200000, 2048), (20000000, 200000, 2048),
                                     (20000000, 30000, 16384), (100000000, 30000, 49152)])
def test_decimator_step(gpu_lib, oracle_mod, fs, bw, n):
    """Decimator::process on every chain SURVEY.md 8(a-3) lists that fits one frame without the reference's fallback."""
    import pebblesdr_amd as P
    x = tones(fs, 4 * n, [(0.5, 1000.0), (0.3, fs / 5), (0.1, -fs / 3)]) + lcg_noise(4 * n, 3, 1e-2)
    ref = oracle_mod.Decimator(fs, bw)
    d = P.Decimator(fs, n)
    assert d.buildDecimationChain(fs, bw) == ref.rate
    assert d.decBy2Stages() == ref.dec_by2_stages
    for f in range(4):
        fr = x[f * n:(f + 1) * n]
        r, g = ref.process(fr), d.process(fr)
        assert len(r) == len(g)
        assert rel_rms(g, r) <= TOL


def test_decimator_short_frames_stream_exactly(gpu_lib, oracle_mod):
    """20 Msps / 30 kHz with the reference's default 2048-sample frames: the reference's later stages see fewer
    samples than taps and silently drop to unfiltered sample skipping (decimator.cpp:602-625).  The library keeps
    exact history instead, so 2048-sample frames give the same stream as the oracle fed 16384-sample frames
    (where no stage falls back; the cascade is frame-invariant, test_oracle_pins.py)."""
    import pebblesdr_amd as P
    fs, bw = 20000000, 30000
    x = tones(fs, 48 * 2048, [(0.5, 1000.0), (0.3, fs / 5)]) + lcg_noise(48 * 2048, 3, 1e-2)
    ref = oracle_mod.Decimator(fs, bw)
    r = np.concatenate([ref.process(x[i:i + 16384]) for i in range(0, len(x), 16384)])
    d = P.Decimator(fs, 2048)
    d.buildDecimationChain(fs, bw)
    g = np.concatenate([d.process(x[i:i + 2048]) for i in range(0, len(x), 2048)])
    assert g.shape == r.shape and rel_rms(g, r) <= TOL
    # a frame that is not a whole number of decimated samples is refused
    with pytest.raises(P.PebbleGpuError) as e:
        d.process(np.zeros(1000, dtype=complex))
    assert e.value.code == -5


@pytest.mark.parametrize("fft,taps,lo,hi", [(2048, 1025, 300, 3000), (2048, 1025, -5000, 5000), (2048, 1025, -3000, -300),
                                            (2048, 1025, 1000, 1500), (8192, 4097, -5000, 5000), (4096, 2049, 300, 3000)])
def test_fastfir_step(gpu_lib, oracle_mod, fft, taps, lo, hi):
    import pebblesdr_amd as P
    n = 2048
    # one tone inside every pass-band under test plus a strong out-of-band one
    x = tones(64000, 8 * n, [(0.4873, 1000.0), (0.3, -12000.0), (0.2, 1250.0), (0.25, -1700.0)]) + lcg_noise(8 * n, 4, 1e-3)
    ref = oracle_mod.FastFIR(fft, taps)
    ref.setup(lo, hi, 0, 64000)
    f = P.FastFIR(fft, taps)
    f.SetupParameters(lo, hi, 0, 64000)
    got_any = 0
    for k in range(8):
        fr = x[k * n:(k + 1) * n]
        r, g = ref.process(fr), f.ProcessData(fr)
        assert len(r) == len(g)
        if len(r):
            got_any += 1
            assert rel_rms(g, r) <= TOL
    assert got_any >= 3
    # invalid parameters: error code, previous taps stay active (fastfir.cpp:208-216)
    with pytest.raises(P.PebbleGpuError) as e:
        f.SetupParameters(3000, 300, 0, 64000)
    assert e.value.code == -4
    ref.setup(3000, 300, 0, 64000)
    fr = x[:n]
    r, g = ref.process(fr), f.ProcessData(fr)
    assert len(r) == len(g) and (len(r) == 0 or rel_rms(g, r) <= TOL)


def test_fastfir_ragged_input_lengths(gpu_lib, oracle_mod):
    """ProcessData accepts any InLength; output count follows whole FFT blocks (fastfir.cpp:281-319)."""
    import pebblesdr_amd as P
    x = lcg_noise(7000, 8, 0.5)
    ref = oracle_mod.FastFIR(); ref.setup(-5000, 5000, 0, 64000)
    f = P.FastFIR(); f.SetupParameters(-5000, 5000, 0, 64000)
    off = 0
    R, G = [], []
    for ln in (1, 1023, 1, 500, 3000, 2475):
        r, g = ref.process(x[off:off + ln]), f.ProcessData(x[off:off + ln])
        assert len(r) == len(g)
        R.append(r); G.append(g)
        off += ln
    assert rel_rms(np.concatenate(G), np.concatenate(R)) <= TOL


def test_am_demod_step(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    n = 2048
    t = np.arange(6 * n) / 64000.0
    am = (0.3 * (1 + 0.5 * np.cos(2 * np.pi * 1000 * t) + 0.2 * np.cos(2 * np.pi * 3300 * t))) * np.exp(0.7j) + lcg_noise(6 * n, 5, 1e-4)
    ref = oracle_mod.DemodAM(64000, 10000)
    d = P.Demod(64000, 256000, n)
    d.setDemodMode(P.DM_AM)
    d.setBandwidth(10000)
    for k in range(6):
        fr = am[k * n:(k + 1) * n]
        if k == 4:  # re-design mid-stream: CFir::InitLPFilter also clears the delay line
            ref.set_bandwidth(6000); d.setBandwidth(6000)
        assert rel_rms(d.processBlock(fr), ref.process(fr)) <= TOL
    # pass-through modes hand back the input pointer (demod.cpp:127-138)
    d.setDemodMode(P.DM_USB)
    fr = am[:n].copy()
    assert d.processBlock(fr) is fr


def test_nfm_pll_demod_step(gpu_lib, oracle_mod):
    """Demod_NFM::processBlockNCO (2nd-order PLL, float loop state) + 75-tap CFir;
    checked against the oracle restatement, including a ragged final call."""
    import pebblesdr_amd as P
    n = 2048
    t = np.arange(6 * n) / 64000.0
    fm = 0.3 * np.exp(1j * 3.0 * np.sin(2 * np.pi * 1000 * t)) + lcg_noise(6 * n, 7, 1e-3)
    ref = oracle_mod.DemodNFM(64000)
    d = P.Demod(64000, 256000, 2 * n)
    d.setDemodMode(P.DM_FMN)
    for off, ln in ((0, n), (n, n), (2 * n, 2 * n), (4 * n, 1000)):
        r, g = ref.process(fm[off:off + ln]), d.processBlock(fm[off:off + ln])
        assert rel_rms(g, r) <= TOL
        assert np.all(g.imag == 0)  # out[i] = <real> assigns imag 0 and the CFir keeps it 0


def test_sam_pll_demod_step(gpu_lib, oracle_mod):
    """Demod_SAM::processBlock.  The reference's PLL keeps its phase/frequency in `float`; its trajectory is chaotic
    at the last-bit level (tests/test_oracle_pins.py::test_sam_reference_algorithm_is_chaotic: a 1e-9 relative change
    of the INPUT moves the oracle's own in-phase output by ~2e-5 and decorrelates the quadrature path).  The device
    sees fp32-rounded input (6e-8), so the bar here is: in-phase path (L+R)/2 within 1e-4, quadrature path (L-R)/2
    statistically equal (RMS level within 25 %)."""
    import pebblesdr_amd as P
    n = 2048
    t = np.arange(6 * n) / 64000.0
    am = (0.3 * (1 + 0.5 * np.cos(2 * np.pi * 800 * t))) * np.exp(2j * np.pi * 30 * t) + lcg_noise(6 * n, 8, 1e-3)
    ref = oracle_mod.DemodSAM(64000)
    d = P.Demod(64000, 256000, 2 * n)
    d.setDemodMode(P.DM_SAM)
    R, G = [], []
    for off, ln in ((0, n), (n, n), (2 * n, 2 * n), (4 * n, 1000)):
        R.append(ref.process(am[off:off + ln])); G.append(d.processBlock(am[off:off + ln]))
    r, g = np.concatenate(R), np.concatenate(G)
    # the bar calibrates itself: the oracle against the oracle fed the same samples rounded to fp32 -- what the device's input
    # format alone does to the reference algorithm (measured over rates and signals: device error 0.6-1.2x of it, tools/diag/pll_err.py)
    ref32 = oracle_mod.DemodSAM(64000)
    r32 = np.concatenate([ref32.process(am[off:off + ln].astype(np.complex64)) for off, ln in ((0, n), (n, n), (2 * n, 2 * n), (4 * n, 1000))])
    own = rel_rms((r32.real + r32.imag) / 2, (r.real + r.imag) / 2)
    assert own > 1e-7  # (it IS sensitive: a linear demodulator would read ~3e-8 here)
    assert rel_rms((g.real + g.imag) / 2, (r.real + r.imag) / 2) <= max(TOL, 3 * own)
    assert rel_rms((g.real + g.imag) / 2, (r.real + r.imag) / 2) <= 1e-4
    gq, rq = (g.real - g.imag) / 2, (r.real - r.imag) / 2
    assert abs(np.std(gq[n:]) / np.std(rq[n:]) - 1) < 0.25
    # the first ~500 samples, before the float trajectories split, agree tightly in both paths
    assert rel_rms(g[:500], r[:500]) <= 1e-5


@pytest.mark.parametrize("fsw", [256000, 312500, 390625])
def test_wfm_mono_demod_step(gpu_lib, oracle_mod, fsw):
    """processDataMono at the three WFM rates SURVEY.md 8(a-3) lists.  All three run the one-kernel path (k_wfm_fir, no scan at
    all); the last call spans twenty of its 1024-output workgroups with a ragged last one.  The sequential path, the Llp == 1
    branch and the short-call history merge are in tests/test_demod_geometry_gpu.py."""
    import pebblesdr_amd as P
    n = 2048
    tw = np.arange(15 * n) / fsw
    fm = 0.5 * np.exp(1j * (75000 / 1000.0) * np.sin(2 * np.pi * 1000 * tw)) + lcg_noise(15 * n, 6, 1e-4)
    ref = oracle_mod.DemodWFM(fsw)
    d = P.Demod(64000, fsw, 12 * n)
    d.setDemodMode(P.DM_FMM)
    off = 0
    for ln in (n, n, 3 * n, 10 * n - 100):
        fr = fm[off:off + ln]
        assert rel_rms(d.processBlock(fr), ref.process(fr)) <= TOL
        off += ln


def _fm_stereo_mpx(fs, n_samples, pilot_phase=1.0):
    """an FM-stereo multiplex (1 kHz left, 2.5 kHz right, 19 kHz pilot, 38 kHz DSB difference) on a 75 kHz-deviation carrier"""
    t = np.arange(n_samples) / fs
    left, right = 0.9 * np.sin(2 * np.pi * 1000 * t), 0.9 * np.sin(2 * np.pi * 2500 * t)
    mpx = 0.45 * (left + right) + 0.1 * np.sin(2 * np.pi * 19000 * t + pilot_phase) + 0.45 * (left - right) * np.sin(2 * (2 * np.pi * 19000 * t + pilot_phase))
    return 0.5 * np.exp(1j * 2 * np.pi * 75000 * np.cumsum(mpx) / fs)


@pytest.mark.parametrize("fsw", [256000, 312500])
@pytest.mark.parametrize("pilot_phase", [1.0, 2.5])
def test_wfm_stereo_mode_is_the_reference_from_the_first_block(gpu_lib, oracle_mod, fsw, pilot_phase):
    """dmFMS (include/pebblegpu.h at pebblegpu_set_demod_mode): processDataStereo restated line by line in the oracle.  Its pilot
    PLL loses lock within the first three blocks and from then on the block delivers the discriminator output, without
    processDataMono's 75 kHz pre-filter, in both channels; a block that ENDS with the lock average under its threshold (pilot phase
    1.0: the first two) is demultiplexed -- left - right = 2 raw sin(2 phase) through the same audio filters.  The device runs that
    loop serially per channel until the first block without lock (k_wfm_pilot) and adds the (L - R) part (k_wfm_lmr_fir): every
    block from the first at 1e-5, both channels.  Switching FMS -> FMM -> FMS on a running stream follows the oracle too (the loop's
    state stays as it was: the channel remains dropped), except for the switch transient: the reference carries the discriminator's
    last sample and the mono pre-filter's state across the switch (one filtered, one not), the device reads the true input history
    -- a one-sample difference that rings through the audio filters' ~700-tap response, so the first block after a switch is
    compared behind it."""
    import pebblesdr_amd as P
    n, blocks = 2048, 16
    x = _fm_stereo_mpx(fsw, n * blocks, pilot_phase) + lcg_noise(n * blocks, 9, 1e-4)
    ref = oracle_mod.DemodWFM(fsw)
    d = P.Demod(64000, fsw, 4 * n)
    d.setDemodMode(P.DM_FMS)
    locks = []
    for k in range(10):
        fr = x[k * n:(k + 1) * n]
        r, lk = ref.process_stereo(fr)
        g = d.processBlock(fr)
        locks.append(lk)
        assert rel_rms(g.real, r.real) <= TOL and rel_rms(g.imag, r.imag) <= TOL, (k, locks)
        got_lock, got_changed = d.getStereoLock()           # Demod_WFM::getStereoLock: the block's lock flag, and whether it changed
        assert got_lock == lk and got_changed == (lk != (locks[-2] if k else True)), (k, locks)
        if lk:
            assert not np.array_equal(r.real, r.imag)  # a demultiplexed block: the channels differ
        if k >= 4:
            assert np.array_equal(g.real, g.imag)      # one signal in both channels once the (L - R) part has rung out
    assert not any(locks[3:])
    if pilot_phase == 1.0 and fsw == 312500:
        assert locks[0] and locks[1]                    # this case exercises the demultiplexed blocks
    d.setDemodMode(P.DM_FMM)
    for k in range(10, 13):
        fr = x[k * n:(k + 1) * n]
        r, g = ref.process(fr), d.processBlock(fr)
        lo = 1024 if k == 10 else 0
        assert rel_rms(g[lo:], r[lo:]) <= TOL
    d.setDemodMode(P.DM_FMS)
    for k in range(13, 16):
        fr = x[k * n:(k + 1) * n]
        r, lk = ref.process_stereo(fr)
        g = d.processBlock(fr)
        lo = 1024 if k == 13 else 0
        assert not lk and rel_rms(g[lo:], r[lo:]) <= TOL


def test_wfm_stereo_mode_in_the_receiver(gpu_lib, oracle_mod):
    """The same through the whole chain: a 2.5 Msps WFM receiver in dmFMS against the oracle's Receiver in the same mode, every
    super-frame from the first, the first two in one call."""
    import pebblesdr_amd as P
    fs, n = 2_500_000, 2048
    rx = P.ReceiverBank(fs, 1, True, True, 0, max_superframes=2)
    rx.set_mode(0, P.DM_FMS)
    rx.set_mixer(0, 250e3)
    sf = rx.superframe
    K = 8
    base = _fm_stereo_mpx(fs, K * sf)
    x = base * np.exp(2j * np.pi * 250e3 * np.arange(K * sf) / fs) + lcg_noise(K * sf, 4, 1e-4)
    ref = oracle_mod.Receiver(fs, n, 0)
    ref.set_mode(oracle_mod.FMS)
    ref.set_mixer(250e3)
    ra = []
    for f in range(K * sf // n):
        a, _ = ref.process(x[f * n:(f + 1) * n], want_spectrum=False)
        if len(a):
            ra.append(a)
    first = rx.process(x[:2 * sf])[0][0]  # two demodulator blocks in one call: the lock decision is per block of frames_per_buffer samples
    ga = [first[:n], first[n:]] + [rx.process(x[k * sf:(k + 1) * sf])[0][0] for k in range(2, K)]
    assert len(ra) == K
    assert not np.array_equal(ra[0].real, ra[0].imag)  # the oracle demultiplexes the first block of this stream (pilot phase 1.0)
    for k in range(K):  # from the first super-frame on: the blocks before the pilot PLL's drop-out included
        assert rel_rms(ga[k].real, ra[k].real) <= TOL and rel_rms(ga[k].imag, ra[k].imag) <= TOL, k
    for k in range(4, K):
        assert np.array_equal(ga[k].real, ga[k].imag)


@pytest.mark.parametrize("fsw", [250000, 312500])
def test_wfm_stereo_rds_branch_against_the_oracle(gpu_lib, oracle_mod, fsw):
    """The RDS branch of processDataStereo (demod_wfm.cpp:296-357, 488-786; tests/test_oracle_pins.py for what the reference's branch
    does with a broadcast multiplex): m_RdsData -- the matched filter's output, behind the down-converter, the low-pass and the PLL -- of
    every processBlock call at 1e-6 (the branch runs in double on the device as in the reference; both sides are handed the same
    single-precision samples, the step's upload format: the wanted signal sits ~70 dB under the multiplex), and the groups
    Demod::fmStereo's one getNextRdsGroupData per call pops, with the function's return values, bit for bit.  The audio of the same calls
    stays at 1e-5."""
    import pebblesdr_amd as P
    from tests import rds_signal as rs
    ng, blk = 24, 4096
    groups = rs.make_groups(ng, seed=11)
    n = int(fsw * (ng * 104 + 60) / 1187.5)
    n -= n % blk
    x = rs.fm_multiplex(groups, float(fsw), n, subcarrier_offset_hz=-14.0).astype(np.complex64).astype(np.complex128)
    ref = oracle_mod.DemodWFM(float(fsw))
    d = P.Demod(64000, fsw, blk)
    d.setDemodMode(P.DM_FMS)
    want = []
    worst = 0.0
    for k in range(n // blk):
        fr = x[k * blk:(k + 1) * blk]
        r, _ = ref.process_stereo(fr)
        g = d.processBlock(fr)
        assert rel_rms(g.real, r.real) <= TOL and rel_rms(g.imag, r.imag) <= TOL, k
        popped = ref.next_rds_group()
        if popped is not None:
            want.append(popped)
        if k % 8 == 0 or k < 4:
            rd, gd = ref.rds_last()[0], d.rdsData()
            assert len(rd) == len(gd) == blk * ref.rds_rate / fsw
            worst = max(worst, rel_rms(gd, rd))
    # measured 5e-8, in the blocks where the loop's residual rotation carries the subcarrier through the real axis: m_RdsData is the
    # imaginary part only, there a small projection of the signal, and the 1e-10 rad by which the oscillator's closed form and the
    # reference's recurrence have drifted apart after 5e5 samples leaks the real part into it, weighted hundreds of times
    assert worst <= 1e-6, worst
    got_g, got_c = d.getNextRdsGroupData()
    assert len(want) >= 12                                       # (most of the 24 groups come through at this subcarrier offset)
    assert [tuple(int(v) for v in row) for row in got_g] == [g for g, _ in want]
    assert list(got_c) == [c for _, c in want]
    sent = [tuple(g) for g in groups]
    assert sum(1 for g, _ in want if g in sent) >= 12
    assert d.getNextRdsGroupData()[0].shape == (0, 4)            # drained


def test_wfm_stereo_rds_groups_in_the_receiver(gpu_lib, oracle_mod):
    """RDS through the whole chain: a 2.5 Msps WFM receiver in dmFMS, 16 super-frames (= frames of the demodulator) per call, against
    the oracle's Receiver fed frame by frame: the groups Demod::fmStereo pops (one getNextRdsGroupData per demodulated frame) and
    their changed flags.  The receive chain in front of the branch runs in single precision here and in double in the oracle: the
    image the decoder works on (see above) keeps three digits, enough for the same bits on this input."""
    import pebblesdr_amd as P
    from tests import rds_signal as rs
    fs, nf, ksf = 2_500_000, 2048, 16
    rx = P.ReceiverBank(fs, 1, True, True, 0, max_superframes=ksf)
    rx.set_mode(0, P.DM_FMS)
    rx.set_mixer(0, 250e3)
    sf = rx.superframe
    ng = 16
    groups = rs.make_groups(ng, seed=12)
    n = int(fs * (ng * 104 + 60) / 1187.5)
    n -= n % (ksf * sf)
    x = rs.fm_multiplex(groups, float(fs), n, subcarrier_offset_hz=-14.0) * np.exp(2j * np.pi * 250e3 * np.arange(n) / fs)
    ref = oracle_mod.Receiver(fs, nf, 0)
    ref.set_mode(oracle_mod.FMS)
    ref.set_mixer(250e3)
    for f in range(n // nf):
        ref.process(x[f * nf:(f + 1) * nf], want_spectrum=False)
    want_g, want_c = ref.rds_polled()
    got_g, got_c = [], []
    for k in range(n // (ksf * sf)):
        rx.process(x[k * ksf * sf:(k + 1) * ksf * sf])
        if k % 3 == 2:                                           # read now and then, not after every call
            g, c = rx.rds_groups(0)
            got_g += [tuple(int(v) for v in r) for r in g]; got_c += list(c)
    g, c = rx.rds_groups(0)
    got_g += [tuple(int(v) for v in r) for r in g]; got_c += list(c)
    assert len(want_g) >= 6
    assert got_g == [tuple(int(v) for v in r) for r in want_g]
    assert got_c == list(want_c)


def test_wfm_stereo_rds_refuses_what_the_branch_cannot_stream(gpu_lib):
    """dmFMS calls must be whole numbers of the RDS down-converter's decimation (CDownConvert halves odd lengths stage by stage in the
    reference -- not reproduced) and at least as long as its widest stage; a refused call leaves the object usable and dmFMM is not
    affected."""
    import pebblesdr_amd as P
    fsw = 250000
    d = P.Demod(64000, fsw, 4096)
    d.setDemodMode(P.DM_FMS)
    x = (0.5 * np.exp(2j * np.pi * 0.01 * np.arange(4096))).astype(np.complex128)
    with pytest.raises(P.PebbleGpuError):
        d.processBlock(x[:2052])          # 2052 = 8 * 256.5
    assert d.processBlock(x[:2048]).shape == (2048,)
    g, c = d.getNextRdsGroupData()
    assert g.shape == (0, 4) and len(c) == 0
    d.setDemodMode(P.DM_FMM)
    assert d.processBlock(x[:2052]).shape == (2052,)


def test_wfm_bank_rds_of_two_stations_in_one_stream(gpu_lib, oracle_mod):
    """Two broadcast multiplexes in one 2.5 Msps stream, a WFM bank of three channels off it -- dmFMS on the first station, dmFMM on it
    too, dmFMS on the second station: every dmFMS channel runs its own RDS branch (own down-converter history, PLL, block synchroniser
    and group queue) and delivers the groups and flags the oracle's Receiver tuned the same way delivers; the mono channel has none."""
    import pebblesdr_amd as P
    from tests import rds_signal as rs
    fs, nf, ksf = 2_500_000, 2048, 16
    tune = (250e3, 250e3, -600e3)
    modes = (P.DM_FMS, P.DM_FMM, P.DM_FMS)
    rx = P.ReceiverBank(fs, 3, True, True, 0, max_superframes=ksf)
    for c in range(3):
        rx.set_mode(c, modes[c]); rx.set_mixer(c, tune[c])
    sf = rx.superframe
    ng = 12
    ga, gb = rs.make_groups(ng, seed=21), rs.make_groups(ng, seed=22, pi=0x1234)
    n = int(fs * (ng * 104 + 60) / 1187.5)
    n -= n % (ksf * sf)
    t = np.arange(n) / fs
    x = rs.fm_multiplex(ga, float(fs), n, subcarrier_offset_hz=-14.0, seed=5) * np.exp(2j * np.pi * 250e3 * t) \
        + 0.7 * rs.fm_multiplex(gb, float(fs), n, subcarrier_offset_hz=-13.0, seed=6) * np.exp(-2j * np.pi * 600e3 * t)
    want = {}
    for c in (0, 2):
        ref = oracle_mod.Receiver(fs, nf, 0)
        ref.set_mode(oracle_mod.FMS); ref.set_mixer(tune[c])
        for f in range(n // nf):
            ref.process(x[f * nf:(f + 1) * nf], want_spectrum=False)
        g, ch = ref.rds_polled()
        want[c] = ([tuple(int(v) for v in r) for r in g], list(ch))
        assert len(g) >= 4
    assert want[0][0] != want[2][0]
    for k in range(n // (ksf * sf)):
        rx.process(x[k * ksf * sf:(k + 1) * ksf * sf])
    for c in (0, 2):
        g, ch = rx.rds_groups(c)
        assert [tuple(int(v) for v in r) for r in g] == want[c][0], c
        assert list(ch) == want[c][1], c
    assert len(rx.rds_groups(1)[0]) == 0


def test_wfm_bank_with_mono_and_stereo_channels(gpu_lib, oracle_mod):
    """dmFMM and dmFMS side by side in one WFM bank off a shared stream (the pre-filter switch is per channel)."""
    import pebblesdr_amd as P
    fs, n = 2_500_000, 2048
    rx = P.ReceiverBank(fs, 2, True, True, 0, max_superframes=1)
    modes = (P.DM_FMM, P.DM_FMS)
    refs = []
    for c, m in enumerate(modes):
        rx.set_mode(c, m); rx.set_mixer(c, 250e3)
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.FMM if m == P.DM_FMM else oracle_mod.FMS); r.set_mixer(250e3)
        refs.append(r)
    sf = rx.superframe
    K = 7
    x = _fm_stereo_mpx(fs, K * sf) * np.exp(2j * np.pi * 250e3 * np.arange(K * sf) / fs) + lcg_noise(K * sf, 6, 1e-4)
    want = [[], []]
    for f in range(K * sf // n):
        for c in range(2):
            a, _ = refs[c].process(x[f * n:(f + 1) * n], want_spectrum=False)
            if len(a):
                want[c].append(a)
    for k in range(K):
        g = rx.process(x[k * sf:(k + 1) * sf])[0]
        for c in range(2):  # from the first super-frame: the stereo channel's blocks before its pilot PLL drops out included
            assert rel_rms(g[c].real, want[c][k].real) <= TOL and rel_rms(g[c].imag, want[c][k].imag) <= TOL, (k, c)
    # the two channels do differ (the mono path's 75 kHz pre-filter): the switch is really per channel
    assert rel_rms(g[0], g[1]) > 1e-4


def test_wfm_bank_of_stereo_channels_with_their_own_pilot_loops(gpu_lib, oracle_mod):
    """Three dmFMS channels in one WFM bank, independent streams with different pilot phases (one of them locks for two blocks, the
    others for none): every channel runs its own pilot loop (k_wfm_pilot: one lane per channel) and gets its own (L - R) part; each
    against the oracle's Receiver from the first super-frame, two super-frames in the first call."""
    import pebblesdr_amd as P
    fs, n = 2_500_000, 2048
    phases = (1.0, 2.5, 3.67)
    rx = P.ReceiverBank(fs, 3, False, True, 0, max_superframes=2)
    refs = []
    for c in range(3):
        rx.set_mode(c, P.DM_FMS); rx.set_mixer(c, 250e3)
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.FMS); r.set_mixer(250e3)
        refs.append(r)
    sf = rx.superframe
    K = 5
    t = np.arange(K * sf)
    x = np.stack([_fm_stereo_mpx(fs, K * sf, ph) * np.exp(2j * np.pi * 250e3 * t / fs) + lcg_noise(K * sf, 6 + c, 1e-4) for c, ph in enumerate(phases)])
    want = [[], [], []]
    for f in range(K * sf // n):
        for c in range(3):
            a, _ = refs[c].process(x[c, f * n:(f + 1) * n], want_spectrum=False)
            if len(a):
                want[c].append(a)
    first = rx.process(x[:, :2 * sf])[0]
    got = [[first[c][:n], first[c][n:]] for c in range(3)]
    for k in range(2, K):
        g = rx.process(x[:, k * sf:(k + 1) * sf])[0]
        for c in range(3):
            got[c].append(g[c])
    assert not np.array_equal(want[0][0].real, want[0][0].imag)  # channel 0's first block is demultiplexed by the oracle
    for c in range(3):
        for k in range(K):
            assert rel_rms(got[c][k].real, want[c][k].real) <= TOL and rel_rms(got[c][k].imag, want[c][k].imag) <= TOL, (c, k)


@pytest.mark.parametrize("bins", [2048, 4096, 8192, 16384, 32768])
def test_spectrum_step(gpu_lib, oracle_mod, bins):
    """fftSpectrum: window, pruned zero-pad FFT, unfold, previous-frame averaging, dB, clip."""
    import pebblesdr_amd as P
    fs = 2.048e6
    x = tones(fs, 4 * 2048, [(10 ** (-10 / 20), 123456.7), (10 ** (-40 / 20), -700001.3)]) + lcg_noise(4 * 2048, 1, 1e-4)
    ref = oracle_mod.Spectrum(bins, 2048)
    sp = P.Spectrum(bins, fs, 2048)
    assert sp.bins == bins
    for f in range(4):
        fr = x[f * 2048:(f + 1) * 2048]
        r = ref.process(fr)
        g, ov = sp.fftSpectrum(fr)
        assert not ov
        assert db_err(g, r) <= TOL_DB
        assert g.min() >= -120.0 and g.max() <= 0.0
    _, ov = sp.fftSpectrum(np.full(2048, 0.95 + 0j))
    assert ov  # m_overLimit = 0.9, fft.cpp:137-140


@pytest.mark.parametrize("nf,bins", [(1024, 2048), (1024, 8192), (4096, 4096), (4096, 16384), (8192, 8192), (8192, 32768), (16384, 16384), (16384, 32768),
                                     (3000, 4096)])
def test_spectrum_step_for_other_frame_lengths(gpu_lib, oracle_mod, nf, bins):
    """FFT::fftSpectrum for framesPerBuffer != 2048 (a setting, settings.cpp:57; 3000: not a power of two): window of the frame's
    length, zero-padding to the bin count, unfold, previous-frame average, dB -- five frames against the oracle."""
    import pebblesdr_amd as P
    fs = 2.048e6
    x = tones(fs, 5 * nf, [(10 ** (-10 / 20), 123456.7), (10 ** (-40 / 20), -700001.3)]) + lcg_noise(5 * nf, 1, 1e-4)
    ref = oracle_mod.Spectrum(bins, nf)
    sp = P.Spectrum(bins, fs, nf)
    assert sp.bins == bins
    for f in range(5):
        fr = x[f * nf:(f + 1) * nf]
        r = ref.process(fr)
        g, ov = sp.fftSpectrum(fr)
        assert not ov
        if f:
            assert db_err(g, r) <= TOL_DB, f
        assert g.min() >= -120.0 and g.max() <= 0.0


@pytest.mark.parametrize("nf,bins,n", [(2048, 4096, 1500), (2048, 2048, 2047), (4096, 8192, 1024), (1024, 2048, 1000)])
def test_spectrum_step_with_fewer_samples_than_the_buffer(gpu_lib, oracle_mod, nf, bins, n):
    """The other branch of FFT::m_applyWindow (fft.cpp:129-157): numSamples != samplesPerBuffer copies the samples, zero-pads
    and applies NO window (the scale still divides by the window's coherent gain).  Four calls of n samples against the oracle;
    a spectrum object serves whole buffers or short ones, not both (its previous-frame average is kept per kernel family)."""
    import pebblesdr_amd as P
    fs = 2.048e6
    x = tones(fs, 4 * n, [(10 ** (-10 / 20), 123456.7), (10 ** (-40 / 20), -700001.3)]) + lcg_noise(4 * n, 2, 1e-4)
    ref = oracle_mod.Spectrum(bins, nf)
    sp = P.Spectrum(bins, fs, nf)
    for f in range(4):
        fr = x[f * n:(f + 1) * n]
        r = ref.process(fr)
        g, _ = sp.fftSpectrum(fr)
        if f:
            assert db_err(g, r) <= TOL_DB, f
    if nf == 2048:
        with pytest.raises(P.PebbleGpuError):
            sp.fftSpectrum(x[:nf])  # the same object with a whole buffer: refused, loudly


def test_spectrum_step_overload_flag_is_a_member_that_whole_buffers_rewrite(gpu_lib, oracle_mod):
    """FFT::m_isOverload is cleared and set on the whole-buffer branch of m_applyWindow only (fft.cpp:133-140); a shorter call tests
    nothing and returns the member as it stands (pinned to the reference binary by tests/test_reference_pins.py, case
    spectrum_overload_then_short).  An object that only ever sees short calls therefore never reports an overload."""
    import pebblesdr_amd as P
    hot = np.full(1500, 0.95 + 0j)
    ref = oracle_mod.Spectrum(2048, 2048)
    sp = P.Spectrum(2048, 2.048e6, 2048)
    for _ in range(2):
        ref.process(hot)
        _, ov = sp.fftSpectrum(hot)
        assert ov == ref.overload == False  # noqa: E712
    whole = P.Spectrum(2048, 2.048e6, 2048)
    ref = oracle_mod.Spectrum(2048, 2048)
    for fr, want in ((np.full(2048, 0.95 + 0j), True), (np.full(2048, 0.5 + 0j), False)):
        ref.process(fr)
        _, ov = whole.fftSpectrum(fr)
        assert ov == ref.overload == want
    with pytest.raises(P.PebbleGpuError):
        whole.fftSpectrum(hot)  # refused (an object of whole buffers): the member stays as the last whole buffer left it
    ref.process(np.full(2048, 0.5 + 0j))
    _, ov = whole.fftSpectrum(np.full(2048, 0.5 + 0j))
    assert ov == ref.overload == False  # noqa: E712
    # 4096-sample buffers into 8192 bins go through the general kernel, which takes whole and shorter calls on one object: the
    # sequence of the reference pin -- a hot whole buffer, then a short call that keeps True, a cool whole one, a hot short one
    ref = oracle_mod.Spectrum(8192, 4096)
    sp = P.Spectrum(8192, 2.048e6, 4096)
    for fr, want in ((np.full(4096, 0.95 + 0j), True), (np.full(1000, 0.5 + 0j), True), (np.full(4096, 0.5 + 0j), False),
                     (np.full(1000, 0.95 + 0j), False)):
        ref.process(fr)
        _, ov = sp.fftSpectrum(fr)
        assert ov == ref.overload == want


def test_receiver_with_4096_sample_frames(gpu_lib, oracle_mod):
    """A receiver created with framesPerBuffer = 4096 (settings.cpp:57): the display transform of every 4096-sample frame at 8192
    bins and the AM chain, against an oracle receiver of the same frame length."""
    import pebblesdr_amd as P
    fs, n, bins = 2048000, 4096, 8192
    rx = P.ReceiverBank(fs, 1, True, False, bins, frames_per_buffer=n, max_superframes=1)
    rx.set_mode(0, P.DM_AM); rx.set_mixer(0, 100e3); rx.set_bandpass(0, -5000, 5000)
    sf = rx.superframe
    t = np.arange(2 * sf) / fs
    x = 0.3 * (1 + 0.5 * np.cos(2 * np.pi * 1000 * t)) * np.exp(2j * np.pi * 100e3 * t) + lcg_noise(2 * sf, 9, 1e-3)
    ref = oracle_mod.Receiver(fs, n, bins)
    ref.set_mode(oracle_mod.AM); ref.set_mixer(100e3); ref.set_filter(-5000, 5000)
    ra, rs = [], []
    for f in range(2 * sf // n):
        a, sp_ = ref.process(x[f * n:(f + 1) * n])
        if a is not None and len(a):
            ra.append(a)
        rs.append(sp_)
    ra = np.concatenate(ra)
    ga, gs = [], []
    for k in range(2):
        a, sp_ = rx.process(x[k * sf:(k + 1) * sf])
        ga.append(a[0]); gs.append(sp_[0])
    ga = np.concatenate(ga); gs = np.concatenate(gs)
    assert gs.shape == (2 * sf // n, bins)
    for f in range(1, gs.shape[0]):
        assert db_err(gs[f], rs[f]) <= TOL_DB, f
    assert ra.shape == ga.shape
    for k in range(len(ga) // n):
        assert rel_rms(ga[k * n:(k + 1) * n], ra[k * n:(k + 1) * n]) <= TOL, k


def test_spectrum_known_answer_on_device(gpu_lib):
    """The reference's own table (fft.cpp:363-369) straight from the device: -10 dB tone at 48 kHz / 1 Msps."""
    import pebblesdr_amd as P
    x = tones(1e6, 2 * 2048, [(10 ** (-10 / 20), 48000.0)])
    for bins, want in ((2048, -10.3044), (4096, -10.1264), (8192, -10.0096), (16384, -10.0096), (32768, -10.0002)):
        sp = P.Spectrum(bins, 1e6, 2048)
        sp.fftSpectrum(x[:2048])
        g, _ = sp.fftSpectrum(x[2048:])
        assert abs(g.max() - want) < 2e-3


# ------------------------------------------------------------------------------------------------
# the receiver bank (Receiver::processIQData)
# ------------------------------------------------------------------------------------------------
def test_config1_am_host_frame_path(gpu_lib, oracle_mod):
    """BASELINE config 1 shape: 2.048 Msps, 1 channel, AM, through the CB_ProcessIQData-shaped host path, with the
    stock 2048/1025 FastFIR; spectrum 4096 bins every frame; 3 audio frames incl. the first."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    ref = oracle_mod.Receiver(fs, n, 4096)
    ref.set_mode(oracle_mod.AM); ref.set_mixer(100e3); ref.set_filter(-5000, 5000)
    rx = P.ReceiverBank(fs, 1, True, False, 4096)
    rx.set_mode(0, P.DM_AM); rx.set_mixer(0, 100e3); rx.set_bandpass(0, -5000, 5000)
    nfr = 3 * 32
    t = np.arange(nfr * n) / fs
    x = 10 ** (-10 / 20) * (1 + 0.5 * np.cos(2 * np.pi * 1000 * t)) * np.exp(2j * np.pi * 100e3 * t) + lcg_noise(nfr * n, 1, 3e-4)
    x = np.round(x * 32767.0) / 32767.0  # 16-bit PCM WAV scaling, wavfile.cpp:299-300
    audio_frames = 0
    for f in range(nfr):
        fr = x[f * n:(f + 1) * n]
        ra, rs = ref.process(fr)
        ga, gs = rx.process_iq(fr, want_spectrum=(f < 4))
        assert len(ra) == len(ga)
        if 1 <= f < 4:
            assert db_err(gs, rs) <= TOL_DB
        if len(ra):
            audio_frames += 1
            assert rel_rms(ga, ra) <= TOL
    assert audio_frames == 3


def test_config1_variant_8192_fastfir(gpu_lib, oracle_mod):
    """Config 1's '4096-tap' band-pass = the parametrised 8192/4097 FastFIR: audio comes out 4096 at a time."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    ref = oracle_mod.Receiver(fs, n, 0, 8192, 4097)
    ref.set_mode(oracle_mod.AM); ref.set_mixer(100e3); ref.set_filter(-5000, 5000)
    rx = P.ReceiverBank(fs, 1, True, False, 0, fastfir_fft=8192, fastfir_taps=4097)
    rx.set_mode(0, P.DM_AM); rx.set_mixer(0, 100e3); rx.set_bandpass(0, -5000, 5000)
    nfr = 6 * 32
    t = np.arange(nfr * n) / fs
    x = 0.3 * (1 + 0.5 * np.cos(2 * np.pi * 1000 * t)) * np.exp(2j * np.pi * 100e3 * t) + lcg_noise(nfr * n, 1, 3e-4)
    got = 0
    for f in range(nfr):
        fr = x[f * n:(f + 1) * n]
        ra, _ = ref.process(fr, want_spectrum=False)
        ga, _ = rx.process_iq(fr)
        assert len(ra) == len(ga)
        if len(ra):
            got += 1
            assert len(ra) == 4096 and rel_rms(ga, ra) <= TOL
    assert got == 3


@pytest.mark.parametrize("route", ["default", "one-wave transform, pipelined calls", "decimator inside the display transform"])
def test_config2_wfm_with_spectrum(gpu_lib, oracle_mod, monkeypatch, route):
    """BASELINE config 2 (the bench workload) at parity size: 20 Msps HackRF-shape int8 IQ, 1 channel, mixer +1 MHz,
    chain hb11x8,hb15,hb23,hb47 -> 312.5 kHz, WFM mono, 8192-bin spectrum on every 2048-sample frame.
    The oracle runs frame size 8192 (>= every stage's taps) because the cascade is frame-invariant
    (tests/test_oracle_pins.py::test_decimator_is_frame_invariant) and 2048 would hit the reference's fallback.
    Second route: the opt-in kernel on the one-wave transform (fft_w64.h) with calls that do not join their two streams."""
    import pebblesdr_amd as P
    fs, n = 20_000_000, 2048
    if route.startswith("one-wave"):
        monkeypatch.setenv("PEBBLEGPU_SPECTRUM_W64", "1")
        monkeypatch.setenv("PEBBLEGPU_PIPELINE", "1")
    elif route.startswith("decimator"):  # k_spectrum_t128<.., DEC>: mixer + hb11 x 8, hb15, hb23, hb47 in the transform's workgroups (opt-in)
        monkeypatch.setenv("PEBBLEGPU_FUSE_DEC", "1")
    rx = P.ReceiverBank(fs, 1, True, True, 8192, max_superframes=4)
    assert rx.kernel_name(1) == ("k_spectrum_w64" if route.startswith("one-wave") else "k_spectrum_t128")
    assert rx.chain() == [(11, 8), (15, 2), (23, 2), (47, 2)] and rx.D == 64 and rx.info.demod_rate == 312500.0
    rx.set_mixer(0, 1.0e6)
    sf = rx.superframe
    N = 6 * sf
    t = np.arange(N) / fs
    x = 0.5 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(N, 2, 1e-2)
    x = (np.round(x.real * 128) + 1j * np.round(x.imag * 128)) / 128.0  # CPX8 * 1/128, deviceinterfacebase.cpp:648-658
    # reference: spectrum per 2048 frame, chain per 8192 frame, demod per 2048 demod-rate samples
    spec = oracle_mod.Spectrum(8192, 2048)
    rs = np.array([spec.process(x[f * n:(f + 1) * n]) for f in range(N // n)])
    mix = oracle_mod.Mixer(fs); mix.set_frequency(1.0e6)
    dec = oracle_mod.Decimator(fs, 200000)
    dem = oracle_mod.DemodWFM(312500)
    z = np.concatenate([dec.process(mix.process(x[i:i + 8192])) for i in range(0, N, 8192)])
    ra = np.concatenate([dem.process(z[i:i + 2048]) for i in range(0, len(z), 2048)])
    ga, gs = [], []
    for lo, hi in ((0, sf), (sf, 2 * sf), (2 * sf, 6 * sf)):  # uneven calls: 1, 1 and 4 super-frames
        a, s = rx.process(x[lo:hi])
        ga.append(a[0]); gs.append(s[0])
    ga, gs = np.concatenate(ga), np.concatenate(gs)
    if route.startswith("decimator"):  # (the first call sits in the oscillator's transient and takes the general kernels; the others are fused)
        assert rx.kernel_name(2) == "k_spectrum_t128 (decimator inside)"
    assert ga.shape == ra.shape and gs.shape == rs.shape
    for k in range(6):
        assert rel_rms(ga[k * 2048:(k + 1) * 2048], ra[k * 2048:(k + 1) * 2048]) <= TOL
    for f in range(1, N // n):
        assert db_err(gs[f], rs[f]) <= TOL_DB


def test_config3_shared_input_usb_bank(gpu_lib, oracle_mod):
    """BASELINE config 3 at parity size: 2.048 Msps shared wideband input, 32 of the 256 USB channels
    (f_c = -960 kHz + 7.5 kHz*c), one tone per channel pass-band + noise, 3 super-frames over 2 calls."""
    import pebblesdr_amd as P
    fs, n, C = 2048000, 2048, 32
    chans = [8 * c for c in range(C)]
    fcs = [-960e3 + 7.5e3 * c for c in chans]
    rng = np.random.RandomState(3)
    ph = rng.uniform(0, 2 * np.pi, 256)
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    refs = []
    for i, fc in enumerate(fcs):
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.USB); r.set_mixer(fc); r.set_filter(300, 3000)
        refs.append(r)
        rx.set_mode(i, P.DM_USB); rx.set_mixer(i, fc); rx.set_bandpass(i, 300, 3000)
    sf = rx.superframe
    assert sf == 32 * 2048
    x = tones(fs, 3 * sf, [(0.003, -960e3 + 7.5e3 * c + 1000.0 + 3.1 * c, ph[c]) for c in range(256)]) + lcg_noise(3 * sf, 3, 1e-3)
    g = np.concatenate([rx.process(x[:sf])[0], rx.process(x[sf:])[0]], axis=1)
    for i in range(C):
        r = np.concatenate([refs[i].process(x[f * n:(f + 1) * n], want_spectrum=False)[0] for f in range(3 * sf // n)])
        assert r.shape == g[i].shape
        for k in range(3):
            assert rel_rms(g[i][k * 2048:(k + 1) * 2048], r[k * 2048:(k + 1) * 2048]) <= TOL


def test_fused_decimator_with_a_ragged_last_channel_group(gpu_lib, oracle_mod):
    """The one-kernel decimator (k_mix_dec_mfma / k_mix_dec_fused) with 80 channels: the last channel group has 16 live lanes.
    Three calls of one super-frame (the second and third start from the first-stage history the kernel itself left), one
    channel without a mixer frequency (the oscillator bypass) and a retune between calls (that call takes the two-kernel
    route inside the oscillator's amplitude transient, the next one comes back)."""
    import pebblesdr_amd as P
    fs, n, C = 2048000, 2048, 80
    fcs = [-900e3 + 22.5e3 * c for c in range(C)]
    fcs[5] = 0.0
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=1)
    for c, fc in enumerate(fcs):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fc); rx.set_bandpass(c, 300, 3000)
    sf = rx.superframe
    K = 5
    x = tones(fs, K * sf, [(0.004, fcs[c] + 700.0 + 11.0 * c, 0.1 * c) for c in range(C)]) + lcg_noise(K * sf, 8, 1e-3)
    check = (0, 5, 63, 64, 79)
    refs = {}
    for c in check:
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.USB); r.set_mixer(fcs[c]); r.set_filter(300, 3000)
        refs[c] = r
    names = []
    for k in range(K):
        if k == 2:  # retune channel 64 between calls (its tone stays inside the pass-band: 1404 -> 904 Hz)
            fcs[64] += 500.0
            rx.set_mixer(64, fcs[64]); refs[64].set_mixer(fcs[64])
        g = rx.process(x[k * sf:(k + 1) * sf])[0]
        names.append(rx.kernel_name(2))
        for c in check:
            want = np.concatenate([refs[c].process(x[k * sf + f * n:k * sf + (f + 1) * n], want_spectrum=False)[0] for f in range(sf // n)])
            assert rel_rms(g[c], want) <= TOL, (k, c)
    # the first call after a (re)tune runs inside an oscillator's amplitude transient: general kernels; otherwise the fused one
    one = ("k_mix_dec_fused", "k_mix_dec_mfma")  # (PEBBLEGPU_BANK_DEC=0 selects the four-wave pipeline; the matrix-pipe kernel is the default)
    assert names[1] in one and names[4] in one and names[2] not in one


def test_bank_oscillators_advanced_on_the_device_stay_on_the_oracle_over_many_calls(gpu_lib, oracle_mod):
    """A bank too large for kernel-argument transport (> 8 channels) carries its oscillators' phases ON the device from call to
    call (OscAdvance in the tail-refresh launch; the host only mirrors them).  Sixty calls of one super-frame, frequencies that
    are not multiples of anything convenient, a change of call length half-way (the per-channel advance table is rebuilt) and a
    retune: the last calls still meet the bar against an oracle that has run the whole stream."""
    import pebblesdr_amd as P
    fs, n, C = 2048000, 2048, 24
    fcs = [-800e3 + 66123.457 * c for c in range(C)]
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    for c, fc in enumerate(fcs):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fc); rx.set_bandpass(c, 300, 3000)
    sf = rx.superframe
    check = (0, 7, 23)
    refs = {}
    for c in check:
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.USB); r.set_mixer(fcs[c]); r.set_filter(300, 3000)
        refs[c] = r
    lens = [1] * 30 + [2] * 15
    total = sum(lens) * sf
    x = tones(fs, total, [(0.01, fcs[c] + 900.0 + 13.0 * c, 0.3 * c) for c in range(C)]) + lcg_noise(total, 5, 1e-3)
    off = 0
    for k, ln in enumerate(lens):
        if k == 20:
            fcs[7] += 250.0
            rx.set_mixer(7, fcs[7]); refs[7].set_mixer(fcs[7])
        seg = x[off:off + ln * sf]
        g = rx.process(seg)[0]
        for c in check:
            want = np.concatenate([refs[c].process(seg[f * n:(f + 1) * n], want_spectrum=False)[0] for f in range(len(seg) // n)])
            if k >= len(lens) - 3 or k in (0, 19, 20, 21, 30, 31):
                assert rel_rms(g[c], want) <= TOL, (k, c)
        off += ln * sf


def test_config4_cic3_chain_mixed_am_usb(gpu_lib, oracle_mod):
    """BASELINE config 4 at parity size: 100 Msps shared input, chain cic3x16,hb11x16,hb15,hb23,hb47 (D = 2048),
    AM on even / USB on odd channels, 4 channels, 2 super-frames.  Oracle frame N = 49152 as SURVEY.md 8(d) prescribes
    (stage inputs 3072/192/96/48 >= taps)."""
    import pebblesdr_amd as P
    fs, C = 100_000_000, 4
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=1)
    assert rx.chain() == [(0, 16), (11, 16), (15, 2), (23, 2), (47, 2)] and rx.D == 2048
    fcs = [1.0e6, -7.3e6, 21.0e6, -33.5e6]
    sf = rx.superframe  # 2048*2048
    N = 2 * sf
    t = np.arange(N) / fs
    x = np.zeros(N, dtype=np.complex128)
    for i, fc in enumerate(fcs):
        if i % 2 == 0:
            x += 0.1 * (1 + 0.5 * np.cos(2 * np.pi * 800 * t)) * np.exp(2j * np.pi * fc * t)
        else:
            x += 0.1 * np.exp(2j * np.pi * (fc + 1200.0) * t)
    x += lcg_noise(N, 4, 1e-3)
    rate = int(rx.info.demod_rate_int)
    assert rate == 48828
    for i, fc in enumerate(fcs):
        rx.set_mixer(i, fc)
        if i % 2 == 0:
            rx.set_mode(i, P.DM_AM); rx.set_bandpass(i, -5000, 5000)
        else:
            rx.set_mode(i, P.DM_USB); rx.set_bandpass(i, 300, 3000)
    ga = np.concatenate([rx.process(x[:sf])[0], rx.process(x[sf:])[0]], axis=1)
    F = 49152
    for i, fc in enumerate(fcs):
        mix = oracle_mod.Mixer(fs); mix.set_frequency(fc)
        dec = oracle_mod.Decimator(fs, 30000)
        # feed the oracle 49152-sample frames; the last frame absorbs the remainder (49152..98303 samples, a multiple
        # of D = 2048) so that no stage ever sees fewer samples than taps
        z = []
        pos = 0
        while pos < N:
            ln = F if N - pos - F >= F else N - pos
            z.append(dec.process(mix.process(x[pos:pos + ln])))
            pos += ln
        z = np.concatenate(z) * 10 ** (2 * 11 / 20.0)  # gain restore, 11 stages
        ff = oracle_mod.FastFIR()
        if i % 2 == 0:
            ff.setup(-5000, 5000, 0, rate)
            am = oracle_mod.DemodAM(rate, 10000)
            r = np.concatenate([am.process(ff.process(z[k:k + 2048])) for k in range(0, len(z), 2048)])
        else:
            ff.setup(300, 3000, 0, rate)
            r = np.concatenate([ff.process(z[k:k + 2048]) for k in range(0, len(z), 2048)])
        assert r.shape == ga[i].shape
        for k in range(2):
            assert rel_rms(ga[i][k * 2048:(k + 1) * 2048], r[k * 2048:(k + 1) * 2048]) <= TOL


def test_independent_streams_and_retune(gpu_lib, oracle_mod):
    """C independent streams (shared_input = 0), a retune and a band-pass change between calls, mode switch to NONE."""
    import pebblesdr_amd as P
    fs, n, C = 2048000, 2048, 3
    rx = P.ReceiverBank(fs, C, False, False, 2048, max_superframes=1)
    refs = [oracle_mod.Receiver(fs, n, 2048) for _ in range(C)]
    f0 = [50e3, -200e3, 333e3]
    for c in range(C):
        refs[c].set_mode(oracle_mod.LSB); refs[c].set_mixer(f0[c]); refs[c].set_filter(-3000, -300)
        rx.set_mode(c, P.DM_LSB); rx.set_mixer(c, f0[c]); rx.set_bandpass(c, -3000, -300)
    sf = rx.superframe
    xs = np.stack([tones(fs, 3 * sf, [(0.2, f0[c] - 1500.0), (0.1, f0[c] + 2000.0)]) + lcg_noise(3 * sf, 10 + c, 1e-3) for c in range(C)])
    for call in range(3):
        if call == 1:
            refs[1].set_mixer(-201e3); rx.set_mixer(1, -201e3)
            refs[2].set_filter(-2500, -500); rx.set_bandpass(2, -2500, -500)
        if call == 2:
            refs[0].set_mode(oracle_mod.NONE); rx.set_mode(0, P.DM_NONE)
        a, s = rx.process(xs[:, call * sf:(call + 1) * sf])
        for c in range(C):
            outs = [refs[c].process(xs[c, call * sf + f * n: call * sf + (f + 1) * n]) for f in range(sf // n)]
            r = np.concatenate([o[0] for o in outs])
            rs = np.array([o[1] for o in outs])
            if call == 2 and c == 0:
                # dmNONE: the reference clears m_audioBuf and returns before the audio callback (receiver.cpp:968-971):
                # nothing comes out of the oracle, and the bank's row for that channel is cleared
                assert len(r) == 0 and not a[c].any()
                assert db_err(s[c], rs) <= TOL_DB  # the spectrum is taken before the branch
                continue
            assert rel_rms(a[c], r) <= TOL
            assert db_err(s[c], rs) <= TOL_DB


def test_bank_with_every_narrow_demod_mode(gpu_lib, oracle_mod):
    """One shared 2.048 Msps stream, five channels in AM / SAM / FMN / USB / CWU at once (per-channel mode lists)."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    modes = [(P.DM_AM, oracle_mod.AM, 100e3, -5000, 5000), (P.DM_SAM, oracle_mod.SAM, 200e3, -5000, 5000),
             (P.DM_FMN, oracle_mod.FMN, 300e3, -7500, 7500), (P.DM_USB, oracle_mod.USB, 400e3, 300, 3000),
             (P.DM_CWU, oracle_mod.CWU, 500e3, -1000, -500)]
    C = len(modes)
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=1)
    refs = []
    for c, (gm, om, fc, lo, hi) in enumerate(modes):
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(om); r.set_mixer(fc); r.set_filter(lo, hi)
        refs.append(r)
        rx.set_mode(c, gm); rx.set_mixer(c, fc); rx.set_bandpass(c, lo, hi)
    sf = rx.superframe
    N = 3 * sf
    t = np.arange(N) / fs
    x = (0.1 * (1 + 0.5 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * 100e3 * t)
         + 0.1 * (1 + 0.4 * np.cos(2 * np.pi * 900 * t)) * np.exp(2j * np.pi * (200e3 + 25.0) * t)
         + 0.1 * np.exp(1j * (2 * np.pi * 300e3 * t + 2.5 * np.sin(2 * np.pi * 1000 * t)))
         + 0.1 * np.exp(2j * np.pi * (400e3 + 1500.0) * t) + 0.1 * np.exp(2j * np.pi * (500e3 - 700.0) * t)) + lcg_noise(N, 6, 1e-3)
    g = np.concatenate([rx.process(x[k * sf:(k + 1) * sf])[0] for k in range(3)], axis=1)
    for c in range(C):
        r = np.concatenate([refs[c].process(x[f * n:(f + 1) * n], want_spectrum=False)[0] for f in range(N // n)])
        assert r.shape == g[c].shape
        if modes[c][0] == P.DM_SAM:
            assert rel_rms((g[c].real + g[c].imag) / 2, (r.real + r.imag) / 2) <= 1e-4  # see test_sam_pll_demod_step
        else:
            # FMN: while the band-pass is still filling (first ~600 samples) its output is at the fp32 rounding floor, so
            # the phase detector sees a different "phase of noise" than the fp64 reference and the PLL acquires along a
            # different transient; once locked (frame 1 on) the outputs agree to ~1e-7
            first = 1 if modes[c][0] == P.DM_FMN else 0
            for k in range(first, 3):
                assert rel_rms(g[c][k * 2048:(k + 1) * 2048], r[k * 2048:(k + 1) * 2048]) <= TOL


@pytest.mark.parametrize("fmt,dtype,lo,hi", [(0, np.int8, -128, 127), (1, np.uint8, 0, 255), (2, np.int16, -32768, 32767), (4, np.int16, -32768, 32767)])
def test_ingest_normalize_iq_integer_formats(gpu_lib, oracle_mod, fmt, dtype, lo, hi):
    """normalizeIQ for every integer device format, all four IQ orders, with a gain.  fp32 results of
    small-integer arithmetic: exact to the last bit of the float product, so the bar is 1e-7 relative."""
    from pebblesdr_amd import binding as B
    rng = np.random.RandomState(fmt)
    raw = rng.randint(lo, hi + 1, size=2 * 10007).astype(dtype)
    raw[:4] = [lo, hi, hi, lo]
    for order in range(4):
        g = B.normalize_iq(raw, fmt, order, gain=0.5)
        r = oracle_mod.normalize_iq(raw, fmt, order, gain=0.5)
        assert np.abs(g - r).max() <= 1e-7 * max(1.0, np.abs(r).max())


def test_ingest_normalize_iq_float(gpu_lib, oracle_mod):
    from pebblesdr_amd import binding as B
    raw = lcg_noise(5000, 3, 2.0).astype(np.complex64).view(np.float32)
    g = B.normalize_iq(raw, B.IQ_F32, B.IQO_QI, gain=1.5)
    r = oracle_mod.normalize_iq(raw, 3, 1, gain=1.5)
    assert np.abs(g - r).max() <= 2e-7 * np.abs(r).max()


# ------------------------------------------------------------------------------------------------
# BASELINE config 5: bank of full-rate streams, overlap-save band-pass + 65536-point display transform
# ------------------------------------------------------------------------------------------------
def _streambank_refs(oracle_mod, fs, bands, N):
    refs = []
    for lo, hi in bands:
        f = oracle_mod.FastFIR(2048, 1025)
        f.setup(lo, hi, 0.0, fs)
        refs.append((f, oracle_mod.Spectrum(N, N, lift_clamp=True)))
    return refs


def test_process_raw_equals_normalize_then_process(gpu_lib, oracle_mod):
    """pebblegpu_receiver_process_raw: HackRF-shape int8 pairs (and int16 in Q,I order for two independent streams) go through
    normalizeIQ on the library's stream and then the ordinary call; the audio and spectrum must be those of process() fed
    the same samples converted on the host with the reference's constants (deviceinterfacebase.cpp:651, :729)."""
    import pebblesdr_amd as P
    fs, bins = 2048000, 4096
    rng = np.random.default_rng(7)
    for fmt, dtype, scale, order, S in ((0, np.int8, 128.0, 0, 1), (2, np.int16, 32768.0, 1, 2)):
        a = P.ReceiverBank(fs, S, S == 1, True, bins, max_superframes=2)
        b = P.ReceiverBank(fs, S, S == 1, True, bins, max_superframes=2)
        for rx in (a, b):
            for c in range(S):
                rx.set_mixer(c, 150e3)
        n = 2 * a.superframe
        t = np.arange(n) / fs
        amp = 0.4 * scale
        sig = np.stack([amp * np.exp(1j * (2 * np.pi * 150e3 * t + (10.0 + 5 * k) * np.sin(2 * np.pi * 1000 * t))) for k in range(S)])
        raw = np.empty((S, n, 2), dtype=dtype)
        raw[..., 0] = np.round(sig.real + rng.uniform(-1, 1, sig.shape)).astype(dtype)
        raw[..., 1] = np.round(sig.imag + rng.uniform(-1, 1, sig.shape)).astype(dtype)
        first, second = (raw[..., 0], raw[..., 1]) if order == 0 else (raw[..., 1], raw[..., 0])  # IQ or QI on the wire
        x = (first.astype(np.float32) * np.float32(0.5 / scale) + 1j * (second.astype(np.float32) * np.float32(0.5 / scale))).astype(np.complex64)
        buf = P.DeviceBuffer.from_array(raw, 0)
        try:
            a.process_raw_device(buf.ptr, n, fmt, order, 0.5)
            ga, sa = a.audio(), a.spectrum()
        finally:
            buf.free()
        gb, sb = b.process(x)
        assert ga.shape == gb.shape and np.abs(ga).max() > 1e-3
        assert np.array_equal(ga, gb)
        assert np.array_equal(sa, sb)
    with pytest.raises(P.PebbleGpuError):
        a.process_raw_device(1, n, 9)  # unknown format


def test_process_raw_on_a_shared_stream_bank(gpu_lib):
    """pebblegpu_receiver_process_raw on a bank of 64 USB channels off one shared stream (RTL2832 uint8 pairs, then HackRF int8 in Q,I
    order with a gain): the bank's one-kernel decimator takes float2 samples, so normalizeIQ runs as one pass over the SHARED stream on
    the decimator's stream (2 + 8 bytes per input sample, once for all channels -- the bank reads the stream C / 32 times from L2 after
    that) -- three calls queued back to back (two-stage calls: each next call's conversion and decimator run beside the previous call's
    band-pass) must leave bit for bit what a twin leaves that is handed the same samples converted on the host with the reference's
    constants (deviceinterfacebase.cpp:651, :689)."""
    import pebblesdr_amd as P
    fs, C = 2048000, 64
    rng = np.random.default_rng(21)
    for fmt, dtype, off, scale, order, gain in ((1, np.uint8, 128.0, 128.0, 0, 1.0), (0, np.int8, 0.0, 128.0, 1, 0.7)):
        a = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
        b = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
        fcs = [(-0.4 + 0.8 * (c + 0.5) / C) * fs for c in range(C)]
        for rx in (a, b):
            for c in range(C):
                rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000)
        n = 2 * a.superframe
        K = 3
        sig = 40.0 * tones(fs, K * n, [(0.1, fc + 1000.0 + 30.0 * i) for i, fc in enumerate(fcs[::4])])
        raw = np.empty((K * n, 2), dtype=dtype)
        raw[:, 0] = np.clip(np.round(sig.real + rng.uniform(-1, 1, K * n) + off), 0 if off else -128, 255 if off else 127).astype(dtype)
        raw[:, 1] = np.clip(np.round(sig.imag + rng.uniform(-1, 1, K * n) + off), 0 if off else -128, 255 if off else 127).astype(dtype)
        first, second = (raw[:, 0], raw[:, 1]) if order == 0 else (raw[:, 1], raw[:, 0])
        g32 = np.float32(gain * (1 / scale))  # the library forms gain / 128 in double and rounds once
        x = ((first.astype(np.float32) - np.float32(off)) * g32 + 1j * ((second.astype(np.float32) - np.float32(off)) * g32)).astype(np.complex64)
        bufs = [P.DeviceBuffer.from_array(raw[k * n:(k + 1) * n], 0) for k in range(K)]
        try:
            for k in range(K):
                a.process_raw_device(bufs[k].ptr, n, fmt, order, gain)  # no synchronisation in between
            a.synchronize()
            ga = a.audio()
        finally:
            for bf in bufs:
                bf.free()
        for k in range(K):
            gb = b.process(x[k * n:(k + 1) * n])[0]
        assert ga.shape == gb.shape and np.abs(gb).max() > 1e-3
        assert np.array_equal(ga, gb)
        assert a.kernel_name(2) == "k_mix_dec_mfma"


def test_pinned_ingest_slots_equal_process_raw(gpu_lib):
    """pebblegpu_receiver_ingest_acquire / _submit / pebblegpu_receiver_process_ingested (the library's pinned double buffer, SURVEY 8b:
    the producer of hackrfdevice.cpp:533-566 fills the slot instead of its own ring): six batches of HackRF int8 pairs at the
    headline shape alternate through the two slots -- each next slot filled and submitted while the previous call is still queued --
    and must leave bit for bit the audio and spectra a twin receiver leaves that is handed the same batches from a device buffer.
    A slot is refused for a second submit while its call is in flight, for more bytes than were acquired, and for a format whose
    pairs do not fit what was submitted."""
    import pebblesdr_amd as P
    fs, bins = 20_000_000, 8192
    a = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=4)
    b = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=4)
    for rx in (a, b):
        rx.set_mixer(0, 150e3)
    n = 4 * a.superframe
    rng = np.random.default_rng(11)
    t = np.arange(n) / fs
    batches = []
    for k in range(6):
        sig = 90.0 * np.exp(1j * (2 * np.pi * 150e3 * t + 10.0 * np.sin(2 * np.pi * (800 + 100 * k) * t)))
        raw = np.empty((n, 2), dtype=np.int8)
        raw[:, 0] = np.round(sig.real + rng.uniform(-2, 2, n)).astype(np.int8)
        raw[:, 1] = np.round(sig.imag + rng.uniform(-2, 2, n)).astype(np.int8)
        batches.append(raw)
    h = a.ingest_buffer(0, 2 * n)
    h[:] = batches[0].reshape(-1)
    a.ingest_submit(0, 2 * n)
    got = []
    for k in range(6):
        s = k & 1
        a.process_ingested(s, n, 0, 0, 1.0)
        with pytest.raises(P.PebbleGpuError):
            a.ingest_submit(s, 2 * n)  # in flight
        if k + 1 < 6:
            h = a.ingest_buffer(s ^ 1, 2 * n)  # waits for call k-1 only; call k is still queued or running
            h[:] = batches[k + 1].reshape(-1)
            a.ingest_submit(s ^ 1, 2 * n)
        got.append((a.audio(), a.spectrum()))
    for k in range(6):
        buf = P.DeviceBuffer.from_array(batches[k], 0)
        try:
            b.process_raw_device(buf.ptr, n, 0, 0, 1.0)
            wa, ws = b.audio(), b.spectrum()
        finally:
            buf.free()
        assert np.abs(wa).max() > 1e-3
        assert np.array_equal(got[k][0], wa), k
        assert np.array_equal(got[k][1], ws), k
    h = a.ingest_buffer(0, 2 * n)
    with pytest.raises(P.PebbleGpuError):
        a.ingest_submit(0, 2 * n + 2)  # more than was acquired
    a.ingest_submit(0, 2 * n)
    with pytest.raises(P.PebbleGpuError):
        a.process_ingested(0, n, 2, 0, 1.0)  # int16 pairs need twice the bytes
    with pytest.raises(P.PebbleGpuError):
        a.ingest_buffer(2, 16)


def test_process_raw_with_zero_gain_and_squelch_never_closes(gpu_lib):
    """Two corners of the call's argument handling.  (1) pebblegpu_receiver_process_raw with gain 0 -- m_userIQGain = 0 multiplies
    every sample by zero in the reference (deviceinterfacebase.cpp:651): silence on the route that converts in the kernels' own
    loads (one WFM channel, 8192 bins) and on the route that stages through normalizeIQ (two streams), which once read the 0 as
    "no scale given".  (2) set_squelch(-120) -- "never closes" -- is accepted by a WFM receiver created for several super-frames per
    call (a threshold that could close its gate is refused there), and the receiver keeps working."""
    import pebblesdr_amd as P
    fs = 20_000_000
    rng = np.random.default_rng(3)
    for S, bins in ((1, 8192), (2, 4096)):
        rx = P.ReceiverBank(fs if S == 1 else 2048000, S, S == 1, True, bins, max_superframes=2)
        for c in range(S):
            rx.set_mixer(c, 150e3)
        rx.set_squelch(0, -120.0)
        with pytest.raises(P.PebbleGpuError):
            rx.set_squelch(0, -60.0)
        n = 2 * rx.superframe
        raw = rng.integers(-100, 100, size=(S, n, 2)).astype(np.int8)
        buf = P.DeviceBuffer.from_array(raw, 0)
        try:
            rx.process_raw_device(buf.ptr, n, 0, 0, 1.0)
            assert np.abs(rx.audio()).max() > 0
            rx.process_raw_device(buf.ptr, n, 0, 0, 0.0)
            rx.process_raw_device(buf.ptr, n, 0, 0, 0.0)  # (the second such call: the filters' memories have drained)
            a, sp = rx.audio(), rx.spectrum()
        finally:
            buf.free()
        assert np.abs(a[:, a.shape[1] // 2:]).max() < 1e-6
        assert sp[:, -1].max() <= -119.9


def test_config5_streambank_small(gpu_lib, oracle_mod):
    """3 streams x 3 calls x 2 frames of 65536: every stream has its own filter; the band-pass overlap and the
    spectrum's previous-frame average carry across calls (fastfir.cpp:312-316, fft.cpp:349-353)."""
    import pebblesdr_amd as P
    fs, S, N, F = 2.0e6, 3, 65536, 2
    bands = [(-50e3, 50e3), (-100e3, -10e3), (300.0, 3000.0)]
    x = np.stack([tones(fs, 3 * F * N, [(0.4, 123456.7 * (c + 1)), (0.01, -700001.3), (0.2, 20000.0 - 30000.0 * c), (0.1, 1700.0)])
                  + lcg_noise(3 * F * N, 70 + c, 1e-4) for c in range(S)])
    sb = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=F)
    for c in range(S):
        sb.set_bandpass(c, *bands[c])
    refs = _streambank_refs(oracle_mod, fs, bands, N)
    for call in range(3):
        blk = x[:, call * F * N:(call + 1) * F * N]
        y, sp = sb.process(blk)
        assert y.shape == (S, F * N) and sp.shape == (S, F, N)
        for c in range(S):
            assert rel_rms(y[c], refs[c][0].process(blk[c])) <= TOL
            for f in range(F):
                r = refs[c][1].process(blk[c, f * N:(f + 1) * N])
                if call or f:
                    assert db_err(sp[c, f], r) <= TOL_DB


def test_streambank_side_by_side_equals_one_stream(gpu_lib, monkeypatch):
    """PEBBLEGPU_SB_SIDE=1 (opt-in: measured equal): the band-pass on a second stream beside the display transform, fork at the call's
    start event and join at its end -- filtered streams and spectra bit for bit those of the default (one stream), three calls."""
    import pebblesdr_amd as P
    fs, S, N, F = 2.0e6, 4, 65536, 2
    x = np.stack([tones(fs, 3 * F * N, [(0.4, 123456.7 * (c + 1)), (0.2, 20000.0 - 30000.0 * c)]) + lcg_noise(3 * F * N, 70 + c, 1e-4) for c in range(S)])
    monkeypatch.setenv("PEBBLEGPU_SB_SIDE", "1")
    a = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=F)
    monkeypatch.delenv("PEBBLEGPU_SB_SIDE")
    b = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=F)
    for sb in (a, b):
        for c in range(S):
            sb.set_bandpass(c, -50e3 - 1e3 * c, 50e3)
    for call in range(3):
        blk = x[:, call * F * N:(call + 1) * F * N]
        ya, sa = a.process(blk)
        yb, sb_ = b.process(blk)
        assert np.abs(ya).max() > 1e-2
        assert np.array_equal(ya, yb) and np.array_equal(sa, sb_)


@pytest.mark.parametrize("S,F", [(128, 4), (64, 8)])
def test_config5_streambank_full_size(gpu_lib, oracle_mod, S, F):
    """BASELINE configs[4] at size: 128 streams x 4 frames -- bench.py's own shard geometry -- and 64 x 8 (33.5 M samples per call
    either way; the spectrum's frame chains run 4 and 8 long).  Oracle on three whole streams; for all streams, call-splitting
    invariance (one F-frame call == F 1-frame calls: bit-exact, both carry states are exact) and a bin-centred tone reading its
    level at its bin in every frame."""
    import pebblesdr_amd as P
    fs, N = 2.0e6, 65536
    t = np.arange(F * N) / fs
    x = np.empty((S, F * N), dtype=np.complex64)
    kbin = [1000 + 37 * c for c in range(S)]
    for c in range(S):
        x[c] = (10 ** (-10 / 20) * np.exp(2j * np.pi * (fs * kbin[c] / N) * t) + lcg_noise(F * N, 500 + c, 1e-4)).astype(np.complex64)
    bands = [(-50e3 - 1e3 * c, 120e3 + 500.0 * c) for c in range(S)]  # every stream's tone is in band (fp32 floor otherwise)
    a = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=F)
    b = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=1)
    for c in range(S):
        a.set_bandpass(c, *bands[c])
        b.set_bandpass(c, *bands[c])
    YA, SA = a.process(x)
    parts = [b.process(x[:, f * N:(f + 1) * N]) for f in range(F)]
    assert np.array_equal(YA, np.concatenate([p[0] for p in parts], axis=1))
    assert np.array_equal(SA, np.concatenate([p[1] for p in parts], axis=1))
    for c in range(S):
        assert np.all(np.argmax(SA[c, 1:], axis=1) == N // 2 + kbin[c])
        assert np.abs(SA[c, 1:].max(axis=1) + 10.0).max() < 2e-3
    for c in (0, 17, S - 1):
        f_ref, s_ref = _streambank_refs(oracle_mod, fs, [bands[c]], N)[0]
        assert rel_rms(YA[c], f_ref.process(x[c])) <= TOL
        for f in range(F):
            r = s_ref.process(x[c, f * N:(f + 1) * N])
            if f:
                assert db_err(SA[c, f], r) <= TOL_DB


def test_config5_error_paths(gpu_lib):
    import pebblesdr_amd as P
    sb = P.StreamBank(2.0e6, 2, frame=65536, spectrum_bins=65536, max_frames=1)
    with pytest.raises(P.PebbleGpuError) as e:
        sb.set_bandpass(0, 3000, 300)
    assert e.value.code == -4
    with pytest.raises(P.PebbleGpuError) as e:
        sb.set_bandpass(2, -1000, 1000)
    assert e.value.code == -1
    buf = P.DeviceBuffer(8 * 2 * 65536)
    with pytest.raises(P.PebbleGpuError) as e:
        sb.process_device(buf.ptr, 1000)
    assert e.value.code == -5
    with pytest.raises(P.PebbleGpuError) as e:
        sb.process_device(buf.ptr, 2 * 65536)  # above max_frames
    assert e.value.code == -5
    with pytest.raises(P.PebbleGpuError) as e:
        P.StreamBank(2.0e6, 2, frame=65536, spectrum_bins=32768)
    assert e.value.code == -6


# ------------------------------------------------------------------------------------------------
# AGC on the narrow branch, fractional resampler after the demodulator
# ------------------------------------------------------------------------------------------------
def test_audio_tail_usb_agc_and_resampler(gpu_lib, oracle_mod):
    """Two USB channels through AGC (MED / knee 30 on one, manual gain 30 -> +6 dB on the other) and the 28-tap sinc
    resampler to 11025 Hz, over three calls of 1, 2 and 2 super-frames against the oracle run frame by frame: the
    output COUNT must match exactly (it comes from the reference's running fp64 time sum) and the samples to 1e-5."""
    import pebblesdr_amd as P
    fs, n, C = 2048000, 2048, 2
    ref = [oracle_mod.Receiver(fs, n, 0) for _ in range(C)]
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2, audio_rate=11025)
    fcs = [-400e3, 300e3]
    for c in range(C):
        ref[c].set_mode(oracle_mod.USB); ref[c].set_mixer(fcs[c]); ref[c].set_filter(300, 3000); ref[c].set_audio_rate(11025)
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000)
    ref[0].set_agc(2, 30); rx.set_agc(0, 2, 30)
    ref[1].set_agc(0, 30); rx.set_agc(1, 0, 30)
    sf = rx.superframe
    t = np.arange(5 * sf) / fs
    env = 0.02 + 0.3 * (np.sin(2 * np.pi * 2.5 * t) > 0)  # level steps exercise attack, decay and the peak-window rescan
    x = env * (np.exp(2j * np.pi * (fcs[0] + 1000.0) * t) + np.exp(2j * np.pi * (fcs[1] + 1700.0) * t)) + lcg_noise(5 * sf, 3, 1e-4)
    g = np.concatenate([rx.process(x[lo:hi])[0] for lo, hi in ((0, sf), (sf, 3 * sf), (3 * sf, 5 * sf))], axis=1)
    for c in range(C):
        r = np.concatenate([ref[c].process(x[f * n:(f + 1) * n])[0] for f in range(5 * sf // n)])
        assert g.shape[1] == len(r)
        assert rel_rms(g[c], r) <= TOL


def test_audio_tail_wfm_resampled(gpu_lib, oracle_mod):
    """WFM mono resampled to 48 kHz (rate 64000/48000: 1536..1537 outputs per 2048-sample frame), two calls."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    ref = oracle_mod.Receiver(fs, n, 0); ref.set_mode(oracle_mod.FMM); ref.set_mixer(200e3); ref.set_audio_rate(48000)
    rx = P.ReceiverBank(fs, 1, True, True, 0, max_superframes=3, audio_rate=48000)
    rx.set_mixer(0, 200e3)
    sf = rx.superframe
    t = np.arange(4 * sf) / fs
    x = 0.5 * np.exp(1j * (2 * np.pi * 200e3 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(4 * sf, 2, 1e-3)
    g = np.concatenate([rx.process(x[:3 * sf])[0], rx.process(x[3 * sf:])[0]], axis=1)
    r = np.concatenate([ref.process(x[f * n:(f + 1) * n])[0] for f in range(4 * sf // n)])
    assert g.shape[1] == len(r)
    assert rel_rms(g[0], r) <= TOL


def test_audio_tail_call_split_invariance_and_host_frames(gpu_lib, oracle_mod):
    """(a) one 4-super-frame call equals four 1-super-frame calls: identical output counts and sample positions (the
    resampler's time sum is replayed per frame, as the reference runs it); (b) the host frame path returns the
    resampled frame counts of the oracle."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    a = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=4, audio_rate=11025)
    b = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=1, audio_rate=11025)
    ref = oracle_mod.Receiver(fs, n, 0); ref.set_mode(oracle_mod.USB); ref.set_mixer(100e3); ref.set_filter(300, 3000); ref.set_audio_rate(11025)
    for rx in (a, b):
        rx.set_mode(0, P.DM_USB); rx.set_mixer(0, 100e3); rx.set_bandpass(0, 300, 3000)
    sf = a.superframe
    t = np.arange(4 * sf) / fs
    x = (0.3 * (1 + 0.5 * np.sin(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * 101e3 * t)).astype(np.complex64)
    A = a.process(x)[0]
    B = np.concatenate([b.process(x[i * sf:(i + 1) * sf])[0] for i in range(4)], axis=1)
    # same counts; values to the oscillator's phase rounding (phase0 is re-based per call), not bit for bit
    assert A.shape == B.shape and np.abs(A - B).max() <= 1e-6
    h = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=1, audio_rate=11025)
    h.set_mode(0, P.DM_USB); h.set_mixer(0, 100e3); h.set_bandpass(0, 300, 3000)
    got, want = [], []
    for f in range(4 * sf // n):
        au, _ = h.process_iq(x[f * n:(f + 1) * n].astype(np.complex128))
        ra, _ = ref.process(x[f * n:(f + 1) * n].astype(np.complex128), want_spectrum=False)
        assert len(au) == len(ra)
        got.append(au); want.append(ra)
    assert rel_rms(np.concatenate(got), np.concatenate(want)) <= TOL


def test_signal_strength_per_frame(gpu_lib, oracle_mod):
    """S-meter (SignalStrength::fdEstimate) for two USB channels over a shared stream and for a WFM bank: (a) against the
    oracle's fdEstimate applied to the oracle's OWN spectrum of each frame (end to end: <= 0.1 dB, from frame 1 on);
    (b) against fdEstimate applied to the device spectrum (the reduction alone: ~1e-5 dB)."""
    import pebblesdr_amd as P
    fs, n, C, bins = 2048000, 2048, 2, 4096
    fcs = [100e3, -300e3]
    rx = P.ReceiverBank(fs, C, True, False, bins, max_superframes=1)
    for c in range(C):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000)
    rx.enable_signal_strength(True)
    sf = rx.superframe
    x = tones(fs, sf, [(0.05, fcs[0] + 1000.0), (0.01, fcs[1] + 2000.0)]) + lcg_noise(sf, 3, 1e-3)
    _, sp = rx.process(x)
    sm = rx.signal_strength()
    assert sm.shape == (C, sf // n, 4)
    ref = oracle_mod.Receiver(fs, n, bins)
    for f in range(sf // n):
        _, rs = ref.process(x[f * n:(f + 1) * n])
        for c in range(C):
            own = oracle_mod.fd_estimate(sp[0, f].astype(np.float64), fs, np.float32(300), np.float32(3000), fcs[c])
            assert np.abs(sm[c, f] - own).max() <= 1e-4
            if f:
                assert np.abs(sm[c, f] - oracle_mod.fd_estimate(rs, fs, np.float32(300), np.float32(3000), fcs[c])).max() <= TOL_DB
    w = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=1)
    w.set_mixer(0, 200e3)
    w.enable_signal_strength(True)
    t = np.arange(w.superframe) / fs
    xw = 0.5 * np.exp(1j * (2 * np.pi * 200e3 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(w.superframe, 2, 1e-3)
    _, spw = w.process(xw)
    smw = w.signal_strength()
    for f in (1, 7, w.superframe // n - 1):
        own = oracle_mod.fd_estimate(spw[0, f].astype(np.float64), fs, np.float32(-100000), np.float32(100000), 200e3)
        assert np.abs(smw[0, f] - own).max() <= 1e-4
    plain = P.ReceiverBank(fs, 1, True, False, 0)
    with pytest.raises(P.PebbleGpuError):
        plain.enable_signal_strength(True)  # no spectrum to measure on


def _gated_signal(fs, sf, fc, wfm, pattern, amp=0.1):
    """one super-frame per entry of `pattern`: carrier present (1) or only the noise floor (0)"""
    N = sf * len(pattern)
    t = np.arange(N) / fs
    env = np.repeat(np.asarray(pattern, dtype=np.float64), sf)
    if wfm:
        sig = amp * np.exp(1j * (2 * np.pi * fc * t + 5.0 * np.sin(2 * np.pi * 1000 * t)))
    else:
        sig = amp * (1 + 0.5 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * fc * t)
    return env * sig + lcg_noise(N, 9, 1e-5)


@pytest.mark.parametrize("wfm", [False, True])
def test_squelch_gate_is_the_reference_early_return(gpu_lib, oracle_mod, wfm):
    """Squelch (receiver.cpp:704-707, gate at :893-897 / :962-965): a super-frame whose avgDb is under the threshold ends
    after the band-pass -- no audio, and nothing behind the gate (AGC, demodulator, resampler) advances, so the audio after
    the gate reopens continues from the state the last open super-frame left.  One channel, one super-frame per call."""
    import pebblesdr_amd as P
    fs, n, bins, fc = 2048000, 2048, 4096, 100e3
    rx = P.ReceiverBank(fs, 1, True, wfm, bins, max_superframes=1, audio_rate=11025)
    ref = oracle_mod.Receiver(fs, n, bins)
    rx.set_mixer(0, fc); ref.set_mixer(fc)
    if wfm:
        ref.set_mode(oracle_mod.FMM)
    else:
        rx.set_mode(0, P.DM_AM); rx.set_bandpass(0, -5000, 5000); rx.set_agc(0, 1, 20)  # AGC_FAST
        ref.set_mode(oracle_mod.AM); ref.set_filter(-5000, 5000); ref.set_agc(1, 20)
    ref.set_audio_rate(11025)
    rx.set_squelch(0, -60.0); ref.set_squelch(-60.0)
    sf = rx.superframe
    pattern = [1, 1, 0, 0, 1, 0, 1]
    x = _gated_signal(fs, sf, fc, wfm, pattern)
    for k, on in enumerate(pattern):
        g = rx.process(x[k * sf:(k + 1) * sf])[0][0]
        r = np.concatenate([ref.process(x[k * sf + f * n:k * sf + (f + 1) * n], want_spectrum=False)[0] for f in range(sf // n)])
        assert len(g) == len(r), "super-frame %d" % k
        assert (len(g) > 0) == bool(on)
        if on:
            assert rel_rms(g, r) <= (TOL_AGC_STARTUP if not wfm else TOL), "super-frame %d" % k  # the narrow case runs AGC_FAST
    # -120 (DB::minDb) never gates: the silent super-frame is demodulated again
    rx.set_squelch(0, -120.0); ref.set_squelch(-120.0)
    g = rx.process(x[2 * sf:3 * sf])[0][0]
    assert len(g) > 0
    wbank = P.ReceiverBank(fs, 2, True, True, bins, max_superframes=1)
    with pytest.raises(P.PebbleGpuError):
        wbank.set_squelch(0, -60.0)  # a WFM receiver gates in the reference's own shape only (narrow banks: test_squelch_in_a_bank)


def test_squelch_on_the_single_frame_host_path(gpu_lib, oracle_mod):
    """CB_ProcessIQData shape with a squelch set: the gate reads the latest frame's spectrum whether or not the host asked
    for it, and a gated super-frame hands back zero audio samples."""
    import pebblesdr_amd as P
    fs, n, bins, fc = 2048000, 2048, 4096, -250e3
    rx = P.ReceiverBank(fs, 1, True, False, bins, max_superframes=1)
    ref = oracle_mod.Receiver(fs, n, bins)
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, fc); rx.set_bandpass(0, 300, 3000); rx.set_squelch(0, -70.0)
    ref.set_mode(oracle_mod.USB); ref.set_mixer(fc); ref.set_filter(300, 3000); ref.set_squelch(-70.0)
    sf = rx.superframe
    pattern = [1, 0, 1]
    N = sf * len(pattern)
    t = np.arange(N) / fs
    x = np.repeat(np.asarray(pattern, dtype=np.float64), sf) * 0.05 * np.exp(2j * np.pi * (fc + 1500.0) * t) + lcg_noise(N, 5, 1e-5)
    got, want = [], []
    for f in range(N // n):
        a, _ = rx.process_iq(x[f * n:(f + 1) * n], want_spectrum=False)
        r, _ = ref.process(x[f * n:(f + 1) * n], want_spectrum=False)
        assert len(a) == len(r), "frame %d" % f
        got.append(a); want.append(r)
    got, want = np.concatenate(got), np.concatenate(want)
    assert len(got) == 2 * 2048
    assert rel_rms(got, want) <= TOL


# ------------------------------------------------------------------------------------------------
# DCRemoval, IQBalance, NoiseBlanker 1/2 ahead of the spectrum and the mixer; NoiseFilter (ANF)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [1, 2, 4, 8, 15])
def test_input_conditioners(gpu_lib, oracle_mod, flags):
    """Each conditioner alone and all four together (reference order), on a stream with a DC offset and three spikes:
    audio and spectrum against the oracle chain over 3 super-frames in 2 calls (state carries across calls)."""
    import pebblesdr_amd as P
    fs, n, bins = 2048000, 2048, 4096
    ref = oracle_mod.Receiver(fs, n, bins); ref.set_mode(oracle_mod.USB); ref.set_mixer(100e3); ref.set_filter(300, 3000)
    ref.set_conditioners(flags, 1.02, 0.03)
    rx = P.ReceiverBank(fs, 1, True, False, bins, max_superframes=2)
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, 100e3); rx.set_bandpass(0, 300, 3000); rx.set_conditioners(0, flags, 1.02, 0.03)
    sf = rx.superframe
    x = tones(fs, 3 * sf, [(0.05, 101e3), (0.02, -250e3)]) + lcg_noise(3 * sf, 5, 1e-3) + 0.01
    x[5000] += 2.0; x[70000:70003] += 1.5j; x[150000] -= 3.0
    outs = [rx.process(x[lo:hi]) for lo, hi in ((0, sf), (sf, 3 * sf))]
    g = np.concatenate([o[0] for o in outs], axis=1)[0]
    gs = np.concatenate([o[1] for o in outs], axis=1)[0]
    want, ws = [], []
    for f in range(3 * sf // n):
        a, sp = ref.process(x[f * n:(f + 1) * n])
        want.append(a); ws.append(sp)
    assert rel_rms(g, np.concatenate(want)) <= TOL
    for f in range(1, len(ws)):
        assert db_err(gs[f], ws[f]) <= TOL_DB
    with pytest.raises(P.PebbleGpuError) as e:
        rx.process_iq(x[:n].astype(np.complex128))  # the conditioners are on the batched path only
    assert e.value.code == -6


def test_noise_filter_anf(gpu_lib, oracle_mod):
    """The ANF kernel against the oracle's ANF on IDENTICAL input (the device's own band-pass output, from a second
    bank): <= 1e-6.  In the chain the algorithm is ill-conditioned -- its input is band-limited to 4 % of the band, and
    a 1e-8 white perturbation of it moves the reference's own output by 1e-4 (test_oracle_pins) -- so against the oracle
    CHAIN, whose band-pass output differs by ~1e-7, the bar is 5e-3 with the first 300 samples (before the adaptation
    has wandered) at 1e-5."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048

    def bank(anf):
        b = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=2)
        b.set_mode(0, P.DM_USB); b.set_mixer(0, 100e3); b.set_bandpass(0, 300, 3000)
        if anf:
            b.set_noise_filter(0, True)
        return b
    a, b = bank(True), bank(False)
    sf = a.superframe
    x = tones(fs, 3 * sf, [(0.05, 101e3), (0.03, 102.2e3)]) + lcg_noise(3 * sf, 5, 1e-2)
    ga = np.concatenate([a.process(x[:sf])[0], a.process(x[sf:])[0]], axis=1)[0]
    gb = np.concatenate([b.process(x[:sf])[0], b.process(x[sf:])[0]], axis=1)[0]
    same_input = oracle_mod.Anf().process(gb.astype(np.complex128))
    assert rel_rms(ga, same_input) <= 1e-6
    ref = oracle_mod.Receiver(fs, n, 0); ref.set_mode(oracle_mod.USB); ref.set_mixer(100e3); ref.set_filter(300, 3000); ref.set_anf(True)
    r = np.concatenate([ref.process(x[f * n:(f + 1) * n], want_spectrum=False)[0] for f in range(3 * sf // n)])
    assert rel_rms(ga, r) <= 5e-3
    assert np.abs(ga[:300] - r[:300]).max() <= 1e-5 * np.abs(r).max()
    w = P.ReceiverBank(fs, 1, True, True, 0)
    with pytest.raises(P.PebbleGpuError):
        w.set_noise_filter(0, True)


def test_error_paths(gpu_lib):
    import pebblesdr_amd as P
    rx = P.ReceiverBank(2048000, 2, True, False, 0)
    with pytest.raises(P.PebbleGpuError) as e:
        rx.set_mixer(5, 1.0)
    assert e.value.code == -1
    with pytest.raises(P.PebbleGpuError) as e:
        rx.set_bandpass(0, 3000, 300)  # lo >= hi: "Filter Parameter error"
    assert e.value.code == -4
    with pytest.raises(P.PebbleGpuError) as e:
        rx.set_mode(0, P.DM_FMS)  # FMM / FMS need a WFM bank
    assert e.value.code == -6
    buf = P.DeviceBuffer(8 * 1000)
    with pytest.raises(P.PebbleGpuError) as e:
        rx.process_device(buf.ptr, 1000)  # not a whole super-frame
    assert e.value.code == -5
    w = P.ReceiverBank(2048000, 1, True, True, 0)
    with pytest.raises(P.PebbleGpuError) as e:
        w.set_agc(0, 2, 30)  # the WFM branch has no AGC step
    assert e.value.code == -6
    with pytest.raises(P.PebbleGpuError) as e:
        rx.set_agc(0, 9, 30)
    assert e.value.code == -1
    with pytest.raises(P.PebbleGpuError):
        P.ReceiverBank(2048000, 1, True, False, 1 << 16)  # 65536 bins clamps to 65535: not a power of two (fft.cpp:76-77)


# ------------------------------------------------------------------------------------------------
# size-independent properties at BASELINE sizes (no oracle: it would take minutes)
# ------------------------------------------------------------------------------------------------
def test_full_size_properties_config2(gpu_lib):
    """Properties that need no oracle, on an 8 Mi-sample call of the bench workload: (a) call-splitting invariance:
    one 64-super-frame call (4 frames per wave group) equals sixty-four 1-super-frame calls, bit for bit in the spectrum and to ~1e-6 in audio
    (the long call runs the chunk-parallel warm-up scans, the short ones the exact carried state);
    (b) a bin-centred -10 dBFS tone reads -10.00 dB at the right bin in every frame; (c) the audio of an unmodulated
    carrier is ~0 after the start-up transient."""
    import pebblesdr_amd as P
    fs, n = 20_000_000, 2048
    k = 64
    a_rx = P.ReceiverBank(fs, 1, True, True, 8192, max_superframes=k)
    b_rx = P.ReceiverBank(fs, 1, True, True, 8192, max_superframes=1)
    sf = a_rx.superframe
    N = k * sf
    fbin = fs * 205 / 2048  # bin-centred for the 2048-sample window
    t = np.arange(N) / fs
    x = (10 ** (-10 / 20) * np.exp(2j * np.pi * fbin * t)).astype(np.complex64)
    for rx in (a_rx, b_rx):
        rx.set_mixer(0, fbin)
    A, SA = a_rx.process(x)
    parts = [b_rx.process(x[i * sf:(i + 1) * sf]) for i in range(k)]
    B = np.concatenate([p[0] for p in parts], axis=1)
    SB = np.concatenate([p[1] for p in parts], axis=1)
    assert np.array_equal(SA, SB)
    assert np.abs(A - B).max() <= 1e-6
    peaks = SA[0][1:].max(axis=1)
    assert np.abs(peaks + 10.0).max() < 2e-3
    assert np.all(np.argmax(SA[0][1:], axis=1) == 4096 + 4 * 205)
    # unmodulated carrier at DC after mixing: discriminator output 0 (after the start-up transient)
    assert np.abs(A[0][4096:]).max() < 1e-4


def test_full_size_configs2_256_ssb_channels(gpu_lib, oracle_mod):
    """BASELINE configs[2] at size: one 2.048 Msps stream, 256 tuned USB channels (f_c = -960 kHz + 7.5 kHz c), a tone
    1000 + 3.1 c Hz above every carrier, two super-frames in one call.  Oracle on three channels; for all 256: the tone
    comes out at its own offset with the level the chain predicts (0.003 x the 10^(2*5/20) gain restore)."""
    import pebblesdr_amd as P
    fs, n, C = 2048000, 2048, 256
    fcs = [-960e3 + 7.5e3 * c for c in range(C)]
    rng = np.random.RandomState(3)
    ph = rng.uniform(0, 2 * np.pi, C)
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    for c, fc in enumerate(fcs):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fc); rx.set_bandpass(c, 300, 3000)
    sf = rx.superframe
    x = tones(fs, 2 * sf, [(0.003, fcs[c] + 1000.0 + 3.1 * c, ph[c]) for c in range(C)]) + lcg_noise(2 * sf, 3, 1e-4)
    g = rx.process(x)[0]
    assert g.shape == (C, 2 * sf // rx.D)
    rate = fs / rx.D
    w = np.hanning(2048)
    for c in range(C):
        sp = np.abs(np.fft.fft(g[c][2048:] * w))
        k = int(np.argmax(sp))
        f = k * rate / 2048
        assert abs(f - (1000.0 + 3.1 * c)) <= rate / 2048  # within a bin
        amp = sp[k - 2:k + 3].max() / (w.sum())
        assert abs(amp / (0.003 * 10 ** (2 * 5 / 20.0)) - 1.0) < 0.2  # scalloping of a Hann bin: within 20 %
    for c in (0, 100, 255):
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.USB); r.set_mixer(fcs[c]); r.set_filter(300, 3000)
        want = np.concatenate([r.process(x[f * n:(f + 1) * n], want_spectrum=False)[0] for f in range(2 * sf // n)])
        assert rel_rms(g[c], want) <= TOL


@pytest.mark.parametrize("k", [8, 32])
def test_bench_geometry_configs2_superframes_in_one_call(gpu_lib, oracle_mod, k):
    """BASELINE configs[2] at the bench's own call geometry: 256 USB channels off one 2.048 Msps stream, 8 super-frames in one
    call (bench.py's configs[2] step: one wave per SIMD, chunks of 64 outputs) and 32 (the batch sweep: two waves per SIMD,
    chunks of 128), the bench's tuning plan.  Two such calls, so the second starts from the running sums, the first-stage
    history and the raw tail the first one left (the first call of a stream sits in the oscillators' transient and takes the
    two-kernel route).  Oracle on four channels over the whole stream; every frame of the last call is compared."""
    import pebblesdr_amd as P
    fs, n, C = 2048000, 2048, 256
    fcs = [(c - C / 2.0) * (0.8 * fs / C) for c in range(C)]
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=k)
    for c, fc in enumerate(fcs):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fc); rx.set_bandpass(c, 300, 3000)
    sf = rx.superframe
    check = (0, 37, 129, 255)
    N = (1 + 2 * k) * sf
    x = tones(fs, N, [(0.004, fcs[c] + 900.0 + 7.0 * c, 0.3 * c) for c in check] + [(0.002, fcs[c] + 1500.0, 0.1 * c) for c in range(3, C, 17)]) + lcg_noise(N, 5, 1e-3)
    g = [rx.process(x[:sf])[0]]
    names = [rx.kernel_name(2)]
    for i in range(2):
        g.append(rx.process(x[sf + i * k * sf:sf + (i + 1) * k * sf])[0])
        names.append(rx.kernel_name(2))
    assert names[1] in ("k_mix_dec_mfma", "k_mix_dec_fused") and names[2] == names[1]
    g = np.concatenate(g, axis=1)
    for c in check:
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.USB); r.set_mixer(fcs[c]); r.set_filter(300, 3000)
        want = np.concatenate([r.process(x[f * n:(f + 1) * n], want_spectrum=False)[0] for f in range(N // n)])
        assert want.shape == g[c].shape
        for f in range(g[c].shape[0] // 2048):
            assert rel_rms(g[c][f * 2048:(f + 1) * 2048], want[f * 2048:(f + 1) * 2048]) <= TOL, (c, f)


def test_full_size_configs3_512_channel_shard(gpu_lib, oracle_mod):
    """BASELINE configs[3], one GPU's shard at size: a 100 Msps stream, 512 AM/USB channels, one super-frame (4.2 M input
    samples, D = 2048).  Sixteen channels carry a signal; oracle (mixer + decimator + band-pass [+ AM]) on three of them,
    and every signalled channel shows its modulation at the right place."""
    import pebblesdr_amd as P
    fs, C = 100_000_000, 512
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=1)
    assert rx.D == 2048
    sf = rx.superframe
    rate = int(rx.info.demod_rate_int)
    fcs = [-44.8e6 + 175e3 * c for c in range(C)]
    lit = list(range(5, C, 32))  # 16 channels
    t = np.arange(sf) / fs
    x = lcg_noise(sf, 4, 1e-3)
    for c in lit:
        if c % 2 == 0:
            x = x + 0.05 * (1 + 0.5 * np.cos(2 * np.pi * 800 * t)) * np.exp(2j * np.pi * fcs[c] * t)
        else:
            x = x + 0.05 * np.exp(2j * np.pi * (fcs[c] + 1200.0) * t)
    for c in range(C):
        rx.set_mixer(c, fcs[c])
        if c % 2 == 0:
            rx.set_mode(c, P.DM_AM); rx.set_bandpass(c, -5000, 5000)
        else:
            rx.set_mode(c, P.DM_USB); rx.set_bandpass(c, 300, 3000)
    g = rx.process(x)[0]
    assert g.shape == (C, 2048)
    w = np.hanning(1024)
    for c in lit:
        sp = np.abs(np.fft.fft(g[c][1024:] * w))
        k = int(np.argmax(sp[1:512])) + 1
        assert abs(k * rate / 1024 - (800.0 if c % 2 == 0 else 1200.0)) <= rate / 1024
    for c in (lit[0], lit[7], lit[15]):
        mix = oracle_mod.Mixer(fs); mix.set_frequency(fcs[c])
        dec = oracle_mod.Decimator(fs, 30000)
        z = dec.process(mix.process(x)) * 10 ** (2 * 11 / 20.0)
        ff = oracle_mod.FastFIR()
        if c % 2 == 0:
            ff.setup(-5000, 5000, 0, rate)
            want = oracle_mod.DemodAM(rate, 10000).process(ff.process(z))
        else:
            ff.setup(300, 3000, 0, rate)
            want = ff.process(z)
        assert rel_rms(g[c], want) <= TOL


def test_configs3_shard_over_three_calls(gpu_lib, oracle_mod):
    """BASELINE configs[3], one GPU's shard (100 Msps, 512 AM / USB channels, chain cic3 x 16, hb11 x 16, hb15, hb23, hb47) over three calls
    of one super-frame: the first inside the oscillators' transient (k_mix_cic_hb + k_cascade), the second and third in one kernel
    (k_mix_dec_mfma with the CIC3 and the hb11 as one twelve-pair first stage), the second from the histories the first left, the third
    from the second's running sums.  Oracle (mixer + decimator + band-pass [+ AM]) on four channels, every frame."""
    import pebblesdr_amd as P
    fs, C, K = 100_000_000, 512, 3
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=1)
    sf = rx.superframe
    rate = int(rx.info.demod_rate_int)
    fcs = [-44.8e6 + 175e3 * c for c in range(C)]
    lit = (0, 130, 333, 511)
    t = np.arange(K * sf) / fs
    x = lcg_noise(K * sf, 4, 1e-3)
    for c in lit:
        if c % 2 == 0:
            x = x + 0.05 * (1 + 0.5 * np.cos(2 * np.pi * 800 * t)) * np.exp(2j * np.pi * fcs[c] * t)
        else:
            x = x + 0.05 * np.exp(2j * np.pi * (fcs[c] + 1200.0) * t)
    del t
    for c in range(C):
        rx.set_mixer(c, fcs[c])
        if c % 2 == 0:
            rx.set_mode(c, P.DM_AM); rx.set_bandpass(c, -5000, 5000)
        else:
            rx.set_mode(c, P.DM_USB); rx.set_bandpass(c, 300, 3000)
    g, names = [], []
    for k in range(K):
        g.append(rx.process(x[k * sf:(k + 1) * sf])[0])
        names.append(rx.kernel_name(2))
    g = np.concatenate(g, axis=1)
    assert names[0] == "k_mix_cic_hb" and names[1] == "k_mix_dec_mfma" and names[2] == "k_mix_dec_mfma", names
    for c in lit:
        mix = oracle_mod.Mixer(fs); mix.set_frequency(fcs[c])
        dec = oracle_mod.Decimator(fs, 30000)
        z = np.concatenate([dec.process(mix.process(x[k * sf:(k + 1) * sf])) for k in range(K)]) * 10 ** (2 * 11 / 20.0)
        ff = oracle_mod.FastFIR()
        if c % 2 == 0:
            ff.setup(-5000, 5000, 0, rate)
            am = oracle_mod.DemodAM(rate, 10000)
            want = np.concatenate([am.process(ff.process(z[k:k + 2048])) for k in range(0, len(z), 2048)])
        else:
            ff.setup(300, 3000, 0, rate)
            want = np.concatenate([ff.process(z[k:k + 2048]) for k in range(0, len(z), 2048)])
        for k in range(K):
            assert rel_rms(g[c][k * 2048:(k + 1) * 2048], want[k * 2048:(k + 1) * 2048]) <= TOL, (c, k)


@pytest.mark.parametrize("fs,C", [(1024000, 3), (2400000, 17), (3200000, 1), (5000000, 17), (8000000, 3), (10000000, 1), (10000000, 17),
                                  (16000000, 3), (25000000, 17), (40000000, 1), (40000000, 3)])
def test_chain_sweep_over_rates_and_bank_sizes(gpu_lib, oracle_mod, fs, C):
    """First-stage forms the ladder of decimator.cpp:74-146 produces between 1 and 40 Msps -- hb11 merged 2/4/8/16 times
    (LDS-tiled for few channels, in registers for a bank, the stride-16 one peeled off the cascade) and CIC3 merged 1/2/3 times
    in front of hb11 x 16 (the fused register front end) -- on the routes one channel and a few channels take, and a one-group
    bank on some of them (the banks' own kernel, every instance and stride of it: tests/test_bank_decimator_gpu.py): USB
    audio of the first and last channel against Mixer -> Decimator -> gain restore -> FastFIR restated by the oracle, three
    calls.  The oracle is fed whole super-frames so that none of its stages sees fewer samples than taps.  The banks of 17 here sit
    on halfband triples that k_mix_dec_mfma has an instance for; a bank on another triple ((15,23,59) at 1.4 and 2.8 Msps, (15,19,31)
    behind a CIC3 at 16 Msps, ...) or behind hb11 x 32 stays on the general route in steady state too: tests/decim_cases.py."""
    import pebblesdr_amd as P
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=1)
    chain = rx.chain()
    rate = int(rx.info.demod_rate_int)
    stages = sum(int(np.log2(st)) for _, st in chain)
    fcs = [(-0.4 + 0.8 * (c + 0.5) / C) * fs for c in range(C)]
    for c in range(C):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000)
    sf = rx.superframe
    K = 3  # calls: the first inside the oscillators' transient, the second from the histories it left, the third from the running sums of the second
    x = tones(fs, K * sf, [(0.05, fc + 1000.0 + 50.0 * i) for i, fc in enumerate(fcs)]) + lcg_noise(K * sf, 5, 1e-3)
    g, names = [], []
    for k in range(K):
        g.append(rx.process(x[k * sf:(k + 1) * sf])[0])
        names.append(rx.kernel_name(2))
    g = np.concatenate(g, axis=1)
    if C >= 16:
        # the banks of >= 16 channels of this table ([cic3 x S0,] hb11 x S + a halfband triple with a matrix instance) run their whole
        # decimator in one kernel once the oscillators have settled
        assert names[1] == "k_mix_dec_mfma" and names[2] == "k_mix_dec_mfma", (names, chain)
    for c in sorted({0, C - 1}):
        mix = oracle_mod.Mixer(fs); mix.set_frequency(fcs[c])
        dec = oracle_mod.Decimator(fs, 30000)
        assert dec.chain() == chain
        z = np.concatenate([dec.process(mix.process(x[k * sf:(k + 1) * sf])) for k in range(K)]) * 10 ** (2 * stages / 20.0)
        ff = oracle_mod.FastFIR(); ff.setup(300, 3000, 0, rate)
        r = np.concatenate([ff.process(z[k:k + 2048]) for k in range(0, len(z), 2048)])
        assert r.shape == g[c].shape
        for k in range(K):
            assert rel_rms(g[c][k * 2048:(k + 1) * 2048], r[k * 2048:(k + 1) * 2048]) <= TOL, "channel %d call %d chain %s" % (c, k, chain)


@pytest.mark.parametrize("fs", [2400000, 5000000, 25000000])
@pytest.mark.parametrize("mode", ["AM", "NFM", "CWU"])
def test_demod_modes_at_the_other_demod_rates(gpu_lib, oracle_mod, fs, mode):
    """The narrow demodulators away from 64 kHz: 37 500, 39 062 and 48 828 Hz (the integer-truncated rates of receiver.h:165)
    behind three different chains.  Oracle: Mixer -> Decimator -> gain restore -> FastFIR -> demodulator on whole
    super-frames.  NFM is compared once its PLL has acquired (see the NFM note in DESIGN.md section 3)."""
    import pebblesdr_amd as P
    rx = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=1)
    rate = int(rx.info.demod_rate_int)
    stages = sum(int(np.log2(st)) for _, st in rx.chain())
    fc = 0.17 * fs
    lo, hi = {"AM": (-5000, 5000), "NFM": (-4000, 4000), "CWU": (-1000, -500)}[mode]
    rx.set_mode(0, {"AM": P.DM_AM, "NFM": P.DM_FMN, "CWU": P.DM_CWU}[mode]); rx.set_mixer(0, fc); rx.set_bandpass(0, lo, hi)
    sf = rx.superframe
    t = np.arange(3 * sf) / fs
    if mode == "AM":
        x = 0.1 * (1 + 0.5 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * fc * t)
    elif mode == "NFM":
        x = 0.1 * np.exp(1j * (2 * np.pi * fc * t + 2.0 * np.sin(2 * np.pi * 800 * t)))
    else:
        x = 0.1 * np.exp(2j * np.pi * (fc + (lo + hi) / 2) * t)
    x = x + lcg_noise(3 * sf, 5, 1e-4)
    g = np.concatenate([rx.process(x[k * sf:(k + 1) * sf])[0] for k in range(3)], axis=1)[0]
    mix = oracle_mod.Mixer(fs); mix.set_frequency(fc)
    dec = oracle_mod.Decimator(fs, 30000)
    z = np.concatenate([dec.process(mix.process(x[k * sf:(k + 1) * sf])) for k in range(3)]) * 10 ** (2 * stages / 20.0)
    ff = oracle_mod.FastFIR(); ff.setup(lo, hi, 0, rate)
    dm = oracle_mod.DemodAM(rate, hi - lo) if mode == "AM" else oracle_mod.DemodNFM(rate) if mode == "NFM" else None
    r = np.concatenate([(dm.process(y) if dm else y) for y in (ff.process(z[k:k + 2048]) for k in range(0, len(z), 2048))])
    assert r.shape == g.shape
    for k in range(1 if mode == "NFM" else 0, 3):
        # NFM: measured 2e-6 .. 5e-6 in frame 1 and 2e-7 .. 4e-7 from frame 2 on at every rate (tools/diag/pll_err.py): the plain bar
        assert rel_rms(g[k * 2048:(k + 1) * 2048], r[k * 2048:(k + 1) * 2048]) <= TOL, "frame %d" % k


@pytest.mark.parametrize("C", [16, 37, 100])
def test_register_first_stage_bank_sizes_and_retune(gpu_lib, oracle_mod, C):
    """k_mix_hb11_bank (lanes = channels off one shared stream): channel counts that fill a wave, leave one ragged and span
    two channel groups; three calls so the mixed-sample history and the oscillator's amplitude transient (first call only)
    are both crossed, with one channel retuned between calls (Mixer::setFrequency resets the oscillator)."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=1)
    assert rx.chain()[0] == (11, 4)
    fcs = [-950e3 + (1900e3 / C) * c for c in range(C)]
    for c in range(C):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000)
    sf = rx.superframe
    check = sorted({0, 1, C // 2, C - 2, C - 1})
    refs = {}
    for c in check:
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.USB); r.set_mixer(fcs[c]); r.set_filter(300, 3000)
        refs[c] = r
    x = tones(fs, 3 * sf, [(0.02, fcs[c] + 900.0 + 11.0 * c) for c in check] + [(0.02, 123456.0 + 1500.0)]) + lcg_noise(3 * sf, 11, 1e-3)
    for k in range(3):
        if k == 2:  # retune the middle channel onto the extra tone
            rx.set_mixer(C // 2, 123456.0); refs[C // 2].set_mixer(123456.0)
        g = rx.process(x[k * sf:(k + 1) * sf])[0]
        for c in check:
            r = np.concatenate([refs[c].process(x[k * sf + f * n:k * sf + (f + 1) * n], want_spectrum=False)[0] for f in range(sf // n)])
            assert g[c].shape == r.shape
            assert rel_rms(g[c], r) <= TOL, "call %d channel %d" % (k, c)


@pytest.mark.parametrize("fs,wfm", [(2048000, False), (20000000, True), (20000000, False)])
def test_two_stream_call_equals_single_stream_call(gpu_lib, oracle_mod, fs, wfm):
    """A one-channel call with a spectrum forks the chain onto a second stream (register first stage: hb11 at 2.048 Msps and
    20 Msps WFM, CIC3 + hb11 at 20 Msps narrow); per-kernel profiling keeps the whole call on one stream with the LDS-tiled
    first stage.  Both must give the oracle's audio and spectrum, call after call."""
    import pebblesdr_amd as P
    n, bins = 2048, 4096
    fc = 0.11 * fs
    a = P.ReceiverBank(fs, 1, True, wfm, bins, max_superframes=2)
    b = P.ReceiverBank(fs, 1, True, wfm, bins, max_superframes=2)
    b.set_profiling(True)
    ref = oracle_mod.Receiver(fs, n, bins)
    for rx in (a, b):
        rx.set_mixer(0, fc)
        if not wfm:
            rx.set_mode(0, P.DM_AM); rx.set_bandpass(0, -5000, 5000)
    ref.set_mixer(fc)
    if wfm:
        ref.set_mode(oracle_mod.FMM)
    else:
        ref.set_mode(oracle_mod.AM); ref.set_filter(-5000, 5000)
    sf = a.superframe
    # At D = 512 a 2048-sample reference frame feeds the late stages fewer samples than taps and the reference degrades to
    # sample dropping (decimator.cpp:602-625; see test_config4_... for the frame size that avoids it): there the two paths
    # are compared with each other only.
    with_oracle = sf <= 200000
    calls = [1, 2, 1] if with_oracle else [1, 1]
    N = sum(calls) * sf
    t = np.arange(N) / fs
    if wfm:
        x = 0.3 * np.exp(1j * (2 * np.pi * fc * t + 20.0 * np.sin(2 * np.pi * 1000 * t)))
    else:
        x = 0.1 * (1 + 0.5 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * fc * t)
    x = x + lcg_noise(N, 13, 1e-3)
    off = 0
    for k in calls:
        seg = x[off:off + k * sf]
        ga, sa = a.process(seg)
        gb, sb = b.process(seg)
        assert ga[0].shape == gb[0].shape == (k * 2048,)
        assert np.sqrt(np.mean(np.abs(gb[0]) ** 2)) > 1e-3
        assert rel_rms(ga[0], gb[0]) <= 2e-6
        assert np.abs(sa - sb).max() <= 1e-3
        if with_oracle:
            ra, rs = [], []
            for f in range(len(seg) // n):
                au, sp = ref.process(seg[f * n:(f + 1) * n])
                ra.append(au); rs.append(sp)
            ra = np.concatenate(ra)
            assert ga[0].shape == ra.shape
            assert rel_rms(ga[0], ra) <= TOL and rel_rms(gb[0], ra) <= TOL
            first = 1 if off == 0 else 0  # frame 0 of a stream is undefined in the reference (uninitialised previous frame)
            for f in range(first, len(rs), max(1, len(rs) // 7)):
                assert db_err(sa[0, f], rs[f]) <= TOL_DB and db_err(sb[0, f], rs[f]) <= TOL_DB
        off += k * sf


def test_lifecycle_and_back_to_back_calls(gpu_lib, oracle_mod):
    """Create/destroy many banks (no leak large enough to fail an allocation), then 40 calls queued back to back without
    a host sync, with retunes, band changes and mode changes in between; the last super-frames must still match the
    oracle that saw the same sequence."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    live = P.binding.live_bytes()
    for _ in range(30):
        b = P.ReceiverBank(fs, 4, True, False, 4096, max_superframes=4, audio_rate=11025)
        b.close()
    assert P.binding.live_bytes() == live  # what the library holds, to the byte (pebblegpu_live_bytes)
    rx = P.ReceiverBank(fs, 1, True, False, 4096, max_superframes=1)
    ref = oracle_mod.Receiver(fs, n, 4096)
    sf = rx.superframe
    calls = 40
    x = tones(fs, calls * sf, [(0.05, 101e3), (0.04, -199e3), (0.03, 50e3)]) + lcg_noise(calls * sf, 9, 1e-3)  # each setting has a tone in band
    buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x))
    plan = {0: ("mix", 100e3), 1: ("band", (300, 3000)), 2: ("mode", "USB"), 11: ("mix", -200e3), 12: ("mode", "AM"), 13: ("band", (-4000, 4000)),
            25: ("mix", 51e3), 26: ("mode", "LSB"), 27: ("band", (-3000, -300))}
    modes = {"USB": (P.DM_USB, oracle_mod.USB), "AM": (P.DM_AM, oracle_mod.AM), "LSB": (P.DM_LSB, oracle_mod.LSB)}
    want = None
    for k in range(calls):
        if k in plan:
            what, arg = plan[k]
            if what == "mix":
                rx.set_mixer(0, arg); ref.set_mixer(arg)
            elif what == "band":
                rx.set_bandpass(0, *arg); ref.set_filter(*arg)
            else:
                rx.set_mode(0, modes[arg][0]); ref.set_mode(modes[arg][1])
        rx.process_device(buf.ptr + 8 * k * sf, sf)  # no sync between calls
        want = np.concatenate([ref.process(x[k * sf + f * n:k * sf + (f + 1) * n])[0] for f in range(sf // n)])
    got = rx.audio()[0]
    assert rel_rms(got, want) <= TOL
    with pytest.raises(P.PebbleGpuError):
        rx.process_device(buf.ptr, 0)



def test_bench_geometry_256_superframes_against_the_oracle(gpu_lib, oracle_mod):
    """bench.py's own call shape: configs[1] with 256 super-frames in ONE call, which makes the 8192-bin transform walk
    chains of 32 frames (two chains per 1024-item workgroup, the halves three barrier intervals apart) and the WFM chain
    run its long-call paths.  Against the oracle: the first three audio frames and the last one, and the spectra at both
    ends of the call and on both sides of three chain boundaries (frames 31|32, 32|33, 8191|8192|8193, 16351|16352);
    then the same input as two calls of 128: bit for bit in the spectrum."""
    import pebblesdr_amd as P
    fs, n, k = 20_000_000, 2048, 256
    rx = P.ReceiverBank(fs, 1, True, True, 8192, max_superframes=k)
    rx.set_mixer(0, 1.0e6)
    sf = rx.superframe
    N = k * sf
    t = np.arange(N, dtype=np.float64) / fs
    x = 0.5 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t)))
    del t
    x += lcg_noise(N, 11, 1e-2)
    x = ((np.round(x.real * 128) + 1j * np.round(x.imag * 128)) / 128.0).astype(np.complex64)
    A, S = rx.process(x)
    assert S.shape == (1, N // n, 8192) and A.shape == (1, N // 64)
    # spectra: frame f averages with frame f - 1, so the oracle transforms the pair (its first output is discarded)
    frames = [1, 2, 31, 32, 33, 8191, 8192, 8193, 16351, 16352, N // n - 1]
    for f in frames:
        sp = oracle_mod.Spectrum(8192, 2048)
        sp.process(x[(f - 1) * n:f * n].astype(np.complex128))
        r = sp.process(x[f * n:(f + 1) * n].astype(np.complex128))
        assert db_err(S[0, f], r) <= TOL_DB, "frame %d" % f
    # audio: the whole stream through the oracle chain (8192-sample decimator frames, see test_config2_wfm_with_spectrum)
    mix = oracle_mod.Mixer(fs); mix.set_frequency(1.0e6)
    dec = oracle_mod.Decimator(fs, 200000)
    dem = oracle_mod.DemodWFM(312500)
    z = np.concatenate([dec.process(mix.process(x[i:i + 8192].astype(np.complex128))) for i in range(0, N, 8192)])
    ra = np.concatenate([dem.process(z[i:i + 2048]) for i in range(0, len(z), 2048)])
    for fr in (0, 1, 2, 127, 128, k - 1):
        assert rel_rms(A[0, fr * 2048:(fr + 1) * 2048], ra[fr * 2048:(fr + 1) * 2048]) <= TOL, "audio frame %d" % fr
    # call splitting at this size
    rx2 = P.ReceiverBank(fs, 1, True, True, 8192, max_superframes=k)
    rx2.set_mixer(0, 1.0e6)
    h = N // 2
    (A1, S1), (A2, S2) = rx2.process(x[:h]), rx2.process(x[h:])
    assert np.array_equal(np.concatenate([S1, S2], axis=1), S)
    assert np.abs(np.concatenate([A1, A2], axis=1) - A).max() <= 1e-6


def test_empty_pass_band_meets_the_input_relative_bar(gpu_lib, oracle_mod):
    """The device stores samples in fp32, so its error is ~1e-7 of the INPUT's RMS; a band-pass that rejects the input's
    energy leaves an output so small that the same absolute error exceeds 1e-5 of the OUTPUT.  The bar is therefore two-sided:
    rel-RMS <= 1e-5 of the output, OR absolute RMS error <= 2e-7 of the input RMS.  Here the pass-band (USB 300-3000 Hz) holds
    nothing but the noise floor 80 dB under an out-of-band tone: the output-relative figure is allowed to miss, the
    input-relative one is not.  A second channel has its tone in band and must meet the output-relative bar."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    rx = P.ReceiverBank(fs, 2, True, False, 0, max_superframes=3)
    fc = [52e3, 80e3]
    refs = []
    for c in range(2):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fc[c]); rx.set_bandpass(c, 300, 3000)
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.USB); r.set_mixer(fc[c]); r.set_filter(300, 3000)
        refs.append(r)
    sf = rx.superframe
    N = 3 * sf
    # one tone: 15 kHz above channel 0's carrier (far outside its 300-3000 Hz pass-band), 1.5 kHz above channel 1's (inside)
    x = tones(fs, N, [(0.5, 52e3 + 15e3), (0.5, 80e3 + 1.5e3)]) + lcg_noise(N, 3, 1e-5)
    g = rx.process(x)[0]
    in_rms = float(np.sqrt(np.mean(np.abs(x) ** 2)))
    for c in range(2):
        r = np.concatenate([refs[c].process(x[f * n:(f + 1) * n], want_spectrum=False)[0] for f in range(N // n)])
        assert r.shape == g[c].shape
        for fr in range(3):
            sl = slice(fr * 2048, (fr + 1) * 2048)
            rel_out = rel_rms(g[c][sl], r[sl])
            abs_in = float(np.sqrt(np.mean(np.abs(g[c][sl] - r[sl]) ** 2))) / in_rms
            assert rel_out <= TOL or abs_in <= 2e-7, "channel %d frame %d: %.2e of output, %.2e of input" % (c, fr, rel_out, abs_in)
            if c == 1:
                assert rel_out <= TOL


@pytest.mark.parametrize("C", [1, 3])
def test_tune_only_mode_freezes_what_lies_behind_it(gpu_lib, oracle_mod, C):
    """dmNONE, "Tune only mode, no demod or output" (receiver.cpp:968-971): the call returns behind the band-pass -- no audio,
    and noise filter, AGC, demodulator and resampler keep the state the last demodulated super-frame left.  AM with a fast
    AGC (whose state a wrongly processed super-frame would visibly move): mode AM, AM, NONE, NONE, AM, AM against the
    oracle; C = 1 is the reference's own shape (the call reports zero samples), C = 3 a bank whose channel 1 alone goes
    tune-only (its row is cleared while the others keep demodulating)."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    fcs = [100e3, 250e3, -300e3][:C]
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=1)
    refs = []
    for c, fc in enumerate(fcs):
        rx.set_mode(c, P.DM_AM); rx.set_mixer(c, fc); rx.set_bandpass(c, -5000, 5000); rx.set_agc(c, 1, 20)
        r = oracle_mod.Receiver(fs, n, 0)
        r.set_mode(oracle_mod.AM); r.set_mixer(fc); r.set_filter(-5000, 5000); r.set_agc(1, 20)
        refs.append(r)
    sf = rx.superframe
    pattern = ["AM", "AM", "NONE", "NONE", "AM", "AM"]
    N = len(pattern) * sf
    t = np.arange(N) / fs
    x = sum(0.1 * (1 + 0.5 * np.cos(2 * np.pi * (600 + 150 * c) * t)) * (1 + 0.8 * np.sin(2 * np.pi * 3.0 * t)) * np.exp(2j * np.pi * fc * t)
            for c, fc in enumerate(fcs)) + lcg_noise(N, 9, 1e-4)
    who = 0 if C == 1 else 1   # the channel that goes tune-only
    for k, m in enumerate(pattern):
        if k == 0 or pattern[k - 1] != m:
            rx.set_mode(who, P.DM_AM if m == "AM" else P.DM_NONE)
            refs[who].set_mode(oracle_mod.AM if m == "AM" else oracle_mod.NONE)
        g = rx.process(x[k * sf:(k + 1) * sf])[0]
        for c in range(C):
            r = np.concatenate([refs[c].process(x[k * sf + f * n:k * sf + (f + 1) * n], want_spectrum=False)[0] for f in range(sf // n)])
            if c == who and m == "NONE":
                assert len(r) == 0
                assert (g.shape[1] == 0) if C == 1 else (g.shape[1] == 2048 and not g[c].any())
            else:
                assert g[c].shape == r.shape
                assert rel_rms(g[c], r) <= TOL_AGC_STARTUP, "super-frame %d channel %d" % (k, c)


@pytest.mark.parametrize("wfm", [False, True])
def test_zoomed_spectrum_of_the_decimated_frames(gpu_lib, oracle_mod, wfm):
    """SignalSpectrum::zoomed (signalspectrum.cpp:89-113, called at receiver.cpp:884 / :942): fftSpectrum with the hi-res bin
    count (settings.cpp:61: 2048) and a BlackmanHarris window over framesPerBuffer samples, of m_sampleBuf -- every frame at the
    demodulator rate, behind the gain restore on the narrow branch.  Two calls (the previous-frame average carries over)."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    C = 1 if wfm else 2
    fcs = [150e3, -320e3][:C]
    rx = P.ReceiverBank(fs, C, True, wfm, 0, max_superframes=3, hires_bins=2048)
    for c in range(C):
        rx.set_mixer(c, fcs[c])
        if not wfm:
            rx.set_mode(c, P.DM_USB); rx.set_bandpass(c, 300, 3000)
    sf = rx.superframe
    N = 5 * sf
    x = tones(fs, N, [(0.2, fcs[0] + 1234.5), (0.02, fcs[0] - 7000.0)] + ([(0.1, fcs[1] + 2500.0)] if C > 1 else [])) + lcg_noise(N, 4, 1e-3)
    Z = np.concatenate([(rx.process(x[lo:hi]), rx.zoom_spectrum())[1] for lo, hi in ((0, 2 * sf), (2 * sf, 5 * sf))], axis=1)
    stages = sum(int(np.log2(st)) for _, st in rx.chain())
    gain = 1.0 if wfm else 10 ** (2 * stages / 20.0)
    for c in range(C):
        mix = oracle_mod.Mixer(fs); mix.set_frequency(fcs[c])
        dec = oracle_mod.Decimator(fs, 200000 if wfm else 30000)
        z = np.concatenate([dec.process(mix.process(x[i:i + 8192])) for i in range(0, N, 8192)]) * gain
        sp = oracle_mod.Spectrum(2048, 2048)
        ref = np.array([sp.process(z[f * n:(f + 1) * n]) for f in range(len(z) // n)])
        assert Z[c].shape == ref.shape
        for f in range(1, len(ref)):
            assert db_err(Z[c][f], ref[f]) <= TOL_DB, "channel %d frame %d" % (c, f)


def test_squelch_in_a_bank(gpu_lib, oracle_mod):
    """The gate per channel of a bank (receiver.cpp:959-965 once per Receiver): three channels off one stream -- AM with a fast AGC,
    USB, and NFM -- each with its own carrier keyed on and off per super-frame in its own pattern, thresholds -60 / -60 / -120
    (never gates), several super-frames per call.  Against one oracle Receiver per channel: an open super-frame's audio matches
    the oracle's (whose AGC, demodulator and filter states slept through the closed ones), a closed one is silence in the
    bank's row where the oracle delivers nothing."""
    import pebblesdr_amd as P
    fs, n, bins = 2048000, 2048, 4096
    fcs = [100e3, -250e3, 400e3]
    modes = [(P.DM_AM, oracle_mod.AM, -5000, 5000), (P.DM_USB, oracle_mod.USB, 300, 3000), (P.DM_FMN, oracle_mod.FMN, -7500, 7500)]
    thr = [-60.0, -60.0, -120.0]
    C = 3
    rx = P.ReceiverBank(fs, C, True, False, bins, max_superframes=3)
    refs = []
    for c in range(C):
        gm, om, lo, hi = modes[c]
        rx.set_mode(c, gm); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, lo, hi)
        r = oracle_mod.Receiver(fs, n, bins)
        r.set_mode(om); r.set_mixer(fcs[c]); r.set_filter(lo, hi)
        if c == 0:
            rx.set_agc(c, 1, 20); r.set_agc(1, 20)
        rx.set_squelch(c, thr[c]); r.set_squelch(thr[c])
        refs.append(r)
    sf = rx.superframe
    patterns = [[1, 0, 1, 1, 0, 0, 1, 1], [0, 1, 1, 0, 1, 0, 0, 1], [1, 0, 0, 1, 1, 1, 0, 1]]
    K = len(patterns[0])
    N = K * sf
    t = np.arange(N) / fs
    x = lcg_noise(N, 9, 1e-5)
    for c in range(C):
        env = np.repeat(np.asarray(patterns[c], dtype=np.float64), sf)
        if c == 0:
            x = x + env * 0.1 * (1 + 0.5 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * fcs[c] * t)
        elif c == 1:
            x = x + env * 0.1 * np.exp(2j * np.pi * (fcs[c] + 1300.0) * t)
        else:
            x = x + env * 0.1 * np.exp(1j * (2 * np.pi * fcs[c] * t + 2.0 * np.sin(2 * np.pi * 800 * t)))
    # oracle, frame by frame: per super-frame either its audio or nothing
    want = [[None] * K for _ in range(C)]
    for c in range(C):
        for k in range(K):
            a = [refs[c].process(x[k * sf + f * n:k * sf + (f + 1) * n], want_spectrum=True)[0] for f in range(sf // n)]
            want[c][k] = np.concatenate(a)
    got = np.concatenate([rx.process(x[lo * sf:hi * sf])[0] for lo, hi in ((0, 3), (3, 4), (4, 6), (6, 8))], axis=1)
    assert got.shape == (C, K * 2048)
    opened = 0
    for c in range(C):
        for k in range(K):
            g = got[c, k * 2048:(k + 1) * 2048]
            if len(want[c][k]) == 0:
                assert thr[c] > -120 and not patterns[c][k]
                assert not g.any(), "channel %d super-frame %d should be gated" % (c, k)
            else:
                opened += 1
                assert len(want[c][k]) == 2048
                if c == 2 and (k == 0 or not patterns[c][k] or not patterns[c][k - 1]):
                    continue  # NFM on noise alone (never gated here: its PLL wanders) or re-acquiring behind it: compared once locked
                    # (see test_bank_with_every_narrow_demod_mode)
                bar = TOL_AGC_STARTUP if c == 0 else TOL
                assert rel_rms(g, want[c][k]) <= bar, "channel %d super-frame %d" % (c, k)
    assert opened >= 12


@pytest.mark.parametrize("fmt,dtype,scale,order,w64", [(0, np.int8, 128.0, 0, 0), (1, np.uint8, 128.0, 1, 0), (2, np.int16, 32768.0, 0, 0),
                                                       (4, np.int16, 32767.0, 3, 0), (3, np.float32, 1.0, 1, 0),
                                                       (0, np.int8, 128.0, 1, 1), (1, np.uint8, 128.0, 0, 1), (2, np.int16, 32768.0, 2, 1),
                                                       (4, np.int16, 32767.0, 0, 1), (3, np.float32, 1.0, 0, 1),
                                                       (0, np.int8, 128.0, 3, 2), (1, np.uint8, 128.0, 2, 2), (2, np.int16, 32768.0, 1, 2),
                                                       (4, np.int16, 32767.0, 3, 2), (3, np.float32, 1.0, 0, 2)])
def test_process_raw_converting_in_the_first_loads(gpu_lib, monkeypatch, fmt, dtype, scale, order, w64):
    """The bench's own shape fed in the device's sample format: at 20 Msps / 8192 bins / one channel the display transform and the
    first decimator stage read the raw pairs themselves (k_spectrum_t128<.., RAW>, k_mix_hb11_lean<RAW>: no float2 copy of the
    stream exists).  Every format and IQ order of normalizeIQ (deviceinterfacebase.cpp:648-838; WAV PCM16: wavfile.cpp:299-300)
    must give, bit for bit, what process() gives on the same samples converted on the host with the same constants -- over two
    calls, so the second one's first windows come from the history the first one left."""
    import pebblesdr_amd as P
    fs, bins = 20_000_000, 8192
    if w64 == 1:  # the opt-in display kernel converts in its loads as well (k_spectrum_w64<FMT>)
        monkeypatch.setenv("PEBBLEGPU_SPECTRUM_W64", "1")
    elif w64 == 2:  # ... and so does the display transform that also runs the decimator (k_spectrum_t128<2, FMT, DEC>)
        monkeypatch.setenv("PEBBLEGPU_FUSE_DEC", "1")
    a = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=4)
    b = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=4)
    for rx in (a, b):
        rx.set_mixer(0, 1.0e6)
    n = 4 * a.superframe
    rng = np.random.default_rng(5)
    t = np.arange(2 * n) / fs
    sig = 0.4 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t)))
    if dtype == np.float32:
        raw = np.stack([sig.real, sig.imag], axis=-1).astype(np.float32)
        conv = raw * np.float32(0.5)
    else:
        off = 128.0 if dtype == np.uint8 else 0.0
        raw = np.round(np.stack([sig.real, sig.imag], axis=-1) * (scale - 1) + off + rng.uniform(-1, 1, (2 * n, 2))).astype(dtype)
        conv = (raw.astype(np.float32) - np.float32(off)) * np.float32(0.5 / scale)
    i, q = conv[:, 0], conv[:, 1]
    x = {0: i + 1j * q, 1: q + 1j * i, 2: i + 1j * i, 3: q + 1j * q}[order].astype(np.complex64)
    for lo, hi in ((0, n), (n, 2 * n)):
        buf = P.DeviceBuffer.from_array(raw[lo:hi], 0)
        try:
            a.process_raw_device(buf.ptr, n, fmt, order, 0.5)
            ga, sa = a.audio(), a.spectrum()
        finally:
            buf.free()
        gb, sb = b.process(x[lo:hi])
        if lo:  # (the first call of a fresh receiver sits inside the oscillator's amplitude transient and takes the general route)
            assert a.kernel_name(2) == ("k_spectrum_t128 (decimator inside)" if w64 == 2 else "k_mix_hb11_lean")
            assert a.kernel_name(1) == ("k_spectrum_w64" if w64 == 1 else "k_spectrum_t128")
        assert np.abs(ga).max() > 1e-3
        assert np.array_equal(ga, gb)
        assert np.array_equal(sa, sb)


def test_pipelined_calls_run_back_to_back_and_match_joined_calls(gpu_lib, monkeypatch):
    """PEBBLEGPU_PIPELINE=1: successive calls no longer join their two streams -- the display transforms follow one another on
    one stream, the chains on the other, and a call's tail runs beside the next call's transform.  Five calls queued without
    a host synchronisation in between, a retune before the fourth (a setter makes the next call join first, so the change
    lands between the right two calls): audio and spectrum bit for bit what a receiver that joins every call gives (same kernels)."""
    import pebblesdr_amd as P
    fs, bins = 20_000_000, 8192
    monkeypatch.setenv("PEBBLEGPU_PIPELINE", "1")
    a = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=2)
    monkeypatch.delenv("PEBBLEGPU_PIPELINE")
    b = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=2)
    for rx in (a, b):
        rx.set_mixer(0, 1.0e6)
    n = 2 * a.superframe
    t = np.arange(5 * n) / fs
    x = (0.4 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(5 * n, 9, 1e-2)).astype(np.complex64)
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(x[k * n:(k + 1) * n]), 0) for k in range(5)]
    try:
        want_a, want_s = [], []
        for k in range(5):
            if k == 3:
                b.set_mixer(0, 1.2e6)
            b.process_device(bufs[k].ptr, n)
            b.synchronize()
            want_a.append(b.audio().copy()); want_s.append(b.spectrum().copy())
        for k in range(3):
            a.process_device(bufs[k].ptr, n)  # no synchronisation between these
        a.synchronize()
        assert np.array_equal(a.audio(), want_a[2]) and np.array_equal(a.spectrum(), want_s[2])
        a.set_mixer(0, 1.2e6)
        for k in (3, 4):
            a.process_device(bufs[k].ptr, n)
        a.synchronize()
        assert np.abs(a.audio()).max() > 1e-3
        assert np.array_equal(a.audio(), want_a[4]) and np.array_equal(a.spectrum(), want_s[4])
    finally:
        for bf in bufs:
            bf.free()


@pytest.mark.parametrize("fs,C,modes", [(2048000, 64, "usb"), (2048000, 20, "am_usb_fm"), (100000000, 64, "am_usb"), (2048000, 3, "am_usb_fm"), (10000000, 1, "usb")])
def test_two_stage_calls_back_to_back_equal_single_stream_calls(gpu_lib, monkeypatch, fs, C, modes):
    """A receiver without a display transform runs every call in two stages on two streams (mixer + decimator | band-pass, AGC,
    demodulators), the second stage beside the NEXT call's decimator, which writes the other of two output buffers; the band-pass's
    look-back is carried from one buffer into the other's head-room.  Calls queued without a host synchronisation in between
    -- one, two, ... seven in a row, a retune and a mode change before the fifth (a setter orders the two streams behind each other
    first) -- must leave bit for bit the audio a receiver created with PEBBLEGPU_BANK_PIPELINE=0 (every call on one stream, one
    output buffer) leaves after the same calls.  Banks on both first-stage forms, AM / USB / NFM channels mixed."""
    import pebblesdr_amd as P
    monkeypatch.setenv("PEBBLEGPU_BANK_PIPELINE", "0")
    b = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    monkeypatch.delenv("PEBBLEGPU_BANK_PIPELINE")
    a = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    kinds = {"usb": [P.DM_USB], "am_usb": [P.DM_AM, P.DM_USB], "am_usb_fm": [P.DM_AM, P.DM_USB, P.DM_FMN]}[modes]
    fcs = [(-0.4 + 0.8 * (c + 0.5) / C) * fs for c in range(C)]
    for rx in (a, b):
        for c in range(C):
            m = kinds[c % len(kinds)]
            rx.set_mode(c, m); rx.set_mixer(c, fcs[c])
            rx.set_bandpass(c, 300, 3000) if m == P.DM_USB else rx.set_bandpass(c, -4000, 4000)
    K = 7
    sf = a.superframe
    lens = [2 * sf, sf, 2 * sf, 2 * sf, sf, 2 * sf, 2 * sf] if fs < 50_000_000 else [sf] * K  # (a super-frame at 100 Msps is 4 M samples)
    x = (tones(fs, sum(lens), [(0.05, fc + 1000.0 + 40.0 * i) for i, fc in enumerate(fcs[:: max(1, C // 8)])]) + lcg_noise(sum(lens), 5, 1e-2)).astype(np.complex64)
    # (banks of fewer than 16 channels run the general kernels -- first stage, cascade -- on the first stream: the same two-stage calls)
    offs = np.concatenate([[0], np.cumsum(lens)])
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(x[offs[k]:offs[k + 1]]), 0) for k in range(K)]

    def retune(rx):
        rx.set_mixer(min(1, C - 1), fcs[min(1, C - 1)] + 700.0)
        rx.set_mode(min(2, C - 1), P.DM_LSB)
        rx.set_bandpass(min(2, C - 1), -3000, -300)
    try:
        want = []
        for k in range(K):
            if k == 4:
                retune(b)
            b.process_device(bufs[k].ptr, lens[k])
            b.synchronize()
            want.append(b.audio().copy())
        assert np.abs(want[-1]).max() > 1e-3
        k = 0
        for run in (1, 2, 1, 3):  # calls 0 | 1 2 | 3 | 4 5 6, each group queued back to back
            if k == 4:
                retune(a)
            for _ in range(run):
                a.process_device(bufs[k].ptr, lens[k])
                k += 1
            a.synchronize()
            got = a.audio()
            assert got.shape == want[k - 1].shape
            assert np.array_equal(got, want[k - 1]), "after call %d" % (k - 1)
        if C >= 16:
            assert a.kernel_name(2) == "k_mix_dec_mfma"
    finally:
        for bf in bufs:
            bf.free()


def test_two_stage_calls_in_long_runs_of_mixed_lengths(gpu_lib, monkeypatch):
    """The rotation of the decimator's output buffers under load: forty calls of 1, 2 and 16 super-frames (from 16 on a 256-channel bank
    rotates two buffers instead of three, with the nap in front of its second stage) in runs of one to seven queued back to back --
    more calls in flight than there are buffers, so the host's wait for the second stage that last read the buffer about to be
    written is exercised -- against the single-stream receiver after every run, bit for bit."""
    import pebblesdr_amd as P
    fs, C, KM = 2_048_000, 256, 16
    # (one wave per SIMD on both sides: by itself the single-stream receiver gives a long call two, i.e. other chunk boundaries and with
    # them other points where the oscillator's phase is set exactly instead of rotated -- 4e-9 of the output, not a bit-for-bit twin)
    monkeypatch.setenv("PEBBLEGPU_BANK_WAVES", "1")
    monkeypatch.setenv("PEBBLEGPU_BANK_PIPELINE", "0")
    b = P.ReceiverBank(fs, C, True, False, 0, max_superframes=KM)
    monkeypatch.delenv("PEBBLEGPU_BANK_PIPELINE")
    a = P.ReceiverBank(fs, C, True, False, 0, max_superframes=KM)
    fcs = [(-0.4 + 0.8 * (c + 0.5) / C) * fs for c in range(C)]
    for rx in (a, b):
        for c in range(C):
            rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000)
    sf = a.superframe
    rng = np.random.default_rng(17)
    pool = {}
    for k in (1, 2, KM):  # one input per call length, reused (the chain carries its state from call to call either way)
        x = (tones(fs, k * sf, [(0.05, fc + 900.0 + 30.0 * i) for i, fc in enumerate(fcs[::32])]) + lcg_noise(k * sf, 20 + k, 1e-2)).astype(np.complex64)
        pool[k] = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x), 0)
    try:
        lens = [int(v) for v in rng.choice([1, 1, 2, 2, 2, KM], size=40)]
        lens[5] = lens[6] = KM  # two long calls in a row, then short ones again
        i = 0
        while i < len(lens):
            run = int(rng.integers(1, 8))
            group = lens[i:i + run]
            for k in group:
                b.process_device(pool[k].ptr, k * sf)
            b.synchronize()
            want = b.audio().copy()
            for k in group:
                a.process_device(pool[k].ptr, k * sf)
            a.synchronize()
            got = a.audio()
            assert got.shape == want.shape and np.abs(want).max() > 1e-3
            assert np.array_equal(got, want), "after call %d (run of %d, lengths %s): rel rms %g" % (i + len(group) - 1, len(group), group, rel_rms(got, want))
            i += len(group)
        assert a.kernel_name(2) == "k_mix_dec_mfma"
    finally:
        for bf in pool.values():
            bf.free()


def test_decimator_inside_the_display_transform_switches_routes_with_a_retune(gpu_lib, monkeypatch):
    """PEBBLEGPU_FUSE_DEC=1: calls inside an oscillator transient (the first one, the one after a retune) take the stand-alone
    kernels, the others run the decimator inside k_spectrum_t128 -- each route leaves what the other needs in front of the next call
    (windowed last frame one way; first-stage tail and mixed-sample history the other).  Six calls of uneven length with a retune
    before the fourth, against a receiver that only ever uses the stand-alone kernels: audio within the parity tolerance on every
    call (4.7e-8 measured), spectra bit for bit."""
    import pebblesdr_amd as P
    fs, bins = 20_000_000, 8192
    monkeypatch.setenv("PEBBLEGPU_FUSE_DEC", "1")
    a = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=3)
    monkeypatch.delenv("PEBBLEGPU_FUSE_DEC")
    b = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=3)
    for rx in (a, b):
        rx.set_mixer(0, 1.0e6)
    sf = a.superframe
    lens = [1, 2, 3, 1, 3, 2]
    N = sum(lens) * sf
    t = np.arange(N) / fs
    x = (0.4 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(N, 11, 1e-2)).astype(np.complex64)
    lo, routes = 0, []
    for k, m in enumerate(lens):
        if k == 3:
            for rx in (a, b):
                rx.set_mixer(0, 1.15e6)
        seg = x[lo:lo + m * sf]
        lo += m * sf
        ga, sa = a.process(seg)
        gb, sb = b.process(seg)
        routes.append(a.kernel_name(2))
        assert b.kernel_name(2) != "k_spectrum_t128 (decimator inside)"
        assert np.abs(gb).max() > 1e-3
        assert rel_rms(ga, gb) <= TOL, "call %d" % k
        assert np.array_equal(sa, sb), "call %d" % k
    fused = "k_spectrum_t128 (decimator inside)"
    assert routes[0] != fused and routes[1] == fused and routes[2] == fused and routes[3] != fused and routes[4] == fused and routes[5] == fused


@pytest.mark.parametrize("fs,bw,simple,chain", [(2048000.0, 15000.0, False, [11, 11, 15, 19, 31]),       # receiver.cpp:198 at the stock rate
                                                 (10e6, 15000.0, False, [0, 11, 11, 11, 11, 15, 27]),      # a CIC3 in front
                                                 (20e6, 200000.0, True, [51] * 6),                         # receiver.cpp:217: the WFM chain
                                                 (250000.0, 48000.0, False, [])])                          # under HB51's limit: oscillator only
def test_downconvert_step_against_the_oracle(gpu_lib, oracle_mod, fs, bw, simple, chain):
    """CDownConvert (pebblelib/downconvert.cpp), the alternate mixer + decimator: pebblegpu_downconvert_* against the oracle's
    restatement -- the quadrature oscillator with its amplitude transient and its phase carried across calls AND across a retune
    (SetFrequency keeps m_Osc1; there is no "frequency 0" exit), the CIC3 ending on the pair's odd sample, the fixed 11-tap
    halfband, the generic halfband with tap 0 counted twice -- four calls of unequal length (the first inside the transient), a retune
    and a CW offset before the third, frequency 0 for the fourth.  Oracle: held to the reference's own CDownConvert on these four
    chains by tests/test_reference_pins.py (downconvert_*); tests/test_oracle_pins.py pins its stage limits to the reference's comments."""
    import pebblesdr_amd as P
    D = 1 << len(chain)
    lens = [D * 600, D * 256, D * 1024, D * 300]
    dc = P.DownConvert(max(lens))
    ref = oracle_mod.DownConvert()
    assert dc.SetDataRate(fs, bw, simple) == ref.set_data_rate(fs, bw, simple) == fs / D
    assert dc.stages() == ref.chain() == chain
    f0 = 0.11 * fs
    dc.SetFrequency(f0); ref.set_frequency(f0)
    n = sum(lens)
    x = tones(fs, n, [(0.3, f0 + 0.02 * fs / D), (0.2, f0 - 0.05 * fs / D), (0.3, f0 + 0.37 * fs), (0.1, 0.013 * fs / D)]) + lcg_noise(n, 4, 1e-3)
    off = 0
    for k, m in enumerate(lens):
        if k == 2:
            dc.SetCwOffset(700.0); ref.set_cw_offset(700.0)
            dc.SetFrequency(f0 + 0.01 * fs / D); ref.set_frequency(f0 + 0.01 * fs / D)
        if k == 3:
            dc.SetCwOffset(0.0); ref.set_cw_offset(0.0)
            dc.SetFrequency(0.0); ref.set_frequency(0.0)
        g = dc.ProcessData(x[off:off + m])
        r = ref.process(x[off:off + m])
        off += m
        assert g.shape == r.shape == (m // D,)
        assert rel_rms(g, r) <= TOL, (k, chain)
        assert np.abs(r).max() > 0.05
    with pytest.raises(P.PebbleGpuError):
        dc.ProcessData(x[:max(lens) + D])        # beyond the size it was created for
    if D > 1:
        with pytest.raises(P.PebbleGpuError):
            dc.ProcessData(x[:D * 600 + 1])      # not a multiple of 2^stages
    with pytest.raises(P.PebbleGpuError):
        P.DownConvert(1024).SetDataRate(100e6, 15000.0)   # eleven stages: the reference's list holds nine


def test_downconvert_rate_change_mirrors_the_tuning_as_the_reference_does(gpu_lib, oracle_mod):
    """SetDataRate ends with SetFrequency(m_NcoFreq) on the stored, already negated frequency (downconvert.cpp:205): tuned first and
    given its rates afterwards the object sits on the mirror frequency.  Reproduced (the oracle test of the same name shows it)."""
    import pebblesdr_amd as P
    fs, f0, n = 2048000.0, 100e3, 32 * 800
    x = tones(fs, n, [(0.5, f0 + 1000.0)])
    a = P.DownConvert(n); a.SetDataRate(fs, 15000.0); a.SetFrequency(f0)
    b = P.DownConvert(n); b.SetFrequency(f0); b.SetDataRate(fs, 15000.0)
    rb = oracle_mod.DownConvert(); rb.set_frequency(f0); rb.set_data_rate(fs, 15000.0)
    ya, yb = a.ProcessData(x), b.ProcessData(x)
    assert np.abs(ya[200:]).min() > 0.4 and np.abs(yb[200:]).max() < 1e-3
    want = rb.process(x)
    assert np.sqrt(np.mean(np.abs(yb - want) ** 2)) <= 2e-7 * 0.5   # (an empty band: the error against the INPUT's level, as everywhere)


def test_downconvert_device_api_equals_the_host_api(gpu_lib):
    """pebblegpu_downconvert_process_device (float2 device buffers in and out, queued on the object's stream) against
    pebblegpu_downconvert_process on the same samples: bit for bit, three calls."""
    import ctypes as C
    import pebblesdr_amd as P
    L = P.load_library()
    fs, n = 2048000.0, 32 * 512
    a, b = P.DownConvert(n), P.DownConvert(n)
    for d in (a, b):
        assert d.SetDataRate(fs, 15000.0) == 64000.0
        d.SetFrequency(123e3)
    x = (tones(fs, 3 * n, [(0.4, 124e3), (0.2, 119.5e3)]) + lcg_noise(3 * n, 3, 1e-3)).astype(np.complex64)
    for k in range(3):
        blk = x[k * n:(k + 1) * n]
        want = a.ProcessData(blk.astype(np.complex128))
        buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(blk), 0)
        try:
            dptr, no = C.c_void_p(), C.c_uint32()
            P.binding.check(L, L.pebblegpu_downconvert_process_device(b.h, C.c_void_p(buf.ptr), n, C.byref(dptr), C.byref(no)))
            P.binding.check(L, L.pebblegpu_downconvert_synchronize(b.h))
            got = np.empty(no.value, dtype=np.complex64)
            P.binding.check(L, L.pebblegpu_memcpy_d2h(0, got.ctypes.data_as(C.c_void_p), dptr, got.nbytes))
        finally:
            buf.free()
        assert no.value == n // 32 and np.abs(got).max() > 0.1
        assert np.array_equal(got.astype(np.complex128), want)


def test_pinned_ingest_slots_on_a_bank(gpu_lib):
    """The pinned slots feeding a shared-stream bank (no display transform: two-stage calls): four batches of int16 pairs through the
    two slots, each next upload queued while the previous call computes, against a twin handed the same pairs from device buffers."""
    import pebblesdr_amd as P
    fs, C = 2048000, 32
    a = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    b = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    fcs = [(-0.4 + 0.8 * (c + 0.5) / C) * fs for c in range(C)]
    for rx in (a, b):
        for c in range(C):
            rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000)
    n = 2 * a.superframe
    rng = np.random.default_rng(5)
    sig = 8000.0 * tones(fs, 4 * n, [(0.1, fc + 900.0) for fc in fcs[::4]])
    raw = np.empty((4 * n, 2), dtype=np.int16)
    raw[:, 0] = np.round(sig.real + rng.uniform(-3, 3, 4 * n)).astype(np.int16)
    raw[:, 1] = np.round(sig.imag + rng.uniform(-3, 3, 4 * n)).astype(np.int16)
    h = a.ingest_buffer(0, 4 * n, dtype=np.int16)
    h[:] = raw[:n].reshape(-1)
    a.ingest_submit(0, 4 * n)
    for k in range(4):
        s = k & 1
        a.process_ingested(s, n, 2, 0, 1.0)
        if k + 1 < 4:
            h = a.ingest_buffer(s ^ 1, 4 * n, dtype=np.int16)
            h[:] = raw[(k + 1) * n:(k + 2) * n].reshape(-1)
            a.ingest_submit(s ^ 1, 4 * n)
    ga = a.audio()
    for k in range(4):
        buf = P.DeviceBuffer.from_array(raw[k * n:(k + 1) * n], 0)
        try:
            b.process_raw_device(buf.ptr, n, 2, 0, 1.0)
            gb = b.audio()
        finally:
            buf.free()
    assert np.abs(gb).max() > 1e-3 and np.array_equal(ga, gb)


def test_two_stage_calls_interleaved_with_single_stream_calls(gpu_lib, monkeypatch):
    """A receiver that alternates between its two call shapes on a running stream: two-stage calls (stage 2 on the other stream,
    alternating output buffers, no tail launch between two bank kernels) and single-stream calls (per-kernel profiling on: every kernel
    on one stream) -- the histories each shape leaves are the ones the other picks up (first-stage staging buffers, the band-pass's
    look-back in the other output buffer, the oscillators advanced by the bank kernel or by the tail launch).  Eight calls queued
    without synchronisation against a receiver that only ever makes single-stream calls: bit for bit."""
    import pebblesdr_amd as P
    fs, C = 2048000, 48
    monkeypatch.setenv("PEBBLEGPU_BANK_PIPELINE", "0")
    b = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    monkeypatch.delenv("PEBBLEGPU_BANK_PIPELINE")
    a = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    fcs = [(-0.4 + 0.8 * (c + 0.5) / C) * fs for c in range(C)]
    for rx in (a, b):
        for c in range(C):
            m = P.DM_AM if c % 3 == 0 else P.DM_USB
            rx.set_mode(c, m); rx.set_mixer(c, fcs[c])
            rx.set_bandpass(c, 300, 3000) if m == P.DM_USB else rx.set_bandpass(c, -4000, 4000)
    sf = a.superframe
    K = 8
    x = (tones(fs, K * sf, [(0.05, fc + 1200.0) for fc in fcs[::6]]) + lcg_noise(K * sf, 12, 1e-2)).astype(np.complex64)
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(x[k * sf:(k + 1) * sf]), 0) for k in range(K)]
    try:
        for k in range(K):
            b.process_device(bufs[k].ptr, sf)
        want = b.audio()
        prof = [False, False, True, False, False, True, True, False]
        for k in range(K):
            a.set_profiling(prof[k])
            a.process_device(bufs[k].ptr, sf)
        got = a.audio()
        assert np.abs(want).max() > 1e-3 and np.array_equal(got, want)
        assert a.kernel_name(2) == "k_mix_dec_mfma"
    finally:
        for bf in bufs:
            bf.free()
