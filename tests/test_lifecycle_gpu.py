"""GPU tier (-m gpu): what a handle allocates it gives back.  pebblegpu_live_bytes counts the device and the pinned host bytes this
library holds in this process; every test reads it first and finds both counters there again at its end -- after a create /
every lazily allocating feature switched on / one call / destroy cycle of each handle type, and after creates the library refuses
when it has already begun to allocate.  After a refusal and after a destroy a fresh handle of the same kind still agrees with the
oracle (the suite's tolerances).

Two cases differ from how the issue behind this file worded them, because the library cannot be brought to what it names:
  - "the zoomed spectrum needs whole frames" (Receiver::create) cannot be reached through the configuration: a super-frame is
    total_decimation * lcm(frame, band-pass block) samples (design::superframe_len), so a call's demodulator-rate length is always
    whole frames.  The zoom pane's other refusal stands in: hires_bins = 3000, no power of two, which Receiver::create meets at the
    same place -- behind the cores, the spectrum and the resampler.
  - frame = 3000 with 4096 bins is a plan the library HAS (the frame rounded up to a power of two is 4096): it is created here and
    compared with the oracle.  The refused one is frame = 3000 with 2048 bins, fewer than the rounded frame.
dmFMS with RDS runs at 2.5 Msps, the rate the suite's other dmFMS receivers use."""
import gc

import numpy as np
import pytest

from tests import testbench_ref as R
from tests.signals import lcg_noise, tones
from tests.test_parity_gpu import TOL, TOL_DB, db_err, rel_rms

pytestmark = pytest.mark.gpu

FS, NF = 2048000, 2048
E_SIZE, E_UNSUPPORTED = -5, -6


def held(P):
    gc.collect()  # (handles of earlier tests that nobody closed go now, not in the middle of this one)
    return P.binding.live_bytes()


def signal(n, seed, fs=FS):
    return tones(fs, n, [(0.3, 101.5e3), (0.2, -199e3), (0.1, 50.7e3)]) + lcg_noise(n, seed, 1e-3)


def as_s8(x):
    """HackRF-shape pairs of the samples (I, Q interleaved int8) and the samples they stand for"""
    q = np.empty(x.shape + (2,), dtype=np.int8)
    q[..., 0] = np.clip(np.round(x.real * 128), -128, 127)
    q[..., 1] = np.clip(np.round(x.imag * 128), -128, 127)
    return q


# ---- one oracle comparison per kind of handle (what "still works" means after a refusal or a destroy) ----
def check_narrow(P, O, C=2, bins=4096, hires=0):
    rx = P.ReceiverBank(FS, C, True, False, bins, hires_bins=hires)
    try:
        x = signal(rx.superframe, 11)
        for c in range(C):
            rx.set_mode(c, P.DM_USB); rx.set_mixer(c, 100e3 + 300.0 * c); rx.set_bandpass(c, 300, 3000)
        audio, spec = rx.process(x)
        for c in range(C):
            ref = O.Receiver(FS, NF, bins)
            ref.set_mode(O.USB); ref.set_mixer(100e3 + 300.0 * c); ref.set_filter(300, 3000)
            out = [ref.process(x[f * NF:(f + 1) * NF]) for f in range(len(x) // NF)]
            assert rel_rms(audio[c], np.concatenate([a for a, _ in out])) <= TOL
            if c == 0:
                for f in range(1, len(out)):
                    assert db_err(spec[0][f], out[f][1]) <= TOL_DB
    finally:
        rx.close()


def check_wfm(P, O, fs=FS):
    rx = P.ReceiverBank(fs, 1, True, True, 0)
    try:
        n = rx.superframe
        t = np.arange(n) / fs
        x = 0.5 * np.exp(1j * (2 * np.pi * 250e3 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(n, 2, 1e-3)
        rx.set_mixer(0, 250e3)
        ref = O.Receiver(fs, NF, 0)
        ref.set_mode(O.FMM); ref.set_mixer(250e3)
        want = np.concatenate([ref.process(x[f * NF:(f + 1) * NF], want_spectrum=False)[0] for f in range(n // NF)])
        assert rel_rms(rx.process(x)[0][0], want) <= TOL
    finally:
        rx.close()


def check_streambank(P, O, N, S=2, F=2):
    fs = 2.0e6
    x = np.stack([tones(fs, F * N, [(0.4, 123456.7 * (c + 1)), (0.2, 20000.0 - 30000.0 * c), (0.1, 1700.0)]) + lcg_noise(F * N, 70 + c, 1e-4) for c in range(S)])
    sb = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=F)
    try:
        for c in range(S):
            sb.set_bandpass(c, -50e3, 50e3)
        y, sp = sb.process(x)
        for c in range(S):
            f = O.FastFIR(2048, 1025)
            f.setup(-50e3, 50e3, 0.0, fs)
            assert rel_rms(y[c], f.process(x[c])) <= TOL
            s = O.Spectrum(N, N, lift_clamp=True)
            rows = [s.process(x[c, k * N:(k + 1) * N]) for k in range(F)]
            assert db_err(sp[c, 1], rows[1]) <= TOL_DB
    finally:
        sb.close()


def check_mixer(P, O):
    x = signal(2 * NF, 3)
    ref, mx = O.Mixer(FS), P.Mixer(FS, NF)
    ref.set_frequency(100e3); mx.setFrequency(100e3)
    for f in range(2):
        assert rel_rms(mx.processBlock(x[f * NF:(f + 1) * NF]), ref.process(x[f * NF:(f + 1) * NF])) <= TOL
    mx.close()


def check_decimator(P, O, d=None):
    x = tones(FS, 3 * NF, [(0.5, 1000.0), (0.3, FS / 5), (0.1, -FS / 3)]) + lcg_noise(3 * NF, 3, 1e-2)  # (a tone the chain passes)
    ref = O.Decimator(FS, 30000)
    d = d or P.Decimator(FS, NF)
    assert d.buildDecimationChain(FS, 30000) == ref.rate
    for f in range(3):
        assert rel_rms(d.process(x[f * NF:(f + 1) * NF]), ref.process(x[f * NF:(f + 1) * NF])) <= TOL
    d.close()


def check_fastfir(P, O):
    x = tones(64000, 4 * NF, [(0.4873, 1000.0), (0.3, -12000.0)]) + lcg_noise(4 * NF, 4, 1e-3)
    ref, f = O.FastFIR(2048, 1025), P.FastFIR(2048, 1025)
    ref.setup(300, 3000, 0, 64000); f.SetupParameters(300, 3000, 0, 64000)
    seen = 0
    for k in range(4):
        r, g = ref.process(x[k * NF:(k + 1) * NF]), f.ProcessData(x[k * NF:(k + 1) * NF])
        assert len(r) == len(g)
        if len(r):
            seen += 1
            assert rel_rms(g, r) <= TOL
    assert seen
    f.close()


def check_demod(P, O):
    t = np.arange(3 * NF) / 64000.0
    am = (0.3 * (1 + 0.5 * np.cos(2 * np.pi * 1000 * t))) * np.exp(0.7j) + lcg_noise(3 * NF, 5, 1e-4)
    ref, d = O.DemodAM(64000, 10000), P.Demod(64000, 256000, NF)
    d.setDemodMode(P.DM_AM); d.setBandwidth(10000)
    for k in range(3):
        assert rel_rms(d.processBlock(am[k * NF:(k + 1) * NF]), ref.process(am[k * NF:(k + 1) * NF])) <= TOL
    d.close()


def check_spectrum(P, O, bins=4096, nf=NF):
    x = signal(3 * nf, 6)
    ref, s = O.Spectrum(bins, nf), P.Spectrum(bins, FS, nf)
    for k in range(3):
        r, (g, _) = ref.process(x[k * nf:(k + 1) * nf]), s.fftSpectrum(x[k * nf:(k + 1) * nf])
        if k:
            assert db_err(g, r) <= TOL_DB
    s.close()


def check_siggen(P, O):
    fs, a, b, rate = 2.048e6, -0.5e6, 0.7e6, 123456789.0
    g = P.SigGen(fs, NF)
    g.set_sweep(P.sweep(a, b, rate, amplitude=0.5, mix=True))
    g.set_noise(0.01, 99)
    x = lcg_noise(4 * NF, 5, 0.1).astype(np.complex64).astype(np.complex128)
    ref, _ = R.serial_sweep(fs, len(x), NF, 0.5, start=a, stop=b, rate=rate)
    want = x + ref + 0.01 * R.noise(99, 0, 0, len(x))[0]
    got = np.concatenate([g.generate(x[k * NF:(k + 1) * NF].copy()) for k in range(4)])
    assert rel_rms(got, want) <= TOL
    g.close()


def check_multibank(P, O):
    C = 3
    mb = P.MultiBank(FS, C, [0, 0], frames_per_buffer=NF, max_superframes=1)
    try:
        x = signal(mb.superframe, 12)
        for c in range(C):
            mb.set_mode(c, P.DM_USB); mb.set_mixer(c, 100e3 + 300.0 * c); mb.set_bandpass(c, 300, 3000)
        audio = mb.process(x)
        for c in range(C):
            ref = O.Receiver(FS, NF, 0)
            ref.set_mode(O.USB); ref.set_mixer(100e3 + 300.0 * c); ref.set_filter(300, 3000)
            want = np.concatenate([ref.process(x[f * NF:(f + 1) * NF], want_spectrum=False)[0] for f in range(len(x) // NF)])
            assert rel_rms(audio[c], want) <= TOL
    finally:
        mb.close()


# ---- the cycles: create, everything that allocates on first use, one smallest call, destroy ----
def receiver_features(P, rx, morse, zoom=False, wfm=False):
    B = P.binding
    C = rx.n_channels
    rx.enable_signal_strength(True)
    rx.set_taps([B.TAP_RAW_IQ, B.TAP_POST_MIXER] + ([] if wfm else [B.TAP_POST_BP]))
    rx.set_conditioners(0, B.COND_DC | B.COND_IQBALANCE | B.COND_NB1, 1.02, 0.03)
    if not wfm:
        for c in range(C):
            rx.set_noise_filter(c, True)
            rx.set_bandpass(c, 300, 3000)
        rx.set_mode(0, P.DM_SAM)       # (the PLL demodulators' buffers come with their first channel)
        rx.set_mode(C - 1, P.DM_FMN)
        if morse:
            rx.set_morse(0, True)
            rx.set_mode(0, P.DM_CWU)
        rx.set_squelch(0, -100.0)      # one channel, one super-frame: the read-back gate; a bank: the per-channel gate on the device
    rx.audio_out_open(B.AUDIO_F32, None, 4)
    rx.record_open(4)
    panes = [B.display_pane(B.PANE_SPECTRUM, B.DISPLAY_PIXELS_I32, B.screen_map(400, 301, -10.0, -110.0, -FS // 4, FS // 3))]
    if zoom:
        panes.append(B.display_pane(B.PANE_ZOOM, B.DISPLAY_WATERFALL_ARGB32, B.screen_map(255, 256, -20.0, -100.0, 0, 0), zoom=0.5))
    rx.display_open(panes, 4)
    rx.display_set_auto_scale(B.AUTO_SCALE_MAX | B.AUTO_SCALE_MIN)
    rx.set_spectrum_updates(10)


def receiver_calls(P, rx, fs=FS):
    n = rx.superframe
    x = signal(n, 21, fs) * 0.5
    raw = P.DeviceBuffer.from_array(as_s8(x))
    flt = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x))
    try:
        rx.process_raw_device(raw.ptr, n, P.binding.IQ_S8, P.binding.IQO_IQ)  # raw-format input: the staging buffer
        rx.process_device(flt.ptr, n)
        rx.synchronize()
    finally:
        raw.free(); flt.free()


def cycle_narrow_bank(P, O):
    rx = P.ReceiverBank(FS, 4, True, False, 4096, audio_rate=11025)
    receiver_features(P, rx, morse=False)
    receiver_calls(P, rx)
    rx.close()


def cycle_narrow_one(P, O):
    rx = P.ReceiverBank(FS, 1, True, False, 4096)
    receiver_features(P, rx, morse=True)
    receiver_calls(P, rx)
    assert rx.morse_status(0) is not None
    rx.close()


def cycle_wfm_rds(P, O):
    fs = 2_500_000
    rx = P.ReceiverBank(fs, 1, True, True, 8192)
    rx.set_mode(0, P.DM_FMS)  # the pilot loop, the (L - R) rows and the RDS branch
    rx.set_mixer(0, 250e3)
    receiver_features(P, rx, morse=False, wfm=True)
    receiver_calls(P, rx, fs)
    rx.rds_groups(0)
    rx.stereo_lock(0)
    rx.close()


def cycle_zoom(P, O):
    rx = P.ReceiverBank(FS, 1, True, False, 2048, hires_bins=2048)
    rx.set_mode(0, P.DM_FMN); rx.set_mixer(0, 300e3)
    receiver_features(P, rx, morse=False, zoom=True)
    receiver_calls(P, rx)
    rx.close()


def streambank_cycle(P, N, S, F):
    B = P.binding
    fs = 2.0e6
    sb = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=F)
    for s in range(S):
        sb.set_bandpass(s, -50e3, 50e3)
        sb.set_conditioners(s, B.COND_DC | B.COND_IQBALANCE | B.COND_NB1 | B.COND_NB2, 1.02, 0.03)
    sb.enable_signal_strength(True)
    sb.set_squelch(0, -100.0)
    sb.iq_out_open(B.AUDIO_F32, None, 4)
    sb.display_open(B.DISPLAY_WATERFALL_ARGB32, B.screen_map(255, 301, -20.0, -100.0, -400_000, 600_000), None, 0, n_slots=4)
    sb.display_set_auto_scale(3)
    x = np.stack([signal(F * N, 30 + s, fs) * 0.5 for s in range(S)])
    raw = P.DeviceBuffer.from_array(as_s8(x))
    flt = P.DeviceBuffer.from_array(B.to_f32_iq(x))
    try:
        sb.process_device(flt.ptr, F * N)
        sb.process_raw_device(raw.ptr, F * N, B.IQ_S8, B.IQO_IQ)   # conditioned: staged as float2
        for s in range(S):
            sb.set_conditioners(s, 0)
        sb.process_raw_device(raw.ptr, F * N, B.IQ_S8, B.IQO_IQ)   # the kernels convert in their loads where they can
        sb.set_spectrum_updates(1000)                              # the frame-list transform
        sb.process_device(flt.ptr, F * N)
        sb.synchronize()
    finally:
        raw.free(); flt.free()
    sb.close()


def cycle_decimator_twice(P, O):
    d = P.Decimator(FS, NF)
    d.buildDecimationChain(FS, 30000)
    d.process(signal(NF, 4))
    d.buildDecimationChain(FS, 200000)  # DecimCore::init a second time, in place
    d.process(signal(NF, 4))
    d.close()


def cycle_spectrum_step(P, O):
    s = P.Spectrum(4096, FS, NF)
    s.fftSpectrum(signal(NF, 6))
    s.mapFFTToScreen(400, 301, -10.0, -110.0, -FS // 4, FS // 3)
    s.mapFFTToScreen(400, 900, -10.0, -110.0, -FS // 4, FS // 3)  # (the pixel row grows)
    s.close()


def cycle_siggen(P, O):
    g = P.SigGen(FS, NF)
    g.set_sweep(P.sweep(-0.5e6, 0.7e6, 123456789.0, amplitude=0.5, mix=True))
    g.set_noise(0.01, 99)
    g.set_morse([P.morse_station(1000.0, 0.1, 25, 5, [0b11010, 0b11101, 0])])  # C, Q, a word space
    g.generate(lcg_noise(NF, 5, 0.1))
    g.generate(lcg_noise(2 * NF, 5, 0.1))  # (longer than the buffer it was created with: it grows)
    g.noise_draws(0, 256)
    g.close()


def cycle_multibank(P, O):
    mb = P.MultiBank(FS, 3, [0, 0], frames_per_buffer=NF, max_superframes=1)
    n = mb.superframe
    for c in range(3):
        mb.set_mode(c, P.DM_USB); mb.set_mixer(c, 100e3 + 300.0 * c); mb.set_bandpass(c, 300, 3000)
    mb.set_morse(1, True)
    host = mb.ingest_buffer(0, 2 * n)  # the pinned slot every shard reads, and the shards' device twins
    host[:] = as_s8(signal(n, 13) * 0.5).reshape(-1)
    mb.ingest_submit(0, 2 * n)
    mb.process_ingested(0, n, P.binding.IQ_S8)
    mb.synchronize()
    mb.close()


CYCLES = {
    "narrow bank, 4096 bins": (cycle_narrow_bank, lambda P, O: check_narrow(P, O)),
    "one narrow channel, Morse": (cycle_narrow_one, lambda P, O: check_narrow(P, O, 1)),
    "WFM dmFMS with RDS": (cycle_wfm_rds, lambda P, O: check_wfm(P, O)),
    "zoom pane": (cycle_zoom, lambda P, O: check_narrow(P, O, 1, 2048, 2048)),
    "65536 / 65536 spectrum": (lambda P, O: streambank_cycle(P, 65536, 2, 2), lambda P, O: check_streambank(P, O, 65536)),
    "stream bank": (lambda P, O: streambank_cycle(P, 2048, 3, 4), lambda P, O: check_streambank(P, O, 2048, 3, 4)),
    "mixer step": (lambda P, O: check_mixer(P, O), check_mixer),
    "decimator step, two chains": (cycle_decimator_twice, lambda P, O: check_decimator(P, O)),
    "fast FIR step": (lambda P, O: check_fastfir(P, O), check_fastfir),
    "demod step": (lambda P, O: check_demod(P, O), check_demod),
    "spectrum step": (cycle_spectrum_step, lambda P, O: check_spectrum(P, O)),
    "test bench step": (cycle_siggen, check_siggen),
    "multibank, one device": (cycle_multibank, check_multibank),
}


@pytest.mark.parametrize("kind", list(CYCLES))
def test_a_handle_gives_back_what_it_took(gpu_lib, oracle_mod, kind):
    import pebblesdr_amd as P
    cycle, check = CYCLES[kind]
    before = held(P)
    cycle(P, oracle_mod)
    assert held(P) == before, kind
    check(P, oracle_mod)  # second use: a fresh handle of the same kind, behind the destroy
    assert held(P) == before, kind


def test_live_bytes_sees_a_handle(gpu_lib):
    """the counters are not trivially constant: a receiver holds device memory, its ingest slot and its rings pinned memory"""
    import pebblesdr_amd as P
    before = held(P)
    rx = P.ReceiverBank(FS, 1, True, False, 4096)
    dev = P.binding.live_bytes()
    assert dev[0] > before[0] + 4 * 4096 and dev[1] >= before[1]
    rx.ingest_buffer(0, 2 * rx.superframe)
    rx.audio_out_open(P.binding.AUDIO_F32, None, 2)
    pin = P.binding.live_bytes()
    assert pin[0] > dev[0] and pin[1] >= before[1] + 2 * rx.superframe
    rx.close()
    assert held(P) == before


def refused(P, code, fn, *a, **kw):
    with pytest.raises(P.PebbleGpuError) as e:
        fn(*a, **kw)
    assert e.value.code == code


def test_refused_zoom_pane_leaves_nothing(gpu_lib, oracle_mod):
    """Receiver::create refuses at its zoom pane, behind the cores, the spectrum buffer and the resampler (the module's docstring says
    why not through "whole frames")"""
    import pebblesdr_amd as P
    before = held(P)
    refused(P, E_UNSUPPORTED, P.ReceiverBank, FS, 2, True, False, 2048, audio_rate=11025, hires_bins=3000)
    assert held(P) == before
    check_narrow(P, oracle_mod, 1, 2048, 2048)
    assert held(P) == before


def test_refused_spectrum_plan_leaves_nothing(gpu_lib, oracle_mod):
    """3000-sample frames round up to 4096: 2048 bins are refused -- by the step, and by a receiver whose cores exist by then"""
    import pebblesdr_amd as P
    before = held(P)
    refused(P, E_UNSUPPORTED, P.Spectrum, 2048, FS, 3000)
    assert held(P) == before
    refused(P, E_UNSUPPORTED, P.ReceiverBank, FS, 1, True, True, 2048, frames_per_buffer=3000)
    assert held(P) == before
    check_spectrum(P, oracle_mod, 4096, 3000)  # (4096 bins over the same frames is a plan the library has)
    assert held(P) == before


def test_refused_second_chain_leaves_nothing(gpu_lib, oracle_mod):
    """a decimator step whose second build_chain is refused (100 Msps / 3 kHz: a first stage of stride 128, too wide for the LDS tile):
    the first chain's buffers are gone, nothing of the second stays, and the same handle takes a third chain"""
    import pebblesdr_amd as P
    before = held(P)
    d = P.Decimator(FS, NF)
    d.buildDecimationChain(FS, 30000)
    with_chain = P.binding.live_bytes()
    refused(P, E_UNSUPPORTED, d.buildDecimationChain, 100000000, 3000)
    assert P.binding.live_bytes()[0] < with_chain[0]
    check_decimator(P, oracle_mod, d)  # (closes it)
    assert held(P) == before
    check_decimator(P, oracle_mod)
    assert held(P) == before
