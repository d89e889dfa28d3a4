"""GPU tier (-m gpu): receivers whose decimation chain is empty -- 48000 / 44100 Hz narrow (Decimator::buildDecimationChain(fs, 30000)
finds no stage below 75 kHz) and WFM below 500 kHz -- against oracle.Receiver frame by frame.

The narrow cases run on both routes of such a receiver: the mixer inside the band-pass's first loads (k_fastfir_t128_mix, the
default) and the stand-alone mixer into the band-pass's row (k_mixer; PEBBLEGPU_NO_FUSED_DEC=1 when the receiver is created).

Bars: those tests/test_parity_gpu.py holds the same paths to at 2.048 Msps -- 1e-5 relative RMS on audio (TOL), the in-phase path of
SAM to 1e-4 (test_sam_pll_demod_step), FMN from the second frame on (test_bank_with_every_narrow_demod_mode) -- and 0.1 dB on
spectra from the second spectrum on."""
import numpy as np
import pytest

from tests import morse_ref as M
from tests import morsegen_ref as G
from tests.signals import lcg_noise, tones
from tests.test_morse_gpu import events_of, oracle_pre_agc
from tests.test_parity_gpu import TOL, TOL_DB, _fm_stereo_mpx, db_err, rel_rms

pytestmark = pytest.mark.gpu

N, BINS = 2048, 4096
MIXING, MIXER = "k_fastfir_t128 (mixing)", "k_mixer"


@pytest.fixture(params=["mixing band-pass", "k_mixer"])
def route(request, monkeypatch):
    """-> the front kernel's name a narrow call without taps, zoom or bank gate must report"""
    if request.param == "k_mixer":
        monkeypatch.setenv("PEBBLEGPU_NO_FUSED_DEC", "1")
        return MIXER
    monkeypatch.delenv("PEBBLEGPU_NO_FUSED_DEC", raising=False)
    return MIXING


def mode_signal(mode, fs, n, fc, seed=5):
    """what each narrow mode demodulates, centred on the mixer frequency fc and inside +-2.5 kHz"""
    t = np.arange(n) / fs
    if mode in ("AM", "SAM"):
        x = 0.1 * (1 + 0.5 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * (fc + (25.0 if mode == "SAM" else 0.0)) * t)
    elif mode == "FMN":
        x = 0.1 * np.exp(1j * (2 * np.pi * fc * t + 2.0 * np.sin(2 * np.pi * 800 * t)))
    elif mode in ("USB", "CWU"):
        x = 0.1 * np.exp(2j * np.pi * (fc + 1500.0) * t) + 0.03 * np.exp(2j * np.pi * (fc + 600.0) * t)
    else:  # LSB, CWL
        x = 0.1 * np.exp(2j * np.pi * (fc - 700.0) * t) + 0.03 * np.exp(2j * np.pi * (fc - 1900.0) * t)
    return x + lcg_noise(n, seed, 1e-4)


def modes_of(P, O):
    return {"AM": (P.DM_AM, O.AM), "SAM": (P.DM_SAM, O.SAM), "FMN": (P.DM_FMN, O.FMN), "USB": (P.DM_USB, O.USB), "CWL": (P.DM_CWL, O.CWL),
            "LSB": (P.DM_LSB, O.LSB)}


def check_audio(mode, g, r, frame, what=""):
    """one frame of one channel against the oracle's, at the bar of its mode"""
    assert g.shape == r.shape, (what, mode, frame, g.shape, r.shape)
    if mode == "SAM":
        e, bar = rel_rms((g.real + g.imag) / 2, (r.real + r.imag) / 2), 1e-4
    elif mode == "FMN" and frame == 0:
        return  # the PLL acquires on the band-pass's fp32 floor (test_bank_with_every_narrow_demod_mode): compared once locked
    else:
        e, bar = rel_rms(g, r), TOL
    print("%s %s frame %d: rel-RMS %.3e (<= %.0e)" % (what, mode, frame, e, bar))
    assert e <= bar, (what, mode, frame, e)


# ------------------------------------------------------------------------------------------------
# 1. one channel, every narrow mode
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [48000, 44100])
def test_one_channel_in_every_narrow_mode(gpu_lib, oracle_mod, route, fs):
    """mixer -4 kHz, filter +-2.5 kHz, AM / SAM / FMN / USB / CWL, six frames, one per call; the receiver reports an empty chain"""
    import pebblesdr_amd as P
    fc = -4000.0
    for mode, (gm, om) in modes_of(P, oracle_mod).items():
        if mode == "LSB":
            continue
        rx = P.ReceiverBank(fs, 1, True, False, BINS)
        assert rx.chain() == [] and rx.D == 1 and rx.superframe == N
        assert int(rx.info.demod_rate_int) == fs and int(rx.info.dec_by2_stages) == 0
        ref = oracle_mod.Receiver(fs, N, BINS)
        rx.set_mode(0, gm); rx.set_mixer(0, fc); rx.set_bandpass(0, -2500, 2500)
        ref.set_mode(om); ref.set_mixer(fc); ref.set_filter(-2500, 2500)
        x = mode_signal(mode, fs, 6 * N, fc)
        for f in range(6):
            a, s = rx.process(x[f * N:(f + 1) * N])
            ra, rs = ref.process(x[f * N:(f + 1) * N])
            check_audio(mode, a[0], ra, f, "%d Hz" % fs)
            if f >= 1:
                assert db_err(s[0][0], rs) <= TOL_DB, (mode, f)
            assert rx.kernel_name(2) == route
        rx.close()


# ------------------------------------------------------------------------------------------------
# 2. mixer frequency 0, 3. a retune between calls
# ------------------------------------------------------------------------------------------------
def test_mixer_frequency_zero_passes_the_input(gpu_lib, oracle_mod, route):
    """Mixer::processBlock returns its input at frequency 0 (mixer.cpp:51-53): no oscillator, so no sqrt(0.95) amplitude either"""
    import pebblesdr_amd as P
    fs = 48000
    rx = P.ReceiverBank(fs, 1, True, False, BINS)
    ref = oracle_mod.Receiver(fs, N, BINS)
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, 0.0); rx.set_bandpass(0, 300, 3000)
    ref.set_mode(oracle_mod.USB); ref.set_mixer(0.0); ref.set_filter(300, 3000)
    x = mode_signal("USB", fs, 4 * N, 0.0, seed=8)
    for f in range(4):
        a, _ = rx.process(x[f * N:(f + 1) * N])
        ra, _ = ref.process(x[f * N:(f + 1) * N])
        assert rel_rms(a[0], ra) <= TOL, f
        if f:
            assert rel_rms(a[0] * np.sqrt(0.95), ra) > 1e-2  # (the bar tells the two apart)
    assert rx.kernel_name(2) == route
    rx.close()


def test_retune_between_calls_keeps_the_old_overlap(gpu_lib, oracle_mod, route):
    """a retune between call 2 and call 3 of 5: the first block of call 3 overlaps samples mixed at the OLD frequency, as
    m_pFFTOverlapBuf holds them, and the oscillator starts over (phase 0, amplitude transient)"""
    import pebblesdr_amd as P
    fs = 48000
    rx = P.ReceiverBank(fs, 1, True, False, 0)
    ref = oracle_mod.Receiver(fs, N, 0)
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, -4000.0); rx.set_bandpass(0, 300, 3000)
    ref.set_mode(oracle_mod.USB); ref.set_mixer(-4000.0); ref.set_filter(300, 3000)
    x = tones(fs, 5 * N, [(0.1, -4000.0 + 1500.0), (0.05, -4000.0 + 2100.0), (0.08, 7000.0 + 900.0)]) + lcg_noise(5 * N, 12, 1e-4)
    for f in range(5):
        if f == 2:
            rx.set_mixer(0, 7000.0); ref.set_mixer(7000.0)
        a, _ = rx.process(x[f * N:(f + 1) * N])
        ra, _ = ref.process(x[f * N:(f + 1) * N], want_spectrum=False)
        e = rel_rms(a[0], ra)
        print("call %d: rel-RMS %.3e" % (f, e))
        assert e <= TOL, f
        assert rx.kernel_name(2) == route
    rx.close()


# ------------------------------------------------------------------------------------------------
# 4. a bank on one shared stream, 5. independent streams
# ------------------------------------------------------------------------------------------------
BANK = [("AM", -4000.0), ("USB", 0.0), ("FMN", 9000.0), ("CWL", -12000.0), ("SAM", 15000.0)]


@pytest.mark.parametrize("fft,taps", [(2048, 1025), (4096, 1025)])
def test_bank_of_five_on_a_shared_stream(gpu_lib, oracle_mod, route, fft, taps):
    """five channels in mixed modes, one at frequency 0, calls of 1, 3 and 1 super-frames (blocks behind a call's first recompute their
    overlap from the stream); the 4096-point band-pass has no mixing variant: whatever was asked for, the call takes k_mixer"""
    import pebblesdr_amd as P
    fs = 48000
    md = modes_of(P, oracle_mod)
    rx = P.ReceiverBank(fs, len(BANK), True, False, 0, fastfir_fft=fft, fastfir_taps=taps, max_superframes=3)
    sf = rx.superframe
    assert sf == (N if fft == 2048 else 3 * N)
    refs = []
    for c, (mode, fc) in enumerate(BANK):
        rx.set_mode(c, md[mode][0]); rx.set_mixer(c, fc); rx.set_bandpass(c, -2500, 2500)
        r = oracle_mod.Receiver(fs, N, 0, fft, taps)
        r.set_mode(md[mode][1]); r.set_mixer(fc); r.set_filter(-2500, 2500)
        refs.append(r)
    n = 5 * sf
    x = sum(mode_signal(mode, fs, n, fc, seed=20 + c) for c, (mode, fc) in enumerate(BANK))
    g = np.concatenate([rx.process(x[lo * sf:hi * sf])[0] for lo, hi in ((0, 1), (1, 4), (4, 5))], axis=1)
    assert rx.kernel_name(2) == (route if fft == 2048 else MIXER)
    for c, (mode, _) in enumerate(BANK):
        r = np.concatenate([refs[c].process(x[f * N:(f + 1) * N], want_spectrum=False)[0] for f in range(n // N)])
        assert r.shape == g[c].shape
        for f in range(n // N):
            check_audio(mode, g[c][f * N:(f + 1) * N], r[f * N:(f + 1) * N], f, "channel %d" % c)
    rx.close()


def test_three_independent_streams(gpu_lib, oracle_mod, route):
    import pebblesdr_amd as P
    fs, C = 48000, 3
    f0 = [-4000.0, 5000.0, -11000.0]
    rx = P.ReceiverBank(fs, C, False, False, BINS)
    refs = [oracle_mod.Receiver(fs, N, BINS) for _ in range(C)]
    for c in range(C):
        rx.set_mode(c, P.DM_LSB); rx.set_mixer(c, f0[c]); rx.set_bandpass(c, -3000, -300)
        refs[c].set_mode(oracle_mod.LSB); refs[c].set_mixer(f0[c]); refs[c].set_filter(-3000, -300)
    xs = np.stack([mode_signal("LSB", fs, 4 * N, f0[c], seed=30 + c) for c in range(C)])
    for f in range(4):
        a, s = rx.process(xs[:, f * N:(f + 1) * N])
        for c in range(C):
            ra, rs = refs[c].process(xs[c, f * N:(f + 1) * N])
            assert rel_rms(a[c], ra) <= TOL, (c, f)
            if f:
                assert db_err(s[c][0], rs) <= TOL_DB, (c, f)
    assert rx.kernel_name(2) == route
    rx.close()


# ------------------------------------------------------------------------------------------------
# 6. the POST_MIXER tap, and the hand-over between the routes
# ------------------------------------------------------------------------------------------------
def test_post_mixer_tap_and_the_route_hand_over(gpu_lib, oracle_mod, route):
    """the tap is the mixer's output and needs the mixed rows: k_mixer while it is on.  Off again, the next call is back on the
    receiver's own route with the overlap the other route left -- in both directions"""
    import pebblesdr_amd as P
    fs, C = 48000, 2
    f0 = [-4000.0, 6000.0]
    rx = P.ReceiverBank(fs, C, True, False, 0)
    refs, mixers = [], []
    for c in range(C):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, f0[c]); rx.set_bandpass(c, 300, 3000)
        r = oracle_mod.Receiver(fs, N, 0)
        r.set_mode(oracle_mod.USB); r.set_mixer(f0[c]); r.set_filter(300, 3000)
        refs.append(r)
        m = oracle_mod.Mixer(fs); m.set_frequency(f0[c])
        mixers.append(m)
    x = sum(mode_signal("USB", fs, 6 * N, f0[c], seed=40 + c) for c in range(C))
    for f, tap_on in enumerate([False, True, False, False, True, False]):
        rx.set_taps([P.TAP_POST_MIXER] if tap_on else [])
        fr = x[f * N:(f + 1) * N]
        a, _ = rx.process(fr)
        assert rx.kernel_name(2) == (MIXER if tap_on else route), f
        t = rx.tap(P.TAP_POST_MIXER)
        assert (t is not None) == tap_on
        for c in range(C):
            mixed = mixers[c].process(fr)
            if tap_on:
                assert t[1] == fs and rel_rms(t[0][c], mixed) <= TOL, (c, f)
            e = rel_rms(a[c], refs[c].process(fr, want_spectrum=False)[0])
            print("call %d channel %d (%s): rel-RMS %.3e" % (f, c, rx.kernel_name(2), e))
            assert e <= TOL, (c, f)
    rx.close()


# ------------------------------------------------------------------------------------------------
# 7. WFM at the input rate
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,fc,beta", [(192000, 20e3, 40.0), (250000, 20e3, 40.0), (300000, -30e3, 60.0), (384000, 50e3, 75.0), (48000, 4e3, 5.0)])
def test_wfm_mono_at_the_input_rate(gpu_lib, oracle_mod, fs, fc, beta):
    """buildDecimationChain(fs, 200000) finds no stage below 500 kHz: Demod_WFM runs at the input rate (FunCube Pro+ at 192000, RTL or
    SDRplay at 250000 / 300000, HPSDR at 384000, a sound card at 48000); a 1 kHz tone at beta kHz deviation, four frames"""
    import pebblesdr_amd as P
    rx = P.ReceiverBank(fs, 1, True, True, BINS)
    assert rx.chain() == [] and rx.D == 1 and rx.superframe == N and int(rx.info.demod_rate_int) == fs
    ref = oracle_mod.Receiver(fs, N, BINS)
    ref.set_mode(oracle_mod.FMM)
    rx.set_mixer(0, fc); ref.set_mixer(fc)
    t = np.arange(4 * N) / fs
    x = 0.5 * np.exp(1j * (2 * np.pi * fc * t + beta * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(4 * N, 2, 1e-3)
    for f in range(4):
        a, s = rx.process(x[f * N:(f + 1) * N])
        ra, rs = ref.process(x[f * N:(f + 1) * N])
        e = rel_rms(a[0], ra)
        print("%d Hz frame %d: rel-RMS %.3e" % (fs, f, e))
        assert len(ra) == N and e <= TOL, f
        if f:
            assert db_err(s[0][0], rs) <= TOL_DB, f
    assert rx.kernel_name(2) == MIXER
    rx.close()


def test_wfm_stereo_at_250000(gpu_lib, oracle_mod):
    """dmFMS at the input rate, held as test_parity_gpu.py::test_wfm_stereo_mode_in_the_receiver holds it at 2.5 Msps: every
    super-frame from the first, the first two in one call, left and right separately"""
    import pebblesdr_amd as P
    fs = 250000
    rx = P.ReceiverBank(fs, 1, True, True, 0, max_superframes=2)
    rx.set_mode(0, P.DM_FMS)
    rx.set_mixer(0, 25e3)
    sf = rx.superframe
    assert sf == N
    K = 8
    x = _fm_stereo_mpx(fs, K * sf) * np.exp(2j * np.pi * 25e3 * np.arange(K * sf) / fs) + lcg_noise(K * sf, 4, 1e-4)
    ref = oracle_mod.Receiver(fs, N, 0)
    ref.set_mode(oracle_mod.FMS)
    ref.set_mixer(25e3)
    ra = [ref.process(x[f * N:(f + 1) * N], want_spectrum=False)[0] for f in range(K)]
    first = rx.process(x[:2 * sf])[0][0]
    ga = [first[:N], first[N:]] + [rx.process(x[k * sf:(k + 1) * sf])[0][0] for k in range(2, K)]
    for k in range(K):
        assert len(ra[k]) == N
        el, er = rel_rms(ga[k].real, ra[k].real), rel_rms(ga[k].imag, ra[k].imag)
        print("block %d: left %.3e right %.3e" % (k, el, er))
        assert el <= TOL and er <= TOL, k
    rx.close()


# ------------------------------------------------------------------------------------------------
# 8. raw device formats
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,dtype,scale,order", [(0, np.int8, 128.0, 0), (2, np.int16, 32768.0, 1)])
def test_raw_calls_equal_float2_calls(gpu_lib, route, fmt, dtype, scale, order):
    """int8 and int16 pairs through _process_raw and through the ingest slots are staged through normalizeIQ: audio and spectrum
    equal, bit for bit, those of a float2 call fed the samples converted on the host with the reference's constants"""
    import pebblesdr_amd as P
    fs = 48000
    rxs = [P.ReceiverBank(fs, 1, True, False, BINS, max_superframes=2) for _ in range(3)]
    for rx in rxs:
        rx.set_mode(0, P.DM_USB); rx.set_mixer(0, -4000.0); rx.set_bandpass(0, 300, 3000)
    a, b, c = rxs
    n = 2 * a.superframe
    rng = np.random.default_rng(7 + fmt)
    item = np.dtype(dtype).itemsize
    for k in range(3):
        sig = 0.4 * scale * tones(fs, n, [(1.0, -4000.0 + 1500.0 + 50.0 * k)])
        raw = np.empty((n, 2), dtype=dtype)
        raw[:, 0] = np.round(sig.real + rng.uniform(-1, 1, n)).astype(dtype)
        raw[:, 1] = np.round(sig.imag + rng.uniform(-1, 1, n)).astype(dtype)
        first, second = (raw[:, 0], raw[:, 1]) if order == 0 else (raw[:, 1], raw[:, 0])
        x = (first.astype(np.float32) * np.float32(0.5 / scale) + 1j * (second.astype(np.float32) * np.float32(0.5 / scale))).astype(np.complex64)
        buf = P.DeviceBuffer.from_array(raw, 0)
        try:
            a.process_raw_device(buf.ptr, n, fmt, order, 0.5)
            ga, sa = a.audio(), a.spectrum()
        finally:
            buf.free()
        h = b.ingest_buffer(k & 1, 2 * n * item, dtype)
        h[:] = raw.reshape(-1)
        b.ingest_submit(k & 1, 2 * n * item)
        b.process_ingested(k & 1, n, fmt, order, 0.5)
        gb, sb = b.audio(), b.spectrum()
        gc, sc = c.process(x)
        assert np.abs(gc).max() > 1e-3
        assert np.array_equal(ga, gc) and np.array_equal(sa, sc), k
        assert np.array_equal(gb, gc) and np.array_equal(sb, sc), k
    assert a.kernel_name(2) == route and b.kernel_name(2) == route
    for rx in rxs:
        rx.close()


# ------------------------------------------------------------------------------------------------
# 9. zoomed spectrum and the resampler
# ------------------------------------------------------------------------------------------------
def test_zoomed_spectrum_of_the_mixed_frames(gpu_lib, oracle_mod, route):
    """SignalSpectrum::zoomed reads m_sampleBuf, here the mixer's output at the input rate: the zoomed transform needs the mixed rows"""
    import pebblesdr_amd as P
    fs, fc = 48000, -4000.0
    rx = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=3, hires_bins=2048)
    ref = oracle_mod.Receiver(fs, N, 0)
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, fc); rx.set_bandpass(0, 300, 3000)
    ref.set_mode(oracle_mod.USB); ref.set_mixer(fc); ref.set_filter(300, 3000)
    x = mode_signal("USB", fs, 5 * N, fc, seed=50)
    got = [(rx.process(x[lo * N:hi * N])[0], rx.zoom_spectrum()) for lo, hi in ((0, 2), (2, 5))]
    assert rx.kernel_name(2) == MIXER
    Z = np.concatenate([z for _, z in got], axis=1)
    A = np.concatenate([a for a, _ in got], axis=1)
    mix = oracle_mod.Mixer(fs); mix.set_frequency(fc)
    sp = oracle_mod.Spectrum(2048, 2048)
    zr = np.array([sp.process(mix.process(x[f * N:(f + 1) * N])) for f in range(5)])
    assert Z[0].shape == zr.shape
    for f in range(5):
        ra, _ = ref.process(x[f * N:(f + 1) * N], want_spectrum=False)
        assert rel_rms(A[0][f * N:(f + 1) * N], ra) <= TOL, f
        if f:
            assert db_err(Z[0][f], zr[f]) <= TOL_DB, f
    rx.close()


@pytest.mark.parametrize("fs,audio_rate", [(48000, 8000), (44100, 48000)])
def test_resampled_audio_counts_and_samples(gpu_lib, oracle_mod, route, fs, audio_rate):
    """CFractResampler behind the demodulator, down (48000 -> 8000) and up (44100 -> 48000): the output count of every call is the
    oracle's (its running fp64 time sum), the samples within the bar"""
    import pebblesdr_amd as P
    rx = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=2, audio_rate=audio_rate)
    ref = oracle_mod.Receiver(fs, N, 0)
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, -4000.0); rx.set_bandpass(0, 300, 3000)
    ref.set_mode(oracle_mod.USB); ref.set_mixer(-4000.0); ref.set_filter(300, 3000); ref.set_audio_rate(audio_rate)
    x = mode_signal("USB", fs, 6 * N, -4000.0, seed=60)
    for lo, hi in ((0, 1), (1, 3), (3, 4), (4, 6)):
        a, _ = rx.process(x[lo * N:hi * N])
        r = np.concatenate([ref.process(x[f * N:(f + 1) * N], want_spectrum=False)[0] for f in range(lo, hi)])
        assert a.shape[1] == len(r), (lo, hi, a.shape, len(r))
        assert rel_rms(a[0], r) <= TOL, (lo, hi)
    assert rx.kernel_name(2) == route
    rx.close()


# ------------------------------------------------------------------------------------------------
# 10. the Morse modem behind the test bench's keyed stations
# ------------------------------------------------------------------------------------------------
LOOP = [(-4000.0, 25, "TEST "), (6000.0, 40, "CQ DE K1ABC ")]


def test_morse_modem_on_a_48_khz_bank(gpu_lib, oracle_mod, route):
    """the CW-skimmer arrangement: one 48 kHz stream, CWU channels with the modem on, two stations keyed on the device 1 kHz above the
    mixers.  Events and status equal the restatement's fed the oracle chain over input + restated stations (tests/test_morsegen_gpu.py
    holds the 2.048 Msps loop the same way).  Measured on the CPU for these inputs: margins 8.8e-3 and 9.5e-2, 13 and 12 events."""
    import pebblesdr_amd as P
    fs = 48000
    rx = P.ReceiverBank(fs, len(LOOP), True, False, 0, max_superframes=8)
    for c, (fc, _, _) in enumerate(LOOP):
        rx.set_mixer(c, fc); rx.set_bandpass(c, 300, 3000); rx.set_morse(c, True); rx.set_mode(c, P.DM_CWU)
    K, per = 12, 8 * N
    n = K * per
    x = lcg_noise(n, 3, 2e-4).astype(np.complex64)
    stations = [(fc + 1000.0, 0.01, wpm, 5, text) for fc, wpm, text in LOOP]
    rx.set_testbench_morse([P.morse_station(f, a, w, r, G.text_tokens(t)) for f, a, w, r, t in stations], mix=True)
    got = [[] for _ in LOOP]
    for k in range(K):
        rx.process(x[k * per:(k + 1) * per])
        for c in range(len(LOOP)):
            got[c] += events_of(rx.morse_events(c))
    assert rx.kernel_name(2) == "k_morsegen + " + route
    total = x.astype(np.complex128) + G.station_sum(fs, [(f, a, w, r, G.text_tokens(t)) for f, a, w, r, t in stations], n)[0]
    for c, (fc, _, _) in enumerate(LOOP):
        a, rate = oracle_pre_agc(oracle_mod, total, fs, fc, 300, 3000)
        assert rate == fs
        r = M.MorseRef(rate, N)
        r.set_demod_mode(M.DM_CWU)
        for j in range(len(a) // N):
            r.process(a[j * N:(j + 1) * N])
        assert min(r.margins) > 1e-4 and len(r.events) >= 10, (c, min(r.margins), len(r.events))
        assert got[c] == r.events, (c, got[c], r.events)
        assert rx.morse_status(c) == r.status()
    rx.close()


# ------------------------------------------------------------------------------------------------
# 11. the bank's squelch
# ------------------------------------------------------------------------------------------------
def test_bank_squelch_gates_per_channel(gpu_lib, oracle_mod):
    """two USB channels with thresholds: one always above its own, one keyed on for two super-frames.  Which super-frames close is
    the oracle's decision (the spectrum averages two frames: the first one behind the carrier stays open); a closed one is silence in
    the bank's row, an open one matches the oracle and the run without thresholds.  The gate keeps the call on k_mixer's route"""
    import pebblesdr_amd as P
    fs, C = 48000, 2
    f0 = [-4000.0, 6000.0]
    pattern = [[1, 1, 1, 1, 1, 1], [0, 1, 1, 0, 0, 0]]
    K = len(pattern[0])
    t = np.arange(K * N) / fs
    x = lcg_noise(K * N, 9, 1e-5)
    for c in range(C):
        x = x + np.repeat(np.asarray(pattern[c], dtype=np.float64), N) * 0.1 * np.exp(2j * np.pi * (f0[c] + 1300.0) * t)
    gated = P.ReceiverBank(fs, C, True, False, BINS, max_superframes=3)
    plain = P.ReceiverBank(fs, C, True, False, BINS, max_superframes=3)
    refs = []
    for c in range(C):
        for rx in (gated, plain):
            rx.set_mode(c, P.DM_USB); rx.set_mixer(c, f0[c]); rx.set_bandpass(c, 300, 3000)
        gated.set_squelch(c, -60.0)
        r = oracle_mod.Receiver(fs, N, BINS)
        r.set_mode(oracle_mod.USB); r.set_mixer(f0[c]); r.set_filter(300, 3000); r.set_squelch(-60.0)
        refs.append(r)
    calls = ((0, 3), (3, 4), (4, 6))
    g = np.concatenate([gated.process(x[lo * N:hi * N])[0] for lo, hi in calls], axis=1)
    p = np.concatenate([plain.process(x[lo * N:hi * N])[0] for lo, hi in calls], axis=1)
    assert gated.kernel_name(2) == MIXER
    closed = 0
    for c in range(C):
        for k in range(K):
            ra, _ = refs[c].process(x[k * N:(k + 1) * N])
            row = g[c, k * N:(k + 1) * N]
            if len(ra) == 0:
                closed += 1
                assert not pattern[c][k] and not row.any(), (c, k)
            else:
                assert rel_rms(row, p[c, k * N:(k + 1) * N]) <= TOL and rel_rms(row, ra) <= TOL, (c, k)
    assert closed == 3
    gated.close()
    plain.close()


# ------------------------------------------------------------------------------------------------
# 12. the host's single-frame entry point, 13. a multibank
# ------------------------------------------------------------------------------------------------
def test_process_iq_frame_by_frame(gpu_lib, oracle_mod, route):
    import pebblesdr_amd as P
    fs, fc = 48000, -4000.0
    rx = P.ReceiverBank(fs, 1, True, False, BINS)
    ref = oracle_mod.Receiver(fs, N, BINS)
    rx.set_mode(0, P.DM_AM); rx.set_mixer(0, fc); rx.set_bandpass(0, -2500, 2500)
    ref.set_mode(oracle_mod.AM); ref.set_mixer(fc); ref.set_filter(-2500, 2500)
    x = mode_signal("AM", fs, 4 * N, fc, seed=70).astype(np.complex64).astype(np.complex128)
    for f in range(4):
        a, s = rx.process_iq(x[f * N:(f + 1) * N], want_spectrum=True)
        ra, rs = ref.process(x[f * N:(f + 1) * N])
        assert len(a) == len(ra) == N
        assert rel_rms(a, ra) <= TOL, f
        if f:
            assert db_err(s, rs) <= TOL_DB, f
    assert rx.kernel_name(2) == route
    rx.close()


def test_multibank_of_four_equals_one_bank(gpu_lib, route):
    """two shards of two channels on one device against ONE bank of four: the same kernels per channel, so the same bits"""
    import pebblesdr_amd as P
    fs, C = 48000, 4
    f0 = [-9000.0, -4000.0, 0.0, 6000.0]
    mb = P.MultiBank(fs, C, [0, 0], shared_input=True, spectrum_bins=0, frames_per_buffer=N, max_superframes=2)
    bank = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    assert mb.superframe == N and mb.D == 1
    for c in range(C):
        for rx in (mb, bank):
            rx.set_mode(c, P.DM_USB); rx.set_mixer(c, f0[c]); rx.set_bandpass(c, 300, 3000)
    x = sum(mode_signal("USB", fs, 5 * N, f0[c], seed=80 + c) for c in range(C))
    for lo, hi in ((0, 1), (1, 3), (3, 5)):
        got = mb.process(x[lo * N:hi * N])
        want = bank.process(x[lo * N:hi * N])[0]
        assert got.shape == want.shape and np.abs(want).max() > 1e-3
        assert np.array_equal(got, want), (lo, hi)
    assert mb.shard(0).kernel_name(2) == mb.shard(1).kernel_name(2) == bank.kernel_name(2) == route
    mb.close()
    bank.close()


# ------------------------------------------------------------------------------------------------
# what else hangs off a receiver: conditioners, AGC, noise filter, the audio and recording rings
# ------------------------------------------------------------------------------------------------
def test_conditioners_agc_and_noise_filter(gpu_lib, oracle_mod, route):
    """at 48 kHz, held as tests/test_parity_gpu.py holds them at 2.048 Msps: all four conditioners against the oracle chain (1e-5,
    0.1 dB); a running AGC inside the first half second of a stream (TOL_AGC_STARTUP, 5e-5: its detector remembers the band-pass's fp32
    floor); the noise filter on identical input to 1e-6 and against the oracle chain to 5e-3, the first 300 samples to 1e-5 of the peak
    (test_noise_filter_anf: the algorithm is ill-conditioned on band-limited input)"""
    import pebblesdr_amd as P
    from tests.test_parity_gpu import TOL_AGC_STARTUP
    fs, fc = 48000, -4000.0

    def pair(bins=0):
        rx = P.ReceiverBank(fs, 1, True, False, bins, max_superframes=2)
        ref = oracle_mod.Receiver(fs, N, bins)
        rx.set_mode(0, P.DM_USB); rx.set_mixer(0, fc); rx.set_bandpass(0, 300, 3000)
        ref.set_mode(oracle_mod.USB); ref.set_mixer(fc); ref.set_filter(300, 3000)
        return rx, ref

    def run(rx, ref, x, spectrum):
        outs = [rx.process(x[lo * N:hi * N]) for lo, hi in ((0, 1), (1, 3), (3, 5), (5, 6))]
        g = np.concatenate([o[0] for o in outs], axis=1)[0]
        gs = np.concatenate([o[1] for o in outs], axis=1)[0] if spectrum else None
        r = [ref.process(x[f * N:(f + 1) * N], want_spectrum=spectrum) for f in range(6)]
        assert rx.kernel_name(2) == route
        return g, gs, np.concatenate([a for a, _ in r]), [s for _, s in r]

    # DCRemoval, IQBalance, both noise blankers, ahead of the spectrum and the mixer
    rx, ref = pair(BINS)
    rx.set_conditioners(0, 15, 1.02, 0.03); ref.set_conditioners(15, 1.02, 0.03)
    x = tones(fs, 6 * N, [(0.05, fc + 1000.0), (0.02, 9000.0)]) + lcg_noise(6 * N, 5, 1e-3) + 0.01
    x[500] += 2.0; x[7000:7003] += 1.5j; x[9000] -= 3.0
    g, gs, r, rs = run(rx, ref, x, True)
    assert rel_rms(g, r) <= TOL
    for f in range(1, 6):
        assert db_err(gs[f], rs[f]) <= TOL_DB, f
    rx.close()
    # AGC::processBlock behind the band-pass
    rx, ref = pair()
    rx.set_agc(0, 2, 30); ref.set_agc(2, 30)
    t = np.arange(6 * N) / fs
    x = (0.02 + 0.3 * (np.sin(2 * np.pi * 9.0 * t) > 0)) * np.exp(2j * np.pi * (fc + 1000.0) * t) + lcg_noise(6 * N, 3, 1e-4)
    g, _, r, _ = run(rx, ref, x, False)
    e = rel_rms(g, r)
    print("AGC: rel-RMS %.3e" % e)
    assert e <= TOL_AGC_STARTUP
    rx.close()
    # NoiseFilter (ANF)
    a, ref = pair()
    b, _ = pair()
    a.set_noise_filter(0, True); ref.set_anf(True)
    x = tones(fs, 6 * N, [(0.05, fc + 1000.0), (0.03, fc + 2200.0)]) + lcg_noise(6 * N, 5, 1e-2)
    ga, _, r, _ = run(a, ref, x, False)
    gb = np.concatenate([b.process(x[lo * N:hi * N])[0] for lo, hi in ((0, 1), (1, 3), (3, 5), (5, 6))], axis=1)[0]
    assert rel_rms(ga, oracle_mod.Anf().process(gb.astype(np.complex128))) <= 1e-6
    assert rel_rms(ga, r) <= 5e-3
    assert np.abs(ga[:300] - r[:300]).max() <= 1e-5 * np.abs(r).max()
    a.close()
    b.close()


def test_audio_and_recording_rings(gpu_lib, route):
    """the audio output stage and IQ recording through their pinned slots: every call's blocks are the host twins' conversion of that
    call's audio rows and of its input"""
    import pebblesdr_amd as P
    fs, C = 48000, 2
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
    for c, fc in enumerate((-4000.0, 6000.0)):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fc); rx.set_bandpass(c, 300, 3000)
    rx.audio_out_open(P.AUDIO_F32, None, 4)
    rx.record_open(4)
    x = (sum(mode_signal("USB", fs, 3 * N, fc, seed=90 + c) for c, fc in enumerate((-4000.0, 6000.0))) * 3.0).astype(np.complex64)
    for k, (lo, hi) in enumerate(((0, 1), (1, 3))):
        audio = rx.process(x[lo * N:hi * N])[0]
        idx, dropped, blk = rx.audio_out_next(True)
        rx.audio_out_release(idx)
        assert (idx, dropped) == (k, 0) and np.abs(audio).max() > 1e-2
        assert np.array_equal(blk, np.stack([P.audio_out_convert(P.AUDIO_F32, 100.0, False, audio[c]) for c in range(C)])), k
        idx, dropped, rec = rx.record_next(True)
        rx.record_release(idx)
        assert (idx, dropped) == (k, 0)
        assert np.array_equal(rec, np.stack([P.iq_record_convert(x[lo * N:hi * N])])), k
    assert rx.kernel_name(2) == route
    rx.audio_out_close()
    rx.record_close()
    rx.close()
