"""GPU tier (-m gpu): FFT::mapFFTToScreen on the device (k_screen_map) against the numpy restatement (tests/screen_map_ref.py).

Parity bar: the device's int32 plot heights equal the restatement's on every pixel fed the device's own float dB.  The one
exception is an averaged pixel whose unrounded value v (10 log10 of the mean power minus maxdB) lies within 1e-9 max(1, |v|) of an
integer: there the height computed from the neighbouring powerdB is accepted too (summation order, and the device's exp10 / log10
against glibc's pow / log10).  Each check reports how many pixels used it.
"""
import math

import numpy as np
import pytest

from tests import screen_map_ref as R
from tests.signals import lcg_noise, tones

pytestmark = pytest.mark.gpu

E_INVALID = -1


def check(dev, db, fft, fs, y, x, max_db, min_db, start, stop, what=""):
    """dev [..., x] against the restatement of the float dB rows db [..., fft]; returns the count of tolerated pixels"""
    want, v, alt = R.map_fft_to_screen(np.asarray(db, dtype=np.float32), fft, fs, y, x, max_db, min_db, start, stop)
    dev = np.asarray(dev)
    assert dev.shape == want.shape, what
    ok = (dev == want) | (dev == alt)
    if not ok.all():
        k = np.argwhere(~ok)[0]
        raise AssertionError("%s: %d pixels differ, first at %s: device %d, restatement %d (v %r)"
                             % (what, int((~ok).sum()), tuple(k), dev[tuple(k)], want[tuple(k)], v[tuple(k)]))
    n_alt = int(((dev != want) & (dev == alt)).sum())
    if n_alt:
        print("%s: %d of %d pixels at an integer boundary took the neighbouring powerdB" % (what, n_alt, dev.size))
    return n_alt


def spectrum_signal(fs, n, seed):
    return tones(fs, n, [(0.3, 0.11 * fs), (0.02, -0.23 * fs), (3e-4, 0.31 * fs)]) + lcg_noise(n, seed, 1e-3)


def ranges(fs):
    h = int(fs // 2)
    return [(-h, h),                             # whole spectrum
            (-h // 10, h // 8),                  # zoomed in
            (int(-fs), int(0.8 * fs)),           # zoomed out: both edges outside
            (int(fs), int(2 * fs)),              # wholly above
            (int(-1.5 * fs), int(-0.6 * fs)),    # wholly below
            (h // 3, -h // 4)]                   # start above stop


# (a) the stand-alone spectrum step over a grid of plot geometries
@pytest.mark.parametrize("bins", [2048, 4096, 8192])
def test_spectrum_step_map_grid(gpu_lib, bins):
    import pebblesdr_amd as P
    used = 0
    for fs in (2.048e6, 100e6):
        sp = P.Spectrum(bins, fs, 2048)
        x = spectrum_signal(fs, 2 * 2048, 11)
        sp.fftSpectrum(x[:2048])
        db, _ = sp.fftSpectrum(x[2048:])
        for start, stop in ranges(fs):
            for xp in (1, 333, 1024, 4096):
                for yp in (255, 600):
                    for mx in (0.0, -10.0):
                        got = sp.mapFFTToScreen(yp, xp, mx, -120.0, start, stop)
                        used += check(got, db, bins, fs, yp, xp, mx, -120.0, start, stop, "bins %d fs %g %d..%d x %d y %d max %g"
                                      % (bins, fs, start, stop, xp, yp, mx))
        assert R.geometry(bins, fs, -int(fs // 2), int(fs // 2), 333)["averaged"]          # both branches are in the grid
        assert not R.geometry(bins, fs, -int(fs // 2) // 10, int(fs // 2) // 8, 4096)["averaged"]
        sp.close()
    print("bins %d: %d tolerated pixels" % (bins, used))


# (b) a receiver at configs[1] geometry: 20 Msps, 8192 bins, one call of 256 super-frames (16384 frames)
def test_receiver_map_every_frame_of_a_configs1_call(gpu_lib):
    import pebblesdr_amd as P
    fs, bins, K = 20_000_000, 8192, 256
    rx = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=K)
    rx.set_mixer(0, 1.0e6)
    n = K * rx.superframe
    t = np.arange(n) / fs
    x = (0.4 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(n, 5, 1e-3)).astype(np.complex64)
    del t
    buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x), 0)
    del x
    try:
        rx.process_device(buf.ptr, n)
        spec = rx.spectrum()
        F = spec.shape[1]
        assert F == 16384
        allf = rx.map_spectrum(255, 1024, 0.0, -120.0, -fs // 2, fs // 2, first_frame=0)
        assert allf.shape == (1, F, 1024)
        check(allf[0], spec[0], bins, float(fs), 255, 1024, 0.0, -120.0, -fs // 2, fs // 2, "configs[1] every frame")
        sub = rx.map_spectrum(255, 1024, 0.0, -120.0, -fs // 2, fs // 2, first_frame=3, n_frames=(F - 3 + 6) // 7, frame_step=7)
        assert np.array_equal(sub[0], allf[0, 3::7])
        last = rx.map_spectrum(600, 1000, -10.0, -120.0, -3_000_000, 4_000_000)
        check(last[0, 0], spec[0, -1], bins, float(fs), 600, 1000, -10.0, -120.0, -3_000_000, 4_000_000, "configs[1] last frame")
    finally:
        buf.free()
        rx.close()


# (c) zoomed spectra of an NFM bank, per-channel mode offsets, repeat branch (and the quint16 span wrap)
def test_zoom_map_of_an_nfm_bank_with_mode_offsets(gpu_lib):
    import pebblesdr_amd as P
    fs, C = 2048000, 4
    fcs = [100e3, -250e3, 400e3, -30e3]
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2, hires_bins=2048)
    for c in range(C):
        rx.set_mixer(c, fcs[c])
        rx.set_mode(c, P.DM_FMN)
        rx.set_bandpass(c, -7500, 7500)
    rate = int(rx.info.demod_rate_int)
    n = 2 * rx.superframe
    x = tones(fs, n, [(0.2, f + 1500.0) for f in fcs]) + lcg_noise(n, 8, 1e-3)
    rx.process(x)
    Z = rx.zoom_spectrum()
    offs = [0, 500, -700, 1234]
    for zoom in (1.0, 0.25, 65536.0 / rate + 0.5):
        span = int(rate * zoom)
        got = rx.map_zoom_spectrum(600, 4096, 0.0, -120.0, zoom, offs, first_frame=0)
        assert got.shape == (C, Z.shape[1], 4096)
        for c in range(C):
            start, stop = R.zoom_edges(rate, zoom, offs[c])
            if span < 65536:
                assert (start, stop) == (-(span // 2) - offs[c], span // 2 - offs[c])
            g = R.geometry(2048, float(rate), start, stop, 4096)
            assert not g["averaged"]
            check(got[c], Z[c], 2048, float(rate), 600, 4096, 0.0, -120.0, start, stop, "zoom %g channel %d" % (zoom, c))
    same = rx.map_zoom_spectrum(255, 512, 0.0, -120.0, 1.0, None)  # NULL offsets: 0 for every channel
    for c in range(C):
        start, stop = R.zoom_edges(rate, 1.0, 0)
        check(same[c, 0], Z[c, -1], 2048, float(rate), 255, 512, 0.0, -120.0, start, stop, "zoom 1, no offsets, channel %d" % c)
    rx.close()


# (d) a stream bank at 128 x 4 frames x 65536 bins: the last frame of each stream
def test_streambank_map_last_frames(gpu_lib):
    import pebblesdr_amd as P
    fs, S, N, F = 200e6, 128, 65536, 4
    sb = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=F)
    base = spectrum_signal(fs, F * N, 21).astype(np.complex64)
    x = np.stack([base * np.complex64(np.exp(2j * np.pi * s / S)) * np.float32(0.5 + s / (2 * S)) for s in range(S)])
    buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x), 0)
    try:
        sb.process_device(buf.ptr, F * N, 2)
        spec = sb.spectrum()
        got = sb.map_spectrum(255, 1024, 0.0, -120.0, -100_000_000, 100_000_000)
        assert got.shape == (S, 1, 1024)
        check(got[:, 0], spec[:, -1], N, fs, 255, 1024, 0.0, -120.0, -100_000_000, 100_000_000, "stream bank last frames")
        two = sb.map_spectrum(600, 333, -10.0, -120.0, -20_000_000, 35_000_000, first_frame=1, n_frames=2, frame_step=2)
        check(two, spec[:, 1::2], N, fs, 600, 333, -10.0, -120.0, -20_000_000, 35_000_000, "stream bank frames 1, 3")
    finally:
        buf.free()
        sb.close()


# (e) process -> map -> process -> map with no host wait: each map sees its own call's spectrum
@pytest.mark.parametrize("pipeline", [False, True])
def test_maps_between_calls_without_a_host_wait(gpu_lib, monkeypatch, pipeline):
    import pebblesdr_amd as P
    fs, bins = 20_000_000, 8192
    if pipeline:
        monkeypatch.setenv("PEBBLEGPU_PIPELINE", "1")
    a = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=2, hires_bins=2048)
    monkeypatch.delenv("PEBBLEGPU_PIPELINE", raising=False)
    b = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=2, hires_bins=2048)
    n = 2 * a.superframe
    K = 5
    t = np.arange(K * n) / fs
    x = (0.4 * np.exp(1j * (2 * np.pi * (1.0e6 + 2e5 * np.floor(t * fs / n)) * t)) + lcg_noise(K * n, 13, 1e-2)).astype(np.complex64)
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(x[k * n:(k + 1) * n]), 0) for k in range(K)]
    F = n // 2048
    W, ZW = 1024, 700
    outs = [P.DeviceBuffer(4 * F * W, 0) for _ in range(K)]
    zouts = [P.DeviceBuffer(4 * 8 * ZW, 0) for _ in range(K)]
    try:
        want, zwant = [], []
        for k in range(K):
            if k == 3:
                b.set_mixer(0, 1.0e6)
            b.process_device(bufs[k].ptr, n)
            b.synchronize()
            want.append(b.map_spectrum(255, W, 0.0, -120.0, -fs // 2, fs // 2, first_frame=0))
            zf = b.zoom_spectrum().shape[1]
            zwant.append(b.map_zoom_spectrum(255, ZW, 0.0, -120.0, 0.5, None, first_frame=0, n_frames=zf))
        for k in range(K):  # nothing waits on the host between these
            if k == 3:
                a.set_mixer(0, 1.0e6)
            a.process_device(bufs[k].ptr, n)
            a.map_spectrum_device(outs[k].ptr, 255, W, 0.0, -120.0, -fs // 2, fs // 2, 0, F)
            a.map_zoom_spectrum_device(zouts[k].ptr, 255, ZW, 0.0, -120.0, 0.5, None, 0, zwant[k].shape[1])
        a.synchronize()
        for k in range(K):
            got = outs[k].download(np.int32, F * W).reshape(1, F, W)
            assert np.array_equal(got, want[k]), "call %d" % k
            zn = zwant[k].size
            assert np.array_equal(zouts[k].download(np.int32, zn).reshape(zwant[k].shape), zwant[k]), "zoom, call %d" % k
        assert len({w.tobytes() for w in want}) == K  # the calls' spectra differ: a stale read would show
    finally:
        for bf in bufs + outs + zouts:
            bf.free()
        a.close()
        b.close()


# (f) refusals: each returns its code before anything is queued, and the handle keeps working
def test_refusals_leave_the_handle_usable(gpu_lib):
    import pebblesdr_amd as P
    fs = 2048000
    rx = P.ReceiverBank(fs, 1, True, False, 4096, max_superframes=1)
    out = P.DeviceBuffer(4 * 64 * 1024, 0)

    def refused(fn, *a, **k):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*a, **k)
        assert e.value.code == E_INVALID, e.value

    try:
        refused(rx.map_spectrum_device, out.ptr, 255, 1024, 0.0, -120.0, -fs // 2, fs // 2, 0, 1)   # no call yet
        refused(rx.map_zoom_spectrum_device, out.ptr, 255, 1024, 0.0, -120.0, 1.0, None, 0, 1)     # no zoomed spectrum
        x = spectrum_signal(fs, rx.superframe, 3)
        rx.process(x)
        F = rx.spectrum().shape[1]
        refused(rx.map_spectrum_device, out.ptr, 255, 0, 0.0, -120.0, -fs // 2, fs // 2, 0, 1)
        refused(rx.map_spectrum_device, out.ptr, 0, 1024, 0.0, -120.0, -fs // 2, fs // 2, 0, 1)
        refused(rx.map_spectrum_device, out.ptr, 255, 1024, -50.0, -50.0, -fs // 2, fs // 2, 0, 1)
        refused(rx.map_spectrum_device, out.ptr, 255, 1024, 0.0, -120.0, -fs // 2, fs // 2, F, 1)
        refused(rx.map_spectrum_device, out.ptr, 255, 1024, 0.0, -120.0, -fs // 2, fs // 2, 0, F + 1)
        refused(rx.map_spectrum_device, out.ptr, 255, 1024, 0.0, -120.0, -fs // 2, fs // 2, 1, 2, F - 1)
        refused(rx.map_spectrum_device, out.ptr, 255, 1024, 0.0, -120.0, -fs // 2, fs // 2, 0, 0)
        m = P.screen_map(255, 1024, 0.0, -120.0, -fs // 2, fs // 2)
        m.struct_size = 8
        assert rx.L.pebblegpu_receiver_map_spectrum(rx.h, m, 0, 1, 1, out.ptr) == E_INVALID
        # still usable: a call and its map
        a2, _ = rx.process(x)
        got = rx.map_spectrum(255, 1024, 0.0, -120.0, -fs // 2, fs // 2, first_frame=0)
        check(got[0], rx.spectrum()[0], 4096, float(fs), 255, 1024, 0.0, -120.0, -fs // 2, fs // 2, "after the refusals")
    finally:
        out.free()
        rx.close()
    nos = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=1)  # no spectrum at all
    try:
        nos.process(spectrum_signal(fs, nos.superframe, 4))
        o = P.DeviceBuffer(4 * 1024, 0)
        refused(nos.map_spectrum_device, o.ptr, 255, 1024, 0.0, -120.0, -fs // 2, fs // 2, 0, 1)
        o.free()
    finally:
        nos.close()
    sb = P.StreamBank(2.0e6, 2, frame=2048, spectrum_bins=4096, max_frames=2)
    try:
        o = P.DeviceBuffer(4 * 2 * 2 * 512, 0)
        refused(sb.map_spectrum_device, o.ptr, 255, 512, 0.0, -120.0, -10**6, 10**6, 0, 1)  # no call yet
        xs = np.stack([spectrum_signal(2.0e6, 4096, 30 + s) for s in range(2)])
        sb.process(xs, what=1)
        refused(sb.map_spectrum_device, o.ptr, 255, 512, 0.0, -120.0, -10**6, 10**6, 0, 1)  # the last call computed no spectrum
        _, spec = sb.process(xs, what=2)
        refused(sb.map_spectrum_device, o.ptr, 255, 512, 1.0, 1.0, -10**6, 10**6, 0, 1)
        refused(sb.map_spectrum_device, o.ptr, 255, 512, 0.0, -120.0, -10**6, 10**6, 2, 1)
        got = sb.map_spectrum(255, 512, 0.0, -120.0, -10**6, 10**6, first_frame=0)
        check(got, spec, 4096, 2.0e6, 255, 512, 0.0, -120.0, -10**6, 10**6, "stream bank after the refusals")
        o.free()
    finally:
        sb.close()
    sp = P.Spectrum(4096, 2.0e6, 2048)
    with pytest.raises(P.PebbleGpuError) as e:
        sp.mapFFTToScreen(255, 512, 0.0, -120.0, -10**6, 10**6)  # no fftSpectrum yet
    assert e.value.code == E_INVALID
    db, _ = sp.fftSpectrum(spectrum_signal(2.0e6, 2048, 5))
    check(sp.mapFFTToScreen(255, 512, 0.0, -120.0, -10**6, 10**6), db, 4096, 2.0e6, 255, 512, 0.0, -120.0, -10**6, 10**6, "step")
    sp.close()


# (g) end to end: the device map of the device spectrum against the restatement of the oracle's double spectrum
def test_map_of_the_device_spectrum_against_the_oracle(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    fs, bins, n = 20e6, 8192, 2048
    sp, ref = P.Spectrum(bins, fs, n), oracle_mod.Spectrum(bins, n)
    x = spectrum_signal(fs, 6 * n, 17)
    worst = 0
    for f in range(6):
        db, _ = sp.fftSpectrum(x[f * n:(f + 1) * n])
        rdb = ref.process(x[f * n:(f + 1) * n])
        if f == 0:
            continue
        m = rdb > -110  # the spectrum's own bar (tests/test_parity_gpu.py)
        assert np.abs(db - rdb)[m].max() <= 0.1
        for (start, stop) in ranges(fs)[:3]:
            for yp, mx, xp in ((255, 0.0, 1024), (600, -10.0, 333), (600, 0.0, 4096)):
                got = sp.mapFFTToScreen(yp, xp, mx, -120.0, start, stop)
                want, _, _ = R.map_fft_to_screen(rdb, bins, fs, yp, xp, mx, -120.0, start, stop)
                bound = math.ceil(abs(float(R.y_scale(yp, mx, -120.0)))) + 1
                d = int(np.abs(got.astype(np.int64) - want).max())
                worst = max(worst, d)
                assert d <= bound, (f, start, stop, yp, xp, d, bound)
    print("largest pixel difference against the oracle's spectrum: %d" % worst)
    sp.close()
