"""GPU tier (-m gpu): the spectrum's update gate (pebblegpu_set_spectrum_updates) against the unchanged oracle.

Which frames get a spectrum: tests/spectrum_gate_ref.py (the reference's rule on the stream's sample clock).  What the spectra are:
oracle.Spectrum fed ONLY the selected frames, in order (FFT::fftSpectrum averages with the previous frame it was given, which behind
SignalSpectrum's timer is the previous selected frame).  Bar: test_parity_gpu.py's 0.1 dB over bins the oracle puts above -110 dB,
the first computed row excluded ("Spectrum frame 0").  Audio must be bit-identical to a handle without the gate.
"""
import numpy as np
import pytest

from tests import screen_map_ref as R
from tests.signals import lcg_noise, tones
from tests.spectrum_gate_ref import GateTimer, LatestRow
from tests.test_parity_gpu import TOL_DB, db_err

pytestmark = pytest.mark.gpu


def run_calls(rx, x, calls, timer, nf):
    """process x in calls (lengths in super-frames) -> (audio [C, n], rows [S, n_sel, bins], global frame numbers, per-call row counts)"""
    sf = rx.superframe
    audio, rows, frames, counts = [], [], [], []
    lo = 0
    for k in calls:
        a, s = rx.process(x[..., lo:lo + k * sf])
        idx = rx.spectrum_frames()
        want = timer.call(k * sf // nf)
        assert list(idx) == want, "call at sample %d: frames %s, model %s" % (lo, list(idx), want)
        assert s.shape[1] == len(want)
        audio.append(a); rows.append(s); counts.append(len(want))
        frames += [lo // nf + i for i in want]
        lo += k * sf
    return np.concatenate(audio, axis=1), np.concatenate(rows, axis=1), frames, counts


def oracle_rows(oracle_mod, x, frames, bins, nf):
    sp = oracle_mod.Spectrum(bins, nf)
    return np.array([sp.process(x[f * nf:(f + 1) * nf]) for f in frames])


def narrow_bank(P, fs, C, bins, nf=2048, max_sf=4, **kw):
    rx = P.ReceiverBank(fs, C, True, False, bins, frames_per_buffer=nf, max_superframes=max_sf, **kw)
    fcs = [100e3, -300e3, 250e3][:C]
    for c in range(C):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000)
    return rx, fcs


def test_selected_frames_follow_the_model_over_calls_of_mixed_lengths(gpu_lib):
    import pebblesdr_amd as P
    fs, nf = 2048000, 2048
    rx, fcs = narrow_bank(P, fs, 1, 4096)
    sf = rx.superframe
    calls = [1, 3, 2, 4, 1, 1, 2]
    x = tones(fs, sum(calls) * sf, [(0.05, fcs[0] + 1000.0)]) + lcg_noise(sum(calls) * sf, 3, 1e-3)
    t = GateTimer(nf, fs)
    for ups, part in ((10, calls[:4]), (40, calls[4:])):   # the rate changes mid-stream: the timer runs on
        rx.set_spectrum_updates(ups); t.set_updates(ups)
        _, rows, frames, counts = run_calls(rx, x, part, t, nf)
        x = x[sum(part) * sf:]
        assert len(frames) >= 2 and rx.kernel_name(1) == "k_spectrum_list_q128"
    # back to the default: every frame again
    rx.set_spectrum_updates(P.SPECTRUM_EVERY_FRAME)
    rx2, _ = narrow_bank(P, fs, 1, 4096)
    y = tones(fs, sf, [(0.05, fcs[0] + 1000.0)])
    _, s = rx.process(y)
    assert s.shape[1] == sf // nf and list(rx.spectrum_frames()) == list(range(sf // nf))
    assert list(rx2.spectrum_frames()) == []   # no call yet
    rx.close(); rx2.close()


@pytest.mark.parametrize("nf,bins", [(2048, 2048), (2048, 4096), (2048, 8192), (2048, 16384), (4096, 8192), (1024, 2048)])
def test_gated_spectra_against_the_oracle_and_audio_bit_identical(gpu_lib, oracle_mod, nf, bins):
    """a narrow bank of two channels off one stream, calls of 2, 1 and 3 super-frames (the two- and three-super-frame calls included)"""
    import pebblesdr_amd as P
    fs, C = 2048000, 2
    rx, fcs = narrow_bank(P, fs, C, bins, nf)
    plain, _ = narrow_bank(P, fs, C, bins, nf)
    sf = rx.superframe
    calls = [2, 1, 3, 2]
    N = sum(calls) * sf
    x = tones(fs, N, [(0.05, fcs[0] + 1000.0), (0.01, fcs[1] + 2000.0), (0.2, 0.31 * fs)]) + lcg_noise(N, 3, 1e-3)
    ups = 60 if nf >= 2048 else 120     # a spectrum every 16 (8) ms
    rx.set_spectrum_updates(ups)
    t = GateTimer(nf, fs); t.set_updates(ups)
    audio, rows, frames, _ = run_calls(rx, x, calls, t, nf)
    assert len(frames) >= 6 and frames[0] > 0
    ref = oracle_rows(oracle_mod, x, frames, bins, nf)
    assert rows.shape == (1,) + ref.shape
    worst = max(db_err(rows[0, i], ref[i]) for i in range(1, len(frames)))
    print("nf %d bins %d: %d gated rows, max |dB| %.4f" % (nf, bins, len(frames), worst))
    assert worst <= TOL_DB
    lo = 0
    for k in calls:
        a, _ = plain.process(x[lo:lo + k * sf])
        assert np.array_equal(a, audio[:, lo // rx.D:(lo + k * sf) // rx.D])
        lo += k * sf
    rx.close(); plain.close()


def test_gated_one_channel_wfm_8192_and_raw_input(gpu_lib, oracle_mod):
    """the headline shape (20 Msps, one WFM channel, 8192 bins): float2 input and HackRF int8 pairs through process_raw (the chain's
    first stage and the listed-frame transform both convert in their own loads); audio bit-identical to handles without the gate"""
    import pebblesdr_amd as P
    fs, nf, bins = 20_000_000, 2048, 8192
    calls = [1, 2, 4, 1]
    mk = lambda: P.ReceiverBank(fs, 1, True, True, bins, max_superframes=4)
    rx, plain, rxr, plainr = mk(), mk(), mk(), mk()
    for r in (rx, plain, rxr, plainr):
        r.set_mixer(0, 1.0e6)
    sf = rx.superframe
    N = sum(calls) * sf
    tt = np.arange(N) / fs
    x = 0.5 * np.exp(1j * (2 * np.pi * 1.0e6 * tt + 75.0 * np.sin(2 * np.pi * 1000 * tt))) + lcg_noise(N, 2, 1e-2)
    raw8 = np.clip(np.stack([np.round(x.real * 128), np.round(x.imag * 128)], axis=-1), -128, 127).astype(np.int8)
    x = (raw8[:, 0].astype(np.float64) + 1j * raw8[:, 1].astype(np.float64)) / 128.0
    ups = 1000   # period 1 ms: every 10th frame
    rx.set_spectrum_updates(ups); rxr.set_spectrum_updates(ups)
    t = GateTimer(nf, fs); t.set_updates(ups)
    audio, rows, frames, counts = run_calls(rx, x, calls, t, nf)
    assert frames[:3] == [10, 20, 30] and len(frames) >= 40
    ref = oracle_rows(oracle_mod, x, frames, bins, nf)
    assert max(db_err(rows[0, i], ref[i]) for i in range(1, len(frames))) <= TOL_DB
    # raw route
    raw_rows, raw_audio, plain_audio, lo = [], [], [], 0
    for k, cnt in zip(calls, counts):
        seg = np.ascontiguousarray(raw8[lo:lo + k * sf])
        buf = P.DeviceBuffer.from_array(seg, 0)
        try:
            rxr.process_raw_device(buf.ptr, k * sf, 0, 0, 1.0)
            raw_audio.append(rxr.audio()); s = rxr.spectrum()
            assert s.shape[1] == cnt
            raw_rows.append(s)
            plainr.process_raw_device(buf.ptr, k * sf, 0, 0, 1.0)
            plain_audio.append(plainr.audio())
        finally:
            buf.free()
        a, _ = plain.process(x[lo:lo + k * sf])
        assert np.array_equal(a, audio[:, lo // rx.D:(lo + k * sf) // rx.D])
        lo += k * sf
    raw_rows = np.concatenate(raw_rows, axis=1)
    assert max(db_err(raw_rows[0, i], ref[i]) for i in range(1, len(frames))) <= TOL_DB
    assert np.array_equal(np.concatenate(raw_audio, axis=1), np.concatenate(plain_audio, axis=1))
    for r in (rx, plain, rxr, plainr):
        r.close()


def test_gated_zoomed_spectrum_of_a_narrow_bank(gpu_lib, oracle_mod):
    """the zoomed spectrum's own timer counts decimated frames at the demodulator rate"""
    import pebblesdr_amd as P
    fs, n, C = 2048000, 2048, 2
    fcs = [150e3, -320e3]
    mk = lambda: P.ReceiverBank(fs, C, True, False, 0, max_superframes=4, hires_bins=2048)
    rx, plain = mk(), mk()
    for r in (rx, plain):
        for c in range(C):
            r.set_mixer(c, fcs[c]); r.set_mode(c, P.DM_USB); r.set_bandpass(c, 300, 3000)
    sf = rx.superframe
    calls = [3, 1, 4, 4, 2]
    N = sum(calls) * sf
    x = tones(fs, N, [(0.2, fcs[0] + 1234.5), (0.02, fcs[0] - 7000.0), (0.1, fcs[1] + 2500.0)]) + lcg_noise(N, 4, 1e-3)
    rate = int(rx.info.demod_rate_int)
    ups = 10
    rx.set_spectrum_updates(ups)
    t = GateTimer(n, rate); t.set_updates(ups)
    Z, frames, lo = [], [], 0
    for k in calls:
        a, _ = rx.process(x[lo:lo + k * sf])
        z = rx.zoom_spectrum()
        nd = k * sf // rx.D // n
        want = t.call(nd)
        assert list(rx.spectrum_frames(zoomed=True)) == want and z.shape[1] == len(want)
        frames += [lo // rx.D // n + i for i in want]
        Z.append(z)
        b, _ = plain.process(x[lo:lo + k * sf])
        assert np.array_equal(a, b)
        lo += k * sf
    Z = np.concatenate(Z, axis=1)
    assert len(frames) >= 3
    stages = sum(int(np.log2(st)) for _, st in rx.chain())
    gain = 10 ** (2 * stages / 20.0)
    for c in range(C):
        mix = oracle_mod.Mixer(fs); mix.set_frequency(fcs[c])
        dec = oracle_mod.Decimator(fs, 30000)
        z = np.concatenate([dec.process(mix.process(x[i:i + 8192])) for i in range(0, N, 8192)]) * gain
        ref = oracle_rows(oracle_mod, z, frames, 2048, n)
        for i in range(1, len(frames)):
            assert db_err(Z[c][i], ref[i]) <= TOL_DB, "channel %d row %d" % (c, i)
    rx.close(); plain.close()


def test_zero_updates_compute_nothing_and_leave_the_audio_alone(gpu_lib):
    import pebblesdr_amd as P
    fs = 2048000
    rx, fcs = narrow_bank(P, fs, 2, 4096, hires_bins=2048)
    plain, _ = narrow_bank(P, fs, 2, 4096, hires_bins=2048)
    sf = rx.superframe
    x = tones(fs, 5 * sf, [(0.05, fcs[0] + 1000.0), (0.01, fcs[1] + 2000.0)]) + lcg_noise(5 * sf, 3, 1e-3)
    rx.set_spectrum_updates(0)
    rx.enable_signal_strength(True)
    lo = 0
    for k in (2, 3):
        a, s = rx.process(x[lo:lo + k * sf])
        assert s.shape == (1, 0, 4096) and rx.zoom_spectrum().shape[1] == 0 and rx.signal_strength().shape[1] == 0
        assert len(rx.spectrum_frames()) == 0 and len(rx.spectrum_frames(zoomed=True)) == 0
        b, _ = plain.process(x[lo:lo + k * sf])
        assert np.array_equal(a, b)
        lo += k * sf
    # a call with no selected frame and no spectrum yet leaves the handle usable: maps are refused, the next calls run
    with pytest.raises(P.PebbleGpuError):
        rx.map_spectrum(255, 512, 0.0, -120.0, -fs // 2, fs // 2)
    rx.set_squelch(0, -60.0)                  # no spectrum exists: the gate stays open
    a, _ = rx.process(x[:sf])
    assert a[0].any()
    rx.set_spectrum_updates(100)
    a, s = rx.process(x[:2 * sf])
    assert s.shape[1] == len(rx.spectrum_frames()) > 0
    rx.close(); plain.close()


def test_s_meter_rows_of_the_gated_spectra(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    fs, nf, bins, C = 2048000, 2048, 4096, 2
    rx, fcs = narrow_bank(P, fs, C, bins)
    rx.enable_signal_strength(True)
    rx.set_spectrum_updates(50)
    t = GateTimer(nf, fs); t.set_updates(50)
    sf = rx.superframe
    calls = [2, 3]
    N = sum(calls) * sf
    x = tones(fs, N, [(0.05, fcs[0] + 1000.0), (0.01, fcs[1] + 2000.0)]) + lcg_noise(N, 3, 1e-3)
    frames, sm, rows, lo = [], [], [], 0
    for k in calls:
        _, s = rx.process(x[lo:lo + k * sf])
        want = t.call(k * sf // nf)
        m = rx.signal_strength()
        assert m.shape == (C, len(want), 4) and s.shape[1] == len(want)
        frames += [lo // nf + i for i in want]
        sm.append(m); rows.append(s)
        lo += k * sf
    sm, rows = np.concatenate(sm, axis=1), np.concatenate(rows, axis=1)
    ref = oracle_rows(oracle_mod, x, frames, bins, nf)
    assert len(frames) >= 4
    for i in range(len(frames)):
        for c in range(C):
            own = oracle_mod.fd_estimate(rows[0, i].astype(np.float64), fs, np.float32(300), np.float32(3000), fcs[c])
            assert np.abs(sm[c, i] - own).max() <= 1e-4
            if i:
                assert np.abs(sm[c, i] - oracle_mod.fd_estimate(ref[i], fs, np.float32(300), np.float32(3000), fcs[c])).max() <= TOL_DB
    rx.close()


def _keyed(fs, N, nf, fcs, off_frames, amp=0.1):
    """carriers that vanish for good at frame off_frames[c]"""
    t = np.arange(N) / fs
    x = lcg_noise(N, 9, 1e-5)
    for fc, off in zip(fcs, off_frames):
        x = x + (np.arange(N) < off * nf) * amp * np.exp(2j * np.pi * (fc + 1300.0) * t)
    return x


def _squelch_model(oracle_mod, x, fs, nf, bins, ups, K, fps, fcs, thr):
    """open/closed per (channel, super-frame) from the oracle's spectra of the selected frames; asserts the 3 dB margin"""
    t = GateTimer(nf, fs); t.set_updates(ups)
    frames = t.call(K * fps)
    ref = oracle_rows(oracle_mod, x, frames, bins, nf)
    latest = LatestRow(); latest.add(frames)
    want = np.ones((len(fcs), K), dtype=bool)
    for c, fc in enumerate(fcs):
        if thr[c] <= -120.0:
            continue   # DB::minDb never closes the gate: no decision to model
        avg = [oracle_mod.fd_estimate(ref[i], fs, np.float32(300), np.float32(3000), fc)[1] for i in range(len(frames))]
        for j in range(K):
            k = latest.at((j + 1) * fps - 1)
            if k is None:
                continue   # no spectrum yet: open
            assert abs(avg[k] - thr[c]) >= 3.0, "channel %d super-frame %d: avgDb %.2f against %.1f" % (c, j, avg[k], thr[c])
            want[c, j] = avg[k] >= thr[c]
    return want, frames


def test_squelch_reads_the_stale_spectrum_one_channel(gpu_lib, oracle_mod):
    """the reference's own shape: a carrier that vanishes between two updates keeps the gate open until the super-frame behind the
    next update that shows its absence (getUnprocessed() holds the last computed spectrum, receiver.cpp:959-965)"""
    import pebblesdr_amd as P
    fs, nf, bins, ups, K = 2048000, 2048, 4096, 10, 20
    rx, fcs = narrow_bank(P, fs, 1, bins, max_sf=1)
    thr = [-60.0]
    rx.set_spectrum_updates(ups)
    rx.set_squelch(0, thr[0])
    sf = rx.superframe
    fps = sf // nf
    off = 250
    x = _keyed(fs, K * sf, nf, fcs, [off])
    want, frames = _squelch_model(oracle_mod, x, fs, nf, bins, ups, K, fps, fcs, thr)
    got = np.array([[len(rx.process(x[j * sf:(j + 1) * sf])[0][0]) > 0 for j in range(K)]])
    assert np.array_equal(got, want), (got, want)
    silent = [j for j in range(K) if j * fps >= off]
    assert any(want[0, j] for j in silent) and not want[0, -1], "the case must hold a stale-open and a closed super-frame"
    rx.close()


def test_squelch_reads_the_stale_spectrum_in_a_bank(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    fs, nf, bins, ups, K, C = 2048000, 2048, 4096, 10, 20, 3
    rx, fcs = narrow_bank(P, fs, C, bins, max_sf=4)
    thr = [-60.0, -55.0, -120.0]
    rx.set_spectrum_updates(ups)
    for c in range(C):
        rx.set_squelch(c, thr[c])
    sf = rx.superframe
    fps = sf // nf
    offs = [250, 130, 10]
    x = _keyed(fs, K * sf, nf, fcs, offs)
    want, frames = _squelch_model(oracle_mod, x, fs, nf, bins, ups, K, fps, fcs, thr)
    spf = sf // rx.D
    got = np.zeros((C, K), dtype=bool)
    j = 0
    for k in (3, 4, 1, 4, 4, 2, 2):
        a, _ = rx.process(x[j * sf:(j + k) * sf])
        for c in range(C):
            for i in range(k):
                got[c, j + i] = a[c, i * spf:(i + 1) * spf].any()
        j += k
    assert j == K
    assert np.array_equal(got, want), (got, want)
    for c in (0, 1):
        silent = [j for j in range(K) if j * fps >= offs[c]]
        assert any(want[c, j] for j in silent) and not want[c, -1]
    rx.close()


def test_map_spectrum_on_gated_rows(gpu_lib):
    import pebblesdr_amd as P
    fs, nf, bins = 2048000, 2048, 4096
    rx, fcs = narrow_bank(P, fs, 1, bins)
    rx.set_spectrum_updates(80)
    sf = rx.superframe
    x = tones(fs, 3 * sf, [(0.3, 0.11 * fs), (0.02, -0.23 * fs), (3e-4, 0.31 * fs)]) + lcg_noise(3 * sf, 11, 1e-3)
    _, rows = rx.process(x)
    F = rows.shape[1]
    assert F == len(rx.spectrum_frames()) >= 3
    for (yp, xp, mx, start, stop) in ((255, 1024, 0.0, -fs // 2, fs // 2), (600, 333, -10.0, -fs // 20, fs // 16), (255, 4096, 0.0, -fs // 20, fs // 16)):
        got = rx.map_spectrum(yp, xp, mx, -120.0, start, stop, first_frame=0)
        want, _, alt = R.map_fft_to_screen(rows[0], bins, float(fs), yp, xp, mx, -120.0, start, stop)
        assert got.shape == (1, F, xp)
        assert ((got[0] == want) | (got[0] == alt)).all()
        last = rx.map_spectrum(yp, xp, mx, -120.0, start, stop)
        assert np.array_equal(last[0, 0], got[0, -1])
    with pytest.raises(P.PebbleGpuError):
        rx.map_spectrum(255, 512, 0.0, -120.0, -fs // 2, fs // 2, first_frame=F, n_frames=1)   # frame numbers are row numbers
    # a call that makes no spectrum: the display maps the one it still holds (m_unprocessedSpectrum), as frame 0
    held = rx.map_spectrum(255, 1024, 0.0, -120.0, -fs // 2, fs // 2)
    rx.set_spectrum_updates(0)
    _, none = rx.process(x[:rx.superframe])
    assert none.shape[1] == 0
    assert np.array_equal(rx.map_spectrum(255, 1024, 0.0, -120.0, -fs // 2, fs // 2), held)
    rx.close()


def test_host_frame_path_hands_out_a_spectrum_only_when_one_was_made(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    fs, nf, bins = 2048000, 2048, 4096
    rx, fcs = narrow_bank(P, fs, 1, bins, max_sf=1)
    rx.set_spectrum_updates(100)
    t = GateTimer(nf, fs); t.set_updates(100)
    sf = rx.superframe
    F = 2 * sf // nf
    x = tones(fs, 2 * sf, [(0.05, fcs[0] + 1000.0)]) + lcg_noise(2 * sf, 3, 1e-3)
    spec = np.full(bins, 7.0)
    frames, kept = [], []
    for f in range(F):
        before = spec.copy()
        _, upd = rx.process_iq_updates(x[f * nf:(f + 1) * nf], spec)
        assert upd == (t.call(1) == [0])
        if upd:
            frames.append(f); kept.append(spec.copy())
        else:
            assert np.array_equal(spec, before)   # the last computed spectrum stays
    assert len(frames) >= 4
    ref = oracle_rows(oracle_mod, x, frames, bins, nf)
    for i in range(1, len(frames)):
        assert db_err(kept[i], ref[i]) <= TOL_DB
    rx.close()
