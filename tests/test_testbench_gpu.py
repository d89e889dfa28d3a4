"""GPU tier of the test bench: the generator (stand-alone and at the head of a receiver's chain) against tests/testbench_ref.py, the taps
against the oracle's steps composed in the order of Receiver::processIQData, the refusals, and the Morse modem fed from its own tap.
Bars: 1e-5 relative RMS in the time domain and 0.1 dB on spectra (tests/test_parity_gpu.py); the noise filter on identical input 1e-6 and
inside the chain 5e-3 (test_noise_filter_anf there)."""
import os
import subprocess

import numpy as np
import pytest

from tests import morse_ref as M
from tests import testbench_ref as R
from tests.signals import lcg_noise
from tests.test_morse_gpu import events_of, keyed
from tests.test_parity_gpu import TOL, TOL_DB, db_err, rel_rms

pytestmark = pytest.mark.gpu

N22 = 1 << 22
RAGGED = [1000003, 4096, 777777, 123]   # odd sizes: calls start at odd samples too (the kernel's 8-byte path)

# (fs, start, stop, rate): rate / fs = 200 Hz exactly; and two whose leg quotient has a fractional part well inside (0, 1)
SW_EXACT = (20e6, -1e6, 1e6, 4e9)
SW_20M = (20e6, -1e6, 1e6, 300000001.0)
SW_2M = (2.048e6, -0.5e6, 0.7e6, 123456789.0)


def unambiguous(sw):
    """the restatement's own leg end does not hang on a rounding: exact sums, or |stop - start| / inc well away from an integer"""
    leg, frac = R.leg_length(*sw)
    exact = (sw[3] / sw[0]).is_integer() and float(sw[1]).is_integer()
    assert (exact and frac == 0.0) or 0.01 <= frac <= 0.99, (sw, frac)
    return leg


def generate_ragged(P, gen, n, fill=None):
    """n samples from the stand-alone generator in calls of unequal sizes over one device buffer -> complex64 [n]"""
    buf = P.DeviceBuffer(8 * n)
    try:
        buf.upload(np.zeros(n, dtype=np.complex64) if fill is None else fill.astype(np.complex64))
        off, k = 0, 0
        while off < n:
            m = min(n - off, RAGGED[k % len(RAGGED)])
            gen.generate_device(buf.ptr + 8 * off, m)
            off += m
            k += 1
        gen.synchronize()
        return buf.download(np.complex64, n)
    finally:
        buf.free()


@pytest.mark.parametrize("sw,sweep_type,mix", [(SW_EXACT, R.REPEAT, False), (SW_20M, R.REPEAT_REVERSE, True), (SW_2M, R.SINGLE, False),
                                               (SW_2M, R.REPEAT, True), (SW_20M, R.REPEAT, False), (SW_EXACT, R.REPEAT_REVERSE, False)])
def test_generator_against_the_serial_restatement(gpu_lib, sw, sweep_type, mix):
    import pebblesdr_amd as P
    leg = unambiguous(sw)
    fs, a, b, rate = sw
    amp = 0.37
    ref, s = R.serial_sweep(fs, N22, 2048, amp, start=a, stop=b, rate=rate, sweep_type=sweep_type)
    assert s.resets[0] == leg and (sweep_type == R.SINGLE) == (len(s.resets) == 1)
    x = lcg_noise(N22, 11, 0.05).astype(np.complex64) if mix else None
    g = P.SigGen(fs)
    g.set_sweep(P.sweep(a, b, rate, amplitude=amp, sweep_type=sweep_type, mix=mix))
    got = generate_ragged(P, g, N22, x)
    want = ref + x.astype(np.complex128) if mix else ref
    err = rel_rms(got, want)
    print("sweep %s type %d mix %d: rel rms %.3e" % (sw, sweep_type, mix, err))
    assert err <= TOL
    # the setter is TestBench::reset: the same stretch again, now in one call
    g.set_sweep(P.sweep(a, b, rate, amplitude=amp, sweep_type=sweep_type, mix=mix))
    buf = P.DeviceBuffer.from_array(np.zeros(1 << 20, dtype=np.complex64) if x is None else x[:1 << 20])
    g.generate_device(buf.ptr, 1 << 20)
    g.synchronize()
    again = buf.download(np.complex64, 1 << 20)
    buf.free()
    assert rel_rms(again, got[:1 << 20]) <= 1e-7   # (a sample's leg table entry depends on the call it falls in: last bits may differ)
    g.close()


def test_pulse_edges_fall_on_the_restatements_samples(gpu_lib):
    import pebblesdr_amd as P
    fs, n = 2.048e6, 2 * 1024001 + 50000     # two periods and the start of a third
    kw = dict(start=-0.5e6, stop=0.7e6, rate=123456789.0, pulse_width=0.01, pulse_period=0.5)
    ref, _ = R.serial_sweep(fs, n, 2048, 1.0, sweep_type=R.REPEAT, **kw)
    g = P.SigGen(fs)
    g.set_sweep(P.sweep(kw["start"], kw["stop"], kw["rate"], amplitude=1.0, sweep_type=R.REPEAT, pulse_width_s=0.01, pulse_period_s=0.5, mix=False))
    got = generate_ragged(P, g, n)
    on_ref, on_got = np.abs(ref) > 0.5, np.abs(got) > 0.5
    assert np.array_equal(np.flatnonzero(np.diff(on_ref.astype(np.int8))), np.flatnonzero(np.diff(on_got.astype(np.int8))))
    assert np.array_equal(on_ref, on_got) and (got[~on_got] == 0).all()
    assert list(np.flatnonzero(np.diff(on_ref.astype(np.int8)))[:3]) == [20478, 1023999, 1024000 + 20479]
    assert rel_rms(got, ref) <= TOL
    g.close()


def test_host_frame_entry_point(gpu_lib):
    """pebblegpu_siggen_generate: TestBench::genSweep + genNoise on CPX frames, in place"""
    import pebblesdr_amd as P
    fs, a, b, rate = SW_2M
    g = P.SigGen(fs, 2048)
    g.set_sweep(P.sweep(a, b, rate, amplitude=0.5, mix=True))
    g.set_noise(0.01, 99)
    x = lcg_noise(8 * 2048, 5, 0.1)
    x = x.astype(np.complex64).astype(np.complex128)
    ref, _ = R.serial_sweep(fs, len(x), 2048, 0.5, start=a, stop=b, rate=rate)
    want = x + ref + 0.01 * R.noise(99, 0, 0, len(x))[0]
    got = np.concatenate([g.generate(x[k * 2048:(k + 1) * 2048].copy()) for k in range(8)])
    assert rel_rms(got, want) <= TOL
    g.close()


def test_noise_is_the_restatements(gpu_lib):
    import pebblesdr_amd as P
    fs, amp, seed = 2.048e6, 0.25, 0x1234ABCD5678
    g = P.SigGen(fs)
    g.set_noise(amp, seed)
    r, att = g.noise_draws(0, 1 << 18)
    ref, r_ref, att_ref = R.noise(seed, 0, 0, N22)
    assert np.array_equal(r, r_ref[:1 << 18]) and np.array_equal(att, att_ref[:1 << 18])
    r2, att2 = g.noise_draws(N22 - 4096, 4096)
    assert np.array_equal(r2, r_ref[-4096:]) and np.array_equal(att2, att_ref[-4096:])
    buf = P.DeviceBuffer.from_array(np.zeros(N22, dtype=np.complex64))
    g.generate_device(buf.ptr, N22)
    g.synchronize()
    one = buf.download(np.complex64, N22)
    buf.free()
    err = rel_rms(one, amp * ref)
    print("noise rel rms %.3e" % err)
    assert err <= 1e-6
    g.set_noise(amp, seed)                    # reset: the counter restarts
    ragged = generate_ragged(P, g, N22)
    assert np.array_equal(ragged.view(np.uint32), one.view(np.uint32))
    g.set_noise(amp, seed)
    g.set_stream(1)
    other = generate_ragged(P, g, 1 << 16)
    assert rel_rms(other, amp * R.noise(seed, 1, 0, 1 << 16)[0]) <= 1e-6
    assert rel_rms(other, one[:1 << 16]) > 1.0     # independent streams
    # moments: within 5 standard errors (from the restatement's own moments) of 0 and amplitude^2, per component
    for comp_ref, comp in ((ref.real, one.real.astype(np.float64)), (ref.imag, one.imag.astype(np.float64))):
        xr = amp * comp_ref
        var = xr.var()
        se_mean = np.sqrt(var / N22)
        se_var = np.sqrt((np.mean((xr - xr.mean()) ** 4) - var ** 2) / N22)
        for v in (xr, comp):
            print("noise mean %.3e (se %.3e) var %.6e (se %.3e)" % (v.mean(), se_mean, v.var(), se_var))
            assert abs(v.mean()) <= 5 * se_mean and abs(v.var() - amp ** 2) <= 5 * se_var
    g.close()


# ------------------------------------------------------------------------------------------------
# the generator at the head of a receiver
# ------------------------------------------------------------------------------------------------
def injected(fs, n_total, streams, sw, amp, noise_amp, seed):
    """what the generator adds to [streams, n_total] samples since its setters: the same sweep on every stream, noise per stream"""
    ref, _ = R.serial_sweep(fs, n_total, 2048, amp, start=sw[1], stop=sw[2], rate=sw[3], sweep_type=R.REPEAT)
    return np.stack([ref + noise_amp * R.noise(seed, s, 0, n_total)[0] for s in range(streams)])


def test_receiver_injects_into_float2_input_of_independent_streams(gpu_lib):
    import pebblesdr_amd as P
    fs = 2048000
    unambiguous(SW_2M)
    rx = P.ReceiverBank(fs, 2, False, False, 4096, max_superframes=2)
    sf = rx.superframe
    x = np.stack([lcg_noise(3 * sf, 31 + s, 0.02) for s in range(2)]).astype(np.complex64)
    rx.set_testbench_sweep(P.sweep(*SW_2M[1:], amplitude=0.2))
    rx.set_testbench_noise(0.003, 77)
    rx.set_taps([P.TAP_RAW_IQ])
    add = injected(fs, 3 * sf, 2, SW_2M, 0.2, 0.003, 77)
    for lo, hi in ((0, sf), (sf, 3 * sf)):
        seg = np.ascontiguousarray(x[:, lo:hi])
        buf = P.DeviceBuffer.from_array(seg)
        rx.process_device(buf.ptr, hi - lo)
        tap, rate = rx.tap(P.TAP_RAW_IQ)
        assert np.array_equal(buf.download(np.complex64, seg.size).reshape(seg.shape), seg)   # the caller's buffer is never written
        buf.free()
        assert rate == fs and tap.shape == (2, hi - lo)
        assert rx.kernel_name(2).startswith("k_testbench + ")
        for s in range(2):
            assert rel_rms(tap[s], x[s, lo:hi].astype(np.complex128) + add[s, lo:hi]) <= TOL, (lo, s)
    assert rel_rms(tap[0] - x[0, sf:], tap[1] - x[1, sf:]) > 1e-3      # the streams' noise differs
    rx.close()


def test_receiver_injects_into_raw_s8_input(gpu_lib):
    import pebblesdr_amd as P
    fs = 2048000
    rx = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=2)
    sf = rx.superframe
    rng = np.random.RandomState(5)
    raw = rng.randint(-20, 21, size=(2 * sf, 2)).astype(np.int8)
    rx.set_testbench_noise(0.004, 3)
    rx.set_testbench_sweep(P.sweep(*SW_2M[1:], amplitude=0.3, mix=True))   # (each setter resets both: the order does not matter)
    rx.set_taps([P.TAP_RAW_IQ])
    buf = P.DeviceBuffer.from_array(raw)
    rx.process_raw_device(buf.ptr, 2 * sf, P.binding.IQ_S8)
    tap, _ = rx.tap(P.TAP_RAW_IQ)
    conv = (raw[:, 0].astype(np.float64) + 1j * raw[:, 1]) / 128.0
    assert rel_rms(tap[0], conv + injected(fs, 2 * sf, 1, SW_2M, 0.3, 0.004, 3)[0]) <= TOL
    assert np.array_equal(buf.download(np.int8, raw.size).reshape(raw.shape), raw)   # the caller's buffer is never written
    buf.free()
    rx.close()


def test_headline_shape_with_the_generator_on(gpu_lib):
    """one WFM channel + 8192 bins at 20 Msps, raw int8 input: the call would be raw-fused side by side; with the generator on it is staged,
    and its audio and spectra are those of a generator-off receiver fed the summed stream"""
    import pebblesdr_amd as P
    fs = 20000000
    unambiguous(SW_20M)

    def make():
        r = P.ReceiverBank(fs, 1, True, True, 8192, max_superframes=2)
        r.set_mixer(0, 1.0e6)
        return r
    a, b = make(), make()
    sf = a.superframe
    n = 2 * sf
    t = np.arange(2 * n) / fs
    x = 0.4 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(2 * n, 2, 1e-3)
    raw = np.stack([np.round(x.real * 100), np.round(x.imag * 100)], axis=1).astype(np.int8)
    buf = P.DeviceBuffer.from_array(raw)
    a.process_raw_device(buf.ptr, n, P.binding.IQ_S8)             # generator off: the fused route
    assert not a.kernel_name(2).startswith("k_testbench")
    a0 = a.audio()
    a.set_testbench_sweep(P.sweep(*SW_20M[1:], amplitude=0.1))
    a.set_testbench_noise(0.002, 41)
    a.set_taps([P.TAP_RAW_IQ])
    a.process_raw_device(buf.ptr + 2 * n, n, P.binding.IQ_S8)
    assert a.kernel_name(2).startswith("k_testbench + ")
    tap, _ = a.tap(P.TAP_RAW_IQ)
    a1, s1 = a.audio(), a.spectrum()
    conv = (raw[n:, 0].astype(np.float64) + 1j * raw[n:, 1]) / 128.0
    assert rel_rms(tap[0], conv + injected(fs, n, 1, SW_20M, 0.1, 0.002, 41)[0]) <= TOL
    # the same two calls on a receiver that never had a generator, the second fed the summed stream from the host
    b.process_raw_device(buf.ptr, n, P.binding.IQ_S8)
    assert np.array_equal(b.audio(), a0)
    b1, t1 = b.process(tap)
    assert np.array_equal(a1.view(np.uint32), b1.view(np.uint32))
    assert s1.shape == t1.shape and db_err(s1[0], t1[0]) <= TOL_DB     # every frame of the call (both receivers carry the same previous frame)
    # both generators off again: bit-equal to the receiver that never had them
    a.set_testbench_sweep(None)
    a.set_testbench_noise(0.0, 0)
    a.set_taps([])
    a.process_raw_device(buf.ptr, n, P.binding.IQ_S8)
    b.process_raw_device(buf.ptr, n, P.binding.IQ_S8)
    assert not a.kernel_name(2).startswith("k_testbench") and a.tap(P.TAP_RAW_IQ) is None
    assert np.array_equal(a.audio().view(np.uint32), b.audio().view(np.uint32))
    buf.free()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------
# taps
# ------------------------------------------------------------------------------------------------
def by_frames(step, x, n=2048):
    """a step of the oracle called as the reference calls it: once per frame of n samples (the demodulators keep per-call state)"""
    return np.concatenate([step.process(x[k:k + n]) for k in range(0, len(x), n)])


def test_taps_of_a_narrow_bank_against_the_composed_oracle(gpu_lib, oracle_mod):
    """AM, USB (with the noise filter), FMN and NONE channels over three calls of two super-frames: every tap against
    oracle.Mixer -> Decimator -> gain restore -> FastFIR -> Anf -> Agc -> Demod*, and audio bit-equal with the taps off"""
    import pebblesdr_amd as P
    O = oracle_mod
    fs = 2048000
    chans = [(P.DM_AM, 100e3, -5000, 5000), (P.DM_USB, 400e3, 300, 3000), (P.DM_FMN, 300e3, -7500, 7500), (P.DM_NONE, -200e3, 300, 3000)]
    C = len(chans)

    def make(taps):
        r = P.ReceiverBank(fs, C, True, False, 0, max_superframes=2)
        for c, (mode, fc, lo, hi) in enumerate(chans):
            r.set_mode(c, mode); r.set_mixer(c, fc); r.set_bandpass(c, lo, hi)
        r.set_noise_filter(1, True)
        if taps:
            r.set_taps([P.TAP_POST_MIXER, P.TAP_POST_BP, P.TAP_MODEM, P.TAP_POST_DEMOD])
        return r
    on, off = make(True), make(False)
    sf = on.superframe
    N = 6 * sf
    t = np.arange(N) / fs
    x = (0.1 * (1 + 0.5 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * 100e3 * t)
         + 0.1 * np.exp(1j * (2 * np.pi * 300e3 * t + 2.5 * np.sin(2 * np.pi * 1000 * t)))
         + 0.05 * np.exp(2j * np.pi * (400e3 + 1500.0) * t) + 0.03 * np.exp(2j * np.pi * (400e3 + 2200.0) * t)
         + 0.05 * np.exp(2j * np.pi * (-200e3 + 1000.0) * t)) + lcg_noise(N, 6, 1e-3)
    got = {p: [] for p in (P.TAP_POST_MIXER, P.TAP_POST_BP, P.TAP_MODEM, P.TAP_POST_DEMOD)}
    audio = []
    for k in range(3):
        seg = x[2 * k * sf:2 * (k + 1) * sf]
        a_on = on.process(seg)[0]
        a_off = off.process(seg)[0]
        assert np.array_equal(a_on.view(np.uint32), a_off.view(np.uint32)), k
        audio.append(a_on)
        for p in got:
            tp, rate = on.tap(p)
            assert rate == on.info.demod_rate_int and tp.shape == a_on.shape
            got[p].append(tp)
    got = {p: np.concatenate(v, axis=1) for p, v in got.items()}
    audio = np.concatenate(audio, axis=1)
    assert np.array_equal(got[P.TAP_POST_DEMOD].view(np.uint32), audio.view(np.uint32))   # no resampler: the audio buffer is the demodulator's output
    for c, (mode, fc, lo, hi) in enumerate(chans):
        mx = O.Mixer(fs)
        mx.set_frequency(fc)
        d = O.Decimator(fs, 30000, 0)
        y = d.process(mx.process(x)) * 10.0 ** (2 * d.dec_by2_stages / 20.0)
        assert rel_rms(got[P.TAP_POST_MIXER][c], y) <= TOL, c
        ff = O.FastFIR()
        ff.setup(float(lo), float(hi), 0.0, float(int(d.rate)))
        bp = ff.process(y)
        assert rel_rms(got[P.TAP_POST_BP][c], bp) <= TOL, c
        if mode == P.DM_NONE:   # the reference returns before the noise filter (receiver.cpp:968-971)
            assert not got[P.TAP_MODEM][c].any() and not got[P.TAP_POST_DEMOD][c].any()
            continue
        if c == 1:
            same_input = by_frames(O.Anf(), got[P.TAP_POST_BP][c].astype(np.complex128))
            assert rel_rms(got[P.TAP_MODEM][c], same_input) <= 1e-6
            md = by_frames(O.Anf(), bp)
            assert rel_rms(got[P.TAP_MODEM][c], md) <= 5e-3
        else:
            assert np.array_equal(got[P.TAP_MODEM][c].view(np.uint32), got[P.TAP_POST_BP][c].view(np.uint32))
            md = bp
        ag = by_frames(O.Agc(float(int(d.rate))), md)
        if mode == P.DM_AM:
            dm = O.DemodAM(float(int(d.rate)))
            dm.set_bandwidth(hi - lo)
            out, first = by_frames(dm, ag), 0
        elif mode == P.DM_FMN:
            # the PLL demodulator on IDENTICAL input (the device's own MODEM tap) at the step's bar (test_nfm_pll_demod_step) ...
            same = by_frames(O.DemodNFM(float(int(d.rate))), by_frames(O.Agc(float(int(d.rate))), got[P.TAP_MODEM][c].astype(np.complex128)))
            e_same = rel_rms(got[P.TAP_POST_DEMOD][c], same)
            print("FMN on identical input: %.3e" % e_same)
            assert e_same <= TOL
            # ... and against the composed chain behind the first frame: there the loop acquires on the band-pass's fp32 floor
            # (test_bank_with_every_narrow_demod_mode)
            out, first = by_frames(O.DemodNFM(float(int(d.rate))), ag), 2048
        else:
            out, first = ag, 0
        assert rel_rms(got[P.TAP_POST_DEMOD][c][first:], out[first:]) <= (5e-3 if c == 1 else TOL), c
    on.close()
    off.close()


def test_post_mixer_tap_of_a_wfm_receiver(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    fs = 2048000
    rx = P.ReceiverBank(fs, 1, True, True, 4096, max_superframes=2)
    rx.set_mixer(0, 250e3)
    rx.set_taps([P.TAP_POST_MIXER, P.TAP_RAW_IQ])
    sf = rx.superframe
    t = np.arange(2 * sf) / fs
    x = 0.3 * np.exp(1j * (2 * np.pi * 250e3 * t + 20.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(2 * sf, 9, 1e-3)
    off = P.ReceiverBank(fs, 1, True, True, 4096, max_superframes=2)
    off.set_mixer(0, 250e3)
    a_on, s_on = rx.process(x)
    a_off, s_off = off.process(x)
    assert np.array_equal(a_on.view(np.uint32), a_off.view(np.uint32)) and np.array_equal(s_on, s_off)
    mx = oracle_mod.Mixer(fs)
    mx.set_frequency(250e3)
    d = oracle_mod.Decimator(fs, 200000, 0)
    tap, rate = rx.tap(P.TAP_POST_MIXER)
    assert rate == rx.info.demod_rate_int
    assert rel_rms(tap[0], d.process(mx.process(x))) <= TOL
    raw, rate = rx.tap(P.TAP_RAW_IQ)
    assert rate == fs and np.array_equal(raw[0], x.astype(np.complex64))
    rx.close()
    off.close()


def test_refusals_leave_the_handle_usable(gpu_lib):
    import pebblesdr_amd as P
    fs = 2048000

    def refused(fn, *a):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*a)
        assert e.value.code == -6, e.value

    w = P.ReceiverBank(fs, 1, True, True, 4096)
    xw = lcg_noise(w.superframe, 1, 0.01)
    for p in (P.TAP_POST_BP, P.TAP_MODEM, P.TAP_POST_DEMOD):
        refused(w.set_taps, [p])
        refused(w.set_taps, [P.TAP_POST_MIXER, p])
        w.process(xw)
    with pytest.raises(P.PebbleGpuError) as e:
        w.set_taps([5])
    assert e.value.code == -1
    w.set_taps([P.TAP_POST_MIXER])
    w.process(xw)
    assert w.tap(P.TAP_POST_MIXER) is not None and w.tap(P.TAP_POST_BP) is None
    w.close()
    # the squelch and the taps behind its gate: whichever comes second is refused -- a one-channel receiver and a bank
    for C in (1, 3):
        for p in (P.TAP_MODEM, P.TAP_POST_DEMOD):
            r = P.ReceiverBank(fs, C, True, False, 4096, max_superframes=1 if C == 1 else 2)
            for c in range(C):
                r.set_mode(c, P.DM_USB); r.set_mixer(c, 100e3 * (c + 1)); r.set_bandpass(c, 300, 3000)
            x = lcg_noise(r.superframe, 2, 0.01)
            r.set_squelch(0, -60.0)
            refused(r.set_taps, [p])
            r.process(x)
            r.set_taps([P.TAP_POST_BP, P.TAP_RAW_IQ])      # in front of the gate: accepted
            r.process(x)
            assert r.tap(P.TAP_POST_BP) is not None
            r.set_squelch(0, -120.0)
            r.set_taps([p])
            refused(r.set_squelch, 0, -60.0)
            r.set_squelch(0, -120.0)                       # "never closes" stays accepted
            a = r.process(x)[0]
            assert r.tap(p)[0].shape == a.shape
            r.close()
    # any tap or generator through pebblegpu_process_iq
    r = P.ReceiverBank(fs, 1, True, False, 0)
    r.set_mode(0, P.DM_USB); r.set_mixer(0, 100e3); r.set_bandpass(0, 300, 3000)
    fr = lcg_noise(2048, 3, 0.01)
    for on, offf in ((lambda: r.set_taps([P.TAP_RAW_IQ]), lambda: r.set_taps([])),
                     (lambda: r.set_testbench_noise(0.1, 1), lambda: r.set_testbench_noise(0.0, 0)),
                     (lambda: r.set_testbench_sweep(P.sweep(0, 1e5, 1e6)), lambda: r.set_testbench_sweep(None))):
        on()
        refused(r.process_iq, fr)
        offf()
        r.process_iq(fr)
    refused(r.set_testbench_sweep, P.sweep(0, 10, 2.048e6))       # legs of 10 samples
    r.process_iq(fr)
    r.close()


def test_morse_modem_and_its_tap_on_the_same_channel(gpu_lib):
    """the MODEM tap is the frame m_iDigitalModem->processBlock receives: fed to the Morse restatement it yields the device's events"""
    import pebblesdr_amd as P
    fs, fc = 2048000, 100000
    rx = P.ReceiverBank(fs, 2, True, False, 0, max_superframes=4)
    for c in range(2):
        rx.set_mixer(c, fc + 20000 * c); rx.set_bandpass(c, 300, 3000)
    rx.set_morse(0, True)
    rx.set_mode(0, P.DM_CWU); rx.set_mode(1, P.DM_USB)
    rx.set_taps([P.TAP_MODEM])
    sf = rx.superframe
    K = 24
    n = K * 4 * sf
    x = lcg_noise(n, 62, 2e-4) + keyed("CQ TEST", 30, fs, n, fc + 1000.0, 0.01)
    ref = M.MorseRef(int(rx.info.demod_rate_int), 2048)
    ref.set_demod_mode(M.DM_CWU)
    got = []
    for k in range(K):
        rx.process(x[k * 4 * sf:(k + 1) * 4 * sf])
        tap, _ = rx.tap(P.TAP_MODEM)
        for f in range(tap.shape[1] // 2048):
            ref.process(tap[0][f * 2048:(f + 1) * 2048].astype(np.complex128))
        got += events_of(rx.morse_events(0))
    assert got == ref.events and len(got) >= 4
    rx.close()


# ------------------------------------------------------------------------------------------------
# the C++ adapter: pebblegpu::Receiver::setTaps / setTestBenchNoise + processIQData (include/pebblegpu_steps.hpp)
# ------------------------------------------------------------------------------------------------
ADAPTER_SRC = r'''
#include <cstdio>
#include <vector>
#include "pebblegpu_steps.hpp"
using namespace pebblegpu;
static void dump(FILE *f, int tag, const CPX *p, int n)
{
    std::fwrite(&tag, sizeof(tag), 1, f);
    std::fwrite(&n, sizeof(n), 1, f);
    std::fwrite(p, sizeof(CPX), (size_t)n, f);
}
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    std::vector<CPX> x;
    CPX v;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    while (std::fread(&v, sizeof(v), 1, f) == 1) x.push_back(v);
    std::fclose(f);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 1;
    Receiver rx(2048000, 2048, false, 0, [out](CPX *a, uint16_t n) { dump(out, 0, a, n); });   // tag 0: the audio callback
    rx.mixerChanged(100000);
    rx.filterChanged(300, 3000);
    rx.demodModeChanged(dmUSB);
    rx.setTestBenchNoise(0.002, 5);
    rx.setTaps(1u << PEBBLEGPU_TAP_RAW_IQ | 1u << PEBBLEGPU_TAP_POST_BP | 1u << PEBBLEGPU_TAP_MODEM,
               [out](int n, CPX *p, double rate, int point) { dump(out, point + ((int)rate << 8), p, n); });
    for (size_t i = 0; i + 2048 <= x.size(); i += 2048) rx.processIQData(&x[i], 2048);
    std::fclose(out);
    return rx.lastStatus() ? 4 : 0;
}
'''


def test_cpp_adapter_hands_out_the_taps_frame_by_frame(gpu_lib, tmp_path):
    """two super-frames through pebblegpu::Receiver with the noise generator and three taps on: the displayData frames are
    ReceiverBank.tap's rows and the audio callback's frames are audio(), bit for bit, frame by frame, taps before audio"""
    import pebblesdr_amd as P
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = str(tmp_path / "tb_adapter.cpp"), str(tmp_path / "tb_adapter")
    with open(src, "w") as f:
        f.write(ADAPTER_SRC)
    libdir = os.path.join(root, "pebblesdr_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(root, "include"), src, "-L" + libdir, "-lpebblegpu", "-Wl,-rpath," + libdir, "-o", exe])
    fs = 2048000
    rx = P.ReceiverBank(fs, 1, True, False, 0, max_superframes=1)
    rx.set_mixer(0, 100000); rx.set_bandpass(0, 300, 3000); rx.set_mode(0, P.DM_USB)
    rx.set_testbench_noise(0.002, 5)
    rx.set_taps([P.TAP_RAW_IQ, P.TAP_POST_BP, P.TAP_MODEM])
    sf = rx.superframe
    t = np.arange(2 * sf) / fs
    x = (0.05 * np.exp(2j * np.pi * 101.5e3 * t) + lcg_noise(2 * sf, 8, 1e-3)).astype(np.complex64).astype(np.complex128)
    x.tofile(str(tmp_path / "x.bin"))
    r = subprocess.run([exe, str(tmp_path / "x.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(str(tmp_path / "out.bin"), "rb").read()
    recs, off = [], 0
    while off < len(raw):
        tag, n = np.frombuffer(raw, dtype=np.int32, count=2, offset=off)
        recs.append((int(tag) & 255, int(tag) >> 8, np.frombuffer(raw, dtype=np.complex128, count=int(n), offset=off + 8)))
        off += 8 + 16 * int(n)
    want = []
    for k in range(2):
        audio = rx.process(x[k * sf:(k + 1) * sf])[0]
        for p in (P.TAP_RAW_IQ, P.TAP_POST_BP, P.TAP_MODEM):   # the adapter's order: every tapped point, then the audio
            row, rate = rx.tap(p)
            want += [(p, int(rate), row[0][i:i + 2048]) for i in range(0, row.shape[1], 2048)]
        want += [(0, 0, audio[0][i:i + 2048]) for i in range(0, audio.shape[1], 2048)]
    assert [(a, b, len(c)) for a, b, c in recs] == [(a, b, len(c)) for a, b, c in want]
    for (_, _, got), (p, _, ref) in zip(recs, want):
        assert np.array_equal(got.astype(np.complex64).view(np.uint32), ref.view(np.uint32)), p
    rx.close()
