"""GPU tier of the Morse stations (pebblegpu_siggen_set_morse, pebblegpu_set_testbench_morse): the stand-alone generator and the generator
at the head of a receiver against the serial restatement in tests/morsegen_ref.py, and the loop generator -> tuner bank -> band-pass ->
Morse decoder closed on the device against tests/morse_ref.py fed the oracle chain.
Bars: 1e-5 relative RMS in the time domain (TOL of tests/test_parity_gpu.py, the project's time-domain bar) and 1e-7 between two ways of
cutting the same stretch into calls (the sweep test's call-split bar, tests/test_testbench_gpu.py)."""
import functools

import numpy as np
import pytest

from tests import morse_ref as M
from tests import morsegen_ref as G
from tests import testbench_ref as R
from tests.signals import lcg_noise
from tests.test_morse_gpu import events_of, oracle_pre_agc
from tests.test_parity_gpu import TOL, rel_rms

pytestmark = pytest.mark.gpu

N19 = 1 << 19
CALLS = [1, 4099, 65536, 30001, 65535, 128, 7, 100000, 2049, 63]   # odd sizes and odd starts (the 8-byte path), then the rest in one call
FS_A = 200000

# (frequency, amplitude, wpm, ms_rise, text): a negative frequency, one near fs / 2, hard keying, texts of 1 to 12 tokens with a word space
FIVE = [(12345.0, 0.30, 50, 0, "CQ DE K1ABC "), (-31000.5, 0.20, 40, 5, "TEST "), (99990.0, 0.25, 25, 5, "A E"),
        (700.25, 0.15, 13, 20, "T "), (55555.0, 0.10, 50, 1, "E")]
TEXTS = ["E ", "TEST ", "SOS K", "CQ DE K1ABC ", "5 NN", "A B C ", " "]   # (the last: a station that never keys)
MANY = [(-90000.0 + 2700.0 * i + 0.125 * (i % 7), 0.002 + 0.0001 * (i % 5), (50, 40, 35, 30)[i % 4], (0, 5, 2, 1, 3)[i % 5], TEXTS[i % len(TEXTS)])
        for i in range(67)]


def as_ref(stations):
    return [(f, a, w, r, G.text_tokens(t)) for f, a, w, r, t in stations]


def as_lib(P, stations):
    return [P.morse_station(f, a, w, r, G.text_tokens(t)) for f, a, w, r, t in stations]


@functools.lru_cache(maxsize=None)
def restated(which):
    """the restatement of a station set over 2^19 samples at 200 kHz, computed once and never written: (samples, keyed)"""
    x, key = G.station_sum(FS_A, as_ref(FIVE if which == "five" else MANY), N19)
    x.setflags(write=False)
    key.setflags(write=False)
    return x, key


def generate_calls(P, gen, n, fill=None):
    buf = P.DeviceBuffer(8 * n)
    try:
        buf.upload(np.zeros(n, dtype=np.complex64) if fill is None else fill.astype(np.complex64))
        off, k = 0, 0
        while off < n:
            m = min(n - off, CALLS[k]) if k < len(CALLS) else n - off
            gen.generate_device(buf.ptr + 8 * off, m)
            off += m
            k += 1
        gen.synchronize()
        return buf.download(np.complex64, n)
    finally:
        buf.free()


# ------------------------------------------------------------------------------------------------
# (a) the stand-alone generator
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["five", "many"])
def test_generator_against_the_serial_restatement(gpu_lib, which):
    import pebblesdr_amd as P
    ref, key = restated(which)
    assert key.mean() > 0.05 and (ref[~key] == 0).all() and (which == "many" or (~key).sum() > 1000)   # (67 stations leave hardly a common gap)
    stations = as_lib(P, FIVE if which == "five" else MANY)
    g = P.SigGen(FS_A)
    g.set_morse(stations, mix=False)
    got = generate_calls(P, g, N19, fill=np.full(N19, 3 + 4j))       # mix = 0: what is in the buffer is not read
    err = rel_rms(got, ref)
    print("%s stations, calls of %s ...: rel rms %.3e" % (which, CALLS[:5], err))
    assert err <= TOL
    assert (got[~key] == 0).all()                                    # exact zeros in the gaps
    # the setter restarts every station: the same stretch in one call
    g.set_morse(stations, mix=False)
    buf = P.DeviceBuffer(8 * N19)
    g.generate_device(buf.ptr, N19)
    g.synchronize()
    one = buf.download(np.complex64, N19)
    buf.free()
    split = rel_rms(one, got)
    print("%s stations, one call against many: %.3e" % (which, split))
    assert split <= 1e-7 and rel_rms(one, ref) <= TOL and (one[~key] == 0).all()
    g.close()


def test_generator_mixes_into_its_input_and_the_host_frame_entry_point_agrees(gpu_lib):
    import pebblesdr_amd as P
    ref, key = restated("five")
    n = 1 << 17
    x = lcg_noise(n, 17, 0.05).astype(np.complex64)
    g = P.SigGen(FS_A, 2048)
    g.set_morse(as_lib(P, FIVE), mix=True)
    got = generate_calls(P, g, n, fill=x)
    assert rel_rms(got, x.astype(np.complex128) + ref[:n]) <= TOL
    assert np.array_equal(got[~key[:n]], x[~key[:n]])                # a gap leaves the input as it is
    # pebblegpu_siggen_generate: CPX frames on the host, in place, with the noise on as well
    g.set_morse(as_lib(P, FIVE), mix=True)
    g.set_noise(0.01, 99)
    m = 16 * 2048
    frames = x[:m].astype(np.complex128)
    host = np.concatenate([g.generate(frames[k * 2048:(k + 1) * 2048].copy()) for k in range(16)])
    assert rel_rms(host, frames + ref[:m] + 0.01 * R.noise(99, 0, 0, m)[0]) <= TOL
    g.set_noise(0.0, 0)                                              # the noise setter does not move the stations
    more = g.generate(np.zeros(2048, dtype=np.complex128))
    assert rel_rms(more, ref[m:m + 2048]) <= TOL
    g.set_morse([])                                                  # off: the frame stays as it is
    same = frames[:2048].copy()
    assert np.array_equal(g.generate(same.copy()), same)
    g.close()


# ------------------------------------------------------------------------------------------------
# (b) the generator at the head of a receiver
# ------------------------------------------------------------------------------------------------
FS_B = 2048000
SW_B = (-0.5e6, 0.7e6, 123456789.0)        # SW_2M of tests/test_testbench_gpu.py
# (fast keying -- 4, 6 and 3 ms per Tcw -- so that a super-frame of 32 ms holds marks, gaps and the texts' wrap-around)
THREE = [(101000.0, 0.05, 300, 1, "TE "), (-300000.5, 0.04, 200, 0, "E T"), (1023000.0, 0.03, 400, 2, "A")]


@functools.lru_cache(maxsize=None)
def restated_b(n):
    x, key = G.station_sum(FS_B, as_ref(THREE), n)
    x.setflags(write=False)
    key.setflags(write=False)
    return x, key


def test_receiver_injects_into_float2_input_of_independent_streams(gpu_lib):
    """sweep + stations + noise on two independent streams: the tap is input + the three restatements; the sweep's and the noise's setters
    leave the stations where they are, and the stations' setter leaves the sweep and the noise counter where they are"""
    import pebblesdr_amd as P
    rx = P.ReceiverBank(FS_B, 2, False, False, 4096, max_superframes=2)
    sf = rx.superframe
    st, key = restated_b(2 * sf)
    assert 0.05 < key.mean() < 0.95
    sweep, _ = R.serial_sweep(FS_B, 2 * sf, 2048, 0.2, start=SW_B[0], stop=SW_B[1], rate=SW_B[2], sweep_type=R.REPEAT)
    noise = [0.003 * R.noise(77, s, 0, 2 * sf)[0] for s in range(2)]
    x = np.stack([lcg_noise(3 * sf, 31 + s, 0.02) for s in range(2)]).astype(np.complex64)
    rx.set_testbench_sweep(P.sweep(*SW_B, amplitude=0.2))
    rx.set_testbench_noise(0.003, 77)
    rx.set_testbench_morse(as_lib(P, THREE), mix=True)
    rx.set_taps([P.TAP_RAW_IQ])
    first, second = slice(0, sf), slice(sf, 2 * sf)
    # call 0: everything from its start.  Then the noise setter (TestBench::reset: sweep and noise start over, the stations go on), then
    # the stations' setter (they start over, sweep and noise go on)
    plan = [(None, first, first), (lambda: rx.set_testbench_noise(0.003, 77), first, second), (lambda: rx.set_testbench_morse(as_lib(P, THREE), mix=True), second, first)]
    for k, (setter, tb_at, st_at) in enumerate(plan):
        if setter:
            setter()
        seg = np.ascontiguousarray(x[:, k * sf:(k + 1) * sf])
        buf = P.DeviceBuffer.from_array(seg)
        rx.process_device(buf.ptr, sf)
        tap, rate = rx.tap(P.TAP_RAW_IQ)
        assert np.array_equal(buf.download(np.complex64, seg.size).reshape(seg.shape), seg)   # the caller's buffer is never written
        buf.free()
        assert rate == FS_B and tap.shape == (2, sf)
        assert rx.kernel_name(2).startswith("k_morsegen + ")
        for s in range(2):
            want = seg[s].astype(np.complex128) + sweep[tb_at] + noise[s][tb_at] + st[st_at]
            err = rel_rms(tap[s], want)
            print("call %d stream %d: rel rms %.3e" % (k, s, err))
            assert err <= TOL, (k, s)
    # the sweep's setter too leaves the stations alone; stations off again: the generator's own kernel is back
    rx.set_testbench_sweep(None)
    rx.set_testbench_noise(0.0, 0)
    seg = np.ascontiguousarray(x[:, :sf])
    rx.process(seg)
    tap, _ = rx.tap(P.TAP_RAW_IQ)
    for s in range(2):
        assert rel_rms(tap[s], seg[s].astype(np.complex128) + st[second]) <= TOL
        assert np.array_equal(tap[s][~key[second]], seg[s][~key[second]])
    rx.set_testbench_morse(None)
    rx.set_testbench_noise(0.003, 77)
    rx.process(seg)
    assert rx.kernel_name(2).startswith("k_testbench + ")
    rx.close()


def test_receiver_injects_into_raw_s8_input(gpu_lib):
    import pebblesdr_amd as P
    rx = P.ReceiverBank(FS_B, 1, True, False, 0, max_superframes=2)
    sf = rx.superframe
    st, key = restated_b(2 * sf)
    rng = np.random.RandomState(5)
    raw = rng.randint(-20, 21, size=(2 * sf, 2)).astype(np.int8)
    conv = (raw[:, 0].astype(np.float64) + 1j * raw[:, 1]) / 128.0
    rx.set_taps([P.TAP_RAW_IQ])
    buf = P.DeviceBuffer.from_array(raw)
    for mix in (True, False):
        rx.set_testbench_morse(as_lib(P, THREE), mix=mix)
        rx.process_raw_device(buf.ptr, 2 * sf, P.binding.IQ_S8)
        tap, _ = rx.tap(P.TAP_RAW_IQ)
        assert rx.kernel_name(2).startswith("k_morsegen + ")
        assert rel_rms(tap[0], (conv if mix else 0.0) + st) <= TOL, mix
        if not mix:
            assert (tap[0][~key] == 0).all()                        # mix = 0: the input is not read
        assert np.array_equal(buf.download(np.int8, raw.size).reshape(raw.shape), raw)   # the caller's buffer is never written
    buf.free()
    rx.close()


# ------------------------------------------------------------------------------------------------
# (c) generator -> tuner bank -> band-pass -> Morse decoder, closed on the device
# ------------------------------------------------------------------------------------------------
LOOP = [(100e3, 25, "TEST ", "TEST TEST"), (-300e3, 40, "CQ DE K1ABC ", "DE K1ABC"), (450e3, 18, "SOS ", "SOS")]


def contains(seq, sub):
    return any(seq[i:i + len(sub)] == sub for i in range(len(seq) - len(sub) + 1))


def test_the_loop_closed_on_the_device(gpu_lib, oracle_mod):
    """Three stations 1 kHz above the mixers of a three-channel CWU bank, summed into lcg noise on the device: every channel's events
    and status are those of the restatement decoder fed the oracle chain over input + restated stations.
    Measured on the CPU for exactly these inputs: the restatement's margins are 7.3e-3, 5.8e-2, 3.2e-3 and it decodes `TEST TEST TES`,
    `FQ DE K1ABC ` (the first character at 40 wpm is read while the speed estimate still moves from 20) and `SOS SO`."""
    import pebblesdr_amd as P
    fs = 2048000
    rx = P.ReceiverBank(fs, 3, True, False, 0, max_superframes=8)
    for c, (fc, _, _, _) in enumerate(LOOP):
        rx.set_mixer(c, fc)
        rx.set_bandpass(c, 300, 3000)
        rx.set_morse(c, True)
        rx.set_mode(c, P.DM_CWU)
    sf = rx.superframe
    assert sf == 65536
    K, per = 16, 8 * sf
    n = K * per
    x = lcg_noise(n, 3, 2e-4).astype(np.complex64)
    stations = [(fc + 1000.0, 0.01, wpm, 5, text) for fc, wpm, text, _ in LOOP]
    rx.set_testbench_morse(as_lib(P, stations), mix=True)
    got = [[] for _ in LOOP]
    for k in range(K):
        rx.process(x[k * per:(k + 1) * per])
        for c in range(len(LOOP)):
            got[c] += events_of(rx.morse_events(c))
    total = x.astype(np.complex128) + G.station_sum(fs, as_ref(stations), n)[0]
    for c, (fc, _, _, expect) in enumerate(LOOP):
        a, rate = oracle_pre_agc(oracle_mod, total, fs, fc, 300, 3000)
        r = M.MorseRef(rate, 2048)
        r.set_demod_mode(M.DM_CWU)
        for j in range(len(a) // 2048):
            r.process(a[j * 2048:(j + 1) * 2048])
        print("channel %d: margin %.3e, %d events" % (c, min(r.margins), len(r.events)))
        assert min(r.margins) > 1e-4, (c, min(r.margins))          # "identical" means something
        assert got[c] == r.events, (c, got[c], r.events)
        assert rx.morse_status(c) == r.status()
        want = M.text_tokens(expect)[:-1]                            # the text's tokens, without the word space behind its last word
        assert contains([(k_, t) for _, t, k_ in got[c]], want), (c, got[c])
    rx.close()


# ------------------------------------------------------------------------------------------------
# (d) refusals leave the handle usable
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(gpu_lib):
    import pebblesdr_amd as P
    fs = 2048000
    ok = G.text_tokens("E ")

    def refused(code, fn, *a, **kw):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*a, **kw)
        assert e.value.code == code, e.value

    r = P.ReceiverBank(fs, 1, True, False, 0)
    r.set_mode(0, P.DM_USB); r.set_mixer(0, 100e3); r.set_bandpass(0, 300, 3000)
    r.set_taps([P.TAP_RAW_IQ])
    sf = r.superframe
    x = lcg_noise(sf, 3, 0.01).astype(np.complex64)
    good = [P.morse_station(101e3, 0.05, 300, 1, ok)]
    ref = G.station_sum(fs, [(101e3, 0.05, 300, 1, ok)], 2 * sf)[0]
    r.set_testbench_morse(good)
    r.process(x)
    assert rel_rms(r.tap(P.TAP_RAW_IQ)[0][0], x.astype(np.complex128) + ref[:sf]) <= TOL
    for code, bad in ((-1, P.morse_station(fs / 2, 0.05, 50, 5, ok)), (-1, P.morse_station(101e3, float("nan"), 50, 5, ok)),
                      (-1, P.morse_station(101e3, 0.05, 50, 5, [])), (-1, P.morse_station(101e3, 0.05, 50, 5, [0x200])),
                      (-6, P.morse_station(101e3, 0.05, 0, 5, ok)), (-6, P.morse_station(101e3, 0.05, 1201, 5, ok)),
                      (-6, P.morse_station(101e3, 0.05, 50, 24, ok)), (-6, P.morse_station(101e3, 0.05, 1, 0, [0x1FF] * 60000))):
        refused(code, r.set_testbench_morse, good + [bad])
    refused(-1, r.set_testbench_morse, good * (P.MORSE_MAX_STATIONS + 1))
    # every refused call left the set as it was, and where it was: the next call goes on with the second super-frame
    r.process(x)
    assert rel_rms(r.tap(P.TAP_RAW_IQ)[0][0], x.astype(np.complex128) + ref[sf:]) <= TOL
    r.set_testbench_morse(good * P.MORSE_MAX_STATIONS)              # the cap itself is accepted
    r.process(x)
    assert rel_rms(r.tap(P.TAP_RAW_IQ)[0][0], x.astype(np.complex128) + P.MORSE_MAX_STATIONS * ref[:sf]) <= TOL
    # pebblegpu_process_iq with stations on: the existing generator rule
    r.set_taps([])
    fr = lcg_noise(2048, 3, 0.01)
    refused(-6, r.process_iq, fr)
    r.set_testbench_morse([])
    r.process_iq(fr)
    r.close()
    # the stand-alone generator
    g = P.SigGen(fs)
    refused(-6, g.set_morse, [P.morse_station(101e3, 0.05, 0, 5, ok)])
    refused(-1, g.set_morse, good * (P.MORSE_MAX_STATIONS + 1))
    g.set_morse(good, mix=False)
    buf = P.DeviceBuffer(8 * 4096)
    g.generate_device(buf.ptr, 4096)
    g.synchronize()
    assert rel_rms(buf.download(np.complex64, 4096), ref[:4096]) <= TOL
    buf.free()
    g.close()
