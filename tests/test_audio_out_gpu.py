"""GPU tier (-m gpu): the audio output stage and IQ recording through the pinned egress slots (pebblegpu_receiver_audio_out_*,
pebblegpu_receiver_record_*).

The twin-receiver pattern of tests/test_screen_map_gpu.py::test_maps_between_calls_without_a_host_wait: receiver `b` is read the
existing way (synchronize, then the audio rows or the RAW_IQ tap), receiver `a` queues all K calls with nothing waiting on the host in
between and only then reads K blocks.  Expected = the host twin (pebblegpu_audio_out_convert / pebblegpu_iq_record_convert, held to
the reference's rule by tests/test_audio_out_host.py) applied to b's rows; the comparison is np.array_equal -- there is no arithmetic
between the audio rows and the block that could justify a tolerance.  Every test asserts that the K expected blocks differ from each
other, so a stale read would show.  2.048 Msps, 2048-sample frames: the super-frame is 65536 samples."""
import numpy as np
import pytest

from tests.signals import lcg_noise

pytestmark = pytest.mark.gpu

FS, NF, SF = 2048000, 2048, 65536
E_INVALID, E_UNSUPPORTED = -1, -6
FCS5 = [100e3, -250e3, 400e3, -600e3, 700e3]


def modes5(P):
    return [(P.DM_AM, -5000, 5000), (P.DM_USB, 300, 3000), (P.DM_CWU, 200, 1200), (P.DM_NONE, 300, 3000), (P.DM_FMN, -7500, 7500)]


def tune5(P, rx, count=5, first=0):
    for c in range(count):
        m, lo, hi = modes5(P)[first + c]
        rx.set_mode(c, m)
        rx.set_mixer(c, FCS5[first + c])
        rx.set_bandpass(c, lo, hi)


def stream5(n_sf, seed=3):
    """a strong AM carrier on channel 0, tones in 1, 2 and 3, an FM carrier on 4, over LCG noise: no two super-frames alike"""
    n = n_sf * SF
    t = np.arange(n) / FS
    x = lcg_noise(n, seed, 1e-3)
    x = x + 0.8 * (1 + 0.9 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * FCS5[0] * t)
    x = x + 0.1 * np.exp(2j * np.pi * (FCS5[1] + 1300.0) * t) + 0.1 * np.exp(2j * np.pi * (FCS5[2] + 700.0) * t)
    x = x + 0.05 * np.exp(2j * np.pi * (FCS5[3] + 1000.0) * t)
    x = x + 0.1 * np.exp(1j * (2 * np.pi * FCS5[4] * t + 2.0 * np.sin(2 * np.pi * 800 * t)))
    return x.astype(np.complex64)


def upload_calls(P, x, sizes, unit=SF):
    bufs, pos = [], 0
    for k in sizes:
        seg = x[..., pos * unit:(pos + k) * unit]
        bufs.append((P.DeviceBuffer.from_array(P.binding.to_f32_iq(seg), 0), k * unit))
        pos += k
    return bufs


def expected_block(P, fmt, rows, levels, sel):
    """the host twin applied to the selected rows of b's audio: [len(sel), n, 2] ([len(sel), n] for the mono format)"""
    return np.stack([P.audio_out_convert(fmt, levels.get(ch, (100.0, False))[0], levels.get(ch, (100.0, False))[1], rows[ch]) for ch in sel])


def read_blocks(nxt, rel, K):
    """K blocks, oldest first, each released once copied: [(call_index, dropped_before, array)]"""
    out = []
    for _ in range(K):
        blk = nxt(True)
        assert blk is not None
        out.append(blk)
        rel(blk[0])
    return out


def all_differ(blocks):
    return len({np.ascontiguousarray(w).tobytes() for w in blocks}) == len(blocks)


def free_all(bufs, *rxs):
    for bf, _ in bufs:
        bf.free()
    for r in rxs:
        r.close()


# 1. the two-stage route of a bank without a display transform
@pytest.mark.parametrize("fmt_name", ["F32", "S16", "S16_MONO"])
def test_two_stage_route(gpu_lib, fmt_name):
    import pebblesdr_amd as P
    fmt = {"F32": P.AUDIO_F32, "S16": P.AUDIO_S16, "S16_MONO": P.AUDIO_S16_MONO}[fmt_name]
    a = P.ReceiverBank(2.048e6, 5, True, False, spectrum_bins=0, max_superframes=2)
    b = P.ReceiverBank(2.048e6, 5, True, False, spectrum_bins=0, max_superframes=2)
    sizes = [1, 2, 1, 2]
    bufs = upload_calls(P, stream5(sum(sizes)), sizes)
    sel, levels = [3, 0, 4], {0: (250.0, False), 3: (37.0, False), 4: (100.0, True)}
    try:
        for rx in (a, b):
            tune5(P, rx)
        a.audio_out_open(fmt, sel, 4)
        for ch, (g, m) in levels.items():
            a.set_audio_level(ch, g, m)
        want = []
        for buf, n in bufs:
            b.process_device(buf.ptr, n)
            b.synchronize()
            want.append(expected_block(P, fmt, b.audio(), levels, sel))
        for buf, n in bufs:  # nothing waits on the host between these
            a.process_device(buf.ptr, n)
        got = read_blocks(a.audio_out_next, a.audio_out_release, len(bufs))
        clip = float(np.float32(0.9999)) if fmt == P.AUDIO_F32 else 32763  # trunc(0.9999f * 32767)
        for k, (call, dropped, blk) in enumerate(got):
            assert (call, dropped) == (k, 0)
            assert blk.shape == want[k].shape and blk.shape[1] == sizes[k] * SF // a.D
            assert np.array_equal(blk, want[k]), "call %d" % k
            assert (np.abs(want[k][1].astype(np.float64)) >= clip).any(), "channel 0 at gain 250 does not clip in call %d" % k
            assert not want[k][2].any() and want[k][1].any()  # the muted row; the loud one
        assert all_differ(want)
        assert a.audio_out_next(False) is None and a.audio_out_dropped() == 0
        for w in range(1, 6):  # the ring does not change the route
            assert a.kernel_name(w) == b.kernel_name(w), w
        assert a.kernel_name(2)
    finally:
        free_all(bufs, a, b)


# 2. the side-by-side route (one WFM channel beside its display transform) and the resampler's ragged counts
@pytest.mark.parametrize("fmt_name", ["F32", "S16"])
def test_side_by_side_route_and_ragged_counts(gpu_lib, fmt_name):
    import pebblesdr_amd as P
    fmt = {"F32": P.AUDIO_F32, "S16": P.AUDIO_S16}[fmt_name]
    a = P.ReceiverBank(2.048e6, 1, True, True, spectrum_bins=2048, audio_rate=11025)
    b = P.ReceiverBank(2.048e6, 1, True, True, spectrum_bins=2048, audio_rate=11025)
    K = 4
    sf = a.superframe
    t = np.arange(K * sf) / 2.048e6
    x = (0.5 * np.exp(1j * (2 * np.pi * 300e3 * t + 30.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(K * sf, 11, 1e-3)).astype(np.complex64)
    bufs = upload_calls(P, x, [1] * K, unit=sf)
    try:
        for rx in (a, b):
            rx.set_mixer(0, 300e3)
        a.audio_out_open(fmt, None, 4)
        a.set_audio_level(0, 180.0, False)
        want = []
        for buf, n in bufs:
            b.process_device(buf.ptr, n)
            b.synchronize()
            want.append(expected_block(P, fmt, b.audio(), {0: (180.0, False)}, [0]))
        for buf, n in bufs:
            a.process_device(buf.ptr, n)
        got = read_blocks(a.audio_out_next, a.audio_out_release, K)
        counts = [w.shape[1] for w in want]
        print("resampled counts per call:", counts)
        assert len(set(counts)) > 1 and any(c % 2 for c in counts)  # ragged: they differ from call to call, odd ones among them
        for k, (call, dropped, blk) in enumerate(got):
            assert (call, dropped) == (k, 0) and blk.shape == want[k].shape
            assert np.array_equal(blk, want[k]), "call %d" % k
            assert want[k].any()
        assert all_differ(want)
        for w in range(1, 6):
            assert a.kernel_name(w) == b.kernel_name(w), w
    finally:
        free_all(bufs, a, b)


# 3. the bank's squelch gate: the block is packed behind run_gate_zero and the clears
def test_bank_gate(gpu_lib):
    import pebblesdr_amd as P
    C = 3
    a = P.ReceiverBank(FS, C, True, False, 4096, max_superframes=2)
    b = P.ReceiverBank(FS, C, True, False, 4096, max_superframes=2)
    sizes = [1, 2, 1, 2]
    pattern = [1, 0, 1, 1, 0, 1]  # channel 1's carrier, per super-frame
    n = sum(sizes) * SF
    t = np.arange(n) / FS
    x = lcg_noise(n, 9, 1e-5)
    x = x + 0.1 * (1 + 0.5 * np.cos(2 * np.pi * 700 * t)) * np.exp(2j * np.pi * FCS5[0] * t)
    x = x + np.repeat(np.asarray(pattern, dtype=np.float64), SF) * 0.1 * np.exp(2j * np.pi * (FCS5[1] + 1300.0) * t)
    x = x + 0.1 * np.exp(2j * np.pi * (FCS5[2] + 700.0) * t)
    bufs = upload_calls(P, x.astype(np.complex64), sizes)
    levels = {0: (250.0, False), 2: (37.0, False)}
    try:
        for rx in (a, b):
            tune5(P, rx, C)
            rx.set_squelch(1, -60.0)
        a.audio_out_open(P.AUDIO_F32, None, 4)
        for ch, (g, m) in levels.items():
            a.set_audio_level(ch, g, m)
        want, rows1 = [], []
        for buf, nn in bufs:
            b.process_device(buf.ptr, nn)
            b.synchronize()
            rows = b.audio()
            rows1.append(rows[1])
            want.append(expected_block(P, P.AUDIO_F32, rows, levels, range(C)))
        for buf, nn in bufs:
            a.process_device(buf.ptr, nn)
        got = read_blocks(a.audio_out_next, a.audio_out_release, len(bufs))
        for k, (call, dropped, blk) in enumerate(got):
            assert (call, dropped) == (k, 0)
            assert np.array_equal(blk, want[k]), "call %d" % k
        # the gate really closed and opened: channel 1's super-frames follow the keying
        segs = np.concatenate(rows1).reshape(len(pattern), -1)
        assert [bool(s.any()) for s in segs] == [bool(p) for p in pattern]
        got1 = np.concatenate([blk[1] for _, _, blk in got]).reshape(len(pattern), -1)
        assert [bool(s.any()) for s in got1] == [bool(p) for p in pattern]
        assert all_differ(want)
    finally:
        free_all(bufs, a, b)


# 4. the one-channel squelch: a closed call still gives its block, with no samples
def test_one_channel_squelch(gpu_lib):
    import pebblesdr_amd as P
    a = P.ReceiverBank(FS, 1, True, False, 4096)
    b = P.ReceiverBank(FS, 1, True, False, 4096)
    K = 5
    n = K * SF
    t = np.arange(n) / FS
    x = (0.1 * np.exp(2j * np.pi * (100e3 + 1300.0) * t) + lcg_noise(n, 4, 1e-4)).astype(np.complex64)
    bufs = upload_calls(P, x, [1] * K)
    try:
        for rx in (a, b):
            rx.set_mode(0, P.DM_USB); rx.set_mixer(0, 100e3); rx.set_bandpass(0, 300, 3000)
        a.audio_out_open(P.AUDIO_F32, None, 8)
        want = []
        for k, (buf, nn) in enumerate(bufs):
            if k in (2, 4):
                b.set_squelch(0, 50.0 if k == 2 else -120.0)
            b.process_device(buf.ptr, nn)
            b.synchronize()
            want.append(expected_block(P, P.AUDIO_F32, b.audio(), {}, [0]))
        for k, (buf, nn) in enumerate(bufs):
            if k in (2, 4):
                a.set_squelch(0, 50.0 if k == 2 else -120.0)
            a.process_device(buf.ptr, nn)
        got = read_blocks(a.audio_out_next, a.audio_out_release, K)
        assert [call for call, _, _ in got] == list(range(K))  # contiguous
        assert [blk.shape[1] for _, _, blk in got] == [SF // a.D, SF // a.D, 0, 0, SF // a.D]
        for k, (call, dropped, blk) in enumerate(got):
            assert dropped == 0 and blk.shape == want[k].shape
            assert np.array_equal(blk, want[k]), "call %d" % k
        assert all_differ([want[0], want[1], want[4]]) and want[4].any()
    finally:
        free_all(bufs, a, b)


# 5. a full ring drops, it does not refuse -- and the chain does not notice
def test_drops(gpu_lib):
    import pebblesdr_amd as P
    a = P.ReceiverBank(2.048e6, 5, True, False, spectrum_bins=0, max_superframes=2)
    b = P.ReceiverBank(2.048e6, 5, True, False, spectrum_bins=0, max_superframes=2)
    K = 5
    bufs = upload_calls(P, stream5(K, seed=8), [1] * K)
    try:
        for rx in (a, b):
            tune5(P, rx)
        a.audio_out_open(P.AUDIO_F32, None, 2)
        want = []
        for buf, n in bufs:
            b.process_device(buf.ptr, n)
            b.synchronize()
            want.append(expected_block(P, P.AUDIO_F32, b.audio(), {}, range(5)))
        for buf, n in bufs[:4]:  # 4 calls, nothing released
            a.process_device(buf.ptr, n)
        first = [a.audio_out_next(True), a.audio_out_next(True)]
        assert [(blk[0], blk[1]) for blk in first] == [(0, 0), (1, 0)]
        assert a.audio_out_next(True) is None  # calls 2 and 3 were dropped
        assert a.audio_out_dropped() == 2
        for k in (0, 1):
            assert np.array_equal(first[k][2], want[k])
            a.audio_out_release(k)
        a.process_device(bufs[4][0].ptr, bufs[4][1])
        call, dropped, blk = a.audio_out_next(True)
        assert (call, dropped) == (4, 2)
        assert np.array_equal(blk, want[4])  # b never dropped anything: a's chain state is b's
        a.audio_out_release(4)
        assert a.audio_out_dropped() == 2 and all_differ(want)
    finally:
        free_all(bufs, a, b)


# 6. end to end against the oracle: the config-1 shape
def test_against_the_oracle(gpu_lib, oracle_mod):
    """One AM channel at 2.048 Msps, three super-frames, float blocks at gain 100, against Audio::SendToOutput's rule (written out
    here) applied to oracle.Receiver's audio.  Bar: the project's own <= 1e-5 relative RMS for this chain -- the clamp is continuous
    (and 1-Lipschitz), so the bar carries over."""
    import pebblesdr_amd as P
    fs, n = 2048000, 2048
    ref = oracle_mod.Receiver(fs, n, 4096)
    ref.set_mode(oracle_mod.AM); ref.set_mixer(100e3); ref.set_filter(-5000, 5000)
    rx = P.ReceiverBank(fs, 1, True, False, 4096)
    rx.set_mode(0, P.DM_AM); rx.set_mixer(0, 100e3); rx.set_bandpass(0, -5000, 5000)
    K = 3
    nfr = K * 32
    t = np.arange(nfr * n) / fs
    x = 10 ** (-10 / 20) * (1 + 0.5 * np.cos(2 * np.pi * 1000 * t)) * np.exp(2j * np.pi * 100e3 * t) + lcg_noise(nfr * n, 1, 3e-4)
    x = np.round(x * 32767.0) / 32767.0  # 16-bit PCM WAV scaling, wavfile.cpp:299-300
    bufs = upload_calls(P, x.astype(np.complex64), [1] * K)
    try:
        rx.audio_out_open(P.AUDIO_F32, None, 4)
        for buf, nn in bufs:
            rx.process_device(buf.ptr, nn)
        got = read_blocks(rx.audio_out_next, rx.audio_out_release, K)
        for k in range(K):
            ra = np.concatenate([ref.process(x[(k * 32 + f) * n:(k * 32 + f + 1) * n])[0] for f in range(32)])
            lr = np.stack([ra.real, ra.imag], axis=1).astype(np.float32)
            tt = (lr.astype(np.float64) * np.float64(np.float32(100.0) / np.float32(100))).astype(np.float32)  # audiopa.cpp:323
            m = np.float32(0.9999)
            wantk = np.where(tt > m, m, np.where(tt < -m, -m, tt))                                          # audiopa.cpp:327-330
            blk = got[k][2][0]
            assert blk.shape == wantk.shape
            err = float(np.sqrt(np.mean((blk.astype(np.float64) - wantk) ** 2)) / np.sqrt(np.mean(wantk.astype(np.float64) ** 2)))
            print("call %d: rel-RMS %.3e" % (k, err))
            assert err <= 1e-5, (k, err)
    finally:
        free_all(bufs, rx)


# 7. the shards of a multibank: setters and read-outs through the borrowed handles
def test_multibank_shards(gpu_lib):
    import pebblesdr_amd as P
    mb = P.MultiBank(FS, 5, [0, 0], frames_per_buffer=NF, max_superframes=2)
    one = P.ReceiverBank(FS, 5, True, False, 0, max_superframes=2)
    sizes = [1, 2, 1]
    bufs = upload_calls(P, stream5(sum(sizes), seed=12), sizes)
    levels = {0: (250.0, False), 1: (37.0, False), 4: (100.0, True)}
    try:
        tune5(P, one)
        for g, (first, count) in enumerate(mb.ranges):
            tune5(P, mb.shard(g), count, first)
        one.audio_out_open(P.AUDIO_F32, None, 4)
        for g in range(mb.n_shards):
            mb.shard(g).audio_out_open(P.AUDIO_F32, None, 4)
        for ch, (gain, mute) in levels.items():
            one.set_audio_level(ch, gain, mute)
            g, c = mb.locate(ch)
            mb.shard(g).set_audio_level(c, gain, mute)
        for buf, n in bufs:
            one.process_device(buf.ptr, n)
            mb.process_device([buf.ptr] * mb.n_shards, n)
        want = read_blocks(one.audio_out_next, one.audio_out_release, len(bufs))
        assert sum(cnt for _, cnt in mb.ranges) == 5 and mb.n_shards == 2
        for g, (first, count) in enumerate(mb.ranges):
            s = mb.shard(g)
            got = read_blocks(s.audio_out_next, s.audio_out_release, len(bufs))
            for k, (call, dropped, blk) in enumerate(got):
                assert (call, dropped) == (k, 0) and blk.shape[0] == count
                assert np.array_equal(blk, want[k][2][first:first + count]), (g, k)
        assert all_differ([w[2] for w in want]) and all(w[2][1].any() and not w[2][4].any() for w in want)
        for g in range(mb.n_shards):
            mb.shard(g).audio_out_close()
    finally:
        free_all(bufs, mb, one)


# 8. IQ recording: what the RAW_IQ tap shows, as PCM16
@pytest.mark.parametrize("feed", ["float2 + sweep, two streams", "raw S8 in QI order"])
def test_recording(gpu_lib, feed):
    import pebblesdr_amd as P
    raw = feed.startswith("raw")
    S = 1 if raw else 2
    a = P.ReceiverBank(FS, S, raw, False, 0)
    b = P.ReceiverBank(FS, S, raw, False, 0)
    K = 3
    bufs = []
    try:
        for rx in (a, b):
            for c in range(S):
                rx.set_mode(c, P.DM_USB); rx.set_mixer(c, 100e3 * (c + 1)); rx.set_bandpass(c, 300, 3000)
        if raw:
            rng = np.random.default_rng(21)
            for k in range(K):
                q = rng.integers(-128, 128, size=(SF, 2), dtype=np.int8)
                q[:8] = [[127, -128], [-128, 127], [0, 1], [1, 0], [-1, 64], [64, -1], [100, -100], [-127, 127]]
                bufs.append((P.DeviceBuffer.from_array(q, 0), SF))
        else:
            t = np.arange(K * SF) / FS
            x = np.stack([0.3 * np.exp(2j * np.pi * 150e3 * t) + lcg_noise(K * SF, 31, 1e-2), 0.7 * np.exp(-2j * np.pi * 90e3 * t) + lcg_noise(K * SF, 32, 1e-2)])
            bufs = upload_calls(P, x.astype(np.complex64), [1] * K)
            for rx in (a, b):
                rx.set_testbench_sweep(P.sweep(-0.5e6, 0.7e6, 123456789.0, amplitude=0.6, mix=True))  # pushes the sum past +-1: saturation
        b.set_taps([P.TAP_RAW_IQ])
        a.record_open(3)

        def call(rx, buf, n):
            if raw:
                rx.process_raw_device(buf.ptr, n, P.binding.IQ_S8, P.binding.IQO_QI)
            else:
                rx.process_device(buf.ptr, n)

        want = []
        for buf, n in bufs:
            call(b, buf, n)
            b.synchronize()
            tap, rate = b.tap(P.TAP_RAW_IQ)
            assert tap.shape == (S, n) and rate == FS
            want.append(np.stack([P.iq_record_convert(row) for row in tap]))
        for buf, n in bufs:
            call(a, buf, n)
        got = read_blocks(a.record_next, a.record_release, K)
        for k, (c_idx, dropped, blk) in enumerate(got):
            assert (c_idx, dropped) == (k, 0) and blk.dtype == np.int16 and blk.shape == (S, SF, 2)
            assert np.array_equal(blk, want[k]), "call %d" % k
        assert all_differ(want)
        if raw:  # QI order: the first pair (127, -128) is Q, I
            assert want[0][0, 0].tolist() == [int(np.trunc(-128 / 128 * 32767)), int(np.trunc(np.float64(np.float32(127 / 128)) * 32767))]
        else:
            assert (np.abs(np.concatenate(want).astype(np.int32)) == 32767).any()  # the sweep on top of the streams saturates somewhere
        assert np.array_equal(a.audio(), b.audio())  # recording leaves the chain alone
        a.record_close()
    finally:
        free_all(bufs, a, b)


# 8c. raw calls of the headline shape: one WFM channel beside the 8192-bin transform at 20 Msps, where the call's own kernels convert in
# their loads and no float2 copy of the stream exists -- the recording kernel converts from the raw pairs itself
def test_recording_raw_beside_the_display_transform(gpu_lib):
    import pebblesdr_amd as P
    fs = 20000000
    a = P.ReceiverBank(fs, 1, True, True, 8192)
    b = P.ReceiverBank(fs, 1, True, True, 8192)
    sf = a.superframe
    K = 4  # three calls with the generator off (the first inside the oscillator's transient: staged; then raw-fused), one with it on
    t = np.arange(K * sf) / fs
    x = 0.4 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(K * sf, 2, 1e-2)
    q = np.stack([np.round(x.imag * 100), np.round(x.real * 100)], axis=1).astype(np.int8)  # Q, I
    q[:4] = [[127, -128], [-128, 127], [0, 1], [-1, 64]]
    buf = P.DeviceBuffer.from_array(q, 0)
    try:
        for rx in (a, b):
            rx.set_mixer(0, 1.0e6)
        b.set_taps([P.TAP_RAW_IQ])
        a.record_open(4)
        want = []
        for k in range(K):
            if k == 3:
                b.set_testbench_sweep(P.sweep(-1e6, 1e6, 300000001.0, amplitude=0.3, mix=True))
            b.process_raw_device(buf.ptr + 2 * k * sf, sf, P.binding.IQ_S8, P.binding.IQO_QI)
            b.synchronize()
            tap, _ = b.tap(P.TAP_RAW_IQ)
            assert tap.shape == (1, sf)
            want.append(np.stack([P.iq_record_convert(row) for row in tap]))
        names = []
        for k in range(K):
            if k == 3:
                a.set_testbench_sweep(P.sweep(-1e6, 1e6, 300000001.0, amplitude=0.3, mix=True))
            a.process_raw_device(buf.ptr + 2 * k * sf, sf, P.binding.IQ_S8, P.binding.IQO_QI)
            names.append(a.kernel_name(2))
        assert names[1] == names[2] == "k_mix_hb11_lean" and names[3].startswith("k_testbench + "), names  # beside the transform; staged
        got = read_blocks(a.record_next, a.record_release, K)
        for k, (c_idx, dropped, blk) in enumerate(got):
            assert (c_idx, dropped) == (k, 0) and blk.shape == (1, sf, 2)
            assert np.array_equal(blk, want[k]), "call %d" % k
        assert all_differ(want)
        assert want[0][0, 0].tolist() == [-32767, int(np.trunc(np.float64(np.float32(127 / 128)) * 32767))]  # QI: (127, -128) is Q, I
        # the generator's call is the raw samples plus the sweep, not the raw samples alone
        plain = P.iq_record_convert((q[3 * sf:, 1].astype(np.float32) + 1j * q[3 * sf:, 0].astype(np.float32)) / np.float32(128))
        assert np.array_equal(want[2][0], P.iq_record_convert((q[2 * sf:3 * sf, 1].astype(np.float32) + 1j * q[2 * sf:3 * sf, 0].astype(np.float32)) / np.float32(128)))
        assert not np.array_equal(want[3][0], plain)
        assert np.array_equal(a.audio(), b.audio()) and np.array_equal(a.spectrum(), b.spectrum())
        a.record_close()
    finally:
        buf.free()
        a.close()
        b.close()


# 2b. rows that are not 16-byte aligned: a resampled bank's odd row pitch sends rows 1, 3, .. through the sample-by-sample loads
@pytest.mark.parametrize("fmt_name", ["F32", "S16_MONO"])
def test_unaligned_rows_of_a_resampled_bank(gpu_lib, fmt_name):
    import ctypes as C
    import pebblesdr_amd as P
    fmt = {"F32": P.AUDIO_F32, "S16_MONO": P.AUDIO_S16_MONO}[fmt_name]
    a = P.ReceiverBank(FS, 3, True, False, 0, audio_rate=11025)
    b = P.ReceiverBank(FS, 3, True, False, 0, audio_rate=11025)
    K = 3
    bufs = upload_calls(P, stream5(K, seed=17), [1] * K)
    sel, levels = [2, 1, 0], {1: (37.0, False), 0: (250.0, False)}
    try:
        for rx in (a, b):
            tune5(P, rx, 3)
        a.audio_out_open(fmt, sel, 4)
        for ch, (g, m) in levels.items():
            a.set_audio_level(ch, g, m)
        want = []
        for buf, n in bufs:
            b.process_device(buf.ptr, n)
            b.synchronize()
            want.append(expected_block(P, fmt, b.audio(), levels, sel))
        na, pitch = C.c_uint64(), C.c_uint64()
        for buf, n in bufs:
            a.process_device(buf.ptr, n)
        p = a.L.pebblegpu_receiver_audio(a.h, C.byref(na), C.byref(pitch))
        assert pitch.value % 2 == 1 and p % 16 == 0, (pitch.value, p)  # so row 1 starts 8 bytes off a 16-byte boundary
        got = read_blocks(a.audio_out_next, a.audio_out_release, K)
        for k, (call, dropped, blk) in enumerate(got):
            assert (call, dropped) == (k, 0) and blk.shape == want[k].shape and blk.shape[1] > 300
            assert np.array_equal(blk, want[k]), "call %d" % k
            assert all(want[k][r].any() for r in range(3))
        assert all_differ(want)
    finally:
        free_all(bufs, a, b)


# 9. refusals return their code before anything is queued, and the handle keeps working
def test_refusals_leave_the_handle_usable(gpu_lib):
    import pebblesdr_amd as P
    a = P.ReceiverBank(FS, 1, True, False, 4096)
    b = P.ReceiverBank(FS, 1, True, False, 4096)
    K = 3
    n = K * SF
    t = np.arange(n) / FS
    x = (0.1 * np.exp(2j * np.pi * (100e3 + 1300.0) * t) + lcg_noise(n, 5, 1e-4)).astype(np.complex64)

    def refused(code, fn, *args):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*args)
        assert e.value.code == code, e.value

    try:
        for rx in (a, b):
            rx.set_mode(0, P.DM_USB); rx.set_mixer(0, 100e3); rx.set_bandpass(0, 300, 3000)
        refused(E_INVALID, a.audio_out_open, P.AUDIO_F32, [1], 4)        # out of range
        refused(E_INVALID, a.audio_out_open, P.AUDIO_F32, [0, 0], 4)     # duplicated
        refused(E_INVALID, a.audio_out_open, P.AUDIO_F32, None, 1)
        refused(E_INVALID, a.audio_out_open, P.AUDIO_F32, None, 9)
        refused(E_INVALID, a.audio_out_open, 3, None, 4)                 # unknown format
        refused(E_INVALID, a.record_open, 1)
        refused(E_INVALID, a.record_open, 9)
        refused(E_INVALID, a.audio_out_next, False)                      # not open
        refused(E_INVALID, a.set_audio_level, 0, -1.0, False)
        refused(E_INVALID, a.set_audio_level, 0, float("inf"), False)
        refused(E_INVALID, a.set_audio_level, 1, 50.0, False)
        a.audio_out_open(P.AUDIO_F32, None, 4)
        refused(E_INVALID, a.audio_out_open, P.AUDIO_F32, None, 4)       # second open
        assert a.audio_out_next(False) is None and a.audio_out_next(True) is None  # nothing queued: host == NULL
        refused(E_INVALID, a.audio_out_release, 0)                       # nothing handed out
        refused(E_UNSUPPORTED, a.process_iq, x[:NF].astype(np.complex128))
        a0, _ = a.process(x[:SF])
        b0, _ = b.process(x[:SF])
        a1, _ = a.process(x[SF:2 * SF])
        b1, _ = b.process(x[SF:2 * SF])
        refused(E_INVALID, a.audio_out_release, 0)                       # queued, but not handed out yet
        c0, d0, blk0 = a.audio_out_next(True)
        c1, d1, blk1 = a.audio_out_next(False)                           # (a.process has synchronised: the copy is over)
        assert (c0, d0, c1, d1) == (0, 0, 1, 0)
        refused(E_INVALID, a.audio_out_release, 1)                       # out of order
        a.audio_out_release(0)
        refused(E_INVALID, a.audio_out_release, 0)
        a.audio_out_release(1)
        assert np.array_equal(blk0[0], P.audio_out_convert(P.AUDIO_F32, 100.0, False, b0[0]))
        assert np.array_equal(blk1[0], P.audio_out_convert(P.AUDIO_F32, 100.0, False, b1[0]))
        assert np.array_equal(a0, b0) and np.array_equal(a1, b1) and a0.any() and not np.array_equal(a0, a1)
        a.audio_out_close()
        refused(E_INVALID, a.audio_out_close)
        a2, _ = a.process(x[2 * SF:])                                    # the existing read path, as before
        b2, _ = b.process(x[2 * SF:])
        assert np.array_equal(a2, b2) and a2.any()
        assert len(a.process_iq(x[:NF].astype(np.complex128))[0]) == 0   # accepted again
    finally:
        a.close()
        b.close()
