"""GPU tier (-m gpu): the stream bank's two egress rings (pebblegpu_streambank_iq_out_*, pebblegpu_streambank_display_*).

What a block must hold is what the bank already computes, so the reference is a twin bank without rings, fed the same calls and
read the old way (filtered / spectrum / map_spectrum behind a synchronize): blocks equal its rows BIT FOR BIT -- the packing kernels
move or map, they add no arithmetic of their own.  The two rules that are the rings' own are held to their restatements exactly:
PCM16 to pebblegpu_iq_record_convert (WavFile::WriteSamples, tests/test_audio_out_host.py pins the twin), colours to
tests/waterfall_ref.py.  Pixels additionally pass tests.test_screen_map_gpu.check against the numpy restatement of
FFT::mapFFTToScreen, with that function's own allowance and nothing wider.

Shape A: 5 streams, 2048-sample frames, 4096 bins, at most 6 frames per call; calls of 1, 3, 6, 2 (and 3) frames, the third without
the band-pass.  Shape B: 65536 / 65536 with 3 streams.  Inputs differ per stream and per call, so a stale or misplaced row shows.
"""
import functools
import threading

import numpy as np
import pytest

from tests import waterfall_ref as W
from tests.signals import lcg_noise, tones
from tests.test_screen_map_gpu import check as check_map, ranges, spectrum_signal
from tests.test_streambank_raw_gpu import GAIN, host_convert, make_raw

pytestmark = pytest.mark.gpu

E_INVALID, E_SIZE = -1, -5
FS, FRAME, BINS, SA, FA = 2.0e6, 2048, 4096, 5, 6
N65 = 65536
CALLS = [(1, 3), (3, 3), (6, 2), (2, 3), (3, 3)]   # (frames, what)
SEL = [3, 0, 4]
LOUD = 3                                           # the stream whose pass-band tone has amplitude 1.5
XP = 301                                           # not a multiple of 4
RANGES = ranges(FS)


def make_bank(P, S=SA, frame=FRAME, bins=BINS, F=FA, ups=None):
    sb = P.StreamBank(FS, S, frame=frame, spectrum_bins=bins, max_frames=F)
    for c in range(S):
        sb.set_bandpass(c, -50e3 - 1e3 * c, 50e3 + 2e3 * c)
    if ups is not None:
        sb.set_spectrum_updates(ups)
    return sb


@functools.lru_cache(maxsize=None)
def inputs_a():
    """one [SA, frames * FRAME] complex64 per call: display tones and noise with a seed per (call, stream), plus a pass-band tone"""
    out = []
    for k, (frames, _) in enumerate(CALLS):
        n = frames * FRAME
        x = np.stack([spectrum_signal(FS, n, 1000 + 37 * k + s) + tones(FS, n, [(1.5 if s == LOUD else 0.3, 10e3 + 3e3 * s, 0.4 * k)])
                      + lcg_noise(n, 5000 + 11 * k + s, 1e-2) for s in range(SA)]).astype(np.complex64)
        x.setflags(write=False)
        out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def twin_a():
    """the calls of shape A through a bank that never heard of rings, read after every call (computed once, shared, read-only):
    per call (filtered or None, spectrum rows [SA, frames, BINS] or None, {range index: pixels at y 255, x XP, every row})"""
    import pebblesdr_amd as P
    sb = make_bank(P)
    out = []
    for x, (frames, what) in zip(inputs_a(), CALLS):
        y, s = sb.process(x, what)
        px = {}
        if what & 2:
            for i, (lo, hi) in enumerate(RANGES):
                px[i] = sb.map_spectrum(255, XP, 0.0, -120.0, lo, hi, first_frame=0, n_frames=frames)
                px[i].setflags(write=False)
            s.setflags(write=False)
        if y is not None:
            y.setflags(write=False)
        out.append((y, s, px))
    sb.close()
    return out


def upload(P, xs):
    return [P.DeviceBuffer.from_array(P.binding.to_f32_iq(x), 0) for x in xs]


def queue_calls(sb, bufs, calls):
    """the calls back to back: nothing waits on the host in between"""
    for b, (frames, what) in zip(bufs, calls):
        sb.process_device(b.ptr, frames * sb.frame, what)


def as_c64(block):
    """an F32 IQ block [rows, n, 2] as complex64 [rows, n]"""
    return np.ascontiguousarray(block).view(np.complex64)[:, :, 0]


def take_iq(sb, expect_call, dropped_before=0):
    got = sb.iq_out_next(True)
    assert got is not None, "no IQ block %d" % expect_call
    call, dropped, rows = got
    assert (call, dropped) == (expect_call, dropped_before)
    sb.iq_out_release(call)
    return rows


def take_display(sb, expect_call, dropped_before=0):
    got = sb.display_next(True)
    assert got is not None, "no display block %d" % expect_call
    call, dropped, first, rows = got
    assert (call, dropped) == (expect_call, dropped_before)
    sb.display_release(call)
    return first, rows


def iq_ring_case(P, fmt, n_calls=4):
    """test 1's body: the first n_calls calls of shape A through a bank with the IQ ring open on SEL"""
    ref = twin_a()
    sb = make_bank(P)
    sb.iq_out_open(fmt, SEL, n_slots=4)
    bufs = upload(P, inputs_a()[:n_calls])
    try:
        queue_calls(sb, bufs, CALLS[:n_calls])
        for k in range(n_calls):
            frames, what = CALLS[k]
            rows = take_iq(sb, k)
            if not what & 1:
                assert rows.shape == (len(SEL), 0, 2)      # a block of 0 samples, with the next index
                continue
            want = ref[k][0][SEL]
            assert np.abs(want).max() > 0.1
            if fmt == P.AUDIO_F32:
                assert rows.dtype == np.float32 and np.array_equal(as_c64(rows).view(np.uint32), want.view(np.uint32))
            else:
                assert rows.dtype == np.int16 and rows.shape == (len(SEL), frames * FRAME, 2)
                conv = np.stack([P.iq_record_convert(w) for w in want])
                assert np.array_equal(rows, conv)
                loud = rows[SEL.index(LOUD)].astype(np.int32)
                assert (loud == 32767).any() and (loud == -32767).any() and (np.abs(loud) < 32000).any()   # the saturating branch runs
                assert np.abs(rows[SEL.index(0)].astype(np.int32)).max() < 32767
        assert sb.iq_out_next(False) is None and sb.iq_out_dropped() == 0
        sb.iq_out_close()
    finally:
        for b in bufs:
            b.free()
        sb.close()


# 1
def test_iq_ring_f32_and_s16(gpu_lib):
    import pebblesdr_amd as P
    iq_ring_case(P, P.AUDIO_F32)
    iq_ring_case(P, P.AUDIO_S16)


def test_an_open_ring_changes_nothing(gpu_lib):
    """a bank's own outputs with both rings open, and those of a bank whose rings were opened and closed again, equal the outputs of
    the bank that never heard of rings; so do the routes"""
    import pebblesdr_amd as P
    ref = twin_a()
    a, b, plain = make_bank(P), make_bank(P), make_bank(P)
    a.iq_out_open(P.AUDIO_S16, SEL, n_slots=2)
    a.display_open(P.DISPLAY_WATERFALL_ARGB32, P.screen_map(255, XP, 0.0, -120.0, *RANGES[0]), [1], 1, 2)
    b.iq_out_open(P.AUDIO_F32, None, n_slots=2)
    b.display_open(P.DISPLAY_DB_F32, None, None, 0, 2)
    b.iq_out_close()
    b.display_close()
    try:
        for k, (x, (frames, what)) in enumerate(zip(inputs_a(), CALLS)):
            yp, sp_ = plain.process(x, what)
            names = (plain.kernel_name(1), plain.kernel_name(2))
            for sb in (a, b):
                y, s = sb.process(x, what)
                assert (sb.kernel_name(1), sb.kernel_name(2)) == names
                assert list(sb.spectrum_frames()) == list(plain.spectrum_frames())
                if what & 1:
                    assert np.array_equal(y, ref[k][0]) and np.array_equal(yp, ref[k][0])
                if what & 2:
                    assert np.array_equal(s, ref[k][1]) and np.array_equal(sp_, ref[k][1])
                    assert np.array_equal(sb.map_spectrum(255, XP, 0.0, -120.0, *RANGES[1], first_frame=0, n_frames=frames), ref[k][2][1])
        assert a.iq_out_dropped() == len(CALLS) - 2 and a.display_dropped() == len(CALLS) - 2   # nothing was read: the rings only dropped
    finally:
        for sb in (a, b, plain):
            sb.close()


def display_case(P, fmt, ri, max_rows=0, n_calls=4):
    """the first n_calls calls of shape A through a bank with the display ring open on SEL -> [(first_row, rows)] per call"""
    sb = make_bank(P)
    screen = None if fmt == P.DISPLAY_DB_F32 else P.screen_map(255, XP, 0.0, -120.0, *RANGES[ri])
    sb.display_open(fmt, screen, SEL, max_rows, n_slots=4)
    bufs = upload(P, inputs_a()[:n_calls])
    try:
        queue_calls(sb, bufs, CALLS[:n_calls])
        out = [take_display(sb, k) for k in range(n_calls)]
        assert sb.display_next(False) is None and sb.display_dropped() == 0
        sb.display_close()
        return out
    finally:
        for b in bufs:
            b.free()
        sb.close()


def check_db_blocks(P, blocks, max_rows=0):
    ref = twin_a()
    for k, (first, rows) in enumerate(blocks):
        frames = CALLS[k][0]
        keep = min(frames, max_rows) if max_rows else frames
        assert first == frames - keep and rows.dtype == np.float32 and rows.shape == (len(SEL), keep, BINS)
        want = ref[k][1][SEL][:, first:]
        assert want.max() > -100.0 and np.array_equal(rows.view(np.uint32), want.view(np.uint32))


# 2
def test_display_ring_db_rows_and_max_rows(gpu_lib):
    import pebblesdr_amd as P
    check_db_blocks(P, display_case(P, P.DISPLAY_DB_F32, 0))
    for max_rows in (1, 2):
        check_db_blocks(P, display_case(P, P.DISPLAY_DB_F32, 0, max_rows), max_rows)


@pytest.mark.parametrize("ri", range(len(RANGES)))
def test_display_ring_pixels_and_waterfall(gpu_lib, ri):
    import pebblesdr_amd as P
    ref = twin_a()
    lo, hi = RANGES[ri]
    pix = display_case(P, P.DISPLAY_PIXELS_I32, ri)
    wf = display_case(P, P.DISPLAY_WATERFALL_ARGB32, ri)
    last = display_case(P, P.DISPLAY_PIXELS_I32, ri, max_rows=2)
    used = 0
    for k, (frames, what) in enumerate(CALLS[:4]):
        want = ref[k][2][ri][SEL]
        first, rows = pix[k]
        assert first == 0 and rows.dtype == np.int32 and rows.shape == (len(SEL), frames, XP)
        assert np.array_equal(rows, want)                                         # map_spectrum's values, bit for bit
        used += check_map(rows, ref[k][1][SEL], BINS, FS, 255, XP, 0.0, -120.0, lo, hi, "range %d call %d" % (ri, k))
        first, colours = wf[k]
        assert first == 0 and colours.dtype == np.uint32 and np.array_equal(colours, W.waterfall(want))
        first, rows2 = last[k]
        assert first == max(0, frames - 2) and np.array_equal(rows2, want[:, first:])
    if ri < 3:
        assert len(np.unique(np.concatenate([p[1].reshape(-1) for p in pix]))) > 8   # a real plot, not a constant
    print("range %d: %d tolerated pixels" % (ri, used))


# 3
def test_under_the_update_gate(gpu_lib):
    """250 spectra per second at 1.024 ms per frame: every fourth frame or so, so several calls select nothing"""
    import pebblesdr_amd as P
    ref = twin_a()
    sb, twin = make_bank(P, ups=250), make_bank(P, ups=250)
    sb.iq_out_open(P.AUDIO_F32, SEL, n_slots=8)
    sb.display_open(P.DISPLAY_DB_F32, None, SEL, 0, n_slots=8)
    bufs = upload(P, inputs_a())
    try:
        counts = []
        for b, (frames, what) in zip(bufs, CALLS):
            sb.process_device(b.ptr, frames * FRAME, what)
            counts.append(len(sb.spectrum_frames()))          # known on the host the moment the call returns: no wait
        assert 0 in counts and max(counts) >= 2 and len(counts) == len(CALLS)
        seen = set()
        for k, (x, (frames, what)) in enumerate(zip(inputs_a(), CALLS)):
            yt, st = twin.process(x, what)
            assert len(twin.spectrum_frames()) == counts[k]
            first, rows = take_display(sb, k)
            assert first == 0 and rows.shape == (len(SEL), counts[k], BINS)      # 0 rows included: nothing is repeated
            if counts[k]:
                assert np.array_equal(rows.view(np.uint32), st[SEL].view(np.uint32))   # the twin's compact rows
                for r in rows.reshape(-1, BINS):
                    assert r.tobytes() not in seen
                    seen.add(r.tobytes())
            iq = take_iq(sb, k)
            if what & 1:
                assert np.array_equal(as_c64(iq), yt[SEL]) and np.array_equal(yt, ref[k][0])   # the gate leaves the band-pass alone
            else:
                assert iq.shape[1] == 0
        sb.iq_out_close()
        sb.display_close()
    finally:
        for b in bufs:
            b.free()
        sb.close()
        twin.close()


# 4
def test_shape_b_both_rings_float2_and_raw(gpu_lib):
    import pebblesdr_amd as P
    S, F, fmt, order = 3, 2, 0, 0
    calls = [(2, 3), (1, 3)]
    sel, dsel = [2, 0], [1, 2]
    raw = make_raw(fmt, S, 3 * N65, 77)
    x = host_convert(raw, fmt, order, GAIN[fmt])
    lo, hi = -int(FS // 2), int(FS // 2)
    f2, rw, twin = (make_bank(P, S, N65, N65, F) for _ in range(3))
    for sb in (f2, rw):
        sb.iq_out_open(P.AUDIO_F32, sel, n_slots=2)
        sb.display_open(P.DISPLAY_PIXELS_I32, P.screen_map(255, 1024, 0.0, -120.0, lo, hi), dsel, 0, n_slots=2)
    xs, rs, at = [], [], 0
    for frames, _ in calls:
        xs.append(np.ascontiguousarray(x[:, at:at + frames * N65]))
        rs.append(np.ascontiguousarray(raw[:, at:at + frames * N65]))
        at += frames * N65
    xb, rb = upload(P, xs), [P.DeviceBuffer.from_array(r, 0) for r in rs]
    try:
        names = []
        for k, (frames, what) in enumerate(calls):
            f2.process_device(xb[k].ptr, frames * N65, what)
            rw.process_raw_device(rb[k].ptr, frames * N65, fmt, order, GAIN[fmt], what)
            names.append((f2.kernel_name(1), f2.kernel_name(2), rw.kernel_name(1), rw.kernel_name(2)))
        assert names == [("k_fastfir_t128", "k_big256_cols + k_big256_rows", "k_fastfir_t128 (raw s8)", "k_big256_cols (raw s8) + k_big256_rows")] * 2
        for k, (frames, what) in enumerate(calls):
            yt, st = twin.process(xs[k], what)
            assert (twin.kernel_name(1), twin.kernel_name(2)) == names[k][:2]           # the same strings as without rings
            pt = twin.map_spectrum(255, 1024, 0.0, -120.0, lo, hi, first_frame=0, n_frames=frames)
            iq_f, iq_r = take_iq(f2, k), take_iq(rw, k)
            assert np.abs(yt).max() > 1e-3 and np.array_equal(as_c64(iq_f), yt[sel])
            assert np.array_equal(iq_r.view(np.uint32), iq_f.view(np.uint32))             # raw route = float2 route, bit for bit
            (first_f, px_f), (first_r, px_r) = take_display(f2, k), take_display(rw, k)
            assert first_f == first_r == 0 and px_f.shape == (2, frames, 1024)
            assert np.array_equal(px_f, pt[dsel]) and np.array_equal(px_r, px_f)
            assert len(np.unique(px_f)) > 8
            check_map(px_f, st[dsel], N65, FS, 255, 1024, 0.0, -120.0, lo, hi, "65536 bins onto 1024 pixels, call %d" % k)
    finally:
        for b in xb + rb:
            b.free()
        for sb in (f2, rw, twin):
            sb.close()


# 5
def test_side_by_side_route(gpu_lib, monkeypatch):
    """PEBBLEGPU_SB_SIDE=1 (read when the bank is created): the band-pass runs on the second stream, the packing kernels behind the join"""
    import pebblesdr_amd as P
    twin_a()                                        # (the reference is the default route's, made before the switch is set)
    monkeypatch.setenv("PEBBLEGPU_SB_SIDE", "1")
    iq_ring_case(P, P.AUDIO_F32)
    check_db_blocks(P, display_case(P, P.DISPLAY_DB_F32, 0))


# 6
def test_a_full_ring_drops_and_counts(gpu_lib):
    import pebblesdr_amd as P
    ref = twin_a()
    sb = make_bank(P)
    sb.iq_out_open(P.AUDIO_F32, SEL, n_slots=2)
    sb.display_open(P.DISPLAY_DB_F32, None, SEL, 0, n_slots=2)
    bufs = upload(P, inputs_a())
    try:
        queue_calls(sb, bufs[:4], CALLS[:4])                  # nothing released: calls 2 and 3 find the rings full
        assert sb.iq_out_dropped() == 2 and sb.display_dropped() == 2
        held = [sb.iq_out_next(True), sb.iq_out_next(True)]
        assert [h[0] for h in held] == [0, 1] and sb.iq_out_next(True) is None
        dheld = [sb.display_next(True), sb.display_next(True)]
        assert [h[0] for h in dheld] == [0, 1] and sb.display_next(True) is None
        for k in (0, 1):
            assert held[k][1] == 0 and np.array_equal(as_c64(held[k][2]), ref[k][0][SEL])
            assert dheld[k][1] == 0 and dheld[k][2] == 0 and np.array_equal(dheld[k][3], ref[k][1][SEL])
            sb.iq_out_release(k)
            sb.display_release(k)
        queue_calls(sb, bufs[4:], CALLS[4:])                   # call 4: delivered, and it says what went missing before it
        assert np.array_equal(as_c64(take_iq(sb, 4, dropped_before=2)), ref[4][0][SEL])   # (the dropped calls' band-pass still ran: the overlap went on)
        first, rows = take_display(sb, 4, dropped_before=2)
        assert first == 0 and np.array_equal(rows, ref[4][1][SEL])
        assert sb.iq_out_dropped() == 2 and sb.display_dropped() == 2
    finally:
        for b in bufs:
            b.free()
        sb.close()                                             # (destroy closes the open rings)


# 7
def test_ingest_slots_in_rings_out_no_host_wait(gpu_lib):
    """K calls through the pinned ingest slots with both rings open and a reader on another thread; the producer calls no synchronize
    until after the last call.  The two threads talk through host-side counters only (no device wait): the reader takes block k once
    call k has been queued (_next does not wait for a block that no call has queued yet), and the producer stays at most 4 calls
    ahead of the reader, so with 4 slots nothing can be dropped whatever the threads' timing."""
    import pebblesdr_amd as P
    K, frames, fmt, order = 8, 2, 0, 1
    n = frames * FRAME
    raw = make_raw(fmt, SA, K * n, 91)
    sb, twin = make_bank(P), make_bank(P)
    screen = P.screen_map(255, XP, 0.0, -120.0, *RANGES[0])
    sb.iq_out_open(P.AUDIO_S16, SEL, n_slots=4)
    sb.display_open(P.DISPLAY_WATERFALL_ARGB32, screen, None, 1, n_slots=4)
    room, queued = threading.Semaphore(4), threading.Semaphore(0)
    got, errors = [], []

    def reader():
        try:
            for k in range(K):
                queued.acquire()
                iq = take_iq(sb, k)
                first, line = take_display(sb, k)
                got.append((iq, first, line))
                room.release()
        except BaseException as e:  # noqa: BLE001 (reported by the test's thread below)
            errors.append(e)
            for _ in range(K):
                room.release()

    th = threading.Thread(target=reader)
    th.start()
    try:
        for k in range(K):
            room.acquire()
            blk = np.ascontiguousarray(raw[:, k * n:(k + 1) * n])
            sb.ingest_acquire(k & 1, blk.nbytes, np.int8)[:] = blk.reshape(-1)
            sb.ingest_submit(k & 1, blk.nbytes)
            sb.process_ingested(k & 1, n, fmt, order, GAIN[fmt])
            queued.release()
        th.join()
        assert not errors, errors
        sb.synchronize()
        assert len(got) == K and sb.iq_out_dropped() == 0 and sb.display_dropped() == 0
        for k in range(K):
            buf = P.DeviceBuffer.from_array(np.ascontiguousarray(raw[:, k * n:(k + 1) * n]), 0)
            try:
                twin.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt])
                y = twin.filtered()
                px = twin.map_spectrum(255, XP, 0.0, -120.0, *RANGES[0])       # the last frame of each stream
            finally:
                buf.free()
            iq, first, line = got[k]
            assert np.array_equal(iq, np.stack([P.iq_record_convert(w) for w in y[SEL]]))
            assert first == frames - 1 and line.shape == (SA, 1, XP) and np.array_equal(line, W.waterfall(px))
    finally:
        for _ in range(K):
            queued.release()                                  # (a producer that failed must not leave the reader waiting)
        th.join()
        sb.close()
        twin.close()


# 8
def test_refusals_leave_the_handle_usable(gpu_lib):
    import pebblesdr_amd as P
    sb = make_bank(P)
    x = inputs_a()[1]
    good = P.screen_map(255, XP, 0.0, -120.0, *RANGES[0])

    def still_works(ring):
        sb.process(x, 3)
        if ring == "iq":
            sb.iq_out_open(P.AUDIO_F32, [1], n_slots=2)
            sb.iq_out_close()
        else:
            sb.display_open(P.DISPLAY_PIXELS_I32, good, [1], 1, n_slots=2)
            sb.display_close()

    def refused(ring, code, fn, *a):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*a)
        assert e.value.code == code, e.value
        still_works(ring)

    try:
        for streams in ([1, 1], [0, SA], [], [2, 0, 2]):
            refused("iq", E_INVALID, sb.iq_out_open, P.AUDIO_F32, streams, 4)
            refused("display", E_INVALID, sb.display_open, P.DISPLAY_DB_F32, None, streams, 0, 4)
        for slots in (0, 1, 9):
            refused("iq", E_INVALID, sb.iq_out_open, P.AUDIO_F32, None, slots)
            refused("display", E_INVALID, sb.display_open, P.DISPLAY_DB_F32, None, None, 0, slots)
        for fmt in (P.AUDIO_S16_MONO, 3, -1):
            refused("iq", E_INVALID, sb.iq_out_open, fmt, None, 4)
        for fmt in (3, -1):
            refused("display", E_INVALID, sb.display_open, fmt, good, None, 0, 4)
        for fmt in (P.DISPLAY_PIXELS_I32, P.DISPLAY_WATERFALL_ARGB32):
            refused("display", E_INVALID, sb.display_open, fmt, None, None, 0, 4)                                          # no map
            refused("display", E_INVALID, sb.display_open, fmt, P.screen_map(255, 0, 0.0, -120.0, *RANGES[0]), None, 0, 4)
            refused("display", E_INVALID, sb.display_open, fmt, P.screen_map(0, XP, 0.0, -120.0, *RANGES[0]), None, 0, 4)
            refused("display", E_INVALID, sb.display_open, fmt, P.screen_map(255, XP, -50.0, -50.0, *RANGES[0]), None, 0, 4)
        refused("display", E_INVALID, sb.display_open, P.DISPLAY_WATERFALL_ARGB32, P.screen_map(600, XP, 0.0, -120.0, *RANGES[0]), None, 0, 4)
        short = P.screen_map(255, XP, 0.0, -120.0, *RANGES[0])
        short.struct_size = 8
        refused("display", E_INVALID, sb.display_open, P.DISPLAY_PIXELS_I32, short, None, 0, 4)

        # a second open of the same ring; release out of order; close, then another selection
        sb.iq_out_open(P.AUDIO_F32, SEL, n_slots=4)
        sb.display_open(P.DISPLAY_DB_F32, None, SEL, 0, n_slots=4)
        for fn, a in ((sb.iq_out_open, (P.AUDIO_S16, None, 4)), (sb.display_open, (P.DISPLAY_DB_F32, None, None, 0, 4))):
            with pytest.raises(P.PebbleGpuError) as e:
                fn(*a)
            assert e.value.code == E_INVALID
        y0, s0 = sb.process(x, 3)
        y1, s1 = sb.process(x, 3)
        for nxt, rel in ((sb.iq_out_next, sb.iq_out_release), (sb.display_next, sb.display_release)):
            with pytest.raises(P.PebbleGpuError) as e:
                rel(0)                                   # nothing has been handed out yet
            assert e.value.code == E_INVALID
            assert nxt(True)[0] == 0 and nxt(True)[0] == 1
            for bad in (1, 2, 7):
                with pytest.raises(P.PebbleGpuError) as e:
                    rel(bad)                             # block 0 is the oldest handed out
                assert e.value.code == E_INVALID
            rel(0)
            with pytest.raises(P.PebbleGpuError):
                rel(0)
            rel(1)
        sb.iq_out_close()
        sb.display_close()
        for fn in (sb.iq_out_close, sb.display_close, sb.iq_out_dropped, sb.display_dropped, lambda: sb.iq_out_next(False), lambda: sb.display_next(False)):
            with pytest.raises(P.PebbleGpuError) as e:
                fn()                                     # not open any more
            assert e.value.code == E_INVALID
        sb.iq_out_open(P.AUDIO_F32, [4, 1], n_slots=2)
        sb.display_open(P.DISPLAY_DB_F32, None, [0, 2, 1], 1, n_slots=2)
        y2, s2 = sb.process(x, 3)
        assert np.array_equal(as_c64(take_iq(sb, 0)), y2[[4, 1]])               # indices count from the new open
        first, rows = take_display(sb, 0)
        assert first == s2.shape[1] - 1 and np.array_equal(rows, s2[[0, 2, 1]][:, -1:])
        with pytest.raises(P.PebbleGpuError):
            sb.process(x[:, :1000], 3)                   # a refused call (not a multiple of the frame): no block, no index
        sb.process(x, 0)
        assert take_iq(sb, 1).shape[1] == 0 and take_display(sb, 1)[1].shape[1] == 0
    finally:
        sb.close()
    nos = P.StreamBank(FS, 2, frame=FRAME, spectrum_bins=0, max_frames=2)   # created without a spectrum of its own choosing
    try:
        with pytest.raises(P.PebbleGpuError) as e:
            nos.display_open(P.DISPLAY_DB_F32, None, None, 0, 4)
        assert e.value.code == E_INVALID
        nos.iq_out_open(P.AUDIO_F32, None, n_slots=2)
        nos.iq_out_close()
    finally:
        nos.close()


def test_a_ring_above_one_gib_of_pinned_memory_is_refused(gpu_lib):
    """128 streams x 6 frames of 65536: an F32 IQ slot of every stream is 384 MiB, a dB slot 192 MiB -- eight of either are past 1 GiB"""
    import pebblesdr_amd as P
    sb = P.StreamBank(FS, 128, frame=N65, spectrum_bins=N65, max_frames=6)
    try:
        for fn, a in ((sb.iq_out_open, (P.AUDIO_F32, None, 8)), (sb.display_open, (P.DISPLAY_DB_F32, None, None, 0, 8))):
            with pytest.raises(P.PebbleGpuError) as e:
                fn(*a)
            assert e.value.code == E_SIZE, e.value
        sb.iq_out_open(P.AUDIO_S16, [5, 100], n_slots=2)       # select fewer streams ...
        sb.display_open(P.DISPLAY_DB_F32, None, None, 1, n_slots=2)   # ... or a smaller max_rows
        sb.iq_out_close()
        sb.display_close()
    finally:
        sb.close()
