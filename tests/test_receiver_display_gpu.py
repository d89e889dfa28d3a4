"""GPU tier (-m gpu): the receiver's display ring (pebblegpu_receiver_display_*): one or two panes per block, unprocessed or zoomed
spectra, dB rows, FFT::mapFFTToScreen pixels or the waterfall's colours, through the pinned egress slots.

The method of tests/test_streambank_egress_gpu.py: a TWIN receiver that never opens a ring is fed the same calls and read the old way,
behind a synchronise after every call (spectrum / zoom_spectrum / map_spectrum / map_zoom_spectrum); the receiver under test queues its
calls back to back and reads its blocks afterwards.  A block must equal the twin: dB rows bit for bit, pixels bit for bit (one
computation, and each row's lanes add in the order the map functions use for that row), colours = tests/waterfall_ref.py of those
pixels.  The twin's pixels additionally pass tests.test_screen_map_gpu.check against tests/screen_map_ref.py, with that function's own
allowance.  Inputs differ per call and per channel, and every comparison asserts that the expected blocks differ from each other, so a
stale or misplaced row would show.

Shape 1: 20 Msps, one WFM channel, 8192 bins, 2048 zoomed bins, super-frames of 131072 samples (the side-by-side route; with
PEBBLEGPU_PIPELINE=1 the call's two pipelines end on different streams and each pane is packed where its source was written).
Shape 2: 2.048 Msps, 70 NFM channels -- more than one chunk of run_screen_map's 64 per-stream geometries -- with per-channel offsets
chosen so that the two chunks get DIFFERENT lane groups (asserted from the restatement's geometry)."""
import threading

import numpy as np
import pytest

from tests import screen_map_ref as R
from tests import waterfall_ref as W
from tests.signals import lcg_noise, tones
from tests.test_screen_map_gpu import check

pytestmark = pytest.mark.gpu

E_INVALID, E_SIZE, E_UNSUPPORTED = -1, -5, -6
FS1, BINS1, ZB, SF1 = 20_000_000, 8192, 2048, 131072
SIZES1 = [1, 2, 3, 1]
FS2, C2, SF2 = 2_048_000, 70, 65536
SIZES2 = [1, 3]
SEL2 = [69, 0, 64, 5, 63]
OFFS2 = [0 if c == 5 else (c * 37) % 401 - 200 for c in range(C2)]
ZOOMS2 = {"averaged": 1.0, "repeated": 0.1}


class Pane:
    """one pane's request, and what a block of it must hold given the twin"""

    def __init__(self, zoomed, fmt, sel=None, max_rows=0, y=255, x=301, max_db=0.0, min_db=-120.0, start=0, stop=0, zoom=1.0, offs=None):
        self.zoomed, self.fmt, self.sel, self.max_rows = zoomed, fmt, sel, max_rows
        self.y, self.x, self.max_db, self.min_db, self.start, self.stop, self.zoom, self.offs = y, x, max_db, min_db, start, stop, zoom, offs

    def c(self, P, with_map=True):
        screen = P.screen_map(self.y, self.x, self.max_db, self.min_db, self.start, self.stop) if with_map else None
        return P.display_pane(P.PANE_ZOOM if self.zoomed else P.PANE_SPECTRUM, self.fmt, screen, self.zoom, self.offs, self.sel, self.max_rows)

    def expected(self, P, b, db, what):
        """db: the twin's rows of this pane's source for the call just made, [sources, F, bins] -> (first_row, rows as the block holds them)"""
        F = db.shape[1]
        k = min(F, self.max_rows) if self.max_rows else F
        first = F - k
        sel = list(range(db.shape[0])) if self.sel is None else self.sel
        if self.fmt == P.DISPLAY_DB_F32:
            return first, db[sel][:, first:]
        if k == 0:  # (the pull interface would map a carried row here: the ring never delivers one)
            px = np.zeros((len(sel), 0, self.x), dtype=np.int32)
        elif self.zoomed:
            px = b.map_zoom_spectrum(self.y, self.x, self.max_db, self.min_db, self.zoom, self.offs, first_frame=first, n_frames=k)[sel]
        else:
            px = b.map_spectrum(self.y, self.x, self.max_db, self.min_db, self.start, self.stop, first_frame=first, n_frames=k)[sel]
        rate = float(b.info.demod_rate_int) if self.zoomed else float(b.fs)  # (b.fs: set by rx1 / rx2 below)
        for r, s in enumerate(sel if k else []):
            start, stop = R.zoom_edges(int(rate), self.zoom, self.offs[s] if self.offs else 0) if self.zoomed else (self.start, self.stop)
            check(px[r], db[s, first:], db.shape[2], rate, self.y, self.x, self.max_db, self.min_db, start, stop, "%s row %d (source %d)" % (what, r, s))
        return first, (W.waterfall(px) if self.fmt == P.DISPLAY_WATERFALL_ARGB32 else px)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def all_differ(arrays):
    arrays = [a for a in arrays if a.size]
    return len({np.ascontiguousarray(a).tobytes() for a in arrays}) == len(arrays)


def upload_calls(P, x, sizes, unit):
    bufs, pos = [], 0
    for k in sizes:
        bufs.append((P.DeviceBuffer.from_array(P.binding.to_f32_iq(x[..., pos * unit:(pos + k) * unit]), 0), k * unit))
        pos += k
    return bufs


def twin_call(P, b, buf, n, panes, what):
    """one call of the twin, read the old way -> what the ring's block of that call must hold, and the call's audio and route"""
    b.process_device(buf.ptr, n)
    b.synchronize()
    spec = b.spectrum() if b.bins else None
    zoom = b.zoom_spectrum()
    return dict(panes=[pn.expected(P, b, zoom if pn.zoomed else spec, "%s pane %d" % (what, i)) for i, pn in enumerate(panes)],
                audio=b.audio(), names=[b.kernel_name(w) for w in range(1, 6)], spec=spec, zoom=zoom,
                frames=(list(b.spectrum_frames()) if b.bins else [], list(b.spectrum_frames(zoomed=True))))


def take(a, call, dropped=0):
    blk = a.display_next(True)
    assert blk is not None, "no block for call %d" % call
    c, d, panes = blk
    assert (c, d) == (call, dropped)
    a.display_release(c)
    return panes


def assert_block(got, want, what):
    assert len(got) == len(want["panes"])
    for i, ((first, arr), (wfirst, warr)) in enumerate(zip(got, want["panes"])):
        assert first == wfirst, "%s pane %d: first_row %d, twin %d" % (what, i, first, wfirst)
        assert arr.shape == warr.shape and arr.dtype == warr.dtype, "%s pane %d: %s %s, twin %s %s" % (what, i, arr.shape, arr.dtype, warr.shape, warr.dtype)
        assert same_bits(arr, warr), "%s pane %d: %d of %d elements differ" % (what, i, int((arr != warr).sum()), arr.size)


def audio_rows(P, twin_audio):
    return np.stack([P.audio_out_convert(P.AUDIO_F32, 100.0, False, row) for row in twin_audio])


# ---- shape 1 ----
def rx1(P):
    rx = P.ReceiverBank(FS1, 1, True, True, BINS1, max_superframes=3, hires_bins=ZB)
    assert rx.superframe == SF1
    rx.fs = FS1
    rx.set_mixer(0, 1.0e6)
    return rx


def stream1(n_sf, seed=13):
    """an unmodulated carrier that steps by 200 kHz every super-frame over noise: no two super-frames, and no two calls, alike"""
    n = n_sf * SF1
    t = np.arange(n) / FS1
    return (0.4 * np.exp(1j * (2 * np.pi * (0.7e6 + 2e5 * np.floor(np.arange(n) / SF1)) * t)) + lcg_noise(n, seed, 1e-2)).astype(np.complex64)


def panes1(P):
    """bottom: the unprocessed spectrum's waterfall, 301 pixels (not a multiple of 4), the last 5 rows; top: the zoomed plot"""
    return [Pane(False, P.DISPLAY_WATERFALL_ARGB32, max_rows=5, x=301, start=-3_000_000, stop=4_000_000),
            Pane(True, P.DISPLAY_PIXELS_I32, y=600, x=699, zoom=0.5)]


@pytest.fixture(scope="module")
def shape1(gpu_lib):
    """the calls of shape 1 on the device and the twin's answer to each, computed once (read-only from then on)"""
    import pebblesdr_amd as P
    bufs = upload_calls(P, stream1(sum(SIZES1)), SIZES1, SF1)
    b = rx1(P)
    try:
        want = [twin_call(P, b, buf, n, panes1(P), "shape 1 call %d" % k) for k, (buf, n) in enumerate(bufs)]
    finally:
        b.close()
    yield bufs, want
    for buf, _ in bufs:
        buf.free()


@pytest.mark.parametrize("pipeline", [False, True])
def test_shape1_two_panes_queued_back_to_back(gpu_lib, shape1, monkeypatch, pipeline):
    import pebblesdr_amd as P
    bufs, want = shape1
    if pipeline:
        monkeypatch.setenv("PEBBLEGPU_PIPELINE", "1")
    a = rx1(P)
    monkeypatch.delenv("PEBBLEGPU_PIPELINE", raising=False)
    try:
        a.audio_out_open(P.AUDIO_F32, None, 4)
        a.display_open([pn.c(P) for pn in panes1(P)], 4)
        names = []
        for buf, n in bufs:  # nothing waits on the host between these
            a.process_device(buf.ptr, n)
            names.append([a.kernel_name(w) for w in range(1, 6)])
        for k in range(len(bufs)):
            got = take(a, k)
            assert_block(got, want[k], "call %d" % k)
            F, ZF = SIZES1[k] * SF1 // 2048, want[k]["zoom"].shape[1]
            assert got[0][1].shape == (1, 5, 301) and got[0][0] == F - 5          # the last max_rows rows, and where they start
            assert got[1][1].shape == (1, ZF, 699) and got[1][0] == 0 and ZF != 5  # the panes' row counts differ
            call, dropped, audio = a.audio_out_next(True)
            assert (call, dropped) == (k, 0) and same_bits(audio, audio_rows(P, want[k]["audio"]))
            a.audio_out_release(call)
            assert names[k] == want[k]["names"], (k, names[k], want[k]["names"])   # the ring changes no call's route
        assert a.display_next(False) is None and a.display_dropped() == 0
        assert all_differ([w["panes"][0][1] for w in want]) and all_differ([w["panes"][1][1] for w in want])
        assert names[0][0] and names[0][1]
        a.display_close()
        with pytest.raises(P.PebbleGpuError) as e:
            a.display_next(False)
        assert e.value.code == E_INVALID
    finally:
        a.close()


def test_a_full_ring_drops_and_counts(gpu_lib, shape1):
    import pebblesdr_amd as P
    bufs, want = shape1
    a = rx1(P)
    try:
        a.display_open([pn.c(P) for pn in panes1(P)], 2)
        for buf, n in bufs:  # four calls, nothing released: calls 2 and 3 find both slots taken
            a.process_device(buf.ptr, n)
        first = [a.display_next(True), a.display_next(True)]
        assert [(blk[0], blk[1]) for blk in first] == [(0, 0), (1, 0)]
        assert a.display_next(True) is None and a.display_dropped() == 2
        for k in (0, 1):
            assert_block(first[k][2], want[k], "call %d" % k)
        # the twin never dropped anything: the chain's and the transforms' state do not depend on the reader
        assert same_bits(a.audio(), want[3]["audio"]) and same_bits(a.spectrum(), want[3]["spec"]) and same_bits(a.zoom_spectrum(), want[3]["zoom"])
        with pytest.raises(P.PebbleGpuError) as e:  # oldest first
            a.display_release(1)
        assert e.value.code == E_INVALID
        a.display_release(0)  # one slot free again: the next call is delivered, as call 4, and says two blocks were dropped before it
        a.process_device(bufs[0][0].ptr, bufs[0][1])
        call, dropped, panes = a.display_next(True)
        assert (call, dropped) == (4, 2) and a.display_dropped() == 2
        a.fs = FS1  # (this block against the receiver's own pull interface: the shared twin has no fifth call)
        a.synchronize()
        mine = dict(panes=[pn.expected(P, a, a.zoom_spectrum() if pn.zoomed else a.spectrum(), "call 4 pane %d" % i) for i, pn in enumerate(panes1(P))])
        assert_block(panes, mine, "call 4")
        a.display_release(1)
        a.display_release(4)
    finally:
        a.close()  # (destroy closes the open ring)


def test_set_pane_between_calls(gpu_lib, shape1):
    """a new dB range and width for the bottom pane, a new zoom for the top one, between calls 1 and 2: block 1 has the old geometry,
    block 2 the new -- though all four calls are queued before any block is read"""
    import pebblesdr_amd as P
    bufs, want = shape1
    old = panes1(P)
    new = [Pane(False, P.DISPLAY_WATERFALL_ARGB32, max_rows=5, x=200, max_db=-20.0, min_db=-100.0, start=-1_000_000, stop=2_500_000),
           Pane(True, P.DISPLAY_PIXELS_I32, y=600, x=699, zoom=0.125, offs=[300])]
    a, b = rx1(P), rx1(P)
    try:
        a.display_open([pn.c(P) for pn in old], 4)
        wide = Pane(False, P.DISPLAY_WATERFALL_ARGB32, max_rows=5, x=305, start=-3_000_000, stop=4_000_000)
        with pytest.raises(P.PebbleGpuError) as e:  # 305 pixels are 1232 bytes a row, the slots were sized for 1216
            a.display_set_pane(0, wide.c(P))
        assert e.value.code == E_SIZE
        with pytest.raises(P.PebbleGpuError) as e:  # a pane keeps its source
            a.display_set_pane(0, new[1].c(P))
        assert e.value.code == E_INVALID
        with pytest.raises(P.PebbleGpuError) as e:
            a.display_set_pane(2, new[1].c(P))
        assert e.value.code == E_INVALID
        twin = []
        for k, (buf, n) in enumerate(bufs):
            if k == 2:
                a.display_set_pane(0, new[0].c(P))
                a.display_set_pane(1, new[1].c(P))
            a.process_device(buf.ptr, n)
            twin.append(twin_call(P, b, buf, n, new if k >= 2 else old, "set_pane call %d" % k))
        for k in range(len(bufs)):
            got = take(a, k)
            assert_block(got, twin[k], "call %d" % k)
            assert got[0][1].shape == (1, 5, 200 if k >= 2 else 301)
        assert_block(twin[1]["panes"], want[1], "the twin itself, call 1")
        assert not same_bits(new[1].expected(P, b, twin[3]["zoom"], "new")[1], old[1].expected(P, b, twin[3]["zoom"], "old")[1])
    finally:
        a.close()
        b.close()


def test_under_the_update_gate(gpu_lib, shape1):
    """50 updates per second at 20 Msps: one unprocessed spectrum per 20 ms against calls of 6.5 to 19.7 ms -- some calls compute no
    row.  Pane rows = the twin's compact rows (pebblegpu_receiver_spectrum_frames counts them), zero-row blocks arrive with the next
    index all the same, and no carried row is ever delivered."""
    import pebblesdr_amd as P
    bufs, _ = shape1
    panes = [Pane(False, P.DISPLAY_PIXELS_I32, x=301, start=-3_000_000, stop=4_000_000), Pane(True, P.DISPLAY_DB_F32)]
    a, b = rx1(P), rx1(P)
    try:
        for rx in (a, b):
            rx.set_spectrum_updates(50)
        a.display_open([panes[0].c(P), panes[1].c(P, with_map=False)], 8)
        twin, counts = [], []
        for rep in range(2):  # the four calls twice: eight calls, 14 super-frames, 92 ms
            for buf, n in bufs:
                a.process_device(buf.ptr, n)
                counts.append((len(a.spectrum_frames()), len(a.spectrum_frames(zoomed=True))))
                twin.append(twin_call(P, b, buf, n, panes, "gated call %d" % len(twin)))
        for k in range(len(twin)):
            got = take(a, k)
            assert_block(got, twin[k], "gated call %d" % k)
            assert (got[0][1].shape[1], got[1][1].shape[1]) == counts[k] == (len(twin[k]["frames"][0]), len(twin[k]["frames"][1]))
            assert got[0][0] == 0 and got[1][0] == 0
        spec_counts = [c[0] for c in counts]
        assert 0 in spec_counts and sum(spec_counts) >= 3, counts     # calls without a row, and rows
        # after a call that made none the pull interface maps the carried row as frame 0; the block of that call had no row at all
        k0 = spec_counts.index(0, 1)
        assert twin[k0]["panes"][0][1].shape == (1, 0, 301)
        assert all_differ([w["panes"][0][1] for w in twin]) and all_differ([w["panes"][1][1] for w in twin])
        assert same_bits(a.audio(), twin[-1]["audio"])
    finally:
        a.close()
        b.close()


def test_reader_on_another_thread_raw_slots_in_rings_out(gpu_lib):
    """K raw calls through the pinned ingest slots with the audio and the display ring open and a reader on another thread; the
    producer calls no synchronize until after the last call.  The threads talk through host-side counters only: the reader takes
    block k once call k has been queued, and the producer stays at most 4 calls ahead of the reader, so with 4 slots nothing can be
    dropped whatever the threads' timing."""
    import pebblesdr_amd as P
    K, n = 8, SF1
    x = stream1(K, seed=29)
    raw = np.stack([np.round(x.real * 100), np.round(x.imag * 100)], axis=1).astype(np.int8)
    panes = [Pane(True, P.DISPLAY_PIXELS_I32, y=400, x=699, zoom=0.5), Pane(False, P.DISPLAY_WATERFALL_ARGB32, max_rows=1, x=1024, start=-FS1 // 2, stop=FS1 // 2)]
    a, b = rx1(P), rx1(P)
    a.audio_out_open(P.AUDIO_S16_MONO, None, 4)
    a.display_open([pn.c(P) for pn in panes], 4)
    room, queued = threading.Semaphore(4), threading.Semaphore(0)
    got, errors = [], []

    def reader():
        try:
            for k in range(K):
                queued.acquire()
                call, dropped, audio = a.audio_out_next(True)
                assert (call, dropped) == (k, 0)
                a.audio_out_release(call)
                got.append((audio, take(a, k)))
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
            blk = np.ascontiguousarray(raw[k * n:(k + 1) * n])
            a.ingest_buffer(k & 1, blk.nbytes, np.int8)[:] = blk.reshape(-1)
            a.ingest_submit(k & 1, blk.nbytes)
            a.process_ingested(k & 1, n, P.binding.IQ_S8)
            queued.release()
        th.join()
        assert not errors, errors
        a.synchronize()
        assert len(got) == K and a.audio_out_dropped() == 0 and a.display_dropped() == 0
        lines = []
        for k in range(K):
            buf = P.DeviceBuffer.from_array(np.ascontiguousarray(raw[k * n:(k + 1) * n]), 0)
            try:
                b.process_raw_device(buf.ptr, n, P.binding.IQ_S8)
                b.synchronize()
                want = dict(panes=[pn.expected(P, b, b.zoom_spectrum() if pn.zoomed else b.spectrum(), "threaded call %d" % k) for pn in panes])
                audio = np.stack([P.audio_out_convert(P.AUDIO_S16_MONO, 100.0, False, row) for row in b.audio()])
            finally:
                buf.free()
            assert same_bits(got[k][0], audio), k
            assert_block(got[k][1], want, "threaded call %d" % k)
            assert got[k][1][1][0] == n // 2048 - 1 and got[k][1][1][1].shape == (1, 1, 1024)   # the latest line of the call
            lines.append(got[k][1][1][1])
        assert all_differ(lines)
    finally:
        for _ in range(K):
            queued.release()  # (a producer that failed must not leave the reader waiting)
        th.join()
        a.close()
        b.close()


def test_refusals_leave_the_handle_usable(gpu_lib, shape1):
    import pebblesdr_amd as P
    bufs, want = shape1
    a = rx1(P)
    nospec = P.ReceiverBank(FS2, 2, True, False, 0, max_superframes=1)            # neither source
    good = panes1(P)

    def refused(code, fn, *args):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*args)
        assert e.value.code == code, (e.value.code, str(e.value))

    def pane(**kw):
        base = dict(zoomed=False, fmt=P.DISPLAY_PIXELS_I32, x=301, start=-3_000_000, stop=4_000_000)
        base.update(kw)
        return Pane(**base).c(P)

    try:
        g = [pn.c(P) for pn in good]
        refused(E_INVALID, a.display_open, [], 4)                                   # n_panes outside 1..2
        refused(E_INVALID, a.display_open, [g[0], g[1], g[0]], 4)
        bad_src = pane()
        bad_src.source = 2
        refused(E_INVALID, a.display_open, [bad_src], 4)                            # unknown source
        bad_fmt = pane()
        bad_fmt.format = 3
        refused(E_INVALID, a.display_open, [bad_fmt], 4)                            # unknown format
        refused(E_INVALID, nospec.display_open, [pane()], 4)                        # spectrum_bins == 0
        refused(E_INVALID, nospec.display_open, [pane(zoomed=True)], 4)             # hires_bins == 0
        refused(E_INVALID, a.display_open, [pane(sel=[0, 0])], 4)                   # duplicate
        refused(E_INVALID, a.display_open, [pane(sel=[1])], 4)                      # out of range
        refused(E_INVALID, a.display_open, [pane(zoomed=True, sel=[])], 4)          # empty
        refused(E_INVALID, a.display_open, g, 1)                                    # n_slots outside 2..8
        refused(E_INVALID, a.display_open, g, 9)
        refused(E_INVALID, a.display_open, [pane(x=0)], 4)                          # what check_screen_map refuses
        refused(E_INVALID, a.display_open, [pane(y=0)], 4)
        refused(E_INVALID, a.display_open, [pane(max_db=-120.0)], 4)
        refused(E_INVALID, a.display_open, [pane(fmt=P.DISPLAY_WATERFALL_ARGB32, y=256)], 4)   # a waterfall of y_pixels != 255
        refused(E_INVALID, a.display_open, [Pane(False, P.DISPLAY_PIXELS_I32).c(P, with_map=False)], 4)  # a mapped format without a map
        refused(E_INVALID, a.display_open, [pane(zoomed=True, zoom=float("nan"))], 4)
        refused(E_INVALID, a.display_open, [pane(zoomed=True, zoom=float("inf"))], 4)
        refused(E_SIZE, a.display_open, [pane(x=1 << 24, max_rows=0)], 8)           # 192 rows of 64 MiB, 8 slots: far above 1 GiB
        refused(E_INVALID, a.display_close)                                         # nothing was opened by any of these
        refused(E_INVALID, a.display_dropped)
        refused(E_INVALID, a.display_release, 0)
        a.display_open(g, 4)
        refused(E_INVALID, a.display_open, g, 4)                                    # a second open
        refused(E_UNSUPPORTED, a.process_iq, np.zeros(2048, dtype=np.complex128))   # the frame path, while the ring is open
        refused(E_INVALID, a.display_release, 0)                                    # nothing handed out yet
        for k, (buf, n) in enumerate(bufs[:2]):                                     # the handle is as it was: good blocks
            a.process_device(buf.ptr, n)
            assert_block(take(a, k), want[k], "call %d" % k)
        a.display_close()
        a.process_iq(np.zeros(2048, dtype=np.complex128))                           # closed: accepted again
    finally:
        a.close()
        nospec.close()


# ---- shape 2: per-channel geometry beyond one chunk ----
def rx2(P):
    rx = P.ReceiverBank(FS2, C2, True, False, 4096, max_superframes=3, hires_bins=ZB)
    assert rx.superframe == SF2 and int(rx.info.demod_rate_int) == 64000
    rx.fs = FS2
    for c in range(C2):
        rx.set_mode(c, P.DM_FMN)
        rx.set_mixer(c, -900e3 + 26e3 * c)
        rx.set_bandpass(c, -7500, 7500)
    return rx


def pane2(P, fmt, zoom):
    return Pane(True, fmt, sel=SEL2, y=255, x=256, zoom=zoom, offs=OFFS2)


@pytest.fixture(scope="module")
def shape2(gpu_lib):
    """a tone of its own level 1.5 kHz above every channel's centre, levels stepping per super-frame, over noise; the twin's zoomed
    spectra and its map of every channel for both zoom values, per call"""
    import pebblesdr_amd as P
    n = sum(SIZES2) * SF2
    x = tones(FS2, n, [(0.002 * (1 + c % 7), -900e3 + 26e3 * c + 1500.0) for c in range(C2)]) * np.repeat([1.0, 0.5, 0.8, 0.3], SF2) + lcg_noise(n, 17, 1e-3)
    bufs = upload_calls(P, x.astype(np.complex64), SIZES2, SF2)
    b = rx2(P)
    try:
        want = []
        for k, (buf, m) in enumerate(bufs):
            panes = [pane2(P, fmt, z) for z in ZOOMS2.values() for fmt in (P.DISPLAY_DB_F32, P.DISPLAY_PIXELS_I32, P.DISPLAY_WATERFALL_ARGB32)]
            w = twin_call(P, b, buf, m, panes, "shape 2 call %d" % k)
            w["by"] = {(z, fmt): w["panes"][i] for i, (z, fmt) in enumerate((z, fmt) for z in ZOOMS2.values() for fmt in range(3))}
            want.append(w)
    finally:
        b.close()
    yield bufs, want
    for buf, _ in bufs:
        buf.free()


def test_shape2_lane_groups_differ_between_the_chunks():
    """the geometry behind shape 2's 'averaged' case, from the restatement alone: channel 5 (offset 0) plots 2048 bins on 256 pixels, 8.0
    bins per pixel -- lanes per pixel 8 for the whole first chunk of 64 channels; channels 64..69 plot 2047 -- 4 lanes; a ring that
    took one lane group for the whole pane would add channel 64's and 69's powers in another order than the map function."""
    bpp = [float(R.geometry(ZB, 64000.0, *R.zoom_edges(64000, 1.0, OFFS2[c]), 256)["bins_per_pixel"]) for c in range(C2)]
    assert max(bpp[:64]) == 8.0 and bpp[5] == 8.0 and max(bpp[64:]) < 8.0 and min(bpp) > 4.0
    rep = [R.geometry(ZB, 64000.0, *R.zoom_edges(64000, 0.1, OFFS2[c]), 256) for c in SEL2]
    assert not any(g["averaged"] for g in rep)
    assert {0, 63, 64, 69} <= set(SEL2) and len(set(OFFS2[c] for c in SEL2)) == len(SEL2)


@pytest.mark.parametrize("zoom_name", list(ZOOMS2))
@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["db_f32", "pixels_i32", "waterfall_argb32"])
def test_shape2_zoomed_pane_of_a_70_channel_bank(gpu_lib, shape2, fmt, zoom_name):
    import pebblesdr_amd as P
    bufs, want = shape2
    zoom = ZOOMS2[zoom_name]
    a = rx2(P)
    try:
        a.display_open([pane2(P, fmt, zoom).c(P, with_map=fmt != P.DISPLAY_DB_F32)], 4)
        for buf, n in bufs:
            a.process_device(buf.ptr, n)
        for k in range(len(bufs)):
            got = take(a, k)
            assert_block(got, dict(panes=[want[k]["by"][(zoom, fmt)]]), "call %d" % k)
            assert got[0][1].shape == (len(SEL2), SIZES2[k], ZB if fmt == P.DISPLAY_DB_F32 else 256) and got[0][0] == 0
            rows = got[0][1]
            assert all_differ([rows[r] for r in range(len(SEL2))])                  # every selected channel has a row of its own
        assert [a.kernel_name(w) for w in range(1, 6)] == want[-1]["names"]
        assert same_bits(a.audio(), want[-1]["audio"])
        assert all_differ([w["by"][(zoom, fmt)][1] for w in want])
    finally:
        a.close()


# ---- through a multibank: every shard has its own ring ----
def test_multibank_shards_deliver_their_own_channels(gpu_lib):
    import pebblesdr_amd as P
    C, sizes = 5, [1, 2]
    fcs = [100e3, -250e3, 400e3, -600e3, 700e3]
    offs = [0, 500, -700, 1234, -90]
    mb = P.MultiBank(FS2, C, [0, 0], frames_per_buffer=2048, max_superframes=2, hires_bins=ZB)
    one = P.ReceiverBank(FS2, C, True, False, 0, max_superframes=2, hires_bins=ZB)
    n = sum(sizes) * SF2
    x = tones(FS2, n, [(0.01 * (c + 1), fcs[c] + 1500.0) for c in range(C)]) * np.repeat([1.0, 0.4, 0.7], SF2) + lcg_noise(n, 23, 1e-3)
    bufs = upload_calls(P, x.astype(np.complex64), sizes, SF2)

    def tune(rx, first, count):
        for c in range(count):
            rx.set_mode(c, P.DM_FMN)
            rx.set_mixer(c, fcs[first + c])
            rx.set_bandpass(c, -7500, 7500)

    try:
        tune(one, 0, C)
        for g, (first, count) in enumerate(mb.ranges):
            tune(mb.shard(g), first, count)
            mb.shard(g).display_open([Pane(True, P.DISPLAY_PIXELS_I32, y=255, x=301, zoom=1.0, offs=offs[first:first + count]).c(P)], 4)
        whole = Pane(True, P.DISPLAY_PIXELS_I32, y=255, x=301, zoom=1.0, offs=offs)
        want = []
        for k, (buf, m) in enumerate(bufs):
            mb.process_device([buf.ptr] * mb.n_shards, m)
            want.append(twin_call(P, one, buf, m, [whole], "multibank call %d" % k))
        assert mb.n_shards == 2 and sum(cnt for _, cnt in mb.ranges) == C
        for g, (first, count) in enumerate(mb.ranges):
            for k in range(len(bufs)):
                got = take(mb.shard(g), k)
                wfirst, warr = want[k]["panes"][0]
                assert got[0][0] == wfirst and same_bits(got[0][1], warr[first:first + count]), (g, k)
        assert all_differ([want[0]["panes"][0][1][c] for c in range(C)])
        for g in range(mb.n_shards):
            mb.shard(g).display_close()
    finally:
        for buf, _ in bufs:
            buf.free()
        mb.close()
        one.close()
