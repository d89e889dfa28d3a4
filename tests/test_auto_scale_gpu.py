"""GPU tier (-m gpu): SpectrumWidget's auto-scale on the device -- k_scale_stats behind the pull functions
(pebblegpu_*_spectrum_scale) and behind the display rings' flags (pebblegpu_*_display_set_auto_scale / _rescale / _display_scale).

Reference: tests/auto_scale_ref.py, the restatement of SpectrumWidget::recalcScale, applied to the float dB rows THE SAME CALL
delivered (spectrum()).  The device adds in another order and has its own exp10 / log10, so a row whose unrounded powerTodB(avg) - 10
or powerTodB(peak) + 10 lies within 1e-6 of an integer could legitimately come out 5 dB away: auto_scale_ref.scale_rows asserts, from
the restatement alone, that EVERY row a test uses is farther away than that (or clamps either way) -- no row is excluded.
avg_power / peak_power: within 1e-11 relative, the worst-case error of summing 65536 positive doubles in any order (65536 * 2^-53).

The rings are held to a TWIN receiver / bank that is fed the same calls, synchronised after each and read through the pull interface:
a block's pixels must equal the twin's map_spectrum / map_zoom_spectrum WITH THE RANGE THE BLOCK REPORTS, bit for bit, its colours the
waterfall of those pixels, and the reported range must be the restatement's for the row the rule says it comes from.  Tone levels are
off the round values (0.13, not 0.1) so that the peaks do not sit on a multiple of 5 dB.
"""
import copy

import numpy as np
import pytest

from tests import auto_scale_ref as A
from tests import waterfall_ref as W
from tests.signals import lcg_noise, tones
from tests.test_receiver_display_gpu import Pane, all_differ, same_bits

pytestmark = pytest.mark.gpu

E_INVALID = -1
FS, SF = 2_048_000, 65536
LEVELS = [0.13, 0.017, 0.0023]           # three streams: peaks near -17.7, -35.4, -52.8 dB
STEP_25DB = 10 ** (25 / 20)
TOL = 1e-11


def ramp(n, frame=2048):
    """an envelope that steps down 3 dB per frame over 8 frames and starts again: the frames of a call get ranges of their own"""
    return 10.0 ** (-0.15 * ((np.arange(n) // frame) % 8))


def streams3(n, seed, frame=2048, fs=FS):
    return np.stack([(tones(fs, n, [(LEVELS[s], 300.37e3 + 41e3 * s)]) * ramp(n, frame) + lcg_noise(n, seed + s, 1e-3)) for s in range(3)]).astype(np.complex64)


def check_scales(got, db, what):
    """got: DISPLAY_SCALE [streams, frames]; db: the same rows' float dB [streams, frames, bins]"""
    want = A.scale_rows(db)
    assert got.shape == db.shape[:2], (what, got.shape, db.shape)
    for r, (g, w) in enumerate(zip(got.reshape(-1), want)):
        assert (int(g["max_db"]), int(g["min_db"])) == (w["max_db"], w["min_db"]), "%s row %d: %s, restatement %s" % (what, r, g, w)
        assert abs(g["avg_power"] - w["avg_power"]) <= TOL * w["avg_power"], (what, r, g["avg_power"], w["avg_power"])
        assert abs(g["peak_power"] - w["peak_power"]) <= TOL * w["peak_power"], (what, r, g["peak_power"], w["peak_power"])
    return want


# ---- 1. the pull function, receiver ----
@pytest.mark.parametrize("bins", [2048, 8192])
def test_receiver_pull(gpu_lib, bins):
    """three streams at three levels, calls of 2 super-frames; 2048 and 8192 bins: two and eight float4 per lane (bins / 1024)"""
    import pebblesdr_amd as P
    rx = P.ReceiverBank(FS, 3, False, False, bins, max_superframes=2)
    n = 2 * SF
    buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(streams3(n, 40)), 0)
    try:
        for c in range(3):
            rx.set_mode(c, P.DM_FMN)
            rx.set_mixer(c, 300e3 + 41e3 * c)
            rx.set_bandpass(c, -7500, 7500)
        assert rx.superframe == SF and rx.n_streams == 3
        rx.process_device(buf.ptr, n)
        F = n // 2048
        got = rx.spectrum_scale(first_frame=0, n_frames=F)
        again = rx.spectrum_scale(first_frame=0, n_frames=F)
        odd = rx.spectrum_scale(first_frame=1, n_frames=F // 2 - 1, frame_step=2)
        last = rx.spectrum_scale()
        db = rx.spectrum()
        assert db.shape == (3, F, bins)
        want = check_scales(got, db, "%d bins" % bins)
        assert same_bits(got, again)                                   # a fixed order, no atomics: the same bits on every run
        assert same_bits(odd, got[:, 1::2][:, :F // 2 - 1]) and same_bits(last, got[:, -1:])
        assert len({(w["max_db"], w["min_db"]) for w in want}) >= 5    # the ranges follow the streams and the frames
        assert len({w["max_db"] for w in want[:F]}) >= 2               # ... within one stream too
        for args in ((0, 0, 1), (F, 1, 1), (1, F // 2 + 1, 2)):        # the map functions' frame rules
            with pytest.raises(P.PebbleGpuError) as e:
                rx.spectrum_scale(*args)
            assert e.value.code == E_INVALID
    finally:
        buf.free()
        rx.close()


# ---- 2. the pull function, stream bank ----
@pytest.mark.parametrize("S,frames,bins", [(2, 1, 65536), (3, 2, 2048)], ids=["2x1x65536", "3x2x2048"])
def test_streambank_pull(gpu_lib, S, frames, bins):
    """the long row (65536 bins: 64 float4 per lane, 256 KiB for one workgroup) and several rows of the shortest"""
    import pebblesdr_amd as P
    sb = P.StreamBank(float(FS), S, frame=bins, spectrum_bins=bins, max_frames=frames)
    try:
        x = streams3(frames * bins, 50, frame=bins)[:S]
        _, db = sb.process(x, 2)
        assert db.shape == (S, frames, bins)
        got = sb.spectrum_scale(first_frame=0, n_frames=frames)
        want = check_scales(got, db, "%d x %d x %d" % (S, frames, bins))
        assert same_bits(got, sb.spectrum_scale(first_frame=0, n_frames=frames))
        assert len({w["max_db"] for w in want}) >= 2
        with pytest.raises(P.PebbleGpuError) as e:
            sb.spectrum_scale(first_frame=frames, n_frames=1)
        assert e.value.code == E_INVALID
    finally:
        sb.close()


# ---- the receiver ring ----
SHAPES = {
    # the smallest receiver with both sources: one narrow channel, 2048 bins, 2048 zoomed bins
    "small": dict(fs=FS, wfm=False, bins=2048, sf=65536, mixer=300e3, tone=301.5e3, zoom=0.5, ups=10),
    # one WFM channel at 20 Msps, 8192 bins: the side-by-side route, whose two pipelines end on different streams under PEBBLEGPU_PIPELINE=1
    "wfm20": dict(fs=20_000_000, wfm=True, bins=8192, sf=131072, mixer=1.0e6, tone=1.003e6, zoom=0.1, ups=50),  # (the tone inside the zoomed span)
}
FIXED = [(-10.0, -110.0), (-20.0, -100.0)]  # the panes' own ranges: nothing the rule can produce for these signals


def make_rx(P, shape, hires=2048, bins=None):
    s = SHAPES[shape]
    rx = P.ReceiverBank(s["fs"], 1, True, s["wfm"], s["bins"] if bins is None else bins, max_superframes=1, hires_bins=hires)
    assert rx.superframe == s["sf"]
    rx.fs = s["fs"]
    if not s["wfm"]:
        rx.set_mode(0, P.DM_FMN)
        rx.set_bandpass(0, -7500, 7500)
    rx.set_mixer(0, s["mixer"])
    return rx


def ring_panes(P, shape):
    """spectrum pixels on top, the zoomed waterfall below"""
    fs = SHAPES[shape]["fs"]
    return [Pane(False, P.DISPLAY_PIXELS_I32, y=400, x=301, max_db=FIXED[0][0], min_db=FIXED[0][1], start=-fs // 4, stop=fs // 3),
            Pane(True, P.DISPLAY_WATERFALL_ARGB32, y=255, x=256, max_db=FIXED[1][0], min_db=FIXED[1][1], zoom=SHAPES[shape]["zoom"])]


def call_input(shape, k, level):
    s = SHAPES[shape]
    n = s["sf"]
    return (tones(s["fs"], n, [(level, s["tone"])], n0=k * n) + lcg_noise(n, 60 + k, 1e-3)).astype(np.complex64)


def with_range(pn, rng):
    """the pane with the ends of `rng` (max_db, min_db) that are not None in place of its own"""
    q = copy.copy(pn)
    if rng[0] is not None:
        q.max_db = float(rng[0])
    if rng[1] is not None:
        q.min_db = float(rng[1])
    return q


def twin_step(P, b, buf, n):
    b.process_device(buf.ptr, n)
    b.synchronize()
    return b.spectrum(), b.zoom_spectrum()


def twin_panes(P, b, panes, spec, zoom, rng, what):
    """what the block of the call the twin has just made must hold when mapped with rng (read-only use of the twin's last call)"""
    return [with_range(pn, rng).expected(P, b, zoom if pn.zoomed else spec, "%s pane %d" % (what, i)) for i, pn in enumerate(panes)]


def take_scaled(a, call, scaled=True):
    """the next block with the ranges it reports (None: the block carries none)"""
    blk = a.display_next(True)
    assert blk is not None and (blk[0], blk[1]) == (call, 0), (call, blk and blk[:2])
    if scaled:
        sc = a.display_scale(call)
    else:
        import pebblesdr_amd as P
        with pytest.raises(P.PebbleGpuError) as e:
            a.display_scale(call)
        assert e.value.code == E_INVALID
        sc = None
    a.display_release(call)
    return blk[2], sc


def assert_panes(got, want, what):
    assert len(got) == len(want)
    for i, ((first, arr), (wfirst, warr)) in enumerate(zip(got, want)):
        assert first == wfirst and arr.shape == warr.shape and arr.dtype == warr.dtype, (what, i, first, wfirst, arr.shape, warr.shape)
        assert same_bits(arr, warr), "%s pane %d: %d of %d elements differ" % (what, i, int((arr != warr).sum()), arr.size)


def assert_reported(sc, rng, refreshed, what):
    """one stream: the block reports rng; avg_power / peak_power are the recalc's in the block of the recalc's call and 0 in any other"""
    assert len(sc) == 1 and (int(sc[0]["max_db"]), int(sc[0]["min_db"])) == rng, (what, sc, rng)
    if refreshed is None:
        assert sc[0]["avg_power"] == 0.0 and sc[0]["peak_power"] == 0.0, (what, sc)
    else:
        assert abs(sc[0]["avg_power"] - refreshed["avg_power"]) <= TOL * refreshed["avg_power"], (what, sc, refreshed)
        assert abs(sc[0]["peak_power"] - refreshed["peak_power"]) <= TOL * refreshed["peak_power"], (what, sc, refreshed)


# ---- 3. the event sequence ----
@pytest.mark.parametrize("shape,pipeline", [("small", False), ("small", True), ("wfm20", True)])
def test_ring_event_sequence(gpu_lib, monkeypatch, shape, pipeline):
    """calls A, B, C queued back to back with no synchronise; the tone is 25 dB stronger from B on and _rescale comes between B and C:
    A's range comes from A's first row, B keeps it, C's is new"""
    import pebblesdr_amd as P
    panes = ring_panes(P, shape)
    n = SHAPES[shape]["sf"]
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(call_input(shape, k, 0.0023 * (STEP_25DB if k else 1.0))), 0) for k in range(3)]
    if pipeline:
        monkeypatch.setenv("PEBBLEGPU_PIPELINE", "1")
    a = make_rx(P, shape)
    monkeypatch.delenv("PEBBLEGPU_PIPELINE", raising=False)
    b = make_rx(P, shape)
    try:
        a.display_open([pn.c(P) for pn in panes], 4)
        a.display_set_auto_scale(P.AUTO_SCALE_MAX | P.AUTO_SCALE_MIN)
        for k, buf in enumerate(bufs):  # nothing waits on the host between these
            if k == 2:
                a.display_rescale()
            a.process_device(buf.ptr, n)
        names = [a.kernel_name(w) for w in range(1, 6)]
        ranges, blocks = [], []
        for k, buf in enumerate(bufs):
            spec, zoom = twin_step(P, b, buf, n)
            first = A.scale_rows(spec[:, :1])[0]                       # the call's FIRST computed row
            new = k != 1
            rng = (first["max_db"], first["min_db"]) if new else ranges[0]
            ranges.append(rng)
            got, sc = take_scaled(a, k)
            assert_reported(sc, rng, first if new else None, "call %d" % k)
            want = twin_panes(P, b, panes, spec, zoom, rng, "call %d" % k)
            assert_panes(got, want, "call %d" % k)
            assert got[0][1].shape[1] == n // 2048 and got[1][1].shape[1] >= 1 and got[1][1].dtype == np.uint32
            blocks.append(got)
            if k == 1:  # B's own first row would have given another range: the block did not use it
                own = A.scale_rows(spec[:, :1])[0]
                assert (own["max_db"], own["min_db"]) != rng
        assert ranges[0] == ranges[1] != ranges[2] and ranges[0] not in [tuple(int(v) for v in f) for f in FIXED]
        assert all_differ([blk[0][1] for blk in blocks]) and all_differ([blk[1][1] for blk in blocks])
        assert names == [b.kernel_name(w) for w in range(1, 6)]        # the flags change no call's route
        assert a.display_next(False) is None and a.display_dropped() == 0
    finally:
        for buf in bufs:
            buf.free()
        a.close()
        b.close()


# ---- 4. under the update gate ----
@pytest.mark.parametrize("shape,pipeline", [("small", False), ("wfm20", True)])
def test_recalc_waits_for_a_computed_row(gpu_lib, monkeypatch, shape, pipeline):
    """10 spectra per second against calls of 32 ms (50 against 6.5 ms at 20 Msps): most calls compute no unprocessed row, and the zoomed
    source has a timer of its own.  The recalc lands on the first call that computes a row; while one is pending a zoomed pane keeps the
    old range.  A block without a row of either pane is empty as ever and carries no ranges.  Under PEBBLEGPU_PIPELINE=1 the zoomed rows
    are packed on the chain's stream, calls with unprocessed rows alone lie between them and the recalc, and nothing is synchronised: the
    order in which the table's write has to wait for readers older than the previous block."""
    import pebblesdr_amd as P
    K, LOUD_FROM, RESCALE_AT = 10, 6, 7
    panes = ring_panes(P, shape)
    n = SHAPES[shape]["sf"]
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(call_input(shape, k, 0.0023 * (STEP_25DB if k >= LOUD_FROM else 1.0))), 0) for k in range(K)]
    if pipeline:
        monkeypatch.setenv("PEBBLEGPU_PIPELINE", "1")
    a = make_rx(P, shape)
    monkeypatch.delenv("PEBBLEGPU_PIPELINE", raising=False)
    b = make_rx(P, shape)
    try:
        for rx in (a, b):
            rx.set_spectrum_updates(SHAPES[shape]["ups"])
        a.display_open([pn.c(P) for pn in panes], 8)
        a.display_set_auto_scale(3)
        pending, rng, kept_while_pending, recalcs, empty_blocks = True, (None, None), 0, [], 0
        for k, buf in enumerate(bufs):
            if k == RESCALE_AT:
                a.display_rescale()
                pending = True
            a.process_device(buf.ptr, n)               # (the ring under test is never synchronised)
            spec, zoom = twin_step(P, b, buf, n)
            fresh = None
            if pending and spec.shape[1]:
                fresh = A.scale_rows(spec[:, :1])[0]
                rng, pending = (fresh["max_db"], fresh["min_db"]), False
                recalcs.append(k)
            if pending and zoom.shape[1] and not spec.shape[1] and rng[0] is not None:
                kept_while_pending += 1
            rows = spec.shape[1] + zoom.shape[1]
            empty_blocks += not rows
            got, sc = take_scaled(a, k, scaled=rows > 0)
            reported = tuple(int(v) for v in FIXED[0]) if rng[0] is None else rng   # before the first recalc: the pane's own (pane 0's)
            if rows:
                assert_reported(sc, reported, fresh, "gated call %d" % k)
            assert_panes(got, twin_panes(P, b, panes, spec, zoom, rng, "gated call %d" % k), "gated call %d" % k)
            assert (got[0][1].shape[1], got[1][1].shape[1]) == (spec.shape[1], zoom.shape[1])
        # the scenario happened: the first recalc waited for a row, the second came after the request, and a zoomed row was mapped in between
        assert len(recalcs) == 2 and recalcs[0] > 0 and recalcs[1] > RESCALE_AT and kept_while_pending >= 1, (recalcs, kept_while_pending)
        assert empty_blocks >= 2
    finally:
        for buf in bufs:
            buf.free()
        a.close()
        b.close()


# ---- 5. one flag only, and the refusals ----
def test_one_flag_and_refusals(gpu_lib):
    import pebblesdr_amd as P
    shape = "small"
    panes = ring_panes(P, shape)
    n = SHAPES[shape]["sf"]
    levels = [0.0023, 0.0023 * STEP_25DB, 0.0023, 0.0023 * STEP_25DB, 0.0023, 0.0023]
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(call_input(shape, k, lv)), 0) for k, lv in enumerate(levels)]
    a, b = make_rx(P, shape), make_rx(P, shape)
    zoom_only = make_rx(P, shape, bins=0)
    fmax, fmin = (int(v) for v in FIXED[0])

    def refused(fn, *args):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*args)
        assert e.value.code == E_INVALID, (e.value.code, str(e.value))

    try:
        refused(a.display_set_auto_scale, 3)                               # no open ring
        refused(a.display_rescale)
        refused(a.display_scale, 0)
        zoom_only.display_open([panes[1].c(P)], 2)
        refused(zoom_only.display_set_auto_scale, 3)                       # no unprocessed spectrum to take the range from
        a.display_open([pn.c(P) for pn in panes], 4)
        refused(a.display_set_auto_scale, 4)                               # unknown bits
        refused(a.display_set_auto_scale, 7)
        a.display_set_pane(0, with_range(panes[0], (0.0, -40.0)).c(P))
        refused(a.display_set_auto_scale, P.AUTO_SCALE_MAX)                # MAX alone over a fixed min_db >= -50
        a.display_set_pane(0, with_range(panes[0], (-80.0, -110.0)).c(P))
        refused(a.display_set_auto_scale, P.AUTO_SCALE_MIN)                # MIN alone under a fixed max_db <= -70
        a.display_set_pane(0, panes[0].c(P))
        # flags per call: MAX; MIN; both; MIN (MAX goes off); MIN with refused set_panes in between; none
        flags = [1, 2, 3, 2, 2, 0]
        cur, live, rng = 0, 0, [None, None]
        for k, buf in enumerate(bufs):
            a.display_set_auto_scale(flags[k])
            if flags[k] == 1:
                refused(a.display_set_pane, 0, with_range(panes[0], (0.0, -40.0)).c(P))    # a _set_pane that would create the refused state
            if k == 4:
                refused(a.display_set_pane, 0, with_range(panes[0], (-80.0, -110.0)).c(P))
                refused(a.display_scale, 99)                               # not handed out
            recalc = bool(flags[k] & ~cur)
            cur = flags[k]
            live &= cur
            a.process_device(buf.ptr, n)
            spec, zoom = twin_step(P, b, buf, n)
            fresh = A.scale_rows(spec[:, :1])[0] if recalc else None
            if recalc:
                rng, live = [fresh["max_db"], fresh["min_db"]], cur
            used = (rng[0] if live & 1 else None, rng[1] if live & 2 else None)
            got, sc = take_scaled(a, k, scaled=cur != 0)
            if cur:
                assert_reported(sc, (used[0] if used[0] is not None else fmax, used[1] if used[1] is not None else fmin), fresh, "call %d" % k)
            assert_panes(got, twin_panes(P, b, panes, spec, zoom, used, "call %d" % k), "call %d" % k)
        assert rng[0] != fmax and rng[1] != fmin
        # MAX alone goes live, then MIN is added: until its recalc lands the table supplies MAX alone, and a fixed min_db >= -50 is refused
        a.display_set_auto_scale(P.AUTO_SCALE_MAX)
        a.process_device(bufs[0].ptr, n)
        take_scaled(a, len(bufs))
        a.display_set_auto_scale(3)
        refused(a.display_set_pane, 0, with_range(panes[0], (float(fmax), -45.0)).c(P))
        zoom_only.process_device(bufs[0].ptr, n)  # the refused ring still delivers
        blk = zoom_only.display_next(True)
        assert blk is not None and blk[0] == 0 and blk[2][0][1].shape[1] >= 1
    finally:
        for buf in bufs:
            buf.free()
        for rx in (a, b, zoom_only):
            rx.close()


# ---- 6. flags 0 change nothing ----
def test_flags_zero_change_nothing(gpu_lib):
    """a ring never given flags, and one whose flags went on and off again before the first call, deliver the twin's blocks bit for bit
    and report the twin's kernels"""
    import pebblesdr_amd as P
    shape = "small"
    panes = ring_panes(P, shape)
    n = SHAPES[shape]["sf"]
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(call_input(shape, k, 0.0023 * (1 + k))), 0) for k in range(2)]
    a, c, b = make_rx(P, shape), make_rx(P, shape), make_rx(P, shape)
    try:
        for rx in (a, c):
            rx.display_open([pn.c(P) for pn in panes], 4)
        c.display_set_auto_scale(3)
        c.display_set_auto_scale(0)
        c.display_rescale()
        for k, buf in enumerate(bufs):
            a.process_device(buf.ptr, n)
            c.process_device(buf.ptr, n)
            spec, zoom = twin_step(P, b, buf, n)
            want = twin_panes(P, b, panes, spec, zoom, (None, None), "call %d" % k)
            for rx in (a, c):
                got, _ = take_scaled(rx, k, scaled=False)
                assert_panes(got, want, "call %d" % k)
                assert [rx.kernel_name(w) for w in range(1, 6)] == [b.kernel_name(w) for w in range(1, 6)]
    finally:
        for buf in bufs:
            buf.free()
        for rx in (a, b, c):
            rx.close()


# ---- 7. the stream bank's ring ----
def test_streambank_ring_per_stream_ranges(gpu_lib):
    """three streams at three levels, 2048 bins, the waterfall format: each stream's rows are mapped with its own range, and gated calls
    with 0 rows keep the recalc pending"""
    import pebblesdr_amd as P
    S, F, bins, K, RESCALE_AT = 3, 4, 2048, 6, 3
    fs = 2.0e6
    lo, hi = -400_000, 600_000
    fixed = (-20, -100)
    xs = [np.ascontiguousarray(streams3(F * bins, 70 + 3 * k, fs=fs) * (4.0 if k >= RESCALE_AT else 1.0)).astype(np.complex64) for k in range(K)]  # 12 dB up from the request on
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(x), 0) for x in xs]
    a = P.StreamBank(fs, S, frame=bins, spectrum_bins=bins, max_frames=F)
    b = P.StreamBank(fs, S, frame=bins, spectrum_bins=bins, max_frames=F)
    try:
        for sb in (a, b):
            sb.set_spectrum_updates(100)                                  # a row about every tenth frame
        with pytest.raises(P.PebbleGpuError) as e:                        # no open ring
            a.display_set_auto_scale(3)
        assert e.value.code == E_INVALID
        a.display_open(P.DISPLAY_DB_F32, None, None, 0, n_slots=2)
        with pytest.raises(P.PebbleGpuError) as e:                        # a DB_F32 ring maps nothing
            a.display_set_auto_scale(3)
        assert e.value.code == E_INVALID
        a.display_close()
        a.display_open(P.DISPLAY_WATERFALL_ARGB32, P.screen_map(255, 301, float(fixed[0]), float(fixed[1]), lo, hi), None, 0, n_slots=8)
        for bad in (4, 8):
            with pytest.raises(P.PebbleGpuError) as e:
                a.display_set_auto_scale(bad)
            assert e.value.code == E_INVALID
        a.display_set_auto_scale(3)
        pending, rngs, recalcs, empty_pending = True, None, [], 0
        for k, buf in enumerate(bufs):
            if k == RESCALE_AT:
                a.display_rescale()
                pending = True
            a.process_device(buf.ptr, F * bins, 2)
            b.process_device(buf.ptr, F * bins, 2)
            db = b.spectrum()
            rows = db.shape[1]
            fresh = None
            if pending and rows:
                fresh = A.scale_rows(db[:, :1])
                before = rngs
                rngs, pending = [(w["max_db"], w["min_db"]) for w in fresh], False
                recalcs.append(k)
                assert len(set(rngs)) == S and rngs != before, (k, rngs, before)   # three streams, three ranges, and new ones
            elif pending and not rows:
                empty_pending += 1
            blk = a.display_next(True)
            assert blk is not None and (blk[0], blk[1], blk[2]) == (k, 0, 0)
            if rows:
                sc = a.display_scale(k)
            else:                                                         # an empty block is empty as ever: no ranges
                with pytest.raises(P.PebbleGpuError) as e:
                    a.display_scale(k)
                assert e.value.code == E_INVALID
            a.display_release(k)
            assert blk[3].shape == (S, rows, 301)
            for s in range(S if rows else 0):
                rng = rngs[s] if rngs else fixed
                assert (int(sc[s]["max_db"]), int(sc[s]["min_db"])) == rng, (k, s, sc[s], rng)
                if fresh:
                    assert abs(sc[s]["avg_power"] - fresh[s]["avg_power"]) <= TOL * fresh[s]["avg_power"]
                    assert abs(sc[s]["peak_power"] - fresh[s]["peak_power"]) <= TOL * fresh[s]["peak_power"]
                else:
                    assert sc[s]["avg_power"] == 0.0 and sc[s]["peak_power"] == 0.0
                if rows:
                    px = b.map_spectrum(255, 301, float(rng[0]), float(rng[1]), lo, hi, first_frame=0, n_frames=rows)[s]
                    assert same_bits(blk[3][s], W.waterfall(px)), "call %d stream %d" % (k, s)
        assert len(recalcs) == 2 and recalcs[0] > 0 and recalcs[1] > RESCALE_AT and empty_pending >= 2, (recalcs, empty_pending)
    finally:
        for buf in bufs:
            buf.free()
        a.close()
        b.close()
