"""GPU tier (-m gpu) of the display map's geometry table (tests/screen_cases.py): map_power_db<G> behind its three kernels --
k_screen_map<G> (the map functions), k_display_map<G, ARGB> (the stream bank's display ring) and k_display_panes (the receiver's) --
on every row of the table, against tests/screen_map_ref.py applied to the float dB rows the device itself delivered.  The restatement is
held to the oracle, and the oracle to the reference's compiled FFT::mapFFTToScreen, by the CPU tier (tests/test_screen_cases_host.py,
tests/test_reference_pins.py).

THE BAR (hold()): every pixel equals the restatement's height.  The one exception is an averaged pixel whose unrounded value v lies
within 1e-9 max(1, |v|) of an integer: there the height of the neighbouring powerdB is accepted too (`alt`).  On pixels whose window is
not flat the restatement itself may flag at most 1 in 10 000 (asserted on the restatement's count, printed); the device may differ on
flagged pixels only.  Where a window is flat (every bin equal: silence, a clipped peak) 10 log10 of the mean lands within an ulp of the
bins' own value, every such pixel is flagged, and instead all flat windows of a row with the same length and value must come out at the
same height.  Every map is run twice and must give the same bits.

Inputs come from the device (there is no way to upload a dB row): tone plus LCG noise; silence (every bin exactly -120); a tone of
amplitude 4 over noise, whose peak bins clip to exactly 0.0.

MEASURED on an MI355X: see DESIGN.md section 3, "Display map: the geometry table".
"""
import numpy as np
import pytest

from tests import screen_cases as S
from tests import screen_map_ref as R
from tests import waterfall_ref as W
from tests.signals import lcg_noise, tones

pytestmark = pytest.mark.gpu

KINDS = ("noise", "silence", "clipped")
FS, BINS = 2048000.0, 2048
# one row per lane group and the rows of 1 and 3 pixels, all at 2048 bins / 2.048 Msps / 255 pixels high (the waterfall's height)
GROUP_ROWS = ["g1_bpp_1p5", "g2_nonint", "g4_at_4", "g8_at_8", "g16_at_16", "g32_below_64", "g64_at_64", "g64_x3", "x1"]


def signal(kind, fs, n, seed, level=0.3):
    if kind == "silence":
        return np.zeros(n, dtype=np.complex128)
    if kind == "clipped":
        return tones(fs, n, [(4.0, 0.11 * fs)]) + lcg_noise(n, seed, 1e-3)
    return tones(fs, n, [(level, 0.11 * fs), (level / 15, -0.23 * fs), (level / 1000, 0.31 * fs)]) + lcg_noise(n, seed, 1e-3)


def _near(v, tol=1e-9):
    with np.errstate(invalid="ignore"):
        return np.abs(v - np.round(v)) <= tol * np.maximum(1.0, np.abs(v))


class Tally:
    """what hold() saw over one test: printed at its end"""

    def __init__(self):
        self.pixels = self.averaged = self.flat = self.flagged = self.tolerated = 0

    def line(self, what):
        """the test's summary; asserts the restatement's own count: at most 1 in 10 000 averaged pixels (flat windows apart) is flagged"""
        assert self.flagged * 10000 <= self.averaged, "%s: the restatement flags %d of %d averaged pixels" % (what, self.flagged, self.averaged)
        return "%s: %d pixels, %d averaged over a window that is not flat (%d of them flagged by the restatement), %d flat windows, " \
               "%d pixels took the neighbouring height" % (what, self.pixels, self.averaged, self.flagged, self.flat, self.tolerated)


def hold(dev, db, bins, fs, y, x, max_db, min_db, start, stop, what, tally):
    """dev [..., x] against the restatement of the float dB rows db [..., bins], by the bar of the module's docstring"""
    db = np.asarray(db, dtype=np.float32)
    assert db.shape[-1] == bins and float(db.min()) >= -120.0 and float(db.max()) <= 0.0, what
    want, v, alt = R.map_fft_to_screen(db, bins, fs, y, x, max_db, min_db, start, stop)
    dev = np.asarray(dev)
    assert dev.shape == want.shape and dev.dtype == np.int32, (what, dev.shape, want.shape)
    rows, dev, want, alt, v = db.reshape(-1, bins), dev.reshape(-1, x), want.reshape(-1, x), alt.reshape(-1, x), v.reshape(-1, x)
    g = R.geometry(bins, fs, start, stop, x)
    b = R.pixel_bins(g, x).astype(np.int64)
    last = np.concatenate([[-1], b[:-1]])
    avg = (b >= 0) & (b < bins) & bool(g["averaged"]) & (last > 0) & (b != last + 1)
    assert np.array_equal(avg, ~np.isnan(v[0])), what
    ok = (dev == want) | (dev == alt)
    if not ok.all():
        k = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d pixels differ, first at %s: device %d, restatement %d (v %r)" % (what, int((~ok).sum()), k, dev[k], want[k], v[k]))
    differ = dev != want
    assert not differ[:, ~avg].any(), what
    tally.pixels += dev.size
    tally.tolerated += int(differ.sum())
    ia = np.nonzero(avg)[0]
    if not len(ia):
        return
    idx = np.empty(2 * len(ia), dtype=np.int64)
    idx[0::2], idx[1::2] = last[ia], b[ia]
    assert (idx[0::2] < idx[1::2]).all() and idx.max() < bins
    hi = np.maximum.reduceat(rows, idx, axis=1)[:, 0::2]
    lo = np.minimum.reduceat(rows, idx, axis=1)[:, 0::2]
    flat = hi == lo
    flagged = _near(v[:, ia])
    assert (differ[:, ia] <= flagged).all(), what                      # the device differs on flagged pixels only
    n_rough, n_flagged = int((~flat).sum()), int((flagged & ~flat).sum())
    tally.averaged += n_rough
    tally.flagged += n_flagged
    tally.flat += int(flat.sum())
    skipped = idx[1::2] - idx[0::2]
    for r in range(rows.shape[0]):                                     # flat windows of one length and value: one height
        seen = {}
        for k in np.nonzero(flat[r])[0]:
            key = (int(skipped[k]), float(hi[r, k]))
            h = int(dev[r, ia[k]])
            assert seen.setdefault(key, h) == h, "%s row %d: flat windows of %d bins at %g dB come out at %d and %d" % (what, r, key[0], key[1], seen[key], h)


def row_args(r):
    return (r.y, r.x, r.max_db, r.min_db, r.start, r.stop)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_input(kind, db):
    """the input is what its name says (on the device's own dB)"""
    db = np.asarray(db)
    if kind == "silence":
        assert (db == -120.0).all()
    elif kind == "clipped":
        assert (db == 0.0).sum() >= 2 and float(db.max()) == 0.0
    else:
        assert -120.0 < float(db.max()) < 0.0 and len(np.unique(db)) > db.size // 2


# ---- (a) every row through the stand-alone spectrum step: k_screen_map, one geometry ----
@pytest.mark.parametrize("kind", KINDS)
def test_every_row_through_the_spectrum_step(gpu_lib, kind):
    import pebblesdr_amd as P
    tally = Tally()
    shapes = sorted({(r.bins, r.fs) for r in S.ROWS})
    assert len(shapes) == 6
    groups_run = set()
    for bins, fs in shapes:
        frame = 65536 if bins == 65536 else 2048          # (the 65536-bin transform takes frames of 65536 only)
        sp = P.Spectrum(bins, fs, frame)
        try:
            x = signal(kind, fs if fs > 1000 else 2048000.0, 2 * frame, 11)
            sp.fftSpectrum(x[:frame])
            db, _ = sp.fftSpectrum(x[frame:])
            assert sp.bins == bins
            check_input(kind, db)
            for r in S.ROWS:
                if (r.bins, r.fs) != (bins, fs):
                    continue
                got = sp.mapFFTToScreen(*row_args(r))
                hold(got, db, bins, fs, *row_args(r), "%s %s" % (kind, r.name), tally)
                assert same_bits(got, sp.mapFFTToScreen(*row_args(r))), r.name
                if r.want["avg"]:
                    groups_run.add(r.want["G"])
        finally:
            sp.close()
    assert groups_run == {1, 2, 4, 8, 16, 32, 64}                        # k_screen_map<G>: all seven instances ran an averaged pixel
    print(tally.line("spectrum step, %s" % kind))
    assert tally.averaged + tally.flat == sum(r.want["avg"] for r in S.ROWS)   # every averaged pixel of the table was held
    if kind == "silence":
        assert tally.averaged == 0
    elif kind == "noise":
        assert tally.flat == 0


# ---- (b) the stream bank: map_spectrum over streams x frames, and its display ring (k_display_map<G, false | true>) ----
LEVELS = [0.13, 0.0023]


def bank_input(call):
    """3 streams x 4 frames: two tone-plus-noise streams 35 dB apart and a clipped one; `call` moves the levels (and the seeds)"""
    n = 4 * 2048
    k = 1.0 if call == 0 else 0.4
    xs = [signal("noise", FS, n, 31 + 7 * call, level=LEVELS[0] * k), signal("noise", FS, n, 32 + 7 * call, level=LEVELS[1] * k),
          signal("clipped", FS, n, 33 + 7 * call)]
    return np.stack(xs).astype(np.complex64)


@pytest.fixture(scope="module")
def bank(gpu_lib):
    import pebblesdr_amd as P
    sb = P.StreamBank(FS, 3, frame=2048, spectrum_bins=BINS, max_frames=4)
    bufs = [P.DeviceBuffer.from_array(P.binding.to_f32_iq(bank_input(c)), 0) for c in range(2)]
    yield sb, bufs
    for b in bufs:
        b.free()
    sb.close()


def test_group_rows_are_what_part_b_needs():
    rows = [S.row(n) for n in GROUP_ROWS]
    assert [r.want["G"] for r in rows[:7]] == [1, 2, 4, 8, 16, 32, 64] and all(r.want["avg"] > 0 for r in rows[:8])
    assert (rows[7].x, rows[8].x) == (3, 1) and all((r.bins, r.fs, r.y) == (BINS, FS, 255) for r in rows)


@pytest.mark.parametrize("frame_step", [1, 3])
def test_streambank_map_spectrum(gpu_lib, bank, frame_step):
    sb, bufs = bank
    tally = Tally()
    sb.process_device(bufs[0].ptr, 4 * 2048, 2)
    spec = sb.spectrum()
    assert spec.shape == (3, 4, BINS)
    check_input("noise", spec[0]), check_input("noise", spec[1]), check_input("clipped", spec[2])
    assert float(spec[0].max()) - float(spec[1].max()) > 30.0          # streams of different levels
    n = len(range(0, 4, frame_step))
    for name in GROUP_ROWS:
        r = S.row(name)
        got = sb.map_spectrum(*row_args(r), first_frame=0, n_frames=n, frame_step=frame_step)
        assert got.shape == (3, n, r.x)
        hold(got, spec[:, ::frame_step], BINS, FS, *row_args(r), "bank step %d %s" % (frame_step, name), tally)
        assert same_bits(got, sb.map_spectrum(*row_args(r), first_frame=0, n_frames=n, frame_step=frame_step)), name
    print(tally.line("stream bank map_spectrum, frame_step %d" % frame_step))


def _ring_block(P, sb, buf, fmt, r, scale=False, rescale_with=None):
    """open the ring on row r's map, make the call(s), -> (rows [3, 4, x], the ranges the block reports or None, the call's spectrum)"""
    sb.display_open(fmt, P.screen_map(*row_args(r)), None, 0, n_slots=2)
    try:
        if scale:
            sb.display_set_auto_scale(P.AUTO_SCALE_MAX | P.AUTO_SCALE_MIN)
        sb.process_device(buf.ptr, 4 * 2048, 2)
        blk = sb.display_next(True)
        if rescale_with is not None:
            sb.display_release(blk[0])
            sb.display_rescale()
            sb.process_device(rescale_with.ptr, 4 * 2048, 2)
            blk = sb.display_next(True)
        assert blk is not None and blk[1] == 0 and blk[2] == 0, blk and blk[:3]
        sc = sb.display_scale(blk[0]) if scale else None
        sb.display_release(blk[0])
        return blk[3], sc, sb.spectrum()
    finally:
        sb.display_close()


def test_streambank_ring_is_the_map_function_bit_for_bit(gpu_lib, bank):
    import pebblesdr_amd as P
    sb, bufs = bank
    for name in GROUP_ROWS:
        r = S.row(name)
        px, _, spec = _ring_block(P, sb, bufs[0], P.DISPLAY_PIXELS_I32, r)
        want = sb.map_spectrum(*row_args(r), first_frame=0, n_frames=4)
        assert px.dtype == np.int32 and same_bits(px, want), "%s: %d of %d pixels differ from map_spectrum" % (name, int((px != want).sum()), want.size)
        argb, _, _ = _ring_block(P, sb, bufs[0], P.DISPLAY_WATERFALL_ARGB32, r)
        want = sb.map_spectrum(*row_args(r), first_frame=0, n_frames=4)    # (of the call the colours came from)
        assert argb.dtype == np.uint32 and same_bits(argb, W.waterfall(want)), name
        assert len(np.unique(want)) > 1, name


def test_streambank_ring_with_auto_scale_after_a_rescale(gpu_lib, bank):
    """both flags on, a call, _rescale, a second call at other levels: the second block's rows are mapped with each stream's own range --
    the ranges the trailer reports -- and equal the restatement with them.  At 1 and 3 pixels a workgroup's round of items spans all
    twelve block rows, whose ranges differ by stream"""
    import pebblesdr_amd as P
    sb, bufs = bank
    tally = Tally()
    for fmt in (P.DISPLAY_PIXELS_I32, P.DISPLAY_WATERFALL_ARGB32):
        for name in GROUP_ROWS:
            r = S.row(name)
            got, sc, spec = _ring_block(P, sb, bufs[0], fmt, r, scale=True, rescale_with=bufs[1])
            rngs = [(int(sc[s]["max_db"]), int(sc[s]["min_db"])) for s in range(3)]
            assert len(sc) == 3 and len(set(rngs)) >= 2, rngs                                    # per-stream ranges, and not all alike
            assert all(-50 <= mx <= 0 and -120 <= mn <= -70 and (mx, mn) != (int(r.max_db), int(r.min_db)) for mx, mn in rngs), rngs
            for s, (mx, mn) in enumerate(rngs):
                a = (r.y, r.x, float(mx), float(mn), r.start, r.stop)
                px = sb.map_spectrum(*a, first_frame=0, n_frames=4)[s]
                hold(px, spec[s], BINS, FS, *a, "auto-scale %s stream %d" % (name, s), tally)
                if fmt == P.DISPLAY_PIXELS_I32:
                    assert same_bits(got[s], px), (name, s, int((got[s] != px).sum()))
                else:
                    assert same_bits(got[s], W.waterfall(px)), (name, s)
    print(tally.line("stream bank ring, auto-scale"))


# ---- (c) the receiver's display ring: k_display_panes ----
def small_rx(P):
    rx = P.ReceiverBank(int(FS), 1, True, False, BINS, max_superframes=1, hires_bins=2048)
    assert rx.superframe == 65536
    rx.set_mode(0, P.DM_FMN)
    rx.set_bandpass(0, -7500, 7500)
    rx.set_mixer(0, 300e3)
    return rx


@pytest.mark.parametrize("kind", ["noise", "clipped"])
def test_receiver_ring_unprocessed_pane_every_switch_arm(gpu_lib, kind):
    import pebblesdr_amd as P
    rx = small_rx(P)
    tally = Tally()
    buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(signal(kind, FS, 65536, 41).astype(np.complex64)), 0)
    try:
        arms = []
        for call, name in enumerate(GROUP_ROWS):
            r = S.row(name)
            for fmt in (P.DISPLAY_PIXELS_I32, P.DISPLAY_WATERFALL_ARGB32):
                rx.display_open([P.display_pane(P.PANE_SPECTRUM, fmt, P.screen_map(*row_args(r)), max_rows=4)], 2)
                try:
                    rx.process_device(buf.ptr, 65536)
                    c, dropped, panes = rx.display_next(True)
                    rx.display_release(c)
                finally:
                    rx.display_close()
                first, got = panes[0]
                assert dropped == 0 and first == 28 and got.shape == (1, 4, r.x)
                spec = rx.spectrum()
                want = rx.map_spectrum(*row_args(r), first_frame=first, n_frames=4)
                if fmt == P.DISPLAY_PIXELS_I32:
                    assert same_bits(got, want), "%s: %d pixels differ from map_spectrum" % (name, int((got != want).sum()))
                    check_input(kind, spec[0, first:])
                    hold(want[0], spec[0, first:], BINS, FS, *row_args(r), "receiver %s %s" % (kind, name), tally)
                    arms.append(r.want["G"])
                else:
                    assert same_bits(got, W.waterfall(want)), name
        assert set(arms) == {1, 2, 4, 8, 16, 32, 64}
    finally:
        buf.free()
        rx.close()
    print(tally.line("receiver ring, unprocessed pane, %s" % kind))


def test_receiver_ring_zoomed_pane_two_chunks_two_lane_groups(gpu_lib):
    """70 NFM channels with per-channel offsets in the averaged branch (tests/test_receiver_display_gpu.py's shape 2): the map function
    runs two launches of 64 and 6 geometries with lane groups 8 and 4; map_zoom_spectrum against the restatement channel by channel, and
    the ring, which packs all 70 rows in one launch from its table, bit for bit against it"""
    import pebblesdr_amd as P
    from tests.test_receiver_display_gpu import C2, FS2, OFFS2, SF2, ZB, rx2
    bins, fs, x, edges, per = S.STREAM_SETS["seventy_two_chunks"]
    assert (bins, x, per, len(edges)) == (ZB, 256, True, C2) and edges == [R.zoom_edges(64000, 1.0, OFFS2[c]) for c in range(C2)]
    assert [G for _, G in S.stream_plan("seventy_two_chunks")] == [8] * 64 + [4] * 6
    n = SF2
    xin = tones(FS2, n, [(0.002 * (1 + c % 7), -900e3 + 26e3 * c + 1500.0) for c in range(C2)]) + lcg_noise(n, 17, 1e-3)
    buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(xin.astype(np.complex64)), 0)
    tally = Tally()
    a = rx2(P)
    try:
        assert int(a.info.demod_rate_int) == 64000
        a.display_open([P.display_pane(P.PANE_ZOOM, P.DISPLAY_PIXELS_I32, P.screen_map(255, x, 0.0, -120.0, 0, 0), 1.0, OFFS2)], 2)
        a.process_device(buf.ptr, n)
        c, dropped, panes = a.display_next(True)
        a.display_release(c)
        first, got = panes[0]
        Z = a.zoom_spectrum()
        want = a.map_zoom_spectrum(255, x, 0.0, -120.0, 1.0, OFFS2, first_frame=0)
        assert first == 0 and dropped == 0 and got.shape == want.shape == (C2, Z.shape[1], x) and Z.shape[1] >= 1
        for ch in range(C2):
            hold(want[ch], Z[ch], bins, fs, 255, x, 0.0, -120.0, edges[ch][0], edges[ch][1], "zoom channel %d" % ch, tally)
        assert same_bits(got, want), "%d of %d pixels differ from map_zoom_spectrum" % (int((got != want).sum()), want.size)
        assert same_bits(want, a.map_zoom_spectrum(255, x, 0.0, -120.0, 1.0, OFFS2, first_frame=0))
        assert len({want[ch].tobytes() for ch in range(C2)}) == C2      # every channel has a row of its own
    finally:
        buf.free()
        a.close()
    print(tally.line("receiver ring, zoomed pane, 70 channels"))
