"""The geometry table of the display map (FFT::mapFFTToScreen, pebblelib/fft.cpp:411-534), shared by tests/test_screen_cases_host.py,
tests/test_screen_cases_gpu.py and the "mapscreen_*" cases of tests/reference_cases.py.

A row is (name, bins, fs, start, stop, x_pixels, y_pixels, max_db, min_db, the edge it exists for, pinned, the recipe of its pin, what the
planner must find).  plan() restates fft.cpp:425-449, :475 and :514 in plain integers -- Python Fractions rounded to float32 / float64 by
_rnd(), written from the reference's text, not from the device's screen_geom.h nor from tests/screen_map_ref.py (numpy) -- and
check_edge() asserts from its result that the row reaches the edge its class names: the table proves that each edge is reached.

    binsPerHz    = (float)fftSize / (float)sampleRate
    binLow       = (qint32)(startFreq * binsPerHz) + fftSize / 2       qint32 * float is float; the conversion truncates
    binHigh      = the same with stopFreq;  fftBinsToPlot = binHigh - binLow
    pixelsPerBin = (float)xPixels / (float)fftBinsToPlot;  binsPerPixel its inverse
    fftBinsToPlot > xPixels:  fftBin = binLow + (i * binsPerPixel)     qint32 + int * float: two float roundings, then truncation
    otherwise:                fftBin = binLow + (i / pixelsPerBin)
    out of [0, fftSize): DB::minDb; averaged over [lastFftBin, fftBin) when lastFftBin > 0 and fftBin != lastFftBin + 1; else direct

PINNED rows are run through the reference's own compiled FFT::mapFFTToScreen (oracle/_ref/ref_driver, stage mapscreen) and recorded as
tests/golden/refpin_mapscreen_<row>.npy.  A row is pinned only if every float -> int conversion it makes is in range (plan()["in_range"]):
a conversion out of range is undefined in C and the driver's answer would be the compiler's.  The rows that rest on what x86-64 does there
(INT_MIN), and the row whose edges come from the quint16 span of mapFFTZoomedToScreen, are UNPINNED: the device and the restatement are
held to each other and to the oracle's written-out x86 rule on them, not to the reference binary.
"""
from collections import namedtuple
from fractions import Fraction as Fr

import numpy as np

from tests.signals import lcg_uniform

INT_MIN = -(1 << 31)
MIN_DB = -120
RECIPES = ("uniform", "flat", "peaks")
PEAK_EVERY = 61  # the "peaks" recipe: 0.0 dB at every 61st bin (bin 0 among them) over -100

Row = namedtuple("Row", "name bins fs start stop x y max_db min_db edge pinned recipe want")

H = 1024000  # half of the default rate


def _r(name, start, stop, x, edge, want, y=255, max_db=0.0, min_db=-120.0, bins=2048, fs=2048000.0, pinned=True, recipe="uniform"):
    return Row(name, bins, fs, start, stop, x, y, max_db, min_db, edge, pinned, recipe, want)


def _w(G, branch, out, direct, avg, max_skipped=0):
    return dict(G=G, branch=branch, out=out, direct=direct, avg=avg, max_skipped=max_skipped)


def _span_wrap_edges():
    """SignalSpectrum::mapFFTZoomedToScreen's quint16 span at 64 kHz, zoom 65536 / 64000 + 0.5 = 1.524: 97536 & 0xffff = 32000"""
    span = int(64000 * (65536.0 / 64000 + 0.5)) & 0xFFFF
    return -(span // 2), span // 2


ROWS = [
    # ---- every lane group in the averaged branch, whole spectrum: 2048 bins on x pixels ----
    _r("g1_bpp_1p5", -H, H, 1365, "g1_skipped_1_2", _w(1, "avg", 0, 683, 682, 2)),
    _r("g1_below_2", -H, H, 1025, "lane_group", _w(1, "avg", 0, 3, 1022, 2)),
    _r("g2_at_2", -H, H, 1024, "lane_group", _w(2, "avg", 0, 2, 1022, 2)),
    _r("g2_nonint", -H, H, 700, "noninteger_bpp", _w(2, "avg", 0, 2, 698, 3)),
    _r("g2_below_4", -H, H, 513, "lane_group", _w(2, "avg", 0, 2, 511, 4)),
    _r("g4_at_4", -H, H, 512, "lane_group", _w(4, "avg", 0, 2, 510, 4)),
    _r("g4_nonint", -H, H, 333, "noninteger_bpp", _w(4, "avg", 0, 2, 331, 7), y=600, max_db=-10.0),
    _r("g8_at_8", -H, H, 256, "lane_group", _w(8, "avg", 0, 2, 254, 8)),
    _r("g8_below_16", -H, H, 129, "lane_group", _w(8, "avg", 0, 2, 127, 16)),
    _r("g16_at_16", -H, H, 128, "lane_group", _w(16, "avg", 0, 2, 126, 16)),
    _r("g32_at_32", -H, H, 64, "lane_group", _w(32, "avg", 0, 2, 62, 32)),
    _r("g32_below_64", -H, H, 33, "lane_group", _w(32, "avg", 0, 2, 31, 63)),
    _r("g64_at_64", -H, H, 32, "lane_group", _w(64, "avg", 0, 2, 30, 64)),
    _r("g64_x7", -H, H, 7, "many_per_lane", _w(64, "avg", 0, 2, 5, 293)),
    _r("g64_x3", -H, H, 3, "many_per_lane", _w(64, "avg", 0, 2, 1, 683)),
    _r("x1", -H, H, 1, "x1", _w(64, "avg", 0, 1, 0, 0), recipe="peaks"),
    # ---- the branch boundary ----
    _r("boundary_equal", -H, H, 2048, "boundary_equal", _w(1, "rep", 0, 2048, 0, 0)),
    # (one bin more than pixels: the averaged branch, but 1.0005 bins per pixel never skip a bin in 2047 pixels -- every read is direct)
    _r("boundary_plus_1", -H, H, 2047, "boundary_plus1", _w(1, "avg", 0, 2047, 0, 0)),
    _r("just_averaged", -H, H, 2000, "g1_skipped_1_2", _w(1, "avg", 0, 1953, 47, 2)),
    # ---- pixel 0 and the pixel behind bin 0, with the left edge below the spectrum; a zoomed range whose pixel 1 IS averaged ----
    _r("bin0_inside_the_plot", -H - 100000, H, 537, "pixel0_and_bin0", _w(4, "avg", 25, 2, 510, 4), max_db=-10.0, min_db=-140.0),
    _r("zoomed_averaged", -H // 2, H // 2, 300, "pixel1_averaged", _w(2, "avg", 0, 1, 299, 4)),
    # (112 bins on 24 pixels from bin -47: i * binsPerPixel is rounded to float BEFORE binLow is added, and that first rounding decides four
    # truncations -- a fused multiply-add reads bin 8 where the reference reads bin 9)
    _r("two_roundings", -1071000, -959000, 24, "two_roundings", _w(4, "avg", 10, 2, 12, 5)),
    # ---- the repeat branch ----
    _r("repeat_int", -20000, 20000, 160, "repeat_int", _w(1, "rep", 0, 160, 0, 0), recipe="peaks"),
    # (252 bins on 288 pixels from bin 19: one of the few geometries where i * binsPerPixel and i / pixelsPerBin truncate to different bins)
    _r("repeat_nonint", -1005000, -753000, 288, "repeat_nonint", _w(1, "rep", 0, 288, 0, 0)),
    _r("repeat_bin_low_m1", -H - 1000, -H + 99000, 400, "repeat_binlow_m1", _w(1, "rep", 1, 399, 0, 0)),
    # ---- range edges (max_db != 0: out of range is -120 without the offset) ----
    _r("right_edge_out", -H, H + 100000, 537, "right_only", _w(4, "avg", 25, 2, 510, 4), max_db=-10.0, min_db=-140.0),
    _r("both_edges_out", -2 * H, 2 * H, 512, "both", _w(8, "avg", 256, 2, 254, 8), max_db=-10.0, min_db=-140.0, recipe="flat"),
    _r("both_edges_out_repeat", -2 * H, 2 * H, 4100, "both", _w(1, "rep", 2049, 2051, 0, 0), y=600, max_db=-10.0, min_db=-140.0),
    _r("wholly_above", 2 * H, 3 * H, 100, "above", _w(8, "avg", 100, 0, 0, 0), max_db=-10.0, min_db=-140.0),
    _r("wholly_below", -3 * H, -2 * H, 1030, "below", _w(1, "rep", 1030, 0, 0, 0), max_db=-10.0, min_db=-140.0),
    # ---- start > stop, start == stop ----
    _r("start_above_stop", 500000, -1500000, 100, "start_gt_stop", _w(1, "rep", 23, 77, 0, 0)),
    _r("start_equals_stop", 0, 0, 37, "start_eq_stop", _w(1, "rep", 0, 37, 0, 0)),
    _r("start_equals_stop_off_centre", 250000, 250000, 160, "start_eq_stop", _w(1, "rep", 0, 160, 0, 0), max_db=-10.0),
    # ---- float rounding of the edges ----
    _r("float_edge_100msps", -49999998, 49999998, 1024, "float_edge", _w(8, "avg", 0, 2, 1022, 8), bins=8192, fs=100e6),
    _r("float_edge_200msps_32768", -99999996, 99999996, 160, "float_edge", _w(64, "avg", 0, 2, 158, 205), bins=32768, fs=200e6),
    # (FFT::fftParams clamps fftSize to 65535, fft.cpp:76-77: the reference cannot be asked for this row; the device's 65536-bin
    # transform exists past that clamp on purpose)
    _r("float_edge_200msps", -99999996, 99999996, 160, "float_edge", _w(64, "avg", 0, 2, 158, 410), bins=65536, fs=200e6, pinned=False),
    # ---- the y rule ----
    _r("y1", -H, H, 64, "y1", _w(32, "avg", 0, 2, 62, 32), y=1, recipe="peaks"),
    _r("y600", -H // 2, H // 2, 150, "y600", _w(4, "avg", 0, 1, 149, 7), y=600),
    _r("range_30_90", -H // 4, H // 4, 160, "min_db", _w(2, "avg", 0, 1, 159, 4), y=255, max_db=-30.0, min_db=-90.0),
    _r("range_30_90_repeat", -50000, 50000, 160, "min_db", _w(1, "rep", 0, 160, 0, 0), y=600, max_db=-30.0, min_db=-90.0),
    _r("range_upside_down", -H // 4, H // 4, 160, "inverted", _w(2, "avg", 0, 1, 159, 4), y=255, max_db=-100.0, min_db=-20.0),
    _r("bin_at_max_db", -61000, 61000, 160, "at_max_db", _w(1, "rep", 0, 160, 0, 0), recipe="peaks"),
    _r("bin_at_max_db_averaged", -H, H, 512, "at_max_db_avg", _w(4, "avg", 0, 2, 510, 4), recipe="peaks"),
    # ---- unpinned: what an x86-64 build does where C says nothing ----
    _r("edge_product_leaves_int32", 1000, 2000000, 64, "int32_overflow", _w(64, "avg", 64, 0, 0, 0), fs=1.0, max_db=-10.0, pinned=False),
    _r("edge_product_leaves_int32_both", -2000000, 2000000, 64, "int32_overflow", _w(1, "rep", 64, 0, 0, 0), fs=1.0, max_db=-10.0, pinned=False),
    # (yScaleFactor = -255 / 1e-7: the product with any powerdB < 0 leaves int32 upward; cvttss2si gives INT_MIN, qBound 0 -- a conversion
    # that saturates, as the device's own instruction does, would give yPixels - 1)
    _r("y_product_leaves_int32", -H, H, 64, "int32_overflow_y", _w(32, "avg", 0, 2, 62, 32), max_db=0.0, min_db=-1e-7, pinned=False),
    _r("zoom_span_wraps", _span_wrap_edges()[0], _span_wrap_edges()[1], 256, "span_wrap", _w(4, "avg", 0, 1, 255, 4), fs=64000.0, pinned=False),
]
# rows whose conversions are all in range and that are unpinned all the same, and why
UNPINNED_IN_RANGE = {"float_edge_200msps": "FFT::fftParams clamps fftSize to 65535 (fft.cpp:76-77)",
                     "zoom_span_wraps": "its edges are the quint16 span of mapFFTZoomedToScreen, a conversion out of range (not pinned)"}
NAMES = [r.name for r in ROWS]
PINNED = [r.name for r in ROWS if r.pinned]


def row(name):
    return next(r for r in ROWS if r.name == name)


# ---- float32 / float64 in plain integers ----
def _rnd(x, p, emin):
    """the Fraction x rounded to the nearest p-bit binary float (ties to even); magnitudes from 2^(emax + 1) on are None (infinite)"""
    x = Fr(x)
    if x == 0:
        return x
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    while Fr(2) ** e > a:
        e -= 1
    while Fr(2) ** (e + 1) <= a:
        e += 1
    q = Fr(2) ** (max(e, emin) - (p - 1))
    n = a / q
    k = n.numerator // n.denominator
    rest = n - k
    if rest > Fr(1, 2) or (rest == Fr(1, 2) and k & 1):
        k += 1
    v = k * q
    assert v < Fr(2) ** (128 if p == 24 else 1024), "overflow to infinity"
    return v if x > 0 else -v


def f32(x):
    return _rnd(x, 24, -126)


def f64(x):
    return _rnd(x, 53, -1022)


def _to_int(v):
    """(qint32) of a float value -> (int, in range); out of range: INT_MIN, as cvttss2si"""
    if v >= -(1 << 31) and v < (1 << 31):
        return int(v), True  # Fraction -> int truncates toward zero
    return INT_MIN, False


def _wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def lane_group(bpp):
    """the lanes that own a pixel: a power of two that doubles while 2 G <= the widest averaged pixel's bins, up to a wave of 64"""
    G = 1
    while G < 64 and 2 * G <= bpp:
        G *= 2
    return G


def plan(r):
    """-> dict: bin_low, bins_to_plot, pixels_per_bin / bins_per_pixel (Fractions; pixels_per_bin None when infinite), averaged, bins
    (every pixel's bin), kind (per pixel 'o' out of range, 'd' direct, 'a' averaged), skipped (per averaged pixel), G, in_range"""
    ok = True
    bph = f32(Fr(r.bins) / f32(Fr(r.fs)))
    lo, a = _to_int(f32(f32(Fr(r.start)) * bph))
    hi, b = _to_int(f32(f32(Fr(r.stop)) * bph))
    ok = ok and a and b
    bin_low, bin_high = lo + r.bins // 2, hi + r.bins // 2
    ok = ok and bin_low == _wrap32(bin_low) and bin_high == _wrap32(bin_high)
    bin_low, bin_high = _wrap32(bin_low), _wrap32(bin_high)
    n = bin_high - bin_low
    ok = ok and n == _wrap32(n)
    n = _wrap32(n)
    ppb = f32(Fr(r.x) / f32(Fr(n))) if n else None  # x / 0.0f = +inf
    bpp = f32(f32(Fr(n)) / Fr(r.x))
    averaged = n > r.x
    bins, kind, skipped = [], [], []
    last = -1
    for i in range(r.x):
        if averaged:
            off = f32(Fr(i) * bpp)
        else:
            off = Fr(0) if ppb is None else f32(Fr(i) / ppb)  # i / inf = 0
        bn, c = _to_int(f32(f32(Fr(bin_low)) + off))
        ok = ok and c
        if bn < 0 or bn >= r.bins:
            kind.append("o")
        elif averaged and last > 0 and bn != last + 1:
            kind.append("a")
            skipped.append(bn - last)
        else:
            kind.append("d")
        last = bn
        bins.append(bn)
    # the y conversion: |yScaleFactor * powerdB - 1| against int32, powerdB within [-120 - maxdB, 0 - maxdB] or -120 for dB in [-120, 0]
    ys = f32(f64(Fr(-r.y) / f64(Fr(r.max_db) - Fr(r.min_db))))
    worst = max(abs(Fr(MIN_DB) - Fr(r.max_db)), abs(Fr(r.max_db)), Fr(-MIN_DB))
    ok = ok and abs(ys) * (worst + 1) + 1 < (1 << 31)
    ok = ok and all(s >= 1 for s in skipped)  # (a window of 0 bins would be 0 / 0, a NaN, and its conversion undefined)
    return dict(bin_low=bin_low, bins_to_plot=n, pixels_per_bin=ppb, bins_per_pixel=bpp, averaged=averaged, bins=bins, kind="".join(kind),
                skipped=skipped, G=lane_group(bpp) if averaged else 1, in_range=ok, y_scale=ys)


def counts(p):
    return dict(G=p["G"], branch="avg" if p["averaged"] else "rep", out=p["kind"].count("o"), direct=p["kind"].count("d"),
                avg=p["kind"].count("a"), max_skipped=max(p["skipped"]) if p["skipped"] else 0)


def check_edge(r):
    """asserts that the row reaches the edge its class names and the counts the table states; -> its plan"""
    p = plan(r)
    c = counts(p)
    assert c == r.want, (r.name, c, r.want)
    assert p["in_range"] == (r.edge not in ("int32_overflow", "int32_overflow_y")), (r.name, p["in_range"])
    assert r.pinned == (p["in_range"] and r.name not in UNPINNED_IN_RANGE), r.name
    e, k, bins = r.edge, p["kind"], p["bins"]
    whole = (p["bin_low"], p["bins_to_plot"]) == (0, r.bins)
    steps = {b - a for a, b in zip(bins, bins[1:])}
    if e == "lane_group":
        assert whole and p["averaged"] and c["avg"] > 0, r.name
    elif e == "g1_skipped_1_2":
        assert whole and p["averaged"] and 1 < p["bins_per_pixel"] < 2 and steps == {1, 2} and set(p["skipped"]) == {2} and c["G"] == 1, r.name
        assert k.count("d") > 2  # the steps of 1 are direct reads (fftBin == lastFftBin + 1)
    elif e == "many_per_lane":
        assert whole and c["G"] == 64 and min(p["skipped"]) > 64, r.name
    elif e == "x1":
        assert whole and r.x == 1 and k == "d" and p["averaged"], r.name
    elif e == "boundary_equal":
        assert p["bins_to_plot"] == r.x and not p["averaged"] and bins == list(range(r.bins)), r.name
    elif e == "boundary_plus1":
        assert p["bins_to_plot"] == r.x + 1 and p["averaged"] and steps == {1} and bins[-1] == r.x - 1, r.name
    elif e == "noninteger_bpp":
        assert whole and p["bins_per_pixel"].denominator != 1 and len(set(p["skipped"])) >= 2, r.name
    elif e == "pixel0_and_bin0":
        j = bins.index(0)
        assert p["averaged"] and j > 0 and bins[j - 1] < 0 and k[j] == "d" and k[j + 1] == "d" and bins[j + 1] > 1 and k[j + 2] == "a", r.name
    elif e == "two_roundings":
        fused = [int(f32(Fr(p["bin_low"]) + Fr(i) * p["bins_per_pixel"])) for i in range(r.x)]  # one rounding
        assert p["averaged"] and p["bin_low"] < 0 and any(a != b and 0 < a < r.bins and 0 < b < r.bins for a, b in zip(fused, bins)), r.name
    elif e == "pixel1_averaged":
        assert p["averaged"] and p["bin_low"] > 0 and k[0] == "d" and k[1] == "a", r.name
    elif e in ("repeat_int", "repeat_nonint"):
        assert not p["averaged"] and 0 < p["bins_to_plot"] < r.x and (p["pixels_per_bin"].denominator == 1) == (e == "repeat_int"), r.name
        assert steps == {0, 1} and k == "d" * r.x, r.name
    elif e == "repeat_binlow_m1":
        assert not p["averaged"] and p["bin_low"] == -1 and bins[0] == -1 and bins.count(0) == 2 * bins.count(1) - 1 and k[0] == "o", r.name
    elif e == "right_only":
        assert bins[0] >= 0 and bins[-1] >= r.bins and k[0] == "d" and k[-1] == "o" and r.max_db != 0, r.name
    elif e == "both":
        assert bins[0] < 0 and bins[-1] >= r.bins and "d" in k and r.max_db != 0, r.name
    elif e == "above":
        assert min(bins) >= r.bins and r.max_db != 0, r.name
    elif e == "below":
        assert max(bins) < 0 and r.max_db != 0, r.name
    elif e == "start_gt_stop":
        assert r.start > r.stop and p["bins_to_plot"] < 0 and not p["averaged"] and steps == {-20} and "o" in k and "d" in k, r.name
    elif e == "start_eq_stop":
        assert r.start == r.stop and p["bins_to_plot"] == 0 and p["pixels_per_bin"] is None and set(bins) == {p["bin_low"]}, r.name
    elif e == "float_edge":
        exact = int(Fr(r.start) * Fr(r.bins) / Fr(r.fs)) + r.bins // 2  # the product in exact arithmetic, truncated
        assert exact != p["bin_low"] and p["bin_low"] == 0 and exact == 1, (r.name, exact, p["bin_low"])
    elif e == "y1":
        assert r.y == 1
    elif e == "y600":
        assert r.y == 600
    elif e == "min_db":
        assert r.min_db != -120.0 and r.max_db < 0 and r.max_db > r.min_db, r.name
    elif e == "inverted":
        assert r.max_db < r.min_db and p["y_scale"] > 0, r.name
    elif e == "at_max_db":
        assert not p["averaged"] and r.max_db == 0.0 and r.recipe == "peaks" and any(b % PEAK_EVERY == 0 for b in bins), r.name
    elif e == "at_max_db_avg":
        assert p["averaged"] and r.max_db == 0.0 and r.recipe == "peaks" and k[0] == "d" and bins[0] == 0, r.name
    elif e == "int32_overflow":
        assert not p["in_range"] and INT_MIN + r.bins // 2 in (p["bin_low"], _wrap32(p["bin_low"] + p["bins_to_plot"])), (r.name, p["bin_low"])
    elif e == "int32_overflow_y":
        assert not p["in_range"] and abs(p["y_scale"]) * 1 >= (1 << 31) and "a" in k and "d" in k, r.name
    elif e == "span_wrap":
        assert (r.start, r.stop) == (-16000, 16000) and int(64000 * (65536.0 / 64000 + 0.5)) == 97536, r.name
    else:
        raise AssertionError("unknown edge %r" % e)
    return p


# ---- inputs: float32 values widened to double, so that the device and the restatement can be fed the same numbers ----
def db_row(bins, recipe, seed=0):
    if recipe == "uniform":
        v = -120.0 * lcg_uniform(bins, 9100 + seed)
    elif recipe == "flat":
        v = np.full(bins, -120.0)
    elif recipe == "peaks":
        v = np.full(bins, -100.0)
        v[::PEAK_EVERY] = 0.0
    else:
        raise AssertionError(recipe)
    return v.astype(np.float32).astype(np.float64)


def row_input(name, recipe=None):
    """the dB row the host tier and the reference pin feed row `name` (recipe None: the row's own)"""
    r = row(name)
    return db_row(r.bins, recipe or r.recipe, NAMES.index(name))


# ---- per-stream geometries: what map_row_plan must give (the zoomed pane of a receiver bank) ----
# (bins, rate, x_pixels, [(start, stop) per stream]); the 70-channel set is tests/test_receiver_display_gpu.py's shape 2
def _zoom64k(off):
    return (-32000 - off, 32000 - off)


STREAM_SETS = {
    "one_for_all": (2048, 64000.0, 256, [_zoom64k(0)] * 5, False),
    "four_repeat": (2048, 64000.0, 4096, [_zoom64k(o) for o in (0, 500, -700, 1234)], True),
    "seventy_two_chunks": (2048, 64000.0, 256, [_zoom64k(0 if c == 5 else (c * 37) % 401 - 200) for c in range(70)], True),
    "sixty_five_last_alone": (2048, 64000.0, 100, [_zoom64k(c) for c in range(64)] + [(-3200, 3200)], True),
}


def stream_plan(name):
    """-> per stream (plan, G): the lane group is the widest averaged pixel's of the stream's chunk of 64 (per_stream) or of stream 0"""
    bins, fs, x, edges, per_stream = STREAM_SETS[name]
    plans = [plan(_r("s%d" % i, e[0], e[1], x, "", None, bins=bins, fs=fs)) for i, e in enumerate(edges)]
    out = []
    for s, p in enumerate(plans):
        if per_stream:
            chunk = plans[(s // 64) * 64:(s // 64) * 64 + 64]
        else:
            chunk, p = [plans[0]], plans[0]
        widest = max([q["bins_per_pixel"] for q in chunk if q["averaged"]] or [Fr(0)])
        out.append((p, lane_group(widest)))
    return out
