"""CPU tier of the display map's geometry table (tests/screen_cases.py; FFT::mapFFTToScreen, pebblelib/fft.cpp:411-534).

 - csrc/screen_geom.h -- the functions the kernels and launchers call for a pixel's bin, the y rule and a launch's lane group -- is
   compiled here with g++ -ffp-contract=off into a small program and held, row by row, to the table's plain-integer planner and to
   tests/screen_map_ref.py's geometry()/pixel_bins(); map_row_plan to the planner's per-stream statement.  The same program is built a
   second time with AddressSanitizer and UBSan (float-cast-overflow included: x86_trunc must never make an out-of-range conversion) and
   run stand-alone.
 - every row reaches the edge its class names (screen_cases.check_edge).
 - the oracle's serial mapFFTToScreen (oracle/pebble_oracle.c, pinned to the reference's compiled code by the mapscreen_* cases of
   tests/test_reference_pins.py on the rows' own recipe) against the restatement, every row x every recipe: exact on every pixel the
   restatement does not flag as lying within 1e-9 of an integer, `alt` accepted on a flagged one, no flagged pixel on the uniform recipe.
   With the reference binary present it is run on every pinned row x recipe too and must equal the oracle exactly.
 - every row discriminates: a deliberately wrong variant of the restatement, chosen for the row's edge, changes at least one pixel of
   the row on its pinned input (or, where pixels cannot tell, the row's geometry: see GEOMETRY_ONLY).
"""
import os
import subprocess

import numpy as np
import pytest

from tests import reference_cases as RC
from tests import screen_cases as S
from tests import screen_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")

MAIN = r"""#include <cstdio>
#include <cstring>
#include <vector>
#include "screen_geom.h"
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static void put(const pg::MapGeom &g) { std::printf("%d %d %08x %08x", g.bin_low, g.bins_to_plot, bits(g.pixels_per_bin), bits(g.bins_per_pixel)); }
int main()
{
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        int bins, x, y;
        double fs, mx, mn;
        if (kind == 'R') {  // one row: geometry, lane group (as run_screen_map plans a launch of one geometry), y scale, every pixel's bin
            int e[2];
            if (std::scanf("%d %lf %d %d %d %d %lf %lf", &bins, &fs, &e[0], &e[1], &x, &y, &mx, &mn) != 8) return 2;
            pg::MapGeom g;
            const int G = pg::map_chunk_plan(bins, fs, e, false, 0, 1, x, &g);
            const bool averaged = g.bins_to_plot > x;
            put(g);
            std::printf(" %d %d %08x |", (int)averaged, G, bits(pg::map_y_scale(y, mx, mn)));
            for (int i = 0; i < x; i++) std::printf(" %d", pg::map_bin(g, averaged, i));
            std::printf(" | %d %d %d\n", pg::map_y(pg::map_y_scale(y, mx, mn), -120, y), pg::map_y(pg::map_y_scale(y, mx, mn), (int)-mx, y),
                        pg::map_lane_group(averaged ? g.bins_per_pixel : 0.0f));
        } else if (kind == 'S') {  // per-stream rows: map_row_plan
            int n, per;
            if (std::scanf("%d %lf %d %d %d", &bins, &fs, &x, &per, &n) != 5) return 2;
            std::vector<int> e(2 * n), groups(n);
            std::vector<pg::MapGeom> geoms(n);
            for (int k = 0; k < 2 * n; k++)
                if (std::scanf("%d", &e[k]) != 1) return 2;
            pg::map_row_plan(bins, fs, e.data(), per != 0, n, x, geoms.data(), groups.data());
            for (int k = 0; k < n; k++) { put(geoms[k]); std::printf(" %d ;", groups[k]); }
            std::printf("\n");
        } else if (kind == 'T') {  // x86_trunc at the limits
            std::printf("%d %d %d %d %d %d\n", pg::x86_trunc(2147483648.0f), pg::x86_trunc(-2147483648.0f), pg::x86_trunc(2147483520.0f),
                        pg::x86_trunc(2147483647.9), pg::x86_trunc(-2147483648.9), pg::x86_trunc(-2147483649.0));
            std::printf("%d %d %d\n", pg::x86_trunc(0.0f / 0.0f), pg::x86_trunc(-0.75f), pg::x86_trunc(1e300));
        } else {
            return 2;
        }
    }
    return 0;
}
"""


def _f32_bits(v):
    """a planner value (Fraction; None: +inf) -> the bits of the float32 it is"""
    f = np.float32(np.inf) if v is None else np.float32(float(v))
    assert v is None or float(f) == float(v)
    return int(f.view(np.uint32))


def _input_text():
    lines = ["R %d %r %d %d %d %d %r %r" % (r.bins, r.fs, r.start, r.stop, r.x, r.y, r.max_db, r.min_db) for r in S.ROWS]
    for name in S.STREAM_SETS:
        bins, fs, x, edges, per = S.STREAM_SETS[name]
        lines.append("S %d %r %d %d %d %s" % (bins, fs, x, int(per), len(edges), " ".join("%d %d" % e for e in edges)))
    lines.append("T")
    return "\n".join(lines) + "\n"


def _build(d, flags, name):
    src, exe = d / "screen_geom_main.cpp", str(d / name)
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off"] + flags + ["-I" + CSRC, str(src), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def header_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("screen_geom")
    exe = _build(d, [], "plain")
    out = subprocess.run([exe], input=_input_text(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return d, out.stdout


@pytest.fixture(scope="module")
def plans():
    return {r.name: S.check_edge(r) for r in S.ROWS}


def _row_line(line):
    head, bins, tail = line.split("|")
    h = head.split()
    return dict(bin_low=int(h[0]), bins_to_plot=int(h[1]), ppb=int(h[2], 16), bpp=int(h[3], 16), averaged=bool(int(h[4])), G=int(h[5]),
                y_scale=int(h[6], 16), bins=[int(v) for v in bins.split()], tail=[int(v) for v in tail.split()])


# ---- the header against the planner and the restatement ----
def test_header_matches_the_planner_on_every_row(header_out, plans):
    lines = header_out[1].strip().split("\n")
    assert len(lines) == len(S.ROWS) + len(S.STREAM_SETS) + 2
    for r, line in zip(S.ROWS, lines):
        got, p = _row_line(line), plans[r.name]
        want = dict(bin_low=p["bin_low"], bins_to_plot=p["bins_to_plot"], ppb=_f32_bits(p["pixels_per_bin"]), bpp=_f32_bits(p["bins_per_pixel"]),
                    averaged=p["averaged"], G=p["G"], y_scale=_f32_bits(p["y_scale"]), bins=p["bins"])
        tail = got.pop("tail")
        assert got == want, (r.name, {k: (got[k], want[k]) for k in want if got[k] != want[k] and k != "bins"})
        assert got["G"] == r.want["G"] and tail[2] == got["G"], r.name   # display_pack_plan's call of map_lane_group gives the launch's group
        # the restatement's geometry (numpy float32) is the same arithmetic
        g = R.geometry(r.bins, r.fs, r.start, r.stop, r.x)
        assert (g["bin_low"], g["bins_to_plot"], bool(g["averaged"])) == (p["bin_low"], p["bins_to_plot"], p["averaged"]), r.name
        assert int(np.float32(g["pixels_per_bin"]).view(np.uint32)) == want["ppb"] and int(np.float32(g["bins_per_pixel"]).view(np.uint32)) == want["bpp"], r.name
        assert R.pixel_bins(g, r.x).tolist() == p["bins"], r.name
        assert int(np.float32(R.y_scale(r.y, r.max_db, r.min_db)).view(np.uint32)) == want["y_scale"], r.name
        # map_y of powerdB -120 and of -maxdB, against to_y
        ys = R.y_scale(r.y, r.max_db, r.min_db)
        assert tail[:2] == [int(R.to_y(np.int32(-120), ys, r.y)), int(R.to_y(np.int32(int(-r.max_db)), ys, r.y))], r.name


def test_lane_group_thresholds_are_the_tables():
    """every group is in the table at its threshold (bins per pixel exactly 2, 4 .. 64) and just below the next one: a threshold moved
    either way changes some row's G, which the test above holds to the header"""
    at = {r.want["G"] for r in S.ROWS if r.name.endswith(("_at_2", "_at_4", "_at_8", "_at_16", "_at_32", "_at_64"))}
    below = {r.want["G"] for r in S.ROWS if "_below_" in r.name}
    assert at == {2, 4, 8, 16, 32, 64} and below == {1, 2, 8, 32}
    assert {r.want["G"] for r in S.ROWS if r.want["branch"] == "avg" and r.want["avg"] > 0} == {1, 2, 4, 8, 16, 32, 64}
    for r in S.ROWS:
        if r.name.endswith(("_at_2", "_at_4", "_at_8", "_at_16", "_at_32", "_at_64")):
            assert S.plan(r)["bins_per_pixel"] == r.want["G"], r.name
        if "_below_" in r.name:
            assert r.want["G"] < S.plan(r)["bins_per_pixel"] < 2 * r.want["G"] and 2 * r.want["G"] == int(r.name.rsplit("_", 1)[1]), r.name


def test_map_row_plan_per_stream(header_out):
    lines = header_out[1].strip().split("\n")[len(S.ROWS):len(S.ROWS) + len(S.STREAM_SETS)]
    seen = {}
    for name, line in zip(S.STREAM_SETS, lines):
        got = [e.split() for e in line.split(";") if e.strip()]
        want = S.stream_plan(name)
        assert len(got) == len(want), name
        for s, (g, (p, G)) in enumerate(zip(got, want)):
            assert (int(g[0]), int(g[1]), int(g[2], 16), int(g[3], 16), int(g[4])) == \
                (p["bin_low"], p["bins_to_plot"], _f32_bits(p["pixels_per_bin"]), _f32_bits(p["bins_per_pixel"]), G), (name, s)
        seen[name] = [G for _, G in want]
    assert seen["one_for_all"] == [8] * 5 and seen["four_repeat"] == [1] * 4
    assert seen["seventy_two_chunks"] == [8] * 64 + [4] * 6                      # two chunks, two lane groups
    assert seen["sixty_five_last_alone"] == [16] * 64 + [2]                      # a chunk of one stream


def test_x86_trunc_at_the_limits(header_out):
    a, b = header_out[1].strip().split("\n")[-2:]
    assert [int(v) for v in a.split()] == [S.INT_MIN, S.INT_MIN, 2147483520, 2147483647, S.INT_MIN, S.INT_MIN]
    assert [int(v) for v in b.split()] == [S.INT_MIN, 0, S.INT_MIN]


def test_header_under_the_sanitizers(header_out):
    """the same program, AddressSanitizer + UBSan (with float-cast-overflow), as a stand-alone run: same output, no report"""
    d, plain = header_out
    exe = _build(d, ["-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"], "sanitized")
    out = subprocess.run([exe], input=_input_text(), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    assert out.stdout == plain


# ---- every row reaches its edge ----
@pytest.mark.parametrize("name", S.NAMES)
def test_row_reaches_its_edge(name):
    S.check_edge(S.row(name))


def test_the_table_covers_what_it_promises():
    edges = {r.edge for r in S.ROWS}
    assert edges >= {"g1_skipped_1_2", "lane_group", "many_per_lane", "x1", "boundary_equal", "boundary_plus1", "noninteger_bpp", "pixel0_and_bin0",
                     "pixel1_averaged", "two_roundings", "repeat_int", "repeat_nonint", "repeat_binlow_m1", "right_only", "both", "above", "below", "start_gt_stop",
                     "start_eq_stop", "float_edge", "y1", "y600", "min_db", "inverted", "at_max_db", "int32_overflow", "int32_overflow_y", "span_wrap"}
    assert {r.y for r in S.ROWS} >= {1, 255, 600}
    assert all(r.pinned for r in S.ROWS if r.name not in S.UNPINNED_IN_RANGE and not r.edge.startswith("int32_overflow"))
    assert (S.row("zoom_span_wraps").start, S.row("zoom_span_wraps").stop) == R.zoom_edges(64000, 65536.0 / 64000 + 0.5)
    assert R.zoom_edges(64000, 65536.0 / 64000 + 0.5) != (-(97536 // 2), 97536 // 2)
    # a pinned fixture holds the whole record wherever x_pixels <= 512 (reference_cases.TAIL)
    assert sum(r.x <= 160 for r in S.ROWS if r.pinned) >= 18


# ---- the restatement against the oracle ----
def _near(v, tol=1e-9):
    with np.errstate(invalid="ignore"):
        return np.abs(v - np.round(v)) <= tol * np.maximum(1.0, np.abs(v))


@pytest.mark.parametrize("name", S.NAMES)
def test_restatement_against_the_oracle(oracle_mod, name):
    r = S.row(name)
    have_binary = r.pinned and os.path.exists(RC.BINARY)
    for recipe in S.RECIPES:
        db = S.row_input(name, recipe)
        args = (r.bins, r.fs, r.y, r.x, r.max_db, r.min_db, r.start, r.stop)
        orc = oracle_mod.map_fft_to_screen(db, *args)
        out, v, alt = R.map_fft_to_screen(db, *args)
        scal = R.map_scalar(db, *args)
        flagged = _near(v)
        assert not flagged[np.isnan(v)].any()
        for what, got in (("map_fft_to_screen", out), ("map_scalar", scal)):
            exact = got == orc
            assert exact[~flagged].all(), (name, recipe, what, np.argwhere(~exact & ~flagged)[:4].ravel(), got[~exact][:4], orc[~exact][:4])
            assert ((got == orc) | (alt == orc)).all(), (name, recipe, what)
        if recipe == "uniform":
            assert int(flagged.sum()) == 0, (name, int(flagged.sum()))
        if have_binary:
            ref = RC.run_driver("mapscreen", db, list(args))
            assert len(ref) == 1 and np.array_equal(ref[0], orc.astype(np.float64)), (name, recipe)


def test_the_y_rows_do_what_their_names_say(oracle_mod):
    """from the oracle's pixels: a 1-pixel plot is all 0; the -30..-90 range clamps at both ends on the uniform recipe; the upside-down
    range is not constant; a bin at max_db comes out as 0 (y = -1, bound) beside neighbours that do not; the yScaleFactor that leaves
    int32 gives 0 on every pixel (INT_MIN, bound), where a saturating conversion would give yPixels - 1"""
    def px(name, recipe=None):
        r = S.row(name)
        return r, oracle_mod.map_fft_to_screen(S.row_input(name, recipe), r.bins, r.fs, r.y, r.x, r.max_db, r.min_db, r.start, r.stop)
    assert set(px("y1")[1].tolist()) == {0}
    for name in ("range_30_90", "range_30_90_repeat"):
        r, p = px(name)
        assert p.min() == 0 and len(set(p.tolist())) > 10, name
        assert p.max() == r.y - 1 or name == "range_30_90"  # (the power mean of three or four uniform bins is never under -90 dB)
        assert set(px(name, "peaks")[1].tolist()) == {0, r.y - 1}, name  # -100 dB under the range, a window with a 0 dB bin over it
    assert len(set(px("range_upside_down")[1].tolist())) > 10
    r, p = px("bin_at_max_db")
    bins = S.plan(r)["bins"]
    peak = np.array([b % S.PEAK_EVERY == 0 for b in bins])
    assert peak.any() and (p[peak] == 0).all() and (p[~peak] == int(R.to_y(np.int32(-100), R.y_scale(r.y, 0.0, -120.0), r.y))).all()
    assert set(px("y_product_leaves_int32")[1].tolist()) == {0}
    for name in ("wholly_above", "wholly_below"):   # powerdB = -120 without the maxdB offset: the bottom row, not 10 dB above it
        r, p = px(name)
        bottom = int(R.to_y(np.int32(-120), R.y_scale(r.y, r.max_db, r.min_db), r.y))
        assert set(p.tolist()) == {bottom} and bottom < r.y - 1 and bottom != int(R.to_y(np.int32(-110), R.y_scale(r.y, r.max_db, r.min_db), r.y)), name


# ---- every row discriminates ----
def _conv(f, variant, saturate=False):
    """float / double -> int32 as the variant converts"""
    f = float(f)
    if f != f:
        return S.INT_MIN
    if variant == "round":
        f = float(np.round(f))
    elif variant == "floor":
        f = float(np.floor(f))
    if -2147483649.0 < f < 2147483648.0:
        return int(f)
    return (2147483647 if f > 0 else S.INT_MIN) if saturate else S.INT_MIN


def variant_geometry(r, variant):
    f = np.float32
    with np.errstate(all="ignore"):
        start, stop = (r.stop, r.start) if variant == "swap_edges" and r.start > r.stop else (r.start, r.stop)
        if variant == "double_edges":
            bph = np.float64(r.bins) / np.float64(r.fs)
            lo, hi = _conv(start * bph, None), _conv(stop * bph, None)
        else:
            bph = f(r.bins) / f(r.fs)
            sat = variant == "saturate"
            lo, hi = _conv(f(start) * bph, None, sat), _conv(f(stop) * bph, None, sat)
        bin_low, bin_high = R.wrap32(lo + r.bins // 2), R.wrap32(hi + r.bins // 2)
        n = R.wrap32(bin_high - bin_low)
        return dict(bin_low=bin_low, bins_to_plot=n, pixels_per_bin=f(r.x) / f(n), bins_per_pixel=f(n) / f(r.x),
                    averaged=(n >= r.x) if variant == "averaged_ge" else (n > r.x))


def variant_map(db, r, variant=None):
    """the reference's loop, pixel by pixel, with one deliberate mistake (variant None: none -- equal to screen_map_ref.map_scalar)"""
    f = np.float32
    g = variant_geometry(r, variant)
    with np.errstate(all="ignore"):
        rng = np.float64(r.max_db) - np.float64(-120.0 if variant == "min_db_ignored" else r.min_db)
        if variant == "abs_range":
            rng = abs(rng)
        ys = np.float64(-r.y) / rng
        if variant != "y_scale_double":
            ys = f(ys)

        def bin_of(i):
            if g["averaged"] or variant == "bpp_in_repeat":
                if variant == "fused_offset":
                    return _conv(f(np.float64(g["bin_low"]) + np.float64(i) * np.float64(g["bins_per_pixel"])), None)
                off = f(i) * g["bins_per_pixel"]
            else:
                off = f(i) / g["pixels_per_bin"]
            return _conv(f(g["bin_low"]) + off, variant if variant in ("round", "floor") else None)

        conv = variant if variant == "round" else None
        out, last = [], -1
        for i in range(r.x):
            b = bin_of(i)
            if variant == "empty_is_silent" and g["bins_to_plot"] == 0:
                pdb = S.MIN_DB
            elif b < 0 or b >= r.bins:
                pdb = _conv(S.MIN_DB - r.max_db, None) if variant == "offset_out_of_range" else S.MIN_DB
            elif g["averaged"] and (last >= 0 if variant == "last_ge_0" else last > 0) and b != last + 1:
                lo, hi = (b, min(max(bin_of(i + 1), b + 1), r.bins)) if variant == "window_next" else (last, b)
                w = db[lo:hi]
                if variant == "db_mean":
                    val = np.float64(w.mean())
                else:
                    t = 0.0
                    for x in w:
                        t += 10.0 ** (float(x) / 10.0)
                    p = np.float64(t) / np.float64(hi - lo)
                    val = S.MIN_DB if p == 0.0 else 10.0 * np.log10(p)
                pdb = _conv(val - r.max_db, conv)
            else:
                pdb = _conv(float(db[b]) - r.max_db, conv)
            last = b
            y = _conv((ys * f(pdb) - f(1.0)) if variant != "y_scale_double" else (ys * np.float64(pdb) - 1.0), conv, variant == "saturate")
            out.append(y if variant == "no_bound" else min(max(y, 0), r.y - 1))
    return np.array(out, dtype=np.int64)


AVERAGING = ["window_next", "db_mean"]
VARIANTS_OF_EDGE = {
    "lane_group": AVERAGING, "g1_skipped_1_2": AVERAGING, "many_per_lane": AVERAGING, "noninteger_bpp": AVERAGING, "pixel1_averaged": AVERAGING,
    "at_max_db_avg": AVERAGING, "two_roundings": ["fused_offset"],
    # (x_pixels 1 on the "peaks" recipe: bin 0 holds 0.0 dB = maxdB, y = -1; a 1-pixel-high plot: any y but -1 is bound to 0 either way)
    "x1": ["no_bound"], "y1": ["no_bound"], "at_max_db": ["no_bound"],
    # (where bins and pixels are equal or one apart both branches read the same bins: a wrong branch cannot show; a wrong conversion does)
    "boundary_equal": ["round"], "boundary_plus1": ["round"],
    "pixel0_and_bin0": ["offset_out_of_range"],
    # (with a whole number of pixels per bin i * binsPerPixel and i / pixelsPerBin agree on every pixel: rounding the quotient shows there)
    "repeat_int": ["round"], "repeat_nonint": ["bpp_in_repeat"], "repeat_binlow_m1": ["floor"],
    "right_only": ["offset_out_of_range"], "both": ["offset_out_of_range"], "above": ["offset_out_of_range"], "below": ["offset_out_of_range"],
    "start_gt_stop": ["swap_edges"], "start_eq_stop": ["empty_is_silent"], "float_edge": ["double_edges"],
    "y600": ["round"] + AVERAGING, "min_db": ["min_db_ignored", "no_bound"], "inverted": ["abs_range"],
    "int32_overflow_y": ["saturate"], "span_wrap": AVERAGING,
}
# rows whose mistake cannot show in a pixel -- the plotted range lies so far outside the spectrum that every pixel is out of range either
# way -- and shows in the geometry, which test_header_matches_the_planner_on_every_row holds to the planner
GEOMETRY_ONLY = {"int32_overflow": "saturate"}


@pytest.mark.parametrize("name", S.NAMES)
def test_row_discriminates(name):
    r = S.row(name)
    db = S.row_input(name)
    args = (r.bins, r.fs, r.y, r.x, r.max_db, r.min_db, r.start, r.stop)
    right = variant_map(db, r)
    assert np.array_equal(right, R.map_scalar(db, *args)), name   # the variant machine without a mistake is the restatement
    if r.edge in GEOMETRY_ONLY:
        a, b = variant_geometry(r, None), variant_geometry(r, GEOMETRY_ONLY[r.edge])
        assert (a["bins_to_plot"], a["averaged"]) != (b["bins_to_plot"], b["averaged"]), name
        assert np.array_equal(right, variant_map(db, r, GEOMETRY_ONLY[r.edge])), name   # ... and indeed not in a pixel
        return
    variants = list(VARIANTS_OF_EDGE[r.edge])
    p = S.plan(r)
    behind_bin0 = [j for j in range(1, r.x) if p["bins"][j - 1] == 0 and p["kind"][j] == "d" and p["bins"][j] > 1]
    if p["averaged"] and behind_bin0 and r.recipe == "uniform" and r.pinned and r.y > 1:   # a pixel whose predecessor read bin 0 and that skipped bins: direct only because of lastFftBin > 0
        variants.append("last_ge_0")
    assert "last_ge_0" in variants or r.edge not in ("pixel0_and_bin0", "many_per_lane", "noninteger_bpp"), name
    for variant in variants:
        wrong = variant_map(db, r, variant)
        assert (wrong != right).any(), "%s: the variant %s changes no pixel" % (name, variant)


def test_every_variant_of_the_issue_is_used():
    used = {v for vs in VARIANTS_OF_EDGE.values() for v in vs}
    assert used >= {"window_next", "offset_out_of_range", "fused_offset", "bpp_in_repeat", "round", "db_mean"}
    assert {r.edge for r in S.ROWS} == set(VARIANTS_OF_EDGE) | set(GEOMETRY_ONLY)
    assert sum("last_ge_0" not in VARIANTS_OF_EDGE.get(r.edge, []) for r in S.ROWS) == len(S.ROWS)  # (added per row, from the plan)
