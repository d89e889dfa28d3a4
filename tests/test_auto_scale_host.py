"""CPU tier of the display rings' auto-scale (SpectrumWidget::recalcScale): the host twin pebblegpu_auto_scale_row against the
restatement tests/auto_scale_ref.py, the NULL-handle refusals of the new calls, and pebblegpu_display_scale's layout as a C compiler
lays the header out.  tests/test_auto_scale_gpu.py holds the device kernel, the pull functions and the rings to the same restatement.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import auto_scale_ref as A
from tests.signals import lcg_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
BINS = 2048
SCALE_FIELDS = ["max_db", "min_db", "avg_power", "peak_power"]


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd
    return pebblesdr_amd


def rows():
    """(name, float32 row of 2048 bins): noise floors from -115 to -20 dB with 6 dB of ripple, a single 0 dB bin, all -120"""
    out = []
    for k, level in enumerate(range(-115, -15, 5)):
        out.append(("floor %d dB" % level, (level + 6.0 * (lcg_uniform(BINS, 100 + k) - 0.5)).astype(np.float32)))
    one = (-100.0 + 6.0 * (lcg_uniform(BINS, 77) - 0.5)).astype(np.float32)
    one[777] = 0.0
    out.append(("a single 0 dB bin", one))
    out.append(("all -120 dB", np.full(BINS, -120.0, dtype=np.float32)))
    return out


def test_host_twin_equals_the_restatement(P):
    seen = set()
    for name, row in rows():
        want = A.scale_rows(row[None, :])[0]           # (asserts the row is safe: no row is excluded)
        max_db, min_db, avg, peak = P.auto_scale_row(row)
        assert (max_db, min_db) == (want["max_db"], want["min_db"]), name
        assert abs(avg - want["avg_power"]) <= 1e-15 * want["avg_power"], (name, avg, want["avg_power"])   # serial fp64 over the same libm
        assert abs(peak - want["peak_power"]) <= 1e-15 * want["peak_power"], (name, peak, want["peak_power"])
        seen.add((max_db, min_db))
    assert len(seen) >= 8, seen                         # the rows exercise the rule, not one clamp
    assert P.auto_scale_row(np.full(BINS, -120.0, dtype=np.float32))[:2] == (-50, -120)
    assert P.auto_scale_row(rows()[-2][1])[0] == 0      # a 0 dB peak: 10 -> clamped to 0


def test_the_rule_in_small():
    """the restatement itself on hand-computed rows: C division toward zero, the truncation, the bounds"""
    assert [A.c_div5(v) for v in (-7, -5, -4, 4, 7, -132)] == [-5, -5, 0, 0, 5, -130]
    r = A.scale_row([-60.0] * 8)                        # avg = peak = 1e-6: -70 -> -70; -50 -> -50
    assert (r["max_db"], r["min_db"]) == (-50, -70)
    r = A.scale_row([-33.0] * 7 + [-12.5])              # peak -12.5 + 10 = -2.5 -> (int) -2 -> 0
    assert r["max_db"] == 0 and r["min_db"] == -70      # avg about -21.5 - 10 -> -31 -> -30, bound to -70
    r = A.scale_row([-97.3] * 16)                       # -107.3 -> -107 -> -105; -87.3 -> -87 -> -85 -> bound to -50
    assert (r["max_db"], r["min_db"]) == (-50, -105)
    assert not A.is_safe(dict(q_avg=-93.0000001, q_peak=-33.3))
    assert A.is_safe(dict(q_avg=-130.0, q_peak=-110.0))  # all -120 dB: both candidates clamp to the same limit
    assert A.is_safe(dict(q_avg=-93.5, q_peak=10.0))     # a 0 dB peak


def test_refusals_without_a_device(P):
    L = P.load_library()
    n = C.c_uint32()
    out = (P.DisplayScale * 4)()
    row = np.zeros(BINS, dtype=np.float32)
    assert L.pebblegpu_auto_scale_row(None, BINS, out) == E_INVALID
    assert L.pebblegpu_auto_scale_row(row.ctypes.data_as(C.c_void_p), BINS, None) == E_INVALID
    assert L.pebblegpu_auto_scale_row(row.ctypes.data_as(C.c_void_p), 0, out) == E_INVALID
    for who in ("receiver", "streambank"):
        assert getattr(L, "pebblegpu_%s_spectrum_scale" % who)(None, 0, 1, 1, None) == E_INVALID
        assert b"null" in L.pebblegpu_last_error()
        assert getattr(L, "pebblegpu_%s_display_set_auto_scale" % who)(None, 3) == E_INVALID
        assert getattr(L, "pebblegpu_%s_display_rescale" % who)(None) == E_INVALID
        assert getattr(L, "pebblegpu_%s_display_scale" % who)(None, 0, out, 4, C.byref(n)) == E_INVALID


def test_binding_structure_matches_the_header(P, tmp_path):
    """sizeof and every offsetof of pebblegpu_display_scale, and the flag values, as a C compiler lays the header out"""
    tag = "pebblegpu_display_scale"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pebblegpu.h"', 'int main(void) {', 'printf("%s %%zu\\n", sizeof(%s));' % (tag, tag)]
    for f in SCALE_FIELDS:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (tag, f, tag, f))
    lines.append('printf("flags %d %d\\n", (int)PEBBLEGPU_AUTO_SCALE_MAX, (int)PEBBLEGPU_AUTO_SCALE_MIN);')
    lines += ['return 0;', '}']
    src, exe = tmp_path / "layout.c", str(tmp_path / "layout")
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    out = dict(line.rsplit(" ", 1) for line in text.splitlines() if not line.startswith("flags"))
    assert int(out[tag]) == C.sizeof(P.DisplayScale) == P.DISPLAY_SCALE.itemsize == 24
    assert [name for name, *_ in P.DisplayScale._fields_] == SCALE_FIELDS == list(P.DISPLAY_SCALE.names)
    for f in SCALE_FIELDS:
        assert int(out["%s.%s" % (tag, f)]) == getattr(P.DisplayScale, f).offset == P.DISPLAY_SCALE.fields[f][1], f
    assert "flags 1 2" in text and (P.AUTO_SCALE_MAX, P.AUTO_SCALE_MIN) == (1, 2)
