"""CPU tier: the receiver's display ring (pebblegpu_receiver_display_*) as far as it goes without a device -- the refusals that need
none, the binding's structures against the header's (sizes and field offsets, printed by a C program compiled against
include/pebblegpu.h), and that the plain-C host example compiles and links.  tests/test_receiver_display_gpu.py holds the ring and its
packing kernel to the map functions on the device.
"""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

PANE_FIELDS = ["struct_size", "source", "format", "max_rows", "map", "zoom", "mode_offset", "rows", "n_rows", "reserved"]
BLOCK_FIELDS = ["struct_size", "format", "call_index", "host", "rows_per_stream", "first_row", "row_elems", "n_streams", "dropped_before",
                "reserved", "row_pitch_bytes", "stream_pitch_bytes"]
MAP_FIELDS = ["struct_size", "y_pixels", "x_pixels", "max_db", "min_db", "start_freq", "stop_freq", "reserved"]


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd
    return pebblesdr_amd


def test_refusals_without_a_device(P):
    L = P.load_library()
    n = C.c_uint64()
    blocks = (P.DisplayBlock * 2)()
    blocks[0].struct_size = blocks[1].struct_size = C.sizeof(P.DisplayBlock)
    pane = P.display_pane(P.PANE_SPECTRUM, P.DISPLAY_DB_F32)
    assert L.pebblegpu_receiver_display_open(None, C.byref(pane), 1, 4) == E_INVALID
    assert b"null" in L.pebblegpu_last_error()
    assert L.pebblegpu_receiver_display_close(None) == E_INVALID
    assert L.pebblegpu_receiver_display_next(None, 0, blocks) == E_INVALID
    assert L.pebblegpu_receiver_display_release(None, 0) == E_INVALID
    assert L.pebblegpu_receiver_display_dropped(None, C.byref(n)) == E_INVALID
    assert L.pebblegpu_receiver_display_set_pane(None, 0, C.byref(pane)) == E_INVALID


def test_display_pane_helper_fills_the_structure(P):
    screen = P.screen_map(255, 301, 0.0, -120.0, -1000, 2000)
    p = P.display_pane(P.PANE_ZOOM, P.DISPLAY_WATERFALL_ARGB32, screen, zoom=0.25, mode_offset=[5, -7, 9], rows=[2, 0], max_rows=3)
    assert p.struct_size == C.sizeof(P.DisplayPane)
    assert (p.source, p.format, p.max_rows, p.n_rows, p.zoom) == (1, 2, 3, 2, 0.25)
    assert (p.map.struct_size, p.map.y_pixels, p.map.x_pixels, p.map.start_freq, p.map.stop_freq) == (C.sizeof(P.ScreenMap), 255, 301, -1000, 2000)
    assert [p.mode_offset[i] for i in range(3)] == [5, -7, 9] and [p.rows[i] for i in range(2)] == [2, 0]
    q = P.display_pane(P.PANE_SPECTRUM, P.DISPLAY_DB_F32)
    assert not q.rows and not q.mode_offset and q.n_rows == 0 and q.max_rows == 0  # NULL: all rows; every row a call computes


def test_binding_structures_match_the_header(P, tmp_path):
    """sizeof and every offsetof of the three structures the ring's calls exchange, as a C compiler lays the header out"""
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pebblegpu.h"', 'int main(void) {']
    for tag, fields in (("pebblegpu_display_pane", PANE_FIELDS), ("pebblegpu_display_block", BLOCK_FIELDS), ("pebblegpu_screen_map", MAP_FIELDS)):
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (tag, tag))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (tag, f, tag, f))
    lines.append('printf("enums %d %d %d\\n", (int)PEBBLEGPU_PANE_SPECTRUM, (int)PEBBLEGPU_PANE_ZOOM, (int)PEBBLEGPU_DISPLAY_MAX_PANES);')
    lines += ['return 0;', '}']
    src, exe = tmp_path / "layout.c", str(tmp_path / "layout")
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
               if not line.startswith("enums"))
    for tag, cls, fields in (("pebblegpu_display_pane", P.DisplayPane, PANE_FIELDS), ("pebblegpu_display_block", P.DisplayBlock, BLOCK_FIELDS),
                             ("pebblegpu_screen_map", P.ScreenMap, MAP_FIELDS)):
        assert int(out[tag]) == C.sizeof(cls), tag
        assert [name for name, *_ in cls._fields_] == fields, tag
        for f in fields:
            assert int(out["%s.%s" % (tag, f)]) == getattr(cls, f).offset, (tag, f)
    assert (P.PANE_SPECTRUM, P.PANE_ZOOM, P.binding.DISPLAY_MAX_PANES) == (0, 1, 2)
    assert "enums 0 1 2" in subprocess.run([exe], capture_output=True, text=True, check=True).stdout


def test_c_host_example_compiles_and_links(P, tmp_path):
    """compile and link only: running it needs a device"""
    src, exe = os.path.join(ROOT, "examples", "receiver_display_host.c"), str(tmp_path / "receiver_display_host")
    libdir = os.path.join(ROOT, "pebblesdr_amd")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lpebblegpu",
                        "-Wl,-rpath," + libdir, "-lm", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(exe)
