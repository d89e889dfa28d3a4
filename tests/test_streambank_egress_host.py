"""CPU tier: the host twin of the display ring's colour rule (pebblegpu_waterfall_colors) against the restatement of
SpectrumWidget's palette and drawWaterfall (tests/waterfall_ref.py), the refusals that need no device, and that the plain-C stream
bank host example compiles and links.

The twin runs the same inline function the packing kernel runs (pebblesdr_amd/csrc/kernels_display.h);
tests/test_streambank_egress_gpu.py holds the kernel to the restatement on the device.
"""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import waterfall_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

# (index, (r, g, b)) of the palette, worked out by hand from spectrumwidget.cpp:97-113
ANCHORS = [(0, (0, 0, 0)), (1, (0, 0, 5)), (42, (0, 0, 249)), (43, (0, 0, 255)), (86, (0, 255, 255)), (87, (0, 255, 255)),
           (119, (0, 255, 0)), (120, (0, 255, 0)), (153, (255, 255, 0)), (154, (255, 255, 0)), (216, (255, 0, 0)), (217, (255, 0, 0)),
           (254, (255, 0, 124)), (255, (255, 0, 128))]
PALETTE_CRC = 0xB58668E3


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd
    return pebblesdr_amd


def test_twin_equals_the_restatement_for_every_pixel_value(P):
    v = np.arange(256, dtype=np.int32)
    got = P.waterfall_colors(v)
    assert got.dtype == np.uint32 and got.shape == v.shape
    assert np.array_equal(got, W.waterfall(v))
    assert np.array_equal(got[::-1], W.palette())      # pixel v reads entry 255 - v
    assert (got >> 24 == 0xFF).all()                   # QColor::setRgb: alpha 255
    px = np.random.default_rng(9).integers(0, 256, size=(3, 5, 301)).astype(np.int32)
    assert np.array_equal(P.waterfall_colors(px), W.waterfall(px))
    assert P.waterfall_colors(np.zeros(0, dtype=np.int32)).shape == (0,)


def test_anchors_and_crc(P):
    pal = P.waterfall_colors(255 - np.arange(256, dtype=np.int32))   # the table itself, entry 0 first
    for i, (r, g, b) in ANCHORS:
        assert W.palette_rgb(i) == (r, g, b), i
        assert int(pal[i]) == 0xFF000000 | (r << 16) | (g << 8) | b, i
    assert zlib.crc32(pal.astype("<u4").tobytes()) == PALETTE_CRC
    assert zlib.crc32(W.palette().astype("<u4").tobytes()) == PALETTE_CRC


@pytest.mark.parametrize("bad", [-1, 256])
def test_pixels_outside_the_table_are_refused(P, bad):
    with pytest.raises(P.PebbleGpuError) as e:
        P.waterfall_colors(np.asarray([0, 255, bad, 7], dtype=np.int32))
    assert e.value.code == E_INVALID


def test_refusals_without_a_device(P):
    L = P.load_library()
    assert C.sizeof(P.DisplayBlock) == 64
    blk, dblk, n = P.AudioBlock(), P.DisplayBlock(), C.c_uint64()
    blk.struct_size, dblk.struct_size = C.sizeof(P.AudioBlock), C.sizeof(P.DisplayBlock)
    assert L.pebblegpu_streambank_iq_out_open(None, 0, None, 0, 4) == E_INVALID
    assert L.pebblegpu_streambank_iq_out_close(None) == E_INVALID
    assert L.pebblegpu_streambank_iq_out_next(None, 0, C.byref(blk)) == E_INVALID
    assert L.pebblegpu_streambank_iq_out_release(None, 0) == E_INVALID
    assert L.pebblegpu_streambank_iq_out_dropped(None, C.byref(n)) == E_INVALID
    assert L.pebblegpu_streambank_display_open(None, 0, None, None, 0, 0, 4) == E_INVALID
    assert L.pebblegpu_streambank_display_close(None) == E_INVALID
    assert L.pebblegpu_streambank_display_next(None, 0, C.byref(dblk)) == E_INVALID
    assert L.pebblegpu_streambank_display_release(None, 0) == E_INVALID
    assert L.pebblegpu_streambank_display_dropped(None, C.byref(n)) == E_INVALID
    assert L.pebblegpu_waterfall_colors(None, 4, None) == E_INVALID
    assert L.pebblegpu_waterfall_colors(None, 0, None) == 0   # nothing to convert


def test_c_host_example_compiles_and_links(P, tmp_path):
    """compile and link only: running it needs a device"""
    src, exe = os.path.join(ROOT, "examples", "streambank_host.c"), str(tmp_path / "streambank_host")
    libdir = os.path.join(ROOT, "pebblesdr_amd")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lpebblegpu",
                        "-Wl,-rpath," + libdir, "-lm", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(exe)
