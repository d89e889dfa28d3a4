"""CPU tier of the stream bank's S-meter and squelch: the declarations, pebblegpu_stream_gate's layout as a C compiler lays the header
out, and the host twin pebblegpu_signal_strength_row against the oracle's SignalStrength::fdEstimate.
tests/test_streambank_smeter_gpu.py holds the device kernel, the gate and the IQ ring's trailer to the same oracle.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.signals import lcg_uniform
from tests.test_abi_symbols import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NEW = ["pebblegpu_signal_strength_row", "pebblegpu_streambank_enable_signal_strength", "pebblegpu_streambank_signal_strength",
       "pebblegpu_streambank_set_squelch", "pebblegpu_streambank_iq_out_gate"]
GATE_FIELDS = ["peak_db", "avg_db", "snr_db", "floor_db", "open", "row"]

# (bins, sample rate, [(bp_lo, bp_hi)]): both noise windows clamp; bpHighBin clamps to `bins`; one bin; the lower edge; bpBins == 0
WINDOWS_2M = [(-5000, 5000), (-900000, 900000), (300000, 1000000), (-1, 1), (-1023000, -1000000), (100, 200)]
CASES = [(2048, 2048000, WINDOWS_2M), (8192, 2048000, WINDOWS_2M), (65536, 200000000, [(-40e6, 40e6), (-99e6, 99e6), (10e6, 10.1e6)])]


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd
    return pebblesdr_amd


def db_row(bins, seed):
    """a noise floor near -100 dB (6 dB of ripple) with one -30 dB bin just above the centre"""
    row = (-100.0 + 6.0 * (lcg_uniform(bins, seed) - 0.5)).astype(np.float32)
    row[bins // 2 + 3] = -30.0
    return row


def test_the_new_names_are_declared_exported_and_bound(P):
    declared = header_functions()
    L = C.CDLL(P.library_path())
    from pebblesdr_amd.binding import SYMBOLS
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in SYMBOLS, name
    assert sorted(SYMBOLS) == sorted(declared)
    txt = open(os.path.join(ROOT, "include", "pebblegpu.h")).read()
    assert "typedef struct pebblegpu_stream_gate {" in txt
    assert L.pebblegpu_abi_version() == 1
    for m in ("enable_signal_strength", "signal_strength", "set_squelch", "iq_out_gate"):
        assert callable(getattr(P.StreamBank, m)), m


def test_binding_structure_matches_the_header(P, tmp_path):
    """sizeof and every offsetof of pebblegpu_stream_gate, and the two row marks, as a C compiler lays the header out"""
    tag = "pebblegpu_stream_gate"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pebblegpu.h"', 'int main(void) {', 'printf("%s %%zu\\n", sizeof(%s));' % (tag, tag)]
    for f in GATE_FIELDS:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (tag, f, tag, f))
    lines.append('printf("marks %u %u\\n", (unsigned)PEBBLEGPU_GATE_ROW_CARRIED, (unsigned)PEBBLEGPU_GATE_ROW_NONE);')
    lines += ['return 0;', '}']
    src, exe = tmp_path / "layout.c", str(tmp_path / "layout")
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    out = dict(line.rsplit(" ", 1) for line in text.splitlines() if not line.startswith("marks"))
    assert int(out[tag]) == C.sizeof(P.StreamGateEntry) == P.STREAM_GATE.itemsize == 24
    assert [name for name, *_ in P.StreamGateEntry._fields_] == GATE_FIELDS == list(P.STREAM_GATE.names)
    for f in GATE_FIELDS:
        assert int(out["%s.%s" % (tag, f)]) == getattr(P.StreamGateEntry, f).offset == P.STREAM_GATE.fields[f][1], f
    assert "marks %u %u" % (P.GATE_ROW_CARRIED, P.GATE_ROW_NONE) in text and (P.GATE_ROW_CARRIED, P.GATE_ROW_NONE) == (0xFFFFFFFE, 0xFFFFFFFF)


def test_host_twin_equals_the_oracle(P, oracle_mod):
    """The twin is the reference's serial loop in double over the same libm; it reports float (the header's float out[4], what the device
    reports), so the oracle's doubles are narrowed the same way before the comparison: 1e-9 dB.  The (100, 200) window has bpBins == 0 and
    one bin in band: avg is x / 0 = +inf -> 0 dB, and the noise average 0 / 0, which the reference's qBound returns as its lower bound:
    snr 0, floor -120 (tests/test_reference_pins.py, cases fdestimate_*).  Every output of every window is finite."""
    seen = 0
    for bins, rate, windows in CASES:
        row = db_row(bins, 1000 + bins)
        for lo, hi in windows:
            want = oracle_mod.fd_estimate(row.astype(np.float64), rate, lo, hi, 0.0)
            got = P.signal_strength_row(row, rate, lo, hi, 0.0)
            name = "%d bins, (%g, %g)" % (bins, lo, hi)
            print(name, want, got)
            if (lo, hi) == (100, 200):
                assert want[1] == 0.0 and want[2] == 0.0 and want[3] == -120.0, (name, want)
                assert got[1] == 0.0 and got[2] == 0.0 and got[3] == np.float32(-120.0), (name, got)
            assert np.isfinite(want).all() and np.isfinite(got).all(), (name, want, got)
            for k in range(4):
                assert abs(float(got[k]) - float(np.float32(want[k]))) <= 1e-9, (name, k, got, want)
            seen += 1
    assert seen == 15
    # the peak bin inside the window: peakDb is the -30 dB bin, and avgDb follows it
    got = P.signal_strength_row(db_row(2048, 3048), 2048000, -5000, 5000)
    assert got[0] == np.float32(-30.0) and -45.0 < got[1] < -35.0 and 60.0 < got[2] < 80.0 and -105.0 < got[3] < -95.0


def test_mixer_frequency_moves_the_window(P, oracle_mod):
    """1.5 MHz clamps the mixer's bin to `bins`: the window is what is left of (-5000, 5000) under the upper edge; every value is finite"""
    row = db_row(2048, 5)
    for mixer in (-400000.0, 123456.0, 1.5e6):
        want = oracle_mod.fd_estimate(row.astype(np.float64), 2048000, -5000, 5000, mixer)
        got = P.signal_strength_row(row, 2048000, -5000, 5000, mixer)
        assert np.isfinite(want).all() and np.isfinite(got).all(), (mixer, want, got)
        for k in range(4):
            assert abs(float(got[k]) - float(np.float32(want[k]))) <= 1e-9, (mixer, k, got, want)


def test_refusals_without_a_device(P):
    L = P.load_library()
    row = np.zeros(2048, dtype=np.float32)
    out = np.zeros(4, dtype=np.float32)
    rp, op = row.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.pebblegpu_signal_strength_row(None, 2048, 2048000, -1.0, 1.0, 0.0, op) == E_INVALID
    assert L.pebblegpu_signal_strength_row(rp, 2048, 2048000, -1.0, 1.0, 0.0, None) == E_INVALID
    assert L.pebblegpu_signal_strength_row(rp, 0, 2048000, -1.0, 1.0, 0.0, op) == E_INVALID
    assert L.pebblegpu_signal_strength_row(rp, 2048, 2047, -1.0, 1.0, 0.0, op) == E_INVALID      # an integer bin width of 0
    assert L.pebblegpu_signal_strength_row(rp, 2048, 2048, -1.0, 1.0, 0.0, op) == 0
    n, rows, pitch = C.c_uint32(), C.c_uint64(7), C.c_uint64(7)
    assert L.pebblegpu_streambank_enable_signal_strength(None, 1) == E_INVALID
    assert b"null" in L.pebblegpu_last_error()
    assert L.pebblegpu_streambank_set_squelch(None, 0, -50.0) == E_INVALID
    assert L.pebblegpu_streambank_iq_out_gate(None, 0, None, 0, C.byref(n)) == E_INVALID
    assert not L.pebblegpu_streambank_signal_strength(None, C.byref(rows), C.byref(pitch)) and rows.value == 0 and pitch.value == 0
