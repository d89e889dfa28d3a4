"""CPU tier of the stream bank's update gate (pebblegpu_streambank_set_spectrum_updates / _spectrum_frames): the two entry points in
header, library and binding, and the model the GPU tests hold the library to (tests/streambank_gate_ref.py) on selections worked out
by hand.  No compute call is made here: without a device the bank refuses to exist."""
import ctypes
import os
import re

import pytest

from tests.spectrum_gate_ref import select as select_global

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pebblegpu_streambank_set_spectrum_updates", "pebblegpu_streambank_spectrum_frames"]


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    return g.build()


def test_header_declares_the_two_calls():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pebblegpu.h")).read(), flags=re.S)
    assert re.search(r"int pebblegpu_streambank_set_spectrum_updates\s*\(\s*pebblegpu_streambank \*\w+,\s*int \w+\)", code)
    assert re.search(r"int pebblegpu_streambank_spectrum_frames\s*\(\s*const pebblegpu_streambank \*\w+,\s*uint32_t \*\w+,\s*uint32_t \w+,\s*"
                     r"uint32_t \*\w+\)", code)
    assert re.search(r"#define\s+PEBBLEGPU_ABI_VERSION\s+1\b", code)


def test_library_exports_them_and_the_listed_pass_a(lib_path):
    L = ctypes.CDLL(lib_path)
    assert not [f for f in NEW if not hasattr(L, f)]
    assert L.pebblegpu_abi_version() == 1  # additive: the version stays
    blob = open(lib_path, "rb").read()
    assert blob.count(b"k_big256_cols_list") >= 6  # float2 input and the five converting instances


def test_binding_lists_them_and_streambank_has_the_methods(lib_path):
    from pebblesdr_amd import binding as B
    for name in NEW:
        assert name in B.SYMBOLS
        assert getattr(B.load_library(), name).argtypes is not None
    assert callable(B.StreamBank.set_spectrum_updates) and callable(B.StreamBank.spectrum_frames)


def test_hand_worked_selections():
    from tests.streambank_gate_ref import select
    # 200 Msps, 65536-sample frames (0.32768 ms each), 10 per second: 100 ms is 305.2 frames
    assert select_global(65536, 200_000_000, 10, [1000]) == [306, 612, 918]
    # 2 MHz: a frame is 32.768 ms.  20 per second (50 ms): every second frame; 40 per second (25 ms): every frame
    assert select(65536, 2_000_000, 20, [3, 1, 4, 2]) == [[2], [], [0, 2], [0]]
    assert select(65536, 2_000_000, 40, [4, 3, 1]) == [[1, 2, 3], [0, 1, 2], [0]]
    # 2048-sample frames are 1.024 ms: 250 per second (4 ms) is every fourth frame
    assert select(2048, 2_000_000, 250, [6, 2, 9, 4]) == [[4], [], [0, 4, 8], [3]]


def test_a_call_without_the_spectrum_advances_the_clock_only():
    from tests.streambank_gate_ref import BankGateTimer
    t = BankGateTimer(65536, 2_000_000)
    t.set_updates(20)
    assert t.call(3) == [2]          # frame 0 starts the timer, frame 2 is 65 ms on
    t.skip(2)                        # frames 3 and 4: f_last stays 2
    assert (t.next, t.f_last) == (5, 2)
    assert t.call(3) == [0, 2]       # global frames 5 and 7
    u = BankGateTimer(65536, 2_000_000)
    u.set_updates(20)
    u.skip(4)                        # a skipped call does not start the timer either
    assert not u.started and u.call(3) == [2] and u.f_last == 6
