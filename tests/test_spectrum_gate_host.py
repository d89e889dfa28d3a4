"""CPU tier: the spectrum update gate's selection rule (tests/spectrum_gate_ref.py, the model the GPU tests hold the library to) on the
selections worked out by hand in the issue, and the new entry points declared in header and binding."""
import os
import re

from tests.spectrum_gate_ref import EVERY_FRAME, GateTimer, LatestRow, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_worked_selections():
    assert select(2048, 20_000_000, 10, [3000]) == [977, 1954, 2931]
    assert select(2048, 2_048_000, 10, [350]) == [100, 200, 300]
    assert select(2048, 1_000_000, 30, [60]) == [17, 34, 51]       # period 1000 // 30 = 33 ms
    assert select(2048, 100_000_000, 10, [10000]) == [4883, 9766]


def test_zero_updates_select_nothing_and_frame_zero_is_never_selected():
    assert select(2048, 2_048_000, 0, [4096]) == []
    for ups in (1, 10, 30, 1000, 5000):   # (1000 // 5000 = 0 ms: every frame but the one that starts the timer)
        sel = select(2048, 2_048_000, ups, [64])
        assert 0 not in sel
    assert select(2048, 2_048_000, 5000, [8]) == [1, 2, 3, 4, 5, 6, 7]


def test_default_selects_every_frame():
    assert select(2048, 2_048_000, EVERY_FRAME, [5, 3]) == list(range(8))


def test_selection_does_not_depend_on_the_split_into_calls():
    for fs, ups in ((2_048_000, 10), (20_000_000, 10), (1_000_000, 30), (2_048_000, 7)):
        one = select(2048, fs, ups, [4096])
        assert one == select(2048, fs, ups, [1024] * 4)
        assert one == select(2048, fs, ups, [1, 999, 17, 2000, 1079])
        assert len(one) >= 3


def test_rate_change_mid_stream_keeps_f_last():
    t = GateTimer(2048, 2_048_000)
    t.set_updates(10)
    assert t.call(250) == [100, 200]
    t.set_updates(20)                       # period 50 ms: counted from frame 200, not from the change
    assert t.call(100) == [0, 50]           # frames 250 and 300
    t.set_updates(0)
    assert t.call(500) == []                # the timer keeps its f_last = 300
    t.set_updates(10)
    assert t.call(10) == [0]                # frame 850: long overdue
    assert t.f_last == 850


def test_from_every_frame_to_a_rate_counts_from_the_previous_calls_last_frame():
    t = GateTimer(2048, 2_048_000)
    assert t.call(64) == list(range(64))
    t.set_updates(10)
    assert t.call(200) == [99, 199]         # frames 163 = 63 + 100 and 263
    u = GateTimer(2048, 2_048_000)          # no call before the change: the first frame starts the timer
    u.set_updates(10)
    assert u.call(201) == [100, 200]


def test_latest_row_model():
    m = LatestRow()
    assert m.at(1000) is None
    m.add([100, 200])
    assert m.at(99) is None and m.at(100) == 0 and m.at(199) == 0 and m.at(200) == 1 and m.at(10 ** 6) == 1


def test_new_symbols_are_declared_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "pebblegpu.h")).read()
    from pebblesdr_amd.binding import SYMBOLS, ReceiverBank
    for name in ("pebblegpu_set_spectrum_updates", "pebblegpu_receiver_spectrum_frames", "pebblegpu_process_iq_updates"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in SYMBOLS
    assert re.search(r"#define\s+PEBBLEGPU_SPECTRUM_EVERY_FRAME\s+\(-1\)", hdr)
    assert "forced open" not in hdr
    assert callable(ReceiverBank.set_spectrum_updates) and callable(ReceiverBank.spectrum_frames)
    import pebblesdr_amd as P
    assert P.SPECTRUM_EVERY_FRAME == -1
