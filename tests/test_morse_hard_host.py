"""CPU tier of tests/morse_hard_cases.py: which branch arms of the restated decoder the keying rows take, measured.

The restatement itself is held to the reference's compiled decoder on the same rows by tests/test_reference_pins.py (cases
morse_hard_*, morse_stream_64000); the device is held to both by tests/test_morse_hard_gpu.py.
"""
import numpy as np
import pytest

from tests import morse_cases as MC
from tests import morse_hard_cases as H
from tests import morse_ref as M

# The arms the rows from before tests/morse_hard_cases.py never take (the morse_cases stream and test_morse_gpu's step streams: TEST /
# MORSE at 15, 25 and 40 WPM with the mode change), on record: 12 that input can reach, and the two of H.UNREACHABLE
# (ut.last_mark_zero, sm.inter.char_empty).
OLD_ROWS_MISS = ["ut.last_mark_zero", "ut.ratio_outside", "ut.below_range", "ut.above_range", "ut.pull_down", "ut.pull_up",
                 "sm.mark.short_to_idle", "sm.mark.short_to_mark", "sm.mark.short_to_inter", "sm.mark.short_to_word",
                 "sm.inter.tone_pending", "sm.inter.buffer_full", "sm.inter.char_empty", "sm.inter.past_word"]

GEOMETRIES = ((H.RATE, H.FRAME), (H.SLOW_RATE, MC.min_frame(H.SLOW_RATE)))


def test_the_hard_rows_take_every_arm_that_can_be_taken():
    per_row = {n: H.reference(n).arms for n in H.NAMES}
    total = H.arms_of(H.reference(n) for n in H.NAMES)
    old = H.old_rows_arms()
    print("%-24s %9s %9s  first hard row that takes it" % ("arm", "old rows", "hard rows"))
    for a in H.ARMS:
        first = next((n for n in H.NAMES if per_row[n][a]), "unreachable" if a in H.UNREACHABLE else "-")
        print("%-24s %9d %9d  %s" % (a, old[a], total[a], first))
    assert set(H.UNREACHABLE) <= set(H.ARMS)
    for a in H.ARMS:
        if a in H.UNREACHABLE:
            assert total[a] == 0 and old[a] == 0, a    # an arm on that list that is taken after all: the argument is wrong
        else:
            assert total[a] > 0, a


def test_the_rows_from_before_miss_these_arms():
    old = H.old_rows_arms()
    assert [a for a in H.ARMS if not old[a]] == OLD_ROWS_MISS
    assert sorted(H.UNREACHABLE) == ["sm.inter.char_empty", "ut.last_mark_zero"] and set(H.UNREACHABLE) <= set(OLD_ROWS_MISS)
    assert len(OLD_ROWS_MISS) - len(H.UNREACHABLE) == 12 and len(H.ARMS) - len(H.UNREACHABLE) == 38


def test_each_row_takes_the_arm_it_is_there_for():
    want = {"spike1": ("sm.mark.short_to_idle", "sm.mark.short_to_inter"), "spike2": ("sm.mark.short_to_mark", "sm.mark.short_to_word"),
            "dropout": ("sm.inter.tone_pending",), "pending_long": ("sm.inter.tone_pending", "sm.inter.past_word"), "nine_dots": ("sm.inter.buffer_full",), "wpm8": ("ut.below_range",),
            "wpm60": ("sm.mark.short_to_mark", "ut.above_range"), "fast_2to1": ("ut.above_range",), "wpm11": ("ut.pull_up",),
            "wpm49": ("ut.above_range",), "pull_down": ("ut.pull_down",), "ratio_out": ("ut.ratio_outside", "ut.ratio_between"),
            "fade12": ("tp.peak_decay", "tp.hold_tone"), "mode_rate_midchar": ("ut.force",)}
    for name, arms in want.items():
        for a in arms:
            assert H.reference(name).arms[a] > 0, (name, a)
    assert H.reference("mode_rate_midchar").arms["ut.force"] == 2
    # the space that passes the word threshold in one result ends the character without an event: the dash of 60 ms is not decoded
    assert H.reference("pending_long").arms["sm.inter.past_word"] == 1 and H.reference("dropout").arms["sm.inter.past_word"] == 0
    assert [M.morse_dotdash(t) for _, t, k in H.reference("pending_long").events if k == M.CHAR] == [".", "-", "."]
    # the six-element token that is no character comes out as a token; the ninth dot ends the character without an event
    ev = H.reference("nonchar6").events
    assert [M.morse_dotdash(t) for _, t, k in ev if k == M.CHAR] == ["-", "....-.", ".-"] and H.stars_of("nonchar6", ev) == [1]
    assert all(len(M.morse_dotdash(t)) < 9 for n in H.NAMES for _, t, k in H.reference(n).events if k == M.CHAR)
    assert [M.morse_dotdash(t) for _, t, k in H.reference("nine_dots").events if k == M.CHAR] == [".", "."]
    # the speed change moves the estimate up and down again; the out-of-range rows end with their flag up
    sp = H.reference("speed_15_35_15")
    assert [s["wpm"] for s, _ in sp.seen][1] > sp.seen[0][0]["wpm"] and sp.seen[-1][0]["wpm"] < max(s["wpm"] for s, _ in sp.seen)
    assert H.reference("wpm8").status()["below_range"] == 1 and H.reference("fast_2to1").status()["above_range"] == 1


@pytest.mark.parametrize("name", H.NAMES)
def test_every_row_keeps_the_margin_at_both_geometries(name):
    """the condition of every row: no restated decision within 1e-4 of a threshold, the spike results included; a row whose last
    events decode to a text (Row.tail) does so at both"""
    for rate, frame in GEOMETRIES:
        ref = H.reference(name, rate, frame)
        if H.row(name).tail:
            want = M.text_tokens(H.row(name).tail)
            assert [(k, t) for _, t, k in ref.events][-len(want):] == want, (name, rate)
        print("%s %d / %d: %d results, smallest margin %.3e" % (name, rate, frame, len(ref.powers), min(ref.margins)))
        assert len(ref.powers) > 100 and min(ref.margins) > H.MARGIN == 1e-4, (name, rate, frame, min(ref.margins))
    # at the slow geometry most calls complete no Goertzel block
    _, total, _, n = MC.geometry(H.SLOW_RATE)
    assert GEOMETRIES[1][1] // total < n // 4


def test_the_unreachable_arms_are_unreachable():
    """the inequalities of H.UNREACHABLE, on the numbers: at every modem rate the project runs and on every reading of every row"""
    shortest = int(M.DOT_MAGIC / (M.WPM_HIGH * 1.10))
    assert shortest == 21818 > 0 and M.DOT_MAGIC // M.WPM_HIGH == 24000 > 0                     # ut.last_mark_zero
    # the thresholds are written by the in-range arm alone, where DOT_MAGIC // dot <= WPM_HIGH: dot > DOT_MAGIC / (WPM_HIGH + 1)
    dot_min = M.DOT_MAGIC // (M.WPM_HIGH + 1) + 1
    assert M.DOT_MAGIC // dot_min == M.WPM_HIGH and M.DOT_MAGIC // (dot_min - 1) == M.WPM_HIGH + 1
    for wpm in range(5, M.WPM_HIGH + 1):                                                       # ... and by init's forced update
        d = M.DOT_MAGIC // wpm
        assert ((3 * d + d) // 2) // 2 >= dot_min
    for dot in list(range(1, 4096)) + [dot_min, 24000, 60000, 240000]:                         # sm.inter.char_empty
        assert 2 * dot > int(dot * 0.25)
    for name in H.NAMES:
        for rate, frame in GEOMETRIES:
            ref = H.reference(name, rate, frame)
            for _, (wpm, above, below, mr, n, ddt, element, char_thr, word_thr, short) in ref.seen:
                assert 0 <= element < char_thr and short == shortest and ddt // 2 >= dot_min


def test_the_segment_keying_is_morse_ref_keying_on_paris_timing():
    """the generator beside morse_ref.keying gives its envelope, sample for sample, where the timing is PARIS"""
    for wpm, rate in ((25, 64000), (15, 12000), (40, 31250)):
        want = M.keying("TEST MORSE", wpm, rate, tail_s=7 * 1.2 / wpm)
        got = H.envelope(H.text("TEST MORSE", wpm, amp=1.0), rate)
        assert np.array_equal(got, want)
