"""CPU tier of the Morse stations (pebblegpu_morse_station_plan, pebblegpu_morse_station_marks): the library's host-side plan and its
per-call mark table against the serial restatement in tests/morsegen_ref.py.  No device is needed for either."""
import ctypes as C
import math

import pytest

from tests import morsegen_ref as G

E_INVALID, E_UNSUPPORTED = -1, -6
TEXT = "CQ DE K1ABC "


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd as P
    P.load_library()
    return P


def restated(fs, wpm, ms_rise, tokens, f=1000.0, amp=0.5):
    g = G.MorseGenRef(fs)
    g.set_params(f, amp, wpm, ms_rise)
    g.set_text_out(tokens)
    return g


def test_restatement_pins():
    """48 ms per Tcw at 25 wpm; at 64 kHz 3072 samples, 320 of rise: dot 320 + 2752 + 320, dash 320 + 8896 + 320; the word space is 7 Tcw - 3
    SAMPLES; the envelope is ampInc (i + 1), amp, amp - ampInc (i + 1) and the carrier restarts at every mark"""
    g = restated(64000, 25, 5, G.text_tokens("A E"), f=1000.0, amp=0.5)
    assert (g.spt, g.rise, g.n_dot_buf, g.n_dash_buf, g.n_word) == (3072, 320, 3392, 9536, 7 * 3072 - 3)
    x, key = g.generate(2 * g.lengths()[4])
    period = g.lengths()[4]
    assert period == 3392 + 3072 + 9536 + 3 * 3072 + (7 * 3072 - 3) + 3392 + 3 * 3072
    assert g.mark_starts[:3] == [(0, False), (3392 + 3072, True), (3392 + 3072 + 9536 + 3 * 3072 + 7 * 3072 - 3, False)]
    assert g.mark_starts[3] == (period, False)                       # the text starts over with nothing in between
    assert (x[~key] == 0).all() and key.sum() == 2 * (2 * 3392 + 9536)
    a = abs(x)
    assert math.isclose(a[0], 0.5 / 320) and math.isclose(a[319], 0.5) and a[320] == pytest.approx(0.5) and a[3392 - 1] <= 2 * 320 * 2.0 ** -53   # (the serial ramp: 2 x 320 additions below 0.5)
    s = 3392 + 3072
    assert x[s].imag == 0.0 and x[s].real == pytest.approx(0.5 / 320)  # phase 0 at the dash's first sample
    assert math.isclose(math.atan2(x[s + 1000].imag, x[s + 1000].real), (2 * math.pi * 1000 * 1000 / 64000) % (2 * math.pi) - 2 * math.pi, abs_tol=1e-9)


@pytest.mark.parametrize("fs", [64000, 200000, 2048000, 20e6])
@pytest.mark.parametrize("wpm", [5, 13, 25, 50])
@pytest.mark.parametrize("ms_rise", [0, 5, 20])
def test_plan_against_the_restatement(P, fs, wpm, ms_rise):
    toks = G.text_tokens(TEXT)
    # (the restatement's lengths need no buffers: set the sizes with a mark-free text first, then ask for the real one's period)
    g = G.MorseGenRef(fs)
    ms_tcw = 1200 // wpm
    spt = int(ms_tcw / (1000.0 / fs))
    rise = int(ms_rise / (1000 / fs))
    g.spt, g.rise, g.fall = spt, rise, rise
    g.n_dot_buf, g.n_dash_buf = rise + rise + (spt - (rise + rise) // 2), rise + rise + (3 * spt - (rise + rise) // 2)
    g.n_element, g.n_char, g.n_word = spt, 3 * spt, 7 * spt - 3
    g.tokens = toks
    st = P.morse_station(1234.5, 0.1, wpm, ms_rise, toks)
    assert P.morse_station_plan(fs, st) == g.lengths()


def test_plan_equals_the_generated_stream(P):
    """the restatement's own buffers and the period it actually generates, at a rate small enough to run the serial loops"""
    for wpm, ms_rise in ((50, 0), (40, 5), (13, 20)):
        toks = G.text_tokens(TEXT)
        g = restated(64000, wpm, ms_rise, toks)
        plan = P.morse_station_plan(64000, P.morse_station(1000.0, 0.5, wpm, ms_rise, toks))
        assert plan == g.lengths() and (len(g.dot_buf), len(g.dash_buf)) == plan[2:4]
        g.generate(plan[4] + 1)
        n_marks = sum(t.bit_length() - 1 for t in toks if t)
        assert g.mark_starts[n_marks] == (plan[4], g.mark_starts[0][1]) and g.mark_starts[0][0] == 0


def test_plan_refusals(P):
    fs = 200000
    ok = G.text_tokens("E")

    def code(st, rate=fs):
        with pytest.raises(P.PebbleGpuError) as e:
            P.morse_station_plan(rate, st)
        return e.value.code

    L = P.load_library()
    v = C.c_uint64()
    assert L.pebblegpu_morse_station_plan(float(fs), None, C.byref(v), None, None, None, None) == E_INVALID       # null struct
    st = P.morse_station(1000.0, 0.1, 25, 5, ok)
    st.struct_size -= 4
    assert code(st) == E_INVALID                                                                                   # mis-sized
    assert code(P.morse_station(float("nan"), 0.1, 25, 5, ok)) == E_INVALID
    assert code(P.morse_station(1000.0, float("inf"), 25, 5, ok)) == E_INVALID
    assert code(P.morse_station(fs / 2, 0.1, 25, 5, ok)) == E_INVALID
    assert code(P.morse_station(-fs / 2, 0.1, 25, 5, ok)) == E_INVALID
    assert code(P.morse_station(1000.0, 0.1, 25, 5, [])) == E_INVALID
    assert code(P.morse_station(1000.0, 0.1, 25, 5, [0x200])) == E_INVALID
    assert code(P.morse_station(1000.0, 0.1, 0, 5, ok)) == E_UNSUPPORTED                                           # wpm 0
    assert code(P.morse_station(1000.0, 0.1, 1201, 5, ok)) == E_UNSUPPORTED                                        # msTcw 0
    assert code(P.morse_station(10.0, 0.1, 1200, 0, ok), 900.0) == E_UNSUPPORTED                                   # samplesPerTcw 0
    assert code(P.morse_station(1000.0, 0.1, 50, 24, ok)) == E_UNSUPPORTED                                         # the dot wraps: rise == Tcw
    assert code(P.morse_station(1000.0, 0.1, 50, 30, ok)) == E_UNSUPPORTED
    assert code(P.morse_station(1000.0, 0.1, 1, 0, ok), 20e6) == E_UNSUPPORTED                                     # dash of 7.2e7 >= 2^26 samples
    assert code(P.morse_station(1000.0, 0.1, 5, 0, [0x1FF] * 40000), 20e6) == E_UNSUPPORTED                        # period >= 2^40
    # what is allowed: the largest token, hard keying, a rise one sample short of the Tcw, a frequency just inside fs/2
    assert P.morse_station_plan(fs, P.morse_station(fs / 2 - 1.0, 0.1, 50, 0, [0x1FF, 1, 0]))[1] == 0
    spt, rise, dot, dash, _ = P.morse_station_plan(fs, P.morse_station(1000.0, 0.1, 50, 23, ok))
    assert (spt, rise, dot, dash) == (4800, 4600, 4600 + 200 + 4600, 4600 + 3 * 4800 - 4600 + 4600)


SIZES = [1, 4099, 65536, 30001]


@pytest.mark.parametrize("wpm,ms_rise,text", [(50, 5, "TEST "), (40, 0, "CQ DE K1ABC "), (13, 20, "E")])
def test_mark_table_against_the_restatement(P, wpm, ms_rise, text):
    """a text cut into calls of 1, 4099, 65536, 30001, ... samples over more than two passes: every call's table is exactly the
    restatement's marks that intersect the call -- the text's wrap-around and marks that straddle calls included"""
    fs = 64000
    toks = G.text_tokens(text)
    g = restated(fs, wpm, ms_rise, toks)
    st = P.morse_station(1000.0, 0.5, wpm, ms_rise, toks)
    period = P.morse_station_plan(fs, st)[4]
    total = 2 * period + 70000
    g.generate(total + 4 * g.n_dash_buf)        # (far enough that every mark starting before `total` is listed)
    ref = [(s, d, s + (g.n_dash_buf if d else g.n_dot_buf)) for s, d in g.mark_starts]
    pos, k, straddles, wrapped = 0, 0, 0, False
    while pos < total:
        n = SIZES[k % len(SIZES)]
        k += 1
        want = [(s - pos, d) for s, d, e in ref if e > pos and s < pos + n]
        got = P.morse_station_marks(fs, st, pos, n)
        assert got == want, (pos, n)
        straddles += sum(1 for s, _ in got if s < 0)
        wrapped |= pos + n > period and any(s >= 0 for s, _ in got)
        pos += n
    assert straddles > 3 and wrapped


def test_a_mark_that_straddles_three_calls(P):
    fs = 64000
    toks = G.text_tokens("T")
    st = P.morse_station(1000.0, 0.5, 13, 5, toks)
    spt, rise, dot, dash, period = P.morse_station_plan(fs, st)
    assert dash > 3 * 4099
    # the second pass's dash begins at `period`: calls of 4099 from 100 samples before it
    p0 = period - 100
    assert P.morse_station_marks(fs, st, p0, 4099) == [(100, True)]
    assert P.morse_station_marks(fs, st, p0 + 4099, 4099) == [(100 - 4099, True)]
    assert P.morse_station_marks(fs, st, p0 + 2 * 4099, 4099) == [(100 - 2 * 4099, True)]
    # the sample behind its last one: nothing; its last one: still listed
    assert P.morse_station_marks(fs, st, period + dash, 1) == []
    assert P.morse_station_marks(fs, st, period + dash - 1, 1) == [(-(dash - 1), True)]
    # a call of several passes lists each pass's mark; a text without marks lists none
    assert P.morse_station_marks(fs, st, 0, 3 * period) == [(0, True), (period, True), (2 * period, True)]
    assert P.morse_station_marks(fs, P.morse_station(1000.0, 0.5, 13, 5, [0, 1]), 0, 10 ** 7) == []
