"""Hard keying rows for the Morse decoder: traffic that takes the branches of Morse::stateMachine, updateThresholds and GoertzelOOK's
TH_PEAK which clean PARIS keying at one speed (tests/morse_cases.py, tests/test_morse_gpu.py) never takes.

Shared by the CPU tier (tests/test_morse_hard_host.py: branch coverage, measured; tests/test_reference_pins.py through
tests/reference_cases.py: the reference's own compiled decoder against the restatement) and the GPU tier (tests/test_morse_hard_gpu.py).

A row is a list of (on, seconds, amplitude) segments, a noise seed and a list of actions (seconds, what) that fall on the first frame
boundary at or after their time: "cwu" / "cwl" = setDemodMode, "rate" = setSampleRate again.  The tone is at -1000 Hz (dmCWL, the mode
on enable and behind every setSampleRate) and moves with the mode, from the same sample on.  It has to: a keyed tone left on the other
side while the decoder listens to noise alone is rejected by 64-bit sums entirely and by the device's 32-bit chain to about -108 dB of
the tone, which is 4e-5 of such a noise-only result (measured on the device, at 64 000 / 2048 and at 12 000 / 16) -- a figure about the
rejection of a tone 2 kHz away, not about the results the decoder decides on.  Every row starts keyed: TH_PEAK's peak starts at 0, so whatever comes before the first
mark reads as tone.

CONDITION OF EVERY ROW, as in tests/morse_cases.py: min(ref.margins) > MARGIN = 1e-4 at every geometry the row is run at -- the spike
results included.  Where a row misses it another seed is chosen; the figure stays.

ARMS.  CountingRef is MorseRef with every branch arm of update_thresholds, th_peak and state_machine counted.  The arms are named from
the decoder's state before the call and told apart by the same comparisons the restated code makes; each count is tied to what the
call then did (the assertions in CountingRef).  UNREACHABLE lists the arms no input can reach, each with its argument.
"""
import functools

import numpy as np

from tests import morse_cases as MC
from tests import morse_ref as M
from tests.signals import lcg_noise

AMP, NOISE = 0.05, 2e-3
MARGIN = MC.MARGIN
RATE, FRAME = 64000, 2048          # the bench's demodulator rate: the merged 11-tap stage
SLOW_RATE = 12000                  # one stage; with morse_cases.min_frame most calls complete no Goertzel block


# ---- keying from segments ----
def envelope(segs, rate):
    """(on, seconds, amplitude) segments -> amplitude per sample at `rate`; boundaries at round(t * rate) like morse_ref.keying"""
    env, t = [], 0.0
    for on, d, a in segs:
        n0, t = int(round(t * rate)), t + d
        env.append(np.full(int(round(t * rate)) - n0, a if on else 0.0))
    return np.concatenate(env)


def code(dotdash, wpm, amp=AMP, gap_wpm=None, tail=7.0):
    """segments of space-separated dot-dash groups ("/" = word gap) at PARIS timing; gaps at gap_wpm (Farnsworth) where given;
    `tail` Tcw of silence behind the last mark"""
    tcw = 1.2 / wpm
    gt = 1.2 / (gap_wpm or wpm)
    segs = []
    for wi, word in enumerate(dotdash.split("/")):
        if wi:
            segs.append((False, 7 * gt, 0.0))
        for ci, ch in enumerate(word.split()):
            if ci:
                segs.append((False, 3 * gt, 0.0))
            for ei, e in enumerate(ch):
                if ei:
                    segs.append((False, tcw, 0.0))
                segs.append((True, tcw if e == "." else 3 * tcw, amp))
    segs.append((False, tail * gt, 0.0))
    return segs


def text(t, wpm, **kw):
    return code("/".join(" ".join(M.ITU[c] for c in w) for w in t.split()), wpm, **kw)


def marks(ms, gap_ms, amp=AMP, tail_ms=400.0):
    """marks of the given lengths (milliseconds) with one gap between them"""
    segs = []
    for i, m in enumerate(ms):
        if i:
            segs.append((False, gap_ms / 1e3, 0.0))
        segs.append((True, m / 1e3, amp))
    segs.append((False, tail_ms / 1e3, 0.0))
    return segs


def on(ms, amp=AMP):
    return [(True, ms / 1e3, amp)]


def off(ms):
    return [(False, ms / 1e3, 0.0)]


def _fade(segs, db):
    """the amplitudes run down by `db` dB, linearly in dB over the marks"""
    k = [i for i, s in enumerate(segs) if s[0]]
    out = list(segs)
    for j, i in enumerate(k):
        o, d, a = segs[i]
        out[i] = (o, d, a * 10 ** (-db * j / (len(k) - 1.0) / 20.0))
    return out


class Row:
    """tail: the text the row's last events decode to at both geometries (morse_cases.check_against's tail), None where to none"""

    def __init__(self, name, segs, seed, actions=(), tail=None, why=""):
        self.name, self.segs, self.seed, self.actions, self.tail, self.why = name, segs, seed, list(actions), tail, why


T25 = 48.0  # ms per Tcw at 25 WPM: 4.8 Goertzel results


def _rows():
    R = []
    # spikes of one and of two Goertzel results (10 ms each at every rate here): from IDLE (behind a word space), inside a character
    # (between two elements, the space already past the element threshold) and in the word-space timing behind a character
    R.append(Row("spike1", text("TE", 25, tail=12) + on(9) + off(300) + text("N", 25, tail=3) + on(9) + off(400)
                 + code(".", 25, tail=1) + on(9) + off(T25) + code("-", 25, tail=9), 3, tail="A",
                 why="one-result spikes: IDLE -> MARK -> IDLE; WORD -> MARK -> WORD; INTER -> MARK -> INTER"))
    R.append(Row("spike2", text("TE", 25, tail=12) + on(19) + off(300) + text("N", 25, tail=3) + on(19) + off(400)
                 + code(".", 25, tail=1) + on(19) + off(T25) + code("-", 25, tail=9), 3,
                 why="two-result spikes: the second tone result sets last_state = MARK_TIMING, so the rejected mark goes on being timed"))
    # a dash split by a drop-out of one to two results, shorter than the element threshold (12 ms at 25 WPM needs two no-tone results)
    R.append(Row("dropout", text("E", 25, tail=3) + on(60) + off(14) + on(70) + off(3 * T25) + text("TE", 25), 3, tail="TE",
                 why="the tone comes back before the element threshold: mark_handled is still false"))
    R.append(Row("pending_long", text("E", 25, tail=3) + on(60) + off(14) + on(400) + off(500) + text("TE", 25), 3, tail="TE",
                 why="the same drop-out, the tone then back for 400 ms: ignored while the mark is pending, with the clock running, so the "
                     "next no-tone result finds a space past the word threshold at once: IDLE, the element appended, no event"))
    R.append(Row("nine_dots", code(". ......... .", 25), 3, tail="E", why="the ninth element finds the buffer full: IDLE"))
    R.append(Row("nonchar6", code("- ....-. .-", 25), 3, tail="A", why="a six-element token that is no character: the reference prints '*'"))
    R.append(Row("wpm8", code(".- .- .- .-", 8), 3, why="below the range: '?? est'"))
    R.append(Row("wpm60", code(".- .- .- .- .- .- .- .-/.- -.", 60), 3, why="dots of two results are rejected as short marks"))
    R.append(Row("fast_2to1", marks([30, 60] * 9, 30), 3, why="marks of 30 and 60 ms: above the range: '?? est'"))
    R.append(Row("wpm11", code(".- .- .- .-", 11), 3, tail="AAAA", why="the estimate comes to rest at 10 or 11: pulled up by WPM_VAR"))
    R.append(Row("wpm49", code(".- .- .- .- .- .-/.- -. .", 49), 3,
                 why="dots of 24.5 ms measure two results and are rejected, or three; the estimate ends above the range"))
    R.append(Row("pull_down", marks([32, 62, 32, 72] * 6, 28), 3,
                 why="marks that measure 30, 60, 30, 70 ms: the filtered estimate comes to rest at 49 or 50 and is pulled down by WPM_VAR"))
    R.append(Row("ratio_out", marks([48, 144, 216, 36, 216, 48, 144], 96), 3,
                 why="a mark 1.5 times the mark before (216 after 144), one a sixth of it (36) and one 6 times it (216): neither dot/dash "
                     "nor dash/dot"))
    R.append(Row("speed_15_35_15", text("AN", 15, tail=4) + text("ANTENNA", 35, tail=5) + text("AN", 15), 3,
                 why="15 -> 35 -> 15 WPM through the 8-deep threshold filter"))
    R.append(Row("farnsworth", text("TEN AT", 25, gap_wpm=10), 3, why="characters at 25 WPM, gaps at 10 WPM"))
    R.append(Row("fade12", _fade(text("TENNET", 25), 12.0), 3, why="12 dB down across a word: TH_PEAK's slow decay decides"))
    R.append(Row("mode_rate_midchar", text("TE", 25, tail=3) + code("-.-.", 25, tail=3) + text("ET", 25, tail=3) + code("--.-", 25, tail=3)
                 + text("TEN", 25), 3, actions=[(0.95, "cwu"), (1.95, "rate")], tail="N",
                 why="setDemodMode in the middle of a character (the Goertzel sums carry on under new coefficients), setSampleRate again in "
                     "the middle of another (a fresh decoder, dmCWL, from the current estimate)"))
    return R


ROWS = _rows()
NAMES = [r.name for r in ROWS]
BANK_ROWS = ("spike2", "speed_15_35_15", "nine_dots")


def row(name):
    return next(r for r in ROWS if r.name == name)


ACT = {"rate": 0, "cwl": M.DM_CWL, "cwu": M.DM_CWU, "status": -1}   # the numbers of oracle/ref_build/ref_driver.cpp's stage morse

# the tokens of valid length the rows decode to that are no character of the reference's table: it prints '*' for them, the library
# hands out the token.  Written here from reading that table; the reference binary is held to them (the "stars" record of a case)
NONCHAR = ("....-.", "......-.", ".--.-.-", "......")


@functools.lru_cache(maxsize=None)
def plan(name, rate, frame):
    """-> (n, plan): the row's length at `rate`, a whole number of frames, and what happens before which frame: [(sample, what)] in
    order, the row's actions on the first frame boundary at or after their time and a "status" (a reading, nothing else) at a quarter,
    a half and three quarters of the stream"""
    r = row(name)
    n = -(-len(envelope(r.segs, rate)) // frame) * frame
    p = [(-(-int(at * rate) // frame) * frame, what) for at, what in r.actions]
    p += [(((n // frame) * q // 4) * frame, "status") for q in (1, 2, 3)]
    return n, sorted(p, key=lambda v: v[0])


@functools.lru_cache(maxsize=4)
def stream(name, rate, frame):
    """-> (x, plan): the row's input at `rate` and its plan"""
    r = row(name)
    n, p = plan(name, rate, frame)
    env = envelope(r.segs, rate)
    env = np.concatenate([env, np.zeros(n - len(env))])
    t = np.arange(n) / float(rate)
    f = np.full(n, -1000.0)
    for at, what in p:          # the tone follows the mode, as a receiver's does: +1000 Hz in dmCWU, -1000 Hz in dmCWL (setSampleRate's mode)
        if what != "status":
            f[at:] = 1000.0 if what == "cwu" else -1000.0
    x = env * np.exp(2j * np.pi * f * t) + lcg_noise(n, r.seed, NOISE)
    x.setflags(write=False)
    return x, p


def driver_args(rate, frame, plan):
    return [rate, frame, 20, 0] + [v for at, what in plan for v in (at, ACT[what])]


def status10(ref):
    """the ten values of the driver's status record"""
    return [ref.wpm, int(ref.above), int(ref.below), ref.rate, ref.n, ref.ddt, ref.element, ref.char_thr, ref.word_thr, ref.shortest]


def feed(ref, x, plan, frame):
    """the stream through a restatement frame by frame; -> its readings: (status, status10) before every "status" and "rate" of the
    plan, in order, and at the end"""
    seen = []
    for k in range(len(x) // frame):
        for at, what in plan:
            if at != k * frame:
                continue
            if what in ("status", "rate"):
                seen.append((ref.status(), status10(ref)))
            if what == "rate":
                ref.set_sample_rate(ref.demod_rate, frame)
            elif what != "status":
                ref.set_demod_mode(ACT[what])
        ref.process(x[k * frame:(k + 1) * frame])
    seen.append((ref.status(), status10(ref)))
    return seen


# ---- the arms ----
UT = ("ut.force", "ut.last_mark_zero", "ut.ratio_dash", "ut.ratio_dot", "ut.ratio_between", "ut.ratio_outside",
      "ut.below_range", "ut.above_range", "ut.pull_down", "ut.pull_up", "ut.no_pull")
TP = ("tp.peak_attack", "tp.peak_decay", "tp.min_attack", "tp.min_decay", "tp.up", "tp.down", "tp.hold_tone", "tp.hold_no_tone")
SM = ("sm.idle.tone", "sm.idle.no_tone", "sm.mark.tone", "sm.mark.short_to_idle", "sm.mark.short_to_mark", "sm.mark.short_to_inter",
      "sm.mark.short_to_word", "sm.mark.end", "sm.inter.tone_handled", "sm.inter.tone_pending", "sm.inter.buffer_full", "sm.inter.dot",
      "sm.inter.dash", "sm.inter.no_element", "sm.inter.keep", "sm.inter.char", "sm.inter.char_empty", "sm.inter.past_word",
      "sm.word.tone", "sm.word.keep", "sm.word.space")
ARMS = UT + TP + SM

# The arms no input reaches, each with its argument; tests/test_morse_hard_host.py checks the inequalities.  sm.inter.past_word is NOT
# one of them: usec_space does not grow by one result a call while a tone is ignored with the mark pending (row pending_long).
UNREACHABLE = {
    "ut.last_mark_zero":
        "update_thresholds(.., False) runs only behind init's forced update, which sets usec_last_mark = DOT_MAGIC // wpm with wpm the "
        "constructor's 20 or an estimate the range arms keep at WPM_HIGH or under: >= DOT_MAGIC // WPM_HIGH = 24000 > 0.  Every later "
        "assignment is usec_last_mark = usec_mark behind the test usec_mark >= shortest = int(DOT_MAGIC / (WPM_HIGH * 1.10)) = 21818 > 0 "
        "(a pending tone only lengthens a space; no path assigns a mark that the test has not passed)",
    "sm.inter.char_empty":
        "INTER_ELEMENT_TIMING is entered behind an accepted mark (mark_handled = False) or back from a rejected one (the buffer then "
        "holds the element that set mark_handled).  With mark_handled False the element is appended as soon as usec_space > element = "
        "int(0.25 dot), and the character arm needs usec_space >= char_thr = 2 dot > int(0.25 dot) for every dot >= 1; a full buffer "
        "returns before the arm.  A tone that comes back while the mark is pending is ignored with the clock running, so the next "
        "no-tone result may find usec_space far past `element` at once: that jump appends the element in the same call, before the "
        "test.  So the buffer is never empty there",
}


class CountingRef(M.MorseRef):
    def __init__(self, demod_rate, frames, wpm=20, arms=None):
        self.arms = arms if arms is not None else dict.fromkeys(ARMS, 0)
        self.demod_rate = demod_rate
        super().__init__(demod_rate, frames, wpm)

    def set_sample_rate(self, demod_rate, frames):
        """as MorseRef's; the per-result record goes on as well (a reader of the device's read-out collects it across the call)"""
        events, margins, arms, powers, tones = self.events, self.margins, self.arms, self.powers, self.tones
        self.__init__(demod_rate, frames, wpm=self.wpm, arms=arms)
        self.events, self.margins, self.powers, self.tones = events, margins, powers, tones

    def hit(self, arm):
        self.arms[arm] += 1

    def update_thresholds(self, usec_new, force):
        before = (self.wpm if hasattr(self, "wpm") else None, getattr(self, "ddt", None), self.below, self.above, self.sma_i, self.sma is None)
        if force:
            self.hit("ut.force")
            updates = True
        elif self.usec_last_mark == 0:
            self.hit("ut.last_mark_zero")
            updates = False
        else:
            ratio = float(np.float32(usec_new) / np.float32(self.usec_last_mark))
            arm = ("ut.ratio_dash" if 2 <= ratio <= 4 else "ut.ratio_dot" if 0.25 <= ratio <= 0.50 else
                   "ut.ratio_between" if 0.5 < ratio < 2.0 else "ut.ratio_outside")
            self.hit(arm)
            updates = arm in ("ut.ratio_dash", "ut.ratio_dot")
        first = self.sma is None
        super().update_thresholds(usec_new, force)
        if not updates:   # the call returned before the filter: nothing moved
            assert before == (self.wpm, getattr(self, "ddt", None), self.below, self.above, self.sma_i, self.sma is None)
            return
        assert first or self.sma_i == (before[4] + 1) % 8
        wpm = M.DOT_MAGIC // (int(self.sma_avg) // 2)
        if self.below:
            assert not force and wpm < M.WPM_LOW
            self.hit("ut.below_range")
        elif self.above:
            assert not force and wpm > M.WPM_HIGH
            self.hit("ut.above_range")
        else:
            arm = "ut.pull_down" if wpm > M.WPM_HIGH - M.WPM_VAR else "ut.pull_up" if wpm < M.WPM_LOW + M.WPM_VAR else "ut.no_pull"
            assert self.wpm == wpm + {"ut.pull_down": -M.WPM_VAR, "ut.pull_up": M.WPM_VAR, "ut.no_pull": 0}[arm]
            self.hit(arm)

    def th_peak(self, p):
        self.hit("tp.peak_attack" if p > self.peak else "tp.peak_decay")
        self.hit("tp.min_attack" if p < self.minp else "tp.min_decay")
        last = self.last_tone
        tone = super().th_peak(p)
        delta = self.peak - self.minp
        if p >= self.minp + (delta * 0.67):
            assert tone
            self.hit("tp.up")
        elif p <= self.minp + (delta * 0.33):
            assert not tone
            self.hit("tp.down")
        else:
            assert tone == last
            self.hit("tp.hold_tone" if last else "tp.hold_no_tone")
        return tone

    def state_machine(self, tone):
        st, last, handled, ndd, nev = self.state, self.last_state, self.mark_handled, len(self.dd), len(self.events)
        super().state_machine(tone)
        now = self.state
        if st == M.IDLE:
            assert now == (M.MARK_TIMING if tone else M.IDLE)
            self.hit("sm.idle.tone" if tone else "sm.idle.no_tone")
        elif st == M.MARK_TIMING:
            if tone:
                assert now == M.MARK_TIMING
                self.hit("sm.mark.tone")
            elif self.usec_mark < self.shortest:
                assert now == last
                self.hit("sm.mark.short_to_" + ("idle", "mark", "inter", "word")[last])
            else:
                assert now == M.INTER_ELEMENT_TIMING and not self.mark_handled
                self.hit("sm.mark.end")
        elif st == M.INTER_ELEMENT_TIMING:
            if tone:
                assert now == (M.MARK_TIMING if handled else M.INTER_ELEMENT_TIMING)
                self.hit("sm.inter.tone_handled" if handled else "sm.inter.tone_pending")
                return
            if (not handled) and self.usec_space > self.element:
                if ndd >= M.MAX_LEN:
                    assert now == M.IDLE and len(self.dd) == ndd
                    self.hit("sm.inter.buffer_full")
                    return
                assert self.mark_handled
                self.hit("sm.inter.dot" if self.usec_mark <= self.ddt else "sm.inter.dash")
                ndd += 1
            else:
                self.hit("sm.inter.no_element")
            if self.usec_space < self.char_thr:
                assert now == M.INTER_ELEMENT_TIMING and len(self.events) == nev
                self.hit("sm.inter.keep")
            elif self.usec_space <= self.word_thr:
                if ndd:
                    assert now == M.WORD_SPACE_TIMING and len(self.events) == nev + 1 and self.events[-1][2] == M.CHAR
                    self.hit("sm.inter.char")
                else:
                    assert now == M.IDLE
                    self.hit("sm.inter.char_empty")
            else:
                assert now == M.IDLE and len(self.events) == nev
                self.hit("sm.inter.past_word")
        else:
            if tone:
                assert now == M.MARK_TIMING
                self.hit("sm.word.tone")
            elif self.usec_space < self.word_thr:
                assert now == M.WORD_SPACE_TIMING
                self.hit("sm.word.keep")
            else:
                assert now == M.IDLE and self.events[-1][2] == M.WORD_SPACE
                self.hit("sm.word.space")


@functools.lru_cache(maxsize=None)
def reference(name, rate=RATE, frame=FRAME):
    """the counting restatement's run of a row, computed once and shared; nothing may change it.  ref.seen: feed's readings"""
    x, plan = stream(name, rate, frame)
    ref = CountingRef(rate, frame)
    ref.seen = feed(ref, x, plan, frame)
    ref.dec = None
    return ref


def stars_of(name, events):
    """the numbers of the events for which the reference prints '*'"""
    return [i for i, (_, t, k) in enumerate(events) if k == M.CHAR and M.morse_dotdash(t) in NONCHAR]


def arms_of(refs):
    total = dict.fromkeys(ARMS, 0)
    for r in refs:
        for k, v in r.arms.items():
            total[k] += v
    return total


def old_rows_arms():
    """the arms the rows from before this module take: the morse_cases stream at 64000 / 2048 and test_morse_gpu's step streams (TEST /
    MORSE at 15, 25 and 40 WPM with the mode change), run through CountingRef"""
    refs = []
    for wpm in (15, 25, 40):
        x, n1 = MC.stream(RATE, FRAME, wpm)
        ref = CountingRef(RATE, FRAME)
        MC.feed(ref, x, n1, FRAME)
        refs.append(ref)
    return arms_of(refs)
