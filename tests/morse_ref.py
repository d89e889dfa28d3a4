"""Restatement of the Morse digital modem's Goertzel path (plugins/MorseDigitalModem, pebblelib), the parity reference for
pebblegpu_morse_* and pebblegpu_set_morse.  Citations are relative to the reference tree.

Decimation runs through the unchanged oracle.Decimator(rate, 1000, 8000).  Everything else is plain Python in the reference's
types: Python floats are IEEE doubles and complex multiplies are computed as (ac - bd, ad + bc) without fused operations, like
std::complex<double>; quint32 values are Python ints kept in range; the one float division (updateThresholds' ratio) is numpy float32.

Left out on purpose: Goertzel's m_avgFilter and stdDev() (goertzel.cpp:234, :684-686), read only by TH_COMPARE / TH_AVERAGE, not by
TH_PEAK; the jitter filter and attack/decay counters (GoertzelOOK::debounce is never called); syncFilterWithWpm (morse.cpp:549-564:
its Goertzel branch only resets m_agc_peak, which the Goertzel path never reads); m_usecLongestMark, m_usecSpikeThreshold and
m_usecFadeThreshold (set, never compared).
"""
import math

import numpy as np

import oracle

DM_LSB, DM_CWL, DM_CWU = 6, 8, 9
DOT_MAGIC = 1200000                          # MorseCode::c_uSecDotMagic, morsecode.h:58
WPM_LOW, WPM_HIGH, WPM_VAR = 10, 50, 2       # morse.h:82-83, :169
MAX_LEN = 8                                  # MorseCode::c_maxMorseLen, morsecode.h:51
TWOPI = 6.28318530717958647692528676656      # pebblelib/cpx.h:18
IDLE, MARK_TIMING, INTER_ELEMENT_TIMING, WORD_SPACE_TIMING = range(4)
CHAR, WORD_SPACE = 0, 1
U32 = 0xFFFFFFFF


def modem_rate(demod_rate):
    """buildDecimationChain(demodRate, 1000, 8000) truncated to int (morse.cpp:193-195)"""
    return int(oracle.Decimator(int(demod_rate), 1000, 8000).rate)


def best_n(rate):
    """findBestGoertzelN(10, 50), morse.cpp:396-446, #else branch: quint32 arithmetic"""
    mid = (WPM_LOW + WPM_HIGH) // 2
    usec_mid = DOT_MAGIC // mid                      # MorseCode::wpmToTcwUsec, morsecode.cpp:296-299
    usec_per_sample = int(1.0e6 / rate)              # quint32 usecPerSample = 1.0e6 / m_modemSampleRate
    return (usec_mid // 4) // usec_per_sample


def goertzel_coeffs(freq, n, rate):
    """Goertzel::setFreq(freq, N, sampleRate), goertzel.cpp:154-219 -> (c_B, c_C, c_D)"""
    if freq < 0:
        freq = freq + rate
    nf = float(freq) / float(rate)
    k = nf * n
    a = TWOPI * k / n
    b = 2 * math.cos(a)
    c = _exp_minus_cj(a, 1.0)                        # exp(-c_j * c_A)
    d = _exp_minus_cj(a, float(n) - 1.0)             # exp(-c_j * c_A * ((double)N - 1.0))
    return b, c, d


CJ_RE = 6.123233995736766e-17                        # pebblelib/cpx.h:158: const CPX c_j = {6.123233995736766e-17, 1}, not {0, 1}


def _exp_minus_cj(a, k):
    """std::exp((-c_j * a) * k): complex times double scales both parts, twice; exp(re) * (cos(im), sin(im)).  With c_j's real part the
    modulus is exp(-6.1e-17 a k), not 1: up to 3e-14 under it at N = 80 (found by tests/test_reference_pins.py's Goertzel cases)"""
    re, im = (-CJ_RE * a) * k, (-1.0 * a) * k
    e = math.exp(re)
    return complex(e * math.cos(im), e * math.sin(im))


def usec_delta(earlier, later, rate):
    """SampleClock::uSecDelta, sampleclock.cpp:19-25"""
    if earlier >= later:
        return 0
    return int(((later - earlier) * 1.0e6) / float(rate)) & U32


class MorseRef:
    """Morse() + setSampleRate(demod_rate, frames) (morse.cpp:160-246); process(frame) = processBlock (:761-894)."""

    def __init__(self, demod_rate, frames, wpm=20):
        self.frames = frames
        self.dec = oracle.Decimator(int(demod_rate), 1000, 8000)
        self.rate = self.modem_rate_of(self.dec.rate)
        self.n = self.best_n_of(self.rate)
        self.mode = DM_CWL                           # morse.cpp:181: dmCWL whatever the receiver's mode
        # GoertzelOOK ctor, goertzel.cpp:351-373, and Goertzel's running sums
        self.s1 = self.s2 = 0j
        self.count = 0
        self.peak = 0.0
        self.minp = 1.0                               # m_minPower = 1.0 while its filter starts at 0
        self.peak_avg = self.min_avg = 0.0
        self.last_tone = False
        self.sma = None                               # m_dotDashThresholdFilter = new MovingAvgFilter(8)
        self.sma_i = 0
        self.abs = 0                                  # modem samples since enabled (the library's event time base)
        self.events = []
        self.powers, self.tones = [], []
        self.state = self.last_state = IDLE
        self.usec_last_mark = self.usec_mark = self.usec_space = 0
        self.mark_handled = False
        self.dd = []
        self.below = self.above = False
        self.init(wpm)

    # the two roundings of setSampleRate, as methods so that tests/morse_cases.py's deliberately wrong models can get them wrong
    def modem_rate_of(self, chain_rate):
        return int(chain_rate)                        # int actualModemRate, morse.cpp:191-192

    def best_n_of(self, rate):
        return best_n(rate)

    def set_sample_rate(self, demod_rate, frames):
        """setSampleRate again (morse.cpp:160-246): a new Decimator, GoertzelOOK and threshold filter, dmCWL, init from the plugin
        object's m_wpmSpeedCurrent; the library's event time base restarts, the events decided so far stay"""
        events, margins = self.events, self.margins
        self.__init__(demod_rate, frames, wpm=self.wpm)
        self.events, self.margins = events, margins

    # ---- init, morse.cpp:566-601 ----
    def init(self, wpm):
        if wpm < 5:
            wpm = 5
        self.wpm = wpm
        self.update_thresholds(DOT_MAGIC // wpm, True)   # reads m_wpmLimitLow/High before they are set: 10 / 50 is what every setSampleRate but the first finds (pinned); at the first, a choice
        self.set_goertzel()                               # updateGoertzel(1000, findBestGoertzelN(10, 50))
        self.shortest = int(DOT_MAGIC / (WPM_HIGH * 1.10))  # setMinMaxMark, :375-381
        self.sma = None                                   # m_dotDashThresholdFilter->reset()
        self.sma_i = 0
        self.reset_clock()
        self.dd = []
        self.last_state = self.state
        self.state = IDLE

    def set_goertzel(self):
        """Morse::updateGoertzel(1000, N), morse.cpp:345-373: -1000 Hz for CWL / LSB, +1000 otherwise; sums carry on"""
        f = -1000 if self.mode in (DM_CWL, DM_LSB) else 1000
        self.B, self.C, self.D = goertzel_coeffs(f, self.n, self.rate)

    def set_demod_mode(self, mode):                       # Morse::setDemodMode, :337-341
        self.mode = mode
        self.set_goertzel()

    def reset_clock(self):                                # resetModemClock, :733-740
        self.clock = 0
        self.tone_end = 0
        self.usec_mark = 0
        self.usec_space = 0

    def sma_sample(self, x):                              # MovingAvgFilter::newSample, SimpleMovingAverage, movingavgfilter.cpp:66-130
        x = float(x)
        if self.sma is None:
            self.sma = [x] * 8
            self.sma_sum = x * 8
            self.sma_avg = x
        else:
            old = self.sma[self.sma_i]
            self.sma_sum = self.sma_sum - old + x
            self.sma_avg = self.sma_sum / 8
            self.sma[self.sma_i] = x
            self.sma_i = (self.sma_i + 1) % 8
        return self.sma_avg

    # ---- updateThresholds, morse.cpp:605-720 ----
    def update_thresholds(self, usec_new, force):
        if force:
            dot, dash = usec_new, usec_new * 3
            self.usec_last_mark = dot
        else:
            if self.usec_last_mark == 0:
                return
            ratio = float(np.float32(usec_new) / np.float32(self.usec_last_mark))
            if 2 <= ratio <= 4:
                dot, dash = self.usec_last_mark, usec_new
            elif 0.25 <= ratio <= 0.50:
                dot, dash = usec_new, self.usec_last_mark
            else:
                return
        ddt = int(self.sma_sample((dash + dot) // 2))
        dot = ddt // 2
        wpm = DOT_MAGIC // dot
        if not force and wpm < WPM_LOW:
            self.below, self.above = True, False
        elif not force and wpm > WPM_HIGH:
            self.below, self.above = False, True
        else:
            self.below = self.above = False
            if wpm > WPM_HIGH - WPM_VAR:
                wpm -= WPM_VAR
            elif wpm < WPM_LOW + WPM_VAR:
                wpm += WPM_VAR
            self.ddt = ddt
            self.element = int(dot * 0.25)
            self.wpm = wpm
            self.char_thr = dot * 2
            self.word_thr = dot * 4

    # ---- GoertzelOOK::processResult, TH_PEAK, goertzel.cpp:664-777 ----
    def th_peak(self, p):
        aw, dw = 1.0 / 20.0, 1.0 / 500.0
        w = aw if p > self.peak else dw
        self.peak_avg = p * w + self.peak_avg * (1 - w)
        self.peak = self.peak_avg
        w = aw if p < self.minp else dw
        self.min_avg = p * w + self.min_avg * (1 - w)
        self.minp = self.min_avg
        delta = self.peak - self.minp
        up = self.minp + (delta * 0.67)
        down = self.minp + (delta * 0.33)
        if p >= up:
            tone = True
        elif p <= down:
            tone = False
        else:
            tone = self.last_tone
        self.last_tone = tone
        self.margins.append(min(abs(p - up), abs(p - down)) / max(abs(p), 1e-300))
        return tone

    # ---- stateMachine, morse.cpp:938-1140 ----
    def emit(self, kind, token):
        self.events.append((self.abs, token, kind))

    def state_machine(self, tone):
        st = self.state
        if st == IDLE:
            if tone:
                self.dd = []
                self.reset_clock()
                self.last_state, self.state = IDLE, MARK_TIMING
            else:
                self.last_state = IDLE
        elif st == MARK_TIMING:
            if tone:
                self.last_state = MARK_TIMING
            else:
                self.tone_end = self.clock
                self.usec_mark = usec_delta(0, self.tone_end, self.rate)
                if self.usec_mark < self.shortest:
                    self.state = self.last_state
                    return
                self.update_thresholds(self.usec_mark, False)
                self.usec_last_mark = self.usec_mark
                self.usec_space = 0
                self.mark_handled = False
                self.last_state, self.state = MARK_TIMING, INTER_ELEMENT_TIMING
        elif st == INTER_ELEMENT_TIMING:
            if tone:
                if self.mark_handled:
                    self.reset_clock()
                    self.last_state, self.state = INTER_ELEMENT_TIMING, MARK_TIMING
            else:
                self.usec_space = usec_delta(self.tone_end, self.clock, self.rate)
                if not self.mark_handled and self.usec_space > self.element:
                    if len(self.dd) >= MAX_LEN:
                        self.last_state, self.state = self.state, IDLE
                        return
                    self.dd.append(0 if self.usec_mark <= self.ddt else 1)
                    self.mark_handled = True
                if self.usec_space < self.char_thr:
                    self.last_state = INTER_ELEMENT_TIMING
                elif self.usec_space <= self.word_thr:
                    if self.dd:
                        tok = 1
                        for b in self.dd:                      # tokenizeDotDash, morsecode.cpp:160-185
                            tok = (tok << 1) | b
                        self.emit(CHAR, tok)
                        self.dd = []
                        self.last_state, self.state = INTER_ELEMENT_TIMING, WORD_SPACE_TIMING
                    else:
                        self.last_state, self.state = INTER_ELEMENT_TIMING, IDLE
                else:
                    self.last_state, self.state = INTER_ELEMENT_TIMING, IDLE
        else:  # WORD_SPACE_TIMING
            if tone:
                self.dd = []
                self.reset_clock()
                self.last_state, self.state = WORD_SPACE_TIMING, MARK_TIMING
            else:
                self.usec_space = usec_delta(self.tone_end, self.clock, self.rate)
                if self.usec_space < self.word_thr:
                    self.last_state = WORD_SPACE_TIMING
                else:
                    self.emit(WORD_SPACE, 0)
                    self.last_state, self.state = WORD_SPACE_TIMING, IDLE

    margins = None

    def process_modem(self, y):
        """modem-rate samples: SampleClock::tick + Goertzel::processSample(CPX) (goertzel.cpp:230-266) + result handling"""
        if self.margins is None:
            self.margins = []
        n = self.n
        for x in y:
            x = complex(x)
            self.clock = (self.clock + 1) & U32
            self.abs += 1
            s0 = x + self.B * self.s1 - self.s2
            if self.count < n - 1:
                self.s2 = self.s1
                self.s1 = s0
                self.count += 1
                continue
            y0 = s0 - self.s1 * self.C
            y0 = y0 * self.D
            self.count = 0
            self.s1 = self.s2 = 0j
            y0 = complex(y0.real / n, y0.imag / n)
            p = y0.real * y0.real + y0.imag * y0.imag     # DB::power, db.h:33-35
            tone = self.th_peak(p)
            self.powers.append(p)
            self.tones.append(tone)
            self.state_machine(tone)

    def process(self, frame):
        """processBlock(CPX *in): copy, Decimator::process, then every modem sample; returns in"""
        self.process_modem(self.dec.process(np.asarray(frame, dtype=np.complex128)))
        return frame

    def status(self):
        return {"wpm": self.wpm, "above_range": int(self.above), "below_range": int(self.below),
                "modem_rate": self.rate, "samples_per_result": self.n}


# ---- test signals: keyed tones and a test-local ITU-R M.1677 letter map (not the reference's table) ----
ITU = {
    "A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---",
    "K": "-.-", "L": ".-..", "M": "--", "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-",
    "U": "..-", "V": "...-", "W": ".--", "X": "-..-", "Y": "-.--", "Z": "--..", "0": "-----", "1": ".----", "2": "..---",
    "3": "...--", "4": "....-", "5": ".....", "6": "-....", "7": "--...", "8": "---..", "9": "----.",
}


def dotdash_token(dd):
    tok = 1
    for c in dd:
        tok = (tok << 1) | (1 if c == "-" else 0)
    return tok


def morse_dotdash(token):
    """the dot-dash string of a token (what MorseCode::tokenLookup takes)"""
    token = int(token)
    n = token.bit_length() - 1
    return "".join("-" if (token >> (n - 1 - i)) & 1 else "." for i in range(n))


def text_tokens(text):
    """the event kinds / tokens a clean sending of `text` decodes to (characters, then a word space after each word)"""
    out = []
    for w in text.split():
        out += [(CHAR, dotdash_token(ITU[ch])) for ch in w] + [(WORD_SPACE, 0)]
    return out


def keying(text, wpm, rate, lead_s=0.0, tail_s=0.6):
    """on/off envelope at `rate` for `text` at `wpm` (PARIS timing: dot 1.2/wpm s, dash 3, gaps 1 / 3 / 7).  TH_PEAK starts with
    its peak at 0, so whatever comes before the first mark reads as tone until the peak has seen one: the default starts keyed."""
    tcw = 1.2 / wpm
    seq = [(False, lead_s)]
    for wi, w in enumerate(text.split()):
        if wi:
            seq.append((False, 7 * tcw))
        for ci, ch in enumerate(w):
            if ci:
                seq.append((False, 3 * tcw))
            for ei, e in enumerate(ITU[ch]):
                if ei:
                    seq.append((False, tcw))
                seq.append((True, tcw if e == "." else 3 * tcw))
    seq.append((False, tail_s))
    env = []
    t = 0.0
    for on, d in seq:
        n0, t = int(round(t * rate)), t + d
        env.append(np.full(int(round(t * rate)) - n0, 1.0 if on else 0.0))
    return np.concatenate(env)
