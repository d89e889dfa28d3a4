"""Serial restatement of the reference's Morse sender, MorseGen (plugins/MorseGenDevice/morsegen.cpp), in plain Python doubles.

setParams builds the dot and dash buffers sample by sample in the reference's statement order -- the serial phase sum acc += phase and
the serial ramps amplitude += ampInc / amplitude -= ampInc -- with its quint32 truncations; genToken / genDot / genDash / genElement /
genChar / genWord assemble a token's samples from those buffers; nextOutputSample hands them out one by one and starts the text over.
Written from reading the reference, with none of its text.  Tokens, not characters: MorseCode::asciiLookup stays with the caller
(tests/morse_ref.py: dotdash_token(ITU[ch]); 0 stands for ' ').

The pure copying (a buffer into the token's buffer, the token's buffer into the output) is done with numpy slices: the values are the
serial ones."""
import math

import numpy as np

from tests.morse_ref import ITU, dotdash_token

TWOPI = 6.28318530717958647692528676656      # pebblelib/cpx.h:18
TCW_DOT, TCW_DASH, TCW_CHAR, TCW_ELEMENT, TCW_WORD = 1, 3, 3, 1, 7   # MorseCode::c_tcw*, morsecode.h:65-69
DOT, DASH, EL_SPACE, CH_SPACE, WORD_SPACE = range(5)
U32 = 0xFFFFFFFF


def db_to_amplitude(db):
    """DB::dBToAmplitude: 10^(dB/20)"""
    return 10.0 ** (db / 20.0)


def text_tokens(text):
    """the tokens MorseGen::genText looks up character by character (morsegen.cpp:224-234); ' ' -> 0"""
    return [0 if ch == " " else dotdash_token(ITU[ch]) for ch in text]


class MorseGenRef:
    def __init__(self, sample_rate):
        self.fs = float(sample_rate)                                   # morsegen.cpp:8
        self.tokens = []

    def set_params(self, frequency, amplitude, wpm, ms_rise):
        """MorseGen::setParams, morsegen.cpp:33-160; amplitude is m_amplitude (linear, :40)"""
        fs = self.fs
        self.frequency, self.amplitude = float(frequency), float(amplitude)   # :38-40
        ms_tcw = 1200 // wpm                                           # :45, MorseCode::wpmToTcwMs (c_mSecDotMagic / wpm, quint32)
        spt = int(ms_tcw / (1000.0 / fs)) & U32                        # :47
        self.rise = int(ms_rise / (1000 / fs)) & U32                   # :55
        self.fall = int(ms_rise / (1000 / fs)) & U32                   # :56
        tcw_rise_fall = (self.rise + self.fall) // 2                   # :58
        self.n_dot = (spt * TCW_DOT - tcw_rise_fall) & U32             # :59 (unsigned: wraps below 0)
        self.n_dot_buf = self.rise + self.fall + self.n_dot            # :61
        self.n_dash = (spt * TCW_DASH - tcw_rise_fall) & U32           # :66
        self.n_dash_buf = self.rise + self.fall + self.n_dash          # :67
        self.n_element = spt * TCW_ELEMENT                             # :72
        self.n_char = spt * TCW_CHAR                                   # :77
        self.n_word = spt * TCW_WORD - 3                               # :84
        self.spt = spt
        phase = TWOPI * self.frequency / fs                            # :90
        self.dot_buf = self._mark(phase, self.rise, self.n_dot)        # :93-117
        self.dash_buf = self._mark(phase, self.fall, self.n_dash)      # :119-142 (ampInc from m_numSamplesFall, :120)
        self.last_symbol = WORD_SPACE                                  # :157

    def _mark(self, phase, n_ramp, n_steady):
        out = np.zeros(self.rise + n_steady + self.fall, dtype=np.complex128)
        acc = 0.0                                                      # :91 / :119
        amp_inc = self.amplitude / n_ramp if n_ramp else math.inf      # :95 / :120 (a double division: by 0 gives inf, never used)
        amplitude = amp_inc                                            # :96
        k = 0
        for _ in range(self.rise):                                     # :98-103
            out[k] = complex(math.cos(acc) * amplitude, math.sin(acc) * amplitude)
            amplitude += amp_inc
            acc += phase
            k += 1
        for _ in range(n_steady):                                      # :105-109
            out[k] = complex(math.cos(acc) * self.amplitude, math.sin(acc) * self.amplitude)
            acc += phase
            k += 1
        amplitude = self.amplitude - amp_inc                           # :111
        for _ in range(self.fall):                                     # :112-117
            out[k] = complex(math.cos(acc) * amplitude, math.sin(acc) * amplitude)
            amplitude -= amp_inc
            acc += phase
            k += 1
        return out

    def set_text_out(self, tokens):
        """MorseGen::setTextOut, morsegen.cpp:163-180, with the text as tokens"""
        self.tokens = [int(t) for t in tokens]
        self.out = np.zeros(0, dtype=np.complex128)                    # m_outSampleBuf, m_numSamplesOutBuf = 0 (:176-177)
        self.out_key = np.zeros(0, dtype=bool)
        self.out_index = 0
        self.text_index = 0                                            # :178
        self.n_out = 0                                                 # samples handed out since setTextOut
        self.mark_starts = []                                          # (sample number since setTextOut, is_dash) of every mark generated

    # ---- genToken and what it calls: each returns (samples, keyed) and appends to self.mark_starts relative to `at` ----
    def _gen_mark(self, parts, dash, at):
        if self.last_symbol in (DOT, DASH):                            # :272-275 / :287-290
            parts.append((np.zeros(self.n_element, dtype=np.complex128), False))   # genElement, :299-307
            self.last_symbol = EL_SPACE
            at += self.n_element
        buf = self.dash_buf if dash else self.dot_buf                  # :276-279 / :291-294
        parts.append((buf, True))
        self.mark_starts.append((at, bool(dash)))
        self.last_symbol = DASH if dash else DOT                       # :280 / :295
        return at + len(buf)

    def _gen_token(self, token, at):
        """genToken, morsegen.cpp:236-267; genWord (:319-328) for token 0 (genText :226-228)"""
        parts = []
        if token == 0:
            parts.append((np.zeros(self.n_word, dtype=np.complex128), False))
            self.last_symbol = WORD_SPACE
        else:
            has_high_bit = False
            for _ in range(9):                                         # :244
                bit = token & 0x100                                    # :245
                if not has_high_bit:                                   # :246-254
                    has_high_bit = bit > 0
                    token = (token << 1) & 0xFFFF
                    continue
                at = self._gen_mark(parts, bit != 0, at)               # :256-260
                token = (token << 1) & 0xFFFF                          # :261
            parts.append((np.zeros(self.n_char, dtype=np.complex128), False))   # genChar, :263, :309-317
            self.last_symbol = CH_SPACE
        x = np.concatenate([p for p, _ in parts])
        key = np.concatenate([np.full(len(p), k, dtype=bool) for p, k in parts])
        return x, key

    def generate(self, n):
        """n calls of nextOutputSample (morsegen.cpp:191-222) -> (samples [n], keyed [n]: inside a dot's or a dash's buffer)"""
        x = np.zeros(n, dtype=np.complex128)
        key = np.zeros(n, dtype=bool)
        if not self.tokens:                                            # :193-194
            return x, key
        k = 0
        while k < n:
            if self.out_index >= len(self.out):                        # :200
                if self.text_index >= len(self.tokens):                # :204-207
                    self.text_index = 0
                tok = self.tokens[self.text_index]                     # :208
                self.text_index += 1
                self.out, self.out_key = self._gen_token(tok, self.n_out + (k))   # :209
                self.out_index = 0                                     # :217
            m = min(n - k, len(self.out) - self.out_index)
            x[k:k + m] = self.out[self.out_index:self.out_index + m]   # :219-221
            key[k:k + m] = self.out_key[self.out_index:self.out_index + m]
            self.out_index += m
            k += m
        self.n_out += n
        return x, key

    def lengths(self):
        """(samplesPerTcw, rise, dot buffer, dash buffer, samples of one pass through the text)"""
        period = 0
        for tok in self.tokens:
            if tok == 0:
                period += self.n_word
                continue
            marks = [(tok >> b) & 1 for b in range(tok.bit_length() - 2, -1, -1)]
            period += sum(self.n_dash_buf if d else self.n_dot_buf for d in marks) + max(0, len(marks) - 1) * self.n_element + self.n_char
        return self.spt, self.rise, self.n_dot_buf, self.n_dash_buf, period


def station_sum(fs, stations, n):
    """the sum of MorseGen stations over n samples, as MorseGenDevice::generate adds them (morsegendevice.cpp:1060), fade off.
    stations: [(frequency, amplitude, wpm, ms_rise, tokens)] -> (samples [n], keyed [n]: some station is inside a mark)"""
    x = np.zeros(n, dtype=np.complex128)
    key = np.zeros(n, dtype=bool)
    for f, a, wpm, rise, toks in stations:
        g = MorseGenRef(fs)
        g.set_params(f, a, wpm, rise)
        g.set_text_out(toks)
        y, k = g.generate(n)
        x += y
        key |= k
    return x, key
