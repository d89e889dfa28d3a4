"""The table of tests/test_morse_geometry_host.py (CPU tier) and tests/test_morse_geometry_gpu.py (GPU tier): the Morse modem
(csrc/kernels_modem.h, csrc/morse.hip) at every form of design::build_chain(rate, 1000, 8000) and every call geometry of a chain.

A row is (demodulator rate, frame).  Chain, total decimation, modem rate and N come from oracle.Decimator(rate, 1000, 8000) and
morse_ref.best_n; the CPU tier pins them to literals.  The rates: no stage (8000), one stage (12000), two with a fractional modem
rate truncated to int (31250 -> 7812), three (37500 -> 4687), the merged 11-tap stage at strides 4, 4, 8 and 16 (48000, 64000, 96000,
256000).  The four frames of a rate:

  min          the smallest multiple of the total decimation at which every stage gets at least its tap count (MorseCore::check's
               limit; at 8000, where that is 1, a frame of 8): 8 or 10 modem samples a call, so most calls complete no Goertzel block
               (k_morse_decide sees nres = 0 and only moves the clock), nearly every tap of every stage comes from the carried tails,
               and the stream has well over 1024 calls, so MorseCore::run drains the event log mid-stream
  N * total    every call ends exactly on a block boundary (the zero-length trailing block)
  (N+1) * total  the block phase moves one sample per call through all N positions
  67 * N * total  67 results a call: lanes 0..2 of k_morse_goertzel run a second block

The input is test_morse_gpu.py's: "TEST" keyed at -1000 Hz (CWL, the mode on enable), then CWU and "MORSE" at +1000 Hz from the first
frame boundary after 2.2 s, amplitude 0.05, lcg_noise 2e-3 with seed 11 + wpm, 25 WPM.

CONDITION OF EVERY ROW: min(ref.margins) > MARGIN = 1e-4, the distance of every restated decision from its thresholds relative to the
power.  It makes "decisions identical" meaningful at a power bar of 1e-5; it is no tolerance.  If a change of text or seed breaks it,
another seed is chosen, the figure stays.

The comparison (check_against) is test_morse_gpu.test_step_against_the_restatement's: result counts equal, decisions identical, powers
within 1e-5 relative on results above -100 dB, events identical with the tail decoding to "MORSE", status equal.

WRONG MODELS (WrongRef): the restatement with one defect of the kind the device's call-by-call design could have.  The CPU tier shows
that each fails check_against on a named row; see its docstring for which.
"""
import functools

import numpy as np

import oracle
from tests import morse_ref as M
from tests.signals import lcg_noise
from tests.test_morse_gpu import keyed  # (plain numpy: amp * keying envelope * tone, placed at a sample of the stream)

RATES = [8000, 12000, 31250, 37500, 48000, 64000, 96000, 256000]
WPM = 25
AMP, NOISE = 0.05, 2e-3
MARGIN = 1e-4
POWER_BAR = 1e-5
TEXT1, TEXT2 = "TEST", "MORSE"

# refusals: (demodulator rate, frame, code name)
REFUSALS = [(390625, 2048, "E_UNSUPPORTED"),   # the first stage is the CIC (ntaps = 0)
            (50, 8, "E_UNSUPPORTED"),          # N = 0
            (64000, 60, "E_SIZE"),             # no multiple of the decimation by 8
            (64000, 56, "E_SIZE")]             # the second stage would get 14 < 15 samples
CODES = {"E_SIZE": -5, "E_UNSUPPORTED": -6}    # include/pebblegpu.h


@functools.lru_cache(maxsize=None)
def geometry(rate):
    """-> (chain [(taps, stride)], total decimation, modem rate, N)"""
    d = oracle.Decimator(int(rate), 1000, 8000)
    chain = [tuple(c) for c in d.chain()]
    mr = M.modem_rate(rate)
    return chain, d.total_decimation, mr, M.best_n(mr)


def min_frame(rate):
    """the smallest multiple of the total decimation that MorseCore::check accepts; 8 where that is 1"""
    chain, total, _, _ = geometry(rate)
    if not chain:
        return 8
    n = total
    while True:
        ln, ok = n, True
        for t, s in chain:
            ok = ok and ln >= t
            ln //= s
        if ok:
            return n
        n += total


def frames(rate):
    _, total, _, n = geometry(rate)
    return [min_frame(rate), n * total, (n + 1) * total, 67 * n * total]


ROWS = None


def rows():
    global ROWS
    if ROWS is None:
        ROWS = [(r, f) for r in RATES for f in frames(r)]
    return ROWS


def row_id(row):
    return "%d-%d" % row


def per_call(rate, frame):
    """-> (modem samples a call, N)"""
    _, total, _, n = geometry(rate)
    return frame // total, n


# ---- the stream ----
@functools.lru_cache(maxsize=2)
def stream(rate, frame, wpm=WPM):
    """-> (x, n1): the whole input and the sample at which the mode becomes CWU, both whole numbers of frames"""
    fs = rate
    n1 = -(-int(2.2 * fs) // frame) * frame
    n = n1 + -(-int(4.6 * fs) // frame) * frame
    x = keyed(TEXT1, wpm, fs, n, -1000.0, AMP) + keyed(TEXT2, wpm, fs, n, 1000.0, AMP, start=n1) + lcg_noise(n, 11 + wpm, NOISE)
    x.setflags(write=False)
    return x, n1


def feed(ref, x, n1, frame):
    """the stream through a restatement (or a wrong model) frame by frame, the mode change at n1"""
    for k in range(len(x) // frame):
        if k * frame == n1:
            ref.set_demod_mode(M.DM_CWU)
        ref.process(x[k * frame:(k + 1) * frame])
    return ref


@functools.lru_cache(maxsize=None)
def reference(rate, frame, wpm=WPM):
    """the restatement's run of a row, computed once and shared; nothing may change it"""
    x, n1 = stream(rate, frame, wpm)
    ref = feed(M.MorseRef(rate, frame), x, n1, frame)
    ref.dec = None
    return ref


# ---- the comparison of the GPU tier ----
def worst_power(powers, ref):
    """-> (worst relative error over the results above -100 dB, its result index)"""
    rp = np.array(ref.powers)
    p = np.asarray(powers, dtype=np.float64)
    m = 10 * np.log10(np.maximum(rp, 1e-300)) > -100
    err = np.where(m, np.abs(p - rp) / np.where(m, rp, 1.0), 0.0)
    i = int(np.argmax(err))
    return float(err[i]), i


def check_against(ref, powers, tones, events, status, label="", tail=TEXT2):
    """test_step_against_the_restatement's bars.  powers / tones per result, events as (sample, token, kind), status a dict.  tail: the
    text the last events decode to (this module's stream ends with TEXT2; a row of tests/morse_hard_cases.py passes the text its
    last events decode to, or None where they decode to none; its events are held to the reference's recorded ones as well)"""
    assert len(powers) == len(ref.powers) > 0, (label, len(powers), len(ref.powers))
    assert min(ref.margins) > MARGIN, (label, min(ref.margins))
    worst, at = worst_power(powers, ref)
    if label:
        print("%s: %d results, worst power error %.3e at result %d, smallest margin %.3e" % (label, len(powers), worst, at, min(ref.margins)))
    assert [bool(t) for t in tones] == ref.tones, label
    assert worst <= POWER_BAR, (label, worst, at)
    assert list(events) == ref.events, label
    if tail is not None:
        want = M.text_tokens(tail)
        assert [(k, t) for _, t, k in events][-len(want):] == want, label
    assert status == ref.status(), label


def check_model(ref, model):
    check_against(ref, model.powers, model.tones, model.events, model.status())


# ---- the deliberately wrong models ----
class StageChain:
    """The modem's decimator the way k_morse_fir computes it, in fp64: out[o] = sum_p h[p] x[o D - (T-1) + p], x[< 0] the tail the stage
    carried from the call before.  zero_stage: that stage's tail is zeroed at every call."""

    def __init__(self, chain, zero_stage=None):
        from tests.decim_cases import halfband_taps
        self.chain = chain
        self.h = [halfband_taps()[t] for t, _ in chain]
        self.hist = [np.zeros(t - 1, dtype=np.complex128) for t, _ in chain]
        self.zero_stage = zero_stage

    def process(self, x):
        x = np.asarray(x, dtype=np.complex128)
        for j, (t, s) in enumerate(self.chain):
            if j == self.zero_stage:
                self.hist[j][:] = 0
            ext = np.concatenate([self.hist[j], x])
            self.hist[j] = ext[len(ext) - (t - 1):].copy()
            x = np.convolve(ext, self.h[j][::-1], "valid")[0:(len(x) // s) * s:s]
        return x


WRONG = ("goertzel_reset", "phase_late", "phase_early", "stage_zeroed", "rate_untruncated", "usec_rounded", "clock_skips_empty_calls",
         "log_not_drained")


class WrongRef(M.MorseRef):
    """MorseRef with one defect (`wrong`), or with none (wrong=None, stage_model=True: the decimator through StageChain, which must pass).

    goertzel_reset           (a) the Goertzel sums and count start from zero at every call
    phase_late, phase_early  (b) first = N - cnt0 + 1 / - 1: the first block of every call ends a sample late / early
    stage_zeroed             (c) stage `stage` starts every call from a zeroed tail
    rate_untruncated         (d) the chain's fractional rate in the coefficients, the clock and the status
    usec_rounded             (e) usecPerSample rounded, not truncated (N = 59 at 6000)
    clock_skips_empty_calls  (f) a call that completes no result does not move the clock
    log_not_drained          (g) no drain between reads: the device counts m / N + 1 possible events a call against the log's
                                 capacity of max(1024, 2 (m / N + 2)); events past that count are lost until the next read
    """

    def __init__(self, rate, frame, wrong=None, stage=None, stage_model=False):
        self.wrong = wrong
        super().__init__(rate, frame)
        chain, total, _, _ = geometry(rate)
        if wrong == "stage_zeroed" or stage_model:
            self.dec = StageChain(chain, stage if wrong == "stage_zeroed" else None)
        m = frame // total
        self.rmax = m // self.n + 1
        self.log_cap = max(1024, 2 * (m // self.n + 2))
        self.queued = 0

    def modem_rate_of(self, chain_rate):
        return float(chain_rate) if self.wrong == "rate_untruncated" else int(chain_rate)

    def best_n_of(self, rate):
        if self.wrong == "usec_rounded":
            return (M.DOT_MAGIC // ((M.WPM_LOW + M.WPM_HIGH) // 2) // 4) // int(round(1.0e6 / rate))
        return M.best_n(rate)

    def emit(self, kind, token):
        if self.wrong == "log_not_drained" and self.queued > self.log_cap:
            return
        super().emit(kind, token)

    def process(self, frame):
        if self.wrong == "goertzel_reset":
            self.s1 = self.s2 = 0j
            self.count = 0
        elif self.wrong == "phase_late":
            self.count -= 1
        elif self.wrong == "phase_early":
            self.count += 1
        clock, nres = self.clock, len(self.powers)
        self.queued += self.rmax
        super().process(frame)
        if self.wrong == "clock_skips_empty_calls" and len(self.powers) == nres:
            self.clock = clock
        return frame


def wrong_run(rate, frame, wrong, stage=None, stage_model=False):
    x, n1 = stream(rate, frame)
    return feed(WrongRef(rate, frame, wrong, stage, stage_model), x, n1, frame)
