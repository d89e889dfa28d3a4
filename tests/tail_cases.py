"""The coverage statement for the tail of a narrow bank -- what runs behind the band-pass: k_anf, k_agc, k_iir_scan<2,1>, k_fir_dec, k_save_tail,
k_pll_demod, k_gate_eval, k_gate_zero and the deferred refresh in k_save_tails (csrc/kernels_demod.h, csrc/kernels_frontend.h, csrc/tail_refresh.h).
Their arithmetic is pinned stage by stage elsewhere; the rows here pin their INDEXING and their STATE HANDLING: each kernel walks a channel list
rebuilt by the host (Receiver::apply_controls, AgcCore::apply, AnfCore::apply), maps a lane or a workgroup to a listed channel, and keeps
per-channel state that must sleep whenever the reference would not have run it (dmNONE, another demodulator mode, a closed squelch gate).

One table of rows, their signals, the oracle drivers and the deliberately wrong models, used by the CPU tier (tests/test_narrow_tail_host.py: the
rows are well formed, reach the list sizes they are there for, the oracle Receiver is the chain of its own parts, and every wrong model misses the
GPU bar by a factor of 100 or more) and by the GPU tier (tests/test_narrow_tail_gpu.py: the same rows through P.ReceiverBank against the oracle).

All rows: one shared stream at 1 024 000 samples/s; oracle.Receiver(1024000, 2048, 0) has four stages, D = 16, demodulator rate 64 000 and a
super-frame of 32 768 samples, 2048 outputs each.  Bars: the suite's own (tests/test_parity_gpu.py), per chunk of 512 consecutive outputs;
compared_chunks() says which chunks those are where the stream starts, and why.

The `modes` row lists five scripted channels and channel 0's twin, six in all.  Channel 2 (SAM, SAM, AM, SAM, FMN, SAM) listens to an AM
carrier that is frequency-modulated only while its FMN call's samples pass (0.217 s .. 0.277 s of the stream): Demod_SAM's float loop is
chaotic under a phase modulation it cannot follow (the oracle fed its own input rounded to fp32 moves by 5e-2 there), and Demod_NFM on a
carrier without one delivers noise alone, on which a relative bar measures nothing (1e-3 by the same test); with the window both stay under
5e-6 and 2e-7.
"""
from collections import namedtuple
import functools

import numpy as np

from tests.demod_cases import chunk_bounds, rel_rms  # noqa: F401  (chunk_bounds is part of this module's interface)
from tests.signals import lcg_noise
from tests.test_parity_gpu import TOL, TOL_AGC_STARTUP

FS, FRAME, SF, SPF, RATE, D = 1024000, 2048, 32768, 2048, 64000, 16
CHUNK = 512
TOL_SAM = 1e-4      # the in-phase form (re + im) / 2, tests/test_parity_gpu.py::test_sam_pll_demod_step
TOL_ANF = 1e-6      # k_anf against oracle.Anf on identical input, tests/test_parity_gpu.py::test_noise_filter_anf
WRONG_FACTOR = 100  # every wrong model misses the channel's bar by this factor at least, on the first chunk it changes
MODE = {"AM": 0, "SAM": 1, "FMN": 2, "USB": 7, "NONE": 12}   # DEMODMODE; oracle.AM .. oracle.NONE and P.DM_AM .. P.DM_NONE (asserted by both tiers)
AGC_OFF, AGC_FAST, AGC_MED, AGC_SLOW = 0, 1, 2, 3
BAND = {"AM": (-5000.0, 5000.0), "SAM": (-5000.0, 5000.0), "FMN": (-7500.0, 7500.0), "USB": (300.0, 3000.0)}
K_MAX_TAPS = 80     # common.h kMaxTaps: the head-room of AmCore::tmp and PllCore::tmp
HI, LO = 0.1, 0.001  # a keyed carrier's two levels: the low one still 40 dB over the noise, so a reopened PLL locks at once
RS_PERIODS = 28     # fractresampler.cpp: an output at time T reads the inputs floor(T) - 27 .. floor(T)

# fc: mixer frequency; band: set_bandpass; modes: the demodulator mode during every call; agc: (mode, threshold) or None (AGC_OFF at unit gain, the
# constructor's state); anf: noise filter on; squelch: threshold in dB, None = never set (-120)
Chan = namedtuple("Chan", "fc band modes agc anf squelch")
# carriers: [(fc, signal, key)]: key None (level HI throughout) or one 0 / 1 per super-frame (LO / HI)
# actions: [(call, channel, kind, args)] setters issued before that call, after the call's mode changes: "bandpass" (lo, hi), "squelch" (dB,)
Row = namedtuple("Row", "name chans carriers calls max_sf bins audio_rate actions noise seed why")


# ------------------------------------------------------------------------------------------------
# signals
# ------------------------------------------------------------------------------------------------
def _carrier(sig, fc, t, level):
    kind, w = sig[0], 2 * np.pi * fc * t
    if kind == "am":      # a carrier with two modulating tones, turned in phase
        _, f1, f2, ph = sig
        return level * (1 + 0.5 * np.cos(2 * np.pi * f1 * t + ph) + 0.3 * np.cos(2 * np.pi * f2 * t)) * np.exp(1j * (w + ph))
    if kind == "amfm":    # the same, frequency-modulated as well while t_on <= t < t_off (whole cycles of fm: the phase stays continuous)
        _, f1, f2, fm, beta, t_on, t_off = sig
        assert abs(fm * t_on - round(fm * t_on)) < 1e-9 and abs(fm * t_off - round(fm * t_off)) < 1e-9
        pm = np.where((t >= t_on) & (t < t_off), beta * np.sin(2 * np.pi * fm * t), 0.0)
        return level * (1 + 0.5 * np.cos(2 * np.pi * f1 * t) + 0.3 * np.cos(2 * np.pi * f2 * t + 0.5)) * np.exp(1j * (w + pm))
    if kind == "fm":
        _, fm, beta = sig
        return level * np.exp(1j * (w + beta * np.sin(2 * np.pi * fm * t)))
    if kind == "tones":   # two tones above the mixer frequency (USB)
        _, o1, o2 = sig
        return level * (np.exp(2j * np.pi * (fc + o1) * t) + 0.6 * np.exp(1j * (2 * np.pi * (fc + o2) * t + 0.7)))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def row_input(name):
    row = ROWS[name]
    n = sum(row.calls) * SF
    t = np.arange(n) / float(FS)
    x = lcg_noise(n, row.seed, row.noise)
    for fc, sig, key in row.carriers:
        level = HI if key is None else np.repeat(np.where(np.asarray(key) > 0, HI, LO), SF)
        x = x + _carrier(sig, fc, t, level)
    x.setflags(write=False)
    return x


def call_offsets(row):
    """[(first super-frame, super-frames)] of every call"""
    out, at = [], 0
    for k in row.calls:
        out.append((at, k))
        at += k
    return out


# ------------------------------------------------------------------------------------------------
# the rows
# ------------------------------------------------------------------------------------------------
def _modes_row():
    fcs = [-400e3, -240e3, -80e3, 80e3, 240e3, 400e3]
    am0 = ("am", 700.0, 3.0, 0.4)
    chans = [
        # leaves AM for two calls of OTHER lengths (1 and 3 super-frames after a call of 2) and returns without a set_bandpass: the idle Demod_AM
        # keeps its delay line (Demod::setDemodMode stores the mode only), so the FIR's history is the end of call 0
        Chan(fcs[0], BAND["AM"], ("AM", "USB", "USB", "AM", "AM", "AM"), None, False, None),
        Chan(fcs[1], BAND["AM"], ("AM",) * 6, None, False, None),                                    # keeps the AM list non-empty
        Chan(fcs[2], BAND["SAM"], ("SAM", "SAM", "AM", "SAM", "FMN", "SAM"), None, False, None),
        Chan(fcs[3], BAND["FMN"], ("FMN", "NONE", "FMN", "FMN", "USB", "FMN"), None, False, None),
        Chan(fcs[4], BAND["USB"], ("USB",) * 6, (AGC_MED, 30), True, None),
        # channel 0's twin on another carrier: the same script, and set_bandpass(-5000, 5000) again after the return, the UI's order, which
        # clears the delay line in both implementations (CFir::InitLPFilter)
        Chan(fcs[5], BAND["AM"], ("AM", "USB", "USB", "AM", "AM", "AM"), None, False, None),
    ]
    carriers = [(fcs[0], am0, None), (fcs[1], ("am", 1000.0, 3300.0, 1.1), None), (fcs[2], ("amfm", 900.0, 2100.0, 1000.0, 1.5, 0.217, 0.277), None),
                (fcs[3], ("fm", 800.0, 2.0), None), (fcs[4], ("tones", 1100.0, 2300.0), None), (fcs[5], ("am", 650.0, 5.0, 2.0), None)]
    return Row("modes", chans, carriers, (2, 1, 3, 1, 2, 1), 3, 0, 0, [(3, 5, "bandpass", BAND["AM"])], 1e-4, 41,
               "mode changes AM <-> USB, SAM <-> AM <-> FMN, FMN <-> NONE / USB with list rebuilds; a channel sits out calls of another length")


LISTS_C = 200
LISTS_MANUAL = (7, 131)   # AGC_OFF with the gain slider at 30: 10^(6/20); listed like every running AGC


def lists_carrier(c):
    """the carrier channel c of the `lists` row listens to -> index into the row's twelve: 0..5 FM, 6..11 AM"""
    q = c // 3
    return q % 6 if c % 3 == 0 else 6 + (q % 6 if c % 3 == 1 else (q + 2) % 6)


def _lists_row():
    fcs = [(i - 5.5) * 80e3 for i in range(12)]
    carriers = [(fcs[i], ("fm", 500.0 + 150.0 * i, 1.5 + 0.1 * i), None) for i in range(6)] + \
               [(fcs[6 + i], ("am", 600.0 + 170.0 * i, 2000.0 + 210.0 * i, 0.3 * i), None) for i in range(6)]
    agc_cycle = [(AGC_FAST, 20), (AGC_MED, 30), (AGC_SLOW, 30)]
    chans, k = [], 0
    for c in range(LISTS_C):
        mode = ("FMN", "SAM", "AM")[c % 3]
        agc = None
        if c % 5 != 0:
            agc = (AGC_OFF, 30) if c in LISTS_MANUAL else agc_cycle[k % 3]
            k += 1
        chans.append(Chan(fcs[lists_carrier(c)], BAND[mode], (mode,) * 3, agc, False, None))
    return Row("lists", chans, [(fc, sig, key) for fc, sig, key in carriers], (1, 2, 1), 2, 0, 0, [], 1e-4, 42,
               "67 / 67 / 66 entries in the FMN / SAM / AM lists and 160 in the AGC list: second and third workgroups of k_pll_demod and k_agc, the last ragged")


def _anf_row():
    fcs = [-400e3, -240e3, -80e3, 80e3, 240e3, 400e3]
    usb = ("USB",) * 3
    chans = [Chan(fcs[c], BAND["USB"], ("USB", "NONE", "USB") if c == 3 else usb, None, c in (1, 3, 4), None) for c in range(6)]
    carriers = [(fcs[c], ("tones", 900.0 + 130.0 * c, 2000.0 + 90.0 * c), None) for c in range(6)]
    return Row("anf-list", chans, carriers, (1, 2, 1), 2, 0, 0, [], 1e-4, 43,
               "k_anf's list {1, 3, 4}, then {1, 4} while channel 3 is tune-only (muted), then {1, 3, 4} again: entries that are not 0..n-1")


GATE_BINS = 4096
GATE_CALLS = (3, 1, 2, 2)
# one 0 / 1 per super-frame; calls cover super-frames 0-2 | 3 | 4-5 | 6-7.  Every pattern: a run of one closed super-frame, a run of two or more,
# a close -> open step inside a call and one across a call boundary (asserted by the CPU tier)
GATE_KEYS = [(1, 0, 1, 1, 0, 0, 1, 1), (0, 1, 1, 0, 1, 0, 0, 1), (1, 0, 0, 1, 0, 1, 1, 0), (0, 0, 1, 0, 1, 1, 0, 1), (0, 1, 0, 0, 1, 1, 0, 1)]
# thresholds: the midpoint of the oracle's fdEstimate avgDb between the keyed levels (the CPU tier measures both states of every channel and
# asserts the midpoint within 1 dB of these and 10 dB of margin to either side)
GATE_THR = {"AM": -49.0, "SAM": -49.0, "FMN": -52.0, "USB": -43.0}
_GATE_FCS = [-400e3, -240e3, -80e3, 80e3, 240e3, 400e3]
_GATE_SIGS = [("am", 700.0, 1900.0, 0.4), ("am", 1000.0, 2600.0, 1.1), ("am", 900.0, 2100.0, 0.2), ("fm", 800.0, 2.0), ("tones", 1100.0, 2300.0), ("tones", 1300.0, 2500.0)]


def _gate_chans(squelch=True):
    spec = [("AM", (AGC_SLOW, 30), False), ("AM", (AGC_FAST, 20), True), ("SAM", None, False), ("FMN", None, False), ("USB", (AGC_MED, 30), True),
            ("USB", None, False)]   # the last one never gates
    n = len(GATE_CALLS)
    return [Chan(_GATE_FCS[c], BAND[m], (m,) * n, agc, anf, GATE_THR[m] if (squelch and c < 5) else None) for c, (m, agc, anf) in enumerate(spec)]


def _gate_row(name, audio_rate, why):
    carriers = [(_GATE_FCS[c], _GATE_SIGS[c], GATE_KEYS[c] if c < 5 else None) for c in range(6)]
    return Row(name, _gate_chans(), carriers, GATE_CALLS, 3, GATE_BINS, audio_rate, [], 1e-5, 44, why)


def _gate_thr_row():
    """the carriers at full level throughout; the gate closes because the threshold is raised between calls, and opens when it is put back"""
    chans = _gate_chans()
    carriers = [(_GATE_FCS[c], _GATE_SIGS[c], None) for c in range(6)]
    actions = []
    for c in range(5):
        k = 1 if c % 2 == 0 else 2   # channels 0, 2, 4 sit out call 1 (one super-frame), channels 1 and 3 call 2 (two)
        actions += [(k, c, "squelch", (50.0,)), (k + 1, c, "squelch", (chans[c].squelch,))]
    return Row("gate-thr", chans, carriers, GATE_CALLS, 3, GATE_BINS, 0, actions, 1e-5, 45, "set_squelch between calls closes and reopens the gate")


def _gate_one_row():
    ch = Chan(_GATE_FCS[0], BAND["AM"], ("AM",) * len(GATE_CALLS), (AGC_FAST, 20), False, GATE_THR["AM"])
    return Row("gate-one", [ch], [(_GATE_FCS[0], _GATE_SIGS[0], GATE_KEYS[0])], GATE_CALLS, 3, GATE_BINS, 0, [], 1e-5, 46,
               "a one-channel handle created for three super-frames per call takes the per-channel route (Receiver::set_squelch: C != 1 || max_sf != 1)")


ROWS = {r.name: r for r in (_modes_row(), _lists_row(), _anf_row(),
                            _gate_row("gate", 0, "every tail kernel under a Gate: AM + AGC SLOW, AM + AGC FAST + ANF, SAM, FMN, USB + ANF + AGC MED, USB never gated"),
                            _gate_thr_row(), _gate_one_row(),
                            _gate_row("gate-11025", 11025, "the same with audio_rate set: the resampler sees the silence of a closed stretch"))}


def mode_lists(row, call):
    """the three demodulator lists, the ANF list and the AGC list of this call as the host builds them (Receiver::apply_controls: by mode;
    AnfCore::apply: on and not muted; AgcCore::apply: every mode but AGC_OFF at unit gain, not muted; muted = tune-only)"""
    out = {"AM": [], "SAM": [], "FMN": [], "ANF": [], "AGC": []}
    for c, ch in enumerate(row.chans):
        m = ch.modes[call]
        if m in ("AM", "SAM", "FMN"):
            out[m].append(c)
        if ch.anf and m != "NONE":
            out["ANF"].append(c)
        if ch.agc is not None and not (ch.agc[0] == AGC_OFF and ch.agc[1] // 5 == 0) and m != "NONE":
            out["AGC"].append(c)
    return out


def actions_before(row, call, ch):
    return [(kind, args) for k, c, kind, args in row.actions if k == call and c == ch]


# ------------------------------------------------------------------------------------------------
# bars and comparison
# ------------------------------------------------------------------------------------------------
def sam_form(a):
    a = np.asarray(a)
    return (a.real + a.imag) / 2


def agc_running(c):
    """a running AGC (its log detector, its 960-sample delay line), not the manual gain of AGC_OFF"""
    return c.agc is not None and c.agc[0] != AGC_OFF


def chan_bar(row, ch, via_twin=False):
    """the bar of a channel and whether it is compared in SAM's in-phase form.  via_twin: compared with the oracle's parts run on the band-passed
    row of a twin bank (identical input), the way a channel behind the noise filter is compared"""
    c = row.chans[ch]
    sam = "SAM" in c.modes
    bar = TOL_ANF if (via_twin and c.anf) else TOL
    if agc_running(c):
        bar = max(bar, TOL_AGC_STARTUP)
    if sam:
        bar = max(bar, TOL_SAM)
    return bar, sam


AGC_DELAY = 960    # (int)(64000 * .015), agc.cpp's DELAY_TIMECONST: a running AGC delivers its input this many samples late
FLOOR = 3e-8       # absolute error of the fp32 overlap-save band-pass under full-level samples of the same block (tests/test_parity_gpu.py, TOL_AGC_STARTUP)


def chunk_figures(got, want, sam, bounds):
    """rel-RMS of the given chunks of one super-frame; the lengths must agree exactly"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == (SPF,), (got.shape, want.shape)
    if sam:
        got, want = sam_form(got), sam_form(want)
    return [rel_rms(got[lo:hi], want[lo:hi]) for lo, hi in bounds]


FOUR = chunk_bounds(SPF, CHUNK)


def script_opened(row, ch):
    """[call][super-frame]: whether the row's script has the channel deliver that super-frame -- its carrier keyed up, its threshold not raised
    for the call, its mode not tune-only.  The CPU tier holds the oracle Receiver to this at the gated rows"""
    c = row.chans[ch]
    key = {fc: k for fc, _, k in row.carriers}[c.fc]
    thr, out = c.squelch, []
    for k, (s0, ns) in enumerate(call_offsets(row)):
        for what, args in actions_before(row, k, ch):
            if what == "squelch":
                thr = args[0]
        gated = thr is not None and thr > -120.0
        raised = gated and thr > 0
        out.append([c.modes[k] != "NONE" and not raised and not (gated and key is not None and not key[j]) for j in range(s0, s0 + ns)])
    return out


TOL_NFM_WRAP = 3e-3   # chunk 0 behind an FMN acquisition (compared_chunks, chunk_bar)


def via_twin(row, ch):
    """a channel behind the noise filter is compared with the oracle's parts run on the band-passed row of a twin bank: identical input"""
    return row.chans[ch].anf


def _behind_acquisition(row, ch, k, j):
    """the stream's second super-frame of a channel whose FMN loop acquired in the first"""
    c = row.chans[ch]
    return call_offsets(row)[k][0] + j == 1 and c.modes[k] == "FMN" and c.modes[0] == "FMN" and script_opened(row, ch)[0][0]


def compared_chunks(row, ch, k, j):
    """the chunks of call k's super-frame j that the GPU tier compares -> [(lo, hi)]; empty where the script has the channel deliver nothing.
    Four chunks of 512 outputs.  Where the stream starts the band-pass fills, and its first outputs, the edge of a 1025-tap response over the
    first input samples, lie under the fp32 floor of the overlap-save block they come from (FLOOR, absolute, under a stream at 0.1).  The CPU
    tier (test_where_the_stream_starts_...) feeds the oracle's own parts the oracle's band-passed row plus FLOOR of white noise, for every
    channel of every row, and holds this rule to what it reads: a chunk is joined to the one behind it only where the oracle itself loses
    the channel's bar on it, and every chunk that is compared holds the bar there.  In the stream's first super-frame:
      - an AM channel without a running AGC: chunk 0 joins chunk 1 (alone 1.2 .. 1.3 bars under that floor; SAM, 0.2 .. 0.3 of its bar,
        and USB, 0.5 .. 0.7, keep all four);
      - behind a running AGC: chunk 0 is the first 512 of the 960 zeros of its delay line (both sides exactly zero, figure 0); chunk 1, 448 zeros
        and the band-pass's first 64 outputs (over a thousand bars under that floor), joins chunk 2;
      - a channel behind the noise filter is compared on identical input (via_twin), where no floor enters: all four;
      - an FMN channel's first super-frame is not compared: its PLL, which does not weigh by amplitude, acquires on that floor along another
        path (tests/test_parity_gpu.py::test_bank_with_every_narrow_demod_mode).  Nothing else is left out."""
    if not script_opened(row, ch)[k][j]:
        return []
    c, at = row.chans[ch], call_offsets(row)[k][0] + j
    if at == 0 and not via_twin(row, ch):
        if c.modes[k] == "FMN":
            return []
        if agc_running(c):
            return [FOUR[0], (FOUR[1][0], FOUR[2][1]), FOUR[3]]
        if c.modes[k] == "AM":
            return [(FOUR[0][0], FOUR[1][1]), FOUR[2], FOUR[3]]
    return FOUR


def chunk_bar(row, ch, k, j, lo):
    """the bar of the chunk of call k's super-frame j that starts at output lo: the channel's (chan_bar), but TOL_NFM_WRAP on chunk 0 of the
    super-frame behind an FMN acquisition.  Demod_NFM wraps its float phase at the end of every block; the run-up of the acquisition (up to
    1.47 rad per sample at the loop's limit) leaves that phase in the hundreds, where a float resolves 3e-5 .. 6e-5 rad, and two loops that
    ended the block one such step apart start the next a true 6e-5 rad apart -- a transient the loop and its DC average take some hundred
    samples to pull in.  The oracle under FLOOR reads up to 1.1e-3 (110 bars) over that chunk and 2.9e-5 still over its second half, and
    under 1e-6 in the three chunks behind it; the CPU tier asserts those figures, the bar is three times the worst.  A call-to-call carry
    gone wrong (the loop's state, the FIR's history) reads 1.0 or more there (the `foreign` models at the `lists` row's call 1: 333 bars and more)."""
    if lo == 0 and _behind_acquisition(row, ch, k, j):
        return TOL_NFM_WRAP
    return chan_bar(row, ch, via_twin=via_twin(row, ch))[0]


def expected_chunks(row, channels):
    """what the GPU tier must have compared -> (chunks, outputs of delivered super-frames left out of every chunk: the stream's first
    super-frame of each FMN channel open there, SPF outputs each, and nothing else)"""
    n = skipped = 0
    for ch in channels:
        for k, (s0, ns) in enumerate(call_offsets(row)):
            for j in range(ns):
                if script_opened(row, ch)[k][j]:
                    b = compared_chunks(row, ch, k, j)
                    n += len(b)
                    skipped += SPF - sum(hi - lo for lo, hi in b)
    return n, skipped


# ------------------------------------------------------------------------------------------------
# oracle drivers
# ------------------------------------------------------------------------------------------------
def oracle_receiver(O, row, ch, kind="full"):
    """one oracle Receiver for channel ch, set up in the order the GPU tier sets the bank up: mode, mixer, band-pass, AGC, noise filter, squelch.
    kind "full": the channel as the row has it; "bandpass": USB with AGC and noise filter off and the same squelch -- its output is the channel's
    band-passed row on the super-frames the gate lets through; "open": the same, never gated"""
    c = row.chans[ch]
    r = O.Receiver(FS, FRAME, row.bins)
    r.set_mode(MODE[c.modes[0]] if kind == "full" else MODE["USB"])
    r.set_mixer(c.fc)
    r.set_filter(*c.band)
    if kind == "full":
        if c.agc is not None:
            r.set_agc(*c.agc)
        if c.anf:
            r.set_anf(True)
        if row.audio_rate:
            r.set_audio_rate(row.audio_rate)
    if c.squelch is not None and kind != "open":
        r.set_squelch(c.squelch)
    return r


def oracle_rows(O, row, ch, kind="full"):
    """-> [call][super-frame] arrays: what the Receiver delivers for every super-frame (nothing where it returns early)"""
    c, x = row.chans[ch], row_input(row.name)
    r = oracle_receiver(O, row, ch, kind)
    out = []
    for k, (s0, ns) in enumerate(call_offsets(row)):
        if kind == "full" and k and c.modes[k] != c.modes[k - 1]:
            r.set_mode(MODE[c.modes[k]])
        for what, args in actions_before(row, k, ch):
            if what == "bandpass":
                r.set_filter(*args)
            elif what == "squelch" and kind != "open":
                r.set_squelch(*args)
        call = []
        for j in range(s0, s0 + ns):
            fr = [r.process(x[j * SF + f * FRAME:j * SF + (f + 1) * FRAME], want_spectrum=bool(row.bins))[0] for f in range(SF // FRAME)]
            call.append(np.concatenate(fr))
        out.append(call)
    return out


_CACHE = {}


def cached_rows(O, name, ch, kind="full"):
    key = (name, ch, kind)
    if key not in _CACHE:
        _CACHE[key] = oracle_rows(O, ROWS[name], ch, kind)
    return _CACHE[key]


def opened_of(rows):
    return [[len(a) > 0 for a in call] for call in rows]


def gate_levels(O, row, ch):
    """the oracle's fdEstimate avgDb of every super-frame's last raw frame (the spectrum the gate reads, receiver.cpp:959-965) -> [super-frame]"""
    c, x = row.chans[ch], row_input(row.name)
    sp = O.Spectrum(row.bins, FRAME)
    out = []
    for j in range(sum(row.calls)):
        for f in range(SF // FRAME):   # the spectrum averages nothing over frames here, but it is run on every frame as the Receiver runs it
            db = sp.process(x[j * SF + f * FRAME:j * SF + (f + 1) * FRAME])
        out.append(float(O.fd_estimate(db, FS, np.float32(c.band[0]), np.float32(c.band[1]), c.fc)[1]))
    return out


# ------------------------------------------------------------------------------------------------
# the chain behind the band-pass, composed of the oracle's own parts -- and the wrong models, each one change to it
# ------------------------------------------------------------------------------------------------
class Parts:
    """NoiseFilter, AGC and the three demodulator objects of one channel (receiver.cpp:974-987), with the channel's mode script"""

    def __init__(self, O, row, ch):
        self.c = row.chans[ch]
        self.row, self.ch = row, ch
        self.anf = O.Anf() if self.c.anf else None
        self.agc = None
        if self.c.agc is not None:
            self.agc = O.Agc(RATE)
            self.agc.set_mode(*self.c.agc)
        self.dem = {"AM": O.DemodAM(RATE), "SAM": O.DemodSAM(RATE), "FMN": O.DemodNFM(RATE)}
        self.used = set()
        self.am_in = None           # the AM FIR's input over the channel's last AM call (the content of AmCore::tmp's row)
        if self.c.modes[0] == "AM":
            self.dem["AM"].set_bandwidth(self.c.band[1] - self.c.band[0])   # Demod::setBandwidth acts in AM only (demod.cpp:230-239)

    def before_call(self, k):
        for what, args in actions_before(self.row, k, self.ch):
            if what == "bandpass" and self.c.modes[k] == "AM":
                self.dem["AM"].set_bandwidth(args[1] - args[0])
        self._am_call = []

    def after_call(self, k):
        if self._am_call:
            self.am_in = np.concatenate(self._am_call)

    def _am_fir_input(self, y):
        """Demod_AM's DC block restated (demod_am.cpp:40-64) from the object's own state, without touching it"""
        last, out = float(self.dem["AM"].s.dc_last), np.empty(len(y))
        a = float(np.float32(0.9999))
        for i, m in enumerate(np.abs(y)):
            dc = a * last + m
            out[i] = dc - last
            last = dc
        return out

    def run(self, k, y, awake=()):
        """one open super-frame of call k.  awake: parts a wrong model runs although the channel sits this super-frame out"""
        mode = self.c.modes[k]
        if self.anf is not None:
            y = self.anf.process(y)
        if self.agc is not None:
            y = self.agc.process(y)
        if mode in self.dem:
            if mode == "AM":
                self._am_call.append(self._am_fir_input(y))
            self.used.add(mode)
            y = self.dem[mode].process(y)
        for m in awake:
            if m in self.dem and m != mode and m in self.used:
                self.dem[m].process(y)
        return y

    def idle(self, k, y, awake):
        """a super-frame the channel sits out altogether (tune-only, or a closed gate): nothing runs -- unless a wrong model keeps parts awake"""
        if "ANF" in awake and self.anf is not None:
            y = self.anf.process(y)
        if "AGC" in awake and self.agc is not None:
            y = self.agc.process(y)
        for m in awake:
            if m in self.dem and m in self.used:
                self.dem[m].process(y)

    def stale_am_history(self, at):
        """the defect of a deferred refresh that touches every row: the AM FIR's delay line becomes am_in[at - T .. at) of the stale row (the end of
        a sat-out call of `at` samples) instead of the end of the last AM call"""
        s = self.dem["AM"].s.lp
        T = s.ntaps
        assert self.am_in is not None and T <= at <= len(self.am_in) and T - 1 <= K_MAX_TAPS
        for m in range(1, T + 1):   # slot state + m holds the input m samples back (po_fir_process_cpx writes slot `state`, then steps it down)
            s.zre[(s.state + m) % T] = s.zim[(s.state + m) % T] = float(self.am_in[at - m])


def compose(O, row, ch, bp, opened, wrong=None):
    """the channel's output per super-frame from its band-passed rows bp[call][sf] (2048 samples each, never gated) and the gate's decisions
    opened[call][sf] -> [call][sf] arrays, empty where the Receiver delivers nothing.  wrong: None, or one of
      ("stale_am", call, at)        the AM delay line taken from the middle of the stale row before this call
      ("awake", parts)              these parts ("AM", "SAM", "FMN", "AGC", "ANF") advanced through what the channel sits out
      ("foreign", call, other_ch, other_bp, other_opened)   for one call the channel runs on another channel's state blocks (list index used as
                                    channel index; channel c given the state of c - 64), which that channel gets back afterwards
      ("gate_shift",)               gate row j read as j - 1 within a call (row 0 as it is)
      ("let_through",)              a closed super-frame's band-pass samples delivered
    A wrong model delivers a super-frame of zeros where it gates what the Receiver delivers (the bank's audio row reads as silence there)."""
    kind = wrong[0] if wrong else None
    own = Parts(O, row, ch)
    other = Parts(O, row, wrong[2]) if kind == "foreign" else None
    awake = tuple(wrong[1]) if kind == "awake" else ()
    out = []
    for k, call in enumerate(bp):
        own.before_call(k)
        if other:
            other.before_call(k)
        if kind == "stale_am" and wrong[1] == k:
            own.stale_am_history(wrong[2])
        op = list(opened[k])
        if kind == "gate_shift":
            op = [op[0]] + op[:-1]
        res = []
        for j, y in enumerate(call):
            mode = own.c.modes[k]
            delivered = opened[k][j] and mode != "NONE"   # what the Receiver does
            exchanged = kind == "foreign" and wrong[1] == k
            if other is not None and not exchanged and wrong[4][k][j] and other.c.modes[k] != "NONE":
                other.run(k, wrong[3][k][j])   # the other channel on its own samples, so that its blocks are where they should be at the exchange
            if op[j] and mode != "NONE":
                if exchanged:   # the other channel's blocks, this channel's samples and mode
                    keep, other.c = other.c, own.c
                    res.append(other.run(k, y))
                    other.c = keep
                else:
                    res.append(own.run(k, y, awake))
            elif kind == "let_through" and mode != "NONE":
                res.append(np.array(y))
            else:
                own.idle(k, y, awake)
                res.append(np.zeros(len(y) if delivered else 0, dtype=np.complex128))
        own.after_call(k)
        if other:
            other.after_call(k)
        out.append(res)
    return out


def first_miss(row, ch, want, got):
    """the first chunk the model changes, of those the GPU tier compares (compared_chunks; the four of 512 where the Receiver delivers nothing,
    which counts as silence, as the bank's audio row holds it) -> (call, super-frame, (lo, hi), rel-RMS there, the chunk's bar), or None when
    it changes nothing"""
    sam = chan_bar(row, ch)[1]
    for k, (wc, gc) in enumerate(zip(want, got)):
        for j, (w, g) in enumerate(zip(wc, gc)):
            bounds = compared_chunks(row, ch, k, j) if len(w) else FOUR
            w = w if len(w) else np.zeros(SPF, dtype=np.complex128)
            g = g if len(g) else np.zeros(SPF, dtype=np.complex128)
            for lo, hi in bounds:
                if not np.array_equal(w[lo:hi], g[lo:hi]):
                    a, b = (sam_form(g[lo:hi]), sam_form(w[lo:hi])) if sam else (g[lo:hi], w[lo:hi])
                    # (the channel's bar against the oracle chain, the wider one where the GPU tier goes by a twin bank's row)
                    return k, j, (lo, hi), rel_rms(a, b), max(chunk_bar(row, ch, k, j, lo), chan_bar(row, ch)[0])
    return None
