"""GPU tier (-m gpu) of tests/morse_hard_cases.py: the device's Morse modem (k_morse_goertzel, k_morse_decide) on keying that takes the
decoder's rare arms -- rejected spikes, both range verdicts, the WPM_VAR pulls, a full element buffer, a token that is no character,
a tone back before the element threshold, speed changes, a mode change and a setSampleRate in the middle of a character.

Three ways: the device against the restatement (tests/morse_ref.py) with morse_cases.check_against as it stands -- counts equal,
decisions identical, powers within 1e-5, events identical, status equal, the status read at three cut points as well -- and, at
64 000 / 2048, against the reference's own compiled decoder as recorded in tests/golden/refpin_morse_hard_*.npy (events, decisions,
every status), which the restatement is held to bit for bit on the CPU (tests/test_reference_pins.py)."""
import numpy as np
import pytest

from tests import morse_cases as MC
from tests import morse_hard_cases as H
from tests import morse_ref as M
from tests import reference_cases as R
from tests.signals import lcg_noise
from tests.test_morse_gpu import events_of, oracle_pre_agc, ref_events

pytestmark = pytest.mark.gpu

KEYS = ("wpm", "above_range", "below_range", "modem_rate", "samples_per_result")   # a status record's first five values


def run_step(P, name, rate, frame):
    """the row through P.Morse frame by frame, its plan carried out -> (powers, decisions, events, the statuses feed() reads)"""
    x, plan = H.stream(name, rate, frame)
    step = P.Morse(rate, frame, keep_results=True)
    pw, tn, ev, seen = [], [], [], []

    def read():
        p, t = step.results()      # (setSampleRate starts the read-out afresh: collect before it)
        pw.append(p)
        tn.append(t)
        ev.extend(events_of(step.events()))

    for k in range(len(x) // frame):
        for at, what in plan:
            if at != k * frame:
                continue
            if what in ("status", "rate"):
                read()
                seen.append(step.status())
            if what == "rate":
                step.setSampleRate(rate, frame)
            elif what != "status":
                step.setDemodMode(H.ACT[what])
        step.processBlock(x[k * frame:(k + 1) * frame])
    read()
    seen.append(step.status())
    assert len(step.events()) == 0
    step.close()
    return np.concatenate(pw), np.concatenate(tn), ev, seen


@pytest.mark.parametrize("name", H.NAMES)
def test_hard_row_at_the_bench_rate_against_restatement_and_reference(gpu_lib, oracle_mod, name):
    import pebblesdr_amd as P
    ref = H.reference(name)
    pw, tn, ev, seen = run_step(P, name, H.RATE, H.FRAME)
    MC.check_against(ref, pw, tn, ev, seen[-1], label="%s %d/%d" % (name, H.RATE, H.FRAME), tail=H.row(name).tail)
    assert seen == [s for s, _ in ref.seen]
    # ... and the reference's own decoder, as recorded
    case = next(c for c in R.cases() if c.name == "morse_hard_%s_%d" % (name, H.RATE))
    fx = R.morse_fixture(case)
    assert len(pw) == fx["results"] and [bool(t) for t in tn] == fx["decisions"]
    assert ev == fx["events"]
    assert [[s[k] for k in KEYS] for s in seen] == [s[:5] for s in fx["statuses"]]
    tail = fx["powers"]
    assert np.max(np.abs(pw[len(pw) - len(tail):] - tail) / np.maximum(tail, 1e-10)) <= MC.POWER_BAR


@pytest.mark.parametrize("name", H.NAMES)
def test_hard_row_in_minimal_calls(gpu_lib, oracle_mod, name):
    """12 000 Hz in the smallest frames the modem takes: most calls complete no Goertzel block and every transition of the row falls
    between calls"""
    import pebblesdr_amd as P
    rate, frame = H.SLOW_RATE, MC.min_frame(H.SLOW_RATE)
    ref = H.reference(name, rate, frame)
    pw, tn, ev, seen = run_step(P, name, rate, frame)
    MC.check_against(ref, pw, tn, ev, seen[-1], label="%s %d/%d" % (name, rate, frame), tail=H.row(name).tail)
    assert seen == [s for s, _ in ref.seen]


# ---- three lanes of one bank, each on its own rare arms ----
BANK_FS = 2048000
BANK_FC = (100e3, -250e3, 412.5e3)
BANK_MODE = (M.DM_CWU, M.DM_CWL, M.DM_CWU)
BANK_AMP, BANK_NOISE = 0.01, 2e-4


def bank_input(sf):
    """the three rows of H.BANK_ROWS keyed at their carriers +- 1000 Hz, a whole number of groups of 1 + 3 + 2 super-frames"""
    envs = [H.envelope(H.row(n).segs, BANK_FS) / H.AMP * BANK_AMP for n in H.BANK_ROWS]
    n = -(-max(len(e) for e in envs) // (6 * sf)) * 6 * sf
    x = lcg_noise(n, 61, BANK_NOISE)
    t = np.arange(n) / float(BANK_FS)
    for e, fc, mode in zip(envs, BANK_FC, BANK_MODE):
        f = fc + (1000.0 if mode == M.DM_CWU else -1000.0)
        x[:len(e)] += e * np.exp(2j * np.pi * f * t[:len(e)])
    return x


def bank_band(mode):
    return (300, 3000) if mode == M.DM_CWU else (-3000, -300)


def bank_reference(oracle_mod, x, c):
    """test_morse_gpu.ref_events' chain for the lane (for the dmCWL lane with the band-pass on the lower side), through CountingRef,
    so that the arms the lane takes through the bank's own chain are on record"""
    a, rate = oracle_pre_agc(oracle_mod, x, BANK_FS, BANK_FC[c], *bank_band(BANK_MODE[c]))
    r = H.CountingRef(rate, 2048)
    r.set_demod_mode(BANK_MODE[c])
    for k in range(len(a) // 2048):
        r.process(a[k * 2048:(k + 1) * 2048])
    return r


# what each lane must take through the bank's chain, as its row does at the step
BANK_ARMS = (("sm.mark.short_to_mark", "sm.mark.short_to_word"), ("ut.ratio_dash", "ut.ratio_dot"), ("sm.inter.buffer_full",))


def test_three_lanes_of_a_bank_on_different_rare_arms(gpu_lib, oracle_mod):
    """one ReceiverBank, three channels in dmCWU / dmCWL / dmCWU carrying the two-result spikes, the speed changes and the nine dots, in
    calls of 1, 3 and 2 super-frames: k_morse_decide's per-channel state does not leak between lanes on the rare arms"""
    import pebblesdr_amd as P
    rx = P.ReceiverBank(BANK_FS, 3, True, False, 0, max_superframes=3)
    sf = rx.superframe
    for c in range(3):
        rx.set_mixer(c, BANK_FC[c])
        rx.set_bandpass(c, *bank_band(BANK_MODE[c]))
        rx.set_morse(c, True)
        rx.set_mode(c, P.DM_CWU if BANK_MODE[c] == M.DM_CWU else P.DM_CWL)
    x = bank_input(sf)
    pos, k = 0, 0
    got = {c: [] for c in range(3)}
    while pos < len(x):
        s = (1, 3, 2)[k % 3] * sf
        rx.process(x[pos:pos + s])
        pos, k = pos + s, k + 1
        if k % 7 == 0:
            for c in range(3):
                got[c] += events_of(rx.morse_events(c))
    for c in range(3):
        got[c] += events_of(rx.morse_events(c))
    refs = [bank_reference(oracle_mod, x, c) for c in range(3)]
    for c, r in enumerate(refs):
        assert min(r.margins) > H.MARGIN, (c, min(r.margins))
        assert got[c] == r.events and len(r.events) > 0, (c, got[c], r.events)
        assert rx.morse_status(c) == r.status(), c
        for a in BANK_ARMS[c]:
            assert r.arms[a] > 0, (c, a)
        if BANK_MODE[c] == M.DM_CWU:      # (the counting restatement is test_morse_gpu.ref_events' restatement)
            plain = ref_events(oracle_mod, x, BANK_FS, BANK_FC[c])
            assert plain.events == r.events and plain.status() == r.status()
    # the spikes and the full buffer stay in their lanes; the speed lane's estimate moves up and ends away from the others' 20 to 24
    assert refs[1].arms["sm.mark.short_to_word"] == 0 and refs[2].arms["sm.mark.short_to_mark"] == 0 and refs[0].arms["sm.inter.buffer_full"] == 0
    assert refs[1].status()["wpm"] > refs[0].status()["wpm"] > refs[2].status()["wpm"]
    # the lanes decode what their rows decode to at the step (the same keying through another chain): different from each other
    tokens = [[t for _, t, k in r.events if k == M.CHAR] for r in refs]
    assert tokens[0] != tokens[1] != tokens[2] != tokens[0]
    rx.close()
