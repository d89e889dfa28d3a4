"""GPU tier (-m gpu) of the Morse geometry table (tests/morse_cases.py): the stand-alone step at every (demodulator rate, frame) row
against the restatement, the refusal rows, and one receiver at the three-stage chain.  Only the public handles are used: no kernel is
launched directly and no environment switch is set.

MEASURED on the MI355X (worst relative power error over a row's results above -100 dB; bar 1e-5): 7.7e-7 to 1.2e-6 over the 32 rows
(8.5e-7 at 8000 with no stage at all: the fp32 input), the same figure at the same result whatever the frame; per rate in DESIGN.md
section 4, "Morse modem: chains, frames and block phases".  Smallest decision margin 2.0e-3 (8000), condition 1e-4.
"""
import numpy as np
import pytest

from tests import morse_cases as MC
from tests import morse_ref as M
from tests.signals import lcg_noise
from tests.test_morse_gpu import events_of, keyed, oracle_pre_agc

pytestmark = pytest.mark.gpu


def run_step(step, x, n1, frame, upto=None, start=0):
    """frames [start, upto) of the stream through the step, CWU from n1 on"""
    import pebblesdr_amd as P
    for k in range(start, len(x) // frame if upto is None else upto):
        if k * frame == n1:
            step.setDemodMode(P.DM_CWU)
        fr = x[k * frame:(k + 1) * frame]
        assert step.processBlock(fr) is fr


@pytest.mark.parametrize("row", MC.rows(), ids=MC.row_id)
def test_step_rows_against_the_restatement(gpu_lib, oracle_mod, row):
    """P.Morse(rate, frame) against MorseRef(rate, frame) with test_step_against_the_restatement's bars: result counts equal, decisions
    identical, powers within 1e-5 relative above -100 dB, events identical (read once, at the end: at the min frame that is after more
    calls than the device log has entries) with the tail decoding to "MORSE", status equal."""
    import pebblesdr_amd as P
    rate, frame = row
    ref = MC.reference(rate, frame)
    x, n1 = MC.stream(rate, frame)
    step = P.Morse(rate, frame, keep_results=True)
    try:
        run_step(step, x, n1, frame)
        p, tone = step.results()
        ev = events_of(step.events())
        MC.check_against(ref, p, tone.tolist(), ev, step.status(), label="morse %d/%d" % row)
        assert len(step.events()) == 0  # drained
    finally:
        step.close()


@pytest.mark.parametrize("rate,frame,code", MC.REFUSALS, ids=lambda v: str(v))
def test_create_refusals(gpu_lib, rate, frame, code):
    import pebblesdr_amd as P
    with pytest.raises(P.PebbleGpuError) as e:
        P.Morse(rate, frame)
    assert e.value.code == MC.CODES[code]


def test_refused_set_sample_rate_leaves_the_decoder_running(gpu_lib, oracle_mod):
    """Every refusal row asked of a running step, between frames: each is refused with its code, and results, events and status stay
    exactly those of a twin that never asked (and both are the restatement's).  A refusal used to release the core and the input
    buffer first; now it is decided before the handle is touched."""
    import pebblesdr_amd as P
    rate, frame = 64000, 648
    ref = MC.reference(rate, frame)
    x, n1 = MC.stream(rate, frame)
    nf = len(x) // frame
    asked = P.Morse(rate, frame, keep_results=True)
    twin = P.Morse(rate, frame, keep_results=True)
    try:
        at = [nf // 5, nf // 3, nf // 2, (3 * nf) // 4]  # spread over both messages, the second message's marks included
        pos = 0
        for k, (r, f, code) in zip(at, MC.REFUSALS):
            run_step(asked, x, n1, frame, upto=k, start=pos)
            pos = k
            before = asked.status()
            with pytest.raises(P.PebbleGpuError) as e:
                asked.setSampleRate(r, f)
            assert e.value.code == MC.CODES[code], (r, f)
            # (a handle the refusal had emptied fails here, at status(), before another frame could be copied to a freed buffer)
            assert asked.n == frame and asked.status() == before
        run_step(asked, x, n1, frame, start=pos)
        run_step(twin, x, n1, frame)
        pa, ta = asked.results()
        pb, tb = twin.results()
        ea, eb = events_of(asked.events()), events_of(twin.events())
        assert np.array_equal(pa, pb) and np.array_equal(ta, tb)
        assert ea == eb and len(ea) > 0
        assert asked.status() == twin.status()
        MC.check_against(ref, pa, ta.tolist(), ea, asked.status(), label="refused setSampleRate %d/%d" % (rate, frame))
    finally:
        asked.close()
        twin.close()


def test_receiver_row_at_the_three_stage_chain(gpu_lib, oracle_mod):
    """2.4 Msps / 64 = 37 500 Hz at the modem hook: chain (11,2),(15,2),(19,2), modem rate 4687 (of 4687.5), N = 46.  Channels 0 and 2
    keyed at their own speeds, channel 1 with the modem off (a hole in the channel list), calls of 1, 2, 1, 3, ... super-frames so that
    tails, Goertzel sums and clock carry over unequal calls.  Events and status per channel equal the restatement fed the oracle
    chain's pre-AGC signal."""
    import pebblesdr_amd as P
    fs, C = 2_400_000, 3
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=3)
    try:
        sf = rx.superframe
        sizes = [1, 2, 1, 3] * 5
        n = sum(sizes) * sf
        fcs = [-300e3, 50e3, 410e3]
        # (text, wpm, what its tail must decode to: from 20 WPM thresholds the first marks at 40 WPM are mis-timed, as in test_morse_host)
        msgs = {0: ("TEST", 25, "TEST"), 2: ("MORSE", 40, "SE")}
        x = lcg_noise(n, 37, 2e-4)
        for c, (text, wpm, _) in msgs.items():
            x += keyed(text, wpm, fs, n, fcs[c] + 1000.0, 0.01)
        for c in range(C):
            rx.set_mixer(c, fcs[c])
            rx.set_bandpass(c, 300, 3000)
            if c in msgs:
                rx.set_morse(c, True)
            rx.set_mode(c, P.DM_CWU)  # after the enable: the modem follows the mode (CWL -> CWU)
        pos = 0
        for s in sizes:
            rx.process(x[pos * sf:(pos + s) * sf])
            pos += s
        assert events_of(rx.morse_events(1)) == []
        with pytest.raises(P.PebbleGpuError):
            rx.morse_status(1)
        for c, (_, _, tail) in msgs.items():
            a, rate = oracle_pre_agc(oracle_mod, x, fs, fcs[c], 300, 3000)
            assert rate == 37500 and MC.geometry(rate) == ([(11, 2), (15, 2), (19, 2)], 8, 4687, 46)
            r = M.MorseRef(rate, sf // 64)
            r.set_demod_mode(M.DM_CWU)
            assert len(a) == sum(sizes) * (sf // 64)
            for k in range(sum(sizes)):
                r.process(a[k * (sf // 64):(k + 1) * (sf // 64)])
            got = events_of(rx.morse_events(c))
            print("receiver channel %d: %d events, smallest margin %.3e" % (c, len(r.events), min(r.margins)))
            assert min(r.margins) > MC.MARGIN, (c, min(r.margins))
            assert got == r.events, (c, got, r.events)
            want = M.text_tokens(tail)
            assert [(k, t) for _, t, k in got][-len(want):] == want, c
            assert rx.morse_status(c) == r.status()
    finally:
        rx.close()
