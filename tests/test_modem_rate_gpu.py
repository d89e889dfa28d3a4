"""GPU tier (-m gpu) of the modem hook ring at a modem rate (pebblegpu_receiver_modem_out_open_rate, k_modem_rate_pack): every selected
channel's rows already through the reference's own Decimator chain for (max_bw, min_rate), on the device, in one launch per call.
Geometry, chains, references and bars: tests/modem_rate_cases.py.

The reference of a block row is oracle.Decimator(demodulator rate, max_bw, min_rate), fresh at open, fed exactly the present pairs of a
twin bank's plain F32 ring rows (existing code on identical input: bit for bit the hook's rows); the bar per present pair is
modem_out_cases.PAIR_BAR.  Where the state must stand still -- a closed gate, dmNONE, a one-channel receiver's closed call, a dropped
block -- two wrong models are computed on the oracle alone first and must miss the bar by a factor of ten."""
import os
import subprocess

import numpy as np
import pytest

from tests import modem_out_cases as MC
from tests import modem_rate_cases as RC
from tests import tail_cases as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def refused(P, code, fn, *args):
    with pytest.raises(P.PebbleGpuError) as e:
        fn(*args)
    assert e.value.code == code, e.value
    return str(e.value)


def close_all(*rxs):
    for rx in rxs:
        rx.close()


def hold_blocks(O, got, twin, rows, rate, bw, mn, spf, D, label):
    """every block row against its reference -> the worst figure; prints it"""
    figs = []
    for r in range(rows):
        figs += [(e, r, k, j) for e, k, j in RC.hold_row(O, got, twin, r, rate, bw, mn, spf, D, label)]
    assert figs, label
    worst = max(figs)
    print("%s (%d Hz, %d Hz): worst of %d present pairs %.3e (row %d, call %d super-frame %d), bar %.0e" % ((label, bw, mn, len(figs)) + worst + (MC.PAIR_BAR,)))
    bad = [f for f in figs if not f[0] <= MC.PAIR_BAR]
    assert not bad, bad
    return worst[0]


# ------------------------------------------------------------------------------------------------
# 1. ungated: every chain of the table
# ------------------------------------------------------------------------------------------------
# name: (channels, selection or None, noise-filter channels, calls in super-frames, the same stream cut another way)
UNGATED = {
    "five-permuted": (6, [4, 0, 5, 2, 1], (1, 4), (1, 3, 2, 3), (3, 1, 3, 2)),
    "seventy": (70, None, (0, 33, 69), (1, 2), (2, 1)),
}


@pytest.mark.parametrize("case,chain", [("five-permuted", c) for c in sorted(RC.CHAINS)] + [("seventy", (1000, 8000))],
                         ids=lambda v: v if isinstance(v, str) else "%d-%d" % v)
def test_ungated_every_chain(gpu_lib, oracle_mod, case, chain):
    """calls of 1, 3, 2 and max_sf super-frames through a permuted subset (and all 70 of 70): every pair, the very first (zero history)
    included, within the bar; flags all 1; rate and samples_per_superframe as defined; audio and kernel names are a twin's with the plain
    ring.

    The same stream cut into other call lengths: the decimated rows are bit-identical wherever the rows they are computed from are.  The
    hook's own rows (the plain ring, existing code) are NOT bit-identical between two cuts for every channel: measured here, channels 1, 2
    and 4 of `five-permuted` differ in up to 1076 of a super-frame's 2048 samples by an ulp or two behind a moved call boundary, channels
    0 and 5 -- at -+3/8 of the sample rate, where an oscillator is periodic in 8 samples; the cause was not looked for -- in none.  So a plain
    twin runs the other cut as well: every pair whose input (its own super-frame and the one in front of it, where its look-back lies) is
    bit-identical between the cuts must be bit-identical behind the decimator, whether it starts a call in one cut and sits inside a call
    in the other or not; channels 0 and 5 must be such rows throughout; and every pair of the other cut is held to the oracle on its
    own twin's rows like the first cut's"""
    import pebblesdr_amd as P
    C, sel, anf, calls, recut = UNGATED[case]
    bw, mn = chain
    stages, D = RC.CHAINS[chain]
    max_sf = max(calls)
    assert sum(calls) == sum(recut) and max(recut) <= max_sf and max_sf in calls
    a, b, c, d = (MC.usb_bank(P, C, 4096, max_sf, anf) for _ in range(4))   # rate ring; plain ring; both again, other calls
    try:
        assert a.superframe == TC.SF and int(a.info.demod_rate_int) == TC.RATE
        info = P.modem_rate_plan(TC.RATE, TC.SPF, bw, mn)
        assert info.chain() == stages and info.total_decimation == D
        x = MC.usb_stream(C, sum(calls), 9)
        rows_of = list(range(C)) if sel is None else sel
        a.modem_out_open_rate(bw, mn, MC.F32, sel, 4)
        b.modem_out_open(MC.F32, sel, 4)
        c.modem_out_open_rate(bw, mn, MC.F32, sel, 4)
        d.modem_out_open(MC.F32, sel, 4)
        got, twin, at = [], [], 0
        for ns in calls:
            seg = x[at * TC.SF:(at + ns) * TC.SF]
            at += ns
            assert np.array_equal(a.process(seg)[0], b.process(seg)[0]), "the rate ring changed the audio"
            got += MC.drain(a, 1)
            twin += MC.drain(b, 1)
            for w in range(1, 7):
                assert a.kernel_name(w) == b.kernel_name(w), (w, a.kernel_name(w), b.kernel_name(w))
        other, other_twin, at = [], [], 0
        for ns in recut:
            c.process(x[at * TC.SF:(at + ns) * TC.SF]); d.process(x[at * TC.SF:(at + ns) * TC.SF])
            at += ns
            other += MC.drain(c, 1)
            other_twin += MC.drain(d, 1)
        m = TC.SPF // D
        for k, (call, dropped, rows, present, rate) in enumerate(got):
            assert (call, dropped, rate) == (k, 0, int(info.rate_int)) and rate == TC.RATE // D
            assert rows.shape == (len(rows_of), calls[k] * m, 2) and rows.dtype == np.float32
            assert present.shape == (len(rows_of), calls[k]) and present.all()
        hold_blocks(oracle_mod, list(enumerate(got)), twin, len(rows_of), TC.RATE, bw, mn, TC.SPF, D, case)
        hold_blocks(oracle_mod, list(enumerate(other)), other_twin, len(rows_of), TC.RATE, bw, mn, TC.SPF, D, case + ", other calls")
        one, two = (np.concatenate([g[2] for g in blocks], axis=1) for blocks in (got, other))
        in_one, in_two = (np.concatenate([g[2] for g in blocks], axis=1) for blocks in (twin, other_twin))
        assert one.shape == two.shape and in_one.shape == in_two.shape and all(one[r].any() for r in range(len(rows_of)))
        starts = lambda cut: {sum(cut[:i]) for i in range(len(cut))}
        moved = starts(calls) ^ starts(recut)          # super-frames that start a call in one cut and not in the other
        checked = {r: set() for r in range(len(rows_of))}
        for r in range(len(rows_of)):
            same = [in_one[r, j * TC.SPF:(j + 1) * TC.SPF].tobytes() == in_two[r, j * TC.SPF:(j + 1) * TC.SPF].tobytes() for j in range(sum(calls))]
            for j in range(sum(calls)):
                if same[j] and (j == 0 or same[j - 1]):
                    assert one[r, j * m:(j + 1) * m].tobytes() == two[r, j * m:(j + 1) * m].tobytes(), "row %d super-frame %d: other call lengths change the rows" % (r, j)
                    checked[r].add(j)
        held = [len(v) for v in checked.values()]
        print("%s: %d of %d pairs held bit for bit between the cuts, %d rows throughout (super-frames %s change their place in a call)"
              % (case, sum(held), len(held) * sum(calls), sum(h == sum(calls) for h in held), sorted(moved)))
        assert moved and all(0 in v for v in checked.values())
        if case == "five-permuted":
            assert all(checked[rows_of.index(ch)] == set(range(sum(calls))) for ch in (0, 5)), checked
        assert a.modem_out_next(False) is None and a.modem_out_dropped() == 0
        a.modem_out_close()
    finally:
        close_all(a, b, c, d)


# ------------------------------------------------------------------------------------------------
# 2. S16 and the empty chain
# ------------------------------------------------------------------------------------------------
def test_s16_is_the_host_twin_of_the_f32_rows_and_the_empty_chain_is_the_plain_ring(gpu_lib):
    import pebblesdr_amd as P
    C, sel, calls = 6, [4, 0, 5, 2, 1], (1, 3, 2)
    a, b, c, d = (MC.usb_bank(P, C, 4096, 3, (1, 4)) for _ in range(4))   # S16 rate; F32 rate; empty chain; plain
    try:
        x = MC.usb_stream(C, sum(calls), 10)
        a.modem_out_open_rate(1000, 8000, MC.S16, sel, 4)
        b.modem_out_open_rate(1000, 8000, MC.F32, sel, 4)
        c.modem_out_open_rate(RC.EMPTY[0], RC.EMPTY[1], MC.S16, sel, 4)
        d.modem_out_open(MC.S16, sel, 4)
        at = 0
        for k, ns in enumerate(calls):
            if k in (1, 2):
                for rx in (a, b, c, d):
                    rx.set_mode(2, P.DM_NONE if k == 1 else P.DM_USB)    # an absent row in the middle of call 1's block
            seg = x[at * TC.SF:(at + ns) * TC.SF]
            at += ns
            blk = []
            for rx in (a, b, c, d):
                rx.process(seg)
                blk += MC.drain(rx, 1)
            s16, f32, empty, plain = blk
            assert s16[2].dtype == np.int16 and s16[2].shape == f32[2].shape == (len(sel), ns * TC.SPF // 8, 2)
            want = np.stack([P.modem_out_convert(MC.S16, f32[2][r]) for r in range(len(sel))])
            assert s16[2].tobytes() == want.tobytes() and s16[2].any(), k
            assert np.array_equal(s16[3], f32[3]) and (s16[4], f32[4]) == (8000, 8000)
            assert bool(s16[3][sel.index(2)].any()) == (k != 1)
            assert empty[2].tobytes() == plain[2].tobytes() and np.array_equal(empty[3], plain[3]) and empty[2].any(), k
            assert (empty[0], empty[1], empty[4]) == (plain[0], plain[1], plain[4]) == (k, 0, TC.RATE)
    finally:
        close_all(a, b, c, d)


# ------------------------------------------------------------------------------------------------
# 3. under the bank gate
# ------------------------------------------------------------------------------------------------
_TWIN = {}


def _gated_twin(P, name, ups):
    """the row through a bank with the PLAIN ring on every channel in a permuted order -> (audio per call, blocks); shared by the chains"""
    if (name, ups) not in _TWIN:
        rx = MC.row_bank(P, TC.ROWS[name])
        try:
            if ups is not None:
                rx.set_spectrum_updates(ups)
            rx.modem_out_open(MC.F32, GATED_SEL, 4)
            _TWIN[(name, ups)] = MC.run_row(rx, TC.ROWS[name], ring=True)
        finally:
            rx.close()
    return _TWIN[(name, ups)]


GATED_SEL = [3, 1, 5, 0, 4, 2]


def _gated(P, O, name, chain, ups):
    row = TC.ROWS[name]
    bw, mn = chain
    D = RC.CHAINS[chain][1]
    audio_twin, twin = _gated_twin(P, name, ups)
    # the two wrong models, on the oracle alone, before the device is judged: each misses the bar tenfold on a reopened pair of the row
    through = restarted = 0.0
    n_reopened = 0
    for r in range(len(GATED_SEL)):
        where = RC.reopened(twin, r)
        n_reopened += len(where)
        truth, w1, w2 = RC.wrong_models(O, twin, r, TC.RATE, bw, mn, TC.SPF)
        through = max(through, RC.miss_factor(truth, w1, where))
        restarted = max(restarted, RC.miss_factor(truth, w2, where))
    print("%s (%d Hz, %d Hz): on %d reopened pairs a decimator run through the absent pairs reads %.0f bars, one restarted at every call %.0f bars"
          % (name, bw, mn, n_reopened, through, restarted))
    assert n_reopened and through >= 10.0 and restarted >= 10.0
    ring = MC.row_bank(P, row)
    try:
        if ups is not None:
            ring.set_spectrum_updates(ups)
        ring.modem_out_open_rate(bw, mn, MC.F32, GATED_SEL, 4)
        audio, blocks = MC.run_row(ring, row, ring=True)
        for k in range(len(row.calls)):
            assert np.array_equal(audio[k], audio_twin[k]), "call %d: the rate ring changed the bank's audio" % k
        flags = np.concatenate([b[3] for b in twin], axis=1)
        assert flags.any() and not flags.all() and [b[0:2] for b in blocks] == [(k, 0) for k in range(len(row.calls))]
        hold_blocks(O, list(enumerate(blocks)), twin, len(GATED_SEL), TC.RATE, bw, mn, TC.SPF, D, name if ups is None else "%s, %d updates/s" % (name, ups))
    finally:
        ring.close()


@pytest.mark.parametrize("chain", sorted(RC.CHAINS), ids=lambda c: "%d-%d" % c)
@pytest.mark.parametrize("name", MC.GATE_ROWS)
def test_under_the_bank_gate(gpu_lib, oracle_mod, name, chain):
    """rows `gate` and `gate-thr` of tail_cases.ROWS, unchanged: flags equal the plain-ring twin's, absent pairs are all-zero, present pairs
    within the bar of the oracle fed present pairs only -- after both wrong models (run through the closed super-frames; restarted at every
    call) have missed that bar tenfold on the oracle alone"""
    import pebblesdr_amd as P
    _gated(P, oracle_mod, name, chain, None)


def test_under_the_bank_gate_with_the_update_timer(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    _gated(P, oracle_mod, "gate", (1000, 8000), 20)


# ------------------------------------------------------------------------------------------------
# 4. state standing still in other ways
# ------------------------------------------------------------------------------------------------
def test_a_channel_in_dmnone_for_two_calls(gpu_lib, oracle_mod):
    """channel 1 sits calls 1 and 2 out in dmNONE: its stream equals the oracle's with those pairs cut"""
    import pebblesdr_amd as P
    C, K, chain = 3, 5, (3000, 8000)
    a, b = MC.usb_bank(P, C, 0, 1, (1,)), MC.usb_bank(P, C, 0, 1, (1,))
    try:
        x = MC.usb_stream(C, K, 11)
        a.modem_out_open_rate(chain[0], chain[1], MC.F32, [2, 1, 0], 8)
        b.modem_out_open(MC.F32, [2, 1, 0], 8)
        for k in range(K):
            if k in (1, 3):
                for rx in (a, b):
                    rx.set_mode(1, P.DM_NONE if k == 1 else P.DM_USB)
            a.process(x[k * TC.SF:(k + 1) * TC.SF]); b.process(x[k * TC.SF:(k + 1) * TC.SF])
        got, twin = MC.drain(a, K), MC.drain(b, K)
        assert [int(t[3][1][0]) for t in twin] == [1, 0, 0, 1, 1]
        truth, w1, w2 = RC.wrong_models(oracle_mod, twin, 1, TC.RATE, chain[0], chain[1], TC.SPF)
        assert RC.miss_factor(truth, w1, {(3, 0)}) >= 10.0 and RC.miss_factor(truth, w2, {(3, 0)}) >= 10.0
        hold_blocks(oracle_mod, list(enumerate(got)), twin, 3, TC.RATE, chain[0], chain[1], TC.SPF, 8, "dmNONE")
    finally:
        close_all(a, b)


def test_one_channel_closed_calls(gpu_lib, oracle_mod):
    """a one-channel receiver's closed calls (threshold 50) give blocks of 0 samples, and the stream continues as if they were cut"""
    import pebblesdr_amd as P
    K, fc, chain = 5, 100e3, (1000, 8000)
    a, b = (MC.usb_bank(P, 1, 4096, 1, (0,), centres=[fc]) for _ in range(2))
    try:
        x = MC.usb_stream(1, K, 4, centres=[fc])
        a.modem_out_open_rate(chain[0], chain[1], MC.F32, None, 8)
        b.modem_out_open(MC.F32, None, 8)
        for k in range(K):
            if k in (2, 4):
                for rx in (a, b):
                    rx.set_squelch(0, 50.0 if k == 2 else -120.0)
            a.process(x[k * TC.SF:(k + 1) * TC.SF]); b.process(x[k * TC.SF:(k + 1) * TC.SF])
        got, twin = MC.drain(a, K), MC.drain(b, K)
        assert [g[2].shape[1] for g in got] == [256, 256, 0, 0, 256] and [t[2].shape[1] for t in twin] == [TC.SPF, TC.SPF, 0, 0, TC.SPF]
        assert [g[3].shape for g in got] == [(1, 1), (1, 1), (1, 0), (1, 0), (1, 1)] and [g[0] for g in got] == list(range(K))
        truth, _, w2 = RC.wrong_models(oracle_mod, twin, 0, TC.RATE, chain[0], chain[1], TC.SPF)
        assert RC.miss_factor(truth, w2, {(4, 0)}) >= 10.0    # (nothing is fed over a closed call: only the restart can be told apart)
        hold_blocks(oracle_mod, list(enumerate(got)), twin, 1, TC.RATE, chain[0], chain[1], TC.SPF, 8, "one channel")
    finally:
        close_all(a, b)


def test_dropped_blocks_were_never_delivered(gpu_lib, oracle_mod):
    """two slots, never released: calls 2 and 3 are dropped and counted; the blocks after the drop are the decimation of the delivered
    pairs only; the bank's audio is bit for bit a bank's without a ring"""
    import pebblesdr_amd as P
    C, K, chain = 5, 6, (1000, 8000)
    a, b, c = MC.usb_bank(P, C, 0, 2), MC.usb_bank(P, C, 0, 2), MC.usb_bank(P, C, 0, 2)   # rate ring, 2 slots; plain ring; no ring
    try:
        x = MC.usb_stream(C, K, 8)
        a.modem_out_open_rate(chain[0], chain[1], MC.F32, None, 2)
        b.modem_out_open(MC.F32, None, 8)
        got = []
        for k in range(K):
            seg = x[k * TC.SF:(k + 1) * TC.SF]
            if k == 4:   # calls 0..3 ran with nothing released: 0 and 1 are queued, 2 and 3 were dropped
                first = [a.modem_out_next(True), a.modem_out_next(True)]
                assert [(blk[0], blk[1]) for blk in first] == [(0, 0), (1, 0)] and a.modem_out_next(True) is None and a.modem_out_dropped() == 2
                for blk in first:
                    got.append((blk[0], blk))
                    a.modem_out_release(blk[0])
            audio = a.process(seg)[0]
            b.process(seg)
            assert np.array_equal(audio, c.process(seg)[0]), k
        twin = MC.drain(b, K)
        for blk in MC.drain(a, 2):
            got.append((blk[0], blk))
        assert [(k, blk[1]) for k, blk in got] == [(0, 0), (1, 0), (4, 2), (5, 0)] and a.modem_out_dropped() == 2
        # the wrong model: a decimator that was fed the dropped calls as well
        for r in (0, C - 1):
            truth = RC.decimated(oracle_mod, TC.RATE, chain[0], chain[1], [MC.as_complex(twin[k][2])[r] for k in (0, 1, 4, 5)])
            fed_all = RC.decimated(oracle_mod, TC.RATE, chain[0], chain[1], [MC.as_complex(twin[k][2])[r] for k in range(K)])
            assert MC.rel_rms(fed_all[4], truth[2]) >= 10.0 * MC.PAIR_BAR
        hold_blocks(oracle_mod, got, twin, C, TC.RATE, chain[0], chain[1], TC.SPF, 8, "drops")
    finally:
        close_all(a, b, c)


# ------------------------------------------------------------------------------------------------
# 5. the ring changes nothing else
# ------------------------------------------------------------------------------------------------
def test_morse_and_the_rate_ring_on_the_same_channels(gpu_lib):
    """with Morse on the same channels, events and status equal a run without the ring; audio rows are bit-identical with the ring open and
    closed; the kernel names are unchanged"""
    import pebblesdr_amd as P
    from tests import morse_ref as M
    C, K, per = 4, 8, 8
    fcs = [-300e3, -100e3, 100e3, 300e3]
    n = K * per * TC.SF
    x = TC.lcg_noise(n, 21, 2e-4)
    for i, c in enumerate((0, 2)):
        env = M.keying(("TEST", "CQ")[i], 30 + 5 * i, TC.FS)[:n]
        t = np.arange(len(env)) / float(TC.FS)
        x[:len(env)] += 0.01 * env * np.exp(2j * np.pi * (fcs[c] + 1000.0) * t)
    rxs = []
    try:
        for with_ring in (True, False):
            rx = P.ReceiverBank(TC.FS, C, True, False, 0, max_superframes=per)
            rxs.append(rx)
            for c in range(C):
                rx.set_mixer(c, fcs[c]); rx.set_bandpass(c, 300, 3000); rx.set_morse(c, True)
                rx.set_mode(c, P.DM_CWU)
            if with_ring:
                rx.modem_out_open_rate(1000, 8000, MC.F32, [2, 0], 4)
        a, b = rxs
        loud = False
        for k in range(K):
            seg = x[k * per * TC.SF:(k + 1) * per * TC.SF]
            assert np.array_equal(a.process(seg)[0], b.process(seg)[0]), k
            call, dropped, rows, present, rate = MC.drain(a, 1)[0]
            assert (call, dropped, rate) == (k, 0, 8000) and rows.shape == (2, per * TC.SPF // 8, 2) and present.all()
            loud = loud or bool(rows.any())
            for w in range(1, 7):
                assert a.kernel_name(w) == b.kernel_name(w), (k, w)
        assert loud
        events = 0
        for c in range(C):
            ea, eb = a.morse_events(c), b.morse_events(c)
            assert ea.tobytes() == eb.tobytes(), c
            assert a.morse_status(c) == b.morse_status(c), c
            events += len(eb)
        assert events > 0, "the keyed channels decode nothing: the comparison is empty"
    finally:
        close_all(*rxs)


# ------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(gpu_lib):
    import pebblesdr_amd as P
    a, b = MC.usb_bank(P, 2, 4096, 1), MC.usb_bank(P, 2, 4096, 1)
    w = P.ReceiverBank(2048000, 1, True, True, 0)
    x = MC.usb_stream(2, 2, 5)
    try:
        refused(P, RC.E_UNSUPPORTED, w.modem_out_open_rate, 1000, 8000)                       # no hook on WFM
        assert "CIC3" in refused(P, RC.E_UNSUPPORTED, a.modem_out_open_rate, RC.CIC3[0], RC.CIC3[1])
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 0, 8000)                              # max_bw == 0
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 1000, 8000, MC.S16_MONO)              # I, Q pairs only
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 1000, 8000, 3)
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 1000, 8000, MC.F32, [2])              # out of range
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 1000, 8000, MC.F32, [1, 1])           # duplicated
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 1000, 8000, MC.F32, [])               # empty
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 1000, 8000, MC.F32, None, 1)
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 1000, 8000, MC.F32, None, 9)
        refused(P, RC.E_INVALID, a.modem_out_next, False)                                     # nothing was opened by any of them
        a.modem_out_open_rate(1000, 8000, MC.F32, [1], 4)
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 1000, 8000)                           # a second open, of either kind
        refused(P, RC.E_INVALID, a.modem_out_open, MC.F32, None, 4)
        a.modem_out_close()
        a.modem_out_open(MC.F32, [1], 4)
        refused(P, RC.E_INVALID, a.modem_out_open_rate, 1000, 8000)
        refused(P, RC.E_UNSUPPORTED, a.modem_out_open_rate, RC.CIC3[0], RC.CIC3[1])           # (the plan is refused before the ring is looked at)
        # the handle is as it was: the plain ring that is open delivers, and the calls are a twin's
        a0, b0 = a.process(x[:TC.SF])[0], b.process(x[:TC.SF])[0]
        blk = MC.drain(a, 1)[0]
        assert (blk[0], blk[1], blk[4]) == (0, 0, TC.RATE) and np.array_equal(MC.as_complex(blk[2])[0], b0[1]) and np.array_equal(a0, b0) and a0.any()
        a.modem_out_close()
        a.modem_out_open_rate(1000, 8000, MC.F32, [1], 4)                                     # and a fresh rate ring opens after all of it
        a1, b1 = a.process(x[TC.SF:])[0], b.process(x[TC.SF:])[0]
        blk = MC.drain(a, 1)[0]
        assert (blk[0], blk[1], blk[4]) == (0, 0, 8000) and blk[2].shape == (1, 256, 2) and blk[2].any() and np.array_equal(a1, b1)
        a.modem_out_close()
    finally:
        close_all(a, b, w)


# ------------------------------------------------------------------------------------------------
# 7. other receivers and hosts
# ------------------------------------------------------------------------------------------------
def test_the_48k_receiver_without_a_decimator(gpu_lib, oracle_mod):
    """a 48 kHz receiver (the band-pass mixes in its loads, no decimator): (1000, 8000) gives [(11, 4), (15, 2)] and rate 6000"""
    import pebblesdr_amd as P
    fs, C, calls, centres = 48000, 3, (1, 3, 2), [-9000.0, 0.0, 9000.0]
    a, b = (MC.usb_bank(P, C, 0, 3, (0,), fs, centres) for _ in range(2))
    try:
        sf = a.superframe
        assert a.D == 1 and sf <= 2048
        x = MC.usb_stream(C, sum(calls), 7, fs, sf, centres)
        info = P.modem_rate_plan(fs, sf, 1000, 8000)
        assert info.chain() == [(11, 4), (15, 2)] and info.rate_int == 6000
        a.modem_out_open_rate(1000, 8000, MC.F32, [2, 0, 1], 4)
        b.modem_out_open(MC.F32, [2, 0, 1], 4)
        got, twin, at = [], [], 0
        for ns in calls:
            seg = x[at * sf:(at + ns) * sf]
            at += ns
            assert np.array_equal(a.process(seg)[0], b.process(seg)[0])
            got += MC.drain(a, 1)
            twin += MC.drain(b, 1)
        assert all(g[4] == 6000 and g[2].shape == (3, ns * sf // 8, 2) and g[3].all() for g, ns in zip(got, calls))
        hold_blocks(oracle_mod, list(enumerate(got)), twin, 3, fs, 1000, 8000, sf, 8, "48 kHz")
    finally:
        close_all(a, b)


def test_multibank_shards(gpu_lib):
    """the shards of a multibank open the rate ring through their borrowed handles: their rows are a single bank's, bit for bit"""
    import pebblesdr_amd as P
    C, sizes = 5, [1, 2, 1]
    mb = P.MultiBank(TC.FS, C, [0, 0], frames_per_buffer=TC.FRAME, max_superframes=2)
    one = MC.usb_bank(P, C, 0, 2, (1, 3))
    x = MC.usb_stream(C, sum(sizes), 12)
    fcs = MC.usb_centres(C)
    bufs = []
    try:
        for g, (first, count) in enumerate(mb.ranges):
            s = mb.shard(g)
            for c in range(count):
                s.set_mode(c, P.DM_USB); s.set_mixer(c, fcs[first + c]); s.set_bandpass(c, 300, 3000)
                if first + c in (1, 3):
                    s.set_noise_filter(c, True)
            s.modem_out_open_rate(1000, 8000, MC.F32, None, 4)
        one.modem_out_open_rate(1000, 8000, MC.F32, None, 4)
        at = 0
        for k in sizes:
            seg = np.atleast_2d(x[at * TC.SF:(at + k) * TC.SF])
            at += k
            bufs.append(P.DeviceBuffer.from_array(P.binding.to_f32_iq(seg), 0))
            one.process_device(bufs[-1].ptr, k * TC.SF)
            mb.process_device([bufs[-1].ptr] * mb.n_shards, k * TC.SF)
        want = MC.drain(one, len(sizes))
        for g, (first, count) in enumerate(mb.ranges):
            got = MC.drain(mb.shard(g), len(sizes))
            for k, (call, dropped, rows, present, rate) in enumerate(got):
                assert (call, dropped, rate) == (k, 0, 8000) and rows.shape == (count, sizes[k] * 256, 2) and present.all()
                assert np.array_equal(rows, want[k][2][first:first + count]), (g, k)
        assert all(w[2][r].any() for w in want for r in range(C))
        for g in range(mb.n_shards):
            mb.shard(g).modem_out_close()
    finally:
        for bf in bufs:
            bf.free()
        mb.close(); one.close()


@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_the_cpp_feeder_on_a_rate_ring(gpu_lib, tmp_path, fmt):
    """pebblegpu::feedModemBlock with the modem's frame (16 samples) on a ring at (1000, 8000): one callback per modem frame of every
    present (row, super-frame), in order, with the block's own samples"""
    lib, src, exe = os.path.join(ROOT, "pebblesdr_amd"), tmp_path / "feeder.cpp", str(tmp_path / "feeder")
    src.write_text(RC.rate_feeder_cpp())
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lpebblegpu", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, fmt], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    per_pair = (TC.SPF // 8) // (MC.DEMOD_FRAME // 8)
    assert per_pair == 16
    assert r.stdout.split() == ["callbacks", str(6 * per_pair), "expected", str(6 * per_pair), "absent", "6", "mismatches", "0", "order", "0"], r.stdout


def test_the_c_host(gpu_lib, tmp_path):
    """examples/modem_rate_host.c: a reader thread runs a tone detector on the 8 kHz rows of a 16-channel bank, no synchronize in either
    loop.  Channel 3 hears a tone 1 kHz above its centre: its +1000 Hz bin holds the tone and the -1000 Hz bin, 1536 whole cycles away over
    the 6144 samples, a thousandth of that power at most (the input's two bits of noise lie 60 dB further down per bin); channel 5 is
    in dmNONE: every pair absent, nothing detected"""
    src, exe = os.path.join(ROOT, "examples", "modem_rate_host.c"), str(tmp_path / "modem_rate_host")
    lib = os.path.join(ROOT, "pebblesdr_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lpebblegpu", "-Wl,-rpath," + lib, "-lm", "-lpthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith("channel 3:") and lines[1].startswith("channel 5:"), r.stdout
    w3, w5 = lines[0].split(), lines[1].split()
    up, dn, n, rate, absent3 = float(w3[4]), float(w3[7]), int(w3[9]), int(w3[12]), int(w3[14])
    assert rate == 8000 and n == 12 * 2 * 256 and absent3 == 0
    assert up > 0.0 and dn <= 1e-3 * up, (up, dn)
    assert (float(w5[4]), float(w5[7]), int(w5[9]), int(w5[14])) == (0.0, 0.0, 0, 24)
