"""GPU tier (-m gpu) of the modem hook ring (pebblegpu_receiver_modem_out_*): the rows a digital-modem plugin receives, behind the noise
filter and ahead of the AGC, through pinned egress slots, with a trailer that says which (channel, super-frame) the reference would have
handed to the hook at all.  Geometry, references and bars: tests/modem_out_cases.py (tail_cases' own: 1.024 Msps, D = 16, 2048
demodulator samples per super-frame, 128 per frame).

Ungated banks are held bit for bit to the MODEM tap of a twin receiver that gets the same calls; gated banks -- where a tap cannot be
enabled at all -- to the oracle: flags to its Receiver's own decisions, band-passed rows at the project's bar, rows behind the noise
filter to oracle.Anf run over the opened super-frames only."""
import os
import subprocess

import numpy as np
import pytest

from tests import modem_out_cases as MC
from tests import tail_cases as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def refused(P, code, fn, *args):
    with pytest.raises(P.PebbleGpuError) as e:
        fn(*args)
    assert e.value.code == code, e.value


def all_differ(blocks):
    return len({np.ascontiguousarray(w).tobytes() for w in blocks}) == len(blocks)


# ------------------------------------------------------------------------------------------------
# 1. ungated, bit for bit against the tap
# ------------------------------------------------------------------------------------------------
# name: (fs, channels, spectrum bins, selection or None, noise-filter channels, calls in super-frames, {call: channels in dmNONE})
UNGATED = {
    "five-permuted": (TC.FS, 6, 4096, [4, 0, 5, 2, 1], (1, 4), (1, 3, 2), {1: (2,)}),
    "all-by-null": (TC.FS, 6, 4096, None, (0, 3), (1, 3, 2), {0: (5,), 1: (5,), 2: ()}),
    "seventy": (TC.FS, 70, 4096, None, tuple(range(70)), (1, 2), {1: (69,)}),        # k_anf's list of 70: more than one 64-entry list
    "two-stage": (TC.FS, 6, 0, [5, 1, 3], (1,), (1, 3, 2), {2: (3,)}),                # no display transform
    "no-decimator": (48000, 3, 0, [2, 0, 1], (0,), (1, 3, 2), {1: (1,)}),             # a 48 kHz receiver: the band-pass mixes in its loads
}


@pytest.mark.parametrize("fmt", [MC.F32, MC.S16], ids=["F32", "S16"])
@pytest.mark.parametrize("case", sorted(UNGATED))
def test_ungated_bit_for_bit_against_the_tap(gpu_lib, case, fmt):
    import pebblesdr_amd as P
    fs, C, bins, sel, anf, calls, none = UNGATED[case]
    centres = [-9000.0, 0.0, 9000.0] if fs == 48000 else None
    a, b, c = (MC.usb_bank(P, C, bins, max(calls), anf, fs, centres) for _ in range(3))   # ring; MODEM tap; neither
    try:
        sf, D = a.superframe, a.D
        x = MC.usb_stream(C, sum(calls), 7, fs, sf, centres)
        b.set_taps([P.TAP_MODEM])
        a.modem_out_open(fmt, sel, 4)
        rows_of = list(range(C)) if sel is None else sel
        want, at = [], 0
        for k, ns in enumerate(calls):
            for rx in (a, b, c):
                for ch in range(C):
                    now, before = ch in none.get(k, ()), k > 0 and ch in none.get(k - 1, ())
                    if now != before:
                        rx.set_mode(ch, P.DM_NONE if now else P.DM_USB)
            seg = x[at * sf:(at + ns) * sf]
            at += ns
            audio_a, audio_b, audio_c = a.process(seg)[0], b.process(seg)[0], c.process(seg)[0]
            tap, rate = b.tap(P.TAP_MODEM)
            assert tap.shape == (C, ns * sf // D)
            want.append(MC.expected_from_tap(P, fmt, tap, rows_of, none.get(k, ()), ns))
            assert audio_b.shape == audio_a.shape
            assert np.array_equal(audio_a, audio_c), "call %d: the ring changed the audio" % k
            for w in range(1, 7):   # the ring changes no route and no kernel: the strings of the same receiver with the ring closed
                assert a.kernel_name(w) == c.kernel_name(w), (k, w, a.kernel_name(w), c.kernel_name(w))
        got = MC.drain(a, len(calls))
        for k, (call, dropped, rows, present, brate) in enumerate(got):
            assert (call, dropped, brate) == (k, 0, int(rate))
            assert rows.shape == want[k][0].shape == (len(rows_of), calls[k] * sf // D, 2) and rows.dtype == want[k][0].dtype
            assert np.array_equal(present, want[k][1]), "call %d flags" % k
            assert rows.tobytes() == want[k][0].tobytes(), "call %d" % k
            for r, ch in enumerate(rows_of):
                assert rows[r].any() == (ch not in none.get(k, ())), (k, ch)
        assert all_differ([w[0] for w in want])
        assert a.modem_out_next(False) is None and a.modem_out_dropped() == 0
        a.modem_out_close()
    finally:
        for rx in (a, b, c):
            rx.close()


# ------------------------------------------------------------------------------------------------
# 2. under the bank gate
# ------------------------------------------------------------------------------------------------
def _gated(P, O, name, ups):
    """one gated row with the ring open on every channel in a permuted order -> the figures, after holding every pair to its reference.
    ups None: flags against the oracle Receiver's decisions (run_gate_eval).  ups > 0: the update timer is on (run_gate_eval_rows), which the
    oracle does not model: flags against what a twin bank without the ring delivers"""
    row = TC.ROWS[name]
    C = len(row.chans)
    sel = [3, 1, 5, 0, 4, 2]
    ring, plain, open_twin = MC.row_bank(P, row), MC.row_bank(P, row), MC.row_bank(P, row, twin=True, squelch=False)
    try:
        if ups is not None:
            for rx in (ring, plain, open_twin):
                rx.set_spectrum_updates(ups)
        ring.modem_out_open(MC.F32, sel, 4)
        audio, blocks = MC.run_row(ring, row, ring=True)
        audio_plain, _ = MC.run_row(plain, row)
        bp_twin, _ = MC.run_row(open_twin, row, twin=True, squelch=False)   # band-passed rows of the noise-filter channels, never gated
        for k in range(len(row.calls)):
            assert np.array_equal(audio[k], audio_plain[k]), "call %d: the ring changed the bank's audio" % k
        offs = TC.call_offsets(row)
        compared = absent = 0
        figs = []   # (rel-RMS / bar, rel-RMS, bar, channel, call, super-frame)
        wrong_worst = 0.0
        for r, ch in enumerate(sel):
            if ups is None:
                opened = TC.opened_of(TC.cached_rows(O, name, ch, "bandpass"))
                assert opened == TC.script_opened(row, ch)
            else:
                opened = [[bool(audio_plain[k][ch][j * TC.SPF:(j + 1) * TC.SPF].any()) for j in range(ns)] for k, (_, ns) in enumerate(offs)]
            got = [[MC.as_complex(blocks[k][2])[r][j * TC.SPF:(j + 1) * TC.SPF] for j in range(ns)] for k, (_, ns) in enumerate(offs)]
            flags = [[bool(blocks[k][3][r][j]) for j in range(ns)] for k, (_, ns) in enumerate(offs)]
            assert flags == opened, (ch, flags, opened)
            if row.chans[ch].anf:
                bp = MC.split_sf(bp_twin, ch, row)
                ref = MC.anf_reference(O, bp, opened)
                wrong = MC.anf_reference(O, bp, opened, through_closed=True)
                bar = TC.TOL_ANF
            else:
                # the oracle's band-passed rows: of the super-frames its gate lets through, or (the update timer's flags are not the oracle's) of all
                ref = TC.cached_rows(O, name, ch, "bandpass" if ups is None else "open")
                wrong, bar = None, MC.PAIR_BAR
            for k, (_, ns) in enumerate(offs):
                assert blocks[k][2].shape == (C, ns * TC.SPF, 2) and blocks[k][3].shape == (C, ns) and (blocks[k][0], blocks[k][1]) == (k, 0)
                for j in range(ns):
                    if not opened[k][j]:
                        assert not got[k][j].any(), "channel %d call %d super-frame %d is absent: zeros" % (ch, k, j)
                        absent += 1
                        continue
                    e = MC.rel_rms(got[k][j], ref[k][j])
                    figs.append((e / bar, e, bar, ch, k, j))
                    compared += 1
                    if wrong is not None:
                        wrong_worst = max(wrong_worst, MC.rel_rms(got[k][j], wrong[k][j]) / bar)
        for bar in sorted({f[2] for f in figs}):
            _, e, _, ch, k, j = max(f for f in figs if f[2] == bar)
            print("%s%s: bar %.0e: worst of %d present pairs %.3e (channel %d, call %d super-frame %d)"
                  % (name, "" if ups is None else " (%d updates/s)" % ups, bar, sum(f[2] == bar for f in figs), e, ch, k, j))
        print("%s: the noise filter kept running through closed super-frames would read %.1f bars" % (name, wrong_worst))
        # every selected (channel, super-frame) of every call was either compared or found absent and zero: none left out
        assert compared + absent == C * sum(row.calls)
        if ups is None:
            assert compared == sum(op for ch in range(C) for call in TC.script_opened(row, ch) for op in call)
        assert compared and absent
        bad = [f for f in figs if not f[0] <= 1.0]
        assert not bad, bad
        if ups is None:   # (under the update timer the noise-filter channels need not close at all)
            assert wrong_worst > 1.0, "the wrong model (noise filter running through closed super-frames) must miss the bar"
        else:
            print("%s (%d updates/s): flags per selected row %s" % (name, ups, [[int(f) for f in np.concatenate([b[3][r] for b in blocks])] for r in range(C)]))
        return compared
    finally:
        for rx in (ring, plain, open_twin):
            rx.close()


@pytest.mark.parametrize("name", MC.GATE_ROWS)
def test_under_the_bank_gate(gpu_lib, oracle_mod, name):
    """rows `gate` and `gate-thr` of tail_cases.ROWS, unchanged: flags equal the oracle Receiver's decisions, absent pairs are all-zero,
    present pairs meet TOL against the oracle's band-passed rows (TOL_ANF against oracle.Anf over the opened super-frames behind the noise
    filter), the count of compared pairs is the script's, the noise filter run through closed super-frames misses the bar, and the bank's
    audio is bit for bit a twin's without the ring"""
    import pebblesdr_amd as P
    n = _gated(P, oracle_mod, name, None)
    assert n == {"gate": sum(sum(k) for k in TC.GATE_KEYS) + 8, "gate-thr": 5 * 8 - (1 + 2 + 1 + 2 + 1) + 8}[name]


def test_under_the_bank_gate_with_the_update_timer(gpu_lib, oracle_mod):
    """the `gate` row once more under set_spectrum_updates(20): every super-frame's decision comes from the latest computed spectrum
    (run_gate_eval_rows), not from its own last frame's; the flags are held to what a twin bank without the ring delivers, the rows to the
    same references and bars"""
    import pebblesdr_amd as P
    _gated(P, oracle_mod, "gate", 20)


# ------------------------------------------------------------------------------------------------
# 3. Morse and ring on the same channels
# ------------------------------------------------------------------------------------------------
def test_morse_and_ring_on_the_same_channels(gpu_lib):
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
                rx.modem_out_open(MC.S16, [2, 0], 4)
        a, b = rxs
        loud = False
        for k in range(K):
            seg = x[k * per * TC.SF:(k + 1) * per * TC.SF]
            assert np.array_equal(a.process(seg)[0], b.process(seg)[0]), k
            call, dropped, rows, present, _ = MC.drain(a, 1)[0]
            assert (call, dropped) == (k, 0) and rows.shape == (2, per * TC.SPF, 2) and present.all()
            loud = loud or bool(rows.any())   # (PCM16 of a keyed-up stretch; between the words the noise alone truncates to 0)
        assert loud
        events = 0
        for c in range(C):
            ea, eb = a.morse_events(c), b.morse_events(c)
            assert ea.tobytes() == eb.tobytes(), c
            assert a.morse_status(c) == b.morse_status(c), c
            events += len(eb)
        assert events > 0, "the keyed channels decode nothing: the comparison is empty"
    finally:
        for rx in rxs:
            rx.close()


# ------------------------------------------------------------------------------------------------
# 4. ring rules
# ------------------------------------------------------------------------------------------------
def test_drops(gpu_lib):
    """a full ring drops and counts, it never refuses -- and the chain does not notice (tests/test_audio_out_gpu.py::test_drops)"""
    import pebblesdr_amd as P
    C, K = 5, 5
    a, b = MC.usb_bank(P, C, 0, 2), MC.usb_bank(P, C, 0, 2)
    x = MC.usb_stream(C, K, 8)
    try:
        b.set_taps([P.TAP_MODEM])
        a.modem_out_open(MC.F32, None, 2)
        want, bufs = [], []
        for k in range(K):
            seg = x[k * TC.SF:(k + 1) * TC.SF]
            b.process(seg)
            want.append(MC.expected_from_tap(P, MC.F32, b.tap(P.TAP_MODEM)[0], range(C), (), 1)[0])
            bufs.append(P.DeviceBuffer.from_array(P.binding.to_f32_iq(np.atleast_2d(seg)), 0))
        for buf in bufs[:4]:   # 4 calls, nothing released
            a.process_device(buf.ptr, TC.SF)
        first = [a.modem_out_next(True), a.modem_out_next(True)]
        assert [(blk[0], blk[1]) for blk in first] == [(0, 0), (1, 0)]
        assert a.modem_out_next(True) is None   # calls 2 and 3 were dropped
        assert a.modem_out_dropped() == 2
        for k in (0, 1):
            assert np.array_equal(first[k][2], want[k])
            a.modem_out_release(k)
        a.process_device(bufs[4].ptr, TC.SF)
        call, dropped, rows, present, _ = a.modem_out_next(True)
        assert (call, dropped) == (4, 2) and present.all()
        assert np.array_equal(rows, want[4])   # b never dropped anything: a's chain state is b's
        a.modem_out_release(4)
        assert a.modem_out_dropped() == 2 and all_differ(want)
        for buf in bufs:
            buf.free()
    finally:
        a.close(); b.close()


def test_one_channel_squelch(gpu_lib):
    """a one-channel receiver's closed call (the read-back gate) still gives its block, with 0 samples, 0 super-frames and no flags
    (tests/test_audio_out_gpu.py::test_one_channel_squelch); the open calls equal a twin's that never closed -- nothing behind the gate moved"""
    import pebblesdr_amd as P
    K = 5
    fc = 100e3
    a, b = (MC.usb_bank(P, 1, 4096, 1, (0,), centres=[fc]) for _ in range(2))
    x = MC.usb_stream(1, K, 4, centres=[fc])
    try:
        a.modem_out_open(MC.F32, None, 8)
        b.modem_out_open(MC.F32, None, 8)
        for k in range(K):
            if k in (2, 4):
                a.set_squelch(0, 50.0 if k == 2 else -120.0)
            a.process(x[k * TC.SF:(k + 1) * TC.SF])
            if k not in (2, 3):
                b.process(x[k * TC.SF:(k + 1) * TC.SF])   # the noise filter of `a` slept through calls 2 and 3; b's band-pass did not see them
        got, ref = MC.drain(a, K), MC.drain(b, 3)
        assert [g[0] for g in got] == list(range(K)) and all(g[1] == 0 for g in got)
        assert [g[2].shape[1] for g in got] == [TC.SPF, TC.SPF, 0, 0, TC.SPF]
        assert [g[3].shape for g in got] == [(1, 1), (1, 1), (1, 0), (1, 0), (1, 1)]
        assert all(g[3].all() and g[2].any() for g in got if g[2].shape[1])
        assert np.array_equal(got[0][2], ref[0][2]) and np.array_equal(got[1][2], ref[1][2]) and all_differ([got[0][2], got[1][2], got[4][2]])
    finally:
        a.close(); b.close()


def test_refusals_leave_the_handle_usable(gpu_lib):
    import pebblesdr_amd as P
    a, b = MC.usb_bank(P, 2, 4096, 1), MC.usb_bank(P, 2, 4096, 1)
    w = P.ReceiverBank(2048000, 1, True, True, 0)
    x = MC.usb_stream(2, 3, 5)
    try:
        refused(P, MC.E_UNSUPPORTED, w.modem_out_open, MC.F32, None, 4)      # the hook is on the narrow branch
        refused(P, MC.E_INVALID, a.modem_out_open, MC.S16_MONO, None, 4)     # I, Q pairs only
        refused(P, MC.E_INVALID, a.modem_out_open, 3, None, 4)
        refused(P, MC.E_INVALID, a.modem_out_open, MC.F32, [2], 4)           # out of range
        refused(P, MC.E_INVALID, a.modem_out_open, MC.F32, [1, 1], 4)        # duplicated
        refused(P, MC.E_INVALID, a.modem_out_open, MC.F32, [], 4)            # empty
        refused(P, MC.E_INVALID, a.modem_out_open, MC.F32, None, 1)
        refused(P, MC.E_INVALID, a.modem_out_open, MC.F32, None, 9)
        refused(P, MC.E_INVALID, a.modem_out_next, False)                    # not open
        refused(P, MC.E_INVALID, a.modem_out_close)
        refused(P, MC.E_INVALID, a.modem_out_dropped)
        a.modem_out_open(MC.F32, [1], 4)
        refused(P, MC.E_INVALID, a.modem_out_open, MC.F32, None, 4)          # second open
        assert a.modem_out_next(False) is None and a.modem_out_next(True) is None   # nothing queued: host == NULL
        refused(P, MC.E_INVALID, a.modem_out_release, 0)                     # nothing handed out
        a0, b0 = a.process(x[:TC.SF])[0], b.process(x[:TC.SF])[0]
        a1, b1 = a.process(x[TC.SF:2 * TC.SF])[0], b.process(x[TC.SF:2 * TC.SF])[0]
        refused(P, MC.E_INVALID, a.modem_out_release, 0)                     # queued, but not handed out yet
        blk0, blk1 = a.modem_out_next(True), a.modem_out_next(False)         # (a.process has synchronised: the copy is over)
        assert (blk0[0], blk0[1], blk1[0], blk1[1]) == (0, 0, 1, 0)
        refused(P, MC.E_INVALID, a.modem_out_release, 1)                     # out of order
        a.modem_out_release(0)
        refused(P, MC.E_INVALID, a.modem_out_release, 0)
        a.modem_out_release(1)
        # USB without a noise filter or an AGC: the modem hook's row is the audio row
        assert np.array_equal(MC.as_complex(blk0[2])[0], b0[1]) and np.array_equal(MC.as_complex(blk1[2])[0], b1[1])
        assert np.array_equal(a0, b0) and np.array_equal(a1, b1) and a0.any() and not np.array_equal(a0, a1)
        a.modem_out_close()
        refused(P, MC.E_INVALID, a.modem_out_close)
        a2, b2 = a.process(x[2 * TC.SF:])[0], b.process(x[2 * TC.SF:])[0]    # the existing read path, as before
        assert np.array_equal(a2, b2) and a2.any()
    finally:
        for rx in (a, b, w):
            rx.close()


def test_process_iq_is_refused_while_the_ring_is_open(gpu_lib):
    import pebblesdr_amd as P
    a = MC.usb_bank(P, 1, 4096, 1, centres=[100e3])
    try:
        frame = MC.usb_stream(1, 1, 6, centres=[100e3])[:TC.FRAME].astype(np.complex128)
        a.modem_out_open(MC.F32, None, 2)
        refused(P, MC.E_UNSUPPORTED, a.process_iq, frame)
        a.modem_out_close()
        assert len(a.process_iq(frame)[0]) == 0   # accepted again
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------
# 5. the shards of a multibank: their borrowed handles
# ------------------------------------------------------------------------------------------------
def test_multibank_shards(gpu_lib):
    import pebblesdr_amd as P
    C, sizes = 5, [1, 2, 1]
    mb = P.MultiBank(TC.FS, C, [0, 0], frames_per_buffer=TC.FRAME, max_superframes=2)
    one = MC.usb_bank(P, C, 0, 2, (1, 3))
    x = MC.usb_stream(C, sum(sizes), 12)
    fcs = MC.usb_centres(C)
    bufs = []
    try:
        assert mb.n_shards == 2 and sorted(cnt for _, cnt in mb.ranges) == [2, 3]
        for g, (first, count) in enumerate(mb.ranges):
            s = mb.shard(g)
            for c in range(count):
                s.set_mode(c, P.DM_USB); s.set_mixer(c, fcs[first + c]); s.set_bandpass(c, 300, 3000)
                if first + c in (1, 3):
                    s.set_noise_filter(c, True)
            s.modem_out_open(MC.F32, None, 4)
        one.modem_out_open(MC.F32, None, 4)
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
                assert (call, dropped, rate) == (k, 0, TC.RATE) and rows.shape[0] == count and present.shape == (count, sizes[k]) and present.all()
                assert np.array_equal(rows, want[k][2][first:first + count]), (g, k)
        assert all_differ([w[2] for w in want]) and all(w[2][r].any() for w in want for r in range(C))
        for g in range(mb.n_shards):
            mb.shard(g).modem_out_close()
    finally:
        for bf in bufs:
            bf.free()
        mb.close(); one.close()


# ------------------------------------------------------------------------------------------------
# 6. the C++ feeder and the plain-C host
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_the_cpp_feeder(gpu_lib, tmp_path, fmt):
    """pebblegpu::feedModemBlock on a three-channel bank (one channel behind a threshold nothing reaches, one in dmNONE during the second
    call): one callback per demodulator frame of every present (row, super-frame), in order, with the block's own samples"""
    lib, src, exe = os.path.join(ROOT, "pebblesdr_amd"), tmp_path / "feeder.cpp", str(tmp_path / "feeder")
    src.write_text(MC.FEEDER_CPP)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lpebblegpu", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe, fmt], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    per_pair = TC.SPF // MC.DEMOD_FRAME
    # call 0: channels 0 and 2 present in both super-frames; call 1: channel 0 alone.  Channel 1 never
    assert r.stdout.split() == ["callbacks", str(6 * per_pair), "expected", str(6 * per_pair), "absent", "6", "mismatches", "0", "order", "0"], r.stdout


def test_the_c_host(gpu_lib, tmp_path):
    """examples/modem_out_host.c: a reader thread counts zero crossings per channel, no synchronize in either loop.  Channel 3 hears a tone
    1 kHz above its centre: 2000 crossings per second of present samples; channel 5 is in dmNONE: every pair absent, nothing counted"""
    src, exe = os.path.join(ROOT, "examples", "modem_out_host.c"), str(tmp_path / "modem_out_host")
    lib = os.path.join(ROOT, "pebblesdr_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lpebblegpu", "-Wl,-rpath," + lib, "-lm", "-lpthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith("channel 3:") and lines[1].startswith("channel 5:"), r.stdout
    w3, w5 = lines[0].split(), lines[1].split()
    cross, n, rate, absent3 = int(w3[2]), int(w3[5]), int(w3[8]), int(w3[10])
    assert rate == 64000 and n == 12 * 2 * 2048 and absent3 == 0
    # the 1025-tap band-pass fills over the stream's first 1024 demodulator samples, 16 ms: 32 crossings of the tone at most are in doubt;
    # one more for the counter's start at 0
    assert abs(cross - 2 * 1000.0 * n / rate) <= 33, (cross, n, rate)
    assert (int(w5[2]), int(w5[5]), int(w5[10])) == (0, 0, 24)
