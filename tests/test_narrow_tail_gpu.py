"""GPU tier of the narrow-bank tail table (tests/tail_cases.py): channel lists, mode changes and the squelch gate of k_anf, k_agc, k_iir_scan<2,1>,
k_fir_dec, k_save_tail, k_pll_demod, k_gate_eval, k_gate_zero and the deferred refresh in k_save_tails, through P.ReceiverBank against one
oracle Receiver per channel -- which tests/test_narrow_tail_host.py shows to be the chain of its own parts, and on whose rows it shows every
wrong model (a stale AM refresh, state advanced through what a channel sits out, another channel's state blocks, a shifted gate row, a closed
super-frame let through) to miss these bars by a factor of 100 or more.

Bars, per chunk of 512 consecutive outputs of every call (tests/test_parity_gpu.py's own): TOL (1e-5); TOL_AGC_STARTUP (5e-5) behind a running
AGC; SAM in the (re + im) / 2 form at 1e-4; a channel behind the noise filter against oracle.Anf (and the oracle's AGC and demodulator behind
it) run on the band-passed row of a twin bank, identical input, at 1e-6 (5e-5 with an AGC behind it).  Output shapes are exact; a super-frame
the oracle does not deliver is exact zeros, one it delivers is not.  Where the stream starts the band-pass fills at its fp32 floor: in the stream's first
super-frame chunk 0 of an AM channel, and chunk 1 behind a running AGC, is joined to the chunk behind it (a chunk of 1024), every other chunk
is one of 512; an FMN channel's first super-frame is not compared (tests/test_parity_gpu.py::test_bank_with_every_narrow_demod_mode), and chunk 0
of its second is held to tail_cases.TOL_NFM_WRAP (the transient of Demod_NFM's phase wrap behind that acquisition).  tail_cases.compared_chunks
and chunk_bar state the rule; the CPU tier holds it, for every channel, to what the oracle itself does under that floor: it loses the bar on each
chunk that is joined and holds it on each that is compared.  Every test counts the chunks it compared and the outputs they cover, and holds
both to the row's script: nothing a channel delivers is left out but that one super-frame per FMN channel.
Measured figures: DESIGN.md, "Narrow bank tail: channel lists, mode changes and the gate"."""
import numpy as np
import pytest

from tests import tail_cases as TC
from tests.demod_cases import E_SIZE   # PEBBLEGPU_E_SIZE (the binding exports no names for the codes)
from tests.test_parity_gpu import TOL, TOL_AGC_STARTUP

pytestmark = pytest.mark.gpu


def _bank(P, row, bins=None, twin=False, squelch=True, audio_rate=None):
    """the row's bank.  twin: its channels behind the noise filter deliver their band-passed rows instead (USB, filter and AGC off)"""
    rx = P.ReceiverBank(TC.FS, len(row.chans), True, False, row.bins if bins is None else bins, max_superframes=row.max_sf,
                        audio_rate=row.audio_rate if audio_rate is None else audio_rate)
    assert rx.superframe == TC.SF and int(rx.info.demod_rate_int) == TC.RATE and rx.D == TC.D
    for c, ch in enumerate(row.chans):
        via = twin and ch.anf
        rx.set_mode(c, TC.MODE["USB" if via else ch.modes[0]]); rx.set_mixer(c, ch.fc); rx.set_bandpass(c, *ch.band)
        if not via:
            if ch.agc is not None:
                rx.set_agc(c, *ch.agc)
            if ch.anf:
                rx.set_noise_filter(c, True)
        if ch.squelch is not None and squelch:
            rx.set_squelch(c, ch.squelch)
    return rx


def _run(rx, row, twin=False, squelch=True):
    """the row's calls with its mode changes and setters -> [call] audio [C, n]"""
    x, out = TC.row_input(row.name), []
    for k, (s0, ns) in enumerate(TC.call_offsets(row)):
        for c, ch in enumerate(row.chans):
            if k and ch.modes[k] != ch.modes[k - 1] and not (twin and ch.anf):
                rx.set_mode(c, TC.MODE[ch.modes[k]])
            for what, args in TC.actions_before(row, k, c):
                if what == "bandpass":
                    rx.set_bandpass(c, *args)
                elif what == "squelch" and squelch:
                    rx.set_squelch(c, *args)
        out.append(rx.process(x[s0 * TC.SF:(s0 + ns) * TC.SF])[0])
    rx.close()
    return out


def _compare(O, row, got, twin_got=None, channels=None, label=""):
    """every channel against its oracle, per chunk; prints the worst chunk per bar, then asserts"""
    channels = range(len(row.chans)) if channels is None else channels
    figs, closed, delivered, covered = [], 0, 0, 0   # (rel-RMS / bar, rel-RMS, bar, channel, call, super-frame, chunk)
    for c in channels:
        ch = row.chans[c]
        via = TC.via_twin(row, c)
        want = TC.cached_rows(O, row.name, c)
        assert TC.opened_of(want) == TC.script_opened(row, c)
        ref = want
        if via:
            bp = [[twin_got[k][c][j * TC.SPF:(j + 1) * TC.SPF].astype(np.complex128) for j in range(ns)] for k, (_, ns) in enumerate(TC.call_offsets(row))]
            ref = TC.compose(O, row, c, bp, TC.opened_of(want))
        bar, sam = TC.chan_bar(row, c, via_twin=via)
        assert bar in (TOL, TOL_AGC_STARTUP, TC.TOL_SAM, TC.TOL_ANF)
        for k, (s0, ns) in enumerate(TC.call_offsets(row)):
            assert got[k].shape == (len(row.chans), ns * TC.SPF)
            for j in range(ns):
                g = got[k][c][j * TC.SPF:(j + 1) * TC.SPF]
                if len(want[k][j]) == 0:
                    assert not g.any(), "channel %d call %d super-frame %d: the oracle delivers nothing here" % (c, k, j)
                    closed += 1
                    continue
                assert g.any(), "channel %d call %d super-frame %d reads zero" % (c, k, j)
                bounds = TC.compared_chunks(row, c, k, j)
                for (lo, hi), e in zip(bounds, TC.chunk_figures(g, ref[k][j], sam, bounds)):
                    b = TC.chunk_bar(row, c, k, j, lo)
                    assert b == bar or (b == TC.TOL_NFM_WRAP and lo == 0 and ch.modes[k] == "FMN")
                    figs.append((e / b, e, b, c, k, j, lo // TC.CHUNK))
                    covered += hi - lo
                delivered += TC.SPF
    for bar in sorted({f[2] for f in figs}):
        r, e, _, c, k, j, i = max(f for f in figs if f[2] == bar)
        print("%s%s: bar %.0e: worst of %d chunks %.3e (channel %d %s, call %d super-frame %d chunk %d)"
              % (row.name, label, bar, sum(f[2] == bar for f in figs), e, c, row.chans[c].modes[k], k, j, i))
    first = [f for f in figs if (f[4], f[5]) == (0, 0)]
    if first:
        r, e, b, c, k, j, i = max(first)
        print("%s%s: the stream's first super-frame: worst of %d chunks %.3e = %.2f bars of %.0e (channel %d %s, chunk %d)"
              % (row.name, label, len(first), e, r, b, c, row.chans[c].modes[0], i))
    n, skipped = TC.expected_chunks(row, channels)
    fmn_first = sum(row.chans[c].modes[0] == "FMN" and TC.script_opened(row, c)[0][0] for c in channels)
    # every output a channel delivers lies in a compared chunk, but the stream's first super-frame of an FMN channel open there
    assert delivered - covered == skipped == fmn_first * TC.SPF
    assert len(figs) == n, (len(figs), n)
    assert closed == sum(not op for c in channels for call in TC.script_opened(row, c) for op in call)
    bad = sorted(f for f in figs if not f[0] <= 1.0)
    for r, e, b, c, k, j, i in bad[-40:]:
        print("   over the bar: channel %d (%s) call %d super-frame %d chunk %d: %.3e = %.1f bars of %.0e" % (c, row.chans[c].modes[k], k, j, i, e, r, b))
    assert not bad, "%d chunks over their bar" % len(bad)
    return len(figs)


def test_mode_tables_agree(gpu_lib):
    import pebblesdr_amd as P
    assert TC.MODE == {"AM": P.DM_AM, "SAM": P.DM_SAM, "FMN": P.DM_FMN, "USB": P.DM_USB, "NONE": P.DM_NONE}


# ------------------------------------------------------------------------------------------------
# row 1: mode changes and list rebuilds, on the three routes of a call
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["two-stage", "single-stream", "side-by-side"])
def test_mode_changes_and_list_rebuilds(gpu_lib, oracle_mod, monkeypatch, route):
    """Six channels over calls of 2, 1, 3, 1, 2 and 1 super-frames: AM -> USB -> USB -> AM without a set_bandpass after the return (the AM FIR's
    delay line must still hold the end of the 2-super-frame call: the deferred refresh of a two-stage call touches the AM list's rows only), its
    twin with the set_bandpass (delay line cleared), AM throughout, SAM / AM / FMN, FMN / NONE / USB, and USB behind the noise filter and an
    AGC.  two-stage: the default route of a bank without a display transform; single-stream: PEBBLEGPU_BANK_PIPELINE=0; side-by-side: a bank
    created with spectrum_bins.  Channel 3's first call is two super-frames long with the FMN acquisition in the first: chunks 1-3 of the second hold
    TOL only if k_pll_demod wraps its phase at the end of every 2048-sample block as Demod_NFM does (once per call: about 2 bars there, CPU tier)."""
    import pebblesdr_amd as P
    row = TC.ROWS["modes"]
    bins = 4096 if route == "side-by-side" else 0
    if route == "single-stream":
        monkeypatch.setenv("PEBBLEGPU_BANK_PIPELINE", "0")
    rx, tw = _bank(P, row, bins), _bank(P, row, bins, twin=True)
    if route == "single-stream":
        monkeypatch.delenv("PEBBLEGPU_BANK_PIPELINE")
    got, twin_got = _run(rx, row), _run(tw, row, twin=True)
    n = _compare(oracle_mod, row, got, twin_got, label=" (%s)" % route)
    # ten super-frames of four chunks; the three AM channels: chunk 0 of the stream's first joins chunk 1 (three there); SAM and the channel
    # behind the noise filter: all four; channel 3: its first super-frame in FMN not compared, nothing in its tune-only call, eight of four
    assert n == 3 * (3 + 9 * 4) + 2 * (10 * 4) + 8 * 4 == 229


# ------------------------------------------------------------------------------------------------
# row 2: more than 64 listed channels
# ------------------------------------------------------------------------------------------------
def test_lists_of_more_than_64_channels(gpu_lib, oracle_mod):
    """200 channels, FMN / SAM / AM by c % 3 (67 / 67 / 66 entries: k_pll_demod's second, ragged workgroup in both PLL modes), an AGC on the 160
    with c % 5 != 0 (k_agc's three workgroups, the last ragged; FAST / MED / SLOW and two on manual gain), every channel against its own
    oracle Receiver; neighbours in every list and the same lane of the next workgroup listen to different carriers"""
    import pebblesdr_amd as P
    row = TC.ROWS["lists"]
    got = _run(_bank(P, row), row)
    n = _compare(oracle_mod, row, got)
    # 67 FMN channels: three super-frames of four behind the first; the 133 others: four super-frames of four, less the one joined chunk of
    # the first -- AM, or behind a running AGC -- which leaves out the 14 SAM channels without one (c % 15 == 10, and channel 7 on manual gain)
    assert n == 67 * (3 * 4) + 133 * (4 * 4) - (133 - 14) == 2813


# ------------------------------------------------------------------------------------------------
# row 3: k_anf's list
# ------------------------------------------------------------------------------------------------
def test_noise_filter_list_with_a_muted_entry(gpu_lib, oracle_mod):
    """six USB channels, the noise filter on 1, 3 and 4; channel 3 is tune-only during the middle call and its filter sleeps through it.  The
    filtered channels against oracle.Anf on a twin bank's rows (identical input) at 1e-6, the others against the oracle chain"""
    import pebblesdr_amd as P
    row = TC.ROWS["anf-list"]
    got, twin_got = _run(_bank(P, row), row), _run(_bank(P, row, twin=True), row, twin=True)
    assert {TC.chan_bar(row, c, True)[0] for c in (1, 3, 4)} == {TC.TOL_ANF}
    n = _compare(oracle_mod, row, got, twin_got)
    assert n == 6 * (4 * 4) - 2 * 4   # USB channels: every chunk of 512, the stream's first included; channel 3's tune-only call has two super-frames


# ------------------------------------------------------------------------------------------------
# row 4: every tail kernel under a Gate
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gate", "gate-thr", "gate-one"])
def test_every_tail_kernel_under_a_gate(gpu_lib, oracle_mod, name):
    """gate: AM + AGC SLOW, AM + AGC FAST + noise filter, SAM, FMN, USB + noise filter + AGC MED and a USB channel that never gates, each
    carrier keyed between 0.1 and 0.001 per super-frame in its own pattern, calls of 3, 1, 2 and 2 super-frames; FMN and SAM are compared from
    the first sample of a reopened super-frame.  gate-thr: the carriers stay up and set_squelch(c, 50) between calls closes the gate.
    gate-one: the keyed script on a one-channel handle created for three super-frames per call (AM + AGC FAST)"""
    import pebblesdr_amd as P
    row = TC.ROWS[name]
    got = _run(_bank(P, row), row)
    twin_got = _run(_bank(P, row, twin=True), row, twin=True) if any(ch.anf for ch in row.chans) else None
    n = _compare(oracle_mod, row, got, twin_got)
    opened = sum(op for c in range(len(row.chans)) for call in TC.script_opened(row, c) for op in call)
    assert opened == {"gate": sum(sum(k) for k in TC.GATE_KEYS) + 8, "gate-thr": 5 * 8 - (1 + 2 + 1 + 2 + 1) + 8, "gate-one": 5}[name]
    # four chunks per delivered super-frame; channel 0 (AM behind a running AGC, compared with the oracle chain) is open at the start of every
    # row: one joined chunk; gate-thr's FMN channel is open from the start as well: its first super-frame is not compared
    assert n == 4 * opened - 1 - 4 * int(name == "gate-thr") == {"gate": 115, "gate-thr": 159, "gate-one": 19}[name]


def test_gated_calls_with_an_audio_rate(gpu_lib, oracle_mod):
    """The gate row with audio_rate = 11025: the resampler sees the silence of a closed stretch (include/pebblegpu.h, pebblegpu_set_squelch).
    The output count of every call equals that of a twin bank whose thresholds are all -120; the never-gated channel meets the oracle at the bar
    per 256 outputs (k_resample's block); and every closed stretch reads exactly zero from 28 resampler inputs past its start until it ends
    (fractresampler.cpp: the output at time T reads the inputs floor(T) - 27 .. floor(T))"""
    import pebblesdr_amd as P
    row = TC.ROWS["gate-11025"]
    got, open_got = _run(_bank(P, row), row), _run(_bank(P, row, squelch=False), row, squelch=False)
    counts = [g.shape[1] for g in got]
    assert counts == [g.shape[1] for g in open_got]
    want = TC.cached_rows(oracle_mod, row.name, 5)
    assert counts == [sum(len(a) for a in call) for call in want]
    dt = float(TC.RATE) / row.audio_rate
    assert abs(sum(counts) - sum(row.calls) * TC.SPF / dt) <= 1
    errs = []
    for k, call in enumerate(want):
        r = np.concatenate(call)
        errs += [(TC.rel_rms(got[k][5][lo:hi], r[lo:hi]), k, i) for i, (lo, hi) in enumerate(TC.chunk_bounds(len(r), 256))]
    e, k, i = max(errs)
    print("gate-11025: never-gated channel, worst of %d chunks of 256 outputs %.3e (call %d chunk %d); outputs per call %s" % (len(errs), e, k, i, counts))
    assert e <= TOL
    audio = np.concatenate(got, axis=1)
    T = np.arange(audio.shape[1]) * dt   # output m is taken at input time m dt of the stream (every super-frame hands the resampler 2048 inputs)
    zeros = 0
    for c in range(5):
        key = TC.GATE_KEYS[c]
        j = 0
        while j < len(key):
            if key[j]:
                j += 1
                continue
            j1 = j
            while j1 < len(key) and not key[j1]:
                j1 += 1
            a, b = j * TC.SPF, j1 * TC.SPF   # the stretch in resampler inputs
            m = (T >= a + TC.RS_PERIODS) & (T < b - 1e-6)
            assert m.sum() >= (b - a - TC.RS_PERIODS) / dt - 2
            assert not audio[c][m].any(), "channel %d, closed super-frames %d..%d" % (c, j, j1 - 1)
            zeros += int(m.sum())
            j = j1
        for j in range(len(key)):   # and an open super-frame is not silent
            if key[j]:
                assert audio[c][(T >= j * TC.SPF + 1024) & (T < (j + 1) * TC.SPF)].any()
    print("gate-11025: %d outputs inside closed stretches read exactly zero" % zeros)


# ------------------------------------------------------------------------------------------------
# PllCore::run refuses what k_save_tail cannot take
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["FMN", "SAM"])
def test_pll_demodulators_refuse_calls_shorter_than_their_history(gpu_lib, oracle_mod, mode):
    """k_save_tail copies tmp[n - 80 .. n): a call of 79 samples is refused with the size code before any kernel launch, as AmCore::run refuses
    it, and leaves the stream where it was, bit for bit, against a handle that never saw it; 80 samples are taken"""
    import pebblesdr_amd as P
    n = 2048
    t = np.arange(3 * n) / float(TC.RATE)
    if mode == "FMN":
        x = 0.3 * np.exp(1j * 3.0 * np.sin(2 * np.pi * 1000 * t)) + TC.lcg_noise(3 * n, 7, 1e-4)
        ref, bar = oracle_mod.DemodNFM(TC.RATE), TOL
    else:
        x = (0.3 * (1 + 0.5 * np.cos(2 * np.pi * 800 * t))) * np.exp(2j * np.pi * 30 * t) + TC.lcg_noise(3 * n, 8, 1e-4)
        ref, bar = oracle_mod.DemodSAM(TC.RATE), TC.TOL_SAM
    d, twin = P.Demod(TC.RATE, 256000, n), P.Demod(TC.RATE, 256000, n)
    at = 0
    for ln in (n, 79, TC.K_MAX_TAPS, 79, n):
        if ln < TC.K_MAX_TAPS:
            with pytest.raises(P.PebbleGpuError) as e:
                d.processBlock(x[at:at + ln])
            assert e.value.code == E_SIZE
            continue
        if at == 0:
            d.setDemodMode(TC.MODE[mode]); twin.setDemodMode(TC.MODE[mode])
        g, w, r = d.processBlock(x[at:at + ln]), twin.processBlock(x[at:at + ln]), ref.process(x[at:at + ln])
        assert g.shape == r.shape == (ln,) and np.array_equal(g, w)
        f = TC.sam_form if mode == "SAM" else (lambda v: v)
        if ln == n:
            assert TC.rel_rms(f(g), f(r)) <= bar
        at += ln
    d.close(); twin.close()
