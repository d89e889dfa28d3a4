"""GPU tier of the receiver frame-size table (tests/frame_cases.py): whole receivers at frames other than 2048 through P.ReceiverBank against
oracle.Receiver(fs, nf, bins, fft, taps) fed frame by frame, every row's calls in one handle; the dmFMS frame rule refused at set_mode with
the handle going on; the short-call WFM history merge once more from raw int8; the CDownConvert step at calls of a few samples.  No
environment switch is set, no kernel is launched directly.  Bars and the rule for where a stream starts: tests/frame_cases.py, which
tests/test_receiver_frames_host.py holds to what the oracle itself does.  Every test prints its worst figure before it asserts."""
import numpy as np
import pytest

from tests import frame_cases as FC
from tests import rds_cases as RC
from tests import tail_cases as TC
from tests.demod_cases import E_SIZE, TOL as WFM_TOL, chunk_errors, rel_rms
from tests.test_parity_gpu import TOL, TOL_AGC_STARTUP

pytestmark = pytest.mark.gpu


def tuples(g):
    return [tuple(int(v) for v in r) for r in g]


# ------------------------------------------------------------------------------------------------
# narrow rows
# ------------------------------------------------------------------------------------------------
def _narrow_bank(P, row):
    rx = P.ReceiverBank(row.fs, len(row.chans), True, False, row.bins, frames_per_buffer=row.nf, fastfir_fft=row.fft, fastfir_taps=row.taps,
                        max_superframes=max(row.calls), audio_rate=row.audio_rate)
    assert rx.superframe == FC.n_superframe(row) and int(rx.info.demod_rate_int) == row.rate and rx.D == row.total
    for c, ch in enumerate(row.chans):
        rx.set_mode(c, FC.MODE[ch.mode]); rx.set_mixer(c, ch.fc); rx.set_bandpass(c, *TC.BAND[ch.mode])
        if ch.agc is not None:
            rx.set_agc(c, *ch.agc)
        if ch.squelch is not None:
            rx.set_squelch(c, ch.squelch)
    return rx


@pytest.mark.parametrize("name", [r.name for r in FC.NARROW])
def test_narrow_receiver_at_this_frame(gpu_lib, oracle_mod, name):
    import pebblesdr_amd as P
    row = FC.NARROW_BY_NAME[name]
    x = FC.n_input(name)
    rx = _narrow_bank(P, row)
    got = [rx.process(x[o:o + n])[0] for o, n in FC.n_calls(row)]
    rx.close()
    spf, figs = FC.n_spf(row), []
    for c, ch in enumerate(row.chans):
        want, opened, _ = FC.n_oracle(oracle_mod, name, c)
        if ch.key is None:
            assert [g.shape for g in got] == [(len(row.chans), len(w)) for w in want], (name, c)   # (behind the resampler: the count of every call)
            gs, ws = np.concatenate([g[c] for g in got]), np.concatenate(want)
            assert np.abs(ws).max() > 1e-3
            figs += [(rel_rms(FC.form(ch, gs[lo:hi]), FC.form(ch, ws[lo:hi])) / bar, bar, c, lo) for lo, hi, bar in FC.stream_chunks(row, c, len(ws))]
            continue
        # behind the keyed squelch: a super-frame the oracle does not deliver reads exactly zero, the others per chunk of 512
        assert not row.audio_rate
        bar, at_w = FC.n_bar(ch), 0
        for k, (g, w, op) in enumerate(zip(got, want, opened)):
            assert g.shape == (len(row.chans), len(op) * spf) and len(w) == sum(op) * spf
            at = 0
            for j, o in enumerate(op):
                seg = g[c][j * spf:(j + 1) * spf]
                if not o:
                    assert not seg.any(), "call %d super-frame %d: the oracle delivers nothing here" % (k, j)
                    continue
                assert seg.any()
                ref = w[at:at + spf]; at += spf
                figs += [(rel_rms(seg[lo:hi], ref[lo:hi]) / bar, bar, c, at_w + lo) for lo, hi in FC.chunk_bounds(spf, FC.CHUNK)]
            at_w += len(op) * spf
    for bar in sorted({f[1] for f in figs}):
        r, _, c, lo = max(f for f in figs if f[1] == bar)
        print("%s: bar %.0e: worst of %d chunks %.3e = %.2f bars (channel %d %s, outputs from %d)"
              % (name, bar, sum(f[1] == bar for f in figs), r * bar, r, c, row.chans[c].mode, lo))
    assert {f[1] for f in figs} <= {TOL, TOL_AGC_STARTUP, TC.TOL_SAM, TC.TOL_NFM_WRAP}
    bad = sorted(f for f in figs if not f[0] <= 1.0)
    for r, bar, c, lo in bad[-20:]:
        print("   over the bar: channel %d (%s) outputs from %d: %.3e = %.1f bars of %.0e" % (c, row.chans[c].mode, lo, r * bar, r, bar))
    assert not bad, "%d chunks over their bar" % len(bad)


# ------------------------------------------------------------------------------------------------
# WFM rows
# ------------------------------------------------------------------------------------------------
WFM = {r.name: r for r in FC.wfm_rows()}


def _wfm_bank(P, row):
    rx = P.ReceiverBank(row.fs, len(row.chans), FC.w_shared(row), True, 0, frames_per_buffer=row.nf, max_superframes=max(row.calls))
    assert rx.superframe == row.total * row.nf and rx.D == row.total
    for c, (mode, _) in enumerate(row.chans):
        rx.set_mode(c, FC.MODE[mode]); rx.set_mixer(c, row.fc)
    return rx


@pytest.mark.parametrize("name", ["w-256", "w-600", "w-65535", "w-dec-512"])
def test_wfm_mono_receiver_at_this_frame(gpu_lib, oracle_mod, name):
    """every channel its own stream and signal; per chunk of 1024 outputs of every call, the first included"""
    import pebblesdr_amd as P
    row = WFM[name]
    x, calls = FC.w_input(name)
    rx = _wfm_bank(P, row)
    got = [rx.process(x[:, o:o + n])[0] for o, n in calls]
    rx.close()
    errs = []
    for c in range(len(row.chans)):
        want = FC.w_oracle(oracle_mod, name, c)[0]
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == (len(row.chans), len(w)) and len(w) == calls[k][1] // row.total
            errs += [(e, c, k, j) for j, e in enumerate(chunk_errors(g[c], w, FC.WFM_CHUNK))]
    for a in range(len(row.chans)):
        for b in range(a + 1, len(row.chans)):
            assert rel_rms(got[-1][a], got[-1][b]) > 1e-2, "the channels carry different content"
    e, c, k, j = max(errs)
    print("%s: worst rel-RMS over %d chunks %.3e, channel %d call %d chunk %d" % (name, len(errs), e, c, k, j))
    assert e <= WFM_TOL


@pytest.mark.parametrize("name", ["w-1024-fms", "w-384k-fms"])
def test_wfm_stereo_receiver_at_this_frame(gpu_lib, oracle_mod, name):
    """dmFMS (and a dmFMM channel beside it) on a broadcast multiplex: the audio of every call, the RDS groups with their `changed` flags as
    Demod::fmStereo polls them once per frame, read every few calls, and the pilot's lock flag after every call"""
    import pebblesdr_amd as P
    row = WFM[name]
    x, calls = FC.w_input(name)
    rx = _wfm_bank(P, row)
    locks = FC.w_locks(oracle_mod, name)
    got, got_g, got_c = [], [], []
    for k, (o, n) in enumerate(calls):
        got.append(rx.process(x[0, o:o + n])[0])
        assert rx.stereo_lock(0)[0] == locks[k], k
        if k % 7 == 6:
            g, ch = rx.rds_groups(0)
            got_g += tuples(g); got_c += list(ch)
    g, ch = rx.rds_groups(0)
    got_g += tuples(g); got_c += list(ch)
    rx.close()
    want, (want_g, want_c) = FC.w_oracle(oracle_mod, name, 0)
    assert [len(g[0]) for g in got] == [len(w) for w in want]
    e_l = RC.call_errors([g[0].real for g in got], [w.real for w in want])
    e_r = RC.call_errors([g[0].imag for g in got], [w.imag for w in want])
    print("%s: %d calls, stereo audio worst left %.3e right %.3e; %d groups, lock after the last call %s" % (name, len(calls), max(e_l), max(e_r), len(want_g), locks[-1]))
    assert max(e_l) <= RC.AUDIO_TOL and max(e_r) <= RC.AUDIO_TOL
    assert len(want_g) >= (10 if name == "w-1024-fms" else 4)
    assert got_g == tuples(want_g) and got_c == list(want_c)
    if len(row.chans) > 1:
        assert row.chans[1][0] == "FMM"
        mono = FC.w_oracle(oracle_mod, name, 1)[0]
        errs = [e for g, w in zip(got, mono) for e in chunk_errors(g[1], w, FC.WFM_CHUNK)]
        print("%s: the dmFMM channel beside it, worst of %d chunks %.3e" % (name, len(errs), max(errs)))
        assert max(errs) <= WFM_TOL
        assert rel_rms(got[-1][0], got[-1][1]) > 1e-2


# ------------------------------------------------------------------------------------------------
# refusal rows
# ------------------------------------------------------------------------------------------------
def _fm(fs, n, fc, seed):
    t = np.arange(n) / float(fs)
    return 0.5 * np.exp(1j * (2 * np.pi * fc * t + 40.0 * np.sin(2 * np.pi * 1000 * t))) + TC.lcg_noise(n, seed, 1e-3)


def _names(rx):
    return [rx.kernel_name(k) for k in range(1, 7)]


@pytest.mark.parametrize("fs,nf,reason", FC.REFUSALS, ids=["%d-%d" % (fs, nf) for fs, nf, _ in FC.REFUSALS])
def test_stereo_is_refused_at_set_mode_and_the_handle_goes_on(gpu_lib, fs, nf, reason):
    """set_mode(FMS) fails with the size code and the rule in its text before a call is made and between calls; the channel stays dmFMM,
    kernel names and the input route stay what they were, and the next three calls are bit for bit those of a twin that was never asked"""
    import pebblesdr_amd as P
    rx, twin = [P.ReceiverBank(fs, 1, True, True, 0, frames_per_buffer=nf, max_superframes=2) for _ in range(2)]
    for r in (rx, twin):
        r.set_mixer(0, 20e3)
    sf = rx.superframe
    x = _fm(fs, 5 * sf, 20e3, 3)
    word = {"not a multiple of D": "multiples of", "stage shorter than its taps": "shorter than", "below 2 (T - 1)": "twice"}[reason]
    at = 0
    for k, m in enumerate((1, 2, 1)):
        before = _names(rx)
        with pytest.raises(P.PebbleGpuError) as ei:
            rx.set_mode(0, P.DM_FMS)
        assert ei.value.code == E_SIZE and "dmFMS" in str(ei.value) and word in str(ei.value), str(ei.value)
        assert _names(rx) == before
        g, w = rx.process(x[at:at + m * sf])[0], twin.process(x[at:at + m * sf])[0]
        at += m * sf
        assert g.shape == w.shape == (1, m * sf) and np.abs(w).max() > 1e-3
        assert np.array_equal(g, w), (k, m)
        assert _names(rx) == _names(twin)
    assert len(rx.rds_groups(0)[0]) == 0 and rx.stereo_lock(0)[0] is False
    rx.set_mode(0, P.DM_FMM)   # what it was: accepted
    rx.close(); twin.close()


def test_a_shards_refusal_leaves_the_multibank_usable(gpu_lib):
    """two shards on one device, a frame of 300 at 256 000: the refusal of shard 1's channel does not set the multibank's failed_text"""
    import pebblesdr_amd as P
    fs, nf = FC.REFUSALS[0][:2]
    mb, twin = [P.MultiBank(fs, 2, [0, 0], shared_input=True, wfm=True, frames_per_buffer=nf, max_superframes=2) for _ in range(2)]
    for m in (mb, twin):
        for c in range(2):
            m.set_mixer(c, 20e3 + 5e3 * c)
    sf = mb.superframe
    x = _fm(fs, 4 * sf, 20e3, 4)
    at = 0
    for k, n in enumerate((1, 2, 1)):
        with pytest.raises(P.PebbleGpuError) as ei:
            mb.set_mode(1, P.DM_FMS)
        assert ei.value.code == E_SIZE
        g, w = mb.process(x[at:at + n * sf]), twin.process(x[at:at + n * sf])
        at += n * sf
        assert g.shape == w.shape == (2, n * sf) and np.array_equal(g, w), k
    mb.close(); twin.close()


# ------------------------------------------------------------------------------------------------
# w-256 once more: float2 against raw int8 through process_raw (the staged route's pitches differ)
# ------------------------------------------------------------------------------------------------
def test_short_wfm_calls_from_raw_int8_equal_the_float2_calls(gpu_lib):
    import pebblesdr_amd as P
    from tests import raw_cases as rc
    row = WFM["w-256"]
    x, calls = FC.w_input("w-256")
    raw = np.stack([np.round(x.real * 120), np.round(x.imag * 120)], axis=-1).astype(np.int8)      # [3, n, 2]
    conv = rc.host_convert(raw, 0, 0, rc.GAIN[0])
    a, b = _wfm_bank(P, row), _wfm_bank(P, row)
    for k, (o, n) in enumerate(calls):
        buf = P.DeviceBuffer.from_array(np.ascontiguousarray(raw[:, o:o + n]), 0)
        try:
            a.process_raw_device(buf.ptr, n, 0, 0, rc.GAIN[0])
            ga = a.audio()
        finally:
            buf.free()
        gb = b.process(conv[:, o:o + n])[0]
        assert a.kernel_name(6) == "k_normalize_iq" and b.kernel_name(6) == "float2"
        assert ga.shape == gb.shape == (3, n) and np.abs(gb).max() > 1e-3
        assert np.array_equal(ga, gb), (k, n)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------
# the CDownConvert step with exact history at any length
# ------------------------------------------------------------------------------------------------
def test_downconvert_step_streams_calls_of_a_few_samples(gpu_lib):
    """2 048 000 / 15 000 (11, 11, 15, 19, 31 taps; D = 32) in calls of 32, 64, 96, 40 x 32 and 32 samples -- one to three outputs a call,
    every stage shorter than its taps -- against the plain fp64 streaming model (frame_cases.downconvert_model: the oscillator in closed
    form, every stage a strided FIR over the whole stream), per call by rds_cases.call_errors' measure"""
    import pebblesdr_amd as P
    fs, bw, f0 = FC.DC_STEP[:3]
    x = FC.dc_step_input()
    want = FC.downconvert_model(fs, bw, f0, x)
    dc = P.DownConvert(4096)
    assert dc.SetDataRate(fs, bw) == fs / 32 and dc.stages() == [11, 11, 15, 19, 31]
    dc.SetFrequency(f0)
    got, ref, at = [], [], 0
    for n in FC.dc_step_calls():
        g = dc.ProcessData(x[at:at + n])
        assert g.shape == (n // 32,)
        got.append(g); ref.append(want[at // 32:(at + n) // 32])
        at += n
    assert at == len(x)
    e = RC.call_errors(got, ref)
    print("DownConvert step, %d calls of 32 .. 96 samples: worst call %.3e (call %d)" % (len(e), max(e), int(np.argmax(e))))
    assert np.abs(np.concatenate(ref)).max() > 0.05
    assert max(e) <= TOL
