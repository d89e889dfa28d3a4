"""GPU tier of the demodulator-rate table (tests/demod_cases.py): both paths of WfmCore, the AM scan at ragged call lengths, k_fir_dec's
per-channel tap counts and channel lists, and the resampler at six ratios, through P.Demod and P.ReceiverBank against the CPU oracle
-- which tests/test_demod_geometry_host.py holds to the plain fp64 chains at exactly these rows and call lengths.

Bar: rel-RMS <= 1e-5 (BASELINE.json north_star) on every chunk of every call, the first included: 512 consecutive outputs (kSub) on
the scan and sequential rows, 1024 (kWfmOutB) on the one-kernel rows, 256 on the resampler rows, a 2048-sample frame in the AM bank;
output counts equal the oracle's exactly.  Every test prints its worst chunk and which one it was.  The only lengths not compared are
the refused ones (79 samples: AmCore::run and WfmCore::run return the size code before any kernel launch; only the upload into the
handle's scratch input buffer has been queued), and every one of those is asserted to be refused and to leave the stream where it
was, bit for bit, against a second handle that never saw it."""
import numpy as np
import pytest

from tests import demod_cases as DC

pytestmark = pytest.mark.gpu

TOL = DC.TOL


def _row(rows, name):
    return {r.name: r for r in rows}[name]


def _run_step(P, make, script, x, ref_call, chunk, before_call=None):
    """script through two handles: `d` is also asked for the refused lengths, `twin` never is.  -> [(call, chunk, rel-RMS)]"""
    d, twin = make(), make()
    errs, at, k = [], 0, 0
    for n in script:
        if n < DC.MIN_CALL:
            with pytest.raises(P.PebbleGpuError) as e:
                d.processBlock(x[at:at + n])
            assert e.value.code == DC.E_SIZE
            continue
        if before_call:
            before_call(k, d, twin)
        fr = x[at:at + n]
        g, t, r = d.processBlock(fr), twin.processBlock(fr), ref_call(k, fr)
        assert g.shape == r.shape == (n,)
        assert np.array_equal(g, t), "call %d (%d samples): the handle that was refused a call differs from the one that was not" % (k, n)
        errs += [(k, c, e) for c, e in enumerate(DC.chunk_errors(g, r, chunk))]
        at += n
        k += 1
    assert at == len(x)
    d.close(); twin.close()
    return errs


# ------------------------------------------------------------------------------------------------
# WFM mono: P.Demod(64000, rate, cap) in DM_FMM against oracle.DemodWFM
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in DC.WFM_ROWS])
def test_wfm_mono_step_on_both_paths(gpu_lib, oracle_mod, name):
    """One-kernel rows (k_wfm_fir; 100 000 and 125 000 with Llp == 1): calls of 80, 81, Lx-1, Lx-1, Lx, Lx+1, 1023, 80, 1024, ... --
    short after short, short after long, long after short, the history merged into either `d_xtail` buffer.  Sequential rows
    (150 000, 192 000, 1 000 000: k_iir_scan<0,1>, k_discrim reading a[-1], k_fir_dec, k_iir_scan<1,2>, head-room refreshed by
    k_save_tails): the same lengths with Lx = 80, ragged last sub-chunks of 1, 7, 8, 9 and 511 samples.
    Measured worst chunk on the MI355X: see DESIGN.md, "Demodulator-rate kernels: paths and call geometry"."""
    import pebblesdr_amd as P
    row = _row(DC.WFM_ROWS, name)
    script, x = DC.wfm_script(row), DC.wfm_input(row)
    ref = oracle_mod.DemodWFM(row.rate)

    def make():
        d = P.Demod(64000, row.rate, max(script))
        d.setDemodMode(P.DM_FMM)
        return d

    errs = _run_step(P, make, script, x, lambda k, fr: ref.process(fr), row.chunk)
    e, c, k = DC.worst_of(errs)
    print("%s (%s): worst rel-RMS over %d chunks %.3e, call %d (%d samples) chunk %d"
          % (name, "one kernel, Lx = %d" % DC.wfm_lx(row) if row.fused else "sequential", len(errs), e, c, DC.valid_calls(script)[c], k))
    assert e <= TOL


# ------------------------------------------------------------------------------------------------
# AM: P.Demod(rate, 256000, cap) in DM_AM against oracle.DemodAM
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in DC.AM_ROWS])
def test_am_step_with_ragged_sub_chunks(gpu_lib, oracle_mod, name):
    """k_iir_scan<2,1> (the 0.9999 DC block), k_fir_dec and k_save_tail over calls of 80, 81, 87, 88, 89, 511, 512, 513, 519, 520, 521,
    1025, 2568 and 80 samples, with one setBandwidth in the middle (other taps, the FIR's delay line cleared)"""
    import pebblesdr_amd as P
    row = _row(DC.AM_ROWS, name)
    script, x = DC.am_script(row), DC.am_input(row)
    ref = oracle_mod.DemodAM(row.rate, DC.AM_BW[0])

    def make():
        d = P.Demod(row.rate, 256000, max(script))
        d.setDemodMode(P.DM_AM)
        d.setBandwidth(DC.AM_BW[0])
        return d

    def before_call(k, d, twin):
        if k == DC.AM_CHANGE_BEFORE:
            ref.set_bandwidth(DC.AM_BW[1]); d.setBandwidth(DC.AM_BW[1]); twin.setBandwidth(DC.AM_BW[1])

    errs = _run_step(P, make, script, x, lambda k, fr: ref.process(fr), row.chunk, before_call)
    e, c, k = DC.worst_of(errs)
    print("%s: worst rel-RMS over %d chunks %.3e, call %d (%d samples) chunk %d" % (name, len(errs), e, c, DC.valid_calls(script)[c], k))
    assert e <= TOL


# ------------------------------------------------------------------------------------------------
# the AM bank: per-channel tap counts and channel lists of k_fir_dec
# ------------------------------------------------------------------------------------------------
def test_am_bank_with_three_tap_counts_and_a_channel_that_leaves_and_returns(gpu_lib, oracle_mod):
    """five channels on one stream: 1, 3 and 4 in AM with 24, 40 and 75 taps, 0 and 2 in USB; six calls of one super-frame; channel 3
    is USB during the fourth and AM again from the fifth, its DC block and FIR history where they were (the idle Demod_AM object).
    Per channel and 2048-sample frame against Mixer -> Decimator -> gain -> FastFIR -> Demod_AM."""
    import pebblesdr_amd as P
    rx = P.ReceiverBank(DC.BANK_FS, DC.BANK_C, True, False, 0, max_superframes=1)
    assert int(rx.info.demod_rate_int) == DC.BANK_RATE
    stages = sum(int(np.log2(st)) for _, st in rx.chain())
    sf = rx.superframe
    pmode = {"AM": P.DM_AM, "USB": P.DM_USB}
    for c, (mode, lo, hi, fc) in enumerate(DC.BANK_CHANNELS):
        rx.set_mode(c, pmode[mode]); rx.set_mixer(c, fc); rx.set_bandpass(c, lo, hi)
    x = DC.bank_input(DC.BANK_CALLS * sf)
    want = DC.bank_oracle(oracle_mod, x, sf, stages)
    errs = []
    for k in range(DC.BANK_CALLS):
        modes = DC.bank_modes(k)
        if modes[DC.BANK_AWAY] != DC.bank_modes(max(k - 1, 0))[DC.BANK_AWAY]:
            rx.set_mode(DC.BANK_AWAY, pmode[modes[DC.BANK_AWAY]])
        g = rx.process(x[k * sf:(k + 1) * sf])[0]
        for c in range(DC.BANK_C):
            assert g[c].shape == want[c][k].shape
            errs += [((c, k), f, e) for f, e in enumerate(DC.chunk_errors(g[c], want[c][k], DC.BANK_FRAME))]
    rx.close()
    e, (c, k), f = DC.worst_of(errs)
    per = [max(e for (cc, _), _, e in errs if cc == c) for c in range(DC.BANK_C)]
    print("AM bank: worst rel-RMS per channel %s; worst frame: channel %d call %d frame %d" % (" ".join("%.3e" % w for w in per), c, k, f))
    assert e <= TOL


# ------------------------------------------------------------------------------------------------
# the resampler
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in DC.RS_ROWS])
def test_resampler_ratios_down_and_up(gpu_lib, oracle_mod, name):
    """k_resample behind a USB channel with manual gain: 8000 (exactly 256 outputs a frame), 8012 (a 256- and a 257-output frame in
    one call: two sub-blocks per frame, one of which leaves at once), 22 050, 44 100, and upsampling to 96 000 from 64 000 and to 48 000 from 37 500 (ResampCore::run and the audio buffer, n / dt + frames + 8 samples a row, take it: sub_blocks
    up to 12); calls of 1, 2 and 1 super-frames; the count of every call is the oracle's, the samples meet the bar per 256 outputs"""
    import pebblesdr_amd as P
    row = _row(DC.RS_ROWS, name)
    rx = P.ReceiverBank(row.fs, 1, True, False, 0, fastfir_fft=2048, fastfir_taps=row.taps, max_superframes=max(DC.RS_CALLS), audio_rate=row.audio_rate)
    assert int(rx.info.demod_rate_int) == row.demod_rate
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, DC.rs_mixer(row)); rx.set_bandpass(0, *DC.RS_BAND); rx.set_agc(0, *DC.RS_AGC)
    want, sf = DC.rs_oracle(oracle_mod, row, row.audio_rate)
    assert rx.superframe == sf
    x, at, errs, counts = DC.rs_input(row, sum(DC.RS_CALLS) * sf), 0, [], []
    for k, n in enumerate(DC.RS_CALLS):
        g = rx.process(x[at:at + n * sf])[0][0]
        r = np.concatenate(want[k])
        assert len(g) == len(r), "call %d: %d outputs, the oracle has %d" % (k, len(g), len(r))
        counts.append(len(g))
        errs += [(k, c, e) for c, e in enumerate(DC.chunk_errors(g, r, DC.RS_CHUNK))]
        at += n * sf
    rx.close()
    e, c, k = DC.worst_of(errs)
    print("%s: outputs per call %s; worst rel-RMS over %d chunks %.3e, call %d chunk %d" % (name, counts, len(errs), e, c, k))
    assert e <= TOL
