"""GPU tier of the general decimator routes (tests/decim_cases.py): every row through P.ReceiverBank with the POST_MIXER tap on -- the
decimated rows behind the gain restore, at full bandwidth, no band-pass and no demodulator in between -- against the oracle's
Mixer -> Decimator fed whole super-frames; the step rows through P.Decimator.  Per call: the kernel names route() predicts, the tap's
shape, rel-RMS <= TOL per 2048-output frame on the channels the plan lists; per run, on EVERY channel: the peak on the bin its tuning
predicts (a lane that received another channel's data shows no tone of its own)."""
import numpy as np
import pytest

from tests import decim_cases as dc
from tests.test_parity_gpu import TOL

pytestmark = pytest.mark.gpu

assert TOL == dc.TOL


@pytest.mark.parametrize("name", [r.name for r in dc.ROWS])
def test_row_at_the_post_mixer_tap(gpu_lib, oracle_mod, name):
    import pebblesdr_amd as P
    from pebblesdr_amd.binding import DeviceBuffer, to_f32_iq
    row = next(r for r in dc.ROWS if r.name == name)
    chain = oracle_mod.Decimator(row.fs, dc.protect_bw(row)).chain()
    p = dc.plan(row, chain)
    want = dc.routes(row, chain)
    rx = P.ReceiverBank(row.fs, row.C, row.shared_input, row.wfm, row.spectrum_bins, max_superframes=max(row.calls))
    try:
        assert rx.chain() == chain and rx.superframe == p.P1
        rx.set_taps([P.TAP_POST_MIXER])
        for c in range(row.C):
            rx.set_mixer(c, p.fc_idx[c] * p.df)
        refs = {c: dc.OracleChannel(oracle_mod, row, p, c, chain) for c in p.compare}
        got = []  # every channel's tap rows, call by call
        worst = (0.0, None)
        for k, sfs in enumerate(row.calls):
            if k == row.retune_before:
                rx.set_mixer(p.retuned, p.extra_fc_idx * p.df)
            x = dc.call_input(row, p, k)
            iq = x if row.shared_input else np.stack([(x * dc.stream_turn(row, c)).astype(np.complex64) for c in range(row.C)])
            buf = DeviceBuffer.from_array(to_f32_iq(iq), rx.device, rx.L)
            try:
                rx.process_device(buf.ptr, len(x))
                names = (rx.kernel_name(2), rx.kernel_name(3))
                t = rx.tap(P.TAP_POST_MIXER)
            finally:
                buf.free()
            assert names == (want[k].front, want[k].rest), (name, k, names, want[k])
            assert t is not None and t[0].shape == (row.C, sfs * dc.FRAME), (name, k)
            got.append(t[0])
            for c in p.compare:
                e = dc.frame_errors(t[0][c], refs[c].call(k, x))
                if e.max() > worst[0]:
                    worst = (float(e.max()), (c, k, int(e.argmax())))
        print("%s: worst rel-RMS %.2e at (channel, call, frame) %s over %d channels" % (name, worst[0], worst[1], len(p.compare)))
        assert worst[0] <= TOL, (name, worst)
        got = np.concatenate(got, axis=1)
        assert got.shape == (row.C, p.NB)
        off_peak = [c for c in range(row.C) if dc.peak_bin(got[c], dc.foreign_bins(row, p, c)) != dc.own_bin(row, p, c)]
        assert not off_peak, (name, off_peak)
    finally:
        rx.close()


@pytest.mark.parametrize("name", [r.name for r in dc.STEP_ROWS])
def test_step_with_calls_shorter_than_the_look_back(gpu_lib, oracle_mod, name):
    """P.Decimator with calls of 1, 1, 3, 255, 256, 257, 1, 513 outputs on one handle against the oracle fed the whole input in one
    block (no stage falls back there; the cascade is frame-invariant, tests/test_oracle_pins.py)"""
    import pebblesdr_amd as P
    row = next(r for r in dc.STEP_ROWS if r.name == name)
    ref = oracle_mod.Decimator(row.fs, row.bw)
    D = ref.total_decimation
    x = dc.step_input(row, D)
    want = ref.process(x)
    d = P.Decimator(row.fs, max(dc.STEP_OUTPUTS) * D)
    assert d.buildDecimationChain(row.fs, row.bw) == ref.rate and d.decBy2Stages() == ref.dec_by2_stages
    got, at = [], 0
    for n_out in dc.STEP_OUTPUTS:
        y = d.process(x[at:at + n_out * D])
        assert y.astype(np.complex64).shape == (n_out,), (name, n_out, y.shape)
        got.append(y)
        at += n_out * D
    got = np.concatenate(got).astype(np.complex64)
    assert got.shape == want.astype(np.complex64).shape == (sum(dc.STEP_OUTPUTS),)
    errs = dc.chunk_errors(got, want)
    print("%s: rel-RMS per %d outputs %s" % (name, dc.STEP_CHUNK, " ".join("%.2e" % e for e in errs)))
    assert max(errs) <= TOL, (name, errs)
