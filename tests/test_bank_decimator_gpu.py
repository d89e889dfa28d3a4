"""GPU tier (-m gpu): k_mix_dec_mfma, the mixer + decimator of every shared-stream bank of 16 or more channels, over the table
of tests/bank_cases.py -- every instance bank_variants() ships, multi-group ragged banks, every front stride the sweep of
tests/test_parity_gpu.py leaves out, chunk lengths that change between the calls of one handle, two waves per SIMD, the WFM
chain, a launch whose chunk pairs do not fill eight workgroups, a retune in mid-run and a channel at exactly 0 Hz.  The CPU
tier (tests/test_bank_decimator_host.py) checks that the rows reach the instances and geometries they name.  No environment
switch is set."""
import numpy as np
import pytest

from tests import bank_cases as B
from tests.test_parity_gpu import TOL, rel_rms

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", B.ROWS, ids=[r.name for r in B.ROWS])
def test_bank_decimator_against_the_oracle(gpu_lib, oracle_mod, row):
    """Two comparisons per row.  Oracle: Mixer -> Decimator -> gain restore -> FastFIR (WFM rows: Mixer -> Decimator ->
    DemodWFM) fed whole super-frames, per 2048-sample output frame rel-RMS <= TOL on the channels at every structural edge
    (first, last and both sides of every 32-, 64- and 128-channel boundary), the 0 Hz channel, the retuned one and three the LCG
    picks.  Lane mapping: every channel's own tone is the largest bin of its last 3 x 2048 outputs, in the bin its tuning predicts
    (the oracle meets this: test_the_oracle_puts_every_compared_peak_where_the_tuning_predicts)."""
    import pebblesdr_amd as P
    rx = P.ReceiverBank(row.fs, row.C, True, row.wfm, row.spectrum_bins, max_superframes=row.max_superframes)
    chain = rx.chain()
    assert B.instance_of(chain) == row.instance, chain
    p = B.plan(row, chain)
    assert rx.D == p.D
    assert rx.superframe == B.FRAME * p.D
    for c in range(row.C):
        rx.set_mixer(c, p.fc[c])
        if row.wfm:
            rx.set_mode(c, P.DM_FMM)
        else:
            rx.set_mode(c, P.DM_USB); rx.set_bandpass(c, *p.band[c])
    refs = {c: B.OracleChannel(oracle_mod, row, p, c, chain) for c in p.compare}
    worst, tail = (0.0, None), np.zeros((row.C, 0), dtype=np.complex64)
    for k in range(len(row.calls)):
        if k == row.retune_before:
            rx.set_mixer(p.retuned, p.extra_fc)
        x = B.call_input(row, p, k)
        g = rx.process(x)[0]
        assert g.shape == (row.C, row.calls[k] * B.FRAME)
        if row.geometry[k] is not None:
            assert rx.kernel_name(2) == "k_mix_dec_mfma", (k, rx.kernel_name(2), chain)
        else:  # (inside the oscillators' transient)
            assert rx.kernel_name(2) != "k_mix_dec_mfma", k
        tail = np.concatenate([tail, g], axis=1)[:, -3 * B.FRAME:]
        for c in p.compare:
            r = refs[c].call(k, x)
            assert r.shape == g[c].shape
            for f in range(row.calls[k]):
                e = rel_rms(g[c][f * B.FRAME:(f + 1) * B.FRAME], r[f * B.FRAME:(f + 1) * B.FRAME])
                worst = max(worst, (e, "channel %d call %d frame %d" % (c, k, f)))
        del x, g
    print("%s %s: worst rel_rms %.3g (%s) against %g" % (row.name, row.instance, worst[0], worst[1], TOL))
    assert worst[0] <= TOL, worst
    got = (B.peak_bins_wfm if row.wfm else B.peak_bins)(tail)
    want = np.array(B.final_bins(row, p))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "channels whose peak is not their own tone's bin: %s (got %s, want %s)" % (bad[:16], got[bad[:16]], want[bad[:16]])
