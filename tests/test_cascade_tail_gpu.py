"""GPU tier of the fixed-tap k_cascade instances' tiles (csrc/kernels_frontend.h cascade_fixed; csrc/decim_route.h cascade_fixed_tile):
k_cascade<15,23,47> at 20 Msps WFM and k_cascade<15,19,31> at 2.048 Msps narrow, against the oracle's Decimator at decim_cases.TOL.

One channel through P.Decimator, consecutive calls on ONE handle so that the head-room carries from call to call, with the smallest
call lengths that give each tile case (the tile is 256 final outputs): 255 outputs (fewer than a tile: the only tile is ragged, with
an odd count, so the last work-item's second window is the unused one), 256 (exactly one), 257 (one tile and a tile of one output)
and 770 (three tiles and a ragged one of two).  Every call is compared on its own, the first included: rel-RMS over the call, or per
256 outputs where it is longer (a receiver's 2048-output frame does not fit these calls; decim_cases.chunk_errors is the step rows' measure).
The step reports no kernel names: that the chain takes the fixed-tap instance is decim_cases.step_route()'s statement, asserted here.

A 3-channel bank through P.ReceiverBank at the POST_MIXER tap, as tests/test_decimator_routes_gpu.py runs its rows: calls of 1, 2, 1
and 3 super-frames (8 .. 24 whole tiles per channel, grid y = 3), per 2048-output frame as decim_cases.frame_errors has it, every
channel, and the kernel names of every call are the ones route() predicts.

Measured on an MI355X (bar 1e-5): the step calls 9.1e-8 .. 9.9e-8 (narrow) and 1.1e-7 .. 1.2e-7 (WFM) per 256 outputs, the bank's
frames 1.1e-7 .. 1.3e-7 (narrow) and up to 1.7e-7 (WFM)."""
import numpy as np
import pytest

from tests import decim_cases as dc

pytestmark = pytest.mark.gpu

CALLS = (255, 256, 257, 3 * 256 + 2)
RATES = {"wfm-20M": (20_000_000, 200000, True, "k_cascade<15,23,47>"), "narrow-2048k": (2_048_000, 30000, False, "k_cascade<15,19,31>")}


@pytest.mark.parametrize("name", sorted(RATES))
def test_one_channel_tiles_on_one_handle(gpu_lib, oracle_mod, name):
    import pebblesdr_amd as P
    fs, bw, _, inst = RATES[name]
    ref = oracle_mod.Decimator(fs, bw)
    chain, D = ref.chain(), ref.total_decimation
    for n_out in CALLS:
        r = dc.step_route(chain, n_out)
        assert (r.rest, r.cascade_inst, r.outb, r.tiles, r.last_tile) == ("k_cascade", inst, 256, -(-n_out // 256), n_out - (-(-n_out // 256) - 1) * 256)
    n = sum(CALLS) * D
    t = np.arange(n) / float(fs)
    out = fs / D
    x = (0.3 * np.exp(2j * np.pi * 1000.0 * t) + 0.2 * np.exp(1j * (2 * np.pi * (-0.26 * out) * t + 0.4)) + 0.2 * np.exp(2j * np.pi * (0.31 * fs) * t)
         + dc.lcg_noise(n, 41, 1e-3))
    want = ref.process(x)  # (the oracle's cascade is frame-invariant: tests/test_oracle_pins.py)
    d = P.Decimator(fs, max(CALLS) * D)
    try:
        assert d.buildDecimationChain(fs, bw) == ref.rate
        at, worst = 0, []
        for n_out in CALLS:
            y = d.process(x[at * D:(at + n_out) * D]).astype(np.complex64)
            assert y.shape == (n_out,), (name, n_out, y.shape)
            errs = dc.chunk_errors(y, want[at:at + n_out].astype(np.complex64))
            print("%s: call of %d outputs, rel-RMS per %d outputs %s" % (name, n_out, dc.STEP_CHUNK, " ".join("%.2e" % e for e in errs)))
            worst.append(max(errs))
            at += n_out
        assert max(worst) <= dc.TOL, (name, worst)
    finally:
        d.close()


@pytest.mark.parametrize("name", sorted(RATES))
def test_three_channel_bank_at_the_post_mixer_tap(gpu_lib, oracle_mod, name):
    import pebblesdr_amd as P
    from pebblesdr_amd.binding import DeviceBuffer, to_f32_iq
    fs, bw, wfm, inst = RATES[name]
    row = dc._row("tail-" + name, fs, 3, "the fixed-tap cascade behind a 3-channel bank", wfm=wfm)
    chain = oracle_mod.Decimator(fs, bw).chain()
    p = dc.plan(row, chain)
    want = dc.routes(row, chain)
    assert all(w.cascade_inst == inst and w.rest == "k_cascade" for w in want)
    rx = P.ReceiverBank(fs, 3, True, wfm, 0, max_superframes=max(row.calls))
    try:
        assert rx.chain() == chain and rx.superframe == p.P1
        rx.set_taps([P.TAP_POST_MIXER])
        for c in range(3):
            rx.set_mixer(c, p.fc_idx[c] * p.df)
        refs = {c: dc.OracleChannel(oracle_mod, row, p, c, chain) for c in range(3)}
        worst = (0.0, None)
        for k, sfs in enumerate(row.calls):
            x = dc.call_input(row, p, k)
            buf = DeviceBuffer.from_array(to_f32_iq(x), rx.device, rx.L)
            try:
                rx.process_device(buf.ptr, len(x))
                names = (rx.kernel_name(2), rx.kernel_name(3))
                t = rx.tap(P.TAP_POST_MIXER)
            finally:
                buf.free()
            assert names == (want[k].front, want[k].rest), (name, k, names, want[k])
            assert t is not None and t[0].shape == (3, sfs * dc.FRAME), (name, k)
            for c in range(3):
                e = dc.frame_errors(t[0][c], refs[c].call(k, x))
                print("%s: call %d channel %d rel-RMS per frame %s" % (name, k, c, " ".join("%.2e" % v for v in e)))
                if e.max() > worst[0]:
                    worst = (float(e.max()), (c, k, int(e.argmax())))
        assert worst[0] <= dc.TOL, (name, worst)
    finally:
        rx.close()
