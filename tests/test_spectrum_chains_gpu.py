"""GPU tier (-m gpu) of the display transforms' chain table (tests/spectrum_cases.py): every kernel family of csrc/kernels_spectrum.h
walking chains of G >= 2 frames -- the recomputed predecessor, the register carry, a ragged last chain, a dead second chain, surplus
workgroups, which chain leaves the carried amplitudes -- against the oracle, and against a second bank that is fed the same frames in
short calls (G = 1 throughout).  That the rows reach those chains, and that the input gives a wrong predecessor away by 6 dB or
more, is the CPU tier's part (tests/test_spectrum_chains_host.py).

Each row's bank runs three calls through StreamBank with what = 2: F frames, 5 frames, F frames.  Compared against oracle.Spectrum
with the suite's bar (TOL_DB over bins the oracle puts above -110 dB), on stream 0, the last stream and one picked by the LCG: rows
0 and 1 of every call, both sides of the first chain boundary and of two more picked by the LCG, the last two rows.  The oracle
transforms the pair (predecessor, frame); row 0 of the second and third call pairs with the last row of the call before; row 0 of a
fresh bank is not compared (the reference's buffer is uninitialised there).

The 8192-bin rows run the instance a stream bank always takes: nothing runs beside its transform, so k_spectrum_t128 holds its
pass-C twiddles in registers (the name the bank reports does not say so)."""
import numpy as np
import pytest

from tests import spectrum_cases as SC
from tests.test_parity_gpu import TOL_DB, db_err

pytestmark = pytest.mark.gpu


def run_calls(P, sb, row, x, split, want):
    """the run's input x in calls of `split` frames -> per call the computed rows [S, n, bins]; selection and kernel name held to
    `want` (per call the computed frames, numbered from the stream's first)"""
    out, lo = [], 0
    for n, sel in zip(split, want):
        blk = np.ascontiguousarray(x[:, lo * row.frame:(lo + n) * row.frame])
        if row.fmt is None:
            _, s = sb.process(blk, what=2)
        else:
            buf = P.DeviceBuffer.from_array(blk, 0)
            try:
                sb.process_raw_device(buf.ptr, n * row.frame, row.fmt, 0, 1.0, what=2)
                s = sb.spectrum()
            finally:
                buf.free()
        assert list(sb.spectrum_frames()) == [g - lo for g in sel], (row.name, lo)
        assert s.shape == (row.S, len(sel), row.bins) and sb.kernel_name(2) == (row.kernel if sel else ""), (row.name, lo, sb.kernel_name(2))
        out.append(s)
        lo += n
    return out


@pytest.mark.parametrize("name", [r.name for r in SC.ROWS])
def test_frame_chains_against_the_oracle_and_another_partition(gpu_lib, oracle_mod, name):
    """Measured on an MI355X, worst max |dB| per row: q128-32768 0.0051, q128-16384 0.0025, q128-2048 0.0026, waves-4096 0.0024,
    t128-float 0.0047, t128-s8 0.0032, any-1024-8192 0.0018, any-3000-4096 0.0025, any-4096-16384 0.0041, big 0.0138,
    big-listed-s8 0.0104; the second partition's spectra equal the first's bit for bit in every family (the seed a chain recomputes
    and the amplitudes it carries in registers come from the same instructions as the amplitudes a call leaves behind).  With a
    chain seeded from frame f - 2 or from zeros, or the carried amplitudes left by the wrong chain, every row fails by 50 dB or more."""
    import pebblesdr_amd as P
    r = {r.name: r for r in SC.ROWS}[name]
    total = sum(SC.calls(r))
    x = SC.bank_input(r, 0, total)
    banks = [P.StreamBank(SC.FS, r.S, frame=r.frame, spectrum_bins=r.bins, fastfir_taps=r.taps, max_frames=m) for m in (r.F, r.chunk)]
    try:
        if r.ups is not None:
            for sb in banks:
                sb.set_spectrum_updates(r.ups)
        sel = SC.computed_frames(r)
        got = run_calls(P, banks[0], r, x, SC.calls(r), sel)
        flat = sum(sel, [])
        at = {g: j for j, g in enumerate(flat)}
        worst, done = 0.0, 0
        for k, rows in enumerate(got):
            for i in SC.compared_rows(r, k, rows.shape[1], SC.chain_length(r, k)):
                g = sel[k][i]
                for s in SC.streams(r):
                    e = db_err(rows[s, i], SC.oracle_pair(oracle_mod, r, s, flat[at[g] - 1], g))
                    print("%s call %d row %d (frame %d) stream %d: max |dB| %.4f" % (name, k, i, g, s, e))
                    assert e <= TOL_DB, (name, k, i, g, s, e)
                    worst, done = max(worst, e), done + 1
        assert done >= 40
        print("%s: %d rows compared, worst max |dB| %.4f (<= %g)" % (name, done, worst, TOL_DB))
        # the same frames in calls of `chunk`
        other = run_calls(P, banks[1], r, x, SC.chunks(r), SC.computed_frames(r, SC.chunks(r)))
        a, b = np.concatenate(got, axis=1), np.concatenate(other, axis=1)
        assert a.shape == b.shape == (r.S, len(flat), r.bins) and a[:, 1:].max() > -40.0
        same = np.array_equal(a, b)
        if not same:
            d = np.abs(a - b)
            print("%s: partitions differ in %d values, by %.3e dB at most, first at %s" % (name, int((d > 0).sum()), float(d.max()), np.argwhere(d > 0)[0]))
        assert same
    finally:
        for sb in banks:
            sb.close()
