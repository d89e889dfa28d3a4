"""GPU tier (-m gpu) for the kernels whose exchange gathers are single 8-byte LDS reads (lds_gather_b64, csrc/fft_lds.h): every kernel
built on fft2048_t128, at the smallest shape that crosses a chain boundary and ends ragged, against the oracle at the bars the
suite's own tests of those kernels use (tests/test_spectrum_chains_gpu.py, tests/test_fastfir_geometry_gpu.py).  The case tables are
imported, not restated.

 * k_spectrum_t128 (8192 bins), float2 input and int8 pairs: one stream.  A chain is G = F / 512 frames long for one stream, so the
   smallest call with chains of two is 1025 frames: 513 chains, the last of one live frame, the last workgroup's second chain dead.
   Then one call of 3 frames (G = 1) whose first frame averages with what that ragged chain left.
 * k_spectrum_q128 (2048 bins, the same transform, one (chain, q) per workgroup): the table's own row.
 * k_fastfir_t128 (2048 / 1025): a call of three blocks and five samples, then the rest of the fourth block.
"""
import numpy as np
import pytest

from tests import fastfir_cases as FC
from tests import spectrum_cases as SC
from tests.test_parity_gpu import TOL_DB, db_err
from tests.test_spectrum_chains_gpu import run_calls

pytestmark = pytest.mark.gpu


def _row(name, **kw):
    return {r.name: r for r in SC.ROWS}[name]._replace(**kw)


@pytest.mark.parametrize("name", ["t128-float", "t128-s8"])
def test_spectrum_t128_one_stream_across_chain_boundaries(gpu_lib, oracle_mod, name):
    import pebblesdr_amd as P
    r = _row(name, S=1, F=1025)
    split = (r.F, 3)
    x = SC.bank_input(r, 0, sum(split))
    sb = P.StreamBank(SC.FS, r.S, frame=r.frame, spectrum_bins=r.bins, fastfir_taps=r.taps, max_frames=r.F)
    try:
        sel = SC.computed_frames(r, split)
        got = run_calls(P, sb, r, x, split, sel)
    finally:
        sb.close()
    worst, done = 0.0, 0
    for k, rows in enumerate(got):
        G = 2 if k == 0 else 1
        lo = sel[k][0]
        for i in SC.compared_rows(r, k, rows.shape[1], G):
            g = lo + i
            e = db_err(rows[0, i], SC.oracle_pair(oracle_mod, r, 0, g - 1, g))
            print("%s call %d row %d (frame %d): max |dB| %.4f" % (name, k, i, g, e))
            assert e <= TOL_DB, (name, k, i, g, e)
            worst, done = max(worst, e), done + 1
    assert done >= 12
    print("%s: %d rows compared, worst max |dB| %.4f (<= %g)" % (name, done, worst, TOL_DB))


def test_spectrum_q128_rows(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    r = _row("q128-2048")
    split = (r.F, 3)
    x = SC.bank_input(r, 0, sum(split))
    sb = P.StreamBank(SC.FS, r.S, frame=r.frame, spectrum_bins=r.bins, fastfir_taps=r.taps, max_frames=r.F)
    try:
        sel = SC.computed_frames(r, split)
        got = run_calls(P, sb, r, x, split, sel)
    finally:
        sb.close()
    worst = 0.0
    for k, rows in enumerate(got):
        lo = sel[k][0]
        for i in SC.compared_rows(r, k, rows.shape[1], r.G if k == 0 else 1):
            for s in (0, r.S - 1):
                e = db_err(rows[s, i], SC.oracle_pair(oracle_mod, r, s, lo + i - 1, lo + i))
                assert e <= TOL_DB, (k, i, s, e)
                worst = max(worst, e)
    print("q128-2048: worst max |dB| %.4f (<= %g)" % (worst, TOL_DB))


def test_fastfir_t128_three_blocks_and_a_ragged_end(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    row = {r.name: r for r in FC.STEP_ROWS}["2048-1025"]
    L = row.L
    x = FC.step_input(row)[:4 * L]
    ref, f = oracle_mod.FastFIR(row.fft, row.taps), P.FastFIR(row.fft, row.taps)
    try:
        assert ref.setup(*FC.BANDS[0]) == 0
        f.SetupParameters(*FC.BANDS[0])
        want, got = [], []
        for lo, hi in ((0, 3 * L + 5), (3 * L + 5, 4 * L)):
            want.append(ref.process(x[lo:hi]))
            got.append(f.ProcessData(x[lo:hi]))
            assert len(got[-1]) == len(want[-1])
    finally:
        f.close()
    want, got = np.concatenate(want), np.concatenate(got)
    assert len(want) == 4 * L
    errs = FC.chunk_errors(got, want, L)
    print("k_fastfir_t128 2048/1025: rel-RMS per block %s (<= %g)" % (" ".join("%.3e" % e for e in errs), FC.TOL))
    assert len(errs) == 4 and max(errs) <= FC.TOL
