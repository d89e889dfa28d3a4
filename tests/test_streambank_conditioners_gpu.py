"""GPU tier (-m gpu): the stream bank's input conditioners -- DCRemoval, IQBalance, NB1, NB2 in time-parallel form
(csrc/kernels_condition.h) ahead of the band-pass and the display transform -- against the oracle's chain.

The oracle's side, the test input and the margin condition are those of tests/test_streambank_conditioners_host.py (see there): the
inputs leave every blanker decision room, and every test that compares decisions asserts that room on the CPU first.

Bars are the suite's own, imported: TOL (1e-5 relative RMS) for _conditioned, _filtered and the IQ ring, TOL_DB (0.1 dB) for spectrum
rows from the second one on and for the S-meter.  NB1's exact-zero positions equal the oracle's; everything between two device runs of
the same kernels is bit for bit.  Every test prints its figures before it asserts.

Shapes: 2048-sample frames (one chunk of the kernels per frame: 1 .. 8 workgroups per stream and call), and 65536-sample frames with
2 and 4 frames per call (64 and 128 workgroups per stream: one and two steps of the per-stream scans).  Spikes sit at -3, +2, +5 around
every chunk boundary of every call (frame and call boundaries are among them), around a wave-step and lane boundaries, and runs of
40 consecutive spikes cross lane and chunk boundaries.
"""
import numpy as np
import pytest

from tests.test_parity_gpu import TOL, TOL_DB, db_err, rel_rms
from tests.test_streambank_conditioners_host import CHUNK, E_INVALID, Chain, assert_margin, edges_for, fastfir_and_spectrum, spiky
from tests.test_streambank_egress_gpu import as_c64

pytestmark = pytest.mark.gpu

FLAGS6 = [0, 1, 2, 4, 8, 15]
GAINS6 = [1.0, 1.01, 1.02, 0.97, 1.03, 1.05]
PHASES6 = [0.0, 0.01, 0.03, -0.02, 0.02, 0.01]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_input(fs, S, frame, calls, seed, runs, splits=()):
    """[S, n] complex64 (what the device is handed; the oracle gets the same floats)"""
    n = sum(calls) * frame
    edges = set(edges_for(n, frame, calls))
    for other in splits:
        edges.update(edges_for(n, frame, other))
    x = np.stack([spiky(fs, n, seed + s, sorted(edges), runs, f_tone=fs * (0.0493 + 0.0034 * s)) for s in range(S)]).astype(np.complex64)
    x.setflags(write=False)
    return x


def run_calls(sb, x, frame, calls, what=3):
    """-> per call (conditioned or None, filtered or None, spectrum or None)"""
    out, at = [], 0
    for c in calls:
        y, s = sb.process(x[:, at * frame:(at + c) * frame], what)
        cond = sb.conditioned()
        out.append((None if cond is None else cond.copy(), y, s))
        at += c
    return out


def joined(res, i):
    return np.concatenate([r[i] for r in res], axis=1)


def oracle_side(oracle_mod, fs, frame, x, flags, gains, phases):
    chains = []
    for s in range(x.shape[0]):
        ch = Chain(oracle_mod, fs, frame)
        ch.set(flags[s], gains[s], phases[s])
        chains.append(ch)
    return chains, [chains[s].process(x[s]) for s in range(x.shape[0])]


# 1
@pytest.mark.parametrize("bins", [2048, 8192])
def test_six_streams_with_their_own_flags(gpu_lib, oracle_mod, bins):
    """flags 0, 1, 2, 4, 8, 15, a gain and phase per stream, 8 frames in calls of 1, 3, 4: _conditioned, _filtered and the spectrum of
    every stream against its oracle chain; the flags-0 stream bit for bit what a bank gives on which the setter was never called."""
    import pebblesdr_amd as P
    fs, frame, S, calls = 2048000.0, 2048, 6, [1, 3, 4]
    band = (-150e3, 150e3)
    x = make_input(fs, S, frame, calls, 20, [5000, 3 * CHUNK - 20])
    sb, twin = [P.StreamBank(fs, S, frame=frame, spectrum_bins=bins, max_frames=4) for _ in range(2)]
    try:
        for b in (sb, twin):
            for s in range(S):
                b.set_bandpass(s, *band)
        for s in range(S):
            sb.set_conditioners(s, FLAGS6[s], GAINS6[s], PHASES6[s])
        res, plain = run_calls(sb, x, frame, calls), run_calls(twin, x, frame, calls)
    finally:
        sb.close(); twin.close()
    assert all(r[0] is None for r in plain)
    cond, filt, spec = joined(res, 0), joined(res, 1), joined(res, 2)
    chains, v = oracle_side(oracle_mod, fs, frame, x, FLAGS6, GAINS6, PHASES6)
    assert_margin(chains, "six streams, %d bins" % bins)
    figures = []
    for s in range(S):
        y, rows = fastfir_and_spectrum(oracle_mod, v[s], fs, frame, bins, *band)
        figures.append((rel_rms(cond[s], v[s]), rel_rms(filt[s], y), max(db_err(spec[s][f], rows[f]) for f in range(1, len(rows))),
                        int(np.count_nonzero(v[s] == 0)), bool(np.array_equal(cond[s] == 0, v[s] == 0))))
    print("flags %s, %d bins: (conditioned, filtered rel RMS, spectrum dB, oracle zeros, same zero positions) %s" % (FLAGS6, bins, figures))
    same0 = [bool(np.array_equal(bits(cond[0]), bits(x[0]))), bool(np.array_equal(bits(filt[0]), bits(joined(plain, 1)[0]))),
             bool(np.array_equal(bits(spec[0]), bits(joined(plain, 2)[0])))]
    print("the flags-0 stream against the untouched bank (conditioned = input, filtered, spectrum): %s" % same0)
    for s in range(S):
        assert figures[s][0] <= TOL and figures[s][1] <= TOL and figures[s][2] <= TOL_DB, (s, figures[s])
        assert figures[s][4], (s, figures[s])
        if FLAGS6[s] & 4:
            assert figures[s][3] > 100
    assert all(same0)


# 2
@pytest.mark.parametrize("calls,flags", [((2, 2), [15, 5]), ((4,), [15])])
def test_long_rows(gpu_lib, oracle_mod, calls, flags):
    """65536-sample frames, 65536 bins: 2 streams (flags 15 and 5), 2 frames per call, 2 calls -- the smallest shape at which one stream
    spans many workgroups in all three scans (64 per call) -- all three outputs; and one stream, 4 frames in one call (128 workgroups:
    the per-stream scans take two steps and carry from the first to the second), what = 0, _conditioned alone."""
    import pebblesdr_amd as P
    fs, frame, bins, S = 20.0e6, 65536, 65536, len(flags)
    what = 3 if len(calls) > 1 else 0
    band = (-2e6, 2e6)
    x = make_input(fs, S, frame, calls, 40, [70000, 33 * CHUNK - 17])
    sb = P.StreamBank(fs, S, frame=frame, spectrum_bins=bins, max_frames=max(calls))
    try:
        for s in range(S):
            sb.set_bandpass(s, *band)
            sb.set_conditioners(s, flags[s], GAINS6[s + 1], PHASES6[s + 1])
        res = run_calls(sb, x, frame, calls, what)
    finally:
        sb.close()
    cond = joined(res, 0)
    chains, v = oracle_side(oracle_mod, fs, frame, x, flags, GAINS6[1:], PHASES6[1:])
    assert_margin(chains, "long rows %s" % (calls,))
    figures = []
    for s in range(S):
        fig = [rel_rms(cond[s], v[s]), int(np.count_nonzero(v[s] == 0)), bool(np.array_equal(cond[s] == 0, v[s] == 0))]
        if what:
            y, rows = fastfir_and_spectrum(oracle_mod, v[s], fs, frame, bins, *band)
            fig += [rel_rms(joined(res, 1)[s], y), max(db_err(joined(res, 2)[s][f], rows[f]) for f in range(1, len(rows)))]
        figures.append(fig)
    print("long rows, calls %s, flags %s: (conditioned rel RMS, oracle zeros, same zero positions[, filtered rel RMS, spectrum dB]) %s"
          % (calls, flags, figures))
    for s, fig in enumerate(figures):
        assert fig[0] <= TOL and fig[2], (s, fig)
        if flags[s] & 4:
            assert fig[1] > 1000
        if what:
            assert fig[3] <= TOL and fig[4] <= TOL_DB, (s, fig)


# 3
def test_call_splitting(gpu_lib, oracle_mod):
    """the same 8 frames as one call and as 1 + 3 + 2 + 2: _conditioned within TOL, the zero positions identical; the same split again
    gives the same bits"""
    import pebblesdr_amd as P
    fs, frame, S, flags = 2048000.0, 2048, 3, [15, 13, 6]
    one, split = [8], [1, 3, 2, 2]
    x = make_input(fs, S, frame, one, 62, [5000, 5 * CHUNK - 20], splits=[split])  # (seed 60 misses the margin condition: 1.4e-5)
    got = []
    for calls in (one, split, split):
        sb = P.StreamBank(fs, S, frame=frame, spectrum_bins=2048, max_frames=8)
        try:
            for s in range(S):
                sb.set_conditioners(s, flags[s], GAINS6[s + 1], PHASES6[s + 1])
            got.append(joined(run_calls(sb, x, frame, calls, 0), 0))
        finally:
            sb.close()
    chains, v = oracle_side(oracle_mod, fs, frame, x, flags, GAINS6[1:], PHASES6[1:])
    assert_margin(chains, "call splitting")
    figures = [(rel_rms(got[1][s], got[0][s]), rel_rms(got[0][s], v[s]), bool(np.array_equal(got[0][s] == 0, got[1][s] == 0)),
                bool(np.array_equal(got[0][s] == 0, v[s] == 0))) for s in range(S)]
    again = bool(np.array_equal(bits(got[1]), bits(got[2])))
    print("one call against 1 + 3 + 2 + 2: (split vs one, one vs oracle rel RMS, same zeros, the oracle's zeros) %s; the split twice: same bits %s"
          % (figures, again))
    for fig in figures:
        assert fig[0] <= TOL and fig[1] <= TOL and fig[2] and fig[3], fig
    assert again


# 4
def test_blankers_off_and_on_again(gpu_lib, oracle_mod):
    """both blankers on for one call, off for the next, on again for the third, every call at another level: switching one on resets its
    averages (and NB1's count) on the device, in stream order, as the oracle's enable does; the DC filter's state and NB1's delay line
    carry across.  Every call against the oracle chain given the same setter calls."""
    import pebblesdr_amd as P
    fs, frame, S, F = 2048000.0, 2048, 2, 4
    plan = [(13, 15), (1, 3), (13, 15)]
    levels = (1.0, 0.5, 2.0)
    n = F * frame
    # (seeds 80, 85, 90 miss the margin condition while NB2's average charges again: 6.2e-5)
    x = np.concatenate([make_input(fs, S, frame, [F], 81 + 5 * k, [5000]) * np.float32(levels[k]) for k in range(3)], axis=1)
    sb = P.StreamBank(fs, S, frame=frame, spectrum_bins=2048, max_frames=F)
    chains = [Chain(oracle_mod, fs, frame) for _ in range(S)]
    figures = []
    try:
        for k, fl in enumerate(plan):
            for s in range(S):
                sb.set_conditioners(s, fl[s], 1.02, 0.03)
                chains[s].set(fl[s], 1.02, 0.03)
            sb.process(x[:, k * n:(k + 1) * n], 0)
            cond = sb.conditioned()
            for s in range(S):
                v = chains[s].process(x[s, k * n:(k + 1) * n])
                figures.append((k, s, rel_rms(cond[s], v), int(np.count_nonzero(v == 0)), bool(np.array_equal(cond[s] == 0, v == 0))))
    finally:
        sb.close()
    assert_margin(chains, "blankers on / off / on")
    print("blankers on / off / on: (call, stream, conditioned rel RMS, oracle zeros, same zero positions) %s" % figures)
    for k, s, e, zeros, same in figures:
        assert e <= TOL and same, (k, s, e)
        assert (zeros > 100) == (k != 1)


# 5
def test_raw_route(gpu_lib):
    """the same samples as int8 through process_raw and as converted float2 through process: bit-identical _conditioned, _filtered and
    spectrum over three calls; kernel_name names the staged route while a flag is set and the converting loads again once all are
    cleared"""
    import pebblesdr_amd as P
    from tests.test_streambank_raw_gpu import host_convert
    fs, frame, bins, S, F, K = 2048000.0, 2048, 8192, 3, 4, 3
    flags = [15, 0, 5]
    n = F * frame
    xf = make_input(fs, S, frame, [F] * K, 100, [5000])
    raw = np.clip(np.round(np.stack([xf.real, xf.imag], axis=-1) * 40.0), -127, 127).astype(np.int8)
    x = host_convert(raw, 0, 0, 1.0)
    a, b = [P.StreamBank(fs, S, frame=frame, spectrum_bins=bins, max_frames=F) for _ in range(2)]
    names, same = [], []
    try:
        for sb in (a, b):
            for s in range(S):
                sb.set_bandpass(s, -150e3, 150e3)
                sb.set_conditioners(s, flags[s], 1.02, 0.03)
        for k in range(K + 1):
            if k == K:  # all flags cleared again: the routes of a bank without conditioners
                for sb in (a, b):
                    for s in range(S):
                        sb.set_conditioners(s, 0)
            lo = (k % K) * n
            buf = P.DeviceBuffer.from_array(np.ascontiguousarray(raw[:, lo:lo + n]), 0)
            try:
                a.process_raw_device(buf.ptr, n, 0, 0, 1.0, 3)
                ra = (a.conditioned(), a.filtered(), a.spectrum())
            finally:
                buf.free()
            names.append((a.kernel_name(1), a.kernel_name(2)))
            yb, sp = b.process(x[:, lo:lo + n], 3)
            rb = (b.conditioned(), yb, sp)
            names.append((b.kernel_name(1), b.kernel_name(2)))
            if k < K:
                same.append([bool(np.array_equal(bits(p), bits(q))) for p, q in zip(ra, rb)])
                assert np.abs(rb[0][0]).max() > 0.1 and np.array_equal(bits(rb[0][1]), bits(x[1, lo:lo + n]))
            else:
                same.append([ra[0] is None and rb[0] is None] + [bool(np.array_equal(bits(p), bits(q))) for p, q in zip(ra[1:], rb[1:])])
    finally:
        a.close(); b.close()
    print("raw int8 against converted float2 (conditioned, filtered, spectrum) per call: %s; routes %s" % (same, names))
    assert all(all(s) for s in same)
    staged = ("k_normalize_iq + k_condition + k_fastfir_t128", "k_normalize_iq + k_condition + k_spectrum_t128")
    plain = ("k_condition + k_fastfir_t128", "k_condition + k_spectrum_t128")
    assert names[:2 * K] == [staged, plain] * K
    assert names[2 * K:] == [("k_fastfir_t128 (raw s8)", "k_spectrum_t128 (raw s8)"), ("k_fastfir_t128", "k_spectrum_t128")]


# 6
def test_downstream_reads_the_conditioned_rows(gpu_lib, oracle_mod):
    """DC removal on and a band-pass across 0 Hz: signal_strength() and an IQ-ring block equal what the oracle's chain gives for the
    CONDITIONED stream (a 0.01 offset under a 0.004 tone: unconditioned, the S-meter would read the offset)"""
    import pebblesdr_amd as P
    from tests.signals import lcg_noise, tones
    fs, frame, bins, S, F = 256000.0, 2048, 2048, 2, 4   # (the 10 Hz high-pass settles within these 16384 samples)
    lo, hi = -5000.0, 5000.0
    n = F * frame
    x = np.stack([tones(fs, 2 * n, [(0.004, 1000.0 + 500.0 * s)]) + lcg_noise(2 * n, 120 + s, 1e-4) + 0.01 for s in range(S)]).astype(np.complex64)
    sb = P.StreamBank(fs, S, frame=frame, spectrum_bins=bins, max_frames=F)
    try:
        for s in range(S):
            sb.set_bandpass(s, lo, hi)
            sb.set_conditioners(s, 1)
        sb.enable_signal_strength(True)
        sb.iq_out_open(P.AUDIO_F32, None, n_slots=2)
        sm, blocks = [], []
        for k in range(2):
            sb.process(x[:, k * n:(k + 1) * n], 3)
            sm.append(sb.signal_strength())
            got = sb.iq_out_next(True)
            assert got is not None and got[0] == k
            blocks.append(as_c64(got[2]).copy())
            sb.iq_out_release(k)
    finally:
        sb.close()
    sm, blocks = np.concatenate(sm, axis=1), np.concatenate(blocks, axis=1)
    chains, v = oracle_side(oracle_mod, fs, frame, x, [1] * S, [1.0] * S, [0.0] * S)
    figures = []
    for s in range(S):
        y, rows = fastfir_and_spectrum(oracle_mod, v[s], fs, frame, bins, lo, hi)
        want = np.array([oracle_mod.fd_estimate(rows[f], int(round(fs)), np.float32(lo), np.float32(hi), 0.0) for f in range(len(rows))])
        raw_rows = fastfir_and_spectrum(oracle_mod, x[s], fs, frame, bins, lo, hi)[1]
        unconditioned = np.array([oracle_mod.fd_estimate(raw_rows[f], int(round(fs)), np.float32(lo), np.float32(hi), 0.0) for f in range(len(rows))])
        figures.append((float(np.abs(sm[s][1:] - want[1:]).max()), rel_rms(blocks[s], y), float(abs(unconditioned[-1, 0] - want[-1, 0]))))
    print("DC removal ahead of a band-pass across 0 Hz: (S-meter dB, IQ block rel RMS, how far the unconditioned peak of the last row lies, dB) %s" % figures)
    for e_db, e_iq, apart in figures:
        assert apart > 10 * TOL_DB   # (or the test could not tell)
        assert e_db <= TOL_DB and e_iq <= TOL


# 7
def test_refusals_leave_the_handle_usable(gpu_lib):
    import pebblesdr_amd as P
    fs, frame, S = 2048000.0, 2048, 2
    L = P.load_library()
    sb = P.StreamBank(fs, S, frame=frame, spectrum_bins=2048, max_frames=2)
    try:
        assert sb.conditioned() is None   # before any flag
        x = make_input(fs, S, frame, [2], 140, [1000])
        sb.process(x, 3)
        assert sb.conditioned() is None   # a call with none
        for args in ((S, 1, 1.0, 0.0), (0, 16, 1.0, 0.0), (0, -1, 1.0, 0.0), (0, 2, float("nan"), 0.0), (0, 2, 1.0, float("inf"))):
            assert L.pebblegpu_streambank_set_conditioners(sb.h, *args) == E_INVALID, args
        assert L.pebblegpu_streambank_set_conditioners(None, 0, 1, 1.0, 0.0) == E_INVALID
        sb.process(x, 3)
        assert sb.conditioned() is None   # nothing was accepted
        sb.set_conditioners(1, 1)
        y, s = sb.process(x, 3)
        c = sb.conditioned()
        assert c is not None and c.shape == x.shape and np.array_equal(bits(c[0]), bits(x[0])) and not np.array_equal(c[1], x[1])
        assert np.isfinite(y).all() and np.isfinite(s).all()
        sb.process_device(0, 0, 3)
        assert sb.conditioned() is None   # a call of no samples conditioned nothing
        sb.set_conditioners(1, 0)
        sb.process(x, 3)
        assert sb.conditioned() is None
    finally:
        sb.close()
