"""GPU tier (-m gpu) of the receivers' S-meter: k_signal_strength behind Receiver::apply_controls' windows (strength_windows, params.h) on
every row of tests/strength_cases.py that a receiver at these rates can be set to, and the three squelch gates that read its avgDb.

Shapes: 2.048 Msps, 2048-sample frames, 2048 and 4096 bins, calls of 1 and of 3 super-frames; WFM receivers at 2.048 Msps (decimated)
and at 192000 and 250000 Hz (no decimator).  One channel per table row, mode USB / LSB / CWL to fit; a tone inside some windows whose
level changes from frame to frame (so a wrong frame shows), LCG noise at 1e-3.

Bars.  Every float4 against oracle.fd_estimate of the device's OWN dB row: TOL_REDUCTION = 1e-4 dB, the project's reduction bar (the
kernel adds 64 partial sums in another order than the serial loop; the float report's rounding near 120 dB is 8e-6).  A value that the
row's class makes a bound (strength_cases.expected) equals it exactly, and nothing is NaN or infinite.  End to end, against fd_estimate
of the oracle's own spectrum of the same frames: TOL_DB (0.1 dB) from the stream's second frame on, for the non-degenerate rows.
Another route's rows are bit for bit the plain route's wherever that route's dB rows are; where a route computes its dB rows with another
kernel (the update gate's list kernels) they are held to their own rows at the reduction bar.  A two-stage call (a bank created without
spectrum_bins) has no spectrum: it refuses the S-meter, which test_refusals_leave_the_handle_usable asserts; the routes of a call WITH a
spectrum are side by side (the default), single-stream (per-kernel profiling), raw input, and the update gate.

Measured on an MI355X: see DESIGN.md section 3, "Receiver S-meter: the window table".
"""
import functools

import numpy as np
import pytest

from tests import strength_cases as S
from tests.raw_cases import host_convert
from tests.signals import lcg_noise
from tests.spectrum_gate_ref import GateTimer
from tests.test_parity_gpu import TOL_DB

pytestmark = pytest.mark.gpu

FS, N = 2048000, 2048
TOL_REDUCTION = 1e-4
E_INVALID, E_FILTER_PARAM = -1, -4
IQ_S16 = 2                         # pebblegpu_iq_format: int16 pairs, normaliser 32768
TONES = {"usb_centred": 1650.0, "centred_64": 500.0, "clipped_low_65": 13000.0, "usb_nhi_bins": 1650.0, "lsb_negative": -1650.0,
         "lsb_clipped_low": -1650.0, "narrow_one_bin": 150.0, "usb_centred_4096": 1650.0, "cw_negative_4096": -750.0,
         "wfm_centred_601": 30e3, "wfm_clipped_high": 20e3}        # offset from the row's mixer frequency, Hz
SENTINELS = ["usb_centred", "lsb_clipped_low", "lsb_lower_edge_one_bin", "mixer_beyond_half_rate", "refused_inverted"]


def narrow_rows(bins):
    return [r for r in S.ROWS if r[1] == FS and r[2] == bins and (r[3], r[4]) != S.WFM]


def mode_of(P, r):
    return P.DM_CWL if r[0].startswith("cw_") else P.DM_LSB if r[0].startswith("lsb_") else P.DM_USB


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def set_window(P, rx, c, r):
    """mode, mixer and band-pass of row r on channel c; a pair with lo >= hi is refused and stored all the same (fastfir.cpp:200-203)"""
    rx.set_mode(c, mode_of(P, r))
    rx.set_mixer(c, r[5])
    if r[3] >= r[4]:
        with pytest.raises(P.PebbleGpuError) as e:
            rx.set_bandpass(c, r[3], r[4])
        assert e.value.code == E_FILTER_PARAM
    else:
        rx.set_bandpass(c, r[3], r[4])


def make_bank(P, rows, bins, shared=True, max_sf=3):
    rx = P.ReceiverBank(FS, len(rows), shared, False, bins, max_superframes=max_sf)
    for c, r in enumerate(rows):
        set_window(P, rx, c, r)
    rx.enable_signal_strength(True)
    return rx


@functools.lru_cache(maxsize=None)
def signal(names, n_frames, seed, level=1.0):
    """complex64 [n_frames * N] (read-only): a tone of amplitude 0.02 inside the window of every row of `names` that has an entry in
    TONES, all scaled by (1, 1.5, 2)[frame % 3] * level, plus LCG noise at 1e-3"""
    t = np.arange(n_frames * N, dtype=np.float64) / FS
    env = np.repeat(1.0 + 0.5 * (np.arange(n_frames) % 3), N) * level
    x = np.zeros(n_frames * N, dtype=np.complex128)
    for name in names:
        if name in TONES:
            x += 0.02 * np.exp(2j * np.pi * (S.row(name)[5] + TONES[name]) * t)
    x = (env * x + lcg_noise(n_frames * N, seed, 1e-3)).astype(np.complex64)
    assert np.abs(x).max() < 0.8
    x.setflags(write=False)
    return x


def run_calls(rx, x, calls):
    """x [streams, n] or [n] in calls of `calls` super-frames -> per call dict(sm [C, rows, 4], spec [streams, rows, bins], audio, frames)"""
    x = np.atleast_2d(x)
    sf, at, out = rx.superframe, 0, []
    for k in calls:
        a, sp = rx.process(x[:, at * sf:(at + k) * sf])
        out.append(dict(sm=rx.signal_strength(), spec=sp, audio=a, frames=list(rx.spectrum_frames()), at=at * sf // N, k=k))
        at += k
    return out


def check_own(oracle_mod, rows, sm, spec, fs=FS, stream_of=None, what=""):
    """sm [C, F, 4] against fd_estimate of the device's own dB rows spec [streams, F, bins] -> worst |dB|; the class's bounds exact"""
    assert sm.shape == (len(rows), spec.shape[1], 4), (what, sm.shape, spec.shape)
    assert np.isfinite(sm).all(), (what, "NaN or inf", np.argwhere(~np.isfinite(sm))[:8])
    worst = 0.0
    for c, r in enumerate(rows):
        s = stream_of[c] if stream_of else 0
        for f in range(sm.shape[1]):
            own = oracle_mod.fd_estimate(spec[s, f].astype(np.float64), fs, np.float32(r[3]), np.float32(r[4]), r[5])
            d = float(np.abs(sm[c, f].astype(np.float64) - own).max())
            worst = max(worst, d)
            assert d <= TOL_REDUCTION, (what, r[0], f, sm[c, f], own)
            for k, v in S.expected(r[6]).items():
                assert sm[c, f, k] == np.float32(v), (what, r[0], f, k, sm[c, f])
    return worst


def oracle_spectra(oracle_mod, x, bins, n_frames):
    sp = oracle_mod.Spectrum(bins, N)
    return np.array([sp.process(x[f * N:(f + 1) * N].astype(np.complex128)) for f in range(n_frames)])


# ------------------------------------------------------------------------------------------------
# 1. narrow bank, shared input: one channel per table row, K = 1 then K = 3
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shared_reference(bins):
    """the rows of `bins` through one bank, calls of 1 and 3 super-frames (computed once, shared) -> (rows, x, results)"""
    import pebblesdr_amd as P
    rows = narrow_rows(bins)
    rx = make_bank(P, rows, bins)
    try:
        fps = rx.superframe // N
        x = signal(tuple(r[0] for r in rows), 4 * fps, 11)
        return rows, x, run_calls(rx, x, [1, 3]), fps
    finally:
        rx.close()


@pytest.mark.parametrize("bins", [2048, 4096])
def test_every_window_on_a_shared_stream(gpu_lib, oracle_mod, bins):
    rows, x, res, fps = shared_reference(bins)
    assert len(rows) >= 3 and {r[6] for r in rows} >= {"centred", "bp0_no_bin"}
    worst = 0.0
    for k, r in enumerate(res):
        assert r["sm"].shape[1] == r["k"] * fps and r["frames"] == list(range(r["k"] * fps))      # every frame of every super-frame has its entry
        worst = max(worst, check_own(oracle_mod, rows, r["sm"], r["spec"], what="call %d" % k))
    sm = np.concatenate([r["sm"] for r in res], axis=1)
    ref = oracle_spectra(oracle_mod, x, bins, 4 * fps)
    worst_end = 0.0
    for c, r in enumerate(rows):
        if r[6] in S.DEGENERATE:
            continue
        for f in range(1, 4 * fps):
            want = oracle_mod.fd_estimate(ref[f], FS, np.float32(r[3]), np.float32(r[4]), r[5])
            d = float(np.abs(sm[c, f] - want).max())
            worst_end = max(worst_end, d)
            assert d <= TOL_DB, (r[0], f, sm[c, f], want)
    print("%d bins, %d channels: reduction max |dB| %.3e (<= %g), end to end max |dB| %.4f (<= %g)" % (bins, len(rows), worst, TOL_REDUCTION, worst_end, TOL_DB))
    # a real meter: the channels with a tone follow its level from frame to frame (levels 1, 1.5, 2, each frame averaged with the one
    # before it: 1.25, 1.75, 1.5 -- 2.9 dB between the extremes)
    for c, r in enumerate(rows):
        if r[0] in TONES and r[6] not in S.DEGENERATE:
            assert sm[c, :, 0].max() > -60.0 and np.ptp(sm[c, 1:, 0]) > 2.0, (r[0], sm[c, :6])


# ------------------------------------------------------------------------------------------------
# 2. independent streams: a level per stream
# ------------------------------------------------------------------------------------------------
def test_every_window_on_its_own_stream(gpu_lib, oracle_mod):
    """shared_input = False: channel c reads stream c (SmBins::stream), whose tones stand at 1 / (1 + c / 4) of the shared test's and whose
    noise has its own seed: another stream's row, or a wrong pitch between the streams' rows, gives another stream's values"""
    import pebblesdr_amd as P
    rows = narrow_rows(2048)
    rx = make_bank(P, rows, 2048, shared=False)
    try:
        fps = rx.superframe // N
        assert rx.n_streams == len(rows)
        names = tuple(r[0] for r in rows)
        x = np.stack([signal(names, 4 * fps, 100 + c, 1.0 / (1.0 + 0.25 * c)) for c in range(len(rows))])
        res = run_calls(rx, x, [1, 3])
    finally:
        rx.close()
    worst, told = 0.0, 0
    for k, r in enumerate(res):
        assert r["spec"].shape[0] == len(rows)
        worst = max(worst, check_own(oracle_mod, rows, r["sm"], r["spec"], stream_of=list(range(len(rows))), what="call %d" % k))
        for c, row in enumerate(rows):                # the neighbour's row would not have passed
            if row[6] in S.DEGENERATE:
                continue
            o = (c + 1) % len(rows)
            other = oracle_mod.fd_estimate(r["spec"][o, 1].astype(np.float64), FS, np.float32(row[3]), np.float32(row[4]), row[5])
            told += int(np.abs(r["sm"][c, 1] - other).max() > 100 * TOL_REDUCTION)
    n_real = sum(r[6] not in S.DEGENERATE for r in rows)
    assert told == 2 * n_real, (told, n_real)
    print("independent streams, %d channels: reduction max |dB| %.3e (<= %g)" % (len(rows), worst, TOL_REDUCTION))


# ------------------------------------------------------------------------------------------------
# 3. WFM receivers: the fixed +-100 kHz window
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,names", [(2048000, ("wfm_centred_601", "wfm_clipped_high")), (192000, ("wfm_192k_all_in_band",)),
                                      (250000, ("wfm_250k_clipped_both",))])
def test_wfm_windows(gpu_lib, oracle_mod, fs, names):
    """a decimated WFM bank at 2.048 Msps (one channel centred, one tuned near the upper edge), and receivers without a decimator at
    192000 Hz (the window covers the whole spectrum: no noise bin) and 250000 Hz (the noise window clipped at both ends)"""
    import pebblesdr_amd as P
    rows = [S.row(n) for n in names]
    assert all((r[3], r[4]) == S.WFM and r[1] == fs and r[2] == 2048 for r in rows)
    rx = P.ReceiverBank(fs, len(rows), True, True, 2048, max_superframes=3)
    try:
        for c, r in enumerate(rows):
            rx.set_mixer(c, r[5])
        rx.enable_signal_strength(True)
        fps = rx.superframe // N
        T = 4 * fps
        t = np.arange(T * N, dtype=np.float64) / fs
        env = np.repeat(1.0 + 0.5 * (np.arange(T) % 3), N)
        x = lcg_noise(T * N, 21, 1e-3)
        for r in rows:
            x = x + 0.1 * env * np.exp(1j * (2 * np.pi * (r[5] + TONES.get(r[0], 10e3)) * t + 20.0 * np.sin(2 * np.pi * 1000.0 * t)))
        x = x.astype(np.complex64)
        res = run_calls(rx, x, [1, 3])
    finally:
        rx.close()
    worst = max(check_own(oracle_mod, rows, r["sm"], r["spec"], fs=fs, what="call %d" % k) for k, r in enumerate(res))
    sm = np.concatenate([r["sm"] for r in res], axis=1)
    assert sm.shape[1] == T
    ref = oracle_spectra(oracle_mod, x, 2048, T)
    worst_end = 0.0
    for c, r in enumerate(rows):
        for f in range(1, T):
            want = oracle_mod.fd_estimate(ref[f], fs, np.float32(r[3]), np.float32(r[4]), r[5])
            idx = [k for k in range(4) if k not in S.expected(r[6])]          # (the bounds are exact, checked above)
            d = float(np.abs(sm[c, f] - want)[idx].max())
            worst_end = max(worst_end, d)
            assert d <= TOL_DB, (r[0], f, sm[c, f], want)
        assert sm[c, :, 0].max() > -60.0
    print("WFM at %d Hz: reduction max |dB| %.3e (<= %g), end to end max |dB| %.4f (<= %g)" % (fs, worst, TOL_REDUCTION, worst_end, TOL_DB))


# ------------------------------------------------------------------------------------------------
# 4. between calls: retune, band-pass, mode, a refused band-pass
# ------------------------------------------------------------------------------------------------
def test_windows_follow_the_setters_between_calls(gpu_lib, oracle_mod):
    """Six USB channels in two banks on one input; between the calls one bank gets set_mixer (channel 0, to the upper edge), set_bandpass
    (1, to one bin), a mode change (2: the window stays), a refused set_bandpass (3: stored, the window is the inverted pair) and a set_mixer
    beyond fs / 2 (4); channel 5 is left alone.  The next call's values follow the new windows from its first frame on (sm_dirty_); the
    untouched channels -- 2 and 5, and all six before the change -- are the twin's bit for bit"""
    import pebblesdr_amd as P
    base = S.row("usb_centred")
    rows0 = [(base[0], FS, 2048, base[3], base[4], base[5] + 40e3 * c, "centred") for c in range(6)]
    rows1 = list(rows0)
    rows1[0] = ("moved", FS, 2048, base[3], base[4], 1020000.0, "clipped_high")
    rows1[1] = ("one_bin", FS, 2048, 100.0, 200.0, rows0[1][5], "bp0_one_bin")
    rows1[3] = ("refused", FS, 2048, 3000.0, 300.0, rows0[3][5], "inverted")
    rows1[4] = ("beyond", FS, 2048, base[3], base[4], 1.2e6, "bp0_no_bin")
    for r in rows1:
        S.check_class(r)
    a, b = make_bank(P, rows0, 2048), make_bank(P, rows0, 2048)
    try:
        fps = a.superframe // N
        x = signal(("usb_centred",), 6 * fps, 31)
        ra, rb = run_calls(a, x, [1]), run_calls(b, x, [1])
        a.set_mixer(0, rows1[0][5])
        a.set_bandpass(1, 100.0, 200.0)
        a.set_mode(2, P.DM_LSB)
        with pytest.raises(P.PebbleGpuError) as e:
            a.set_bandpass(3, 3000.0, 300.0)
        assert e.value.code == E_FILTER_PARAM
        a.set_mixer(4, 1.2e6)
        sf = a.superframe
        for k, n_sf in enumerate((2, 3)):
            rest = x[(1 + 2 * k) * sf:]
            ra += run_calls(a, rest, [n_sf])
            rb += run_calls(b, rest, [n_sf])
    finally:
        a.close()
        b.close()
    assert np.array_equal(bits(ra[0]["sm"]), bits(rb[0]["sm"])) and check_own(oracle_mod, rows0, ra[0]["sm"], ra[0]["spec"]) <= TOL_REDUCTION
    for k in (1, 2):
        assert np.array_equal(bits(ra[k]["spec"]), bits(rb[k]["spec"]))
        check_own(oracle_mod, rows1, ra[k]["sm"], ra[k]["spec"], what="changed bank, call %d" % k)      # (every frame, the first included)
        check_own(oracle_mod, rows0, rb[k]["sm"], rb[k]["spec"], what="twin, call %d" % k)
        for c in (2, 5):
            assert np.array_equal(bits(ra[k]["sm"][c]), bits(rb[k]["sm"][c])), (k, c)
        for c in (0, 1, 3, 4):
            assert not np.array_equal(bits(ra[k]["sm"][c, 0]), bits(rb[k]["sm"][c, 0])), (k, c)      # ... and does differ from the old window's


# ------------------------------------------------------------------------------------------------
# 5. routes: a few sentinel rows through every way a call with a spectrum can go
# ------------------------------------------------------------------------------------------------
CALLS = [1, 1, 1, 3]


@functools.lru_cache(maxsize=None)
def raw_input(n_frames):
    """(int16 [1, n, 2] raw pairs, complex64 [n]: the same samples as normalizeIQ converts them)"""
    x = signal(tuple(SENTINELS), n_frames, 41)
    raw = np.round(np.stack([x.real, x.imag], axis=-1) * 30000.0).astype(np.int16)[None]
    return raw, host_convert(raw, IQ_S16, 0, 1.0)[0]


def run_route(P, route):
    rows = [S.row(n) for n in SENTINELS]
    rx = make_bank(P, rows, 2048)
    try:
        sf, fps = rx.superframe, rx.superframe // N
        raw, x = raw_input(sum(CALLS) * fps)
        if route == "gated":
            rx.set_spectrum_updates(20)
        if route == "single-stream":
            rx.set_profiling(True)
        if route != "raw":
            return rows, fps, run_calls(rx, x, CALLS)
        out, at = [], 0
        buf = P.DeviceBuffer.from_array(raw, 0)
        try:
            for k in CALLS:
                rx.process_raw_device(buf.ptr + at * sf * 4, k * sf, IQ_S16, 0, 1.0)
                out.append(dict(sm=rx.signal_strength(), spec=rx.spectrum(), audio=rx.audio(), frames=list(rx.spectrum_frames()), at=at * fps, k=k))
                at += k
        finally:
            buf.free()
        return rows, fps, out
    finally:
        rx.close()


@functools.lru_cache(maxsize=None)
def plain_route():
    import pebblesdr_amd as P
    return run_route(P, "plain")


@pytest.mark.parametrize("route", ["plain", "raw", "single-stream", "gated"])
def test_sentinel_rows_on_every_route(gpu_lib, oracle_mod, route):
    import pebblesdr_amd as P
    rows, fps, plain = plain_route()
    _, _, res = (rows, fps, plain) if route == "plain" else run_route(P, route)
    timer = GateTimer(N, FS)
    if route == "gated":
        timer.set_updates(20)
    same_rows = n_rows = 0
    for k, (r, q) in enumerate(zip(res, plain)):
        sel = timer.call(r["k"] * fps)
        assert r["frames"] == sel and r["sm"].shape == (len(rows), len(sel), 4), (route, k, r["frames"], sel)      # (a gated call may compute no row)
        if not sel:
            continue
        check_own(oracle_mod, rows, r["sm"], r["spec"], what="%s call %d" % (route, k))
        for i, f in enumerate(sel):
            n_rows += 1
            if np.array_equal(bits(r["spec"][0, i]), bits(q["spec"][0, f])):
                same_rows += 1
                assert np.array_equal(bits(r["sm"][:, i]), bits(q["sm"][:, f])), (route, k, f)
    print("%s: %d rows, %d with the plain route's dB bits (their S-meter entries then equal bit for bit)" % (route, n_rows, same_rows))
    if route in ("plain", "raw"):
        assert same_rows == n_rows == sum(CALLS) * fps
    if route == "gated":                               # 20 per second at 1 ms per frame: frames 50, 100, 150; two calls compute no row
        assert [len(r["frames"]) for r in res].count(0) >= 2 and n_rows == (sum(CALLS) * fps - 1) // 50


# ------------------------------------------------------------------------------------------------
# 6. the squelch on degenerate windows, through the three gates
# ------------------------------------------------------------------------------------------------
GATE_ROWS = [("clamped", FS, 2048, S.USB[0], S.USB[1], 1.2e6, "bp0_no_bin"), ("one_bin", FS, 2048, 100.0, 200.0, 100e3, "bp0_one_bin"),
             ("open", FS, 2048, S.USB[0], S.USB[1], 100e3, "centred")]
GATE_THRESHOLDS = [-60.0, -1.0, None]


def gate_signal(n_frames):
    t = np.arange(n_frames * N, dtype=np.float64) / FS
    x = 0.05 * np.exp(2j * np.pi * 100150.0 * t) + 0.05 * np.exp(2j * np.pi * 101650.0 * t) + lcg_noise(n_frames * N, 51, 1e-3)
    return x.astype(np.complex64)


@pytest.mark.parametrize("which", [0, 1])
def test_one_channel_gate_on_a_degenerate_window(gpu_lib, oracle_mod, which):
    """the host read-back (one channel, one super-frame per call).  Mixer bin clamped to `bins`: avg is -120, a threshold of -60 closes every
    call -- no audio, from the device and from the oracle's receiver.  bpBins == 0 with a bin in band: avg is 0 dB, open even at -1"""
    import pebblesdr_amd as P
    r, thr = GATE_ROWS[which], GATE_THRESHOLDS[which]
    S.check_class(r)
    rx = P.ReceiverBank(FS, 1, True, False, 2048, max_superframes=1)
    ref = oracle_mod.Receiver(FS, N, 2048)
    try:
        set_window(P, rx, 0, r)
        ref.set_mode(oracle_mod.USB); ref.set_mixer(r[5]); ref.set_filter(r[3], r[4])
        rx.set_squelch(0, thr); ref.set_squelch(thr)
        sf = rx.superframe
        x = gate_signal(3 * sf // N)
        for k in range(3):
            blk = x[k * sf:(k + 1) * sf]
            got = rx.process(blk)[0][0]
            want = sum(len(ref.process(blk[f * N:(f + 1) * N].astype(np.complex128), want_spectrum=False)[0]) for f in range(sf // N))
            sm = rx.signal_strength()
            assert np.isfinite(sm).all() and sm[0, -1, 1] == np.float32(S.expected(r[6])[1])
            assert len(got) == want, (k, len(got), want)
            assert (len(got) == 0) == (which == 0), (k, len(got))
    finally:
        rx.close()


@pytest.mark.parametrize("gated", [False, True])
def test_bank_gate_on_degenerate_windows(gpu_lib, oracle_mod, gated):
    """k_gate_eval (every frame has a row) and k_gate_eval_rows (under the update gate, 20 rows per second: frames 50, 100, 150 -- the first
    super-frame has no row yet and stays open, the third reads the carried row).  Channel 0 (mixer clamped, threshold -60): zeros wherever
    a row exists; channel 1 (one bin in band, threshold -1) and channel 2 (no threshold) deliver throughout"""
    import pebblesdr_amd as P
    for r in GATE_ROWS:
        S.check_class(r)
    rx = make_bank(P, GATE_ROWS, 2048)
    try:
        for c, thr in enumerate(GATE_THRESHOLDS):
            if thr is not None:
                rx.set_squelch(c, thr)
        if gated:
            rx.set_spectrum_updates(20)
        sf, fps, spf = rx.superframe, rx.superframe // N, rx.superframe // rx.D
        x = gate_signal(sum(CALLS) * fps)
        res = run_calls(rx, x, CALLS)
    finally:
        rx.close()
    timer = GateTimer(N, FS)
    if gated:
        timer.set_updates(20)
    have_row, n_closed, n_open0 = False, 0, 0
    for k, r in enumerate(res):
        sel = timer.call(r["k"] * fps)
        assert r["frames"] == sel and np.isfinite(r["sm"]).all()
        if sel:
            check_own(oracle_mod, GATE_ROWS, r["sm"], r["spec"], what="call %d" % k)
        assert r["audio"].shape == (3, r["k"] * spf)
        for j in range(r["k"]):
            have_row = have_row or any(f <= (j + 1) * fps - 1 for f in sel)
            seg = r["audio"][:, j * spf:(j + 1) * spf]
            assert seg[1].any() and seg[2].any(), (k, j)
            assert seg[0].any() != have_row, (gated, k, j, have_row)
            n_closed += int(have_row)
            n_open0 += int(not have_row)
    assert (n_closed, n_open0) == ((sum(CALLS) - 1, 1) if gated else (sum(CALLS), 0))
    if not gated:                                     # the oracle's receiver does the same, channel by channel
        for c, (r, thr) in enumerate(zip(GATE_ROWS, GATE_THRESHOLDS)):
            ref = oracle_mod.Receiver(FS, N, 2048)
            ref.set_mode(oracle_mod.USB); ref.set_mixer(r[5]); ref.set_filter(r[3], r[4])
            if thr is not None:
                ref.set_squelch(thr)
            got = sum(len(ref.process(x[f * N:(f + 1) * N].astype(np.complex128), want_spectrum=False)[0]) for f in range(sum(CALLS) * fps))
            assert (got == 0) == (c == 0), (c, got)


# ------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(gpu_lib, oracle_mod):
    import pebblesdr_amd as P

    def refused(code, fn, *a):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*a)
        assert e.value.code == code, e.value

    rows = [S.row("usb_centred"), S.row("mixer_beyond_half_rate")]
    nos = P.ReceiverBank(FS, 2, True, False, 0, max_superframes=1)                  # no spectrum (the two-stage route): nothing to measure on
    try:
        for c, r in enumerate(rows):
            set_window(P, nos, c, r)
        refused(E_INVALID, nos.enable_signal_strength, True)
        refused(E_INVALID, nos.set_squelch, 0, -50.0)
        x = signal(("usb_centred",), nos.superframe // N, 61)
        a, sp = nos.process(x)
        assert sp is None and a.shape[0] == 2 and a.any() and nos.signal_strength().size == 0
    finally:
        nos.close()
    rx = make_bank(P, rows, 2048, max_sf=1)
    try:
        refused(E_INVALID, rx.set_squelch, 2, -50.0)                                # channel out of range
        refused(E_INVALID, rx.set_mixer, 2, 1000.0)
        refused(E_INVALID, rx.set_bandpass, 2, 300.0, 3000.0)
        refused(E_INVALID, rx.set_mode, 2, P.DM_USB)
        a, sp = rx.process(x)
        assert check_own(oracle_mod, rows, rx.signal_strength(), sp) <= TOL_REDUCTION and a.any()
    finally:
        rx.close()
