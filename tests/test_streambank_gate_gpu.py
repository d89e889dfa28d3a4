"""GPU tier (-m gpu): the stream bank's update gate (pebblegpu_streambank_set_spectrum_updates) against the unchanged oracle.

Which frames get a spectrum: tests/streambank_gate_ref.py (the receiver's rule, one timer per bank, plus `skip` for calls without the
spectrum).  What the spectra are: oracle.Spectrum fed ONLY the selected frames, in order -- FFT::fftSpectrum averages with the
previous frame it was given (fft.cpp:378-386), which behind the timer is the previous selected frame.  Bar: test_parity_gpu.py's
TOL_DB (0.1 dB) over bins the oracle puts above -110 dB; the first row a handle ever computes is not compared (its predecessor is
undefined in the reference).  The band-pass output must equal an ungated twin's bit for bit, and raw routes a
gated float2 bank's bit for bit.  All at fs = 2 MHz: a 65536-sample frame is 32.768 ms, a 2048-sample frame 1.024 ms."""
import functools

import numpy as np
import pytest

from tests.signals import lcg_noise, tones
from tests.streambank_gate_ref import BankGateTimer
from tests.test_parity_gpu import TOL_DB, db_err
from tests.test_screen_map_gpu import check as check_map
from tests.test_streambank_raw_gpu import GAIN, TAG, host_convert, make_raw

pytestmark = pytest.mark.gpu

FS = 2.0e6
N65 = 65536
BIG_LIST = "k_big256_cols_list + k_big256_rows"


@functools.lru_cache(maxsize=None)
def signal(S, n, seed=0):
    """[S, n] complex64, a different tone set per stream (read-only: shared between tests)"""
    x = np.stack([tones(FS, n, [(0.4, 123456.7 * (c + 1)), (0.01, -700001.3 + 1000.0 * seed), (0.2, 20000.0 - 30000.0 * c), (0.1, 1700.0)])
                  + lcg_noise(n, 70 + 3 * seed + c, 1e-4) for c in range(S)]).astype(np.complex64)
    x.setflags(write=False)
    return x


def bank(P, S, frame, bins, F, ups=None):
    sb = P.StreamBank(FS, S, frame=frame, spectrum_bins=bins, max_frames=F)
    for c in range(S):
        sb.set_bandpass(c, -50e3 - 1e3 * c, 50e3 + 2e3 * c)
    if ups is not None:
        sb.set_spectrum_updates(ups)
    return sb


def run_calls(sb, x, calls, timer, frame, twin=None, name=None, twin_rows=None):
    """x in calls (lengths in frames), every selection held to the model -> (rows [S, n_sel, bins], global frame numbers).
    twin: another bank fed the same calls (ungated, or on another route), whose band-pass output must equal sb's bit for bit; its
    spectra are appended to twin_rows."""
    rows, frames, lo = [], [], 0
    for k in calls:
        blk = np.ascontiguousarray(x[:, lo * frame:(lo + k) * frame])
        y, s = sb.process(blk)
        want = timer.call(k)
        assert list(sb.spectrum_frames()) == want, "call at frame %d: frames %s, model %s" % (lo, list(sb.spectrum_frames()), want)
        assert s.shape == (x.shape[0], len(want), s.shape[2])
        if name is not None:
            assert sb.kernel_name(2) == (name if want else "")
        if twin is not None:
            yt, st = twin.process(blk)
            assert np.abs(yt).max() > 1e-3 and np.array_equal(y, yt)
            if twin_rows is not None:
                twin_rows.append(st)
        rows.append(s)
        frames += [lo + i for i in want]
        lo += k
    return np.concatenate(rows, axis=1), frames


def oracle_rows(oracle_mod, x, frames, bins, frame):
    """[S, len(frames), bins]: every stream's listed frames through one oracle.Spectrum each, in order"""
    out = []
    for c in range(x.shape[0]):
        sp = oracle_mod.Spectrum(bins, frame, lift_clamp=True) if frame == N65 else oracle_mod.Spectrum(bins, frame)
        out.append([sp.process(x[c, f * frame:(f + 1) * frame]) for f in frames])
    return np.array(out)


def worst_db(rows, ref, first=1):
    """largest |dB| over every stream's rows from `first` on (the first row a handle computes has no defined predecessor)"""
    assert rows.shape == ref.shape and rows.shape[1] > first
    return max(db_err(rows[c, i], ref[c, i]) for c in range(rows.shape[0]) for i in range(first, rows.shape[1]))


# 1
def test_selection_shapes_and_names(gpu_lib):
    import pebblesdr_amd as P
    S, calls = 2, [3, 1, 4, 2]
    x = signal(3, 10 * N65)[:S]
    sb = bank(P, S, N65, N65, 4)
    assert list(sb.spectrum_frames()) == []   # no call yet
    sb.set_spectrum_updates(20)
    assert list(sb.spectrum_frames()) == []
    t = BankGateTimer(N65, int(FS)); t.set_updates(20)
    rows, frames = run_calls(sb, x, calls, t, N65, name=BIG_LIST)
    assert frames == [2, 4, 6, 8] and rows.shape == (S, 4, N65)
    for want in ([0], []):                    # frames 10 and 11, one call each: the second selects nothing
        y, s = sb.process(x[:, :N65])
        assert t.call(1) == want == list(sb.spectrum_frames())
        assert s.shape == (S, len(want), N65) and y.shape == (S, N65) and sb.kernel_name(2) == (BIG_LIST if want else "")
        assert sb.last_ms(2) >= 0.0 and sb.last_ms(0) >= sb.last_ms(1) > 0.0
    with pytest.raises(P.PebbleGpuError) as e:
        sb.set_spectrum_updates(-2)
    assert e.value.code == -1
    sb.set_spectrum_updates(P.SPECTRUM_EVERY_FRAME)
    _, s = sb.process(x[:, :3 * N65])
    assert s.shape == (S, 3, N65) and list(sb.spectrum_frames()) == [0, 1, 2] and sb.kernel_name(2) == "k_big256_cols + k_big256_rows"
    sb.close()


# 2
def test_gated_65536_rows_against_the_oracle_and_band_pass_bit_identical(gpu_lib, oracle_mod):
    """rows 1..3 of the four computed: the first row of a call behind an empty call (carried predecessor), the second listed row of
    one call (listed predecessor) and the first row of the next call"""
    import pebblesdr_amd as P
    S, calls = 3, [3, 1, 4, 2]
    x = signal(3, 10 * N65)
    sb, twin = bank(P, S, N65, N65, 4, 20), bank(P, S, N65, N65, 4)
    t = BankGateTimer(N65, int(FS)); t.set_updates(20)
    rows, frames = run_calls(sb, x, calls, t, N65, twin=twin, name=BIG_LIST)
    assert frames == [2, 4, 6, 8]
    worst = worst_db(rows, oracle_rows(oracle_mod, x, frames, N65, N65))
    print("gated 65536: %d rows x %d streams, max |dB| %.4f" % (len(frames), S, worst))
    assert worst <= TOL_DB
    sb.close(); twin.close()


# 3
@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 4])
def test_raw_formats_equal_the_gated_float2_bank(gpu_lib, fmt):
    """40 per second selects every frame but the first: 3, 3 and 1 listed frames, so odd counts reach the 8-bit pairing.  Format 0
    also goes through the pinned slots."""
    import pebblesdr_amd as P
    S, calls, order = 2, [4, 3, 1], fmt % 2
    raw = make_raw(fmt, S, sum(calls) * N65, 200 + fmt)
    x = host_convert(raw, fmt, order, GAIN[fmt])
    a, b = bank(P, S, N65, N65, 4, 40), bank(P, S, N65, N65, 4, 40)
    c = bank(P, S, N65, N65, 4, 40) if fmt == 0 else None
    t = BankGateTimer(N65, int(FS)); t.set_updates(40)
    name = "k_big256_cols_list (raw %s) + k_big256_rows" % TAG[fmt]
    lo = 0
    for call, k in enumerate(calls):
        n = k * N65
        blk = np.ascontiguousarray(raw[:, lo:lo + n])
        want = t.call(k)
        yb, sb_ = b.process(np.ascontiguousarray(x[:, lo:lo + n]))
        buf = P.DeviceBuffer.from_array(blk, 0)
        try:
            a.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt])
            ya, sa = a.filtered(), a.spectrum()
        finally:
            buf.free()
        assert list(a.spectrum_frames()) == want == list(b.spectrum_frames()) and len(want) == (3, 3, 1)[call]
        assert (a.kernel_name(1), a.kernel_name(2)) == ("k_fastfir_t128 (raw %s)" % TAG[fmt], name) and b.kernel_name(2) == BIG_LIST
        assert sa.shape == (S, len(want), N65) and sb_.max() > -100.0 and np.abs(yb).max() > 1e-3
        assert np.array_equal(sa, sb_) and np.array_equal(ya, yb)
        if c is not None:
            c.ingest_acquire(call & 1, blk.nbytes, np.int8)[:] = blk.reshape(-1)
            c.ingest_submit(call & 1, blk.nbytes)
            c.process_ingested(call & 1, n, fmt, order, GAIN[fmt])
            assert list(c.spectrum_frames()) == want and c.kernel_name(2) == name
            assert np.array_equal(c.spectrum(), sb_) and np.array_equal(c.filtered(), yb)
        lo += n
    for s in (a, b, c):
        if s is not None:
            s.close()


# 4
def test_a_list_longer_than_one_launch_65536(gpu_lib, oracle_mod):
    """one call of 66 frames at 40 per second: 65 rows, two launches of pass A (64 + 1) into one compact Y"""
    import pebblesdr_amd as P
    x = signal(1, 66 * N65, 1)
    sb = bank(P, 1, N65, N65, 66, 40)
    t = BankGateTimer(N65, int(FS)); t.set_updates(40)
    rows, frames = run_calls(sb, x, [66], t, N65, name=BIG_LIST)
    assert frames == list(range(1, 66)) and rows.shape == (1, 65, N65)
    worst = worst_db(rows, oracle_rows(oracle_mod, x, frames, N65, N65))
    print("65 listed 65536-point rows: max |dB| %.4f" % worst)
    assert worst <= TOL_DB
    sb.close()


def test_a_list_longer_than_one_launch_2048(gpu_lib, oracle_mod):
    """2048-sample frames, 8192 bins, 5000 per second (period 0): one call of 130 frames -> 129 rows in three launches"""
    import pebblesdr_amd as P
    S = 2
    x = signal(3, 130 * 2048, 2)[:S]
    sb = bank(P, S, 2048, 8192, 130, 5000)
    t = BankGateTimer(2048, int(FS)); t.set_updates(5000)
    rows, frames = run_calls(sb, x, [130], t, 2048, name="k_spectrum_list_q128")
    assert frames == list(range(1, 130))
    assert worst_db(rows, oracle_rows(oracle_mod, x, frames, 8192, 2048)) <= TOL_DB
    sb.close()


# 5
@pytest.mark.parametrize("frame,bins", [(2048, 2048), (2048, 4096), (2048, 8192), (4096, 8192)])
def test_short_frames_through_the_list_kernels(gpu_lib, oracle_mod, frame, bins):
    """2048-sample frames at 250 per second (every fourth frame) in calls of 6, 2, 9 and 4 frames; 4096-sample frames take the
    general list kernel"""
    import pebblesdr_amd as P
    S, calls = 2, [6, 2, 9, 4]
    x = signal(3, 21 * frame, 3)[:S]
    sb, twin = bank(P, S, frame, bins, 9, 250), bank(P, S, frame, bins, 9)
    t = BankGateTimer(frame, int(FS)); t.set_updates(250)
    rows, frames = run_calls(sb, x, calls, t, frame, twin=twin, name="k_spectrum_list_q128" if frame == 2048 else "k_spectrum_list_any")
    if frame == 2048:
        assert frames == [4, 8, 12, 16, 20]
    assert len(frames) >= 4
    worst = worst_db(rows, oracle_rows(oracle_mod, x, frames, bins, frame))
    print("frame %d bins %d: %d gated rows, max |dB| %.4f" % (frame, bins, len(frames), worst))
    assert worst <= TOL_DB
    sb.close(); twin.close()


def test_a_staged_raw_call_on_short_frames(gpu_lib):
    """4096 bins have no converting every-frame kernel, so a raw call is staged through k_normalize_iq under the gate too"""
    import pebblesdr_amd as P
    S, calls, fmt, order = 2, [6, 2, 9, 4], 2, 1
    raw = make_raw(fmt, S, sum(calls) * 2048, 300)
    x = host_convert(raw, fmt, order, GAIN[fmt])
    a, b = bank(P, S, 2048, 4096, 9, 250), bank(P, S, 2048, 4096, 9, 250)
    t = BankGateTimer(2048, int(FS)); t.set_updates(250)
    lo = 0
    for k in calls:
        n = k * 2048
        want = t.call(k)
        buf = P.DeviceBuffer.from_array(np.ascontiguousarray(raw[:, lo:lo + n]), 0)
        try:
            a.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt])
            ya, sa = a.filtered(), a.spectrum()
        finally:
            buf.free()
        yb, sb_ = b.process(np.ascontiguousarray(x[:, lo:lo + n]))
        assert list(a.spectrum_frames()) == want and a.kernel_name(2) == ("k_normalize_iq + k_spectrum_list_q128" if want else "")
        assert sa.shape == (S, len(want), 4096) and np.array_equal(sa, sb_) and np.array_equal(ya, yb)
        lo += n
    a.close(); b.close()


# 6
def test_rows_do_not_depend_on_the_split_into_calls(gpu_lib):
    import pebblesdr_amd as P
    S = 2
    x = signal(3, 10 * N65)[:S]
    out = []
    for calls in ([3, 1, 4, 2], [5, 5]):
        sb = bank(P, S, N65, N65, 5, 20)
        t = BankGateTimer(N65, int(FS)); t.set_updates(20)
        out.append(run_calls(sb, x, calls, t, N65))
        sb.close()
    assert out[0][1] == out[1][1] == [2, 4, 6, 8]
    assert out[0][0].max() > -100.0 and np.array_equal(out[0][0], out[1][0])


# 7
def test_rate_changes_keep_the_timer_and_the_carried_amplitudes(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    S = 2
    x = signal(3, 11 * N65, 4)[:S]
    sb = bank(P, S, N65, N65, 4)
    t = BankGateTimer(N65, int(FS))
    rows, frames, lo, sels = [], [], 0, []
    for ups, k in ((20, 3), (0, 2), (10, 4), (P.SPECTRUM_EVERY_FRAME, 2)):
        sb.set_spectrum_updates(ups); t.set_updates(ups)
        r, f = run_calls(sb, x[:, lo * N65:], [k], t, N65)
        rows.append(r); sels.append(f); frames += [lo + i for i in f]
        lo += k
    assert sels == [[2], [], [1], [0, 1]] and frames == [2, 6, 9, 10]
    rows = np.concatenate(rows, axis=1)
    worst = worst_db(rows, oracle_rows(oracle_mod, x, frames, N65, N65))
    print("rate changes: max |dB| %.4f" % worst)
    assert worst <= TOL_DB
    sb.close()


# 8
def test_calls_without_the_spectrum_advance_the_clock_only(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    S = 2
    x = signal(3, 10 * N65)[:S, :8 * N65]
    sb, twin = bank(P, S, N65, N65, 3, 20), bank(P, S, N65, N65, 3)
    t = BankGateTimer(N65, int(FS)); t.set_updates(20)
    r0, f0 = run_calls(sb, x[:, :3 * N65], [3], t, N65, twin=twin)
    y, s = sb.process(x[:, 3 * N65:5 * N65], what=1)
    t.skip(2)
    yt, _ = twin.process(x[:, 3 * N65:5 * N65], what=1)
    assert s is None and np.array_equal(y, yt) and list(sb.spectrum_frames()) == [] and sb.kernel_name(2) == ""
    with pytest.raises(P.PebbleGpuError):
        sb.map_spectrum(255, 512, 0.0, -120.0, -10**6, 10**6)   # the last call did not ask for the spectrum
    r1, f1 = run_calls(sb, x[:, 5 * N65:], [3], t, N65, twin=twin)
    assert (f0, f1) == ([2], [0, 2])
    rows = np.concatenate([r0, r1], axis=1)
    assert worst_db(rows, oracle_rows(oracle_mod, x, [2, 5, 7], N65, N65)) <= TOL_DB
    sb.close(); twin.close()


# 9
def test_the_map_indexes_compact_rows_and_keeps_the_latest(gpu_lib):
    import pebblesdr_amd as P
    S = 2
    x = signal(3, 10 * N65)[:S]
    sb = bank(P, S, N65, N65, 4, 20)
    args = (255, 1024, 0.0, -120.0, -400000, 600000)
    sb.process(x[:, :N65])                     # frame 0 starts the timer: nothing computed yet
    with pytest.raises(P.PebbleGpuError) as e:
        sb.map_spectrum(*args)
    assert e.value.code == -1
    _, s = sb.process(x[:, N65:5 * N65])       # frames 1..4: rows for 2 and 4
    assert list(sb.spectrum_frames()) == [1, 3]
    got = sb.map_spectrum(*args, first_frame=0, n_frames=2)
    assert got.shape == (S, 2, 1024) and len(np.unique(got)) > 8
    check_map(got, s, N65, FS, *args, "both compact rows")
    with pytest.raises(P.PebbleGpuError):
        sb.map_spectrum(*args, first_frame=1, n_frames=2)   # there are two rows, not four
    _, e0 = sb.process(x[:, 5 * N65:6 * N65])  # frame 5: empty
    assert e0.shape == (S, 0, N65)
    latest = sb.map_spectrum(*args)
    assert latest.shape == (S, 1, 1024)
    check_map(latest[:, 0], s[:, -1], N65, FS, *args, "the latest row behind an empty call")
    assert np.array_equal(latest[:, 0], got[:, 1])
    with pytest.raises(P.PebbleGpuError):
        sb.map_spectrum(*args, first_frame=1, n_frames=1)   # only frame 0 exists there
    sb.close()


# 10
@pytest.mark.parametrize("switch,value", [("PEBBLEGPU_BIG_BATCH_MB", "1"), ("PEBBLEGPU_SB_SIDE", "1"), ("PEBBLEGPU_BIG_SPLIT32", "1")])
def test_switches(gpu_lib, oracle_mod, monkeypatch, switch, value):
    """stream batches sized by the compact Y (1 MiB: two streams of one listed frame, one stream of two) and the side-by-side route
    equal the default bit for bit; under BIG_SPLIT32 the listed transform still takes the 256 x 256 kernels, held to the oracle"""
    import pebblesdr_amd as P
    S, calls = 3, [3, 1, 4, 2]
    x = signal(3, 10 * N65)
    monkeypatch.setenv(switch, value)
    a = bank(P, S, N65, N65, 4, 20)
    monkeypatch.delenv(switch)
    b = bank(P, S, N65, N65, 4, 20)
    t = BankGateTimer(N65, int(FS)); t.set_updates(20)
    rb = []
    ra, fa = run_calls(a, x, calls, t, N65, twin=b, name=BIG_LIST, twin_rows=rb)   # (the twin is the gated default route)
    rb = np.concatenate(rb, axis=1)
    assert fa == [2, 4, 6, 8] and rb.shape == ra.shape and rb.max() > -100.0
    if switch == "PEBBLEGPU_BIG_SPLIT32":
        assert worst_db(ra, oracle_rows(oracle_mod, x, fa, N65, N65)) <= TOL_DB
    else:
        assert np.array_equal(ra, rb)
    a.close(); b.close()
