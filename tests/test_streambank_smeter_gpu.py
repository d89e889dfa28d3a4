"""GPU tier (-m gpu): the stream bank's S-meter (k_stream_strength), its squelch gate (k_stream_gate_eval, the gated k_iq_pack) and
the IQ block's trailer, against the unchanged oracle.

Shapes: 3 streams of 2048-sample frames at 2.048 Msps, at most 4 frames per call, 2048 and 8192 bins; 2 streams of 65536 / 65536 at
200 Msps, 2 frames per call (the k_big256_* route).  Per stream one tone INSIDE the stream's band-pass whose amplitude doubles from frame
to frame (6 dB), plus LCG noise at 1e-3; the band-passes are the windows of tests/test_streambank_smeter_host.py; the empty one -- (100, 200):
no noise bin -- has a test of its own, test_the_empty_window.

Bounds.  The reduction alone -- every float4 against oracle.fd_estimate on the device's OWN dB row -- 1e-4 dB, the bound of
test_parity_gpu.py::test_signal_strength_per_frame (b).  End to end -- against fd_estimate on the oracle's spectrum of the same frames --
TOL_DB (0.1 dB), from the second computed row on (the first has no averaged predecessor).  Everything else is bit for bit.
"""
import functools

import numpy as np
import pytest

from tests.signals import lcg_noise
from tests.test_parity_gpu import TOL_DB
from tests.test_streambank_egress_gpu import as_c64
from tests.test_streambank_gate_gpu import oracle_rows
from tests.test_streambank_raw_gpu import GAIN, host_convert, make_raw

pytestmark = pytest.mark.gpu

E_INVALID, E_SIZE = -1, -5
TOL_REDUCTION = 1e-4
# key: (sample rate, streams, frame, bins, max_frames, [(lo, hi, tone Hz)], calls in frames, IQ ring selection)
SHAPES = {
    "2048": (2048000.0, 3, 2048, 2048, 4, [(-5000, 5000, 1000.0), (-900000, 900000, 300e3), (300000, 1000000, 600e3)], [4, 1, 3], [2, 0, 1]),
    "8192": (2048000.0, 3, 2048, 8192, 4, [(-1, 1, 0.0), (-1023000, -1000000, -1010e3), (-5000, 5000, 1000.0)], [4, 1, 3], [2, 0, 1]),
    "65536": (200e6, 2, 65536, 65536, 2, [(-40e6, 40e6, 5e6), (10e6, 10.1e6, 10.05e6)], [2, 1, 2], [1, 0]),
}
FIELDS = ["peak_db", "avg_db", "snr_db", "floor_db"]


@functools.lru_cache(maxsize=None)
def signal(key):
    """[S, total frames * frame] complex64 (read-only): stream s's tone has amplitude 0.4 / (1 + s / 4) in the last frame and half of the
    next frame's in every frame before"""
    fs, S, frame, _, _, wins, calls, _ = SHAPES[key]
    T = sum(calls)
    t = np.arange(T * frame, dtype=np.float64) / fs
    out = []
    for s in range(S):
        amp = np.repeat(0.4 / (1.0 + 0.25 * s) * 2.0 ** (np.arange(T) - (T - 1)), frame)
        out.append(amp * np.exp(2j * np.pi * wins[s][2] * t) + lcg_noise(T * frame, 900 + 7 * s, 1e-3))
    x = np.stack(out).astype(np.complex64)
    x.setflags(write=False)
    return x


def make_bank(P, key, smeter=True, thresholds=None, fmt=None, ups=None):
    fs, S, frame, bins, F, wins, _, sel = SHAPES[key]
    sb = P.StreamBank(fs, S, frame=frame, spectrum_bins=bins, max_frames=F)
    for s in range(S):
        sb.set_bandpass(s, wins[s][0], wins[s][1])
    if ups is not None:
        sb.set_spectrum_updates(ups)
    if smeter:
        sb.enable_signal_strength(True)
    for s, th in enumerate(thresholds or []):
        if th is not None:
            sb.set_squelch(s, th)
    if fmt is not None:
        sb.iq_out_open(fmt, sel, n_slots=2)
    return sb


def take(sb, k, gated=True):
    """IQ block k and (S-meter on) its trailer, read while the block is handed out"""
    got = sb.iq_out_next(True)
    assert got is not None and got[:2] == (k, 0)
    gate = sb.iq_out_gate(k) if gated else None
    sb.iq_out_release(k)
    return got[2], gate


def run_calls(P, sb, key, calls=None, whats=None, ring=True, gated=True):
    """the shape's signal in its calls -> per call dict(y, s, frames, sm, block, gate); read after every call"""
    frame = SHAPES[key][2]
    x, at, out = signal(key), 0, []
    for k, frames in enumerate(calls or SHAPES[key][6]):
        what = whats[k] if whats else 3
        y, s = sb.process(x[:, at * frame:(at + frames) * frame], what)
        r = dict(y=y, s=s, frames=list(sb.spectrum_frames()), sm=sb.signal_strength(), at=at, n=frames, what=what)
        if ring:
            r["block"], r["gate"] = take(sb, k, gated and bool(what & 1))
        out.append(r)
        at += frames
    return out


@functools.lru_cache(maxsize=None)
def reference(key):
    """the shape's calls through a bank with the S-meter on, no threshold, the F32 ring open (computed once, shared)"""
    import pebblesdr_amd as P
    sb = make_bank(P, key, fmt=P.AUDIO_F32)
    try:
        return run_calls(P, sb, key)
    finally:
        sb.close()


@functools.lru_cache(maxsize=None)
def oracle_values(key):
    """[S, total frames, 4]: fd_estimate on the oracle's spectrum of every frame"""
    import oracle
    oracle.build()
    fs, S, frame, bins, _, wins, calls, _ = SHAPES[key]
    rows = oracle_rows(oracle, signal(key), list(range(sum(calls))), bins, frame)
    return np.array([[oracle.fd_estimate(rows[s, f], int(round(fs)), np.float32(wins[s][0]), np.float32(wins[s][1]), 0.0) for f in range(rows.shape[1])]
                     for s in range(S)])


def own_values(oracle_mod, key, s_rows):
    """fd_estimate on the device's own dB rows [S, rows, bins] -> [S, rows, 4]"""
    fs, S, _, _, _, wins, _, _ = SHAPES[key]
    return np.array([[oracle_mod.fd_estimate(s_rows[s, f].astype(np.float64), int(round(fs)), np.float32(wins[s][0]), np.float32(wins[s][1]), 0.0)
                      for f in range(s_rows.shape[1])] for s in range(S)])


def gate_values(g):
    return np.stack([g[f] for f in FIELDS], axis=-1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# 4
@pytest.mark.parametrize("key", list(SHAPES))
def test_against_the_oracle(gpu_lib, oracle_mod, key):
    ref = reference(key)
    S = SHAPES[key][1]
    sm = np.concatenate([r["sm"] for r in ref], axis=1)
    spec = np.concatenate([r["s"] for r in ref], axis=1)
    assert sm.shape == (S, sum(SHAPES[key][6]), 4) and np.isfinite(sm).all()
    own = own_values(oracle_mod, key, spec)
    worst_own = float(np.abs(sm - own).max())
    end = oracle_values(key)
    worst_end = float(np.abs(sm[:, 1:] - end[:, 1:]).max())
    print("%s bins: reduction max |dB| %.3e (<= %g), end to end from row 1 max |dB| %.4f (<= %g)" % (key, worst_own, TOL_REDUCTION, worst_end, TOL_DB))
    assert worst_own <= TOL_REDUCTION
    assert worst_end <= TOL_DB
    for r in ref:                                   # every frame has its own row; the trailer is the S-meter's floats, all open
        sel = SHAPES[key][7]
        assert r["gate"].shape == (len(sel), r["n"])
        assert np.array_equal(bits(gate_values(r["gate"])), bits(r["sm"][sel]))
        assert (r["gate"]["open"] == 1).all() and np.array_equal(r["gate"]["row"], np.tile(np.arange(r["n"], dtype=np.uint32), (len(sel), 1)))
        assert np.array_equal(bits(as_c64(r["block"])), bits(r["y"][sel]))
    assert float(sm[:, :, 0].max()) > -40.0 and float(np.ptp(sm[:, :, 1], axis=1).min()) > 15.0    # a real meter, not a constant


def test_the_empty_window(gpu_lib, oracle_mod):
    """(100, 200) at 2048 bins of 1000 Hz: bpBins == 0, one bin in band, no noise bin.  avg is x / 0 = +inf -> 0 dB, and the noise average
    0 / 0, which the reference's qBound returns as its lower bound: snr 0, floor -120, nothing NaN.  An avg of 0 dB stays open at any
    threshold up to 0; the stream next to it, (-5000, 5000) with a threshold of 50, closes"""
    import pebblesdr_amd as P
    fs, frame, bins, F = 2048000.0, 2048, 2048, 3
    x = signal("2048")[:2, :F * frame]
    sb = P.StreamBank(fs, 2, frame=frame, spectrum_bins=bins, max_frames=F)
    try:
        sb.set_bandpass(0, 100, 200)
        sb.set_bandpass(1, -5000, 5000)
        sb.enable_signal_strength(True)
        sb.set_squelch(0, -1.0)
        sb.set_squelch(1, 50.0)
        sb.iq_out_open(P.AUDIO_F32, [0, 1], n_slots=2)
        y, s = sb.process(x, 3)
        sm = sb.signal_strength()
        blk, gate = take(sb, 0)
    finally:
        sb.close()
    assert sm.shape == (2, F, 4) and np.isfinite(sm).all()
    for s_, (lo, hi) in enumerate([(100, 200), (-5000, 5000)]):
        for f in range(F):
            own = oracle_mod.fd_estimate(s[s_, f].astype(np.float64), int(fs), np.float32(lo), np.float32(hi), 0.0)
            assert np.isfinite(own).all() and np.abs(sm[s_, f] - own).max() <= TOL_REDUCTION, (s_, f, sm[s_, f], own)
    assert (sm[0, :, 1] == 0.0).all() and (sm[0, :, 2] == 0.0).all() and (sm[0, :, 3] == np.float32(-120.0)).all() and (sm[0, :, 0] < -20.0).all()
    assert np.array_equal(bits(gate_values(gate)), bits(sm)) and (gate[0]["open"] == 1).all() and (gate[1]["open"] == 0).all()
    assert np.array_equal(bits(as_c64(blk)[0]), bits(y[0])) and not blk[1].any()


# 5
@pytest.mark.parametrize("key", ["8192", "65536"])
def test_two_runs_give_the_same_bits(gpu_lib, key):
    import pebblesdr_amd as P
    ref = reference(key)
    sb = make_bank(P, key, fmt=P.AUDIO_F32)
    try:
        again = run_calls(P, sb, key)
    finally:
        sb.close()
    for a, b in zip(ref, again):
        assert a["sm"].size and np.array_equal(bits(a["sm"]), bits(b["sm"]))
        assert a["gate"].tobytes() == b["gate"].tobytes()


# 6
@pytest.mark.parametrize("key", ["8192", "65536"])
def test_float2_raw_and_ingested_calls_give_the_same_bits(gpu_lib, key):
    import pebblesdr_amd as P
    fs, S, frame, bins, F, _, _, _ = SHAPES[key]
    fmt, order, n = 0, 0, F * frame
    raw = make_raw(fmt, S, n, 31, fs=fs)
    x = host_convert(raw, fmt, order, GAIN[fmt])
    f2, rw, ing = (make_bank(P, key) for _ in range(3))
    buf = P.DeviceBuffer.from_array(raw, 0)
    try:
        _, s0 = f2.process(x, 3)
        a = f2.signal_strength()
        rw.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt], 3)
        b = rw.signal_strength()
        ing.ingest_acquire(0, raw.nbytes, np.int8)[:] = raw.reshape(-1)
        ing.ingest_submit(0, raw.nbytes)
        ing.process_ingested(0, n, fmt, order, GAIN[fmt], 3)
        c = ing.signal_strength()
        assert a.shape == (S, F, 4) and np.isfinite(a).all() and float(a[:, :, 0].max()) > -40.0
        assert np.array_equal(bits(s0), bits(rw.spectrum())) and "raw s8" in rw.kernel_name(2)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    finally:
        buf.free()
        for sb in (f2, rw, ing):
            sb.close()


# 7
def test_under_the_update_gate(gpu_lib, oracle_mod):
    """500 spectra per second at 1 ms per frame: every second frame once the timer runs.  Frames 0 | 1 | 2 3 4 5 | 6 | 7: the first call
    runs without the spectrum (bit 1 of `what` clear), frame 1 starts the timer, frames 3, 5 and 7 get rows -- so the third call has a
    frame before any row exists, two rows of its own and a frame that reads the row before it, and the fourth call selects nothing and
    reads the carried row.  Stream 1's threshold of 50 closes every frame that reads a row."""
    import pebblesdr_amd as P
    key = "2048"
    S, sel = SHAPES[key][1], SHAPES[key][7]
    calls, whats = [1, 1, 4, 1, 1], [1, 3, 3, 3, 3]
    sb = make_bank(P, key, thresholds=[None, 50.0, None], fmt=P.AUDIO_F32, ups=500)
    try:
        res = run_calls(P, sb, key, calls, whats)
    finally:
        sb.close()
    counts = [len(r["frames"]) for r in res]
    assert counts == [0, 0, 2, 0, 1] and res[2]["frames"] == [1, 3], (counts, res[2]["frames"])
    carried, seen_carried, seen_own = None, 0, 0
    for k, r in enumerate(res):
        assert r["sm"].shape == (S, counts[k], 4)                                   # one entry per computed row, possibly none
        if counts[k]:
            assert np.abs(r["sm"] - own_values(oracle_mod, key, r["s"])).max() <= TOL_REDUCTION
        g = r["gate"]
        assert g.shape == (len(sel), r["n"])
        for j in range(r["n"]):
            row = sum(1 for f in r["frames"] if f <= j) - 1
            for i, s in enumerate(sel):
                e = g[i, j]
                if row >= 0:
                    want, mark = r["sm"][s, row], row
                    seen_own += 1
                elif carried is not None:
                    want, mark = carried[s], P.GATE_ROW_CARRIED
                    seen_carried += 1
                else:
                    want, mark = np.zeros(4, dtype=np.float32), P.GATE_ROW_NONE
                assert int(e["row"]) == mark, (k, j, s, e)
                assert np.array_equal(bits(gate_values(e)), bits(want)), (k, j, s, e, want)
                assert int(e["open"]) == (1 if mark == P.GATE_ROW_NONE or s != 1 else 0), (k, j, s, e)
        if counts[k]:
            carried = r["sm"][:, -1].copy()
        blk = as_c64(r["block"])
        for i, s in enumerate(sel):
            if s == 1 and k > 0 and (g[i]["open"] == 0).all():
                assert not blk[i].any()
            elif (g[i]["open"] == 1).all():
                assert np.array_equal(bits(blk[i]), bits(r["y"][s]))
    assert (res[0]["gate"]["row"] == P.GATE_ROW_NONE).all() and (res[0]["gate"]["open"] == 1).all()
    assert seen_carried and seen_own


def thresholds_for(key):
    """per stream: a midpoint between two of its avg_db values (stream 0), 50 (stream 1: always closed), -120 (the rest)"""
    ref = reference(key)
    S = SHAPES[key][1]
    avg = np.concatenate([r["sm"] for r in ref], axis=1)[:, :, 1]
    for vals in (avg, oracle_values(key)[:, :, 1]):
        for s in range(S):
            d = np.diff(np.sort(vals[s].astype(np.float64)))
            assert (d > 1.0).all(), "stream %d: avg_db values %s are not 1 dB apart" % (s, np.sort(vals[s]))
    v = np.sort(avg[0].astype(np.float64))
    k = len(v) // 2
    return [float(np.float32((v[k - 1] + v[k]) / 2)), 50.0, -120.0][:S]


# 8
@pytest.mark.parametrize("key,fmt_name", [("2048", "AUDIO_F32"), ("2048", "AUDIO_S16"), ("8192", "AUDIO_S16"), ("65536", "AUDIO_F32")])
def test_squelch(gpu_lib, key, fmt_name):
    import pebblesdr_amd as P
    fmt = getattr(P, fmt_name)
    ref = reference(key)
    frame, sel = SHAPES[key][2], SHAPES[key][7]
    th = thresholds_for(key)
    sb = make_bank(P, key, smeter=False, thresholds=th, fmt=fmt)    # (a threshold above -120 turns the S-meter on)
    try:
        res = run_calls(P, sb, key)
    finally:
        sb.close()
    n_open = n_closed = 0
    for r, q in zip(res, ref):
        assert np.array_equal(bits(r["y"]), bits(q["y"])) and np.array_equal(bits(r["s"]), bits(q["s"]))   # in front of the gate
        assert np.array_equal(bits(r["sm"]), bits(q["sm"]))
        g = r["gate"]
        assert np.array_equal(bits(gate_values(g)), bits(gate_values(q["gate"]))) and np.array_equal(g["row"], q["gate"]["row"])
        for i, s in enumerate(sel):
            for j in range(r["n"]):
                is_open = not (g[i, j]["avg_db"] < np.float32(th[s]))              # the trailer's own float
                assert int(g[i, j]["open"]) == int(is_open), (s, j, g[i, j], th[s])
                got = r["block"][i, j * frame:(j + 1) * frame]
                src = r["y"][s, j * frame:(j + 1) * frame]
                if not is_open:
                    assert not got.any()
                    n_closed += 1
                elif fmt == P.AUDIO_F32:
                    assert np.array_equal(bits(as_c64(got[None])[0]), bits(src))
                    n_open += 1
                else:
                    assert np.array_equal(got, P.iq_record_convert(src))
                    n_open += 1
        if fmt == P.AUDIO_F32 and key != "8192":
            assert np.abs(r["y"][sel]).max() > 1e-4                                  # open frames carry a signal, not zeros
    T = sum(SHAPES[key][6])
    assert n_closed >= T + 1 and n_open >= 2, (n_open, n_closed)                     # stream 1 throughout, stream 0 on both sides of its threshold
    per0 = np.concatenate([r["gate"][sel.index(0)]["open"] for r in res])
    assert per0.min() == 0 and per0.max() == 1


# 9
def test_feature_off_changes_nothing(gpu_lib):
    import pebblesdr_amd as P
    key = "2048"
    never, toggled = make_bank(P, key, smeter=False, fmt=P.AUDIO_S16), make_bank(P, key, smeter=True, fmt=P.AUDIO_S16)
    toggled.set_squelch(0, -30.0)
    toggled.set_squelch(0, -120.0)
    toggled.enable_signal_strength(False)
    frame, x = SHAPES[key][2], signal(key)
    try:
        for k in range(2):
            blk = x[:, 4 * k * frame:4 * (k + 1) * frame]
            out = []
            for sb in (never, toggled):
                y, s = sb.process(blk, 3)
                assert sb.signal_strength().shape[1] == 0
                got = sb.iq_out_next(True)
                assert got is not None and got[0] == k
                with pytest.raises(P.PebbleGpuError) as e:
                    sb.iq_out_gate(k)
                assert e.value.code == E_INVALID
                sb.iq_out_release(k)
                out.append((y, s, got[2], sb.kernel_name(1), sb.kernel_name(2)))
            a, b = out
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
            assert a[3:] == b[3:] and a[3] and a[4]
            assert np.abs(a[2].astype(np.int32)).max() > 100
    finally:
        never.close()
        toggled.close()


# 10
def test_refusals_leave_the_handle_usable(gpu_lib, oracle_mod):
    import pebblesdr_amd as P
    key = "2048"
    fs, S, frame, bins, F, _, _, sel = SHAPES[key]
    x = signal(key)[:, :2 * frame]

    def refused(code, fn, *a):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*a)
        assert e.value.code == code, e.value

    nos = P.StreamBank(fs, 2, frame=frame, spectrum_bins=0, max_frames=2)          # no spectrum: nothing to measure on
    try:
        refused(E_INVALID, nos.enable_signal_strength, True)
        refused(E_INVALID, nos.set_squelch, 0, -50.0)
        nos.set_bandpass(0, -5000, 5000)
        y, _ = nos.process(x[:2], 1)
        assert y.shape == (2, 2 * frame)
    finally:
        nos.close()
    sb = make_bank(P, key, fmt=P.AUDIO_F32)
    try:
        refused(E_INVALID, sb.set_squelch, S, -50.0)
        for bad in (float("nan"), float("inf"), float("-inf")):
            refused(E_INVALID, sb.set_squelch, 0, bad)
        sb.set_squelch(1, -10.0)
        refused(E_INVALID, sb.enable_signal_strength, False)                       # the squelch reads the S-meter
        with pytest.raises(P.PebbleGpuError):
            sb.set_bandpass(0, 5000, -5000)                                        # refused: the window stays (-5000, 5000)
        refused(E_INVALID, sb.iq_out_gate, 0)                                      # nothing queued, nothing handed out
        y, s = sb.process(x, 3)
        refused(E_INVALID, sb.iq_out_gate, 0)                                      # queued, not handed out yet
        got = sb.iq_out_next(True)
        assert got[0] == 0
        refused(E_INVALID, sb.iq_out_gate, 1)
        refused(E_SIZE, sb.iq_out_gate, 0, len(sel) * 2 - 1)
        g = sb.iq_out_gate(0, len(sel) * 2)
        assert g.shape == (len(sel), 2) and (g[sel.index(1)]["open"] == 0).all() and (g[sel.index(0)]["open"] == 1).all()
        assert np.abs(sb.signal_strength() - own_values(oracle_mod, key, s)).max() <= TOL_REDUCTION   # stream 0's window is still what was accepted
        sb.iq_out_release(0)
        refused(E_INVALID, sb.iq_out_gate, 0)                                      # released
        sb.set_squelch(1, -120.0)
        sb.enable_signal_strength(False)
        sb.process(x, 3)
        assert sb.iq_out_next(True)[0] == 1
        refused(E_INVALID, sb.iq_out_gate, 1)                                      # queued while the S-meter was off
        sb.iq_out_release(1)
    finally:
        sb.close()
