"""GPU tier of raw device-format input into a receiver (tests/raw_cases.py is the coverage statement): pebblegpu_receiver_process_raw
on the raw-fused route -- k_mix_hb11_lean<FMT> beside k_spectrum_t128<2, FMT>, both converting in their own loads -- and on the staged
route through k_normalize_iq, for every sample format and IQ order.

The twin everywhere is a second receiver handed raw_cases.host_convert(raw) through process(): audio and spectrum bit for bit
(np.array_equal), call by call.  pebblegpu_receiver_kernel_name(rx, 6) (the input route) and (rx, 2) (the first stage) are asserted
on every call, so a change that quietly stages a fused call, or fuses a staged one, fails here and not in the benchmark.  Five rows
are tied to the oracle instead, with the bars tests/test_parity_gpu.py holds the same receivers to."""
import numpy as np
import pytest

from tests import raw_cases as rc
from tests.test_parity_gpu import TOL, TOL_DB, db_err, rel_rms

pytestmark = pytest.mark.gpu

E_INVALID, E_SIZE = -1, -5
SMALL = "u8-x2-iq"   # 1.024 Msps: the smallest super-frame (32768 samples), for the tests that are about hand-overs and not a stride


def receivers(P, row, n=2, C=1, shared=True, bins=rc.BINS):
    out = []
    for _ in range(n):
        rx = P.ReceiverBank(row.fs, C, shared, row.wfm, bins, max_superframes=rc.MAX_SF)
        for c in range(C):
            rx.set_mixer(c, rc.FC[row.fs])
            if not row.wfm:
                rx.set_mode(c, P.DM_USB)
                rx.set_bandpass(c, 300, 3000)
        out.append(rx)
    return out


def raw_call(P, rx, chunk, fmt, order, gain):
    """one process_raw call from a fresh device buffer -> (audio, spectrum, input route, first-stage kernel, display kernel)"""
    n = chunk.shape[-2]
    buf = P.DeviceBuffer.from_array(np.ascontiguousarray(chunk), 0)
    try:
        rx.process_raw_device(buf.ptr, n, fmt, order, gain)
        return rx.audio(), rx.spectrum(), rx.kernel_name(6), rx.kernel_name(2), rx.kernel_name(1)
    finally:
        buf.free()


def same(got_a, got_s, want_a, want_s, what):
    assert got_a.shape == want_a.shape and np.abs(want_a).max() > 1e-3, what
    assert np.array_equal(got_a, want_a), what
    assert got_s.shape == want_s.shape and want_s.max() > -100.0, what
    assert np.array_equal(got_s, want_s), what


def row_calls(row, sf):
    raw = rc.row_raw(row.name, sf)
    x = rc.host_convert(raw, row.fmt, row.order, rc.GAIN[row.fmt])
    return [(raw[lo:lo + n], x[lo:lo + n]) for lo, n in rc.call_bounds(sf)]


# ---- a. every row against the twin ----
@pytest.mark.parametrize("name", [r.name for r in rc.ROWS])
def test_every_row_call_by_call_against_the_twin(gpu_lib, name):
    """calls of 1, 2, 1, 3 super-frames: call 0 (oscillator transient) is staged and takes k_mix_hb11_bank, calls 1..3 convert in
    the loads of k_mix_hb11_lean<FMT> and k_spectrum_t128<2, FMT>; every call bit for bit the twin's"""
    import pebblesdr_amd as P
    row = rc.ROW[name]
    a, b = receivers(P, row)
    assert a.chain()[0] == (11, row.stride)
    assert a.kernel_name(6) == ""
    for k, (raw, x) in enumerate(row_calls(row, a.superframe)):
        ga, gs, route, front, disp = raw_call(P, a, raw, row.fmt, row.order, rc.GAIN[row.fmt])
        wa, ws = b.process(x)
        assert (route, front) == (rc.input_route(row, k), rc.front_kernel(row, k)), (name, k)
        assert a.input_route() == route
        if k:
            assert disp == "k_spectrum_t128", (name, k)   # the plain two-chain instance: raw input never takes "twiddles held" on a receiver
        assert (b.kernel_name(6), b.kernel_name(2)) == ("float2", rc.front_kernel(row, k)), (name, k)
        same(ga, gs, wa, ws, (name, k))


# ---- b. the oracle tie ----
@pytest.mark.parametrize("name", rc.ORACLE_ROWS)
def test_oracle_tie(gpu_lib, oracle_mod, name):
    """one row per rate and format against oracle.Receiver fed the converted samples: rel-RMS <= TOL per 2048-sample audio frame, the
    first included; <= TOL_DB over the bins the oracle puts above -110 dB, from the run's second spectrum on"""
    import pebblesdr_amd as P
    row = rc.ROW[name]
    (a,) = receivers(P, row, n=1)
    sf = a.superframe
    calls = row_calls(row, sf)
    want_a, want_s = rc.oracle_run(oracle_mod, row, np.concatenate([x for _, x in calls]))
    worst, worst_db, at_a, at_s = 0.0, 0.0, 0, 0
    for k, (raw, _) in enumerate(calls):
        ga, gs, route, front, _ = raw_call(P, a, raw, row.fmt, row.order, rc.GAIN[row.fmt])
        assert (route, front) == (rc.input_route(row, k), rc.front_kernel(row, k))
        ga, gs = ga[0], gs[0]
        assert np.abs(ga).max() > 1e-3
        for i in range(0, len(ga), rc.FRAME):
            worst = max(worst, rel_rms(ga[i:i + rc.FRAME], want_a[at_a + i:at_a + i + rc.FRAME]))
        for f in range(len(gs)):
            if at_s + f:
                worst_db = max(worst_db, db_err(gs[f], want_s[at_s + f]))
        at_a += len(ga)
        at_s += len(gs)
    assert at_a == len(want_a) and at_s == len(want_s)
    print("%s against the oracle: worst rel-RMS per audio frame %.3e, worst |dB| %.4f" % (name, worst, worst_db))
    assert worst <= TOL
    assert worst_db <= TOL_DB


# ---- c. under the update timer ----
@pytest.mark.parametrize("name", rc.GATED_ROWS)
def test_under_the_update_timer(gpu_lib, name):
    """set_spectrum_updates on: the listed frames of a raw call are computed by k_spectrum_list_q128<true> from the raw pairs; the
    selection and the rows are the twin's, bit for bit, and so is the audio"""
    import pebblesdr_amd as P
    row = rc.ROW[name]
    a, b = receivers(P, row)
    for rx in (a, b):
        rx.set_spectrum_updates(100)
    rows = 0
    for k, (raw, x) in enumerate(row_calls(row, a.superframe)):
        ga, gs, route, front, disp = raw_call(P, a, raw, row.fmt, row.order, rc.GAIN[row.fmt])
        fa = a.spectrum_frames()
        wa, ws = b.process(x)
        fb = b.spectrum_frames()
        assert (route, front) == (rc.input_route(row, k), rc.front_kernel(row, k)), (name, k)
        assert len(fb) >= 2 and np.array_equal(fa, fb), (name, k)
        assert disp == b.kernel_name(1) == "k_spectrum_list_q128"
        assert gs.shape == (1, len(fb), rc.BINS)
        same(ga, gs, wa, ws, (name, k))
        rows += len(fb)
    assert rows < sum(rc.SCRIPT) * a.superframe // rc.FRAME // 2   # the gate did select


# ---- d. recording and the RAW_IQ tap ----
@pytest.mark.parametrize("name", rc.RECORD_ROWS)
def test_recording_and_the_raw_iq_tap(gpu_lib, name):
    """the record ring (k_iq_record from the raw pairs) against iq_record_convert(host_convert(raw)) computed on the host, the RAW_IQ
    tap (k_normalize_iq into the tap) against host_convert(raw): on the staged call 0 and on two fused calls"""
    import pebblesdr_amd as P
    row = rc.ROW[name]
    a, b = receivers(P, row)
    a.record_open(4)
    a.set_taps([P.TAP_RAW_IQ])
    for k, (raw, x) in enumerate(row_calls(row, a.superframe)[:3]):
        ga, gs, route, front, _ = raw_call(P, a, raw, row.fmt, row.order, rc.GAIN[row.fmt])
        assert (route, front) == (rc.input_route(row, k), rc.front_kernel(row, k)), (name, k)
        tap, rate = a.tap(P.TAP_RAW_IQ)
        assert rate == row.fs and tap.shape == (1, len(x))
        assert np.array_equal(tap[0].view(np.uint32), np.ascontiguousarray(x).view(np.uint32)), (name, k)
        blk = a.record_next(True)
        assert blk is not None
        idx, dropped, rec = blk
        a.record_release(idx)
        assert (idx, dropped) == (k, 0) and rec.dtype == np.int16 and rec.shape == (1, len(x), 2)
        want = P.iq_record_convert(x)
        assert len(np.unique(want)) > 100
        assert np.array_equal(rec[0], want), (name, k)
        same(ga, gs, *b.process(x), (name, k))


# ---- e. hand-overs on one handle ----
def test_raw_and_float2_calls_alternate(gpu_lib):
    """raw (staged), raw, float2, raw, float2, raw on one handle against float2 throughout on the twin: the ten mixed samples of
    d_hist_mixed and the display transform's carried amplitudes cross routes in both directions"""
    import pebblesdr_amd as P
    row = rc.ROW["s16-x8-iq"]
    a, b = receivers(P, row)
    sf = a.superframe
    raw = rc.row_raw(row.name, sf)[:6 * sf]
    x = rc.host_convert(raw, row.fmt, row.order, rc.GAIN[row.fmt])
    routes = []
    for k in range(6):
        r, xx = raw[k * sf:(k + 1) * sf], x[k * sf:(k + 1) * sf]
        if k in (2, 4):
            ga, gs = a.process(xx)
        else:
            ga, gs = raw_call(P, a, r, row.fmt, row.order, rc.GAIN[row.fmt])[:2]
        routes.append((a.kernel_name(6), a.kernel_name(2)))
        same(ga, gs, *b.process(xx), k)
    lean = "k_mix_hb11_lean"
    assert routes == [("k_normalize_iq", "k_mix_hb11_bank"), ("raw s16", lean), ("float2", lean), ("raw s16", lean), ("float2", lean), ("raw s16", lean)]


def test_the_format_changes_from_call_to_call(gpu_lib):
    """wav16 (staged), then s8, s16, f32, u8 on the fused route of one handle, each in another IQ order: every call picks its own
    instances, and what one leaves (mixed history, carried amplitudes) the next one takes up"""
    import pebblesdr_amd as P
    row = rc.ROW[SMALL]
    a, b = receivers(P, row)
    sf = a.superframe
    plan = [(4, 0), (0, 1), (2, 2), (3, 3), (1, 1)]
    for k, (fmt, order) in enumerate(plan):
        raw = rc.stream_raw(fmt, row.fs, False, sf, 300 + k, first=k * sf)
        rc.plant(raw, fmt, 0)
        rc.plant(raw, fmt, sf - rc.PLANT)
        x = rc.host_convert(raw, fmt, order, rc.GAIN[fmt])
        ga, gs, route, front, _ = raw_call(P, a, raw, fmt, order, rc.GAIN[fmt])
        assert (route, front) == (("k_normalize_iq", "k_mix_hb11_bank") if k == 0 else ("raw " + rc.TAG[fmt], "k_mix_hb11_lean")), k
        same(ga, gs, *b.process(x), k)


def test_a_retune_in_mid_run_is_staged_and_fuses_again(gpu_lib):
    import pebblesdr_amd as P
    row = rc.ROW["f32-x8-iq"]
    a, b = receivers(P, row)
    sf = a.superframe
    raw = rc.row_raw(row.name, sf)
    x = rc.host_convert(raw, row.fmt, row.order, rc.GAIN[row.fmt])
    routes = []
    for k in range(5):
        if k == 2:
            for rx in (a, b):
                rx.set_mixer(0, rc.FC[row.fs] + 1500.0)   # (the tone is 2.5 kHz above the channel now: still inside 300..3000 Hz)
        lo, hi = k * sf, (k + 1) * sf
        ga, gs, route, front, _ = raw_call(P, a, raw[lo:hi], row.fmt, row.order, rc.GAIN[row.fmt])
        routes.append((route, front))
        same(ga, gs, *b.process(x[lo:hi]), k)
    staged, fused = ("k_normalize_iq", "k_mix_hb11_bank"), ("raw f32", "k_mix_hb11_lean")
    assert routes == [staged, fused, staged, fused, fused]


def test_conditioners_on_for_a_call_and_off_again(gpu_lib):
    """a conditioned call reads a conditioned float2 copy of the stream, so it is staged; with the conditioners off again the handle
    returns to the converting loads (the call that applies the switch-off still finds the change pending)"""
    import pebblesdr_amd as P
    row = rc.ROW["wav16-x2-ionly"]
    a, b = receivers(P, row)
    sf = a.superframe
    raw = rc.row_raw(row.name, sf)
    x = rc.host_convert(raw, row.fmt, row.order, rc.GAIN[row.fmt])
    routes = []
    for k in range(6):
        if k in (2, 3):
            for rx in (a, b):
                rx.set_conditioners(0, 1 if k == 2 else 0)
        lo, hi = k * sf, (k + 1) * sf
        ga, gs, route, front, _ = raw_call(P, a, raw[lo:hi], row.fmt, row.order, rc.GAIN[row.fmt])
        routes.append(route)
        same(ga, gs, *b.process(x[lo:hi]), k)
    # call 2 is conditioned; call 3 switches the conditioner off but is planned with the change still pending (CallFacts::cond_dirty)
    assert routes == ["k_normalize_iq", "raw wav16", "k_normalize_iq", "k_normalize_iq", "raw wav16", "raw wav16"]


@pytest.mark.parametrize("shape", ["two-streams", "4096-bins"])
@pytest.mark.parametrize("fmt,order", [(2, 1), (3, 2)])
def test_receivers_that_stage_every_raw_call(gpu_lib, shape, fmt, order):
    """two independent streams, and a 4096-bin display transform (no converting instance): staged on every call, and says so"""
    import pebblesdr_amd as P
    row = rc.ROW[SMALL]
    S = 2 if shape == "two-streams" else 1
    a, b = receivers(P, row, C=S, shared=S == 1, bins=rc.BINS if S == 2 else 4096)
    assert a.n_streams == S
    sf = a.superframe
    for k in range(3):
        raw = np.stack([rc.stream_raw(fmt, row.fs, False, sf, 500 + 10 * k + s, first=k * sf) for s in range(S)])
        rc.plant(raw[0], fmt, 0)
        x = rc.host_convert(raw, fmt, order, rc.GAIN[fmt])
        ga, gs, route, _, _ = raw_call(P, a, raw, fmt, order, rc.GAIN[fmt])
        assert route == "k_normalize_iq", k
        same(ga, gs, *b.process(x), k)


# ---- f. the pinned ingest slots ----
@pytest.mark.parametrize("name", ["s16-x8-iq", "f32-x8-iq"])
def test_ingest_slots_with_wide_pairs(gpu_lib, name):
    """4- and 8-byte pairs through ingest_buffer / ingest_submit / process_ingested, alternating slots, against process_raw_device on
    the twin; a slot that holds int8 pairs for the call is refused for the float format and the handle goes on"""
    import pebblesdr_amd as P
    row = rc.ROW[name]
    a, b = receivers(P, row)
    dtype = rc.FORMATS[row.fmt][0]
    calls = row_calls(row, a.superframe)
    for k, (raw, x) in enumerate(calls):
        n = len(x)
        nbytes = n * rc.PAIR_BYTES[row.fmt]
        host = a.ingest_buffer(k & 1, nbytes, dtype)
        host[:] = raw.reshape(-1)
        a.ingest_submit(k & 1, nbytes)
        a.process_ingested(k & 1, n, row.fmt, row.order, rc.GAIN[row.fmt])
        ga, gs = a.audio(), a.spectrum()
        assert (a.kernel_name(6), a.kernel_name(2)) == (rc.input_route(row, k), rc.front_kernel(row, k)), (name, k)
        wa, ws, route, _, _ = raw_call(P, b, raw, row.fmt, row.order, rc.GAIN[row.fmt])
        assert route == rc.input_route(row, k)
        same(ga, gs, wa, ws, (name, k))
    sf = a.superframe
    a.ingest_buffer(0, 2 * sf)[:] = 1
    a.ingest_submit(0, 2 * sf)
    with pytest.raises(P.PebbleGpuError) as e:
        a.process_ingested(0, sf, 3, 0, 1.0)   # sf int8 pairs were submitted: a quarter of what sf float pairs take
    assert e.value.code == E_SIZE
    raw, x = calls[0]
    ga, gs = raw_call(P, a, raw, row.fmt, row.order, rc.GAIN[row.fmt])[:2]
    same(ga, gs, *b.process(x), "after the refusal")


def test_the_multibank_refuses_a_misaligned_shard_pointer_and_goes_on(gpu_lib):
    """the multibank makes the receiver's call per shard: a misaligned entry is refused before any shard is asked (a shard that
    refused alone would leave the shards out of step and close the multibank), and the next good call is a twin multibank's"""
    import pebblesdr_amd as P
    fs, C, fmt = 2048000, 5, 2
    mbs = [P.MultiBank(fs, C, [0, 0], max_superframes=2) for _ in range(2)]
    for mb in mbs:
        for c in range(C):
            mb.set_mode(c, P.DM_USB)
            mb.set_mixer(c, -600e3 + 300e3 * c)
            mb.set_bandpass(c, 300, 3000)
    a, b = mbs
    sf = a.superframe
    raw = rc.stream_raw(fmt, fs, False, 2 * sf, 77, fc=0.0)
    buf = P.DeviceBuffer(sf * rc.PAIR_BYTES[fmt] + 64, 0)
    try:
        for k in range(2):
            buf.upload(np.ascontiguousarray(raw[k * sf:(k + 1) * sf]))
            for ptrs in ([buf.ptr + 16, buf.ptr], [buf.ptr, buf.ptr + 2]):
                with pytest.raises(P.PebbleGpuError) as e:
                    a.process_raw_device(ptrs, sf, fmt, 0, rc.GAIN[fmt])
                assert e.value.code == E_INVALID
            a.process_raw_device([buf.ptr, buf.ptr], sf, fmt, 0, rc.GAIN[fmt])
            b.process_raw_device([buf.ptr, buf.ptr], sf, fmt, 0, rc.GAIN[fmt])
            ga, gb = a.audio(), b.audio()
            assert ga.shape == (C, sf // a.D) and np.abs(gb[2]).max() > 1e-3
            assert np.array_equal(ga, gb), k
    finally:
        buf.free()
        for mb in mbs:
            mb.close()


# ---- g. refusals ----
@pytest.mark.parametrize("name", ["s8-x2-qi", "f32-x2-qonly"])
def test_refusals_leave_the_handle_usable(gpu_lib, name):
    """every refused call returns its code before anything is queued -- the misaligned pointers never reach a kernel -- leaves the
    input route of the last good call standing, and the next good call is the twin's"""
    import pebblesdr_amd as P
    row = rc.ROW[name]
    a, b = receivers(P, row)
    sf = a.superframe
    pair = rc.PAIR_BYTES[row.fmt]
    raw = rc.row_raw(row.name, sf)
    x = rc.host_convert(raw, row.fmt, row.order, rc.GAIN[row.fmt])
    g = rc.GAIN[row.fmt]
    big = P.DeviceBuffer((rc.MAX_SF + 1) * sf * pair + 64, 0)   # room for every refused call's samples, should one be let through

    def code(*args):
        with pytest.raises(P.PebbleGpuError) as e:
            a.process_raw_device(*args)
        return e.value.code

    try:
        assert big.ptr % rc.RAW_ALIGN == 0
        for k in range(3):
            lo, hi = k * sf, (k + 1) * sf
            big.upload(np.ascontiguousarray(raw[lo:hi]))
            if k:
                assert code(big.ptr + 2, sf, row.fmt, row.order, g) == E_INVALID                  # not aligned for any wide load
                assert code(big.ptr + 16, sf, row.fmt, row.order, g) == E_INVALID                 # aligned for 16 bytes, not for 32
                assert code(big.ptr, sf, 5, row.order, g) == E_INVALID                            # unknown format
                assert code(big.ptr, sf, row.fmt, 4, g) == E_INVALID                              # unknown IQ order
                assert code(big.ptr, (rc.MAX_SF + 1) * sf, row.fmt, row.order, g) == E_SIZE       # over capacity
                assert code(big.ptr, sf - rc.FRAME, row.fmt, row.order, g) == E_SIZE              # not whole super-frames
                assert code(0, sf, row.fmt, row.order, g) == E_INVALID                            # null
                assert a.kernel_name(6) == rc.input_route(row, k - 1)
            a.process_raw_device(big.ptr, sf, row.fmt, row.order, g)
            ga, gs = a.audio(), a.spectrum()
            assert (a.kernel_name(6), a.kernel_name(2)) == (rc.input_route(row, k), rc.front_kernel(row, k))
            same(ga, gs, *b.process(x[lo:hi]), k)
    finally:
        big.free()
