"""GPU tier of the stream bank's raw-format input: pebblegpu_streambank_process_raw, the pinned ingest slots and kernel_name.

Every comparison but one is against a TWIN bank that is handed the same samples converted on the host the way
test_process_raw_converting_in_the_first_loads converts them -- (raw.astype(float32) - off) * float32(gain / normaliser), then the IQ
order -- and is bit for bit (np.array_equal on filtered() and spectrum()): the kernels that convert in their own loads round the same
single product, and the band-pass's overlap carries converted samples.  One test ties the raw route to the oracle instead."""
import numpy as np
import pytest

from tests.raw_cases import FORMATS, GAIN, TAG, host_convert, make_raw  # noqa: F401  (the table module of the receiver's raw tests keeps them)
from tests.signals import lcg_noise, tones

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_DB = 0.1
N65 = 65536

def banks(P, S, frame, bins, F, n=2, fs=2.0e6):
    out = []
    for _ in range(n):
        sb = P.StreamBank(fs, S, frame=frame, spectrum_bins=bins, max_frames=F)
        for c in range(S):
            sb.set_bandpass(c, -50e3 - 1e3 * c, 50e3 + 2e3 * c)
        out.append(sb)
    return out


def results(sb, what):
    return (sb.filtered() if what & 1 else None), (sb.spectrum() if what & 2 else None)


def assert_same(ra, rb, what):
    if what & 1:
        assert ra[0].shape == rb[0].shape and np.abs(rb[0]).max() > 1e-3
        assert np.array_equal(ra[0], rb[0])
    if what & 2:
        assert ra[1].shape == rb[1].shape and rb[1].max() > -100.0
        assert np.array_equal(ra[1], rb[1])


def run_pair(P, a, b, raw, fmt, order, gain, n, what, K, read_every_call):
    """K calls of n samples: raw into a, host-converted into b; compared after every call, or queued back to back and compared once"""
    S = raw.shape[0]
    x = host_convert(raw, fmt, order, gain)
    bufs = [P.DeviceBuffer.from_array(np.ascontiguousarray(raw[:, k * n:(k + 1) * n]), 0) for k in range(K)]
    xb = [P.DeviceBuffer.from_array(np.ascontiguousarray(x[:, k * n:(k + 1) * n]).view(np.float32), 0) for k in range(K)]
    names = []
    try:
        for k in range(K):
            a.process_raw_device(bufs[k].ptr, n, fmt, order, gain, what)  # no host synchronisation in between
            names.append((a.kernel_name(1), a.kernel_name(2)))
            b.process_device(xb[k].ptr, n, what)
            if read_every_call:
                assert_same(results(a, what), results(b, what), what)
        assert_same(results(a, what), results(b, what), what)
    finally:
        for d in bufs + xb:
            d.free()
    assert S == a.n_streams
    return names


@pytest.mark.parametrize("what", [1, 2, 3])
@pytest.mark.parametrize("fmt,order", [(0, 0), (0, 1), (1, 2), (1, 3), (2, 1), (2, 2), (3, 0), (3, 3), (4, 0), (4, 1)])
def test_configs4_geometry_converts_in_the_loads(gpu_lib, fmt, order, what):
    """65536-sample frames, 65536 bins, 2048/1025: every format (two IQ orders each, all four orders over the set), the band-pass
    alone, the transform alone and both, an odd number of streams, three calls back to back without a host synchronise -- the second
    and third start from the overlap the raw call before them left.  Both kernels are the converting instances on every call."""
    import pebblesdr_amd as P
    S, F, K = 5, 2, 3
    a, b = banks(P, S, N65, N65, F)
    n = F * N65
    raw = make_raw(fmt, S, K * n, 10 * fmt + order)
    names = run_pair(P, a, b, raw, fmt, order, GAIN[fmt], n, what, K, read_every_call=False)
    ff = "k_fastfir_t128 (raw %s)" % TAG[fmt] if what & 1 else ""
    sp = "k_big256_cols (raw %s) + k_big256_rows" % TAG[fmt] if what & 2 else ""
    assert names == [(ff, sp)] * K
    assert (b.kernel_name(1), b.kernel_name(2)) == ("k_fastfir_t128" if what & 1 else "", "k_big256_cols + k_big256_rows" if what & 2 else "")


@pytest.mark.parametrize("bins,fmt,order", [(8192, 0, 1), (8192, 1, 0), (8192, 2, 3), (8192, 3, 1), (8192, 4, 2),
                                            (2048, 0, 0), (2048, 2, 1), (4096, 1, 3), (4096, 4, 0), (4096, 3, 2)])
def test_2048_sample_frames_convert_or_stage(gpu_lib, bins, fmt, order):
    """2048-sample frames: with 8192 bins k_spectrum_t128's converting instances serve three streams at once (a receiver only ever
    hands them one) beside the converting band-pass; 2048 and 4096 bins have no converting display kernel, so the call is staged
    through k_normalize_iq as a whole -- and says so.  Compared after every one of three calls."""
    import pebblesdr_amd as P
    S, F, K = 3, 8, 3
    a, b = banks(P, S, 2048, bins, F)
    n = F * 2048
    raw = make_raw(fmt, S, K * n, 100 + bins + fmt)
    names = run_pair(P, a, b, raw, fmt, order, GAIN[fmt], n, 3, K, read_every_call=True)
    if bins == 8192:
        want = ("k_fastfir_t128 (raw %s)" % TAG[fmt], "k_spectrum_t128 (raw %s)" % TAG[fmt])
    else:
        want = ("k_normalize_iq + k_fastfir_t128", "k_normalize_iq + " + ("k_spectrum_q128" if bins == 2048 else "k_spectrum<2>"))
    assert names == [want] * K


def test_a_band_pass_without_converting_loads_is_staged(gpu_lib):
    """A 4096-point band-pass (k_fastfir) has no converting loads: the whole call is staged although the display transform could
    convert, and continues exactly."""
    import pebblesdr_amd as P
    S, F, K, fmt, order = 2, 8, 2, 0, 1
    a, b = [P.StreamBank(2.0e6, S, frame=2048, spectrum_bins=8192, fastfir_fft=4096, fastfir_taps=2049, max_frames=F) for _ in range(2)]
    for sb in (a, b):
        for c in range(S):
            sb.set_bandpass(c, -40e3, 60e3)
    n = F * 2048
    raw = make_raw(fmt, S, K * n, 77)
    names = run_pair(P, a, b, raw, fmt, order, GAIN[fmt], n, 3, K, read_every_call=True)
    assert names == [("k_normalize_iq + k_fastfir", "k_normalize_iq + k_spectrum_t128")] * K


@pytest.mark.parametrize("frame", [4096, 1024])
def test_the_general_display_transform_is_staged(gpu_lib, frame):
    """Frames other than 2048 samples take the general display transform (k_spectrum_any), which has no converting loads -- with 8192
    bins too, where 2048-sample frames would convert: the whole call is staged, nothing fails half-way, and the stream continues."""
    import pebblesdr_amd as P
    S, F, K, fmt, order = 3, 4, 3, 0, 1
    a, b = banks(P, S, frame, 8192, F)
    n = F * frame
    raw = make_raw(fmt, S, K * n, 88)
    names = run_pair(P, a, b, raw, fmt, order, GAIN[fmt], n, 3, K, read_every_call=True)
    assert names == [("k_normalize_iq + k_fastfir_t128", "k_normalize_iq + k_spectrum_any")] * K


@pytest.mark.parametrize("fmt,order", [(0, 1), (1, 0)])
def test_odd_numbers_of_frames_with_8_bit_pairs(gpu_lib, fmt, order):
    """Pass A's 8-bit instances deal tiles to XCDs in pairs of frames: calls of one, three and one frames leave the last pair half
    empty (the workgroups of the missing frame leave at once).  Compared with the twin after every call."""
    import pebblesdr_amd as P
    S, F = 5, 3
    a, b = banks(P, S, N65, N65, F)
    frames = [1, 3, 1]
    raw = make_raw(fmt, S, sum(frames) * N65, 90 + fmt)
    x = host_convert(raw, fmt, order, GAIN[fmt])
    at = 0
    for f in frames:
        n = f * N65
        buf = P.DeviceBuffer.from_array(np.ascontiguousarray(raw[:, at:at + n]), 0)
        try:
            a.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt])
            ra = results(a, 3)
        finally:
            buf.free()
        assert ra[1].shape == (S, f, N65) and a.kernel_name(2) == "k_big256_cols (raw %s) + k_big256_rows" % TAG[fmt]
        assert_same(ra, b.process(np.ascontiguousarray(x[:, at:at + n])), 3)
        at += n


@pytest.mark.parametrize("fmt", [0, 2])
def test_the_transform_in_batches_of_streams_with_raw_input(gpu_lib, monkeypatch, fmt):
    """PEBBLEGPU_BIG_BATCH_MB: the 65536-point transform in batches of streams (five streams as 2 + 2 + 1) -- every batch's raw rows
    start at its first stream's pairs, whatever the pair's size."""
    import pebblesdr_amd as P
    S, F, K, order = 5, 2, 2, 0
    monkeypatch.setenv("PEBBLEGPU_BIG_BATCH_MB", "2")  # 2 frames x 65536 points x 8 bytes = 1 MiB of intermediate per stream
    (a,) = banks(P, S, N65, N65, F, n=1)
    monkeypatch.delenv("PEBBLEGPU_BIG_BATCH_MB")
    (b,) = banks(P, S, N65, N65, F, n=1)
    n = F * N65
    raw = make_raw(fmt, S, K * n, 95 + fmt)
    names = run_pair(P, a, b, raw, fmt, order, GAIN[fmt], n, 3, K, read_every_call=True)
    assert names == [("k_fastfir_t128 (raw %s)" % TAG[fmt], "k_big256_cols (raw %s) + k_big256_rows" % TAG[fmt])] * K


@pytest.mark.parametrize("frame,bins", [(N65, N65), (2048, 4096)])
def test_raw_and_float2_calls_alternate_on_one_bank(gpu_lib, frame, bins):
    """raw, float2, raw on one bank against float2, float2, float2 on the twin (a converting and a staged geometry): the overlap
    buffer holds converted samples whichever call wrote it."""
    import pebblesdr_amd as P
    S, F, fmt, order = 3, 2 if frame == N65 else 8, 2, 1
    a, b = banks(P, S, frame, bins, F)
    n = F * frame
    raw = make_raw(fmt, S, 3 * n, 5)
    x = host_convert(raw, fmt, order, GAIN[fmt])
    for k in range(3):
        blk = np.ascontiguousarray(x[:, k * n:(k + 1) * n])
        if k == 1:
            ra = a.process(blk)
            assert a.kernel_name(1) == "k_fastfir_t128"
        else:
            buf = P.DeviceBuffer.from_array(np.ascontiguousarray(raw[:, k * n:(k + 1) * n]), 0)
            try:
                a.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt])
                ra = results(a, 3)
            finally:
                buf.free()
            assert a.kernel_name(1) != "k_fastfir_t128"
        assert_same(ra, b.process(blk), 3)


@pytest.mark.parametrize("frame,bins", [(N65, N65), (2048, 2048)])
def test_gain_zero_is_silence_on_both_routes(gpu_lib, frame, bins):
    """m_userIQGain = 0 multiplies every sample by zero (deviceinterfacebase.cpp:651): filtered() is all zeros and the spectrum is
    the floor, where the kernels convert in their loads and where the call is staged (which must not read the 0 as "no scale")."""
    import pebblesdr_amd as P
    S, F, fmt = 3, 2 if frame == N65 else 8, 0
    (a,) = banks(P, S, frame, bins, F, n=1)
    n = F * frame
    buf = P.DeviceBuffer.from_array(make_raw(fmt, S, n, 9), 0)
    try:
        a.process_raw_device(buf.ptr, n, fmt, 0, 1.0)
        y, sp = results(a, 3)
        assert np.abs(y).max() > 1e-3 and sp.max() > -100.0
        a.process_raw_device(buf.ptr, n, fmt, 0, 0.0)
        a.process_raw_device(buf.ptr, n, fmt, 0, 0.0)  # (the second such call: the overlap holds zeros too)
        y, sp = results(a, 3)
    finally:
        buf.free()
    assert y.shape == (S, n) and not y.any()
    assert sp.shape[0] == S and sp.max() <= -119.9


def test_side_by_side_with_raw_input_equals_the_default(gpu_lib, monkeypatch):
    """PEBBLEGPU_SB_SIDE=1 with raw input, from device buffers and through the pinned slots (both streams wait for the slot's upload)."""
    import pebblesdr_amd as P
    S, F, K, fmt, order = 4, 2, 3, 0, 1
    monkeypatch.setenv("PEBBLEGPU_SB_SIDE", "1")
    (a,) = banks(P, S, N65, N65, F, n=1)
    monkeypatch.delenv("PEBBLEGPU_SB_SIDE")
    (b,) = banks(P, S, N65, N65, F, n=1)
    n = F * N65
    raw = make_raw(fmt, S, K * n, 31)
    for k in range(K):
        blk = np.ascontiguousarray(raw[:, k * n:(k + 1) * n])
        buf = P.DeviceBuffer.from_array(blk, 0)
        try:
            if k == 1:
                a.ingest_acquire(0, blk.nbytes, np.int8)[:] = blk.reshape(-1)
                a.ingest_submit(0, blk.nbytes)
                a.process_ingested(0, n, fmt, order, GAIN[fmt])
            else:
                a.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt])
            b.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt])
            assert_same(results(a, 3), results(b, 3), 3)
        finally:
            buf.free()


@pytest.mark.parametrize("read_every_call", [False, True])
def test_pinned_slots_overlap_upload_and_compute(gpu_lib, read_every_call):
    """Six batches alternating through the two slots, each next slot filled and submitted while the previous call is still queued,
    against process_raw on device buffers (and once more with the results read after every call)."""
    import pebblesdr_amd as P
    S, F, K, fmt, order = 5, 2, 6, 0, 0
    a, b = banks(P, S, N65, N65, F)
    n = F * N65
    raw = make_raw(fmt, S, K * n, 41)
    nbytes = S * n * 2
    bufs = [P.DeviceBuffer.from_array(np.ascontiguousarray(raw[:, k * n:(k + 1) * n]), 0) for k in range(K)]
    try:
        for k in range(K):
            s = k & 1
            host = a.ingest_acquire(s, nbytes, np.int8)  # waits for the call that read this slot two batches ago, not for the last one
            host[:] = raw[:, k * n:(k + 1) * n].reshape(-1)
            a.ingest_submit(s, nbytes)
            a.process_ingested(s, n, fmt, order, GAIN[fmt])
            assert a.kernel_name(1) == "k_fastfir_t128 (raw s8)"
            b.process_raw_device(bufs[k].ptr, n, fmt, order, GAIN[fmt])
            if read_every_call:
                assert_same(results(a, 3), results(b, 3), 3)
        assert_same(results(a, 3), results(b, 3), 3)
    finally:
        for d in bufs:
            d.free()


def test_refusals_leave_the_bank_usable(gpu_lib):
    """The three slot mistakes and the argument mistakes are refused with their codes before anything is queued, and the next valid
    call still matches the twin."""
    import pebblesdr_amd as P
    S, F, fmt, order = 3, 2, 0, 0
    a, b = banks(P, S, N65, N65, F)
    n = F * N65
    raw = make_raw(fmt, S, 2 * n, 51)
    nbytes = S * n * 2
    buf = P.DeviceBuffer.from_array(np.ascontiguousarray(raw[:, :n]), 0)
    big = P.DeviceBuffer(S * (n + N65) * 2 + 64, 0)

    def code(fn, *args):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*args)
        return e.value.code

    try:
        assert code(a.process_raw_device, buf.ptr, n, 9, 0, 1.0) == -1            # unknown format
        assert code(a.process_raw_device, buf.ptr, n, fmt, 4, 1.0) == -1          # unknown IQ order
        assert code(a.process_raw_device, buf.ptr, n - 2048, fmt, 0, 1.0) == -5   # not a multiple of the frame
        assert code(a.process_raw_device, big.ptr, n + N65, fmt, 0, 1.0) == -5    # above the capacity
        assert code(a.process_raw_device, buf.ptr + 16, n, fmt, 0, 1.0) == -1     # not aligned for the wide loads
        assert code(a.ingest_submit, 0, nbytes) == -5                             # nothing acquired
        assert code(a.ingest_acquire, 2, nbytes) == -1                            # slots are 0 and 1
        host = a.ingest_acquire(0, nbytes, np.int8)
        host[:] = raw[:, :n].reshape(-1)
        assert code(a.ingest_submit, 0, nbytes + 2) == -5                         # more bytes than acquired
        assert code(a.process_ingested, 0, n, fmt, order, 1.0) == -5              # nothing submitted yet
        a.ingest_submit(0, nbytes)
        assert code(a.process_ingested, 0, n, 2, order, 1.0) == -5                # int16 pairs need twice the bytes
        assert code(a.process_ingested, 0, n, 9, order, 1.0) == -1
        a.process_ingested(0, n, fmt, order, GAIN[fmt])
        assert code(a.ingest_submit, 0, nbytes) == -1                             # submitted again without an acquire
        b.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt])
        assert_same(results(a, 3), results(b, 3), 3)
        # ... and the next valid call, raw from a device buffer, still continues the stream
        buf.upload(np.ascontiguousarray(raw[:, n:]))
        a.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt])
        x = host_convert(raw[:, n:], fmt, order, GAIN[fmt])
        assert_same(results(a, 3), b.process(x), 3)
    finally:
        buf.free()
        big.free()


def test_map_spectrum_after_a_raw_call(gpu_lib):
    import pebblesdr_amd as P
    S, F, fmt, order = 3, 2, 1, 1
    a, b = banks(P, S, N65, N65, F)
    n = F * N65
    raw = make_raw(fmt, S, n, 61)
    buf = P.DeviceBuffer.from_array(raw, 0)
    try:
        a.process_raw_device(buf.ptr, n, fmt, order, GAIN[fmt], 2)
        b.process(host_convert(raw, fmt, order, GAIN[fmt]), 2)
        args = (256, 1024, -20.0, -110.0, -400000, 600000)
        ma, mb = a.map_spectrum(*args, first_frame=0, n_frames=F), b.map_spectrum(*args, first_frame=0, n_frames=F)
    finally:
        buf.free()
    assert ma.shape == (S, F, 1024) and len(np.unique(mb)) > 8
    assert np.array_equal(ma, mb)


def _rel_rms(a, b):
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / max(np.sqrt(np.mean(np.abs(b) ** 2)), 1e-12))


def test_raw_int8_against_the_oracle(gpu_lib, oracle_mod):
    """One tie to the reference rather than to the twin: int8 pairs at the size of test_config5_streambank_small through
    oracle.normalize_iq, the oracle's band-pass and its transform.  rel-RMS <= 1e-5 per 2048-sample frame, the first included;
    <= 0.1 dB over bins the oracle puts above -110 dB, the very first frame's spectrum included (it averages with the zeros both
    sides start from)."""
    import pebblesdr_amd as P
    fs, S, N, F, gain = 2.0e6, 3, N65, 2, 0.7
    bands = [(-50e3, 50e3), (-100e3, -10e3), (300.0, 3000.0)]
    sig = np.stack([tones(fs, 3 * F * N, [(0.4, 123456.7 * (c + 1)), (0.01, -700001.3), (0.2, 20000.0 - 30000.0 * c), (0.1, 1700.0)])
                    + lcg_noise(3 * F * N, 70 + c, 1e-4) for c in range(S)])
    raw = np.round(np.stack([sig.real, sig.imag], axis=-1) * 126.0).astype(np.int8)
    sb = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=F)
    refs = []
    for c in range(S):
        sb.set_bandpass(c, *bands[c])
        f = oracle_mod.FastFIR(2048, 1025)
        f.setup(bands[c][0], bands[c][1], 0.0, fs)
        refs.append((f, oracle_mod.Spectrum(N, N, lift_clamp=True)))
    worst, worst_db = 0.0, 0.0
    for call in range(3):
        blk = np.ascontiguousarray(raw[:, call * F * N:(call + 1) * F * N])
        buf = P.DeviceBuffer.from_array(blk, 0)
        try:
            sb.process_raw_device(buf.ptr, F * N, 0, 0, gain)
            y, sp = results(sb, 3)
        finally:
            buf.free()
        assert sb.kernel_name(1) == "k_fastfir_t128 (raw s8)"
        for c in range(S):
            x = oracle_mod.normalize_iq(blk[c].reshape(-1), 0, 0, gain)
            r = refs[c][0].process(x)
            for k in range(F * N // 2048):
                worst = max(worst, _rel_rms(y[c, k * 2048:(k + 1) * 2048], r[k * 2048:(k + 1) * 2048]))
            for f in range(F):
                rs = refs[c][1].process(x[f * N:(f + 1) * N])
                m = rs > -110
                assert m.sum() > 100
                worst_db = max(worst_db, float(np.abs(sp[c, f] - rs)[m].max()))
    print("raw int8 against the oracle: worst rel-RMS per 2048-sample frame %.3e, worst |dB| %.4f" % (worst, worst_db))
    assert worst <= TOL
    assert worst_db <= TOL_DB


def test_full_size_int8(gpu_lib):
    """BASELINE configs[4]'s per-GPU size once: 128 streams x 4 frames of int8 pairs, bit for bit the twin; both kernels timed."""
    import pebblesdr_amd as P
    S, F, fmt, order, gain = 128, 4, 0, 0, 1.0
    a, b = [P.StreamBank(2.0e6, S, frame=N65, spectrum_bins=N65, max_frames=F) for _ in range(2)]
    for sb in (a, b):
        for c in range(S):
            sb.set_bandpass(c, -50e3 - 100.0 * c, 50e3)
    n = F * N65
    rng = np.random.default_rng(8)
    raw = rng.integers(-128, 128, size=(S, n, 2), dtype=np.int8)
    raw[:, :, 0] = np.clip(raw[:, :, 0] // 4 + np.round(60 * np.cos(2 * np.pi * 0.01 * np.arange(n))).astype(np.int16), -128, 127).astype(np.int8)
    x = host_convert(raw, fmt, order, gain)
    buf = P.DeviceBuffer.from_array(raw, 0)
    xb = P.DeviceBuffer.from_array(x.view(np.float32), 0)
    try:
        for _ in range(2):  # the second call starts from the overlap the first left
            a.process_raw_device(buf.ptr, n, fmt, order, gain)
            b.process_device(xb.ptr, n)
        assert a.last_ms(1) > 0 and a.last_ms(2) > 0 and a.last_ms(0) >= a.last_ms(1)
        assert (a.kernel_name(1), a.kernel_name(2)) == ("k_fastfir_t128 (raw s8)", "k_big256_cols (raw s8) + k_big256_rows")
        assert_same(results(a, 3), results(b, 3), 3)
    finally:
        buf.free()
        xb.free()
