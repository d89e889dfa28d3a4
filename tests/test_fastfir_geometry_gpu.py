"""GPU tier of the band-pass geometry table (tests/fastfir_cases.py): every overlap-save geometry the library accepts, through the
step, the receiver bank and the stream bank, against the CPU oracle -- which tests/test_fastfir_geometry_host.py holds to the fp64
convolution at every one of these rows.

Bar: rel-RMS <= 1e-5 (BASELINE.json north_star) on every chunk of max(L, 1024) consecutive output samples of every call, the first
included; per call the output length equals the oracle's exactly.  Every test prints its worst chunk.  The sizes the library refuses
(taps outside [2, fft/2 + 1]) are refused at every create call, and nothing here takes such a size past its create call."""
import functools

import numpy as np
import pytest

from tests import fastfir_cases as FC

pytestmark = pytest.mark.gpu

TOL = FC.TOL
E_INVALID, E_FILTER_PARAM = -1, -4


def _row(rows, name):
    return {r.name: r for r in rows}[name]


# ------------------------------------------------------------------------------------------------
# the step: P.FastFIR against oracle.FastFIR
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,b", [(r.name, b) for r, b in FC.step_cases()])
def test_step_against_the_oracle(gpu_lib, oracle_mod, name, b):
    """calls of 1, L-1, L, L+1, 3L and 66L+5 samples (the last through the 64-block device loop twice, leaving a ragged rest), with the
    same parameters repeated, the invalid pair refused and a redesign on the way; the constructor row designs nothing and is silent"""
    import pebblesdr_amd as P
    row = _row(FC.STEP_ROWS, name)
    ref, f = oracle_mod.FastFIR(row.fft, row.taps), P.FastFIR(row.fft, row.taps)

    def setup(lo, hi, offset, rate):
        want = ref.setup(lo, hi, offset, rate) == 0
        try:
            f.SetupParameters(lo, hi, offset, rate)
            got = True
        except P.PebbleGpuError as e:
            assert e.code == E_FILTER_PARAM
            got = False
        assert got == want
        return got

    errs, outputs = [], 0

    def call(x):
        nonlocal outputs
        r, g = ref.process(x), f.ProcessData(x)
        if row.ctor:
            assert len(g) == len(r) and not np.any(r) and not np.any(g)
        else:
            errs.extend(FC.chunk_errors(g, r, row.L))
        outputs += len(r)
        return g

    x = FC.step_input(row)
    FC.run_script(FC.step_script(row, b), x, setup, call)
    assert outputs == (len(x) // row.L) * row.L and outputs >= 5 * row.L
    f.close()
    if row.ctor:
        print("step %s: %d output samples, all zero on both sides" % (name, outputs))
        return
    assert len(errs) == outputs // row.L
    print("step %s band %d: worst rel-RMS over %d chunks %.3e" % (name, b, len(errs), max(errs)))
    assert max(errs) <= TOL


# ------------------------------------------------------------------------------------------------
# the receiver bank: P.ReceiverBank against oracle.Receiver fed 2048-sample frames
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in FC.RX_ROWS])
def test_receiver_bank_against_the_oracle(gpu_lib, oracle_mod, name):
    """three channels on one shared stream, calls of 1, 2 and 1 super-frames of 32 * lcm(2048, L) samples, every channel and call from
    the first sample"""
    import pebblesdr_amd as P
    row = _row(FC.RX_ROWS, name)
    C = len(FC.RX_CHANNELS)
    modes = {"USB": (P.DM_USB, oracle_mod.USB), "AM": (P.DM_AM, oracle_mod.AM)}
    rx = P.ReceiverBank(FC.RX_FS, C, True, False, 0, fastfir_fft=row.fft, fastfir_taps=row.taps, max_superframes=max(FC.RX_CALLS))
    sf = rx.superframe
    assert sf == FC.rx_superframe(row) and rx.D == FC.RX_D
    refs = []
    for c, (mode, lo, hi, fc) in enumerate(FC.RX_CHANNELS):
        r = oracle_mod.Receiver(FC.RX_FS, FC.RX_FRAME, 0, row.fft, row.taps)
        r.set_mode(modes[mode][1]); r.set_mixer(fc); r.set_filter(lo, hi)
        refs.append(r)
        rx.set_mode(c, modes[mode][0]); rx.set_mixer(c, fc); rx.set_bandpass(c, lo, hi)
    x = FC.rx_input(sum(FC.RX_CALLS) * sf)
    at, worst = 0, [0.0] * C
    for k in FC.RX_CALLS:
        n = k * sf
        g = rx.process(x[at:at + n])[0]
        assert rx.kernel_name(4) == ("k_fastfir_t128" if row.fft == 2048 else "k_fastfir")
        for c in range(C):
            want = np.concatenate([refs[c].process(x[i:i + FC.RX_FRAME], want_spectrum=False)[0] for i in range(at, at + n, FC.RX_FRAME)])
            assert g[c].shape == want.shape == (n // FC.RX_D,)
            worst[c] = max([worst[c]] + FC.chunk_errors(g[c], want, row.L))
        at += n
    rx.close()
    print("receiver %s: worst rel-RMS per channel %s" % (name, " ".join("%.3e" % w for w in worst)))
    assert max(worst) <= TOL


# ------------------------------------------------------------------------------------------------
# the stream bank: P.StreamBank against a per-stream oracle.FastFIR
# ------------------------------------------------------------------------------------------------
def _bank(P, oracle_mod, row):
    sb = P.StreamBank(FC.FS, FC.SB_S, frame=row.frame, spectrum_bins=row.bins, fastfir_fft=row.fft, fastfir_taps=row.taps, max_frames=FC.SB_FRAMES)
    refs = []
    for s, (lo, hi) in enumerate(FC.SB_BANDS):
        sb.set_bandpass(s, lo, hi)
        r = oracle_mod.FastFIR(row.fft, row.taps)
        assert r.setup(lo, hi, 0.0, FC.FS) == 0
        refs.append(r)
    return sb, refs


def _sb_call(P, sb, fed, fmt, gain, what):
    """one call -> filtered [S, n]"""
    if fmt is None:
        return sb.process(fed, what)[0]
    buf = P.DeviceBuffer.from_array(np.ascontiguousarray(fed), 0)
    try:
        sb.process_raw_device(buf.ptr, fed.shape[1], fmt, 0, gain, what)
        return sb.filtered()
    finally:
        buf.free()


def _sb_compare(y, refs, x, L, worst):
    assert y.shape == x.shape
    for s, r in enumerate(refs):
        worst[s] = max([worst[s]] + FC.chunk_errors(y[s], r.process(x[s]), L))


@pytest.mark.parametrize("name,fmt", [(r.name, f) for r, f in FC.sb_cases()])
def test_stream_bank_against_the_oracle(gpu_lib, oracle_mod, name, fmt):
    """three streams with a pass-band each, three calls of two frames.  float2 input runs the band-pass beside the display transform;
    raw input asks for the band-pass alone, which the 2048-point plan converts in its first loads: kernel_name says which instance ran"""
    import pebblesdr_amd as P
    row = _row(FC.SB_ROWS, name)
    sb, refs = _bank(P, oracle_mod, row)
    fed, x, gain = FC.sb_input(row, fmt, oracle_mod)
    n, what, worst = FC.sb_call_samples(row), 3 if fmt is None else 1, [0.0] * FC.SB_S
    for k in range(FC.SB_CALLS):
        y = _sb_call(P, sb, fed[:, k * n:(k + 1) * n], fmt, gain, what)
        assert sb.kernel_name(1) == FC.sb_kernel(row, fmt, what)
        _sb_compare(y, refs, x[:, k * n:(k + 1) * n], row.L, worst)
    sb.close()
    print("stream bank %s %s: worst rel-RMS per stream %s" % (name, "float2" if fmt is None else FC.FORMATS[fmt][0], " ".join("%.3e" % w for w in worst)))
    assert max(worst) <= TOL


@pytest.mark.parametrize("order", [(2, None, 0), (None, 1, None), (4, 3, None)])
def test_raw_and_float2_calls_continue_each_other(gpu_lib, oracle_mod, order):
    """2048/513: the overlap a call leaves in `tail_out` holds CONVERTED samples whichever kernel wrote it (kernels_fastfir.h), so a raw
    call continues a float2 call and the reverse, and one raw format another -- held to the oracle fed the same sequence, not to a twin"""
    import pebblesdr_amd as P
    row = _row(FC.SB_ROWS, "sb-2048-513")
    sb, refs = _bank(P, oracle_mod, row)
    n, worst, names = FC.sb_call_samples(row), [0.0] * FC.SB_S, []
    for k, fmt in enumerate(order):
        fed, x, gain = FC.sb_input(row, fmt, oracle_mod)
        y = _sb_call(P, sb, fed[:, k * n:(k + 1) * n], fmt, gain, 1)
        names.append(sb.kernel_name(1))
        _sb_compare(y, refs, x[:, k * n:(k + 1) * n], row.L, worst)
    sb.close()
    assert names == [FC.sb_kernel(row, fmt, 1) for fmt in order]
    print("stream bank 2048/513, calls %s: worst rel-RMS per stream %s" % (names, " ".join("%.3e" % w for w in worst)))
    assert max(worst) <= TOL


def test_a_raw_call_with_the_display_transform_is_staged_and_continues(gpu_lib, oracle_mod):
    """the same bank asked for both results: frames of 3072 samples have no converting display kernel, the call is staged as a whole
    and says so -- between two converting calls, one stream all the way"""
    import pebblesdr_amd as P
    row, fmt = _row(FC.SB_ROWS, "sb-2048-513"), 0
    sb, refs = _bank(P, oracle_mod, row)
    fed, x, gain = FC.sb_input(row, fmt, oracle_mod)
    n, worst = FC.sb_call_samples(row), [0.0] * FC.SB_S
    for k, what in enumerate((1, 3, 1)):
        y = _sb_call(P, sb, fed[:, k * n:(k + 1) * n], fmt, gain, what)
        assert sb.kernel_name(1) == FC.sb_kernel(row, fmt, what)
        assert sb.kernel_name(2) == ("k_normalize_iq + k_spectrum_any" if what & 2 else "")
        _sb_compare(y, refs, x[:, k * n:(k + 1) * n], row.L, worst)
    sb.close()
    assert max(worst) <= TOL


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _valid_truth(kind):
    """the oracle's answer for the small valid run that follows every refusal (computed once)"""
    import oracle as O
    if kind == "step":
        x = FC.tones(FC.FS, 2048, FC.TONES) + FC.lcg_noise(2048, 5, FC.SIGMA)
        r = O.FastFIR(2048, 1025)
        r.setup(*FC.BANDS[0])
        return x, r.process(x)
    if kind == "rx":
        sf = 32 * 2048
        x = FC.rx_input(4 * 32 * 6144)[:sf]
        r = O.Receiver(FC.RX_FS, FC.RX_FRAME, 0)
        r.set_mode(O.USB); r.set_mixer(FC.RX_CHANNELS[0][3]); r.set_filter(300.0, 3000.0)
        return x, np.concatenate([r.process(x[i:i + FC.RX_FRAME], want_spectrum=False)[0] for i in range(0, sf, FC.RX_FRAME)])
    x = (FC.tones(FC.FS, 4096, FC.TONES) + FC.lcg_noise(4096, 6, FC.SIGMA)).astype(np.complex64)
    r = O.FastFIR(2048, 1025)
    r.setup(300.0, 3000.0, 0.0, FC.FS)
    return x, r.process(x.astype(np.complex128))


def _valid_step(P):
    x, want = _valid_truth("step")
    f = P.FastFIR(2048, 1025)
    f.SetupParameters(*FC.BANDS[0])
    g = f.ProcessData(x)
    f.close()
    assert max(FC.chunk_errors(g, want, 1024)) <= TOL


def _valid_rx(P):
    x, want = _valid_truth("rx")
    rx = P.ReceiverBank(FC.RX_FS, 1, True, False, 0)
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, FC.RX_CHANNELS[0][3]); rx.set_bandpass(0, 300.0, 3000.0)
    g = rx.process(x)[0][0]
    rx.close()
    assert max(FC.chunk_errors(g, want, 1024)) <= TOL


def _valid_sb(P):
    x, want = _valid_truth("sb")
    sb = P.StreamBank(FC.FS, 1, frame=2048, spectrum_bins=2048, max_frames=2)
    sb.set_bandpass(0, 300.0, 3000.0)
    g = sb.process(x[None, :], 1)[0][0]
    sb.close()
    assert max(FC.chunk_errors(g, want, 1024)) <= TOL


@pytest.mark.parametrize("fft,taps", [(2048, 1026), (4096, 2050), (8192, 4098), (2048, 2048), (4096, 4096), (8192, 8192), (2048, 1), (4096, 1), (8192, 1)])
def test_sizes_outside_the_rule_are_refused_at_every_create(gpu_lib, fft, taps):
    """taps = fft/2 + 2, taps = fft and taps = 1 through the step, the receiver bank and the stream bank: PEBBLEGPU_E_INVALID with the
    rule in the message, no object; a valid object of the same kind made right afterwards works"""
    import pebblesdr_amd as P
    assert not FC.accepted(fft, taps)
    makers = [(lambda: P.FastFIR(fft, taps), _valid_step),
              (lambda: P.ReceiverBank(FC.RX_FS, len(FC.RX_CHANNELS), True, False, 0, fastfir_fft=fft, fastfir_taps=taps, max_superframes=2), _valid_rx),
              (lambda: P.StreamBank(FC.FS, FC.SB_S, frame=2048, spectrum_bins=2048, fastfir_fft=fft, fastfir_taps=taps, max_frames=2), _valid_sb)]
    for make, valid in makers:
        with pytest.raises(P.PebbleGpuError) as e:
            make()
        assert e.value.code == E_INVALID
        assert "[2, fft/2 + 1]" in str(e.value)
        valid(P)
