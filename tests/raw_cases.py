"""The coverage statement for raw device-format input into a receiver (pebblegpu_receiver_process_raw): the converting loads of
csrc/raw_load.h inside the one-channel first stage k_mix_hb11_lean<FMT> and the 8192-bin display transform k_spectrum_t128<2, FMT>
(the raw-fused route, CallRoute::raw_fused of csrc/call_route.h), and the staged route through k_normalize_iq beside it.  One table
of rows, read by the CPU tier (tests/test_receiver_raw_host.py: the loaders themselves, compiled for the host, against host_convert()
bit for bit; the route every call of every row takes; the table's own claims; wrong conversions against the oracle) and by the GPU
tier (tests/test_receiver_raw_gpu.py: every row call by call against a twin receiver that is handed host_convert(raw) through
process(), bit for bit, with the input route and the first-stage kernel asserted on every call; five rows against the oracle).

Every row is a one-channel P.ReceiverBank with spectrum_bins = 8192 and max_superframes = 3 that takes calls of 1, 2, 1, 3
super-frames (decim_cases.SCRIPT).  Call 0 finds the oscillator inside its amplitude transient and is STAGED (k_normalize_iq, then
k_mix_hb11_bank at cl_log2 0); calls 1..3 are RAW-FUSED: k_mix_hb11_lean<FMT> (its window loads through raw_load4_even<FMT>, its edge
workgroup through the run-time raw_load) beside k_spectrum_t128<2, FMT> (raw_fetch4 + raw_convert4, stagger 7).

Rates (decim_cases.py's lean rows, and the headline): 1 024 000 -> hb11 x 2 (j_first = 5), 2 800 000 -> hb11 x 8 (j_first = 2),
9 800 000 -> hb11 x 32 (j_first = 1), 20 000 000 WFM -> hb11 x 8 with k_cascade<15,23,47> behind it.

Inputs (row_raw): an FM carrier (WFM rows) or a tone 1 kHz above the channel (narrow rows, USB 300..3000 Hz) at 0.45 of full scale
plus uniform noise of +-0.5 of full scale drawn per component, so that I and Q are distinct and every IQ order gives another stream;
at the start and at the end of EVERY call a block of 16 aligned quads carries the format's extreme codes (-128 / 127, 0 / 255,
-32768 / 32767; -0.0f, a denormal, +-1.5 for float) at each of the four positions of a quad in both components.  The CPU tier asserts
all of this on the arrays, and that every one of the eight shift lanes of raw_convert4 / raw_load4_even sees a negative value.

Wrong conversions (WRONG, run by the CPU tier on the oracle alone; figures in DESIGN.md): each must move the oracle-tied comparison
of every row of its format by at least MARGIN bars.  TWIN_ONLY names the ones only the bit-for-bit twin comparison can see.
"""
from collections import namedtuple
import functools

import numpy as np

from tests import decim_cases

# pebblegpu_iq_format -> (numpy type of a component, offset, normaliser); deviceinterfacebase.cpp:651,689,729, wavfile.cpp:299-300
FORMATS = {0: (np.int8, 0.0, 128.0), 1: (np.uint8, 128.0, 128.0), 2: (np.int16, 0.0, 32768.0), 3: (np.float32, 0.0, 1.0), 4: (np.int16, 0.0, 32767.0)}
TAG = {0: "s8", 1: "u8", 2: "s16", 3: "f32", 4: "wav16"}
# a gain per format; 0.5 where the normaliser is no power of two (the library forms gain * (1 / 32767.0) in double, the host
# gain / 32767.0: equal for a power-of-two gain whatever the last bit of the reciprocal)
GAIN = {0: 0.7, 1: 1.0, 2: 1.3, 3: 0.9, 4: 0.5}
PAIR_BYTES = {0: 2, 1: 2, 2: 4, 3: 8, 4: 4}   # csrc/raw_load.h kRawPairBytes
ORDER_NAME = {0: "IQ", 1: "QI", 2: "I only", 3: "Q only"}
RAW_ALIGN = 32                                # include/pebblegpu.h PEBBLEGPU_RAW_ALIGN

TOL = 1e-5      # tests/test_parity_gpu.py TOL, TOL_DB: the bars of the oracle-tied comparison
TOL_DB = 0.1
MARGIN = 100    # bars a wrong conversion must move that comparison by
FRAME = 2048
BINS = 8192
MAX_SF = 3
SCRIPT = decim_cases.SCRIPT


def make_raw(fmt, S, n, seed, fs=2.0e6):
    """[S, n, 2] components of `fmt`: a few tones per stream plus noise, filling most of the format's range"""
    from tests.signals import tones
    dtype, off, norm = FORMATS[fmt]
    rng = np.random.default_rng(seed)
    sig = np.stack([tones(fs, n, [(0.4, 123456.7 * (c + 1)), (0.2, 20000.0 - 30000.0 * c), (0.1, 1700.0)]) for c in range(S)])
    comp = np.stack([sig.real, sig.imag], axis=-1)
    if dtype == np.float32:
        return (comp + rng.uniform(-1e-3, 1e-3, comp.shape)).astype(np.float32)
    return np.round(comp * (norm - 2) + off + rng.uniform(-1, 1, comp.shape)).astype(dtype)


def order_select(a, b, order):
    """(re, im) of one sample from its first and second component"""
    return {0: (a, b), 1: (b, a), 2: (a, a), 3: (b, b)}[order]


def host_convert_parts(raw, fmt, order, gain):
    """DeviceInterfaceBase::normalizeIQ on the host with the library's constants -> float32 [..., n, 2] (re, im): the one product
    float32(v - off) * float32(gain / normaliser) per component, then the order select and nothing else (signed zeros, NaN
    payloads and denormals come through as the product leaves them)"""
    _, off, norm = FORMATS[fmt]
    with np.errstate(invalid="ignore", over="ignore"):   # (the host tier feeds NaNs and infinities through it)
        conv = (raw.astype(np.float32) - np.float32(off)) * np.float32(gain / norm)
    re, im = order_select(conv[..., 0], conv[..., 1], order)
    return np.ascontiguousarray(np.stack([re, im], axis=-1))


def host_convert(raw, fmt, order, gain):
    """... -> complex64 [..., n]"""
    return host_convert_parts(raw, fmt, order, gain).view(np.complex64)[..., 0]


# ------------------------------------------------------------------------------------------------
# the rows
# ------------------------------------------------------------------------------------------------
Row = namedtuple("Row", "name fs wfm fmt order stride oracle why")
WFM_FS = 20_000_000
FC = {1_024_000: 150e3, 2_800_000: 150e3, 9_800_000: 150e3, WFM_FS: 1.0e6}   # the channel's centre


def _row(name, fs, fmt, order, stride, why, oracle=False):
    return Row(name, fs, fs == WFM_FS, fmt, order, stride, oracle, why)


ROWS = [
    # ---- CPX8 (HackRF): the one format the route had run with, kept as the anchor, and the two strides it had not seen ----
    _row("s8-wfm-iq", WFM_FS, 0, 0, 8, "the headline shape as the bench runs it: k_mix_hb11_lean<0>, k_spectrum_t128<2, 0>", oracle=True),
    _row("s8-x2-qi", 1_024_000, 0, 1, 2, "stride 2: a window is 4 * 2 + 10 samples, five first outputs go to the edge workgroup; Q,I order"),
    _row("s8-x32-ionly", 9_800_000, 0, 2, 32, "stride 32: windows 64 bytes apart; I only (both parts from the first byte's lane)"),
    # ---- CPXU8 (RTL2832): k_mix_hb11_lean<1>, k_spectrum_t128<2, 1>; the - 128 offset behind the byte lanes ----
    _row("u8-x2-iq", 1_024_000, 1, 0, 2, "uint8 at stride 2", oracle=True),
    _row("u8-x8-qonly", 2_800_000, 1, 3, 8, "uint8 at stride 8, Q only (both parts from the second byte's lane)"),
    _row("u8-wfm-qi", WFM_FS, 1, 1, 8, "uint8 at the headline shape with k_cascade<15,23,47> behind, Q,I order"),
    # ---- CPX16: k_mix_hb11_lean<2>, k_spectrum_t128<2, 2>; sign extension by shift pairs of four words ----
    _row("s16-x32-qi", 9_800_000, 2, 1, 32, "int16 at stride 32, Q,I order", oracle=True),
    _row("s16-x8-iq", 2_800_000, 2, 0, 8, "int16 at stride 8"),
    # ---- CPXFLOAT: k_mix_hb11_lean<3>, k_spectrum_t128<2, 3>; two 16-byte loads per quad at base[i >> 1] ----
    _row("f32-x8-iq", 2_800_000, 3, 0, 8, "float at stride 8", oracle=True),
    _row("f32-x2-qonly", 1_024_000, 3, 3, 2, "float at stride 2 (a window starts at every even sample: both float4 phases), Q only"),
    # ---- WAV PCM16: k_mix_hb11_lean<4>, k_spectrum_t128<2, 4>; CPX16's loads with the 1 / 32767 scale ----
    _row("wav16-x8-qi", 2_800_000, 4, 1, 8, "WAV PCM16 at stride 8, Q,I order", oracle=True),
    _row("wav16-x2-ionly", 1_024_000, 4, 2, 2, "WAV PCM16 at stride 2, I only"),
    _row("wav16-wfm-iq", WFM_FS, 4, 0, 8, "WAV PCM16 at the headline shape"),
]
ROW = {r.name: r for r in ROWS}
ORACLE_ROWS = [r.name for r in ROWS if r.oracle]
GATED_ROWS = ["s8-x2-qi", "u8-x2-iq", "s16-x8-iq", "f32-x2-qonly", "wav16-x2-ionly"]      # under the update timer: one per format
RECORD_ROWS = ["s8-x2-qi", "u8-x8-qonly", "s16-x8-iq", "f32-x2-qonly", "wav16-x2-ionly"]  # recording + RAW_IQ tap: four not in IQ order


def lean_instance(row):
    return "k_mix_hb11_lean<%d>" % row.fmt


def spectrum_instance(row):
    return "k_spectrum_t128<2, %d>" % row.fmt


def input_route(row, k):
    """pebblegpu_receiver_kernel_name(rx, 6) of call k"""
    return "k_normalize_iq" if k == 0 else "raw " + TAG[row.fmt]


def front_kernel(row, k):
    """pebblegpu_receiver_kernel_name(rx, 2) of call k"""
    return "k_mix_hb11_bank" if k == 0 else "k_mix_hb11_lean"


def call_facts(row, k):
    """what plan_call_route() (csrc/call_route.h) reads at call k of a row, everything else at its default"""
    return dict(with_spectrum=1, with_chain=1, raw=1, C=1, S=1, nf=FRAME, n=SCRIPT[k], wfm=int(row.wfm), dec_lds_free_front=1, dec_raw_front=1,
                spec_raw_ready=1, osc_transient=int(k == 0))


def protect_bw(row):
    return 200000 if row.wfm else 30000


def superframe(chain):
    return FRAME * decim_cases.decimation(chain)


def call_bounds(sf):
    """[(first sample, samples)] of the script's calls"""
    out, at = [], 0
    for k in SCRIPT:
        out.append((at, k * sf))
        at += k * sf
    return out


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def extremes(fmt):
    """the codes planted at every quad position: (low, high) twice over -- for float -0.0f and a denormal, then -1.5 and 1.5"""
    dtype = FORMATS[fmt][0]
    if dtype == np.float32:
        return [np.float32(-0.0), np.float32(1e-40), np.float32(-1.5), np.float32(1.5)]
    info = np.iinfo(dtype)
    return [dtype(info.min), dtype(info.max)] * 2


PLANT = 64   # samples of a planted block: 4 quad positions x 2 components x 4 codes = 32 values, one per quad, two values per quad


def plant(raw, fmt, at):
    """raw[at : at + PLANT] (at a multiple of 4): quad j = 4 * pos + code carries code `code` at position pos, in both components"""
    assert at % 4 == 0
    ex = extremes(fmt)
    for pos in range(4):
        for code in range(4):
            q = at + 4 * (4 * pos + code)
            raw[q + pos, 0] = ex[code]
            raw[q + pos, 1] = ex[code ^ 1]   # (the other code of the pair: the two components of a sample differ)


def plant_sites(sf):
    """every call starts and ends with a planted block: the first windows (the edge workgroup, the history of the call before) and
    the last ones (the history the call leaves)"""
    return [at for lo, n in call_bounds(sf) for at in (lo, lo + n - PLANT)]


def stream_raw(fmt, fs, wfm, n, seed, fc=None, first=0):
    """[n, 2] components of `fmt`, samples first .. first + n of the stream: the carrier or tone at 0.45 of full scale + uniform noise
    of +-0.5 of full scale per component (no planted codes)"""
    dtype, off, norm = FORMATS[fmt]
    t = (np.arange(n, dtype=np.float64) + first) / fs
    fc = FC[fs] if fc is None else fc
    if wfm:
        ph = 2 * np.pi * ((fc * t) % 1.0) + 75.0 * np.sin(2 * np.pi * 1000.0 * t)
    else:
        ph = 2 * np.pi * (((fc + 1000.0) * t) % 1.0)
    rng = np.random.default_rng(seed)
    comp = np.stack([0.45 * np.cos(ph), 0.45 * np.sin(ph)], axis=-1) + rng.uniform(-0.5, 0.5, (n, 2))
    if dtype == np.float32:
        return comp.astype(np.float32)
    return np.round(comp * (norm - 2) + off).astype(dtype)


@functools.lru_cache(maxsize=4)
def row_raw(name, sf):
    """[sum(SCRIPT) * sf, 2] components of the row's format with the planted blocks (read-only: shared by the tests)"""
    row = ROW[name]
    raw = stream_raw(row.fmt, row.fs, row.wfm, sum(SCRIPT) * sf, 1000 + ROWS.index(row))
    for at in plant_sites(sf):
        plant(raw, row.fmt, at)
    raw.setflags(write=False)
    return raw


def setup_receiver(rx, row, P=None, oracle_mod=None):
    """the same tuning on a P.ReceiverBank (P given) or an oracle.Receiver (oracle_mod given)"""
    fc = FC[row.fs]
    if P is not None:
        rx.set_mixer(0, fc)
        if not row.wfm:
            rx.set_mode(0, P.DM_USB)
            rx.set_bandpass(0, 300, 3000)
    else:
        rx.set_mixer(fc)
        if row.wfm:
            rx.set_mode(oracle_mod.FMM)
        else:
            rx.set_mode(oracle_mod.USB)
            rx.set_filter(300, 3000)


def oracle_frame(chain):
    """the shortest frame, 2048 samples doubled as often as needed, at which every decimator stage of the oracle sees at least as many
    samples as it has taps.  Below that the reference drops to unfiltered sample skipping (decimator.cpp:602-625), which the oracle
    reproduces and the library, by its contract (include/pebblegpu.h), does not: 9.8 Msps hands its 59-tap last stage 16 samples of
    a 2048-sample frame.  The cascade is frame-invariant above it (tests/test_oracle_pins.py), and tests/test_parity_gpu.py feeds the
    oracle such frames for the same reason (test_config2_wfm_with_spectrum, test_decimator_short_frames_stream_exactly)."""
    frame = FRAME
    while True:
        n, ok = frame, True
        for taps, stride in chain:
            ok = ok and n >= taps
            n //= stride
        if ok:
            return frame
        frame *= 2


def oracle_narrow_audio(oracle_mod, row, x, frame):
    """the narrow chain of oracle.Receiver (po_receiver_process) put together from the oracle's own parts, so that the decimator can be
    fed frames of `frame` samples while the band-pass still gets its 2048: Mixer -> Decimator -> gain restore (receiver.cpp:935-938)
    -> FastFIR 2048/1025 -> AGC (off by default) -> the SSB pass-through.  With frame = 2048 this IS oracle.Receiver, sample for
    sample (the host tier asserts it on the rows whose stages never fall back)."""
    assert not row.wfm
    mix = oracle_mod.Mixer(row.fs)
    mix.set_frequency(FC[row.fs])
    dec = oracle_mod.Decimator(row.fs, protect_bw(row))
    bp = oracle_mod.FastFIR(2048, 1025)
    bp.setup(300, 3000, 0, float(int(dec.rate)))
    agc = oracle_mod.Agc(float(int(dec.rate)))
    z = np.concatenate([dec.process(mix.process(x[i:i + frame])) for i in range(0, len(x), frame)])
    z = z * 10 ** ((dec.dec_by2_stages * 2) / 20.0)
    return np.concatenate([agc.process(bp.process(z[i:i + FRAME])) for i in range(0, len(z), FRAME)])


def oracle_run(oracle_mod, row, x):
    """oracle.Receiver over whole super-frames of converted samples -> (audio [n / D], spectra [frames, BINS]).  Where a stage of the
    row's decimator would fall back at 2048-sample frames (oracle_frame), the audio comes from oracle_narrow_audio at the frame
    length at which none does, and only the spectra from oracle.Receiver"""
    frame = oracle_frame(oracle_mod.Decimator(row.fs, protect_bw(row)).chain())
    ref = oracle_mod.Receiver(row.fs, FRAME, BINS)
    setup_receiver(ref, row, oracle_mod=oracle_mod)
    audio, spec = [], []
    for f in range(len(x) // FRAME):
        a, s = ref.process(x[f * FRAME:(f + 1) * FRAME])
        if a is not None and len(a):
            audio.append(a)
        spec.append(s)
    if frame != FRAME:
        assert len(x) % frame == 0
        return oracle_narrow_audio(oracle_mod, row, x, frame), np.array(spec)
    return np.concatenate(audio), np.array(spec)


def rel_rms(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / max(np.sqrt(np.mean(np.abs(b) ** 2)), 1e-12))


def db_err(g, r):
    m = r > -110
    return float(np.abs(g - r)[m].max())


def bars(audio, spec, ref_audio, ref_spec):
    """the oracle-tied comparison of tests/test_parity_gpu.py in units of its bars: rel-RMS per 2048-sample audio frame over TOL, and
    |dB| over the bins the reference puts above -110 dB over TOL_DB, spectra from row 1 on -> the larger of the two worst figures"""
    assert audio.shape == ref_audio.shape and spec.shape == ref_spec.shape
    wa = max(rel_rms(audio[k:k + FRAME], ref_audio[k:k + FRAME]) for k in range(0, len(ref_audio), FRAME))
    wd = max(db_err(spec[f], ref_spec[f]) for f in range(1, len(ref_spec)))
    return max(wa / TOL, wd / TOL_DB), wa, wd


# ------------------------------------------------------------------------------------------------
# deliberately wrong conversions
# ------------------------------------------------------------------------------------------------
WRONG = ("no-sign-extension", "u8-without-offset", "iq-swapped", "order-taken-as-iq", "quad-rotated", "second-word-for-first", "scale-twice")
# wrong conversions that only the bit-for-bit twin comparison can see: WAV PCM16 normalised by 32768 instead of 32767 is 3e-5
# relative, three bars of the audio and 3e-4 dB
TWIN_ONLY = ("wav-by-32768",)


def applies(wrong, row):
    if wrong == "no-sign-extension":
        return row.fmt in (0, 2, 4)
    if wrong == "u8-without-offset":
        return row.fmt == 1
    if wrong == "order-taken-as-iq":
        return row.order >= 2
    if wrong == "wav-by-32768":
        return row.fmt == 4
    return True


def wrong_convert(wrong, raw, fmt, order, gain):
    """host_convert() with one mistake -> complex64 [n]"""
    dtype, off, norm = FORMATS[fmt]
    raw = np.ascontiguousarray(raw)
    if wrong == "no-sign-extension":       # the bytes / halfwords read as unsigned
        wide = raw.view(np.uint8 if fmt == 0 else np.uint16).astype(np.int32)
        conv = wide.astype(np.float32) * np.float32(gain / norm)
        re, im = order_select(conv[..., 0], conv[..., 1], order)
        return (re + 1j * im).astype(np.complex64)
    if wrong == "u8-without-offset":
        conv = raw.astype(np.float32) * np.float32(gain / norm)
        re, im = order_select(conv[..., 0], conv[..., 1], order)
        return (re + 1j * im).astype(np.complex64)
    if wrong == "iq-swapped":
        return host_convert(raw, fmt, order ^ 1, gain)
    if wrong == "order-taken-as-iq":
        return host_convert(raw, fmt, 0, gain)
    if wrong == "quad-rotated":            # the four samples of every aligned quad leave one place on
        return host_convert(np.roll(raw.reshape(-1, 4, 2), 1, axis=1).reshape(-1, 2), fmt, order, gain)
    if wrong == "second-word-for-first":
        # raw_fetch4's units: a quad of 8-bit pairs is two 32-bit words (two samples each), one of 16-bit pairs four (one sample each),
        # one of float pairs two 16-byte loads (two samples each) -- the second unit where the first belongs
        w = raw.reshape(-1).view(np.uint32).reshape(-1, PAIR_BYTES[fmt]).copy()   # (4 pairs of PAIR_BYTES bytes = PAIR_BYTES words)
        if fmt == 3:
            w[:, 0:4] = w[:, 4:8]
        else:
            w[:, 0] = w[:, 1]
        return host_convert(w.reshape(-1).view(dtype).reshape(-1, 2), fmt, order, gain)
    if wrong == "scale-twice":
        return (host_convert(raw, fmt, order, gain) * np.float32(gain / norm)).astype(np.complex64)
    if wrong == "wav-by-32768":
        return host_convert(raw, 2, order, gain)
    raise ValueError(wrong)
