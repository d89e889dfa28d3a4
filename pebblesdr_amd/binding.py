"""ctypes bindings for libpebblegpu (include/pebblegpu.h) and the receiver-bank convenience class."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBNAME = "libpebblegpu.so"

(DM_AM, DM_SAM, DM_FMN, DM_FMM, DM_FMS, DM_DSB, DM_LSB, DM_USB, DM_CWL, DM_CWU, DM_DIGL, DM_DIGU, DM_NONE) = range(13)

# every symbol include/pebblegpu.h declares (tests/test_abi_symbols.py checks the header against this list too)
SYMBOLS = [
    "pebblegpu_last_error", "pebblegpu_abi_version", "pebblegpu_device_count",
    "pebblegpu_malloc", "pebblegpu_free", "pebblegpu_memcpy_h2d", "pebblegpu_memcpy_d2h", "pebblegpu_memset",
    "pebblegpu_device_synchronize", "pebblegpu_probe_copy_gbps", "pebblegpu_live_bytes", "pebblegpu_normalize_iq",
    "pebblegpu_receiver_create", "pebblegpu_receiver_destroy", "pebblegpu_receiver_info",
    "pebblegpu_set_mixer_freq", "pebblegpu_set_bandpass", "pebblegpu_set_demod_mode", "pebblegpu_receiver_rds_groups", "pebblegpu_receiver_stereo_lock", "pebblegpu_set_agc", "pebblegpu_set_conditioners", "pebblegpu_set_noise_filter", "pebblegpu_set_squelch", "pebblegpu_receiver_process_raw",
    "pebblegpu_receiver_process", "pebblegpu_receiver_audio", "pebblegpu_receiver_spectrum", "pebblegpu_receiver_zoom_spectrum",
    "pebblegpu_receiver_ingest_acquire", "pebblegpu_receiver_ingest_submit", "pebblegpu_receiver_process_ingested", "pebblegpu_receiver_last_ms", "pebblegpu_receiver_kernel_name", "pebblegpu_receiver_mean_ms", "pebblegpu_receiver_set_profiling", "pebblegpu_receiver_enable_signal_strength", "pebblegpu_receiver_signal_strength", "pebblegpu_receiver_synchronize", "pebblegpu_process_iq",
    "pebblegpu_streambank_create", "pebblegpu_streambank_destroy", "pebblegpu_streambank_set_bandpass",
    "pebblegpu_streambank_process", "pebblegpu_streambank_filtered", "pebblegpu_streambank_spectrum",
    "pebblegpu_streambank_last_ms", "pebblegpu_streambank_synchronize",
    "pebblegpu_streambank_process_raw", "pebblegpu_streambank_ingest_acquire", "pebblegpu_streambank_ingest_submit",
    "pebblegpu_streambank_process_ingested", "pebblegpu_streambank_kernel_name",
    "pebblegpu_mixer_create", "pebblegpu_mixer_destroy", "pebblegpu_mixer_set_frequency", "pebblegpu_mixer_process",
    "pebblegpu_decimator_create", "pebblegpu_decimator_destroy", "pebblegpu_decimator_build_chain",
    "pebblegpu_decimator_dec_by2_stages", "pebblegpu_decimator_process",
    "pebblegpu_downconvert_create", "pebblegpu_downconvert_destroy", "pebblegpu_downconvert_set_data_rate", "pebblegpu_downconvert_set_frequency",
    "pebblegpu_downconvert_set_cw_offset", "pebblegpu_downconvert_stages", "pebblegpu_downconvert_process", "pebblegpu_downconvert_process_device",
    "pebblegpu_downconvert_synchronize",
    "pebblegpu_fastfir_create", "pebblegpu_fastfir_destroy", "pebblegpu_fastfir_setup", "pebblegpu_fastfir_process",
    "pebblegpu_demod_create", "pebblegpu_demod_destroy", "pebblegpu_demod_set_mode", "pebblegpu_demod_set_bandwidth",
    "pebblegpu_demod_process", "pebblegpu_demod_rds_groups", "pebblegpu_demod_rds_signal", "pebblegpu_demod_stereo_lock",
    "pebblegpu_spectrum_create", "pebblegpu_spectrum_destroy", "pebblegpu_spectrum_bins", "pebblegpu_spectrum_process",
    "pebblegpu_receiver_map_spectrum", "pebblegpu_receiver_map_zoom_spectrum", "pebblegpu_streambank_map_spectrum",
    "pebblegpu_spectrum_map_to_screen",
    "pebblegpu_set_morse", "pebblegpu_receiver_morse_events", "pebblegpu_receiver_morse_status",
    "pebblegpu_morse_create", "pebblegpu_morse_destroy", "pebblegpu_morse_set_demod_mode", "pebblegpu_morse_process",
    "pebblegpu_morse_events", "pebblegpu_morse_status", "pebblegpu_morse_results", "pebblegpu_morse_set_sample_rate",
    "pebblegpu_morse_keep_results",
    "pebblegpu_set_spectrum_updates", "pebblegpu_receiver_spectrum_frames", "pebblegpu_process_iq_updates",
    "pebblegpu_streambank_set_spectrum_updates", "pebblegpu_streambank_spectrum_frames",
    "pebblegpu_sweep_plan", "pebblegpu_set_testbench_sweep", "pebblegpu_set_testbench_noise", "pebblegpu_receiver_set_taps", "pebblegpu_receiver_tap",
    "pebblegpu_siggen_create", "pebblegpu_siggen_destroy", "pebblegpu_siggen_set_sweep", "pebblegpu_siggen_set_noise", "pebblegpu_siggen_set_stream",
    "pebblegpu_siggen_generate_device", "pebblegpu_siggen_synchronize", "pebblegpu_siggen_generate", "pebblegpu_siggen_noise_draws",
    "pebblegpu_morse_station_plan", "pebblegpu_morse_station_marks", "pebblegpu_set_testbench_morse", "pebblegpu_siggen_set_morse",
    "pebblegpu_multibank_plan", "pebblegpu_multibank_create", "pebblegpu_multibank_destroy", "pebblegpu_multibank_shards", "pebblegpu_multibank_shard",
    "pebblegpu_multibank_locate", "pebblegpu_multibank_process", "pebblegpu_multibank_process_raw", "pebblegpu_multibank_ingest_acquire",
    "pebblegpu_multibank_ingest_submit", "pebblegpu_multibank_process_ingested", "pebblegpu_multibank_synchronize", "pebblegpu_multibank_last_ms",
    "pebblegpu_receiver_audio_out_open", "pebblegpu_receiver_audio_out_close", "pebblegpu_set_audio_level", "pebblegpu_receiver_audio_out_next",
    "pebblegpu_receiver_audio_out_release", "pebblegpu_receiver_audio_out_dropped", "pebblegpu_audio_out_convert",
    "pebblegpu_receiver_record_open", "pebblegpu_receiver_record_close", "pebblegpu_receiver_record_next", "pebblegpu_receiver_record_release",
    "pebblegpu_iq_record_convert",
    "pebblegpu_receiver_modem_out_open", "pebblegpu_receiver_modem_out_close", "pebblegpu_receiver_modem_out_next",
    "pebblegpu_receiver_modem_out_release", "pebblegpu_receiver_modem_out_dropped", "pebblegpu_modem_out_convert", "pebblegpu_modem_out_layout",
    "pebblegpu_receiver_modem_out_open_rate", "pebblegpu_modem_rate_plan",
    "pebblegpu_streambank_iq_out_open", "pebblegpu_streambank_iq_out_close", "pebblegpu_streambank_iq_out_next", "pebblegpu_streambank_iq_out_release",
    "pebblegpu_streambank_iq_out_dropped",
    "pebblegpu_streambank_display_open", "pebblegpu_streambank_display_close", "pebblegpu_streambank_display_next",
    "pebblegpu_streambank_display_release", "pebblegpu_streambank_display_dropped", "pebblegpu_waterfall_colors",
    "pebblegpu_receiver_display_open", "pebblegpu_receiver_display_close", "pebblegpu_receiver_display_next",
    "pebblegpu_receiver_display_release", "pebblegpu_receiver_display_dropped", "pebblegpu_receiver_display_set_pane",
    "pebblegpu_auto_scale_row", "pebblegpu_receiver_spectrum_scale", "pebblegpu_streambank_spectrum_scale",
    "pebblegpu_receiver_display_set_auto_scale", "pebblegpu_receiver_display_rescale", "pebblegpu_receiver_display_scale",
    "pebblegpu_streambank_display_set_auto_scale", "pebblegpu_streambank_display_rescale", "pebblegpu_streambank_display_scale",
    "pebblegpu_signal_strength_row", "pebblegpu_streambank_enable_signal_strength", "pebblegpu_streambank_signal_strength",
    "pebblegpu_streambank_set_squelch", "pebblegpu_streambank_iq_out_gate",
    "pebblegpu_streambank_set_conditioners", "pebblegpu_streambank_conditioned", "pebblegpu_receiver_conditioned",
]

SPECTRUM_EVERY_FRAME = -1  # PEBBLEGPU_SPECTRUM_EVERY_FRAME
COND_DC, COND_IQBALANCE, COND_NB1, COND_NB2 = 1, 2, 4, 8  # PEBBLEGPU_COND_*


class PebbleGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libpebblegpu error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("sample_rate", C.c_double),
        ("frames_per_buffer", C.c_uint32), ("n_channels", C.c_uint32), ("shared_input", C.c_uint32),
        ("wfm", C.c_uint32), ("spectrum_bins", C.c_uint32), ("fastfir_fft", C.c_uint32),
        ("fastfir_taps", C.c_uint32), ("max_superframes", C.c_uint32), ("audio_rate", C.c_uint32), ("hires_bins", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class StreamBankConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("sample_rate", C.c_double), ("n_streams", C.c_uint32),
        ("frame", C.c_uint32), ("spectrum_bins", C.c_uint32), ("fastfir_fft", C.c_uint32), ("fastfir_taps", C.c_uint32),
        ("max_frames", C.c_uint32), ("reserved", C.c_uint32 * 5),
    ]


class ScreenMap(C.Structure):
    """pebblegpu_screen_map: FFT::mapFFTToScreen's plot geometry (pebblelib/fft.cpp:411-419)"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("y_pixels", C.c_int32), ("x_pixels", C.c_int32), ("max_db", C.c_double), ("min_db", C.c_double),
        ("start_freq", C.c_int32), ("stop_freq", C.c_int32), ("reserved", C.c_uint32 * 4),
    ]


def screen_map(y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq):
    m = ScreenMap()
    m.struct_size = C.sizeof(ScreenMap)
    m.y_pixels, m.x_pixels = int(y_pixels), int(x_pixels)
    m.max_db, m.min_db = float(max_db), float(min_db)
    m.start_freq, m.stop_freq = int(start_freq), int(stop_freq)
    return m


class Sweep(C.Structure):
    """pebblegpu_sweep: NCO::initSweep's arguments + the amplitude and mix switch TestBench::genSweep passes"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("sweep_type", C.c_int32), ("start_hz", C.c_double), ("stop_hz", C.c_double), ("rate_hz_per_s", C.c_double),
        ("pulse_width_s", C.c_double), ("pulse_period_s", C.c_double), ("amplitude", C.c_double), ("mix", C.c_int32), ("reserved", C.c_uint32 * 3),
    ]


SWEEP_SINGLE, SWEEP_REPEAT, SWEEP_REPEAT_REVERSE = 0, 1, 2  # NCO::SweepType
TAP_RAW_IQ, TAP_POST_MIXER, TAP_POST_BP, TAP_POST_DEMOD, TAP_MODEM = 1, 2, 3, 4, 16  # PEBBLEGPU_TAP_*


def sweep(start_hz, stop_hz, rate_hz_per_s, amplitude=1.0, sweep_type=SWEEP_REPEAT, pulse_width_s=0.0, pulse_period_s=0.0, mix=True):
    s = Sweep()
    s.struct_size = C.sizeof(Sweep)
    s.sweep_type = int(sweep_type)
    s.start_hz, s.stop_hz, s.rate_hz_per_s = float(start_hz), float(stop_hz), float(rate_hz_per_s)
    s.pulse_width_s, s.pulse_period_s = float(pulse_width_s), float(pulse_period_s)
    s.amplitude = float(amplitude)
    s.mix = 1 if mix else 0
    return s


def sweep_plan(sample_rate, s, lib=None):
    """what the library makes of a sweep, on the host (no device): (leg_samples, pulse_period_samples, pulse_on_samples)"""
    L = lib or load_library()
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(L, L.pebblegpu_sweep_plan(float(sample_rate), C.byref(s), C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


MORSE_MAX_STATIONS = 256  # PEBBLEGPU_MORSE_MAX_STATIONS


class MorseStation(C.Structure):
    """pebblegpu_morse_station: MorseGen::setParams' arguments (amplitude linear) and the text as MorseCode tokens (0: a word space)"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("wpm", C.c_uint32), ("ms_rise", C.c_uint32), ("n_tokens", C.c_uint32),
        ("frequency_hz", C.c_double), ("amplitude", C.c_double), ("tokens", C.POINTER(C.c_uint16)), ("reserved", C.c_uint32 * 2),
    ]


def morse_station(frequency_hz, amplitude, wpm, ms_rise, tokens):
    """tokens: MorseCode tokens (a leading 1, then 1 per dash and 0 per dot; 0: a word space).  The struct keeps its token array alive."""
    st = MorseStation()
    st.struct_size = C.sizeof(MorseStation)
    st.wpm, st.ms_rise = int(wpm), int(ms_rise)
    st.frequency_hz, st.amplitude = float(frequency_hz), float(amplitude)
    toks = [int(t) for t in tokens]
    st._tokens = (C.c_uint16 * max(1, len(toks)))(*toks)
    st.tokens = C.cast(st._tokens, C.POINTER(C.c_uint16))
    st.n_tokens = len(toks)
    return st


def _station_array(stations):
    stations = list(stations or [])
    arr = (MorseStation * max(1, len(stations)))()
    for i, st in enumerate(stations):
        C.memmove(C.byref(arr[i]), C.byref(st), C.sizeof(MorseStation))
    return arr, len(stations), stations  # (the third keeps the token arrays alive over the call)


def morse_station_plan(sample_rate, st, lib=None):
    """what the library makes of a station, on the host (no device): (samples_per_tcw, rise_samples, dot_samples, dash_samples, period_samples)"""
    L = lib or load_library()
    v = [C.c_uint64() for _ in range(5)]
    check(L, L.pebblegpu_morse_station_plan(float(sample_rate), C.byref(st), *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def morse_station_marks(sample_rate, st, first_sample, n, lib=None):
    """the library's mark table for a call of n samples that begins first_sample samples after the station was set, on the host:
    [(start relative to the call's first sample, is_dash)]"""
    L = lib or load_library()
    cap, cnt = 4096, C.c_uint32()
    while True:
        buf = (C.c_int64 * cap)()
        rc = L.pebblegpu_morse_station_marks(float(sample_rate), C.byref(st), int(first_sample), int(n), buf, cap, C.byref(cnt))
        if rc == -5 and cnt.value > cap:  # PEBBLEGPU_E_SIZE
            cap = cnt.value
            continue
        check(L, rc)
        return [(int(v) >> 1, bool(int(v) & 1)) for v in buf[:cnt.value]]


def _frame_range(frames, first_frame, n_frames, frame_step):
    """None for first_frame maps the last frame; None for n_frames every frame from first_frame on at frame_step"""
    if first_frame is None:
        first_frame = frames - 1 if frames else 0
    if n_frames is None:
        n_frames = max(0, (frames - first_frame + frame_step - 1) // frame_step) if frame_step else 1
    return int(first_frame), int(n_frames), int(frame_step)


def _download_i32(L, device, p, shape):
    out = np.empty(shape, dtype=np.int32)
    if out.size:
        check(L, L.pebblegpu_memcpy_d2h(device, out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes))
    return out


# pebblegpu_morse_event as a numpy record: (sample, token, kind); kind MORSE_CHAR carries the dot-dash token, MORSE_WORD_SPACE " "
MORSE_EVENT = np.dtype([("sample", np.uint64), ("token", np.uint32), ("kind", np.uint32)])
MORSE_CHAR, MORSE_WORD_SPACE = 0, 1


class MorseReport(C.Structure):
    """pebblegpu_morse_report: what Morse::refreshOutput shows (morse.cpp:477-500)"""
    _fields_ = [("wpm", C.c_int32), ("above_range", C.c_int32), ("below_range", C.c_int32),
                ("modem_rate", C.c_uint32), ("samples_per_result", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def morse_token_to_dotdash(token):
    """The dot-dash string MorseCode::tokenLookup takes for a token (the inverse of tokenizeDotDash, morsecode.cpp:160-185)"""
    token = int(token)
    if token < 2:
        return ""
    n = token.bit_length() - 1
    return "".join("-" if (token >> (n - 1 - i)) & 1 else "." for i in range(n))


def _morse_events(L, fn, *args, cap=4096):
    out = []
    while True:
        ev = np.zeros(cap, dtype=MORSE_EVENT)
        n = C.c_uint32(0)
        check(L, fn(*args, ev.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        out.append(ev[:n.value].copy())
        if n.value < cap:
            return np.concatenate(out)


class Info(C.Structure):
    _fields_ = [
        ("demod_rate", C.c_double), ("demod_rate_int", C.c_uint32), ("dec_by2_stages", C.c_uint32),
        ("total_decimation", C.c_uint32), ("chain_len", C.c_uint32), ("stage_taps", C.c_uint32 * 16),
        ("stage_stride", C.c_uint32 * 16), ("superframe", C.c_uint64), ("n_streams", C.c_uint32),
        ("spectrum_bins", C.c_uint32),
    ]


AUDIO_F32, AUDIO_S16, AUDIO_S16_MONO = range(3)  # pebblegpu_audio_format
_AUDIO_DTYPE = {AUDIO_F32: (np.float32, 2), AUDIO_S16: (np.int16, 2), AUDIO_S16_MONO: (np.int16, 1)}  # element type, elements per sample


class AudioBlock(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_uint32), ("call_index", C.c_uint64), ("host", C.c_void_p),
                ("samples_per_channel", C.c_uint64), ("pitch_bytes", C.c_uint64), ("n_channels", C.c_uint32), ("dropped_before", C.c_uint32)]


def _block_array(b):
    """a copy of the block's rows: [rows, samples, 2] (float32 or int16), [rows, samples] for the mono format"""
    dt, per = _AUDIO_DTYPE[int(b.format)]
    rows, n, pitch = int(b.n_channels), int(b.samples_per_channel), int(b.pitch_bytes)
    out = np.zeros((rows, n, per), dtype=dt)
    if n:
        raw = np.ctypeslib.as_array(C.cast(b.host, C.POINTER(C.c_uint8)), shape=(rows * pitch,)).reshape(rows, pitch)
        out = raw[:, : n * per * np.dtype(dt).itemsize].copy().view(dt).reshape(rows, n, per)
    return out[:, :, 0] if per == 1 else out


class ModemBlock(C.Structure):
    """pebblegpu_modem_block: the modem hook's rows of one call, with the trailer's presence flags"""
    _fields_ = AudioBlock._fields_ + [("rate", C.c_uint32), ("n_superframes", C.c_uint32), ("samples_per_superframe", C.c_uint64),
                                      ("present", C.POINTER(C.c_uint8))]


MODEM_RATE_MAX_STAGES = 16


class ModemRateInfo(C.Structure):
    """pebblegpu_modem_rate_info: the chain of a modem ring at a modem rate"""
    _fields_ = [("struct_size", C.c_uint32), ("rate_int", C.c_uint32), ("rate", C.c_float), ("total_decimation", C.c_uint32), ("n_stages", C.c_uint32),
                ("lookback", C.c_uint32), ("samples_per_superframe", C.c_uint64), ("taps", C.c_uint32 * MODEM_RATE_MAX_STAGES),
                ("stride", C.c_uint32 * MODEM_RATE_MAX_STAGES)]

    def chain(self):
        """[(taps, stride)], as oracle.Decimator.chain()"""
        return [(int(self.taps[j]), int(self.stride[j])) for j in range(self.n_stages)]


DISPLAY_DB_F32, DISPLAY_PIXELS_I32, DISPLAY_WATERFALL_ARGB32 = range(3)  # pebblegpu_display_format
_DISPLAY_DTYPE = {DISPLAY_DB_F32: np.float32, DISPLAY_PIXELS_I32: np.int32, DISPLAY_WATERFALL_ARGB32: np.uint32}


class DisplayBlock(C.Structure):
    """pebblegpu_display_block: the display rows one stream-bank call computed, in pinned host memory"""
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_uint32), ("call_index", C.c_uint64), ("host", C.c_void_p),
                ("rows_per_stream", C.c_uint32), ("first_row", C.c_uint32), ("row_elems", C.c_uint32), ("n_streams", C.c_uint32),
                ("dropped_before", C.c_uint32), ("reserved", C.c_uint32), ("row_pitch_bytes", C.c_uint64), ("stream_pitch_bytes", C.c_uint64)]


def _display_array(b):
    """a copy of the block's rows: [streams, rows, row_elems] float32 (dB), int32 (pixels) or uint32 (0xFFRRGGBB)"""
    dt = _DISPLAY_DTYPE[int(b.format)]
    S, R, E = int(b.n_streams), int(b.rows_per_stream), int(b.row_elems)
    if not R:
        return np.zeros((S, 0, E), dtype=dt)
    sp, rp = int(b.stream_pitch_bytes), int(b.row_pitch_bytes)
    raw = np.ctypeslib.as_array(C.cast(b.host, C.POINTER(C.c_uint8)), shape=(S * sp,)).reshape(S, sp)[:, : R * rp].reshape(S, R, rp)
    return raw[:, :, : 4 * E].copy().view(dt).reshape(S, R, E)


PANE_SPECTRUM, PANE_ZOOM = range(2)  # pebblegpu_pane_source
DISPLAY_MAX_PANES = 2                 # PEBBLEGPU_DISPLAY_MAX_PANES


class DisplayPane(C.Structure):
    """pebblegpu_display_pane: one pane of the receiver's display ring (display_pane(...) fills one and keeps its arrays alive)"""
    _fields_ = [("struct_size", C.c_uint32), ("source", C.c_uint32), ("format", C.c_uint32), ("max_rows", C.c_uint32), ("map", ScreenMap),
                ("zoom", C.c_double), ("mode_offset", C.POINTER(C.c_int32)), ("rows", C.POINTER(C.c_uint32)), ("n_rows", C.c_uint32),
                ("reserved", C.c_uint32 * 5)]


def display_pane(source, fmt, screen=None, zoom=1.0, mode_offset=None, rows=None, max_rows=0):
    """screen: a ScreenMap for the two mapped formats (a zoomed pane reads y_pixels, x_pixels, max_db, min_db of it); mode_offset: one int per
    channel of the receiver (zoomed panes; None: all 0); rows: the selected streams / channels in block order (None: all)"""
    p = DisplayPane()
    p.struct_size = C.sizeof(DisplayPane)
    p.source, p.format, p.max_rows, p.zoom = int(source), int(fmt), int(max_rows), float(zoom)
    if screen is not None:
        p.map = screen
    if mode_offset is not None:
        p._off = (C.c_int32 * max(1, len(mode_offset)))(*[int(v) for v in mode_offset])
        p.mode_offset = C.cast(p._off, C.POINTER(C.c_int32))
    if rows is not None:
        p._rows = (C.c_uint32 * max(1, len(rows)))(*[int(v) for v in rows])
        p.rows = C.cast(p._rows, C.POINTER(C.c_uint32))
        p.n_rows = len(rows)
    return p


AUTO_SCALE_MAX, AUTO_SCALE_MIN = 1, 2  # PEBBLEGPU_AUTO_SCALE_*


class DisplayScale(C.Structure):
    """pebblegpu_display_scale: the plot range SpectrumWidget::recalcScale gives one spectrum row, and the powers it came from"""
    _fields_ = [("max_db", C.c_int32), ("min_db", C.c_int32), ("avg_power", C.c_double), ("peak_power", C.c_double)]


# the same 24 bytes as a numpy record (what the pull functions and display_scale() return)
DISPLAY_SCALE = np.dtype([("max_db", np.int32), ("min_db", np.int32), ("avg_power", np.float64), ("peak_power", np.float64)])


def auto_scale_row(db, lib=None):
    """host twin of the auto-scale rule (no device): one row of float dB -> (max_db, min_db, avg_power, peak_power)"""
    L = lib or load_library()
    row = np.ascontiguousarray(db, dtype=np.float32).reshape(-1)
    out = DisplayScale()
    check(L, L.pebblegpu_auto_scale_row(row.ctypes.data_as(C.c_void_p), row.size, C.byref(out)))
    return int(out.max_db), int(out.min_db), float(out.avg_power), float(out.peak_power)


class StreamGateEntry(C.Structure):
    """pebblegpu_stream_gate: one (selected stream, frame) of a stream-bank IQ block's trailer"""
    _fields_ = [("peak_db", C.c_float), ("avg_db", C.c_float), ("snr_db", C.c_float), ("floor_db", C.c_float), ("open", C.c_uint32), ("row", C.c_uint32)]


# the same 24 bytes as a numpy record (what StreamBank.iq_out_gate returns)
STREAM_GATE = np.dtype([("peak_db", np.float32), ("avg_db", np.float32), ("snr_db", np.float32), ("floor_db", np.float32),
                        ("open", np.uint32), ("row", np.uint32)])
GATE_ROW_CARRIED, GATE_ROW_NONE = 0xFFFFFFFE, 0xFFFFFFFF  # PEBBLEGPU_GATE_ROW_*


def signal_strength_row(db, sample_rate, bp_lo, bp_hi, mixer_freq=0.0, lib=None):
    """host twin of the S-meter rule (SignalStrength::fdEstimate, no device): one row of float dB -> float32 [4] (peakDb, avgDb, snrDb, floorDb)"""
    L = lib or load_library()
    row = np.ascontiguousarray(db, dtype=np.float32).reshape(-1)
    out = np.zeros(4, dtype=np.float32)
    check(L, L.pebblegpu_signal_strength_row(row.ctypes.data_as(C.c_void_p), row.size, int(sample_rate), float(bp_lo), float(bp_hi), float(mixer_freq),
                                             out.ctypes.data_as(C.c_void_p)))
    return out


def _pull_scale(obj, fn, frames, first_frame, n_frames, frame_step):
    """the pull functions' shared body: queue, synchronise, download -> DISPLAY_SCALE [streams, n_frames]"""
    if first_frame is None and n_frames is None:
        n_frames = 1
    first_frame, n_frames, frame_step = _frame_range(frames, first_frame, n_frames, frame_step)
    out = np.zeros((obj.n_streams, n_frames), dtype=DISPLAY_SCALE)
    buf = DeviceBuffer(max(1, out.nbytes), obj.device, obj.L)
    try:
        check(obj.L, fn(obj.h, first_frame, n_frames, frame_step, C.c_void_p(buf.ptr)))
        obj.synchronize()
        if out.size:
            check(obj.L, obj.L.pebblegpu_memcpy_d2h(obj.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(buf.ptr), out.nbytes))
        return out
    finally:
        buf.free()


def _ring_scale(L, fn, h, call_index, cap):
    out = np.zeros(max(1, int(cap)), dtype=DISPLAY_SCALE)
    n = C.c_uint32()
    check(L, fn(h, int(call_index), out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)))
    return out[: n.value].copy()


def waterfall_colors(pixels, lib=None):
    """the host twin of the waterfall's colour rule (SpectrumWidget::drawWaterfall): int32 pixel values 0..255 -> uint32 0xFFRRGGBB, same shape"""
    L = lib or load_library()
    px = np.ascontiguousarray(pixels, dtype=np.int32)
    out = np.zeros(px.shape, dtype=np.uint32)
    check(L, L.pebblegpu_waterfall_colors(px.ctypes.data_as(C.c_void_p), px.size, out.ctypes.data_as(C.c_void_p)))
    return out


def audio_out_convert(fmt, gain, mute, lr, lib=None):
    """the host twin of the audio packing kernel: lr float32 [n, 2] (or complex64 [n]) -> [n, 2] float32 / int16, [n] int16 for the mono format"""
    L = lib or load_library()
    lr = np.ascontiguousarray(lr)
    if np.iscomplexobj(lr):
        lr = lr.astype(np.complex64).view(np.float32)
    lr = np.ascontiguousarray(lr, dtype=np.float32).reshape(-1, 2)
    n = lr.shape[0]
    if int(fmt) not in _AUDIO_DTYPE:
        out = np.zeros(1, dtype=np.float32)  # (the call refuses the format itself)
    else:
        dt, per = _AUDIO_DTYPE[int(fmt)]
        out = np.zeros((n, per), dtype=dt)
    check(L, L.pebblegpu_audio_out_convert(int(fmt), float(gain), 1 if mute else 0, lr.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)))
    return out[:, 0] if out.shape[1] == 1 else out


def iq_record_convert(iq, lib=None):
    """the host twin of the recording kernel: float32 [n, 2] (or complex64 [n]) -> int16 [n, 2], left = I, right = Q"""
    L = lib or load_library()
    iq = np.ascontiguousarray(iq)
    if np.iscomplexobj(iq):
        iq = iq.astype(np.complex64).view(np.float32)
    iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1, 2)
    out = np.zeros(iq.shape, dtype=np.int16)
    check(L, L.pebblegpu_iq_record_convert(iq.ctypes.data_as(C.c_void_p), iq.shape[0], out.ctypes.data_as(C.c_void_p)))
    return out


def modem_out_convert(fmt, iq, lib=None):
    """the host twin of the modem ring's packing kernel: float32 [n, 2] (or complex64 [n]) -> [n, 2] float32 (verbatim) or int16 (the record rule)"""
    L = lib or load_library()
    iq = np.ascontiguousarray(iq)
    if np.iscomplexobj(iq):
        iq = iq.astype(np.complex64).view(np.float32)
    iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1, 2)
    out = np.zeros(iq.shape, dtype=np.int16 if int(fmt) == AUDIO_S16 else np.float32)
    check(L, L.pebblegpu_modem_out_convert(int(fmt), iq.ctypes.data_as(C.c_void_p), iq.shape[0], out.ctypes.data_as(C.c_void_p)))
    return out


def modem_out_layout(fmt, n_channels, samples_per_channel, n_superframes, lib=None):
    """-> (pitch_bytes, trailer_offset, trailer_bytes) of a modem block"""
    L = lib or load_library()
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(L, L.pebblegpu_modem_out_layout(int(fmt), int(n_channels), int(samples_per_channel), int(n_superframes), C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def modem_rate_plan(demod_rate, samples_per_superframe, max_bw, min_rate=0, lib=None):
    """-> ModemRateInfo for Decimator::buildDecimationChain(demod_rate, max_bw, min_rate) on super-frames of that many demodulator samples;
    raises with the code a modem_out_open at that rate would"""
    L = lib or load_library()
    info = ModemRateInfo()
    info.struct_size = C.sizeof(ModemRateInfo)
    check(L, L.pebblegpu_modem_rate_plan(int(demod_rate), int(samples_per_superframe), int(max_bw), int(min_rate), C.byref(info)))
    return info


def library_path():
    return os.path.join(_HERE, _LIBNAME)


_lib = None


def _declare(L):
    vp, u32, u64, i32, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
    dp = C.POINTER(C.c_double)
    L.pebblegpu_last_error.restype = C.c_char_p
    L.pebblegpu_malloc.argtypes = [i32, C.c_size_t, C.POINTER(vp)]
    L.pebblegpu_free.argtypes = [i32, vp]
    L.pebblegpu_memcpy_h2d.argtypes = [i32, vp, vp, C.c_size_t]
    L.pebblegpu_memcpy_d2h.argtypes = [i32, vp, vp, C.c_size_t]
    L.pebblegpu_memset.argtypes = [i32, vp, i32, C.c_size_t]
    L.pebblegpu_device_synchronize.argtypes = [i32]
    L.pebblegpu_normalize_iq.argtypes = [i32, i32, i32, dbl, vp, u64, vp]
    L.pebblegpu_probe_copy_gbps.argtypes = [i32, i32, C.c_size_t, i32, C.POINTER(C.c_float)]
    L.pebblegpu_live_bytes.argtypes = [C.POINTER(u64), C.POINTER(u64)]
    L.pebblegpu_receiver_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.pebblegpu_receiver_destroy.argtypes = [vp]
    L.pebblegpu_receiver_info.argtypes = [vp, C.POINTER(Info)]
    L.pebblegpu_set_mixer_freq.argtypes = [vp, u32, dbl]
    L.pebblegpu_set_bandpass.argtypes = [vp, u32, dbl, dbl]
    L.pebblegpu_set_demod_mode.argtypes = [vp, u32, i32]
    L.pebblegpu_set_agc.argtypes = [vp, u32, i32, i32]
    L.pebblegpu_set_conditioners.argtypes = [vp, u32, i32, dbl, dbl]
    L.pebblegpu_set_noise_filter.argtypes = [vp, u32, i32]
    L.pebblegpu_set_squelch.argtypes = [vp, u32, C.c_double]
    L.pebblegpu_receiver_process.argtypes = [vp, vp, u64]
    L.pebblegpu_receiver_process_raw.argtypes = [vp, i32, i32, C.c_double, vp, u64]
    L.pebblegpu_receiver_audio.restype = vp
    L.pebblegpu_receiver_audio.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.pebblegpu_receiver_spectrum.restype = vp
    L.pebblegpu_receiver_spectrum.argtypes = [vp, C.POINTER(u64)]
    L.pebblegpu_receiver_zoom_spectrum.restype = vp
    L.pebblegpu_receiver_zoom_spectrum.argtypes = [vp, C.POINTER(u64), C.POINTER(u32)]
    L.pebblegpu_receiver_last_ms.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.pebblegpu_receiver_mean_ms.argtypes = [vp, i32, u32, C.POINTER(C.c_float)]
    L.pebblegpu_receiver_set_profiling.argtypes = [vp, i32]
    L.pebblegpu_receiver_ingest_acquire.argtypes = [vp, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]
    L.pebblegpu_receiver_ingest_submit.argtypes = [vp, C.c_uint32, C.c_uint64]
    L.pebblegpu_receiver_process_ingested.argtypes = [vp, C.c_uint32, i32, i32, C.c_double, C.c_uint64]
    L.pebblegpu_receiver_kernel_name.restype = C.c_char_p
    L.pebblegpu_receiver_kernel_name.argtypes = [vp, i32]
    L.pebblegpu_receiver_enable_signal_strength.argtypes = [vp, i32]
    L.pebblegpu_receiver_signal_strength.restype = vp
    L.pebblegpu_receiver_signal_strength.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.pebblegpu_receiver_synchronize.argtypes = [vp]
    L.pebblegpu_process_iq.argtypes = [vp, dp, C.c_uint16, dp, C.POINTER(u32), dp]
    L.pebblegpu_process_iq_updates.argtypes = [vp, dp, C.c_uint16, dp, C.POINTER(u32), dp, C.POINTER(u32)]
    L.pebblegpu_set_spectrum_updates.argtypes = [vp, i32]
    L.pebblegpu_receiver_spectrum_frames.argtypes = [vp, i32, C.POINTER(u32), u32, C.POINTER(u32)]
    L.pebblegpu_streambank_set_spectrum_updates.argtypes = [vp, i32]
    L.pebblegpu_streambank_spectrum_frames.argtypes = [vp, C.POINTER(u32), u32, C.POINTER(u32)]
    L.pebblegpu_streambank_create.argtypes = [C.POINTER(StreamBankConfig), C.POINTER(vp)]
    L.pebblegpu_streambank_destroy.argtypes = [vp]
    L.pebblegpu_streambank_set_bandpass.argtypes = [vp, u32, dbl, dbl]
    L.pebblegpu_streambank_process.argtypes = [vp, vp, u64, u32]
    L.pebblegpu_streambank_filtered.restype = vp
    L.pebblegpu_streambank_filtered.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.pebblegpu_streambank_spectrum.restype = vp
    L.pebblegpu_streambank_spectrum.argtypes = [vp, C.POINTER(u64), C.POINTER(u32)]
    L.pebblegpu_streambank_last_ms.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.pebblegpu_streambank_synchronize.argtypes = [vp]
    L.pebblegpu_streambank_process_raw.argtypes = [vp, i32, i32, dbl, vp, u64, u32]
    L.pebblegpu_streambank_ingest_acquire.argtypes = [vp, u32, u64, C.POINTER(vp)]
    L.pebblegpu_streambank_ingest_submit.argtypes = [vp, u32, u64]
    L.pebblegpu_streambank_process_ingested.argtypes = [vp, u32, i32, i32, dbl, u64, u32]
    L.pebblegpu_streambank_kernel_name.restype = C.c_char_p
    L.pebblegpu_streambank_kernel_name.argtypes = [vp, i32]
    # stand-alone steps
    L.pebblegpu_mixer_create.argtypes = [i32, u32, u32, C.POINTER(vp)]
    L.pebblegpu_mixer_destroy.argtypes = [vp]
    L.pebblegpu_mixer_set_frequency.argtypes = [vp, dbl]
    L.pebblegpu_mixer_process.argtypes = [vp, dp, C.POINTER(dp)]
    L.pebblegpu_decimator_create.argtypes = [i32, u32, u32, C.POINTER(vp)]
    L.pebblegpu_decimator_destroy.argtypes = [vp]
    L.pebblegpu_decimator_build_chain.argtypes = [vp, u32, u32, u32, C.POINTER(C.c_float)]
    L.pebblegpu_decimator_dec_by2_stages.argtypes = [vp, C.POINTER(u32)]
    L.pebblegpu_decimator_process.argtypes = [vp, dp, dp, u32, C.POINTER(u32)]
    L.pebblegpu_downconvert_create.argtypes = [i32, u32, C.POINTER(vp)]
    L.pebblegpu_downconvert_destroy.argtypes = [vp]
    L.pebblegpu_downconvert_set_data_rate.argtypes = [vp, C.c_double, C.c_double, i32, C.POINTER(C.c_double)]
    L.pebblegpu_downconvert_set_frequency.argtypes = [vp, C.c_double]
    L.pebblegpu_downconvert_set_cw_offset.argtypes = [vp, C.c_double]
    L.pebblegpu_downconvert_stages.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), u32]
    L.pebblegpu_downconvert_process.argtypes = [vp, u32, dp, dp, C.POINTER(u32)]
    L.pebblegpu_downconvert_process_device.argtypes = [vp, vp, u32, C.POINTER(vp), C.POINTER(u32)]
    L.pebblegpu_downconvert_synchronize.argtypes = [vp]
    L.pebblegpu_fastfir_create.argtypes = [i32, u32, u32, C.POINTER(vp)]
    L.pebblegpu_fastfir_destroy.argtypes = [vp]
    L.pebblegpu_fastfir_setup.argtypes = [vp, dbl, dbl, dbl, dbl]
    L.pebblegpu_fastfir_process.argtypes = [vp, i32, dp, dp, C.POINTER(i32)]
    L.pebblegpu_demod_create.argtypes = [i32, u32, u32, u32, C.POINTER(vp)]
    L.pebblegpu_demod_destroy.argtypes = [vp]
    L.pebblegpu_demod_set_mode.argtypes = [vp, i32]
    L.pebblegpu_demod_set_bandwidth.argtypes = [vp, dbl]
    L.pebblegpu_demod_process.argtypes = [vp, dp, i32, C.POINTER(dp)]
    L.pebblegpu_demod_rds_groups.argtypes = [vp, vp, vp, u32, C.POINTER(u32)]
    L.pebblegpu_demod_rds_signal.argtypes = [vp, dp, u32, C.POINTER(u32)]
    L.pebblegpu_demod_stereo_lock.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.pebblegpu_receiver_stereo_lock.argtypes = [vp, u32, C.POINTER(i32), C.POINTER(i32)]
    L.pebblegpu_receiver_rds_groups.argtypes = [vp, u32, vp, vp, u32, C.POINTER(u32)]
    L.pebblegpu_spectrum_create.argtypes = [i32, u32, dbl, u32, C.POINTER(vp)]
    L.pebblegpu_spectrum_destroy.argtypes = [vp]
    L.pebblegpu_spectrum_bins.argtypes = [vp, C.POINTER(u32)]
    L.pebblegpu_spectrum_process.argtypes = [vp, dp, i32, dp, C.POINTER(i32)]
    smp, ip = C.POINTER(ScreenMap), C.POINTER(C.c_int32)
    L.pebblegpu_receiver_map_spectrum.argtypes = [vp, smp, u32, u32, u32, vp]
    L.pebblegpu_receiver_map_zoom_spectrum.argtypes = [vp, C.c_int32, C.c_int32, dbl, dbl, dbl, ip, u32, u32, u32, vp]
    L.pebblegpu_streambank_map_spectrum.argtypes = [vp, smp, u32, u32, u32, vp]
    L.pebblegpu_spectrum_map_to_screen.argtypes = [vp, smp, ip]
    L.pebblegpu_set_morse.argtypes = [vp, u32, i32]
    L.pebblegpu_receiver_morse_events.argtypes = [vp, u32, vp, u32, C.POINTER(u32)]
    L.pebblegpu_receiver_morse_status.argtypes = [vp, u32, C.POINTER(MorseReport)]
    L.pebblegpu_morse_create.argtypes = [i32, u32, u32, C.POINTER(vp)]
    L.pebblegpu_morse_destroy.argtypes = [vp]
    L.pebblegpu_morse_set_demod_mode.argtypes = [vp, i32]
    L.pebblegpu_morse_process.argtypes = [vp, dp]
    L.pebblegpu_morse_events.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.pebblegpu_morse_status.argtypes = [vp, C.POINTER(MorseReport)]
    L.pebblegpu_morse_results.argtypes = [vp, dp, vp, u32, C.POINTER(u32)]
    L.pebblegpu_morse_set_sample_rate.argtypes = [vp, u32, u32]
    L.pebblegpu_morse_keep_results.argtypes = [vp, i32]
    swp, u64p = C.POINTER(Sweep), C.POINTER(u64)
    L.pebblegpu_sweep_plan.argtypes = [dbl, swp, u64p, u64p, u64p]
    L.pebblegpu_set_testbench_sweep.argtypes = [vp, swp]
    L.pebblegpu_set_testbench_noise.argtypes = [vp, dbl, u64]
    msp = C.POINTER(MorseStation)
    L.pebblegpu_morse_station_plan.argtypes = [dbl, msp, u64p, u64p, u64p, u64p, u64p]
    L.pebblegpu_morse_station_marks.argtypes = [dbl, msp, u64, u64, C.POINTER(C.c_int64), u32, C.POINTER(u32)]
    L.pebblegpu_set_testbench_morse.argtypes = [vp, msp, u32, i32]
    L.pebblegpu_siggen_set_morse.argtypes = [vp, msp, u32, i32]
    L.pebblegpu_receiver_set_taps.argtypes = [vp, u32]
    L.pebblegpu_receiver_tap.restype = vp
    L.pebblegpu_receiver_tap.argtypes = [vp, i32, u64p, u64p, dp]
    L.pebblegpu_receiver_conditioned.restype = vp
    L.pebblegpu_receiver_conditioned.argtypes = [vp, u64p, u64p]
    L.pebblegpu_siggen_create.argtypes = [i32, dbl, u32, C.POINTER(vp)]
    L.pebblegpu_siggen_destroy.argtypes = [vp]
    L.pebblegpu_siggen_set_sweep.argtypes = [vp, swp]
    L.pebblegpu_siggen_set_noise.argtypes = [vp, dbl, u64]
    L.pebblegpu_siggen_set_stream.argtypes = [vp, u32]
    L.pebblegpu_siggen_generate_device.argtypes = [vp, vp, u64]
    L.pebblegpu_siggen_synchronize.argtypes = [vp]
    L.pebblegpu_siggen_generate.argtypes = [vp, dp, u32]
    L.pebblegpu_siggen_noise_draws.argtypes = [vp, u64, u32, vp, vp]
    u32p, vpp = C.POINTER(u32), C.POINTER(vp)
    L.pebblegpu_multibank_plan.argtypes = [u32, u32, u32p, u32p]
    L.pebblegpu_multibank_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_int32), u32, u32, vpp]
    L.pebblegpu_multibank_destroy.argtypes = [vp]
    L.pebblegpu_multibank_shards.argtypes = [vp, u32p]
    L.pebblegpu_multibank_shard.argtypes = [vp, u32, vpp, C.POINTER(C.c_int32), u32p, u32p]
    L.pebblegpu_multibank_locate.argtypes = [vp, u32, u32p, u32p]
    L.pebblegpu_multibank_process.argtypes = [vp, vpp, u64]
    L.pebblegpu_multibank_process_raw.argtypes = [vp, i32, i32, dbl, vpp, u64]
    L.pebblegpu_multibank_ingest_acquire.argtypes = [vp, u32, u64, vpp]
    L.pebblegpu_multibank_ingest_submit.argtypes = [vp, u32, u64]
    L.pebblegpu_multibank_process_ingested.argtypes = [vp, u32, i32, i32, dbl, u64]
    L.pebblegpu_multibank_synchronize.argtypes = [vp]
    L.pebblegpu_multibank_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    blk = C.POINTER(AudioBlock)
    L.pebblegpu_receiver_audio_out_open.argtypes = [vp, i32, u32p, u32, u32]
    L.pebblegpu_receiver_audio_out_close.argtypes = [vp]
    L.pebblegpu_set_audio_level.argtypes = [vp, u32, C.c_float, i32]
    L.pebblegpu_receiver_audio_out_next.argtypes = [vp, i32, blk]
    L.pebblegpu_receiver_audio_out_release.argtypes = [vp, u64]
    L.pebblegpu_receiver_audio_out_dropped.argtypes = [vp, C.POINTER(u64)]
    L.pebblegpu_audio_out_convert.argtypes = [i32, C.c_float, i32, vp, u64, vp]
    L.pebblegpu_receiver_record_open.argtypes = [vp, u32]
    L.pebblegpu_receiver_record_close.argtypes = [vp]
    L.pebblegpu_receiver_record_next.argtypes = [vp, i32, blk]
    L.pebblegpu_receiver_record_release.argtypes = [vp, u64]
    L.pebblegpu_iq_record_convert.argtypes = [vp, u64, vp]
    L.pebblegpu_receiver_modem_out_open.argtypes = [vp, i32, u32p, u32, u32]
    L.pebblegpu_receiver_modem_out_open_rate.argtypes = [vp, i32, u32p, u32, u32, u32, u32]
    L.pebblegpu_modem_rate_plan.argtypes = [u32, u64, u32, u32, C.POINTER(ModemRateInfo)]
    L.pebblegpu_receiver_modem_out_close.argtypes = [vp]
    L.pebblegpu_receiver_modem_out_next.argtypes = [vp, i32, C.POINTER(ModemBlock)]
    L.pebblegpu_receiver_modem_out_release.argtypes = [vp, u64]
    L.pebblegpu_receiver_modem_out_dropped.argtypes = [vp, C.POINTER(u64)]
    L.pebblegpu_modem_out_convert.argtypes = [i32, vp, u64, vp]
    L.pebblegpu_modem_out_layout.argtypes = [i32, u32, u64, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    dblk = C.POINTER(DisplayBlock)
    L.pebblegpu_streambank_iq_out_open.argtypes = [vp, i32, u32p, u32, u32]
    L.pebblegpu_streambank_iq_out_close.argtypes = [vp]
    L.pebblegpu_streambank_iq_out_next.argtypes = [vp, i32, blk]
    L.pebblegpu_streambank_iq_out_release.argtypes = [vp, u64]
    L.pebblegpu_streambank_iq_out_dropped.argtypes = [vp, C.POINTER(u64)]
    L.pebblegpu_streambank_display_open.argtypes = [vp, i32, smp, u32p, u32, u32, u32]
    L.pebblegpu_streambank_display_close.argtypes = [vp]
    L.pebblegpu_streambank_display_next.argtypes = [vp, i32, dblk]
    L.pebblegpu_streambank_display_release.argtypes = [vp, u64]
    L.pebblegpu_streambank_display_dropped.argtypes = [vp, C.POINTER(u64)]
    L.pebblegpu_waterfall_colors.argtypes = [vp, u64, vp]
    dpane = C.POINTER(DisplayPane)
    L.pebblegpu_receiver_display_open.argtypes = [vp, dpane, u32, u32]
    L.pebblegpu_receiver_display_close.argtypes = [vp]
    L.pebblegpu_receiver_display_next.argtypes = [vp, i32, dblk]
    L.pebblegpu_receiver_display_release.argtypes = [vp, u64]
    L.pebblegpu_receiver_display_dropped.argtypes = [vp, C.POINTER(u64)]
    L.pebblegpu_receiver_display_set_pane.argtypes = [vp, u32, dpane]
    L.pebblegpu_auto_scale_row.argtypes = [vp, u32, C.POINTER(DisplayScale)]
    L.pebblegpu_receiver_spectrum_scale.argtypes = [vp, u32, u32, u32, vp]
    L.pebblegpu_streambank_spectrum_scale.argtypes = [vp, u32, u32, u32, vp]
    L.pebblegpu_signal_strength_row.argtypes = [vp, u32, u32, C.c_float, C.c_float, dbl, vp]
    L.pebblegpu_streambank_enable_signal_strength.argtypes = [vp, i32]
    L.pebblegpu_streambank_signal_strength.restype = vp
    L.pebblegpu_streambank_signal_strength.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.pebblegpu_streambank_set_squelch.argtypes = [vp, u32, dbl]
    L.pebblegpu_streambank_iq_out_gate.argtypes = [vp, u64, vp, u32, C.POINTER(u32)]
    L.pebblegpu_streambank_set_conditioners.argtypes = [vp, u32, C.c_int, dbl, dbl]
    L.pebblegpu_streambank_conditioned.restype = vp
    L.pebblegpu_streambank_conditioned.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    for who in ("receiver", "streambank"):
        getattr(L, "pebblegpu_%s_display_set_auto_scale" % who).argtypes = [vp, u32]
        getattr(L, "pebblegpu_%s_display_rescale" % who).argtypes = [vp]
        getattr(L, "pebblegpu_%s_display_scale" % who).argtypes = [vp, u64, vp, u32, C.POINTER(u32)]
    return L


def load_library(path=None):
    """Load libpebblegpu.so (built in-tree by __graft_entry__.build()).  No fallback of any kind."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    p = path or library_path()
    if not os.path.exists(p):
        raise PebbleGpuError(-2, "%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                 "(hipcc --offload-arch=gfx950); there is no CPU implementation" % p)
    L = _declare(C.CDLL(p))
    if path is None:
        _lib = L
    return L


def check(L, rc):
    if rc != 0:
        raise PebbleGpuError(rc, (L.pebblegpu_last_error() or b"").decode("utf-8", "replace"))


def probe_copy_gbps(lane_bytes=16, nbytes=1 << 30, iters=10, device=0, lib=None):
    L = lib or load_library()
    g = C.c_float()
    check(L, L.pebblegpu_probe_copy_gbps(device, lane_bytes, nbytes, iters, C.byref(g)))
    return g.value


def live_bytes(lib=None):
    """(device bytes, pinned host bytes) this library holds in this process right now"""
    L = lib or load_library()
    d, p = C.c_uint64(), C.c_uint64()
    check(L, L.pebblegpu_live_bytes(C.byref(d), C.byref(p)))
    return d.value, p.value


IQ_S8, IQ_U8, IQ_S16, IQ_F32, IQ_WAV16 = range(5)
IQO_IQ, IQO_QI, IQO_IONLY, IQO_QONLY = range(4)


def normalize_iq(raw, fmt, order=IQO_IQ, gain=1.0, device=0, lib=None):
    """raw: numpy array of interleaved I,Q in the device's native type -> complex64 array converted on the GPU"""
    L = lib or load_library()
    raw = np.ascontiguousarray(raw)
    n = raw.size // 2
    src = DeviceBuffer.from_array(raw, device, L)
    dst = DeviceBuffer(8 * n, device, L)
    try:
        check(L, L.pebblegpu_normalize_iq(device, fmt, order, float(gain), C.c_void_p(src.ptr), n, C.c_void_p(dst.ptr)))
        return dst.download(np.complex64, n)
    finally:
        src.free()
        dst.free()


class DeviceBuffer:
    """A device allocation owned through the C ABI (pebblegpu_malloc / pebblegpu_free)."""

    def __init__(self, nbytes, device=0, lib=None):
        self.L = lib or load_library()
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        check(self.L, self.L.pebblegpu_malloc(device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_array(cls, a, device=0, lib=None):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes, device, lib)
        b.upload(a)
        return b

    def upload(self, a, offset=0):
        a = np.ascontiguousarray(a)
        check(self.L, self.L.pebblegpu_memcpy_h2d(self.device, C.c_void_p(self.ptr + offset), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def download(self, dtype, count, offset=0):
        out = np.empty(count, dtype=dtype)
        check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr + offset), out.nbytes))
        return out

    def free(self):
        if getattr(self, "ptr", None):
            self.L.pebblegpu_free(self.device, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def to_f32_iq(x):
    """complex array -> interleaved float32 (n, 2) device layout"""
    x = np.asarray(x)
    if x.dtype == np.complex64:
        return np.ascontiguousarray(x).view(np.float32)
    return np.ascontiguousarray(x.astype(np.complex64)).view(np.float32)


class ReceiverBank:
    """C tuned channels over one shared stream or C independent streams (pebblegpu_receiver_*)."""

    def __init__(self, sample_rate, n_channels=1, shared_input=True, wfm=False, spectrum_bins=0,
                 frames_per_buffer=2048, fastfir_fft=0, fastfir_taps=0, max_superframes=1, device=0, lib=None, audio_rate=0, hires_bins=0):
        self.L = lib or load_library()
        cfg = Config()
        cfg.struct_size = C.sizeof(Config)
        cfg.device = device
        cfg.sample_rate = float(sample_rate)
        cfg.frames_per_buffer = frames_per_buffer
        cfg.n_channels = n_channels
        cfg.shared_input = 1 if shared_input else 0
        cfg.wfm = 1 if wfm else 0
        cfg.spectrum_bins = spectrum_bins
        cfg.fastfir_fft = fastfir_fft
        cfg.fastfir_taps = fastfir_taps
        cfg.max_superframes = max_superframes
        cfg.audio_rate = audio_rate
        cfg.hires_bins = hires_bins
        self.h = C.c_void_p()
        check(self.L, self.L.pebblegpu_receiver_create(C.byref(cfg), C.byref(self.h)))
        self._read_info(device, n_channels, frames_per_buffer)

    def _read_info(self, device, n_channels, frames_per_buffer):
        self.device = device
        self.n_channels = n_channels
        self.nf = frames_per_buffer
        info = Info()
        check(self.L, self.L.pebblegpu_receiver_info(self.h, C.byref(info)))
        self.info = info
        self.superframe = int(info.superframe)
        self.n_streams = int(info.n_streams)
        self.bins = int(info.spectrum_bins)
        self.D = int(info.total_decimation)

    def chain(self):
        return [(int(self.info.stage_taps[i]), int(self.info.stage_stride[i])) for i in range(self.info.chain_len)]

    @classmethod
    def borrowed(cls, handle, device, n_channels, frames_per_buffer, lib=None):
        """a view over a receiver handle somebody else owns (a MultiBank's shard): every setter and read-out, but close() leaves the handle alone"""
        self = cls.__new__(cls)
        self.L = lib or load_library()
        self._borrowed = True
        self.h = C.c_void_p(handle)
        self._read_info(device, n_channels, frames_per_buffer)
        return self

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            if not getattr(self, "_borrowed", False):
                self.L.pebblegpu_receiver_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_mixer(self, ch, f):
        check(self.L, self.L.pebblegpu_set_mixer_freq(self.h, ch, float(f)))

    def set_bandpass(self, ch, lo, hi):
        check(self.L, self.L.pebblegpu_set_bandpass(self.h, ch, float(lo), float(hi)))

    def set_mode(self, ch, mode):
        check(self.L, self.L.pebblegpu_set_demod_mode(self.h, ch, int(mode)))

    def stereo_lock(self, ch):
        """Demod_WFM::getStereoLock of a dmFMS channel -> (pilot lock of the last frame, changed since the last call)"""
        lk, chg = C.c_int32(0), C.c_int32(0)
        check(self.L, self.L.pebblegpu_receiver_stereo_lock(self.h, ch, C.byref(lk), C.byref(chg)))
        return bool(lk.value), bool(chg.value)

    def rds_groups(self, ch, cap=4096):
        """dmFMS channel of a WFM bank: what Demod::fmStereo popped from the RDS group queue since the last call ->
        ((n, 4) uint16 blocks A..D, (n,) bool: getNextRdsGroupData's return value)"""
        g = np.zeros((cap, 4), dtype=np.uint16)
        chg = np.zeros(cap, dtype=np.uint8)
        n = C.c_uint32(0)
        check(self.L, self.L.pebblegpu_receiver_rds_groups(self.h, ch, g.ctypes.data_as(C.c_void_p), chg.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return g[:n.value].copy(), chg[:n.value].astype(bool)

    def set_morse(self, ch, on=True):
        """Receiver::setDigitalModem("Morse") on a channel (on) or off: the Morse decoder behind the noise filter"""
        check(self.L, self.L.pebblegpu_set_morse(self.h, ch, 1 if on else 0))

    def morse_events(self, ch):
        """the channel's Morse events since the last read -> MORSE_EVENT records (sample, token, kind), oldest first"""
        return _morse_events(self.L, self.L.pebblegpu_receiver_morse_events, self.h, ch)

    def morse_status(self, ch):
        st = MorseReport()
        check(self.L, self.L.pebblegpu_receiver_morse_status(self.h, ch, C.byref(st)))
        return st.as_dict()

    def set_testbench_sweep(self, s):
        """TestBench::reset + the sweep generator at the head of the chain; s: a Sweep (see sweep()), None switches it off"""
        check(self.L, self.L.pebblegpu_set_testbench_sweep(self.h, C.byref(s) if s is not None else None))

    def set_testbench_morse(self, stations, mix=True):
        """MorseGen stations at the head of the chain (see morse_station()); replaces the set and restarts it, None or [] switches it off"""
        arr, n, _keep = _station_array(stations)
        check(self.L, self.L.pebblegpu_set_testbench_morse(self.h, arr, n, 1 if mix else 0))

    def set_testbench_noise(self, amplitude, seed=0):
        """NCO::genNoise at the head of the chain, always mixed; amplitude <= 0 switches it off"""
        check(self.L, self.L.pebblegpu_set_testbench_noise(self.h, float(amplitude), int(seed)))

    def set_taps(self, points):
        """points: iterable of TAP_* (empty: every tap off)"""
        mask = 0
        for p in points:
            mask |= 1 << int(p)
        check(self.L, self.L.pebblegpu_receiver_set_taps(self.h, mask))

    def tap(self, point):
        """-> (complex64 [rows, n] of the last call at that point, rate in Hz); None when the point is off or was not reached"""
        n, pitch, rate = C.c_uint64(), C.c_uint64(), C.c_double()
        p = self.L.pebblegpu_receiver_tap(self.h, int(point), C.byref(n), C.byref(pitch), C.byref(rate))
        if not p:
            return None
        self.synchronize()
        rows = self.n_streams if int(point) == TAP_RAW_IQ else self.n_channels
        out = np.empty((rows, int(n.value)), dtype=np.complex64)
        for r in range(rows):
            check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out[r].ctypes.data_as(C.c_void_p), C.c_void_p(p + r * int(pitch.value) * 8), out[r].nbytes))
        return out, rate.value

    def set_conditioners(self, stream, flags, iq_gain=1.0, iq_phase=0.0):
        check(self.L, self.L.pebblegpu_set_conditioners(self.h, stream, int(flags), float(iq_gain), float(iq_phase)))

    def conditioned(self):
        """-> complex64 [streams, n]: the conditioned rows the last call's spectrum and mixer read, or None when it conditioned nothing"""
        n, pitch = C.c_uint64(), C.c_uint64()
        p = self.L.pebblegpu_receiver_conditioned(self.h, C.byref(n), C.byref(pitch))
        if not p or not int(n.value):
            return None
        self.synchronize()
        out = np.empty((self.n_streams, int(n.value)), dtype=np.complex64)
        for r in range(self.n_streams):  # rows are pitched at the handle's capacity
            check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out[r].ctypes.data_as(C.c_void_p), C.c_void_p(p + r * int(pitch.value) * 8), out[r].nbytes))
        return out

    def set_noise_filter(self, ch, on=True):
        check(self.L, self.L.pebblegpu_set_noise_filter(self.h, ch, 1 if on else 0))

    def set_squelch(self, ch, squelch_db):
        """Receiver::squelchChanged: below squelch_db (avgDb of the latest spectrum) a call ends after the band-pass with no audio"""
        check(self.L, self.L.pebblegpu_set_squelch(self.h, ch, float(squelch_db)))

    def set_agc(self, ch, agc_mode, threshold):
        check(self.L, self.L.pebblegpu_set_agc(self.h, ch, int(agc_mode), int(threshold)))

    def set_spectrum_updates(self, updates_per_sec):
        """SignalSpectrum::setUpdatesPerSec on the stream's sample clock: -1 every frame (default), 0 none, else spectra per second"""
        check(self.L, self.L.pebblegpu_set_spectrum_updates(self.h, int(updates_per_sec)))

    def spectrum_frames(self, zoomed=False):
        """-> uint32 [n]: which frames of the last call (relative to its first) the rows of spectrum() / zoom_spectrum() belong to"""
        f = C.c_uint64()
        if zoomed:
            self.L.pebblegpu_receiver_zoom_spectrum(self.h, C.byref(f), None)
        else:
            self.L.pebblegpu_receiver_spectrum(self.h, C.byref(f))
        idx = np.zeros(max(1, int(f.value)), dtype=np.uint32)
        n = C.c_uint32()
        check(self.L, self.L.pebblegpu_receiver_spectrum_frames(self.h, 1 if zoomed else 0, idx.ctypes.data_as(C.POINTER(C.c_uint32)), len(idx), C.byref(n)))
        return idx[: n.value].copy()

    def process_device(self, dptr, n_samples):
        check(self.L, self.L.pebblegpu_receiver_process(self.h, C.c_void_p(dptr), int(n_samples)))

    def process_raw_device(self, dptr, n_samples, fmt, iq_order=0, gain=1.0):
        """raw device-format IQ pairs (pebblegpu_iq_format) already on the device, aligned to PEBBLEGPU_RAW_ALIGN (32) bytes: converted in the first
        kernels' own loads where the call's shape allows it, through a normalizeIQ pass otherwise (input_route() says which)"""
        check(self.L, self.L.pebblegpu_receiver_process_raw(self.h, int(fmt), int(iq_order), float(gain), C.c_void_p(dptr), int(n_samples)))

    def input_route(self):
        """pebblegpu_receiver_kernel_name(rx, 6): "float2", "raw s8" .. "raw wav16" (converted in the loads), "k_normalize_iq" (staged)"""
        return self.kernel_name(6)

    def ingest_buffer(self, slot, nbytes, dtype=np.int8):
        """the slot's pinned host buffer as a numpy array (valid until the slot is acquired again with a larger size)"""
        p = C.c_void_p()
        check(self.L, self.L.pebblegpu_receiver_ingest_acquire(self.h, int(slot), int(nbytes), C.byref(p)))
        n = int(nbytes) // np.dtype(dtype).itemsize
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(n,))

    def ingest_submit(self, slot, nbytes):
        check(self.L, self.L.pebblegpu_receiver_ingest_submit(self.h, int(slot), int(nbytes)))

    def process_ingested(self, slot, n_samples, fmt, iq_order=0, gain=1.0):
        check(self.L, self.L.pebblegpu_receiver_process_ingested(self.h, int(slot), int(fmt), int(iq_order), float(gain), int(n_samples)))

    def synchronize(self):
        check(self.L, self.L.pebblegpu_receiver_synchronize(self.h))

    # ---- host egress: the audio output stage and IQ recording through pinned slots ----
    def audio_out_open(self, fmt=AUDIO_F32, channels=None, n_slots=4):
        """channels: row r of every block is channel channels[r] (None: all, in order)"""
        if channels is None:
            check(self.L, self.L.pebblegpu_receiver_audio_out_open(self.h, int(fmt), None, 0, int(n_slots)))
        else:
            arr = (C.c_uint32 * max(1, len(channels)))(*[int(c) for c in channels])
            check(self.L, self.L.pebblegpu_receiver_audio_out_open(self.h, int(fmt), arr, len(channels), int(n_slots)))

    def audio_out_close(self):
        check(self.L, self.L.pebblegpu_receiver_audio_out_close(self.h))

    def set_audio_level(self, ch, gain=100.0, mute=False):
        """Receiver::m_gain (the UI's 0..100) and m_mute of one channel; takes effect at the next call"""
        check(self.L, self.L.pebblegpu_set_audio_level(self.h, int(ch), float(gain), 1 if mute else 0))

    def _egress_next(self, fn, wait):
        b = AudioBlock()
        b.struct_size = C.sizeof(AudioBlock)
        check(self.L, fn(self.h, 1 if wait else 0, C.byref(b)))
        if not b.host:
            return None
        return int(b.call_index), int(b.dropped_before), _block_array(b)

    def audio_out_next(self, wait=True):
        """-> (call_index, dropped_before, copy of the block's rows) or None; the block stays taken until audio_out_release(call_index)"""
        return self._egress_next(self.L.pebblegpu_receiver_audio_out_next, wait)

    def audio_out_release(self, call_index):
        check(self.L, self.L.pebblegpu_receiver_audio_out_release(self.h, int(call_index)))

    def audio_out_dropped(self):
        n = C.c_uint64()
        check(self.L, self.L.pebblegpu_receiver_audio_out_dropped(self.h, C.byref(n)))
        return int(n.value)

    def record_open(self, n_slots=4):
        check(self.L, self.L.pebblegpu_receiver_record_open(self.h, int(n_slots)))

    def record_close(self):
        check(self.L, self.L.pebblegpu_receiver_record_close(self.h))

    def record_next(self, wait=True):
        """-> (call_index, dropped_before, int16 [streams, n, 2]) or None"""
        return self._egress_next(self.L.pebblegpu_receiver_record_next, wait)

    def record_release(self, call_index):
        check(self.L, self.L.pebblegpu_receiver_record_release(self.h, int(call_index)))

    # ---- host egress: the modem hook ring (the rows a digital-modem plugin receives, with presence flags) ----
    def modem_out_open(self, fmt=AUDIO_F32, channels=None, n_slots=4):
        """channels: row r of every block is channel channels[r] (None: all, in order)"""
        if channels is None:
            check(self.L, self.L.pebblegpu_receiver_modem_out_open(self.h, int(fmt), None, 0, int(n_slots)))
        else:
            arr = (C.c_uint32 * max(1, len(channels)))(*[int(c) for c in channels])
            check(self.L, self.L.pebblegpu_receiver_modem_out_open(self.h, int(fmt), arr, len(channels), int(n_slots)))

    def modem_out_open_rate(self, max_bw, min_rate=0, fmt=AUDIO_F32, channels=None, n_slots=4):
        """the same ring with every row decimated on the device by Decimator::buildDecimationChain(demodulator rate, max_bw, min_rate)"""
        if channels is None:
            check(self.L, self.L.pebblegpu_receiver_modem_out_open_rate(self.h, int(fmt), None, 0, int(n_slots), int(max_bw), int(min_rate)))
        else:
            arr = (C.c_uint32 * max(1, len(channels)))(*[int(c) for c in channels])
            check(self.L, self.L.pebblegpu_receiver_modem_out_open_rate(self.h, int(fmt), arr, len(channels), int(n_slots), int(max_bw), int(min_rate)))

    def modem_out_close(self):
        check(self.L, self.L.pebblegpu_receiver_modem_out_close(self.h))

    def modem_out_next(self, wait=True):
        """-> (call_index, dropped_before, copy of the rows [rows, samples, 2], present uint8 [rows, super-frames], rate) or None; the block stays
        taken until modem_out_release(call_index)"""
        b = ModemBlock()
        b.struct_size = C.sizeof(ModemBlock)
        check(self.L, self.L.pebblegpu_receiver_modem_out_next(self.h, 1 if wait else 0, C.byref(b)))
        if not b.host:
            return None
        rows, k = int(b.n_channels), int(b.n_superframes)
        present = np.zeros((rows, k), dtype=np.uint8)
        if rows * k:
            present = np.ctypeslib.as_array(b.present, shape=(rows * k,)).copy().reshape(rows, k)
        return int(b.call_index), int(b.dropped_before), _block_array(b), present, int(b.rate)

    def modem_out_release(self, call_index):
        check(self.L, self.L.pebblegpu_receiver_modem_out_release(self.h, int(call_index)))

    def modem_out_dropped(self):
        n = C.c_uint64()
        check(self.L, self.L.pebblegpu_receiver_modem_out_dropped(self.h, C.byref(n)))
        return int(n.value)

    # ---- host egress: the display ring (one or two panes per block) ----
    def display_open(self, panes, n_slots=4):
        """panes: one or two display_pane(...) -- SpectrumWidget::newFftData's top and bottom panel"""
        arr = (DisplayPane * max(1, len(panes)))(*panes)
        check(self.L, self.L.pebblegpu_receiver_display_open(self.h, arr, len(panes), int(n_slots)))
        self._display_panes = len(panes)

    def display_close(self):
        check(self.L, self.L.pebblegpu_receiver_display_close(self.h))

    def display_set_pane(self, pane, geometry):
        """a pane's plot geometry (map, zoom, mode offsets) from the next call on; geometry: a display_pane(...) with the pane's source and format"""
        check(self.L, self.L.pebblegpu_receiver_display_set_pane(self.h, int(pane), C.byref(geometry)))

    def display_next(self, wait=True):
        """-> (call_index, dropped_before, [(first_row, copy of the pane's rows [selected, rows, row_elems]) per pane]) or None; taken until
        display_release(call_index)"""
        n = getattr(self, "_display_panes", 1)
        b = (DisplayBlock * DISPLAY_MAX_PANES)()
        for k in range(DISPLAY_MAX_PANES):
            b[k].struct_size = C.sizeof(DisplayBlock)
        check(self.L, self.L.pebblegpu_receiver_display_next(self.h, 1 if wait else 0, b))
        if not b[0].host:
            return None
        return int(b[0].call_index), int(b[0].dropped_before), [(int(b[k].first_row), _display_array(b[k])) for k in range(n)]

    def display_release(self, call_index):
        check(self.L, self.L.pebblegpu_receiver_display_release(self.h, int(call_index)))

    # ---- auto-scale (SpectrumWidget::recalcScale) ----
    def spectrum_scale(self, first_frame=None, n_frames=None, frame_step=1):
        """the auto-scale range of frames first_frame + j * frame_step of the last call's spectrum -> DISPLAY_SCALE [streams, n_frames]
        (default: the last frame only)"""
        n = C.c_uint64()
        self.L.pebblegpu_receiver_spectrum(self.h, C.byref(n))
        return _pull_scale(self, self.L.pebblegpu_receiver_spectrum_scale, int(n.value), first_frame, n_frames, frame_step)

    def display_set_auto_scale(self, flags):
        """AUTO_SCALE_MAX | AUTO_SCALE_MIN: "Auto" in the max / min dB box; a host flag, consumed by the next call (no wait)"""
        check(self.L, self.L.pebblegpu_receiver_display_set_auto_scale(self.h, int(flags)))

    def display_rescale(self):
        """m_scaleNeedsRecalc = true (an LO change): the next call that computes a spectrum row recomputes the range"""
        check(self.L, self.L.pebblegpu_receiver_display_rescale(self.h))

    def display_scale(self, call_index, cap=4096):
        """the ranges the handed-out block of call_index was mapped with -> DISPLAY_SCALE [pane 0's selected rows]"""
        return _ring_scale(self.L, self.L.pebblegpu_receiver_display_scale, self.h, call_index, cap)

    def display_dropped(self):
        n = C.c_uint64()
        check(self.L, self.L.pebblegpu_receiver_display_dropped(self.h, C.byref(n)))
        return int(n.value)

    def enable_signal_strength(self, on=True):
        check(self.L, self.L.pebblegpu_receiver_enable_signal_strength(self.h, 1 if on else 0))

    def signal_strength(self):
        """-> float32 [C, frames, 4] = (peakDb, avgDb, snrDb, floorDb) of the last call"""
        f, pitch = C.c_uint64(), C.c_uint64()
        p = self.L.pebblegpu_receiver_signal_strength(self.h, C.byref(f), C.byref(pitch))
        self.synchronize()
        out = np.empty((self.n_channels, int(f.value), 4), dtype=np.float32)
        for c in range(self.n_channels if out.size else 0):
            check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out[c].ctypes.data_as(C.c_void_p), C.c_void_p(p + c * int(pitch.value) * 16), out[c].nbytes))
        return out

    def set_profiling(self, per_kernel=True):
        check(self.L, self.L.pebblegpu_receiver_set_profiling(self.h, 1 if per_kernel else 0))

    def last_ms(self, which=0):
        ms = C.c_float()
        check(self.L, self.L.pebblegpu_receiver_last_ms(self.h, which, C.byref(ms)))
        return ms.value

    def kernel_name(self, which):
        return (self.L.pebblegpu_receiver_kernel_name(self.h, which) or b"").decode()

    def mean_ms(self, which=0, last_k=1):
        ms = C.c_float()
        check(self.L, self.L.pebblegpu_receiver_mean_ms(self.h, which, last_k, C.byref(ms)))
        return ms.value

    def audio(self):
        """-> complex64 [C, n] of the last call"""
        n, pitch = C.c_uint64(), C.c_uint64()
        p = self.L.pebblegpu_receiver_audio(self.h, C.byref(n), C.byref(pitch))
        n, pitch = int(n.value), int(pitch.value)
        self.synchronize()
        out = np.empty((self.n_channels, n), dtype=np.complex64)
        for c in range(self.n_channels):  # rows are pitched on the device
            check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out[c].ctypes.data_as(C.c_void_p), C.c_void_p(p + c * pitch * 8), n * 8))
        return out

    def spectrum(self):
        """-> float32 [streams, frames, bins] of the last call"""
        n = C.c_uint64()
        p = self.L.pebblegpu_receiver_spectrum(self.h, C.byref(n))
        frames = int(n.value)
        self.synchronize()
        out = np.empty((self.n_streams, frames, self.bins), dtype=np.float32)
        if out.size:  # (a gated call may have computed no row)
            check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes))
        return out

    def zoom_spectrum(self):
        """-> float32 [C, frames, hires_bins]: SignalSpectrum::zoomed of every decimated frame of the last call"""
        f, b = C.c_uint64(), C.c_uint32()
        p = self.L.pebblegpu_receiver_zoom_spectrum(self.h, C.byref(f), C.byref(b))
        self.synchronize()
        out = np.empty((self.n_channels, int(f.value), int(b.value)), dtype=np.float32)
        if out.size:
            check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes))
        return out

    def map_spectrum_device(self, d_out, y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq, first_frame, n_frames, frame_step=1):
        """queue FFT::mapFFTToScreen of the last call's spectrum into the device buffer d_out (int32 [streams, n_frames, x_pixels])"""
        m = screen_map(y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq)
        check(self.L, self.L.pebblegpu_receiver_map_spectrum(self.h, C.byref(m), int(first_frame), int(n_frames), int(frame_step), C.c_void_p(d_out)))

    def map_zoom_spectrum_device(self, d_out, y_pixels, x_pixels, max_db, min_db, zoom, mode_offset, first_frame, n_frames, frame_step=1):
        """queue SignalSpectrum::mapFFTZoomedToScreen of the last call's zoomed spectra into d_out (int32 [channels, n_frames, x_pixels])"""
        off = None
        if mode_offset is not None:
            off = np.ascontiguousarray(np.broadcast_to(np.asarray(mode_offset, dtype=np.int32), (self.n_channels,)))
        check(self.L, self.L.pebblegpu_receiver_map_zoom_spectrum(self.h, int(y_pixels), int(x_pixels), float(max_db), float(min_db), float(zoom),
                                                                  off.ctypes.data_as(C.POINTER(C.c_int32)) if off is not None else None,
                                                                  int(first_frame), int(n_frames), int(frame_step), C.c_void_p(d_out)))

    def map_spectrum(self, y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq, first_frame=None, n_frames=None, frame_step=1):
        """FFT::mapFFTToScreen on the device -> int32 [streams, n_frames, x_pixels]; frames first_frame + j * frame_step of the
        last call (default: its last frame only when first_frame is None, every frame from first_frame on otherwise)"""
        n = C.c_uint64()
        self.L.pebblegpu_receiver_spectrum(self.h, C.byref(n))
        if first_frame is None and n_frames is None:
            n_frames = 1
        first_frame, n_frames, frame_step = _frame_range(int(n.value), first_frame, n_frames, frame_step)
        buf = DeviceBuffer(4 * max(1, self.n_streams * n_frames * int(x_pixels)), self.device, self.L)
        try:
            self.map_spectrum_device(buf.ptr, y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq, first_frame, n_frames, frame_step)
            self.synchronize()
            return _download_i32(self.L, self.device, buf.ptr, (self.n_streams, n_frames, int(x_pixels)))
        finally:
            buf.free()

    def map_zoom_spectrum(self, y_pixels, x_pixels, max_db, min_db, zoom=1.0, mode_offset=None, first_frame=None, n_frames=None, frame_step=1):
        """SignalSpectrum::mapFFTZoomedToScreen per channel on the device -> int32 [channels, n_frames, x_pixels]"""
        f, b = C.c_uint64(), C.c_uint32()
        self.L.pebblegpu_receiver_zoom_spectrum(self.h, C.byref(f), C.byref(b))
        if first_frame is None and n_frames is None:
            n_frames = 1
        first_frame, n_frames, frame_step = _frame_range(int(f.value), first_frame, n_frames, frame_step)
        buf = DeviceBuffer(4 * max(1, self.n_channels * n_frames * int(x_pixels)), self.device, self.L)
        try:
            self.map_zoom_spectrum_device(buf.ptr, y_pixels, x_pixels, max_db, min_db, zoom, mode_offset, first_frame, n_frames, frame_step)
            self.synchronize()
            return _download_i32(self.L, self.device, buf.ptr, (self.n_channels, n_frames, int(x_pixels)))
        finally:
            buf.free()

    def process(self, iq):
        """iq: complex [streams, n] (or [n] for one stream).  Returns (audio [C, n/D], spectrum or None)."""
        iq = np.atleast_2d(np.asarray(iq))
        assert iq.shape[0] == self.n_streams, "expected %d streams" % self.n_streams
        buf = DeviceBuffer.from_array(to_f32_iq(iq), self.device, self.L)
        try:
            self.process_device(buf.ptr, iq.shape[1])
            a = self.audio()
            s = self.spectrum() if self.bins else None
        finally:
            buf.free()
        return a, s

    def process_iq(self, frame, want_spectrum=False):
        """Host single-frame path (CB_ProcessIQData shape).  -> (audio complex128 [n_audio], spectrum or None)"""
        x = np.ascontiguousarray(frame, dtype=np.complex128)
        dp = C.POINTER(C.c_double)
        cap = max(self.nf, self.superframe // self.D)
        audio = np.empty(cap, dtype=np.complex128)
        spec = np.empty(self.bins, dtype=np.float64) if (want_spectrum and self.bins) else None
        n_audio = C.c_uint32()
        check(self.L, self.L.pebblegpu_process_iq(self.h, x.ctypes.data_as(dp), len(x), audio.ctypes.data_as(dp), C.byref(n_audio),
                                                 spec.ctypes.data_as(dp) if spec is not None else None))
        return audio[: n_audio.value].copy(), spec

    def process_iq_updates(self, frame, spectrum):
        """pebblegpu_process_iq_updates: `spectrum` (float64 [bins]) is the host's own buffer, overwritten only when the frame got a
        spectrum.  -> (audio complex128 [n_audio], updated)"""
        x = np.ascontiguousarray(frame, dtype=np.complex128)
        dp = C.POINTER(C.c_double)
        assert spectrum.dtype == np.float64 and spectrum.flags.c_contiguous and spectrum.size == self.bins
        audio = np.empty(max(self.nf, self.superframe // self.D), dtype=np.complex128)
        n_audio, upd = C.c_uint32(), C.c_uint32()
        check(self.L, self.L.pebblegpu_process_iq_updates(self.h, x.ctypes.data_as(dp), len(x), audio.ctypes.data_as(dp), C.byref(n_audio),
                                                         spectrum.ctypes.data_as(dp), C.byref(upd)))
        return audio[: n_audio.value].copy(), bool(upd.value)


class SigGen:
    """The test bench's generator as a stand-alone step (pebblegpu_siggen_*): NCO::genSweep + NCO::genNoise on one stream"""

    def __init__(self, sample_rate, frames_per_buffer=2048, device=0, lib=None):
        self.L = lib or load_library()
        self.h = C.c_void_p()
        check(self.L, self.L.pebblegpu_siggen_create(device, float(sample_rate), int(frames_per_buffer), C.byref(self.h)))
        self.device = device

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.pebblegpu_siggen_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sweep(self, s):
        check(self.L, self.L.pebblegpu_siggen_set_sweep(self.h, C.byref(s) if s is not None else None))

    def set_noise(self, amplitude, seed=0):
        check(self.L, self.L.pebblegpu_siggen_set_noise(self.h, float(amplitude), int(seed)))

    def set_morse(self, stations, mix=True):
        arr, n, _keep = _station_array(stations)
        check(self.L, self.L.pebblegpu_siggen_set_morse(self.h, arr, n, 1 if mix else 0))

    def set_stream(self, stream):
        check(self.L, self.L.pebblegpu_siggen_set_stream(self.h, int(stream)))

    def generate_device(self, dptr, n):
        """the next n samples into the device float2 buffer at dptr, in place; queued"""
        check(self.L, self.L.pebblegpu_siggen_generate_device(self.h, C.c_void_p(dptr), int(n)))

    def synchronize(self):
        check(self.L, self.L.pebblegpu_siggen_synchronize(self.h))

    def generate(self, frame):
        """TestBench::genSweep + genNoise on a host frame (complex128, modified in place and returned)"""
        assert frame.dtype == np.complex128 and frame.flags.c_contiguous
        check(self.L, self.L.pebblegpu_siggen_generate(self.h, frame.ctypes.data_as(C.POINTER(C.c_double)), len(frame)))
        return frame

    def noise_draws(self, first_sample, n):
        """-> (uint32 [n, 2] accepted draws, uint8 [n] accepted attempt) of the generator's stream and seed, from the device"""
        r = np.zeros((n, 2), dtype=np.uint32)
        a = np.zeros(n, dtype=np.uint8)
        check(self.L, self.L.pebblegpu_siggen_noise_draws(self.h, int(first_sample), int(n), r.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)))
        return r, a


class StreamBank:
    """S full-rate streams through the overlap-save band-pass and the display transform (pebblegpu_streambank_*)."""

    BANDPASS, SPECTRUM = 1, 2

    def __init__(self, sample_rate, n_streams, frame=65536, spectrum_bins=65536, fastfir_fft=0, fastfir_taps=0,
                 max_frames=1, device=0, lib=None):
        self.L = lib or load_library()
        cfg = StreamBankConfig()
        cfg.struct_size = C.sizeof(StreamBankConfig)
        cfg.device = device
        cfg.sample_rate = float(sample_rate)
        cfg.n_streams = n_streams
        cfg.frame = frame
        cfg.spectrum_bins = spectrum_bins
        cfg.fastfir_fft = fastfir_fft
        cfg.fastfir_taps = fastfir_taps
        cfg.max_frames = max_frames
        self.h = C.c_void_p()
        self.split32 = os.environ.get("PEBBLEGPU_BIG_SPLIT32") == "1"  # (the library reads its switches when the bank is created)
        check(self.L, self.L.pebblegpu_streambank_create(C.byref(cfg), C.byref(self.h)))
        self.device, self.n_streams, self.frame = device, n_streams, frame

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.pebblegpu_streambank_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_bandpass(self, stream, lo, hi):
        check(self.L, self.L.pebblegpu_streambank_set_bandpass(self.h, stream, float(lo), float(hi)))

    def set_spectrum_updates(self, updates_per_sec):
        """SignalSpectrum::setUpdatesPerSec on the bank's sample clock: -1 every frame (default), 0 none, else spectra per second"""
        check(self.L, self.L.pebblegpu_streambank_set_spectrum_updates(self.h, int(updates_per_sec)))

    def spectrum_frames(self):
        """-> uint32 [n]: which frames of the last call (relative to its first) the rows of spectrum() belong to"""
        f = C.c_uint64()
        self.L.pebblegpu_streambank_spectrum(self.h, C.byref(f), None)
        idx = np.zeros(max(1, int(f.value)), dtype=np.uint32)
        n = C.c_uint32()
        check(self.L, self.L.pebblegpu_streambank_spectrum_frames(self.h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), len(idx), C.byref(n)))
        return idx[: n.value].copy()

    def process_device(self, dptr, n_samples, what=3):
        check(self.L, self.L.pebblegpu_streambank_process(self.h, C.c_void_p(dptr), int(n_samples), int(what)))

    def process_raw_device(self, dptr, n_samples, fmt, iq_order=0, gain=1.0, what=3):
        """[streams, n_samples] raw device-format IQ pairs (pebblegpu_iq_format) already on the device, 32-byte aligned"""
        check(self.L, self.L.pebblegpu_streambank_process_raw(self.h, int(fmt), int(iq_order), float(gain), C.c_void_p(dptr), int(n_samples), int(what)))

    def ingest_acquire(self, slot, nbytes, dtype=np.int8):
        """the slot's pinned host buffer as a numpy array (valid until the slot is acquired again with a larger size)"""
        p = C.c_void_p()
        check(self.L, self.L.pebblegpu_streambank_ingest_acquire(self.h, int(slot), int(nbytes), C.byref(p)))
        n = int(nbytes) // np.dtype(dtype).itemsize
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(n,))

    def ingest_submit(self, slot, nbytes):
        check(self.L, self.L.pebblegpu_streambank_ingest_submit(self.h, int(slot), int(nbytes)))

    def process_ingested(self, slot, n_samples, fmt, iq_order=0, gain=1.0, what=3):
        check(self.L, self.L.pebblegpu_streambank_process_ingested(self.h, int(slot), int(fmt), int(iq_order), float(gain), int(n_samples), int(what)))

    def kernel_name(self, which):
        """the kernel route the last call took: which 1 band-pass, 2 display transform"""
        return (self.L.pebblegpu_streambank_kernel_name(self.h, int(which)) or b"").decode()

    def synchronize(self):
        check(self.L, self.L.pebblegpu_streambank_synchronize(self.h))

    def last_ms(self, which=0):
        ms = C.c_float()
        check(self.L, self.L.pebblegpu_streambank_last_ms(self.h, which, C.byref(ms)))
        return ms.value

    def spectrum_kernels(self):
        """label of the kernels behind last_ms(2)"""
        return ("k_big_cols + k_big_rows" if self.split32 else "k_big256_cols + k_big256_rows") if self.frame == 65536 else "k_spectrum"

    def filtered(self):
        n, pitch = C.c_uint64(), C.c_uint64()
        p = self.L.pebblegpu_streambank_filtered(self.h, C.byref(n), C.byref(pitch))
        self.synchronize()
        out = np.empty((self.n_streams, int(n.value)), dtype=np.complex64)
        if out.size:
            check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes))
        return out

    def spectrum(self):
        f, b = C.c_uint64(), C.c_uint32()
        p = self.L.pebblegpu_streambank_spectrum(self.h, C.byref(f), C.byref(b))
        self.synchronize()
        out = np.empty((self.n_streams, int(f.value), int(b.value)), dtype=np.float32)
        if out.size:
            check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes))
        return out

    def map_spectrum_device(self, d_out, y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq, first_frame, n_frames, frame_step=1):
        """queue FFT::mapFFTToScreen of the last call's spectrum into the device buffer d_out (int32 [streams, n_frames, x_pixels])"""
        m = screen_map(y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq)
        check(self.L, self.L.pebblegpu_streambank_map_spectrum(self.h, C.byref(m), int(first_frame), int(n_frames), int(frame_step), C.c_void_p(d_out)))

    def map_spectrum(self, y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq, first_frame=None, n_frames=None, frame_step=1):
        """FFT::mapFFTToScreen on the device -> int32 [streams, n_frames, x_pixels] (default: the last frame of each stream; under an
        update gate the frames are the compact rows, and after a call that selected none the latest row made before it is frame 0)"""
        f, b = C.c_uint64(), C.c_uint32()
        self.L.pebblegpu_streambank_spectrum(self.h, C.byref(f), C.byref(b))
        if first_frame is None and n_frames is None:
            n_frames = 1
        first_frame, n_frames, frame_step = _frame_range(int(f.value), first_frame, n_frames, frame_step)
        buf = DeviceBuffer(4 * max(1, self.n_streams * n_frames * int(x_pixels)), self.device, self.L)
        try:
            self.map_spectrum_device(buf.ptr, y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq, first_frame, n_frames, frame_step)
            self.synchronize()
            return _download_i32(self.L, self.device, buf.ptr, (self.n_streams, n_frames, int(x_pixels)))
        finally:
            buf.free()

    # ---- host egress: band-passed IQ and display rows through pinned slots ----
    def _stream_list(self, streams):
        if streams is None:
            return None, 0
        return (C.c_uint32 * max(1, len(streams)))(*[int(c) for c in streams]), len(streams)

    def iq_out_open(self, fmt=AUDIO_F32, streams=None, n_slots=4):
        """streams: row r of every block is stream streams[r] (None: all, in order); fmt AUDIO_F32 (verbatim) or AUDIO_S16"""
        arr, n = self._stream_list(streams)
        check(self.L, self.L.pebblegpu_streambank_iq_out_open(self.h, int(fmt), arr, n, int(n_slots)))
        self._iq_rows = self.n_streams if streams is None else len(streams)

    def iq_out_close(self):
        check(self.L, self.L.pebblegpu_streambank_iq_out_close(self.h))

    def iq_out_next(self, wait=True):
        """-> (call_index, dropped_before, copy of the rows: [streams, n, 2] float32 or int16) or None; taken until iq_out_release(call_index)"""
        b = AudioBlock()
        b.struct_size = C.sizeof(AudioBlock)
        check(self.L, self.L.pebblegpu_streambank_iq_out_next(self.h, 1 if wait else 0, C.byref(b)))
        if not b.host:
            return None
        return int(b.call_index), int(b.dropped_before), _block_array(b)

    def iq_out_release(self, call_index):
        check(self.L, self.L.pebblegpu_streambank_iq_out_release(self.h, int(call_index)))

    def iq_out_dropped(self):
        n = C.c_uint64()
        check(self.L, self.L.pebblegpu_streambank_iq_out_dropped(self.h, C.byref(n)))
        return int(n.value)

    # ---- S-meter and squelch (SignalStrength::fdEstimate, receiver.cpp:959-965) ----
    def enable_signal_strength(self, on=True):
        """host state, consumed by the next call (no wait): one more launch per call that computes spectrum rows"""
        check(self.L, self.L.pebblegpu_streambank_enable_signal_strength(self.h, 1 if on else 0))

    def signal_strength(self):
        """-> float32 [streams, rows, 4] (peakDb, avgDb, snrDb, floorDb): one entry per spectrum row the last call computed"""
        rows, pitch = C.c_uint64(), C.c_uint64()
        p = self.L.pebblegpu_streambank_signal_strength(self.h, C.byref(rows), C.byref(pitch))
        self.synchronize()
        full = np.zeros((self.n_streams, int(pitch.value), 4), dtype=np.float32)
        if int(rows.value):
            check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, full.ctypes.data_as(C.c_void_p), C.c_void_p(p), full.nbytes))
        return full[:, : int(rows.value)].copy()

    def set_squelch(self, stream, squelch_db):
        """closed = avgDb < squelch_db per (stream, frame): a closed frame is zeros in the IQ ring's block; -120 and below never closes"""
        check(self.L, self.L.pebblegpu_streambank_set_squelch(self.h, int(stream), float(squelch_db)))

    # ---- input conditioners (receiver.cpp:814-823: DCRemoval, IQBalance, NB1, NB2) ----
    def set_conditioners(self, stream, flags, iq_gain=1.0, iq_phase=0.0):
        """flags: COND_* or'ed; a host flag, consumed by the next call (no wait).  While any stream has one set every call conditions first"""
        check(self.L, self.L.pebblegpu_streambank_set_conditioners(self.h, int(stream), int(flags), float(iq_gain), float(iq_phase)))

    def conditioned(self):
        """-> complex64 [streams, n]: the rows the last call's transforms read, or None when it conditioned nothing"""
        n, pitch = C.c_uint64(), C.c_uint64()
        p = self.L.pebblegpu_streambank_conditioned(self.h, C.byref(n), C.byref(pitch))
        if not p or not int(n.value):
            return None
        self.synchronize()
        out = np.empty((self.n_streams, int(pitch.value)), dtype=np.complex64)
        check(self.L, self.L.pebblegpu_memcpy_d2h(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes))
        return out[:, : int(n.value)]

    def iq_out_gate(self, call_index, cap=1 << 16):
        """the gate trailer of the handed-out IQ block of call_index -> STREAM_GATE [selected streams, frames]"""
        out = np.zeros(max(1, int(cap)), dtype=STREAM_GATE)
        n = C.c_uint32()
        check(self.L, self.L.pebblegpu_streambank_iq_out_gate(self.h, int(call_index), out.ctypes.data_as(C.c_void_p), int(cap), C.byref(n)))
        frames = int(n.value)
        if not frames:
            return out[:0].reshape(0, 0)
        return out.reshape(-1)[: (len(out) // frames) * frames].reshape(-1, frames)[: self._iq_rows].copy()

    def display_open(self, fmt=DISPLAY_DB_F32, screen=None, streams=None, max_rows=0, n_slots=4):
        """screen: a ScreenMap (screen_map(...)) for the two mapped formats; max_rows 0: the bank's max_frames"""
        arr, n = self._stream_list(streams)
        check(self.L, self.L.pebblegpu_streambank_display_open(self.h, int(fmt), C.byref(screen) if screen is not None else None, arr, n,
                                                               int(max_rows), int(n_slots)))

    def display_close(self):
        check(self.L, self.L.pebblegpu_streambank_display_close(self.h))

    def display_next(self, wait=True):
        """-> (call_index, dropped_before, first_row, copy of the rows [streams, rows, row_elems]) or None; taken until display_release(call_index)"""
        b = DisplayBlock()
        b.struct_size = C.sizeof(DisplayBlock)
        check(self.L, self.L.pebblegpu_streambank_display_next(self.h, 1 if wait else 0, C.byref(b)))
        if not b.host:
            return None
        return int(b.call_index), int(b.dropped_before), int(b.first_row), _display_array(b)

    def display_release(self, call_index):
        check(self.L, self.L.pebblegpu_streambank_display_release(self.h, int(call_index)))

    # ---- auto-scale (SpectrumWidget::recalcScale) ----
    def spectrum_scale(self, first_frame=None, n_frames=None, frame_step=1):
        """the auto-scale range of frames first_frame + j * frame_step of the last call's spectrum -> DISPLAY_SCALE [streams, n_frames]"""
        f = C.c_uint64()
        self.L.pebblegpu_streambank_spectrum(self.h, C.byref(f), None)
        return _pull_scale(self, self.L.pebblegpu_streambank_spectrum_scale, int(f.value), first_frame, n_frames, frame_step)

    def display_set_auto_scale(self, flags):
        """AUTO_SCALE_MAX | AUTO_SCALE_MIN; a host flag, consumed by the next call (no wait)"""
        check(self.L, self.L.pebblegpu_streambank_display_set_auto_scale(self.h, int(flags)))

    def display_rescale(self):
        check(self.L, self.L.pebblegpu_streambank_display_rescale(self.h))

    def display_scale(self, call_index, cap=4096):
        """the ranges the handed-out block of call_index was mapped with -> DISPLAY_SCALE [selected streams]"""
        return _ring_scale(self.L, self.L.pebblegpu_streambank_display_scale, self.h, call_index, cap)

    def display_dropped(self):
        n = C.c_uint64()
        check(self.L, self.L.pebblegpu_streambank_display_dropped(self.h, C.byref(n)))
        return int(n.value)

    def process(self, iq, what=3):
        """iq: complex [streams, n] -> (filtered [S, n] or None, spectrum [S, frames, bins] or None); under an update gate
        (set_spectrum_updates) frames counts the computed rows only, spectrum_frames() says which they are"""
        iq = np.atleast_2d(np.asarray(iq))
        assert iq.shape[0] == self.n_streams
        buf = DeviceBuffer.from_array(to_f32_iq(iq), self.device, self.L)
        try:
            self.process_device(buf.ptr, iq.shape[1], what)
            y = self.filtered() if what & 1 else None
            s = self.spectrum() if what & 2 else None
        finally:
            buf.free()
        return y, s


MULTIBANK_MAX_SHARDS = 16       # PEBBLEGPU_MULTIBANK_MAX_SHARDS
MULTIBANK_SPECTRUM_SHARD0 = 1   # PEBBLEGPU_MULTIBANK_SPECTRUM_SHARD0


def multibank_plan(n_channels, n_shards, lib=None):
    """pebblegpu_multibank_plan, on the host (no device): [(first, count)] -- shard g owns the channels [g*C/G, (g+1)*C/G)"""
    L = lib or load_library()
    first, count = (C.c_uint32 * MULTIBANK_MAX_SHARDS)(), (C.c_uint32 * MULTIBANK_MAX_SHARDS)()
    check(L, L.pebblegpu_multibank_plan(int(n_channels), int(n_shards), first, count))
    return [(int(first[g]), int(count[g])) for g in range(int(n_shards))]


class MultiBank:
    """A bank's channels sharded across devices, driven from this one process (pebblegpu_multibank_*).  device_ids may repeat a
    device ([0, 0]: two shards on one GPU, a test rig).  Channels are global; shard(g) is a ReceiverBank view of shard g."""

    def __init__(self, sample_rate, n_channels, device_ids, flags=0, shared_input=True, wfm=False, spectrum_bins=0,
                 frames_per_buffer=2048, fastfir_fft=0, fastfir_taps=0, max_superframes=1, lib=None, audio_rate=0, hires_bins=0):
        self.L = lib or load_library()
        cfg = Config()
        cfg.struct_size = C.sizeof(Config)
        cfg.sample_rate = float(sample_rate)
        cfg.frames_per_buffer = frames_per_buffer
        cfg.n_channels = n_channels
        cfg.shared_input = 1 if shared_input else 0
        cfg.wfm = 1 if wfm else 0
        cfg.spectrum_bins = spectrum_bins
        cfg.fastfir_fft = fastfir_fft
        cfg.fastfir_taps = fastfir_taps
        cfg.max_superframes = max_superframes
        cfg.audio_rate = audio_rate
        cfg.hires_bins = hires_bins
        ids = [int(d) for d in device_ids]
        arr = (C.c_int32 * max(1, len(ids)))(*ids)
        self.h = C.c_void_p()
        check(self.L, self.L.pebblegpu_multibank_create(C.byref(cfg), arr, len(ids), int(flags), C.byref(self.h)))
        self.n_channels, self.shared_input, self.nf = n_channels, bool(shared_input), frames_per_buffer
        g = C.c_uint32()
        check(self.L, self.L.pebblegpu_multibank_shards(self.h, C.byref(g)))
        self.n_shards = int(g.value)
        self.shards, self.ranges, self.devices = [], [], []
        for k in range(self.n_shards):
            rx, dev, first, cnt = C.c_void_p(), C.c_int32(), C.c_uint32(), C.c_uint32()
            check(self.L, self.L.pebblegpu_multibank_shard(self.h, k, C.byref(rx), C.byref(dev), C.byref(first), C.byref(cnt)))
            self.shards.append(ReceiverBank.borrowed(rx.value, int(dev.value), int(cnt.value), frames_per_buffer, self.L))
            self.ranges.append((int(first.value), int(cnt.value)))
            self.devices.append(int(dev.value))
        self.superframe = self.shards[0].superframe
        self.D = self.shards[0].D

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            for s in self.shards:
                s.close()  # (views: they only forget the handle)
            self.L.pebblegpu_multibank_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard(self, g):
        """the ReceiverBank view of shard g (channels local to the shard; it does not own the handle)"""
        return self.shards[g]

    def locate(self, ch):
        """global channel -> (shard, channel within the shard)"""
        g, c = C.c_uint32(), C.c_uint32()
        check(self.L, self.L.pebblegpu_multibank_locate(self.h, int(ch), C.byref(g), C.byref(c)))
        return int(g.value), int(c.value)

    def _at(self, ch):
        g, c = self.locate(ch)
        return self.shards[g], c

    def set_mixer(self, ch, f):
        s, c = self._at(ch)
        s.set_mixer(c, f)

    def set_bandpass(self, ch, lo, hi):
        s, c = self._at(ch)
        s.set_bandpass(c, lo, hi)

    def set_mode(self, ch, mode):
        s, c = self._at(ch)
        s.set_mode(c, mode)

    def set_morse(self, ch, on=True):
        s, c = self._at(ch)
        s.set_morse(c, on)

    def morse_events(self, ch):
        s, c = self._at(ch)
        return s.morse_events(c)

    def morse_status(self, ch):
        s, c = self._at(ch)
        return s.morse_status(c)

    def _ptrs(self, dptrs):
        assert len(dptrs) == self.n_shards, "one device pointer per shard"
        return (C.c_void_p * self.n_shards)(*[C.c_void_p(int(p)) for p in dptrs])

    def process_device(self, dptrs, n_samples):
        """dptrs[g]: float2 input resident on shard g's device (the whole shared stream, or the shard's rows)"""
        check(self.L, self.L.pebblegpu_multibank_process(self.h, self._ptrs(dptrs), int(n_samples)))

    def process_raw_device(self, dptrs, n_samples, fmt, iq_order=0, gain=1.0):
        check(self.L, self.L.pebblegpu_multibank_process_raw(self.h, int(fmt), int(iq_order), float(gain), self._ptrs(dptrs), int(n_samples)))

    def ingest_buffer(self, slot, nbytes, dtype=np.int8):
        """the multibank's pinned host slot as a numpy array: [n] pairs of a shared stream, [C][n] pairs of independent streams"""
        p = C.c_void_p()
        check(self.L, self.L.pebblegpu_multibank_ingest_acquire(self.h, int(slot), int(nbytes), C.byref(p)))
        n = int(nbytes) // np.dtype(dtype).itemsize
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(n,))

    def ingest_submit(self, slot, nbytes):
        check(self.L, self.L.pebblegpu_multibank_ingest_submit(self.h, int(slot), int(nbytes)))

    def process_ingested(self, slot, n_samples, fmt, iq_order=0, gain=1.0):
        check(self.L, self.L.pebblegpu_multibank_process_ingested(self.h, int(slot), int(fmt), int(iq_order), float(gain), int(n_samples)))

    def synchronize(self):
        check(self.L, self.L.pebblegpu_multibank_synchronize(self.h))

    def last_ms(self):
        """the slowest shard's time of the last call (pebblegpu_receiver_last_ms(rx, 0) maximised over the shards)"""
        ms = C.c_float()
        check(self.L, self.L.pebblegpu_multibank_last_ms(self.h, C.byref(ms)))
        return ms.value

    def audio(self):
        """-> complex64 [C, n] of the last call: the shards' rows concatenated in global channel order"""
        self.synchronize()
        return np.concatenate([s.audio() for s in self.shards], axis=0)

    def process(self, iq):
        """iq: host complex [n] (shared stream) or [C, n] (independent streams), uploaded per shard.  -> audio [C, n/D]"""
        iq = np.atleast_2d(np.asarray(iq))
        assert iq.shape[0] == (1 if self.shared_input else self.n_channels), "expected %d streams" % (1 if self.shared_input else self.n_channels)
        bufs = []
        try:
            for g, (first, cnt) in enumerate(self.ranges):
                rows = iq if self.shared_input else iq[first:first + cnt]
                bufs.append(DeviceBuffer.from_array(to_f32_iq(rows), self.devices[g], self.L))
            self.process_device([b.ptr for b in bufs], iq.shape[1])
            return self.audio()
        finally:
            for b in bufs:
                b.free()
