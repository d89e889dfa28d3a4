"""pebblesdr_amd -- MI355X-native IQ receive chain behind PebbleSDR's plugin surface.

The product is the HIP library `libpebblegpu.so` (C ABI: include/pebblegpu.h).  This package is the
thin Python face used by the tests and the bench: ctypes bindings plus numpy conveniences.  There is
no CPU implementation here: importing works anywhere, but every compute call needs the built
library and a HIP device and fails loudly otherwise.
"""
from .binding import (  # noqa: F401
    PebbleGpuError, load_library, library_path, ReceiverBank, StreamBank, DeviceBuffer, ScreenMap, screen_map,
    MORSE_EVENT, MORSE_CHAR, MORSE_WORD_SPACE, morse_token_to_dotdash, SPECTRUM_EVERY_FRAME,
    DM_AM, DM_SAM, DM_FMN, DM_FMM, DM_FMS, DM_DSB, DM_LSB, DM_USB, DM_CWL, DM_CWU, DM_DIGL, DM_DIGU, DM_NONE,
    SigGen, Sweep, sweep, sweep_plan, SWEEP_SINGLE, SWEEP_REPEAT, SWEEP_REPEAT_REVERSE,
    TAP_RAW_IQ, TAP_POST_MIXER, TAP_POST_BP, TAP_POST_DEMOD, TAP_MODEM,
    MorseStation, morse_station, morse_station_plan, morse_station_marks, MORSE_MAX_STATIONS,
    MultiBank, multibank_plan, MULTIBANK_MAX_SHARDS, MULTIBANK_SPECTRUM_SHARD0,
    AUDIO_F32, AUDIO_S16, AUDIO_S16_MONO, AudioBlock, audio_out_convert, iq_record_convert, ModemBlock, modem_out_convert, modem_out_layout,
    ModemRateInfo, modem_rate_plan, MODEM_RATE_MAX_STAGES,
    DISPLAY_DB_F32, DISPLAY_PIXELS_I32, DISPLAY_WATERFALL_ARGB32, DisplayBlock, waterfall_colors,
    PANE_SPECTRUM, PANE_ZOOM, DisplayPane, display_pane,
    AUTO_SCALE_MAX, AUTO_SCALE_MIN, DisplayScale, DISPLAY_SCALE, auto_scale_row,
    StreamGateEntry, STREAM_GATE, GATE_ROW_CARRIED, GATE_ROW_NONE, signal_strength_row,
    COND_DC, COND_IQBALANCE, COND_NB1, COND_NB2,
)
from .steps import Mixer, Decimator, DownConvert, FastFIR, Demod, Spectrum, Morse  # noqa: F401

__all__ = [
    "PebbleGpuError", "load_library", "library_path", "ReceiverBank", "StreamBank", "DeviceBuffer", "ScreenMap", "screen_map",
    "Mixer", "Decimator", "DownConvert", "FastFIR", "Demod", "Spectrum", "Morse", "morse_token_to_dotdash",
    "SigGen", "Sweep", "sweep", "sweep_plan", "MorseStation", "morse_station", "morse_station_plan",
    "MultiBank", "multibank_plan", "audio_out_convert", "iq_record_convert", "ModemBlock", "modem_out_convert", "modem_out_layout", "ModemRateInfo", "modem_rate_plan", "DisplayBlock", "waterfall_colors",
    "PANE_SPECTRUM", "PANE_ZOOM", "DisplayPane", "display_pane",
    "AUTO_SCALE_MAX", "AUTO_SCALE_MIN", "DisplayScale", "DISPLAY_SCALE", "auto_scale_row",
    "StreamGateEntry", "STREAM_GATE", "GATE_ROW_CARRIED", "GATE_ROW_NONE", "signal_strength_row",
]
