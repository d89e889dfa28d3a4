"""Time the Morse digital modem's added cost per receiver call: the same bank with the modem on every channel against the modem off.

  configs[2]        2.048 Msps shared stream -> 256 CWU channels, 8 super-frames per call (64 kHz demodulator rate; modem chain
                    hb11 x4 + hb15 to 8 kHz, N = 80)
  configs[3] shard  100 Msps shared stream -> 512 CWU channels, 1 super-frame per call (48828 Hz; modem 6103 Hz, N = 61)

A host clock around `reps` calls queued back to back and one synchronise, after warm-up calls; the two banks alternate, best of
three.  Prints one JSON line per shape.  The events are left in the device logs, so the calls include the host's drain of the
logs whenever they could wrap (every log_cap / results-per-call calls: a host wait for the call in flight and a copy of every
channel's log, which the per-call figure averages in).  Kernel times: run under `rocprofv3 --kernel-trace --stats`
(k_morse_fir, k_morse_tails, k_morse_goertzel, k_morse_decide).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pebblesdr_amd as P  # noqa: E402
from pebblesdr_amd.binding import check  # noqa: E402
from tests.signals import lcg_noise  # noqa: E402


def make(fs, C, max_sf, morse):
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=max_sf)
    for c in range(C):
        rx.set_mixer(c, -0.45 * fs + 0.9 * fs * c / C)
        rx.set_bandpass(c, 300, 3000)
        if morse:
            rx.set_morse(c, True)
        rx.set_mode(c, P.DM_CWU)
    return rx


def timed(rx, dbuf, n, reps):
    """every return code is checked: a refused or failed call must not be timed as a fast one"""
    L = rx.L
    for _ in range(3):
        check(L, L.pebblegpu_receiver_process(rx.h, dbuf.ptr, n))
    check(L, L.pebblegpu_receiver_synchronize(rx.h))
    t0 = time.perf_counter()
    for _ in range(reps):
        check(L, L.pebblegpu_receiver_process(rx.h, dbuf.ptr, n))
    check(L, L.pebblegpu_receiver_synchronize(rx.h))
    return (time.perf_counter() - t0) * 1e3 / reps


def shape(name, fs, C, sf_per_call, reps):
    off, on = make(fs, C, sf_per_call, False), make(fs, C, sf_per_call, True)
    n = off.superframe * sf_per_call
    x = (lcg_noise(n, 7, 1e-3)).astype(np.complex64)
    dbuf = P.DeviceBuffer.from_array(x, 0, off.L)
    t_off, t_on = [], []
    for _ in range(3):
        t_off.append(timed(off, dbuf, n, reps))
        t_on.append(timed(on, dbuf, n, reps))
    st = on.morse_status(0)
    nd = n // off.D                                             # demodulator-rate samples per channel per call
    dm = int(round(fs / off.D / st["modem_rate"]))              # the modem chain's decimation
    print(json.dumps({"shape": name, "channels": C, "samples_per_call": n, "demod_samples_per_channel": nd,
                      "modem_rate": st["modem_rate"], "samples_per_result": st["samples_per_result"],
                      "results_per_channel_per_call": round(nd / dm / st["samples_per_result"], 1),
                      "modem_read_MB": round(C * nd * 8 / 1e6, 1),
                      "ms_per_call_off": round(min(t_off), 4), "ms_per_call_on": round(min(t_on), 4),
                      "added_ms": round(min(t_on) - min(t_off), 4), "runs_off": [round(t, 4) for t in t_off],
                      "runs_on": [round(t, 4) for t in t_on], "reps": reps}), flush=True)
    dbuf.free()
    off.close()
    on.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--only", choices=["c2", "c3"])
    a = ap.parse_args()
    if a.only in (None, "c2"):
        shape("configs[2]", 2048000, 256, 8, a.reps)
    if a.only in (None, "c3"):
        shape("configs[3] shard", 100e6, 512, 1, a.reps)
