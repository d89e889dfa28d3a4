"""Time FFT::mapFFTToScreen on the device (k_screen_map) for the two shapes DESIGN.md quotes:

  bank   the last frame of each stream of a 128-stream, 65536-bin stream bank (configs[4] shard), to 1024 pixels
  every  every frame of a configs[1] call (256 super-frames = 16384 frames x 8192 bins at 20 Msps), to 1024 pixels: the
         waterfall's worst case

A host clock around `reps` maps queued back to back and one synchronise (the library queues its kernels on private streams;
a map's launch overlaps the previous map's kernel), after warm-up maps.  Prints one JSON line per shape: ms per map, the bytes
it must read (the dB rows it covers) and write (the pixels), the rate over those bytes, and the count of fp64 exp10 it runs.
Kernel times alone: run under `rocprofv3 --kernel-trace --stats` (k_screen_map<G>).
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pebblesdr_amd as P  # noqa: E402
from tests import screen_map_ref as R  # noqa: E402

PEAK_GBS = 8000.0  # MI355X HBM3E datasheet


def timed(fn, reps, sync):
    fn()
    fn()
    sync()
    best = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        best.append((time.perf_counter() - t0) * 1e3 / reps)
    return min(best), best


def averaged_bins(fft, fs, start, stop, xp):
    """bins the averaged branch sums per row (one exp10 each)"""
    g = R.geometry(fft, fs, start, stop, xp)
    b = R.pixel_bins(g, xp).astype(np.int64)
    last = np.concatenate([[-1], b[:-1]])
    avg = (b >= 0) & (b < fft) & g["averaged"] & (last > 0) & (b != last + 1)
    return int((b - last)[avg].sum())


def report(name, rows, fft, xp, fs, start, stop, ms, runs, extra):
    read = rows * fft * 4
    write = rows * xp * 4
    exp10 = rows * averaged_bins(fft, fs, start, stop, xp)
    d = {"shape": name, "rows": rows, "bins": fft, "x_pixels": xp, "ms_per_map": round(ms, 5), "runs_ms": [round(r, 5) for r in runs],
         "bytes_read": read, "bytes_written": write, "GBps": round((read + write) / ms / 1e6, 1),
         "frac_of_8TBps": round((read + write) / ms / 1e6 / PEAK_GBS, 3), "fp64_exp10": exp10}
    d.update(extra)
    print(json.dumps(d), flush=True)


def bank(reps):
    fs, S, N, F = 200e6, 128, 65536, 4
    sb = P.StreamBank(fs, S, frame=N, spectrum_bins=N, max_frames=F)
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((S, F * N)) + 1j * rng.standard_normal((S, F * N))).astype(np.complex64) * 0.05
    buf = P.DeviceBuffer.from_array(x.view(np.float32), 0)
    out = P.DeviceBuffer(4 * S * 1024, 0)
    sb.process_device(buf.ptr, F * N, 2)
    sb.synchronize()
    ms, runs = timed(lambda: sb.map_spectrum_device(out.ptr, 255, 1024, 0.0, -120.0, -100_000_000, 100_000_000, F - 1, 1), reps, sb.synchronize)
    report("bank_last_frames", S, N, 1024, fs, -100_000_000, 100_000_000, ms, runs, {"streams": S, "frames_per_call": F})
    buf.free()
    out.free()
    sb.close()


def every(reps):
    fs, bins, K = 20_000_000, 8192, 256
    rx = P.ReceiverBank(fs, 1, True, True, bins, max_superframes=K)
    n = K * rx.superframe
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * 0.1
    buf = P.DeviceBuffer.from_array(x.view(np.float32), 0)
    F = n // 2048
    out = P.DeviceBuffer(4 * F * 1024, 0)
    rx.process_device(buf.ptr, n)
    rx.synchronize()
    ms, runs = timed(lambda: rx.map_spectrum_device(out.ptr, 255, 1024, 0.0, -120.0, -fs // 2, fs // 2, 0, F), reps, rx.synchronize)
    report("configs1_every_frame", F, bins, 1024, float(fs), -fs // 2, fs // 2, ms, runs, {"frames": F})
    buf.free()
    out.free()
    rx.close()


if __name__ == "__main__":
    L = P.load_library()
    if L.pebblegpu_device_count() <= 0:
        sys.exit("no HIP device visible: this benchmark times the device and has no CPU path")
    which = sys.argv[1:] or ["bank", "every"]
    if "bank" in which:
        bank(500)
    if "every" in which:
        every(30)
