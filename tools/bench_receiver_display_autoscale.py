"""What the display ring's auto-scale costs a call.  The tool and shape behind profiles/receiver_display.json (tools/bench_receiver_display.py,
variant b): BASELINE configs[1] -- 20 Msps, one WFM channel, 8192 bins -- with a 2048-bin zoomed spectrum, float2 input resident on the
device, calls of --superframes super-frames, the ring open with 4 slots (bottom pane: the unprocessed spectrum's waterfall at 1024
pixels, max_rows 1; top pane: the zoomed spectrum as pixels at 1024 x 400), the host taking and releasing the block 3 calls back.

    bench_receiver_display_autoscale.py [--calls 200] [--repeats 5] [--superframes 8] [--root DIR] [--out FILE]

Variants, run alternately, --repeats times each (one measurement: a host clock around --calls calls ending in a synchronise, after ten
untimed ones; the clocks settle first as in bench.py):

    ring_fixed          the ring as before this interface: flags never set
    ring_auto           pebblegpu_receiver_display_set_auto_scale(MAX | MIN), the recalc done in the untimed calls: none pending
    ring_auto_rescale   the same with pebblegpu_receiver_display_rescale() before EVERY call: one k_scale_stats launch per call

--root imports pebblesdr_amd (and its library) from another checkout: a tree from before the interface runs ring_fixed alone, which is
how the comparison against the parent commit is made -- both processes in one visit to the device, alternating."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--superframes", type=int, default=8)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import pebblesdr_amd as P  # noqa: E402
from pebblesdr_amd.binding import DISPLAY_MAX_PANES, DisplayBlock, check  # noqa: E402

FS, BINS, ZB, K, SLOTS, XP, ZOOM = 20_000_000, 8192, 2048, args.superframes, 4, 1024, 0.5
HAS_AUTO = hasattr(P, "AUTO_SCALE_MAX")
L = P.load_library()
rx = P.ReceiverBank(FS, 1, True, True, BINS, max_superframes=K, hires_bins=ZB)
rx.set_mixer(0, 1.0e6)
n = K * rx.superframe
t = np.arange(n) / FS
rng = np.random.default_rng(1)
x = (0.4 * np.exp(1j * (2 * np.pi * 1.0e6 * t + 75.0 * np.sin(2 * np.pi * 1000 * t))) + 1e-2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x), 0)
del t, x
h = rx.h
bottom = P.screen_map(255, XP, 0.0, -120.0, -FS // 2, FS // 2)
top = P.screen_map(400, XP, 0.0, -120.0, 0, 0)
blocks = (DisplayBlock * DISPLAY_MAX_PANES)()
for b in blocks:
    b.struct_size = C.sizeof(DisplayBlock)


def call():
    check(L, L.pebblegpu_receiver_process(h, C.c_void_p(buf.ptr), n))


def settle(max_s=0.5, batch=20):
    """bench.py's settle(): untimed batches until one is no more than 2 % faster than the one before"""
    rx.synchronize()
    prev, t_start = None, time.perf_counter()
    while time.perf_counter() - t_start < max_s:
        t0 = time.perf_counter()
        for _ in range(batch):
            call()
        rx.synchronize()
        dt = (time.perf_counter() - t0) / batch
        if prev is not None and dt > prev * 0.98:
            break
        prev = dt
        if dt * batch < 0.005:
            batch, prev = int(0.005 / dt) + 1, None


def variant(flags, rescale):
    rx.display_open([P.display_pane(P.PANE_SPECTRUM, P.DISPLAY_WATERFALL_ARGB32, bottom, max_rows=1),
                     P.display_pane(P.PANE_ZOOM, P.DISPLAY_PIXELS_I32, top, zoom=ZOOM)], SLOTS)
    if flags:
        rx.display_set_auto_scale(flags)
    queued = 0

    def take():
        check(L, L.pebblegpu_receiver_display_next(h, 1, blocks))
        assert blocks[0].host and not blocks[0].dropped_before
        check(L, L.pebblegpu_receiver_display_release(h, blocks[0].call_index))

    def run(calls):
        nonlocal queued
        for _ in range(calls):
            if rescale:
                rx.display_rescale()
            call()
            queued += 1
            if queued > SLOTS - 1:  # lagging by SLOTS - 1 calls
                take()
                queued -= 1
        while queued:
            take()
            queued -= 1
        rx.synchronize()

    run(10)
    t0 = time.perf_counter()
    run(args.calls)
    ms = (time.perf_counter() - t0) / args.calls * 1e3
    assert rx.display_dropped() == 0
    rx.display_close()
    return ms


variants = {"ring_fixed": lambda: variant(0, False)}
if HAS_AUTO:
    variants["ring_auto"] = lambda: variant(3, False)
    variants["ring_auto_rescale"] = lambda: variant(3, True)
call()
settle()
ms = {v: [] for v in variants}
for _ in range(args.repeats):  # alternating: what drifts during the run drifts for all of them
    for v, fn in variants.items():
        ms[v].append(fn())
result = {
    "workload": "configs[1] with a zoomed spectrum: 20 Msps, one WFM channel, %d bins, %d zoomed bins, float2 input on the device, calls of %d "
                "super-frames (%d samples); display ring open, %d slots; %d calls per measurement, %d repeats, variants alternating, clocks settled "
                "first" % (BINS, ZB, K, n, SLOTS, args.calls, args.repeats),
    "auto_scale_interface": HAS_AUTO, "kernels": [rx.kernel_name(w) for w in range(1, 6)],
    "variants": {v: {"ms_per_call": round(float(np.median(ms[v])), 4), "min": round(min(ms[v]), 4), "max": round(max(ms[v]), 4)} for v in variants},
}
buf.free()
rx.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
