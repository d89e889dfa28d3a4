"""What getting a receiver's display rows to the host costs a call: the display ring (pebblegpu_receiver_display_*) beside the only
way there was before it.  Not the bench line (bench.py measures configs[1] without a zoomed spectrum); the figures go into
profiles/receiver_display.json, DESIGN.md section 5 and the README.

    bench_receiver_display.py [--calls 200] [--repeats 5] [--superframes 8] [--out profiles/receiver_display.json]

Shape: BASELINE configs[1] -- 20 Msps, one WFM channel, 8192 bins -- with a 2048-bin zoomed spectrum, float2 input resident on the
device, calls of --superframes super-frames.  One process, one device visit.  The clocks settle first as in bench.py (untimed batches
until one is no more than 2 % faster than the one before).  The variants run alternately, --repeats times each; one measurement is a
host clock around --calls calls ending in a synchronise, after ten untimed ones:

    a_calls_alone        the calls alone: the floor (on the parent commit the same figure says what an unopened ring costs)
    b_display_ring       the ring open, 4 slots: bottom pane the unprocessed spectrum's waterfall at 1024 pixels, max_rows 1; top pane the
                         zoomed spectrum as pixels at 1024 x 400, every row of the call; the host takes and releases the block 3 calls back
    c_map_sync_memcpy    the same rows the old way: pebblegpu_receiver_map_spectrum of the last frame + pebblegpu_receiver_map_zoom_spectrum
                         of every zoomed frame, pebblegpu_receiver_synchronize, pebblegpu_memcpy_d2h of both into pageable host memory
    d_display_ring_gated as b under pebblegpu_set_spectrum_updates(10)
    a_gated              the calls alone under the same gate (d's floor)

Reported per variant: ms per call (median over the repeats, their min and max), the host's own time per call inside the process call
and inside next + release, and pebblegpu_receiver_last_ms(rx, 0) of the measurement's last call (for the ring variants that call's
end is recorded by the synchronise behind the drain -- a side-by-side call records no end of its own -- so it includes host time)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pebblesdr_amd as P  # noqa: E402
from pebblesdr_amd.binding import DISPLAY_MAX_PANES, DisplayBlock, check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--superframes", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
FS, BINS, ZB, K, SLOTS, XP = 20_000_000, 8192, 2048, args.superframes, 4, 1024
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
state = {"call_s": 0.0, "take_s": 0.0, "variant": ""}
host_us, own_ms = {}, {}
bottom = P.screen_map(255, XP, 0.0, -120.0, -FS // 2, FS // 2)
top = P.screen_map(400, XP, 0.0, -120.0, 0, 0)
ZOOM = 0.5


def call():
    t0 = time.perf_counter()
    check(L, L.pebblegpu_receiver_process(h, C.c_void_p(buf.ptr), n))
    state["call_s"] += time.perf_counter() - t0


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


def timed(body, drain=None):
    for _ in range(10):
        body()
    if drain:
        drain()
    rx.synchronize()
    state["call_s"] = state["take_s"] = 0.0
    t0 = time.perf_counter()
    for _ in range(args.calls):
        body()
    if drain:
        drain()
    rx.synchronize()
    ms = (time.perf_counter() - t0) / args.calls * 1e3
    host_us.setdefault(state["variant"], []).append((state["call_s"] / args.calls * 1e6, state["take_s"] / args.calls * 1e6))
    own_ms.setdefault(state["variant"], []).append(rx.last_ms(0))
    return ms


call()
rx.synchronize()
ZF = rx.zoom_spectrum().shape[1]
px_host, zpx_host = np.empty((1, XP), dtype=np.int32), np.empty((ZF, XP), dtype=np.int32)
d_px, d_zpx = P.DeviceBuffer(px_host.nbytes, 0), P.DeviceBuffer(zpx_host.nbytes, 0)
F = n // 2048


def variant_c():
    def body():
        call()
        rx.map_spectrum_device(d_px.ptr, 255, XP, 0.0, -120.0, -FS // 2, FS // 2, F - 1, 1)
        rx.map_zoom_spectrum_device(d_zpx.ptr, 400, XP, 0.0, -120.0, ZOOM, None, 0, ZF)
        rx.synchronize()
        check(L, L.pebblegpu_memcpy_d2h(0, px_host.ctypes.data_as(C.c_void_p), C.c_void_p(d_px.ptr), px_host.nbytes))
        check(L, L.pebblegpu_memcpy_d2h(0, zpx_host.ctypes.data_as(C.c_void_p), C.c_void_p(d_zpx.ptr), zpx_host.nbytes))
    return timed(body)


blocks = (DisplayBlock * DISPLAY_MAX_PANES)()
for b in blocks:
    b.struct_size = C.sizeof(DisplayBlock)


def variant_ring(ups):
    rx.set_spectrum_updates(ups)
    rx.display_open([P.display_pane(P.PANE_SPECTRUM, P.DISPLAY_WATERFALL_ARGB32, bottom, max_rows=1),
                     P.display_pane(P.PANE_ZOOM, P.DISPLAY_PIXELS_I32, top, zoom=ZOOM)], SLOTS)
    queued = {"n": 0}

    def take():
        t0 = time.perf_counter()
        check(L, L.pebblegpu_receiver_display_next(h, 1, blocks))
        assert blocks[0].host and not blocks[0].dropped_before
        check(L, L.pebblegpu_receiver_display_release(h, blocks[0].call_index))
        state["take_s"] += time.perf_counter() - t0

    def body():
        call()
        queued["n"] += 1
        if queued["n"] > SLOTS - 1:  # lagging by SLOTS - 1 calls
            take()
            queued["n"] -= 1

    def drain():
        while queued["n"]:
            take()
            queued["n"] -= 1
    ms = timed(body, drain)
    d = rx.display_dropped()
    rx.display_close()
    rx.set_spectrum_updates(P.SPECTRUM_EVERY_FRAME)
    assert d == 0, d
    return ms


def variant_alone(ups):
    rx.set_spectrum_updates(ups)
    ms = timed(call)
    rx.set_spectrum_updates(P.SPECTRUM_EVERY_FRAME)
    return ms


variants = {"a_calls_alone": lambda: variant_alone(P.SPECTRUM_EVERY_FRAME), "b_display_ring": lambda: variant_ring(P.SPECTRUM_EVERY_FRAME),
            "c_map_sync_memcpy": variant_c, "d_display_ring_gated": lambda: variant_ring(10), "a_gated": lambda: variant_alone(10)}
settle()
ms = {v: [] for v in variants}
for _ in range(args.repeats):  # alternating: what drifts during the run drifts for all of them
    for v, fn in variants.items():
        state["variant"] = v
        ms[v].append(fn())
result = {
    "workload": "configs[1] with a zoomed spectrum: 20 Msps, one WFM channel, %d bins, %d zoomed bins, float2 input on the device, calls of %d "
                "super-frames (%d samples); %d calls per measurement, %d repeats, variants alternating, clocks settled first" % (BINS, ZB, K, n, args.calls, args.repeats),
    "slots": SLOTS, "panes": "bottom: unprocessed waterfall, %d pixels, max_rows 1; top: zoomed pixels, %d x 400, zoom %g, %d rows per call" % (XP, XP, ZOOM, ZF),
    "bytes_per_call": (1 + ZF) * XP * 4, "kernels": [rx.kernel_name(w) for w in range(1, 6)], "variants": {},
}
for v in variants:
    med = float(np.median(ms[v]))
    result["variants"][v] = {"ms_per_call": round(med, 4), "min": round(min(ms[v]), 4), "max": round(max(ms[v]), 4),
                             "host_us_in_process": round(float(np.median([a for a, _ in host_us[v]])), 1),
                             "host_us_in_next_release": round(float(np.median([b for _, b in host_us[v]])), 1),
                             "last_ms_call": round(float(np.median(own_ms[v])), 4)}
d_px.free()
d_zpx.free()
buf.free()
rx.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
