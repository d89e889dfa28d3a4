"""What getting a stream bank's results to the host costs a call: the two egress rings (pebblegpu_streambank_iq_out_*,
pebblegpu_streambank_display_*) beside the only way there was before them.  Not the bench line (bench.py measures configs[1]); the
figures go into profiles/streambank_egress.json, DESIGN.md section 5 and the README.

    bench_streambank_egress.py [--calls 100] [--repeats 5] [--streams 128] [--frames 4] [--only PREFIX,...] [--out profiles/streambank_egress.json]

Shape: a BASELINE configs[4] shard -- 128 streams x 4 frames of 65536 samples per call, 65536 bins, int8 pairs fed through the pinned
ingest slots.  One process, one device visit.  The variants run alternately, --repeats times each; one measurement is a host clock
around --calls calls ending in a synchronise, after a warm-up:

    D            the calls alone: the floor
    A_iq         process_ingested, pebblegpu_streambank_synchronize, pebblegpu_memcpy_d2h of the 8 selected rows of
                 pebblegpu_streambank_filtered into (pageable) host memory: what a host that wants those rows had to do without the ring
    A_pixels     process_ingested, pebblegpu_streambank_map_spectrum of the last frame of all streams at 1024 pixels, synchronize,
                 memcpy_d2h of the pixels
    B_f32, B_s16 the IQ ring, 8 streams selected, 4 slots; the host takes and releases the block of the call 3 calls back
    C_pixels, C_waterfall   the display ring over all streams, max_rows = 1, 1024 pixels
    C_waterfall_auto        the same with pebblegpu_streambank_display_set_auto_scale(MAX | MIN), the recalc done in the warm-up: every
                            stream's row mapped with its own range from the table
    C_waterfall_auto_rescale  ... and pebblegpu_streambank_display_rescale() before EVERY call: k_scale_stats over 128 rows of 65536 bins
                            in each call
--only runs the variants whose names start with one of the prefixes (the auto-scale figures: --only D,C_display_ring_waterfall).

Reported per variant: ms per call (median over the repeats, and their min / max), bytes per call, for the rings bytes per call over ms
per call in GB/s, the host's own time per call inside the process calls and inside next + release, and pebblegpu_streambank_last_ms
(sb, 1) / (sb, 2) of the measurement's last call: the call's own kernels, which an open ring leaves alone.  The reader touches no
sample (a host hands the pinned pointer on); A's copies land in pageable memory because the C ABI offers a host nothing else.  An F32
block of ALL streams would be streams x frames x 512 KiB per call (268 MB at the default shape) and can only be bound by the link: it
is not timed here."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pebblesdr_amd as P  # noqa: E402
from pebblesdr_amd.binding import IQ_S8, AudioBlock, DisplayBlock, check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--only", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()
FS, S, F, N65, SLOTS, XP = 200e6, args.streams, args.frames, 65536, 4, 1024
SEL = [(S // 8) * i + 1 for i in range(8)] if S >= 16 else list(range(min(S, 8)))
L = P.load_library()

sb = P.StreamBank(FS, S, frame=N65, spectrum_bins=N65, max_frames=F)
for c in range(S):
    sb.set_bandpass(c, -20e6, 20e6)
n = F * N65
raw_bytes = 2 * n * S
rng = np.random.default_rng(1)
for slot in (0, 1):
    sb.ingest_acquire(slot, raw_bytes)[:] = rng.integers(-100, 100, size=raw_bytes, dtype=np.int8)
h, gain, p = sb.h, C.c_double(1.0), C.c_void_p()
state = {"i": 0, "call_s": 0.0, "take_s": 0.0, "variant": ""}
host_us, own_ms = {}, {}
screen = P.screen_map(255, XP, 0.0, -120.0, int(-FS // 2), int(FS // 2))


def call():  # the steady state of section 4 of INTEGRATION.md (the slot's samples are left as they are: no host fill is timed)
    t = time.perf_counter()
    slot = state["i"] & 1
    state["i"] += 1
    check(L, L.pebblegpu_streambank_ingest_acquire(h, slot, raw_bytes, C.byref(p)))
    check(L, L.pebblegpu_streambank_ingest_submit(h, slot, raw_bytes))
    check(L, L.pebblegpu_streambank_process_ingested(h, slot, IQ_S8, 0, gain, n, 3))
    state["call_s"] += time.perf_counter() - t


def timed(body, drain=None):
    for _ in range(10):
        body()
    if drain:
        drain()
    sb.synchronize()
    state["call_s"] = state["take_s"] = 0.0
    t0 = time.perf_counter()
    for _ in range(args.calls):
        body()
    if drain:
        drain()
    sb.synchronize()
    ms = (time.perf_counter() - t0) / args.calls * 1e3
    host_us.setdefault(state["variant"], []).append((state["call_s"] / args.calls * 1e6, state["take_s"] / args.calls * 1e6))
    own_ms.setdefault(state["variant"], []).append((sb.last_ms(1), sb.last_ms(2)))
    return ms


call()
sb.synchronize()
d_filt = L.pebblegpu_streambank_filtered(h, None, None)
rows_host = np.empty((len(SEL), n), dtype=np.complex64)
px_host = np.empty((S, XP), dtype=np.int32)
d_px = P.DeviceBuffer(px_host.nbytes, 0)


def variant_a_iq():
    def body():
        call()
        sb.synchronize()
        for r, s in enumerate(SEL):  # the selected rows lie apart on the device: one copy each
            check(L, L.pebblegpu_memcpy_d2h(0, rows_host[r].ctypes.data_as(C.c_void_p), C.c_void_p(d_filt + 8 * n * s), 8 * n))
    return timed(body)


def variant_a_pixels():
    def body():
        call()
        check(L, L.pebblegpu_streambank_map_spectrum(h, C.byref(screen), F - 1, 1, 1, C.c_void_p(d_px.ptr)))
        sb.synchronize()
        check(L, L.pebblegpu_memcpy_d2h(0, px_host.ctypes.data_as(C.c_void_p), C.c_void_p(d_px.ptr), px_host.nbytes))
    return timed(body)


def variant_ring(open_, close, nxt, release, dropped, blk, pre=None):
    open_()
    queued = {"n": 0}

    def take():
        t = time.perf_counter()
        check(L, nxt(h, 1, C.byref(blk)))
        assert blk.host and not blk.dropped_before
        check(L, release(h, blk.call_index))
        state["take_s"] += time.perf_counter() - t

    def body():
        if pre:
            pre()
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
    d = dropped()
    close()
    assert d == 0, d
    return ms


ablk, dblk = AudioBlock(), DisplayBlock()
ablk.struct_size, dblk.struct_size = C.sizeof(AudioBlock), C.sizeof(DisplayBlock)


def iq_ring(fmt):
    return variant_ring(lambda: sb.iq_out_open(fmt, SEL, SLOTS), sb.iq_out_close, L.pebblegpu_streambank_iq_out_next,
                        L.pebblegpu_streambank_iq_out_release, sb.iq_out_dropped, ablk)


def display_ring(fmt, flags=0, rescale=False):
    def open_():
        sb.display_open(fmt, screen, None, 1, SLOTS)
        if flags:
            sb.display_set_auto_scale(flags)
    return variant_ring(open_, sb.display_close, L.pebblegpu_streambank_display_next, L.pebblegpu_streambank_display_release, sb.display_dropped, dblk,
                        sb.display_rescale if rescale else None)


variants = {"D_calls_alone": lambda: timed(call), "A_iq_sync_memcpy_d2h": variant_a_iq, "A_pixels_map_sync_memcpy_d2h": variant_a_pixels,
            "B_iq_ring_f32": lambda: iq_ring(P.AUDIO_F32), "B_iq_ring_s16": lambda: iq_ring(P.AUDIO_S16),
            "C_display_ring_pixels": lambda: display_ring(P.DISPLAY_PIXELS_I32), "C_display_ring_waterfall": lambda: display_ring(P.DISPLAY_WATERFALL_ARGB32),
            "C_display_ring_waterfall_auto": lambda: display_ring(P.DISPLAY_WATERFALL_ARGB32, 3),
            "C_display_ring_waterfall_auto_rescale": lambda: display_ring(P.DISPLAY_WATERFALL_ARGB32, 3, True)}
if args.only:
    variants = {v: fn for v, fn in variants.items() if v.startswith(tuple(args.only.split(",")))}
ms = {v: [] for v in variants}
for _ in range(args.repeats):  # alternating: what drifts during the run drifts for all of them
    for v, fn in variants.items():
        state["variant"] = v
        ms[v].append(fn())
nbytes = {"D_calls_alone": 0, "A_iq_sync_memcpy_d2h": rows_host.nbytes, "A_pixels_map_sync_memcpy_d2h": px_host.nbytes,
          "B_iq_ring_f32": len(SEL) * n * 8, "B_iq_ring_s16": len(SEL) * n * 4, "C_display_ring_pixels": S * XP * 4, "C_display_ring_waterfall": S * XP * 4,
          "C_display_ring_waterfall_auto": S * XP * 4 + S * 24, "C_display_ring_waterfall_auto_rescale": S * XP * 4 + S * 24}
result = {
    "workload": "configs[4] shard: %d streams x %d frames of 65536 (65536 bins), int8 pairs through the ingest slots; %d calls per measurement, %d repeats, "
                "variants alternating" % (S, F, args.calls, args.repeats),
    "slots": SLOTS, "iq_selection": SEL, "display_selection": "all %d streams, max_rows 1, %d pixels" % (S, XP),
    "kernels": [sb.kernel_name(1), sb.kernel_name(2)], "raw_bytes_per_call": raw_bytes, "variants": {},
    "not_timed": "an F32 block of all %d streams is %d bytes per call and can only be bound by the link" % (S, S * n * 8),
}
for v in variants:
    med = float(np.median(ms[v]))
    r = {"ms_per_call": round(med, 4), "min": round(min(ms[v]), 4), "max": round(max(ms[v]), 4), "bytes_per_call": nbytes[v]}
    if v[0] in "BC":
        r["d2h_GBps"] = round(nbytes[v] / (med * 1e-3) / 1e9, 3)
    r["host_us_in_process"] = round(float(np.median([a for a, _ in host_us[v]])), 1)
    r["host_us_in_next_release"] = round(float(np.median([b for _, b in host_us[v]])), 1)
    r["last_ms_bandpass"] = round(float(np.median([a for a, _ in own_ms[v]])), 4)
    r["last_ms_spectrum"] = round(float(np.median([b for _, b in own_ms[v]])), 4)
    result["variants"][v] = r
d_px.free()
sb.close()
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
