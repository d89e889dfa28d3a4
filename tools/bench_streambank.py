"""Time BASELINE configs[4] (S streams @ 2 Msps, 2048/1025 band-pass + 65536-point spectrum) on one GPU.
Not the bench line (bench.py measures configs[1]); the numbers go into profiles/README.md.

    bench_streambank.py [F [S]]                       float2 input, the keys this tool has always printed
    bench_streambank.py [F [S]] --format s8 [--out profiles/streambank_raw.json] [--calls 24]
        the raw-format routes beside it, ALTERNATED inside one run (medians and min..max of --calls timed calls each):
        A  resident input: pebblegpu_normalize_iq + pebblegpu_streambank_process (the only route for integer samples without
           pebblegpu_streambank_process_raw), timed twice, against pebblegpu_streambank_process_raw -- host clock around calls that end
           in a synchronise, since normalize_iq is a call of its own.  normalize_iq synchronises the host itself, so that route pays
           TWO host synchronisations per call against one: what such a host pays, but not all of the difference is the removed pass
           (the float2 call of B on the same host clock, "float2_process_ms", is the route without the pass and with one synchronise);
        B  resident input, per kernel: process on float2 against process_raw (last_ms 1 and 2, device events);
        C  from host memory through the pinned slots: samples/s for the format and for float32 pairs, bytes uploaded / time (medians of 7 runs of 8 batches)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pebblesdr_amd as P  # noqa: E402

FORMATS = {"s8": (0, np.int8, 2), "u8": (1, np.uint8, 2), "s16": (2, np.int16, 4), "f32": (3, np.float32, 8), "wav16": (4, np.int16, 4)}
N = 65536
ap = argparse.ArgumentParser()
ap.add_argument("F", nargs="?", type=int, default=8)
ap.add_argument("S", nargs="?", type=int, default=128)
ap.add_argument("--format", choices=sorted(FORMATS), default=None)
ap.add_argument("--calls", type=int, default=24)
ap.add_argument("--out", default=None)
args = ap.parse_args()
F, S = args.F, args.S
n = F * N
rng = np.random.default_rng(1)
x = (rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))).astype(np.complex64) * 0.1
sb = P.StreamBank(2.0e6, S, frame=N, spectrum_bins=N, max_frames=F)
for c in range(S):
    sb.set_bandpass(c, -50e3, 50e3)
buf = P.DeviceBuffer.from_array(x.view(np.float32))


def stat(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


if args.format is None:
    for _ in range(3):
        sb.process_device(buf.ptr, n)
    sb.synchronize()
    tot, bp, sp = [], [], []
    for _ in range(20):
        sb.process_device(buf.ptr, n)
        tot.append(sb.last_ms(0)); bp.append(sb.last_ms(1)); sp.append(sb.last_ms(2))
    ms = float(np.median(tot))
    print(json.dumps({"workload": "configs[4]: %d streams x %d frames of 65536" % (S, F), "samples": S * n, "ms": ms,
                      "bandpass_ms": float(np.median(bp)), "spectrum_ms": float(np.median(sp)),
                      "gsamples_per_s": S * n / ms / 1e6,
                      "bandpass_GBps": 16.0 * S * n / float(np.median(bp)) / 1e6,
                      "spectrum_GBps": 12.0 * S * n / float(np.median(sp)) / 1e6}))
    sys.exit(0)

fmt, dtype, pair = FORMATS[args.format]
L = sb.L
if dtype == np.float32:
    raw = np.ascontiguousarray(x).view(np.float32).reshape(S, n, 2).copy()
else:
    top = float(np.iinfo(dtype).max)
    off = 128.0 if dtype == np.uint8 else 0.0
    raw = np.clip(np.round(x.view(np.float32).reshape(S, n, 2) * (top if not off else 127.0) * 2.0 + off), np.iinfo(dtype).min, top).astype(dtype)
rbuf = P.DeviceBuffer.from_array(raw)
stage = P.DeviceBuffer(8 * S * n)  # the float2 buffer a host owns on the parent route


def wall(fn):
    t0 = time.perf_counter()
    fn()
    sb.synchronize()
    return (time.perf_counter() - t0) * 1e3


def parent_route():
    P.binding.check(L, L.pebblegpu_normalize_iq(0, fmt, 0, 1.0, rbuf.ptr, S * n, stage.ptr))
    sb.process_device(stage.ptr, n)


def raw_route():
    sb.process_raw_device(rbuf.ptr, n, fmt)


def float_route():
    sb.process_device(buf.ptr, n)


for _ in range(3):  # clocks and code objects
    for fn in (parent_route, raw_route, float_route):
        wall(fn)
tA1, tA2, tRaw, tFloat = [], [], [], []
kRaw, kFloat = ([], []), ([], [])
for _ in range(args.calls):  # the routes alternate inside one run
    tA1.append(wall(parent_route))
    tRaw.append(wall(raw_route)); kRaw[0].append(sb.last_ms(1)); kRaw[1].append(sb.last_ms(2))
    names = (sb.kernel_name(1), sb.kernel_name(2))
    tA2.append(wall(parent_route))
    tFloat.append(wall(float_route)); kFloat[0].append(sb.last_ms(1)); kFloat[1].append(sb.last_ms(2))
mA1, mA2, mRaw = float(np.median(tA1)), float(np.median(tA2)), float(np.median(tRaw))
A = {"normalize_iq_then_process_ms": stat(tA1), "the_same_measured_again_ms": stat(tA2), "process_raw_ms": stat(tRaw),
     "spread_of_the_parent_route_ms": round(abs(mA1 - mA2), 4), "raw_over_parent": round(mRaw / min(mA1, mA2), 4),
     "clock": "host, each call followed by a synchronise; pebblegpu_normalize_iq synchronises too: two per call on that route, one on the others"}
B = {"float2_process_ms": stat(tFloat), "bandpass_ms": {"float2": stat(kFloat[0]), "raw": stat(kRaw[0])},
     "spectrum_ms": {"float2": stat(kFloat[1]), "raw": stat(kRaw[1])}, "kernels_of_the_raw_call": names, "clock": "device events (last_ms)"}


def slots(sfmt, spair, batch):
    """K batches through the two pinned slots, the next upload queued while the previous call computes; the slots are filled once,
    outside the timed loop (a device plugin writes its samples straight into them)"""
    nbytes = S * n * spair
    for s in (0, 1):
        sb.ingest_acquire(s, nbytes, np.uint8)[:] = batch.view(np.uint8).reshape(-1)
    K = 8

    def run():
        sb.ingest_acquire(0, nbytes, np.uint8)
        sb.ingest_submit(0, nbytes)
        for k in range(K):
            s = k & 1
            sb.process_ingested(s, n, sfmt)
            if k + 1 < K:
                sb.ingest_acquire(s ^ 1, nbytes, np.uint8)  # (blocks until that slot's last call is over)
                sb.ingest_submit(s ^ 1, nbytes)
        sb.synchronize()
    run()
    t = []
    for _ in range(7):
        t0 = time.perf_counter()
        run()
        t.append((time.perf_counter() - t0) / K * 1e3)
    med = float(np.median(t))
    return {"ms_per_batch": stat(t), "Msamples_per_s": round(S * n / med / 1e3, 1), "uploaded_GBps": round(nbytes / med / 1e6, 2),
            "bytes_per_batch": nbytes, "runs": len(t), "batches_per_run": K}


C_ = {args.format: slots(fmt, pair, raw)}
if args.format != "f32":
    C_["f32"] = slots(3, 8, np.ascontiguousarray(x).view(np.float32))
C_["probe_copy_gbps_device"] = round(P.binding.probe_copy_gbps(16, 1 << 30, 10), 1)
for k in C_:
    if isinstance(C_[k], dict):
        C_[k]["share_of_device_copy_rate"] = round(C_[k]["uploaded_GBps"] / C_["probe_copy_gbps_device"], 4)
out = {"workload": "configs[4]: %d streams x %d frames of 65536" % (S, F), "samples": S * n, "format": args.format, "timed_calls_per_route": args.calls,
       "A_resident_against_the_staging_route": A, "B_resident_against_float2": B, "C_from_host_memory_through_the_pinned_slots": C_}
print(json.dumps(out))
if args.out:
    prev = {}
    if os.path.exists(args.out):
        prev = json.load(open(args.out))
    prev[args.format] = out
    json.dump(prev, open(args.out, "w"), indent=1)
