"""What a multibank call costs the host (pebblegpu_multibank_*, one worker thread per shard), beside a plain ReceiverBank in the same run.
Not the bench line (bench.py measures configs[1]); the figures go into profiles/multibank.json and DESIGN.md section 6.

    bench_multibank.py [DEVICES] [--calls 200] [--channels 512] [--out profiles/multibank.json]

Shape: the BASELINE configs[3] shard -- 512 channels off one 100 Msps stream, int8 pairs, max_superframes = 1 -- as ONE plain
ReceiverBank, as a multibank of one shard, and as a multibank of G shards on DEVICES (comma separated, default "0,0": two shards on one
device, the rig of a one-GPU machine; the 512 channels are split over the shards).  Per subject, over --calls calls:

    host_us          time until process_raw returns, calls queued back to back (median, min, max).  A receiver without a display
                     transform lets the host run three calls ahead and then waits, so back to back this is bounded below by the
                     device's time per call;
    host_paced_us    the same with a synchronise before every call: the cost of queueing alone, nothing to wait for;
    call_ms          wall time of the back-to-back run, final synchronise included, per call;
    last_ms          the library's own figure for the last call (the maximum over the shards).

What a one-GPU machine can show is the host side only: whether a G-shard call returns in about the time one shard's call takes to
queue rather than G times that.  Two shards on ONE device share it: their call_ms is no statement about two devices."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pebblesdr_amd as P  # noqa: E402
from pebblesdr_amd.binding import IQ_S8  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("devices", nargs="?", default="0,0")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--channels", type=int, default=512)
ap.add_argument("--out", default=None)
args = ap.parse_args()
devices = [int(d) for d in args.devices.split(",")]
FS, CH = 100e6, args.channels
fcs = [-45e6 + 175e3 * c + 1e3 * (c % 7) for c in range(CH)]
L = P.load_library()


def stat(v):
    v = np.asarray(v, dtype=np.float64) * 1e6
    return {"median": round(float(np.median(v)), 1), "min": round(float(v.min()), 1), "max": round(float(v.max()), 1)}


def measure(call, sync, last_ms):
    for _ in range(20):
        call()
    sync()
    t = []
    t0 = time.perf_counter()
    for _ in range(args.calls):
        a = time.perf_counter()
        call()
        t.append(time.perf_counter() - a)
    sync()
    wall = time.perf_counter() - t0
    ms = last_ms()
    paced = []
    for _ in range(args.calls):
        sync()
        a = time.perf_counter()
        call()
        paced.append(time.perf_counter() - a)
    sync()
    return {"host_us": stat(t), "host_paced_us": stat(paced), "call_ms": round(wall / args.calls * 1e3, 4), "last_ms": round(ms, 4)}


def tuned(rx):
    for c in range(CH):
        rx.set_mode(c, P.DM_USB)
        rx.set_mixer(c, fcs[c])
        rx.set_bandpass(c, 300, 3000)


def raw_input(n, device):
    rng = np.random.default_rng(1)
    return P.DeviceBuffer.from_array(rng.integers(-100, 100, size=(n, 2), dtype=np.int8), device)


def plain():
    rx = P.ReceiverBank(FS, CH, True, False, 0, max_superframes=1, device=devices[0])
    tuned(rx)
    n = rx.superframe
    buf = raw_input(n, devices[0])
    h, p, g = rx.h, C.c_void_p(buf.ptr), C.c_double(1.0)
    r = measure(lambda: P.binding.check(L, L.pebblegpu_receiver_process_raw(h, IQ_S8, 0, g, p, n)), rx.synchronize, rx.last_ms)
    r["kernels"] = [rx.kernel_name(k) for k in (2, 3, 4)]
    rx.close()
    buf.free()
    return r, n


def multi(devs):
    mb = P.MultiBank(FS, CH, devs, max_superframes=1)
    tuned(mb)
    n = mb.superframe
    bufs = {d: raw_input(n, d) for d in sorted(set(devs))}
    ptrs = (C.c_void_p * len(devs))(*[C.c_void_p(bufs[d].ptr) for d in devs])
    h, g = mb.h, C.c_double(1.0)
    r = measure(lambda: P.binding.check(L, L.pebblegpu_multibank_process_raw(h, IQ_S8, 0, g, ptrs, n)), mb.synchronize, mb.last_ms)
    r["shards"] = [{"device": d, "channels": cnt} for d, (_, cnt) in zip(devs, mb.ranges)]
    mb.close()
    for b in bufs.values():
        b.free()
    return r


bank, n = plain()
out = {
    "workload": "configs[3] shard: %d channels off one 100 Msps stream, int8 pairs, %d samples per call, %d calls" % (CH, n, args.calls),
    "devices": devices,
    "receiver_bank": bank,
    "multibank_1": multi(devices[:1]),
    "multibank_%d" % len(devices): multi(devices),
}
if len(set(devices)) < len(devices):
    out["note"] = "shards that share a device run slower than one bank of the same channels: their kernels share the device"
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
