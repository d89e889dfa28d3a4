#!/usr/bin/env python3
"""What a stream-bank call costs behind the spectrum's update gate (pebblegpu_streambank_set_spectrum_updates).

The configs[4] shard as bench.py shapes it (128 streams x 4 frames of 65536 samples per call, 2048/1025 band-pass + 65536-point
spectrum, the input resident in HBM, clocks settled by bench.settle, what = 3) at 200 Msps, where a frame lasts 0.32768 ms: ten
spectra a second are one frame in 306, about one call in 76.  Three legs, one handle each -- the gate at -1 (every frame: the default
route), at 10 per second, at 0 (no spectrum) -- alternate over --rounds rounds in this process, so that their spread on this box
comes out of the same run.  Each leg is timed over --steps calls queued back to back (host clock, a device synchronise at both
ends); the calls of the 10-per-second leg that SELECT a frame are then timed on their own, from the call's device events (last_ms),
beside as many calls that select nothing.

--parent PATH: a built checkout of the parent commit.  Its tools/bench_streambank.py 4 128 and this tree's are run alternately as
fresh child processes BEFORE this process opens the device, for the one timing condition of the change: the default route is no
slower than the parent's by more than the run-to-run spread seen in that same alternated run.

  python tools/bench_streambank_gate.py [--steps 400 --warmup 10 --rounds 3] [--parent ../parent] [--out profiles/streambank_gate.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, N, F = 128, 65536, 4
FS = 200.0e6


def shard_call(tree):
    """one run of a tree's own tools/bench_streambank.py 4 128 in a fresh process -> its JSON line"""
    out = subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_streambank.py"), str(F), str(S)], cwd=tree, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=300, check=True).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def spread(v):
    return round((max(v) - min(v)) / (sum(v) / len(v)) * 100.0, 2) if len(v) > 1 else None


def stat(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4), "calls": int(v.size)} if v.size else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three rounds: the legs' spread is part of the result")

    res = {"shape": "configs[4] shard: %d streams x %d frames of %d at %g Msps, what = 3" % (S, F, N, FS / 1e6), "steps": args.steps, "rounds": args.rounds}
    if args.parent:
        own, par = [], []
        for _ in range(args.rounds):
            par.append(shard_call(os.path.abspath(args.parent)))
            own.append(shard_call(ROOT))
        cmp_ = {}
        for key in ("ms", "bandpass_ms", "spectrum_ms"):
            p, o = [round(r[key], 4) for r in par], [round(r[key], 4) for r in own]
            cmp_[key] = {"parent": p, "this_tree": o, "parent_mean": round(sum(p) / len(p), 4), "this_tree_mean": round(sum(o) / len(o), 4),
                         "spread_pct": {"parent": spread(p), "this_tree": spread(o)}}
        res["default_route_against_the_parent"] = cmp_

    import bench as B
    import pebblesdr_amd as P
    L = P.load_library()
    if L.pebblegpu_device_count() <= 0:
        raise SystemExit("bench_streambank_gate.py needs an MI355X: libpebblegpu has no CPU path")
    n = F * N
    rng = np.random.default_rng(4)
    x = np.empty((S, n), dtype=np.complex64)
    for s in range(S):
        x[s] = (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)) * np.float32(0.1)
    dbuf = P.DeviceBuffer.from_array(x.view(np.float32), 0)
    del x
    legs = {}
    for name, ups in (("every_frame", -1), ("10_per_s", 10), ("none", 0)):
        sb = P.StreamBank(FS, S, frame=N, spectrum_bins=N, max_frames=F)
        for c in range(S):
            sb.set_bandpass(c, -5.0e6, 5.0e6)
        if ups != -1:
            sb.set_spectrum_updates(ups)
        legs[name] = {"sb": sb, "ms": [], "selecting_calls_per_round": []}

    def barrier():
        P.binding.check(L, L.pebblegpu_device_synchronize(0))

    sel = {0: [], 1: [], 2: []}    # last_ms(which) of the 10-per-second leg's selecting calls
    rest = {0: [], 1: [], 2: []}   # and of as many calls that selected nothing
    sel_name, sel_rows = "", 0
    for _ in range(args.rounds):
        for name, leg in legs.items():
            sb = leg["sb"]
            step = lambda: sb.process_device(dbuf.ptr, n)
            B.settle(step, sb.synchronize)
            for _ in range(args.warmup):
                step()
            sb.synchronize()
            el = B.timed_steps(step, barrier, args.steps, None)
            leg["ms"].append(round(el / args.steps * 1e3, 4))
            if name != "10_per_s":
                leg["spectrum_kernels"] = sb.kernel_name(2)
                continue
            hits = 0
            for _ in range(args.steps):   # the same calls once more, each followed by the (host-only) question whether it selected
                step()
                rows = len(sb.spectrum_frames())
                if rows:
                    hits += 1
                    sel_name, sel_rows = sb.kernel_name(2), rows
                if rows or len(rest[0]) < len(sel[0]):
                    for w in (0, 1, 2):
                        (sel if rows else rest)[w].append(sb.last_ms(w))
            leg["selecting_calls_per_round"].append(hits)
    for name, leg in legs.items():
        leg.pop("sb").close()
        leg["ms_mean"] = round(sum(leg["ms"]) / len(leg["ms"]), 4)
        leg["spread_pct"] = spread(leg["ms"])
        leg["Msamples_per_s"] = round(S * n / leg["ms_mean"] / 1e3, 1)
    dbuf.free()
    legs["10_per_s"]["selecting_call"] = {"rows": sel_rows, "spectrum_kernels": sel_name, "call_ms": stat(sel[0]), "bandpass_ms": stat(sel[1]),
                                          "spectrum_ms": stat(sel[2]), "clock": "device events (last_ms), each call followed by a synchronise"}
    legs["10_per_s"]["call_that_selects_nothing"] = {"call_ms": stat(rest[0]), "bandpass_ms": stat(rest[1]), "spectrum_ms": stat(rest[2])}
    res["gate"] = legs
    res["bytes_in_per_call"] = S * n * 8
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
