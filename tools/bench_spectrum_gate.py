#!/usr/bin/env python3
"""What a call costs behind the spectrum's update gate (pebblegpu_set_spectrum_updates), on the headline shape.

configs[1] as bench.py runs it (20 Msps, one WFM channel, 8192 bins, 256 super-frames = 33.5 M samples per call, the input resident
in HBM, clocks settled by bench.settle), timed three ways in this process, one handle each: the gate at -1 (every frame: the default
route), at 10 per second (16 of a call's 16384 frames), at 0 (no spectrum).  The three legs alternate over --rounds rounds, so that
their spread on this box comes out of the same run.

--parent-bench PATH: the bench.py of a checkout of the parent commit (built).  It and this tree's bench.py are run alternately as
child processes BEFORE this process opens the device, for the one timing condition of the change: the default route is no slower
than the parent by more than the box's run-to-run spread.

  python tools/bench_spectrum_gate.py [--steps 200 --warmup 10 --rounds 3] [--parent-bench ../parent/bench.py] [--out profiles/x.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def headline(bench_py, steps, warmup):
    """one run of a tree's own bench.py in a fresh process -> ms per step"""
    out = subprocess.run([sys.executable, bench_py, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=os.path.dirname(bench_py),
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300, check=True).stdout.decode()
    line = [l for l in out.splitlines() if l.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def spread(v):
    return round((max(v) - min(v)) / (sum(v) / len(v)) * 100.0, 2) if len(v) > 1 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--superframes", type=int, default=256)
    ap.add_argument("--parent-bench", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    res = {"shape": "configs[1]: 20 Msps, 1 WFM channel, 8192 bins, %d super-frames per call" % args.superframes, "steps": args.steps, "rounds": args.rounds}
    if args.parent_bench:
        own, par = [], []
        for _ in range(args.rounds):
            par.append(headline(os.path.abspath(args.parent_bench), args.steps, args.warmup))
            own.append(headline(os.path.join(ROOT, "bench.py"), args.steps, args.warmup))
        res["headline_ms_per_step"] = {"parent": par, "this_tree": own, "parent_mean": round(sum(par) / len(par), 4), "this_tree_mean": round(sum(own) / len(own), 4),
                                       "spread_pct": {"parent": spread(par), "this_tree": spread(own)}}

    import bench as B
    import pebblesdr_amd as P
    L = P.load_library()
    if L.pebblegpu_device_count() <= 0:
        raise SystemExit("bench_spectrum_gate.py needs an MI355X: libpebblegpu has no CPU path")
    legs = {}
    n = None
    for name, ups in (("every_frame", -1), ("10_per_s", 10), ("none", 0)):
        rx = P.ReceiverBank(B.FS, n_channels=1, shared_input=True, wfm=True, spectrum_bins=B.BINS, max_superframes=args.superframes)
        rx.set_mixer(0, B.MIX_HZ)
        if ups != -1:
            rx.set_spectrum_updates(ups)
        legs[name] = {"rx": rx, "ms": [], "rows_per_call": None}
        n = args.superframes * rx.superframe
    dbuf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(B.make_input(n, 1000)), 0)

    def barrier():
        P.binding.check(L, L.pebblegpu_device_synchronize(0))

    for _ in range(args.rounds):
        for name, leg in legs.items():
            rx = leg["rx"]
            step = lambda: rx.process_device(dbuf.ptr, n)
            B.settle(step, rx.synchronize)
            for _ in range(args.warmup):
                step()
            rx.synchronize()
            el = B.timed_steps(step, barrier, args.steps, None)
            leg["ms"].append(round(el / args.steps * 1e3, 4))
            leg["rows_per_call"] = len(rx.spectrum_frames()) if name != "every_frame" else n // B.NF
            leg["spectrum_kernel"] = rx.kernel_name(1)
            leg["first_stage_kernel"] = rx.kernel_name(2)
    for name, leg in legs.items():
        leg.pop("rx").close()
        leg["ms_mean"] = round(sum(leg["ms"]) / len(leg["ms"]), 4)
        leg["spread_pct"] = spread(leg["ms"])
        leg["Msamples_per_s"] = round(n / leg["ms_mean"] / 1e3, 1)
    dbuf.free()
    res["gate"] = legs
    res["bytes_in_per_call"] = n * 8
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
