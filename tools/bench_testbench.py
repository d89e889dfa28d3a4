#!/usr/bin/env python3
"""What the test bench costs (pebblegpu_set_testbench_sweep / _noise, pebblegpu_receiver_set_taps).

  generator  configs[1] as bench.py runs it (20 Msps, one WFM channel, 8192 bins, 256 super-frames = 33.5 M samples per call, float2
             input resident in HBM, clocks settled by bench.settle): generator off (the default side-by-side route), sweep on, sweep +
             noise on -- one handle each, the legs alternated over --rounds rounds.
  kernel     k_testbench alone on a buffer of the same 33.5 M samples (the stand-alone step: sweep / noise / both) against k_normalize_iq
             over the same samples (float2 -> float2: one read and one write of the stream each), each call timed to its synchronise.
  taps       configs[2] (2.048 Msps shared stream, 256 USB channels, 8 super-frames per call): all four narrow taps on against off.  The
             taps-off leg is the two-stage pipelined route, the taps-on leg runs on one stream (include/pebblegpu.h); --one-stream adds a
             taps-off leg with PEBBLEGPU_BANK_PIPELINE=0 so that the copies' own cost can be told from the route's.

--parent-bench PATH: the bench.py of a checkout of the parent commit (built).  It and this tree's bench.py are run alternately as child
processes BEFORE this process opens the device: the default route must be no slower than the parent beyond the box's own spread.

  python tools/bench_testbench.py [--steps 100 --warmup 10 --rounds 3] [--parent-bench ../parent/bench.py] [--out profiles/testbench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def headline(bench_py, steps, warmup):
    out = subprocess.run([sys.executable, bench_py, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=os.path.dirname(bench_py),
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300, check=True).stdout.decode()
    line = [l for l in out.splitlines() if l.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def spread(v):
    return round((max(v) - min(v)) / (sum(v) / len(v)) * 100.0, 2) if len(v) > 1 else None


def summarise(leg):
    leg["ms_mean"] = round(sum(leg["ms"]) / len(leg["ms"]), 4)
    leg["spread_pct"] = spread(leg["ms"])
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--superframes", type=int, default=256)
    ap.add_argument("--parent-bench", default=None)
    ap.add_argument("--one-stream", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    res = {"steps": args.steps, "rounds": args.rounds}
    if args.parent_bench:
        own, par = [], []
        for _ in range(args.rounds):
            par.append(headline(os.path.abspath(args.parent_bench), args.steps, args.warmup))
            own.append(headline(os.path.join(ROOT, "bench.py"), args.steps, args.warmup))
            print("headline ms per step: parent %.4f, this tree %.4f" % (par[-1], own[-1]), file=sys.stderr, flush=True)
        res["headline_ms_per_step"] = {"parent": par, "this_tree": own, "parent_mean": round(sum(par) / len(par), 4), "this_tree_mean": round(sum(own) / len(own), 4),
                                       "spread_pct": {"parent": spread(par), "this_tree": spread(own)}}

    import bench as B
    import pebblesdr_amd as P
    L = P.load_library()
    if L.pebblegpu_device_count() <= 0:
        raise SystemExit("bench_testbench.py needs an MI355X: libpebblegpu has no CPU path")

    def barrier():
        P.binding.check(L, L.pebblegpu_device_synchronize(0))

    # ---- generator on the headline shape ----
    sw = P.sweep(-1e6, 1e6, 4e9, amplitude=0.1)
    legs, n = {}, None
    for name in ("off", "sweep", "sweep_noise"):
        rx = P.ReceiverBank(B.FS, n_channels=1, shared_input=True, wfm=True, spectrum_bins=B.BINS, max_superframes=args.superframes)
        rx.set_mixer(0, B.MIX_HZ)
        if name != "off":
            rx.set_testbench_sweep(sw)
        if name == "sweep_noise":
            rx.set_testbench_noise(0.01, 1)
        legs[name] = {"rx": rx, "ms": []}
        n = args.superframes * rx.superframe
    dbuf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(B.make_input(n, 1000)), 0)
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
            leg["first_stage_kernel"] = rx.kernel_name(2)
    for leg in legs.values():
        leg.pop("rx").close()
        summarise(leg)
    print("generator legs done", file=sys.stderr, flush=True)
    res["generator"] = {"shape": "configs[1]: 20 Msps, 1 WFM channel, 8192 bins, %d super-frames (%d samples) per call, float2 input" % (args.superframes, n), "legs": legs}

    # ---- the kernel alone against the conversion pass ----
    scratch = P.DeviceBuffer(8 * n, 0)
    kern = {}

    def time_calls(fn, sync):
        fn(); sync()
        B.settle(fn, sync)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        sync()
        return round((time.perf_counter() - t0) / args.steps * 1e3, 4)

    gens = {}
    for name in ("sweep", "noise", "sweep_noise"):
        g = P.SigGen(B.FS)
        if "sweep" in name:
            g.set_sweep(sw)
        if "noise" in name:
            g.set_noise(0.01, 1)
        gens[name] = g
        kern["k_testbench " + name] = {"ms": []}
    kern["k_normalize_iq f32"] = {"ms": []}
    for _ in range(args.rounds):
        for name, g in gens.items():
            kern["k_testbench " + name]["ms"].append(time_calls(lambda: g.generate_device(scratch.ptr, n), g.synchronize))
        kern["k_normalize_iq f32"]["ms"].append(time_calls(
            lambda: P.binding.check(L, L.pebblegpu_normalize_iq(0, P.binding.IQ_F32, 0, 1.0, dbuf.ptr, n, scratch.ptr)), barrier))
    for g in gens.values():
        g.close()
    for k in kern.values():
        summarise(k)
        k["GB_per_s"] = round(16.0 * n / k["ms_mean"] / 1e6, 1)
    base = kern["k_normalize_iq f32"]["ms_mean"]
    for name, k in kern.items():
        k["ratio_to_conversion_pass"] = round(k["ms_mean"] / base, 3)
    print("kernel legs done", file=sys.stderr, flush=True)
    res["kernel_alone"] = {"samples": n, "note": "each call timed to its synchronise; k_normalize_iq through pebblegpu_normalize_iq (blocking)", "kernels": kern}
    scratch.free()
    dbuf.free()

    # ---- taps on configs[2] ----
    fs, C, k = 2_048_000, 256, 8
    freqs = [B.bank_plan(fs, C, g) for g in range(C)]
    tlegs = {}

    def make_bank():
        rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=k)
        for c in range(C):
            rx.set_mode(c, P.DM_USB); rx.set_mixer(c, freqs[c]); rx.set_bandpass(c, 300, 3000)
        return rx
    tlegs["taps_off"] = {"rx": make_bank(), "ms": []}
    tlegs["taps_on"] = {"rx": make_bank(), "ms": []}
    tlegs["taps_on"]["rx"].set_taps([P.TAP_POST_MIXER, P.TAP_POST_BP, P.TAP_MODEM, P.TAP_POST_DEMOD])
    if args.one_stream:
        os.environ["PEBBLEGPU_BANK_PIPELINE"] = "0"
        tlegs["taps_off_one_stream"] = {"rx": make_bank(), "ms": []}
        del os.environ["PEBBLEGPU_BANK_PIPELINE"]
    nb = k * tlegs["taps_on"]["rx"].superframe
    bbuf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(B.make_bank_input(fs, nb, freqs, 7)), 0)
    for _ in range(args.rounds):
        for name, leg in tlegs.items():
            rx = leg["rx"]
            step = lambda: rx.process_device(bbuf.ptr, nb)
            B.settle(step, rx.synchronize)
            for _ in range(args.warmup):
                step()
            rx.synchronize()
            el = B.timed_steps(step, barrier, 4 * args.steps, None)
            leg["ms"].append(round(el / (4 * args.steps) * 1e3, 4))
    for leg in tlegs.values():
        leg.pop("rx").close()
        summarise(leg)
    bbuf.free()
    res["taps"] = {"shape": "configs[2]: 2.048 Msps shared stream, 256 USB channels, %d super-frames per call" % k, "bytes_copied_per_call": 4 * C * (nb // 32) * 8,
                   "legs": tlegs, "added_ms_per_call": round(tlegs["taps_on"]["ms_mean"] - tlegs["taps_off"]["ms_mean"], 4)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
