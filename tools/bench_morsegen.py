#!/usr/bin/env python3
"""What the Morse stations cost (pebblegpu_set_testbench_morse, k_morsegen).

The configs[2] shape as bench.py runs it -- one 2.048 Msps stream shared by 256 USB channels, 8 super-frames (524288 samples) per call,
float2 input resident in HBM, calls queued back to back, clocks settled by bench.settle -- under:
  off          generators off: the default two-stage pipelined route, the baseline
  sweep_noise  the existing k_testbench: sweep + noise
  morse_N      N stations at 25 wpm, 5 ms rise, one per channel 1 kHz above its mixer, mixed into the input (N = 1, 16, 256)
one handle each, the legs alternated over --rounds rounds.  Then k_morsegen alone on one stream of the same 524288 samples (the stand-alone
step), each call timed to its synchronise.

--parent-root PATH: a built checkout of the parent commit.  The generators-off leg is run there and here alternately, as child processes
(--only-off), BEFORE this process opens the device: the default route must equal the parent's within the box's own spread.

  python tools/bench_morsegen.py [--steps 200 --warmup 20 --rounds 3] [--parent-root ../parent] [--out profiles/morsegen.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, C, K = 2_048_000, 256, 8
MSGS = ["TEST ", "CQ DE K1ABC ", "SOS ", "73 ", "QTH ", "RST 599 "]
ITU = {"A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---", "K": "-.-", "L": ".-..", "M": "--",
       "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-", "U": "..-", "V": "...-", "W": ".--", "X": "-..-", "Y": "-.--", "Z": "--..",
       "0": "-----", "1": ".----", "2": "..---", "3": "...--", "4": "....-", "5": ".....", "6": "-....", "7": "--...", "8": "---..", "9": "----."}


def tokens(text):
    out = []
    for ch in text:
        t = 1
        for d in ITU.get(ch, ""):
            t = (t << 1) | (1 if d == "-" else 0)
        out.append(0 if ch == " " else t)
    return out


def spread(v):
    return round((max(v) - min(v)) / (sum(v) / len(v)) * 100.0, 2) if len(v) > 1 else None


def summarise(leg):
    leg["ms_mean"] = round(sum(leg["ms"]) / len(leg["ms"]), 4)
    leg["spread_pct"] = spread(leg["ms"])
    return leg


def only_off(root, steps, warmup):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--only-off", "--steps", str(steps), "--warmup", str(warmup)],
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300, check=True).stdout.decode()
    return float(json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["ms_per_call"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--root", default=HERE, help="the tree whose library and bench.py are used")
    ap.add_argument("--only-off", action="store_true")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    res = {"steps": args.steps, "rounds": args.rounds}
    if args.parent_root:
        own, par = [], []
        for _ in range(args.rounds):
            par.append(only_off(os.path.abspath(args.parent_root), args.steps, args.warmup))
            own.append(only_off(HERE, args.steps, args.warmup))
            print("generators off, ms per call: parent %.4f, this tree %.4f" % (par[-1], own[-1]), file=sys.stderr, flush=True)
        res["generators_off_ms_per_call"] = {"parent": par, "this_tree": own, "parent_mean": round(sum(par) / len(par), 4), "this_tree_mean": round(sum(own) / len(own), 4),
                                             "spread_pct": {"parent": spread(par), "this_tree": spread(own)}}

    sys.path.insert(0, os.path.abspath(args.root))
    import bench as B
    import pebblesdr_amd as P
    L = P.load_library()
    if L.pebblegpu_device_count() <= 0:
        raise SystemExit("bench_morsegen.py needs an MI355X: libpebblegpu has no CPU path")

    def barrier():
        P.binding.check(L, L.pebblegpu_device_synchronize(0))

    freqs = [B.bank_plan(FS, C, g) for g in range(C)]

    def make_bank():
        rx = P.ReceiverBank(FS, C, True, False, 0, max_superframes=K)
        for c in range(C):
            rx.set_mode(c, P.DM_USB); rx.set_mixer(c, freqs[c]); rx.set_bandpass(c, 300, 3000)
        return rx

    def run_leg(rx, buf, n):
        step = lambda: rx.process_device(buf.ptr, n)
        B.settle(step, rx.synchronize)
        for _ in range(args.warmup):
            step()
        rx.synchronize()
        return round(B.timed_steps(step, barrier, args.steps, None) / args.steps * 1e3, 4)

    if args.only_off:
        rx = make_bank()
        n = K * rx.superframe
        buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(B.make_bank_input(FS, n, freqs, 7)), 0)
        ms = run_leg(rx, buf, n)
        rx.close()
        buf.free()
        print(json.dumps({"ms_per_call": ms}))
        return

    def stations(count):
        return [P.morse_station(freqs[c] + 1000.0, 0.002, 25, 5, tokens(MSGS[c % len(MSGS)])) for c in range(count)]

    legs = {}
    for name in ("off", "sweep_noise", "morse_1", "morse_16", "morse_256"):
        rx = make_bank()
        if name == "sweep_noise":
            rx.set_testbench_sweep(P.sweep(-0.5e6, 0.7e6, 123456789.0, amplitude=0.1))
            rx.set_testbench_noise(0.001, 1)
        if name.startswith("morse_"):
            rx.set_testbench_morse(stations(int(name.split("_")[1])), mix=True)
        legs[name] = {"rx": rx, "ms": []}
    n = K * legs["off"]["rx"].superframe
    buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(B.make_bank_input(FS, n, freqs, 7)), 0)
    for _ in range(args.rounds):
        for name, leg in legs.items():
            leg["ms"].append(run_leg(leg["rx"], buf, n))
            leg["first_stage_kernel"] = leg["rx"].kernel_name(2)
            print("%s: %.4f ms per call" % (name, leg["ms"][-1]), file=sys.stderr, flush=True)
    for leg in legs.values():
        leg.pop("rx").close()
        summarise(leg)
    for name, leg in legs.items():
        leg["added_ms_per_call"] = round(leg["ms_mean"] - legs["off"]["ms_mean"], 4)
    res["bank"] = {"shape": "configs[2]: 2.048 Msps shared stream, %d USB channels, %d super-frames (%d samples) per call, float2 input" % (C, K, n), "legs": legs}
    buf.free()

    # ---- the kernel alone: one stream of the same length, each call timed to its synchronise ----
    scratch = P.DeviceBuffer(8 * n, 0)
    kern = {}
    for name in ("sweep_noise", "morse_1", "morse_16", "morse_256"):
        g = P.SigGen(FS)
        if name == "sweep_noise":
            g.set_sweep(P.sweep(-0.5e6, 0.7e6, 123456789.0, amplitude=0.1))
            g.set_noise(0.001, 1)
        else:
            g.set_morse(stations(int(name.split("_")[1])), mix=True)
        kern[name] = {"gen": g, "ms": []}
    for _ in range(args.rounds):
        for name, k in kern.items():
            g = k["gen"]
            fn = lambda: g.generate_device(scratch.ptr, n)
            fn(); g.synchronize()
            B.settle(fn, g.synchronize)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            g.synchronize()
            k["ms"].append(round((time.perf_counter() - t0) / args.steps * 1e3, 4))
    for name, k in kern.items():
        k.pop("gen").close()
        summarise(k)
        k["stream_GB_per_s"] = round(16.0 * n / k["ms_mean"] / 1e6, 1)
        if name.startswith("morse_"):
            k["station_samples_per_s"] = round(int(name.split("_")[1]) * n / k["ms_mean"] * 1e3, 0)
    scratch.free()
    res["kernel_alone"] = {"samples": n, "note": "the stand-alone step in place on one stream (one read, one write); launch and table upload included", "kernels": kern}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
