"""A/B of the two routes of a receiver without a decimator (an empty chain): a bank of 256 SSB channels on one shared 48 kHz stream,
calls of 8 and of 32 super-frames.
  mixing band-pass : k_fastfir_t128_mix rotates the stream's samples in its own loads (the default)
  k_mixer          : the stand-alone mixer writes the mixed rows, k_fastfir_t128 reads them (PEBBLEGPU_NO_FUSED_DEC=1)
The switch is read when a receiver is created, and one process's figure depends on where its buffers landed: each variant is
measured in fresh processes, started in alternating pairs (A B A B ...) of one device visit.  A difference counts only when it is
larger than the spread between processes of the same variant.
  python tools/bench_no_decimator.py [--pairs 4] [--out profiles/no_decimator.json]
  (--child <variant>: one measuring process; prints one JSON line)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"mixing band-pass": {}, "k_mixer": {"PEBBLEGPU_NO_FUSED_DEC": "1"}}
FS, C, KS = 48000, 256, (8, 32)
WARM, TIMED, ROUNDS = 50, 200, 5


def child(variant):
    sys.path.insert(0, ROOT)
    import numpy as np
    import pebblesdr_amd as P
    out = {"variant": variant}
    for k in KS:
        rx = P.ReceiverBank(FS, C, True, False, 0, max_superframes=k)
        for c in range(C):
            rx.set_mode(c, P.DM_USB)
            rx.set_mixer(c, -22000.0 + 170.0 * c)
            rx.set_bandpass(c, 300, 3000)
        n = k * rx.superframe
        rng = np.random.default_rng(1)
        x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.05).astype(np.complex64)
        buf = P.DeviceBuffer.from_array(x.view(np.float32))
        for _ in range(WARM):
            rx.process_device(buf.ptr, n)
        rx.synchronize()
        ev, host = [], []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(TIMED):
                rx.process_device(buf.ptr, n)
            rx.synchronize()
            host.append((time.perf_counter() - t0) * 1e3 / TIMED)
            ev.append(rx.mean_ms(0, 30))
        out["k%d" % k] = {"kernel": rx.kernel_name(2), "band_pass": rx.kernel_name(4), "call_ms_events": round(float(np.median(ev)), 5),
                          "call_ms_host": round(float(np.median(host)), 5), "channel_Msamples_per_s": round(C * n / float(np.median(host)) / 1e3, 1)}
        rx.close()
        buf.free()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    runs = {v: [] for v in VARIANTS}
    for _ in range(a.pairs):
        for v, env in VARIANTS.items():
            e = dict(os.environ)
            e.pop("PEBBLEGPU_NO_FUSED_DEC", None)
            e.update(env)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v], env=e, capture_output=True, text=True, timeout=180)
            if p.returncode != 0:  # nothing more is started on the device behind a process that failed
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("measuring process for %r ended with status %d" % (v, p.returncode))
            runs[v].append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"workload": "%d USB channels on one shared %d Hz stream, frames of 2048, band-pass 2048/1025" % (C, FS), "pairs": a.pairs,
           "calls_timed_per_process": TIMED * ROUNDS, "processes": runs, "summary": {}}
    for k in KS:
        s = {}
        for v in VARIANTS:
            t = sorted(r["k%d" % k]["call_ms_host"] for r in runs[v])
            s[v] = {"kernel": runs[v][0]["k%d" % k]["kernel"], "call_ms_host_median": t[len(t) // 2] if len(t) % 2 else round((t[len(t) // 2 - 1] + t[len(t) // 2]) / 2, 5),
                    "call_ms_host_min": t[0], "call_ms_host_max": t[-1], "spread_ms": round(t[-1] - t[0], 5),
                    "call_ms_events": sorted(r["k%d" % k]["call_ms_events"] for r in runs[v])}
        a_, b_ = s["mixing band-pass"], s["k_mixer"]
        s["k_mixer_minus_mixing_ms"] = round(b_["call_ms_host_median"] - a_["call_ms_host_median"], 5)
        s["larger_spread_ms"] = max(a_["spread_ms"], b_["spread_ms"])
        s["mixing_faster_beyond_spread"] = a_["call_ms_host_max"] < b_["call_ms_host_min"]
        res["summary"]["%d super-frames per call" % k] = s
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
