#!/usr/bin/env python3
"""What a modem ring AT A MODEM RATE costs a call (pebblegpu_receiver_modem_out_open_rate, k_modem_rate_pack) beside the plain ring, whose
float rows are bound by the host link.  Not the bench line (bench.py measures configs[1]); the figures go into profiles/modem_rate.json,
DESIGN.md section 5 and the README.  tools/bench_modem_out.py's rules, word for word:

    bench_modem_rate.py [--parent-lib PATH/libpebblegpu.so] [--pairs 4] [--calls 200] [--out profiles/modem_rate.json]

Shape: BASELINE configs[2] -- 256 SSB channels off one 2.048 Msps stream -- on device-resident float2 input, in calls of eight
super-frames and of one.  --pairs alternating pairs of FRESH processes in one device visit: the parent commit's library (--parent-lib,
a build of the parent commit) and this tree's.  This process never opens the device.  Cases, each on a fresh bank, per call length:

    calls           the calls alone, ring never opened -- parent and this library: the one pass / fail figure (this library's range against
                    the parent's process-to-process spread)
    ring_f32        the existing plain ring on all 256 channels, float rows at 64 kHz; the host takes and releases the block of the call
                    three calls back
    rate_f32        the ring at (1000 Hz, 8000 Hz) on all 256 channels: float rows at 8 kHz, an eighth of the bytes
    rate_s16        the same, PCM16 pairs
    gated           a squelched bank (4096-bin display transform, a threshold on every channel: every second one never opens, the others
                    never close), the gated route alone
    gated_rate_f32  the same bank with the ring at (1000 Hz, 8000 Hz) open on all channels
The parent's process runs `calls` only.  One measurement is a host clock around --calls calls ending in a synchronise, after a settled
warm-up (bench.settle); reported per case and library: the median over the pairs and their range, ms per call."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, CH, SLOTS = 2.048e6, 256, 4
CASES = ["calls", "ring_f32", "rate_f32", "rate_s16", "gated", "gated_rate_f32"]
MAX_BW, MIN_RATE = 1000, 8000
LENGTHS = (8, 1)


def child(lib_path, cases, calls):
    """one process, one library: every case and call length on a fresh bank -> {"case/k": ms per call}"""
    from pebblesdr_amd.binding import Config, Info, ModemBlock, DM_USB
    L = C.CDLL(lib_path)
    vp, u32, u64, i32, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
    L.pebblegpu_last_error.restype = C.c_char_p
    L.pebblegpu_malloc.argtypes = [i32, C.c_size_t, C.POINTER(vp)]
    L.pebblegpu_free.argtypes = [i32, vp]
    L.pebblegpu_memcpy_h2d.argtypes = [i32, vp, vp, C.c_size_t]
    L.pebblegpu_memcpy_d2h.argtypes = [i32, vp, vp, C.c_size_t]
    L.pebblegpu_receiver_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.pebblegpu_receiver_destroy.argtypes = [vp]
    L.pebblegpu_receiver_info.argtypes = [vp, C.POINTER(Info)]
    L.pebblegpu_set_mixer_freq.argtypes = [vp, u32, dbl]
    L.pebblegpu_set_bandpass.argtypes = [vp, u32, dbl, dbl]
    L.pebblegpu_set_demod_mode.argtypes = [vp, u32, i32]
    L.pebblegpu_set_squelch.argtypes = [vp, u32, dbl]
    L.pebblegpu_receiver_process.argtypes = [vp, vp, u64]
    L.pebblegpu_receiver_synchronize.argtypes = [vp]

    def check(rc):
        if rc:
            raise SystemExit("%s: %s" % (lib_path, (L.pebblegpu_last_error() or b"").decode()))

    if L.pebblegpu_device_count() <= 0:
        raise SystemExit("bench_modem_rate.py needs an MI355X: libpebblegpu has no CPU path")
    import bench as B
    out = {}
    rng = np.random.default_rng(1)
    for k in LENGTHS:
        for case in cases:
            gated = case.startswith("gated")
            cfg = Config()
            cfg.struct_size, cfg.device, cfg.sample_rate, cfg.frames_per_buffer = C.sizeof(Config), 0, FS, 2048
            cfg.n_channels, cfg.shared_input, cfg.spectrum_bins, cfg.max_superframes = CH, 1, 4096 if gated else 0, k
            h = vp()
            check(L.pebblegpu_receiver_create(C.byref(cfg), C.byref(h)))
            info = Info()
            check(L.pebblegpu_receiver_info(h, C.byref(info)))
            for c in range(CH):
                check(L.pebblegpu_set_demod_mode(h, c, DM_USB))
                check(L.pebblegpu_set_mixer_freq(h, c, -900e3 + 1800e3 * (c + 0.5) / CH))
                check(L.pebblegpu_set_bandpass(h, c, 300, 3000))
                if gated:
                    check(L.pebblegpu_set_squelch(h, c, 50.0 if c & 1 else -119.0))
            n = k * int(info.superframe)
            x = (rng.standard_normal(2 * n) * 0.05).astype(np.float32)
            d_in = vp()
            check(L.pebblegpu_malloc(0, x.nbytes, C.byref(d_in)))
            check(L.pebblegpu_memcpy_h2d(0, d_in, x.ctypes.data_as(vp), x.nbytes))
            ring = "ring" in case or "rate" in case
            if ring:
                L.pebblegpu_receiver_modem_out_open.argtypes = [vp, i32, C.POINTER(u32), u32, u32]
                L.pebblegpu_receiver_modem_out_open_rate.argtypes = [vp, i32, C.POINTER(u32), u32, u32, u32, u32]
                L.pebblegpu_receiver_modem_out_close.argtypes = [vp]
                L.pebblegpu_receiver_modem_out_next.argtypes = [vp, i32, C.POINTER(ModemBlock)]
                L.pebblegpu_receiver_modem_out_release.argtypes = [vp, u64]
                fmt = 1 if case.endswith("s16") else 0
                if "rate" in case:
                    check(L.pebblegpu_receiver_modem_out_open_rate(h, fmt, None, 0, SLOTS, MAX_BW, MIN_RATE))
                else:
                    check(L.pebblegpu_receiver_modem_out_open(h, fmt, None, 0, SLOTS))
            blk = ModemBlock()
            blk.struct_size = C.sizeof(ModemBlock)
            st = {"queued": 0}

            def take():
                check(L.pebblegpu_receiver_modem_out_next(h, 1, C.byref(blk)))
                assert blk.host and not blk.dropped_before
                check(L.pebblegpu_receiver_modem_out_release(h, blk.call_index))
                st["queued"] -= 1

            def step():
                check(L.pebblegpu_receiver_process(h, d_in, n))
                if ring:
                    st["queued"] += 1
                    if st["queued"] > SLOTS - 1:   # the reader lags by SLOTS - 1 calls
                        take()

            def sync():
                while st["queued"]:
                    take()
                check(L.pebblegpu_receiver_synchronize(h))

            B.settle(step, sync)
            for _ in range(10):
                step()
            sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                step()
            sync()
            out["%s/%d" % (case, k)] = round((time.perf_counter() - t0) / calls * 1e3, 4)
            if ring:
                check(L.pebblegpu_receiver_modem_out_close(h))
            check(L.pebblegpu_receiver_destroy(h))
            check(L.pebblegpu_free(0, d_in))
    print(json.dumps(out))


def run_child(lib_path, cases, calls):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, "--cases", ",".join(cases), "--calls", str(calls)],
                         cwd=ROOT, stdout=subprocess.PIPE, timeout=600, check=True).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def stat(v):
    v = sorted(v)
    return {"median": round(float(np.median(v)), 4), "min": v[0], "max": v[-1], "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.cases.split(","), args.calls)
    own_lib = os.path.join(ROOT, "pebblesdr_amd", "libpebblegpu.so")
    par, own = [], []
    for _ in range(args.pairs):
        if args.parent_lib:
            par.append(run_child(os.path.abspath(args.parent_lib), ["calls"], args.calls))
        own.append(run_child(own_lib, CASES, args.calls))
    res = {"shape": "configs[2]: %d SSB channels off one %g Msps stream, device-resident float2 input, calls of %s super-frames; gated: 4096-bin "
                    "display transform, every second channel never opens" % (CH, FS / 1e6, " and ".join(str(k) for k in LENGTHS)),
           "calls": args.calls, "pairs": args.pairs, "slots": SLOTS, "max_bw": MAX_BW, "min_rate": MIN_RATE, "ms_per_call": {}}
    for k in LENGTHS:
        m = {}
        if par:
            m["calls_parent"] = stat([r["calls/%d" % k] for r in par])
        for case in CASES:
            m[case] = stat([r["%s/%d" % (case, k)] for r in own])
        if par:
            p, o = m["calls_parent"], m["calls"]
            m["ring_never_opened_against_the_parent"] = {"parent_range": [p["min"], p["max"]], "this_library_range": [o["min"], o["max"]],
                                                         "ranges_overlap": bool(o["min"] <= p["max"] and p["min"] <= o["max"]),
                                                         "no_slower_than_the_parents_slowest_process": bool(o["median"] <= p["max"])}
        nd = k * 65536 // 32
        m["bytes_per_call"] = {"ring_f32": CH * nd * 8, "rate_f32": CH * nd * 8 // 8, "rate_s16": CH * nd * 4 // 8}
        m["ring_f32_minus_calls"] = round(m["ring_f32"]["median"] - m["calls"]["median"], 4)
        m["rate_f32_minus_calls"] = round(m["rate_f32"]["median"] - m["calls"]["median"], 4)
        m["rate_s16_minus_calls"] = round(m["rate_s16"]["median"] - m["calls"]["median"], 4)
        m["gated_rate_minus_gated"] = round(m["gated_rate_f32"]["median"] - m["gated"]["median"], 4)
        res["ms_per_call"]["%d_superframes" % k] = m
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
