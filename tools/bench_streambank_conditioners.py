#!/usr/bin/env python3
"""What the stream bank's input conditioners cost a call.  Not the bench line (bench.py measures configs[1]); the figures go into
profiles/streambank_conditioners.json, DESIGN.md sections 4 and 5 and the README.

    bench_streambank_conditioners.py [--parent-lib PATH/libpebblegpu.so] [--pairs 3] [--calls 50] [--serial-calls 3] [--out profiles/streambank_conditioners.json]

Shape: a configs[4] shard -- 128 streams x 4 frames of 65536 samples per call at 200 Msps, 65536 bins, the 2048/1025 band-pass at
+-40 MHz, what = 3 -- on DEVICE-RESIDENT input, float2 (pebblegpu_streambank_process) and int8 pairs (pebblegpu_streambank_process_raw).
--pairs alternating pairs of FRESH processes in one device visit: the parent commit's library (--parent-lib, a build of the parent
commit) and this tree's.  This process never opens the device.  One measurement is a host clock around --calls calls ending in a
synchronise, after a settled warm-up; reported per case and library: the median over the pairs and their range.

    (a) calls_f32, calls_s8        no flag set, both libraries: an untouched call must cost what the parent's costs
    (b) dc, iq, nb1, nb2, all      every stream with that flag (all: 15), float2 input; all_s8: 15 on int8 input (staged).  Cost = case -
                                   calls_f32, with the passes over the rows (16 bytes per sample per out-of-place pass: 8 read, 8 written;
                                   a summary pass reads 8) and the rate against pebblegpu_probe_copy_gbps of the same process
    (c) serial_*                   the same rows through ConditionCore's kernels (k_iir_scan in its sequential mode, k_iq_balance,
                                   k_noise_blank): a receiver bank of 128 independent streams, pebblegpu_set_conditioners on every one, cost =
                                   the call with the flag minus the call without (--serial-calls calls each, in a process of its own;
                                   the receivers' IQBalance restarts every 2048 samples, the bank's every 65536: serialnf_* is
                                   k_iq_balance on receivers of 32768-sample frames -- they refuse 65536 --, as many chains per call)
"""
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

FS, S, F, N65 = 200e6, 128, 4, 65536
NF_SERIAL = 32768     # frames of the k_iq_balance harness: receivers refuse frames_per_buffer above 65535
FS_SERIAL = 2.048e6   # the receivers of (c): a super-frame of 131072 samples (at 200 Msps it is longer than the call); the kernels' cost does not depend on it
BP = 40e6
N = F * N65
BOTH = ["calls_f32", "calls_s8"]
OWN = ["dc", "iq", "nb1", "nb2", "all", "all_s8"]
FLAGS = {"dc": 1, "iq": 2, "nb1": 4, "nb2": 8, "all": 15, "all_s8": 15}
# passes over a stream's rows per call: (8-byte reads, 8-byte writes) per sample
PASSES = {"dc": (2, 1), "iq": (2, 2), "nb1": (3, 1), "nb2": (2, 1), "all": (2 + 1 + 3 + 2, 1 + 1 + 1 + 1)}
SERIAL = [0, 1, 2, 4, 8, 15]


def child(lib_path, cases, calls, serial_calls):
    """one process, one library: every case on a fresh bank -> {case: ms per call}"""
    from pebblesdr_amd.binding import IQ_S8, StreamBankConfig
    L = C.CDLL(lib_path)
    vp, u32, u64, i32, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
    L.pebblegpu_last_error.restype = C.c_char_p
    L.pebblegpu_malloc.argtypes = [i32, u64, C.POINTER(vp)]
    L.pebblegpu_free.argtypes = [i32, vp]
    L.pebblegpu_memcpy_h2d.argtypes = [i32, vp, vp, u64]
    L.pebblegpu_streambank_create.argtypes = [C.POINTER(StreamBankConfig), C.POINTER(vp)]
    L.pebblegpu_streambank_destroy.argtypes = [vp]
    L.pebblegpu_streambank_set_bandpass.argtypes = [vp, u32, dbl, dbl]
    L.pebblegpu_streambank_process.argtypes = [vp, vp, u64, u32]
    L.pebblegpu_streambank_process_raw.argtypes = [vp, i32, i32, dbl, vp, u64, u32]
    L.pebblegpu_streambank_synchronize.argtypes = [vp]

    def check(rc):
        if rc:
            raise SystemExit("%s: %s" % (lib_path, (L.pebblegpu_last_error() or b"").decode()))

    if L.pebblegpu_device_count() <= 0:
        raise SystemExit("bench_streambank_conditioners.py needs an MI355X: libpebblegpu has no CPU path")
    import bench as B
    rng = np.random.default_rng(1)
    raw = rng.integers(-100, 100, size=2 * N * S, dtype=np.int8)
    d_raw, d_f32 = vp(), vp()
    check(L.pebblegpu_malloc(0, raw.nbytes, C.byref(d_raw)))
    check(L.pebblegpu_memcpy_h2d(0, d_raw, raw.ctypes.data_as(vp), raw.nbytes))
    f32 = raw.astype(np.float32) * np.float32(1.0 / 128.0)
    check(L.pebblegpu_malloc(0, f32.nbytes, C.byref(d_f32)))
    check(L.pebblegpu_memcpy_h2d(0, d_f32, f32.ctypes.data_as(vp), f32.nbytes))
    out = {}
    for case in cases:
        cfg = StreamBankConfig()
        cfg.struct_size, cfg.device, cfg.sample_rate = C.sizeof(StreamBankConfig), 0, FS
        cfg.n_streams, cfg.frame, cfg.spectrum_bins, cfg.max_frames = S, N65, N65, F
        h = vp()
        check(L.pebblegpu_streambank_create(C.byref(cfg), C.byref(h)))
        for c in range(S):
            check(L.pebblegpu_streambank_set_bandpass(h, c, -BP, BP))
        if case in FLAGS:
            L.pebblegpu_streambank_set_conditioners.argtypes = [vp, u32, i32, dbl, dbl]
            for c in range(S):
                check(L.pebblegpu_streambank_set_conditioners(h, c, FLAGS[case], 1.02, 0.03))

        def step():
            if case.endswith("_s8"):
                check(L.pebblegpu_streambank_process_raw(h, IQ_S8, 0, 1.0, d_raw, N, 3))
            else:
                check(L.pebblegpu_streambank_process(h, d_f32, N, 3))

        def sync():
            check(L.pebblegpu_streambank_synchronize(h))

        B.settle(step, sync)
        for _ in range(5):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            step()
        sync()
        out[case] = round((time.perf_counter() - t0) / calls * 1e3, 4)
        check(L.pebblegpu_streambank_destroy(h))
    if serial_calls or "all" in cases:
        L.pebblegpu_probe_copy_gbps.argtypes = [i32, i32, C.c_size_t, i32, C.POINTER(C.c_float)]
        g = C.c_float()
        check(L.pebblegpu_probe_copy_gbps(0, 16, 1 << 30, 10, C.byref(g)))
        out["copy_gbps"] = round(g.value, 1)
    if serial_calls:
        # ConditionCore's kernels on the same float2 rows: 128 independent receivers (2048-sample frames in whole super-frames)
        import pebblesdr_amd as P
        PL = P.load_library(lib_path)
        probe = P.ReceiverBank(FS_SERIAL, 1, False, False, 0, lib=PL)
        sf = probe.superframe
        probe.close()
        # whole super-frames only: the largest run of them within the rows (the buffer is read as [S][ns]); ms are scaled to N samples
        ns = (N // sf) * sf
        if not ns:
            raise SystemExit("a super-frame of %d samples does not fit %d" % (sf, N))
        out["serial_samples_per_call"] = ns
        for fl in SERIAL:
            rx = P.ReceiverBank(FS_SERIAL, S, False, False, 0, max_superframes=ns // sf, lib=PL)
            for c in range(S):
                rx.set_conditioners(c, fl, 1.02, 0.03)
            for _ in range(2):
                rx.process_device(d_f32.value, ns)
            rx.synchronize()
            t0 = time.perf_counter()
            for _ in range(serial_calls):
                rx.process_device(d_f32.value, ns)
            rx.synchronize()
            out["serial_%d" % fl] = round((time.perf_counter() - t0) / serial_calls * 1e3 * N / ns, 4)
            rx.close()
        # k_iq_balance near the bank's frame length: receivers take frames below 65536, so 32768-sample frames (NF_SERIAL), as many
        # (stream, frame) chains per call as the bank's call has (S * F), each half as long; fewer streams of longer rows, the same
        # device buffer read as [streams][super-frame]
        try:
            probe = P.ReceiverBank(FS_SERIAL, 1, False, False, 0, frames_per_buffer=NF_SERIAL, lib=PL)
            sf = probe.superframe
            probe.close()
            streams = (S * F) // (sf // NF_SERIAL)
            if streams < 1 or streams * sf > S * N:
                raise RuntimeError("a super-frame of %d samples: %d streams do not fit the buffer" % (sf, streams))
            for fl in (0, 2):
                rx = P.ReceiverBank(FS_SERIAL, streams, False, False, 0, frames_per_buffer=NF_SERIAL, max_superframes=1, lib=PL)
                for c in range(streams):
                    rx.set_conditioners(c, fl, 1.02, 0.03)
                rx.process_device(d_f32.value, sf)
                rx.synchronize()
                t0 = time.perf_counter()
                for _ in range(serial_calls):
                    rx.process_device(d_f32.value, sf)
                rx.synchronize()
                out["serialnf_%d" % fl] = round((time.perf_counter() - t0) / serial_calls * 1e3, 4)
                rx.close()
            out["serialnf_shape"] = "%d streams x %d frames of %d" % (streams, sf // NF_SERIAL, NF_SERIAL)
        except Exception as e:  # (a refusal is a result too)
            out["serialnf_error"] = str(e)[-300:]
    check(L.pebblegpu_free(0, d_raw))
    check(L.pebblegpu_free(0, d_f32))
    print(json.dumps(out))


def run_child(lib_path, cases, calls, serial_calls=0):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, "--cases", ",".join(cases), "--calls", str(calls),
                          "--serial-calls", str(serial_calls)], cwd=ROOT, stdout=subprocess.PIPE, timeout=900, check=True).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def stat(v):
    v = sorted(v)
    return {"median": round(float(np.median(v)), 4), "min": v[0], "max": v[-1], "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--serial-calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--cases", default=",".join(BOTH + OWN))
    args = ap.parse_args()
    if args.child:
        return child(args.child, [c for c in args.cases.split(",") if c], args.calls, args.serial_calls)
    own_lib = os.path.join(ROOT, "pebblesdr_amd", "libpebblegpu.so")
    par, own = [], []
    for _ in range(args.pairs):
        if args.parent_lib:
            par.append(run_child(os.path.abspath(args.parent_lib), BOTH, args.calls))
        own.append(run_child(own_lib, BOTH + OWN, args.calls))
    serial = {}
    if args.serial_calls:  # (a process of its own)
        try:
            serial = run_child(own_lib, [], args.calls, args.serial_calls)
        except subprocess.SubprocessError as e:
            serial = {"error": str(e)[-300:]}
    res = {"shape": "configs[4] shard: %d streams x %d frames of %d samples per call, device-resident float2 and int8 pairs, %g Msps, band-pass +-%g MHz, "
                    "what = 3" % (S, F, N65, FS / 1e6, BP / 1e6), "calls": args.calls, "pairs": args.pairs, "ms_per_call": {}}
    m = res["ms_per_call"]
    for case in BOTH:
        if par:
            m[case + "_parent"] = stat([r[case] for r in par])
    for case in BOTH + OWN:
        m[case] = stat([r[case] for r in own])
    if par:
        res["untouched_calls_against_the_parent"] = {}
        for case in BOTH:
            p, o = m[case + "_parent"], m[case]
            res["untouched_calls_against_the_parent"][case] = {
                "parent_range": [p["min"], p["max"]], "this_library_range": [o["min"], o["max"]], "parent_median": p["median"],
                "this_library_median": o["median"], "ranges_overlap": bool(o["min"] <= p["max"] and p["min"] <= o["max"]),
                "no_slower_than_the_parents_slowest_process": bool(o["median"] <= p["max"])}
    copy = float(np.median([r["copy_gbps"] for r in own if "copy_gbps" in r]))
    res["copy_gbps"] = copy
    samples = S * N
    res["conditioners"] = {}
    for case in ("dc", "iq", "nb1", "nb2", "all"):
        ms = m[case]["median"] - m["calls_f32"]["median"]
        rd, wr = PASSES[case]
        nbytes = samples * 8 * (rd + wr)
        res["conditioners"][case] = {"ms_per_call": round(ms, 4), "passes_read_8B": rd, "passes_written_8B": wr, "bytes_per_call": nbytes,
                                     "GBps": round(nbytes / ms / 1e6, 1) if ms > 0 else None,
                                     "fraction_of_copy_rate": round(nbytes / ms / 1e6 / copy, 3) if ms > 0 else None}
    res["conditioners"]["all_s8"] = {"ms_per_call": round(m["all_s8"]["median"] - m["calls_s8"]["median"], 4),
                                     "note": "against the converting-loads call: includes k_normalize_iq (2 B read, 8 B written per sample)"}
    last = serial
    if "error" in last:
        res["serial_kernels_error"] = last["error"]
    if "serial_0" in last:
        res["serial_samples_per_call"] = last["serial_samples_per_call"]
        res["serial_kernels_ms_per_call"] = {str(fl): round(last["serial_%d" % fl] - last["serial_0"], 4) for fl in SERIAL if fl}
        res["serial_kernels_ms_per_call"]["receiver_call_without_flags"] = last["serial_0"]
        res["against_the_serial_kernels"] = {
            name: {"serial_ms": res["serial_kernels_ms_per_call"][str(fl)], "time_parallel_ms": res["conditioners"][name]["ms_per_call"],
                   "ratio": round(res["serial_kernels_ms_per_call"][str(fl)] / res["conditioners"][name]["ms_per_call"], 1)
                   if res["conditioners"][name]["ms_per_call"] > 0 else None}
            for name, fl in (("dc", 1), ("iq", 2), ("nb1", 4), ("nb2", 8), ("all", 15))}
    if "serialnf_2" in last:
        ms = round(last["serialnf_2"] - last["serialnf_0"], 4)
        res["k_iq_balance_at_32768_sample_frames"] = {
            "shape": last["serialnf_shape"], "ms_per_call": ms, "chains_per_call": S * F, "steps_per_chain": NF_SERIAL,
            "us_per_1000_steps": round(ms * 1e3 / (NF_SERIAL / 1000.0), 3),
            "k_cond_iq_us_per_1000_steps": round(res["conditioners"]["iq"]["ms_per_call"] * 1e3 / (N65 / 1000.0), 3),
            "note": "both are one chain of dependent steps per (stream, frame), 512 chains per call: time per step is what compares"}
    elif "serialnf_error" in last:
        res["k_iq_balance_at_32768_sample_frames"] = {"error": last["serialnf_error"]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
