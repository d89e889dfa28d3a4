#!/usr/bin/env python3
"""What the stream bank's S-meter and squelch cost a call.  Not the bench line (bench.py measures configs[1]); the figures go into
profiles/streambank_smeter.json, DESIGN.md section 4 and the README.

    bench_streambank_smeter.py [--parent-lib PATH/libpebblegpu.so] [--pairs 4] [--calls 200] [--kernel-ns NS] [--out profiles/streambank_smeter.json]

Shape: the configs[4] shard of tools/bench_streambank_gate.py -- 128 streams x 4 frames of 65536 samples per call at 200 Msps, 65536
bins, what = 3 -- fed as int8 pairs through the pinned ingest slots (acquire, submit, process_ingested per call, the slots' samples left
as they are), the 2048/1025 band-pass at +-40 MHz.  --pairs alternating pairs of FRESH processes in one device visit: the parent
commit's library (--parent-lib, a build of the parent commit) and this tree's.  This process never opens the device.  Cases:

    calls           the calls alone, parent and this library: does an S-meter that is off cost anything?
    smeter          pebblegpu_streambank_enable_signal_strength: k_stream_strength over 512 rows of 65536 bins per call; at +-40 MHz both
                    noise windows clamp, so every row is read whole: 134 MB of compulsory traffic per call
    squelch_ring    a threshold of -60 dB on every stream, the F32 IQ ring open on 8 streams (the gated packing instance)
    open_ring       the same ring, S-meter on, every threshold at -120 (the trailer only: the ungated packing instance)
The parent's process runs `calls` only.  One measurement is a host clock around --calls calls ending in a synchronise, after a settled
warm-up; reported per case and library: the median over the pairs and their range.  The loop is bound by the upload of 67 MB per call,
so (smeter - calls) says what the S-meter costs a host and not how long k_stream_strength runs.  The kernel's own time comes from a
run of its own under the profiler, outside this tool:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_streambank_smeter.py --child pebblesdr_amd/libpebblegpu.so --cases smeter --calls 40
    python tools/kernel_stats.py DIR kernels.csv
--kernel-ns takes k_stream_strength's average from that table and states the achieved bandwidth against the compulsory bytes.
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

FS, S, F, N65, SLOTS = 200e6, 128, 4, 65536, 4
BP = 40e6
HBM_PEAK_GBPS = 8000.0   # MI355X: 8 TB/s
CASES = ["calls", "smeter", "squelch_ring", "open_ring"]


def child(lib_path, cases, calls):
    """one process, one library: every case on a fresh bank -> {case: ms per call}"""
    from pebblesdr_amd.binding import IQ_S8, AudioBlock, StreamBankConfig
    L = C.CDLL(lib_path)
    vp, u32, u64, i32, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
    L.pebblegpu_last_error.restype = C.c_char_p
    L.pebblegpu_streambank_create.argtypes = [C.POINTER(StreamBankConfig), C.POINTER(vp)]
    L.pebblegpu_streambank_destroy.argtypes = [vp]
    L.pebblegpu_streambank_set_bandpass.argtypes = [vp, u32, dbl, dbl]
    L.pebblegpu_streambank_ingest_acquire.argtypes = [vp, u32, u64, C.POINTER(vp)]
    L.pebblegpu_streambank_ingest_submit.argtypes = [vp, u32, u64]
    L.pebblegpu_streambank_process_ingested.argtypes = [vp, u32, i32, i32, dbl, u64, u32]
    L.pebblegpu_streambank_synchronize.argtypes = [vp]
    L.pebblegpu_streambank_iq_out_open.argtypes = [vp, i32, C.POINTER(u32), u32, u32]
    L.pebblegpu_streambank_iq_out_next.argtypes = [vp, i32, C.POINTER(AudioBlock)]
    L.pebblegpu_streambank_iq_out_release.argtypes = [vp, u64]

    def check(rc):
        if rc:
            raise SystemExit("%s: %s" % (lib_path, (L.pebblegpu_last_error() or b"").decode()))

    if L.pebblegpu_device_count() <= 0:
        raise SystemExit("bench_streambank_smeter.py needs an MI355X: libpebblegpu has no CPU path")
    import bench as B
    n = F * N65
    raw_bytes = 2 * n * S
    rng = np.random.default_rng(1)
    out = {}
    for case in cases:
        cfg = StreamBankConfig()
        cfg.struct_size, cfg.device, cfg.sample_rate = C.sizeof(StreamBankConfig), 0, FS
        cfg.n_streams, cfg.frame, cfg.spectrum_bins, cfg.max_frames = S, N65, N65, F
        h = vp()
        check(L.pebblegpu_streambank_create(C.byref(cfg), C.byref(h)))
        for c in range(S):
            check(L.pebblegpu_streambank_set_bandpass(h, c, -BP, BP))
        p = vp()
        for slot in (0, 1):
            check(L.pebblegpu_streambank_ingest_acquire(h, slot, raw_bytes, C.byref(p)))
            np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int8)), shape=(raw_bytes,))[:] = rng.integers(-100, 100, size=raw_bytes, dtype=np.int8)
        ring = case in ("squelch_ring", "open_ring")
        if case != "calls":
            L.pebblegpu_streambank_enable_signal_strength.argtypes = [vp, i32]
            L.pebblegpu_streambank_set_squelch.argtypes = [vp, u32, dbl]
            check(L.pebblegpu_streambank_enable_signal_strength(h, 1))
        if case == "squelch_ring":
            for c in range(S):
                check(L.pebblegpu_streambank_set_squelch(h, c, -60.0))
        if ring:
            sel = (u32 * 8)(*[(S // 8) * i + 1 for i in range(8)])
            check(L.pebblegpu_streambank_iq_out_open(h, 0, sel, 8, SLOTS))
        blk = AudioBlock()
        blk.struct_size = C.sizeof(AudioBlock)
        st = {"i": 0, "queued": 0}

        def take():
            check(L.pebblegpu_streambank_iq_out_next(h, 1, C.byref(blk)))
            assert blk.host and not blk.dropped_before
            check(L.pebblegpu_streambank_iq_out_release(h, blk.call_index))
            st["queued"] -= 1

        def step():
            slot = st["i"] & 1
            st["i"] += 1
            check(L.pebblegpu_streambank_ingest_acquire(h, slot, raw_bytes, C.byref(p)))
            check(L.pebblegpu_streambank_ingest_submit(h, slot, raw_bytes))
            check(L.pebblegpu_streambank_process_ingested(h, slot, IQ_S8, 0, 1.0, n, 3))
            if ring:
                st["queued"] += 1
                if st["queued"] > SLOTS - 1:   # the reader lags by SLOTS - 1 calls
                    take()

        def sync():
            while st["queued"]:
                take()
            check(L.pebblegpu_streambank_synchronize(h))

        B.settle(step, sync)
        for _ in range(10):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            step()
        sync()
        out[case] = round((time.perf_counter() - t0) / calls * 1e3, 4)
        check(L.pebblegpu_streambank_destroy(h))
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
    ap.add_argument("--kernel-ns", type=float, default=None)
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
    res = {"shape": "configs[4] shard: %d streams x %d frames of %d int8 pairs through the ingest slots at %g Msps, band-pass +-%g MHz, what = 3"
                    % (S, F, N65, FS / 1e6, BP / 1e6), "calls": args.calls, "pairs": args.pairs, "ms_per_call": {}}
    if par:
        res["ms_per_call"]["calls_parent"] = stat([r["calls"] for r in par])
    for case in CASES:
        res["ms_per_call"][case] = stat([r[case] for r in own])
    m = res["ms_per_call"]
    if par:
        p, o = m["calls_parent"], m["calls"]
        res["smeter_off_against_the_parent"] = {"parent_range": [p["min"], p["max"]], "this_library_range": [o["min"], o["max"]],
                                                "parent_median": p["median"], "this_library_median": o["median"],
                                                "ranges_overlap": bool(o["min"] <= p["max"] and p["min"] <= o["max"]),
                                                "no_slower_than_the_parents_slowest_process": bool(o["median"] <= p["max"])}
    rows = S * F
    traffic = rows * N65 * 4
    delta = m["smeter"]["median"] - m["calls"]["median"]
    res["k_stream_strength"] = {"rows_per_call": rows, "compulsory_bytes_per_call": traffic, "smeter_minus_calls_ms": round(delta, 4),
                                "note": "the loop is upload-bound: the difference of the two medians is what the S-meter costs a host per call"}
    if args.kernel_ns:
        gbps = traffic / args.kernel_ns
        res["k_stream_strength"].update({"kernel_ms_from_a_kernel_trace": round(args.kernel_ns / 1e6, 4), "GBps": round(gbps, 1),
                                         "fraction_of_hbm_peak_8TBps": round(gbps / HBM_PEAK_GBPS, 3)})
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
