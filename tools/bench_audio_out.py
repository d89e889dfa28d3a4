"""What getting the audio to the host costs a call: the egress ring (pebblegpu_receiver_audio_out_*) beside the only way there was before it.
Not the bench line (bench.py measures configs[1]); the figures go into profiles/audio_out.json, DESIGN.md section 5 and the README.

    bench_audio_out.py [--calls 200] [--repeats 5] [--channels 256] [--out profiles/audio_out.json]

Shape: BASELINE configs[2] -- 256 SSB channels off one 2.048 Msps stream, int8 pairs fed through the pinned ingest slots -- in calls of 1
and of 8 super-frames.  One process, one device visit.  Per call length the four variants run alternately, --repeats times each; one
measurement is a host clock around --calls calls ending in a synchronise, after a warm-up:

    A  synchronize + memcpy_d2h   process_ingested, pebblegpu_receiver_synchronize, pebblegpu_memcpy_d2h of all audio rows into (pageable)
                                  host memory: what a host that wants the audio had to do without the ring
    B  ring, F32                  4 slots, all channels; the host takes and releases the block of the call 3 calls back
    C  ring, S16_MONO             as B, a quarter of the bytes
    D  no audio read              the calls alone: the published figure, the floor

Reported per variant: ms per call (median over the repeats, and their min / max), bytes per call, for B and C bytes per call over
ms per call in GB/s, and the host's own time per call inside the process calls (a process call waits for its run-ahead bound there)
and inside next + release.  The reader in B and C touches no sample (a host hands the pinned pointer to its sound device); A's copy
lands in pageable memory because the C ABI offers a host nothing else."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pebblesdr_amd as P  # noqa: E402
from pebblesdr_amd.binding import IQ_S8, AudioBlock, check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--out", default=None)
args = ap.parse_args()
FS, CH, SLOTS = 2.048e6, args.channels, 4
L = P.load_library()


def bank(k):
    rx = P.ReceiverBank(FS, CH, True, False, 0, max_superframes=k)
    for c in range(CH):
        rx.set_mode(c, P.DM_USB)
        rx.set_mixer(c, -900e3 + 1800e3 * (c + 0.5) / CH)
        rx.set_bandpass(c, 300, 3000)
    return rx


def run_shape(k):
    rx = bank(k)
    n = k * rx.superframe
    rng = np.random.default_rng(1)
    for slot in (0, 1):
        rx.ingest_buffer(slot, 2 * n)[:] = rng.integers(-100, 100, size=2 * n, dtype=np.int8)
    h, gain, p = rx.h, C.c_double(1.0), C.c_void_p()
    state = {"i": 0, "call_s": 0.0, "take_s": 0.0}

    def call():
        t = time.perf_counter()
        call_()
        state["call_s"] += time.perf_counter() - t

    def call_():  # the steady state of section 4 of INTEGRATION.md (the slot's samples are left as they are: no host fill is timed)
        slot = state["i"] & 1
        state["i"] += 1
        check(L, L.pebblegpu_receiver_ingest_acquire(h, slot, 2 * n, C.byref(p)))
        check(L, L.pebblegpu_receiver_ingest_submit(h, slot, 2 * n))
        check(L, L.pebblegpu_receiver_process_ingested(h, slot, IQ_S8, 0, gain, n))

    host_us = {}
    na, pitch = C.c_uint64(), C.c_uint64()
    call()
    rx.synchronize()
    d_audio = L.pebblegpu_receiver_audio(h, C.byref(na), C.byref(pitch))
    host = np.empty(CH * int(pitch.value) * 2, dtype=np.float32)  # every row, as the rows lie on the device
    blk = AudioBlock()
    blk.struct_size = C.sizeof(AudioBlock)

    def take():
        t = time.perf_counter()
        check(L, L.pebblegpu_receiver_audio_out_next(h, 1, C.byref(blk)))
        assert blk.host and not blk.dropped_before
        check(L, L.pebblegpu_receiver_audio_out_release(h, blk.call_index))
        state["take_s"] += time.perf_counter() - t

    def timed(body, drain=None):
        for _ in range(10):
            body(-1)
        if drain:
            drain()
        rx.synchronize()
        state["call_s"] = state["take_s"] = 0.0
        t0 = time.perf_counter()
        for i in range(args.calls):
            body(i)
        if drain:
            drain()
        rx.synchronize()
        ms = (time.perf_counter() - t0) / args.calls * 1e3
        host_us.setdefault(state["variant"], []).append((state["call_s"] / args.calls * 1e6, state["take_s"] / args.calls * 1e6))
        return ms

    def variant_a():
        def body(i):
            call()
            rx.synchronize()
            check(L, L.pebblegpu_memcpy_d2h(0, host.ctypes.data_as(C.c_void_p), C.c_void_p(d_audio), host.nbytes))
        return timed(body)

    def variant_ring(fmt):
        rx.audio_out_open(fmt, None, SLOTS)
        queued = {"n": 0}

        def body(i):
            call()
            queued["n"] += 1
            if queued["n"] > SLOTS - 1:  # lagging by SLOTS - 1 calls
                take()
                queued["n"] -= 1

        def drain():
            while queued["n"]:
                take()
                queued["n"] -= 1
        ms = timed(body, drain)
        dropped = rx.audio_out_dropped()
        rx.audio_out_close()
        assert dropped == 0, dropped
        return ms

    variants = {"A_sync_memcpy_d2h": variant_a, "B_ring_f32": lambda: variant_ring(P.AUDIO_F32), "C_ring_s16_mono": lambda: variant_ring(P.AUDIO_S16_MONO),
                "D_no_audio_read": lambda: timed(lambda i: call())}
    ms = {v: [] for v in variants}
    for _ in range(args.repeats):  # alternating: what drifts during the run drifts for all four
        for v, fn in variants.items():
            state["variant"] = v
            ms[v].append(fn())
    samples = int(na.value)
    nbytes = {"A_sync_memcpy_d2h": host.nbytes, "B_ring_f32": CH * samples * 8, "C_ring_s16_mono": CH * samples * 2, "D_no_audio_read": 0}
    out = {"superframes_per_call": k, "samples_per_call": n, "audio_samples_per_channel": samples, "kernels": [rx.kernel_name(w) for w in (2, 3, 4)], "variants": {}}
    for v in variants:
        med = float(np.median(ms[v]))
        r = {"ms_per_call": round(med, 4), "min": round(min(ms[v]), 4), "max": round(max(ms[v]), 4), "bytes_per_call": nbytes[v]}
        if v[0] in "BC":
            r["d2h_GBps"] = round(nbytes[v] / (med * 1e-3) / 1e9, 2)
        # where the host's time goes, per call: inside acquire + submit + process_ingested, and inside next + release
        r["host_us_in_process"] = round(float(np.median([a for a, _ in host_us[v]])), 1)
        r["host_us_in_next_release"] = round(float(np.median([b for _, b in host_us[v]])), 1)
        out["variants"][v] = r
    rx.close()
    return out


result = {
    "workload": "configs[2]: %d SSB channels off one 2.048 Msps stream, int8 pairs through the ingest slots; %d calls per measurement, %d repeats, variants alternating"
                % (CH, args.calls, args.repeats),
    "slots": SLOTS,
    "shapes": [run_shape(1), run_shape(8)],
}
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
