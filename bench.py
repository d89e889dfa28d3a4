"""bench.py -- IQ Msamples/s through the full receive chain on MI355X (BASELINE.json metric).

Headline workload (BASELINE.json configs[1]): synthetic 20 Msps HackRF-shape IQ, one tuned channel per GPU, mixer ->
decimator (hb11x8, hb15, hb23, hb47 -> 312.5 kHz) -> WFM mono demod, plus the 8192-bin SignalSpectrum FFT on every
2048-sample frame.  One "step" = one pass of that chain over one batch of `--superframes` super-frames
(131072 samples each) already resident in HBM.

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]   # N = 1
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   # one rank per GPU

A plain run does only what the headline needs: set-up, warm-up (W steps, the untimed settle phase settle(), one untimed call
after re-tuning the oscillator, W steps), exactly K timed steps, the outputs of the last timed step if --dump-outputs is given,
and the JSON line (value, ms_per_step and the headline kernel's roofline from the HIP events of the timed steps).  Everything
else, described below, runs with --full only.

--dump-outputs DIR (rank 0): what a caller of the timed path receives after the last timed step, as float32 .npy files:
  audio.npy             [1, n / 64, 2]   the channel's audio (pebblegpu_receiver_audio), (re, im)
  spectrum_sample.npy   [1, 512, 8192]   512 of the call's 16 384 spectrum rows (pebblegpu_receiver_spectrum), picked with
                                         np.random.default_rng(0) and sorted; all rows when the call has no more than 512
The input is regenerated from fixed seeds, and the re-tune resets the oscillator's phase, so that how many steps settle() ran
does not reach the outputs: runs with the same arguments dump the same arrays.

With --full the same JSON line also carries the un-settled rate (the K steps right after the W warm-ups, before settle()), the
spectrum kernel alone, the measured copy peak and socket power, the CPU baseline (unless --no-cpu-baseline) and, under
"configs" (unless --headline-only), the other BASELINE workloads timed with the same discipline (warm-up, barrier
+ device sync, K steps, barrier + device sync, max over ranks), each with its own per-kernel HIP-event times and roofline:
  configs[2]        2.048 Msps shared stream -> 256 tuned USB channels: mixer + hb11x4,hb15,hb19,hb31 + FastFIR 2048/1025
                    (the full mixer -> decimate -> FastFIR -> demod chain the metric names); N = 1 only (a one-GPU config)
  configs[3] shard  100 Msps shared stream -> 512 AM/USB channels per GPU (rank r tunes global channels [512 r, 512 r + 512))
  configs[4] shard  128 full-rate streams per GPU: FastFIR 2048/1025 + 65536-point spectrum (rank r owns streams [128 r, ...))
and, at N = 1, the headline fed as raw int8 pairs ("raw_int8": pebblegpu_receiver_process_raw) and the PCIe-inclusive
rates ("pcie_inclusive", never `value`).

Channels / streams are independent: every rank owns its shard, nothing is exchanged, so the only
collectives are the control-plane barrier and the max-over-ranks of the elapsed time (gloo, CPU tensors) -- weak scaling.
Rank 0 prints ONE JSON line.  With fewer devices than ranks the run exits non-zero instead of oversubscribing a GPU.

The CPU baseline leg (--full) builds and runs oracle/cpu_baseline.cpp (the oracle's scalar fp64 restatement of the reference chain,
-O3 -march=native, std::threads over the host's cores); it is the only place this file touches oracle/.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS = 20_000_000
NF = 2048
BINS = 8192
MIX_HZ = 1.0e6
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E datasheet peak (MI355X_MICROARCH.md); the same guide measures 6.29 TB/s for a float4 copy
C3_PER_GPU, C4_PER_GPU = 512, 128  # BASELINE.json configs[3], configs[4]: channels / streams per GPU


def shard_streams(world, rank, per_rank=1):
    """Static contiguous shards: rank r owns units [r*per_rank, (r+1)*per_rank)."""
    return list(range(rank * per_rank, (rank + 1) * per_rank))


def aggregate_msps(samples_per_rank, world, seconds):
    return samples_per_rank * world / seconds / 1e6


def make_input(n, seed):
    """FM-modulated 1 kHz tone, 75 kHz deviation, +1 MHz offset, noise; quantised to int8/128 (HackRF CPX8 shape)."""
    from tests.signals import lcg_noise
    out = np.empty(n, dtype=np.complex64)
    blk = 1 << 22
    for lo in range(0, n, blk):
        hi = min(n, lo + blk)
        t = np.arange(lo, hi, dtype=np.float64) / FS
        x = 0.5 * np.exp(1j * (2 * np.pi * MIX_HZ * t + 75.0 * np.sin(2 * np.pi * 1000 * t)))
        x = x + lcg_noise(hi - lo, seed + lo // blk, 1e-2)
        out[lo:hi] = (np.round(x.real * 128) + 1j * np.round(x.imag * 128)) / 128.0
    return out


def bank_plan(fs, n_global, g):
    """Tuning plan of the shared-stream banks: global channel g of n_global sits at (g - G/2) * 0.8 fs / G."""
    return (g - n_global / 2.0) * (0.8 * fs / n_global)


def make_bank_input(fs, n, freqs, seed):
    """a tone 1.5 kHz above a sample of the channels' centres (inside each USB / AM pass-band) plus LCG noise, |x| < 0.9"""
    from tests.signals import lcg_noise
    rng = np.random.default_rng(seed)
    x = lcg_noise(n, seed, 0.05).astype(np.complex64)
    t = np.arange(n, dtype=np.float64) / fs
    pick = freqs if len(freqs) <= 32 else [freqs[i] for i in np.linspace(0, len(freqs) - 1, 32).astype(int)]
    for f in pick:
        x += (0.01 * np.exp(1j * (2 * np.pi * (f + 1500.0) * t + rng.uniform(0, 2 * np.pi)))).astype(np.complex64)
    return x


def cpu_baseline(workload, seconds, what):
    """oracle/cpu_baseline.cpp on this host: 1 thread and all threads."""
    exe = os.path.join(ROOT, "oracle", "_build", "cpu_baseline")
    try:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "_build/cpu_baseline"], stdout=subprocess.DEVNULL)
        r = json.loads(subprocess.check_output([exe, str(workload), str(seconds), "0"]).decode())
    except Exception as e:  # no compiler on the box: say so instead of inventing a number
        return {"value": None, "unit": "Msamples/s", "cores": 0, "kind": "port", "sample": "cpu_baseline could not be built/run: %r" % (e,)}
    return {"value": r["msamples_per_s_all_threads"], "unit": "Msamples/s", "cores": r["threads"], "kind": "port", "dtype": "f64",
            "value_1thread": r["msamples_per_s_1thread"], "cpu_model": r["cpu_model"], "hardware_concurrency": r["hardware_concurrency"],
            "sample": "%s: %.0f s on 1 thread, then %.0f s with the %d units spread over %d std::threads; oracle/ scalar fp64 "
                      "(-O3 -march=native), frame loop in C++; the GPU path computes in f32" % (what, r["seconds_per_leg"], r["seconds_per_leg"], r["units"], r["threads"])}


def pmc_traffic(superframes):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE in
    separate runs, gfx950 half-count correction calibrated on known-size copies): tools/pmc_workload.py +
    tools/parse_traffic.py.  Only valid for the batch size it was measured on (256 super-frames)."""
    for name in ("r03_traffic_head.json", "r02_traffic.json", "r01_traffic.json"):
        path = os.path.join(ROOT, "profiles", name)
        if superframes != 256 or not os.path.exists(path):
            continue
        try:
            return int(round(json.load(open(path))["kernels"]["k_spectrum"]["hbm_bytes"])), "profiles/" + name + " (rocprofv3 --pmc passes of the same workload, not collected in this run)"
        except Exception:
            continue
    return None, None


def attach_measured_traffic(ks, roof, files):
    """HBM bytes per launch from the committed PMC passes of the same geometry (tools/profile_round.sh: tools/pmc_bank.py 2|3,
    tools/pmc_streambank.py; FETCH_SIZE and WRITE_SIZE in separate runs, parsed by tools/parse_traffic.py) onto the per-kernel lines
    and the dominant kernel's roofline.  A label naming two launches ("a + b") gets the sum of both."""
    for name in files:
        path = os.path.join(ROOT, "profiles", name)
        try:
            meas = json.load(open(path))["kernels"]
        except Exception:
            continue

        def total(label):
            parts = [p.strip().split("<")[0].split(" ")[0] for p in label.split(" + ")]
            if not all(p in meas for p in parts):
                return None
            return int(round(sum(meas[p]["hbm_bytes"] for p in parts)))
        hit = False
        for kn, v in ks.items():
            t = total(kn)
            if t is not None:
                v["hbm_bytes_measured"] = t
                hit = True
        if roof is not None and total(roof["kernel"]) is not None:
            roof["traffic"] = total(roof["kernel"])
            roof["traffic_source"] = "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same workload, not collected in this run)" % name
        if hit:
            return


def socket_power(step, sync, seconds=2.5):
    """Socket power (rocm-smi) while the workload's steps are queued back to back for a couple of seconds, untimed: whether the
    kernel the roofline prices runs against the chip's power limit rather than a pipe's.  Returns {"busy_W", "idle_W"} or None
    when rocm-smi is not there to ask."""
    import shutil
    import threading
    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if not os.path.exists(exe):
        return None

    def read():
        try:
            out = subprocess.run([exe, "--showpower"], capture_output=True, text=True, timeout=20).stdout
        except Exception:
            return None
        for line in out.splitlines():
            if "(W):" in line:
                try:
                    return float(line.split("(W):")[1])
                except ValueError:
                    return None
        return None

    sync()
    idle = read()
    stop = threading.Event()

    def work():
        while not stop.is_set():
            for _ in range(50):
                step()
            sync()

    th = threading.Thread(target=work)
    th.start()
    time.sleep(seconds * 0.5)
    busy = [read() for _ in range(2)]
    stop.set()
    th.join()
    busy = [b for b in busy if b is not None]
    if not busy:
        return None
    return {"busy_W": round(sum(busy) / len(busy), 0), "idle_W": idle, "how": "rocm-smi --showpower, twice, ~1.3 s into an untimed run of back-to-back steps"}


def settle(step, sync, max_s=0.5, batch=20):
    """Untimed steps until the step time stops falling.  After an idle spell (set-up, a host-side pause) the GPU's clocks take
    tens of milliseconds of sustained load to come up: the first 40 steps of the headline workload run at 0.35 ms, from step
    ~100 on at 0.29 (profiles/README.md), and 2 s of idleness resets that.  The W warm-up steps of the contract (a handful)
    would leave the K timed steps inside that ramp; a receive chain runs continuously, so the rate that means something is the
    settled one.  Batches of `batch` steps (at least 5 ms of work each) with a device sync after each, until a batch is no more than 2 % faster than the one
    before it or `max_s` seconds have passed; returns the number of steps run."""
    sync()
    prev, total = None, 0
    t_start = time.perf_counter()
    while time.perf_counter() - t_start < max_s:
        t0 = time.perf_counter()
        for _ in range(batch):
            step()
        sync()
        dt = (time.perf_counter() - t0) / batch
        total += batch
        if prev is not None and dt > prev * 0.98:
            break
        prev = dt
        if dt * batch < 0.005:  # (a batch shorter than the ramp's own time scale would look settled at once: at least 5 ms of work each)
            batch = int(0.005 / dt) + 1
            prev = None
    return total


def timed_steps(step, barrier, steps, dist):
    """barrier + device sync, exactly `steps` steps, barrier + device sync; MAX of the elapsed time over ranks."""
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed


def control_plane_rehearsal(args, rank, world, dist):
    n = args.superframes * 131072
    shard = shard_streams(world, rank)

    def barrier():
        if dist is not None:
            dist.barrier()

    elapsed = timed_steps(lambda: time.sleep(0.002 * (rank + 1)), barrier, args.steps, dist)
    if dist is not None:
        owned, owned3, owned4 = [None] * world, [None] * world, [None] * world
        dist.all_gather_object(owned, shard)
        dist.all_gather_object(owned3, shard_streams(world, rank, C3_PER_GPU)[::C3_PER_GPU - 1])
        dist.all_gather_object(owned4, shard_streams(world, rank, C4_PER_GPU)[::C4_PER_GPU - 1])
    else:
        owned, owned3, owned4 = [shard], [shard_streams(1, 0, C3_PER_GPU)[::C3_PER_GPU - 1]], [shard_streams(1, 0, C4_PER_GPU)[::C4_PER_GPU - 1]]
    if rank == 0:
        print(json.dumps({"metric": "control-plane rehearsal (no GPU work)", "n_gpus": world, "steps": args.steps,
                          "value": round(aggregate_msps(n * args.steps, world, elapsed), 2), "unit": "Msamples/s",
                          "ms_per_step": round(elapsed / args.steps * 1e3, 4), "scaling": "weak", "streams_by_rank": owned,
                          "configs3_channel_range_by_rank": owned3, "configs4_stream_range_by_rank": owned4}))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


DUMP_SPECTRUM_ROWS = 512


def dump_outputs(rx, out_dir):
    """--dump-outputs: the last call's audio and a fixed, seeded sample of its spectrum rows as float32 .npy (about 20 MB at the
    default --superframes 256); see the module docstring."""
    os.makedirs(out_dir, exist_ok=True)
    a = rx.audio()  # complex64 [C, n / D]
    np.save(os.path.join(out_dir, "audio.npy"), np.ascontiguousarray(a).view(np.float32).reshape(a.shape + (2,)))
    s = rx.spectrum()  # float32 [streams, frames, bins]
    if s.shape[1] > DUMP_SPECTRUM_ROWS:
        s = s[:, np.sort(np.random.default_rng(0).choice(s.shape[1], DUMP_SPECTRUM_ROWS, replace=False))]
    np.save(os.path.join(out_dir, "spectrum_sample.npy"), np.ascontiguousarray(s, dtype=np.float32))


def kernel_lines(groups):
    """[(name, ms, algorithmic bytes)] -> per-kernel dict + the dominant kernel's roofline object"""
    ks = {}
    for name, ms, b in groups:
        if name and ms > 0:
            ks[name] = {"ms": round(ms, 4), "algorithmic_bytes": int(b), "GBps": round(b / (ms * 1e-3) / 1e9, 1)}
    if not ks:
        return ks, None
    dom = max(ks, key=lambda k: ks[k]["ms"])
    roof = {"bound": "hbm", "kernel": dom, "achieved": ks[dom]["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(ks[dom]["GBps"] / HBM_PEAK_GBS, 4), "traffic": None, "avg_launch_ms": ks[dom]["ms"],
            "algorithmic_bytes_per_launch": ks[dom]["algorithmic_bytes"]}
    return ks, roof


def run_bank(P, name, fs, C, modes, k, rank, world, device, barrier, args, dist):
    """A shared-stream bank of C channels per GPU: mixer + decimator + FastFIR + demod for every channel (no spectrum)."""
    G = C * world
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=k, device=device)
    freqs = []
    for c in range(C):
        g = rank * C + c
        m = modes[g % len(modes)]
        rx.set_mode(c, m)
        f = bank_plan(fs, G, g)
        freqs.append(f)
        rx.set_mixer(c, f)
        if m == P.DM_USB:
            rx.set_bandpass(c, 300, 3000)
        else:
            rx.set_bandpass(c, -4000, 4000)
    n = k * rx.superframe
    x = make_bank_input(fs, n, freqs, 3)  # the shared wideband stream is replicated to every GPU
    buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x), device)
    del x
    settled = settle(lambda: rx.process_device(buf.ptr, n), rx.synchronize)
    for _ in range(max(2, args.warmup)):
        rx.process_device(buf.ptr, n)
    rx.synchronize()
    # these calls take under 0.1 ms and run as two overlapping stages: with the contract's K (20) a tenth of the timed region is the
    # pipeline filling and draining around the barriers -- the side configurations are timed over at least 200 calls ("steps" below)
    bank_steps = max(args.steps, 200)
    elapsed = timed_steps(lambda: rx.process_device(buf.ptr, n), barrier, bank_steps, dist)
    # per-kernel HIP events (four more event records per call, so outside the timed region)
    rx.set_profiling(True)
    for _ in range(4):
        rx.process_device(buf.ptr, n)
    rx.synchronize()
    ms = {w: rx.mean_ms(w, 3) for w in (2, 3, 4, 5)}
    names = {w: rx.kernel_name(w) for w in (2, 3, 4, 5)}
    chain = rx.chain()
    D = rx.D
    n_am = sum(1 for c in range(C) if modes[(rank * C + c) % len(modes)] == P.DM_AM)
    d0 = chain[0][1] * (chain[1][1] if names[2] == "k_mix_cic_hb" else 1)
    if names[3] == "":
        d0 = D  # the whole decimator is one kernel: nothing is written above the demod rate
    front_b = 8 * n + 8 * C * n // d0
    rest_b = 8 * C * n // d0 + 8 * C * n // D
    groups = [(names[2], ms[2], front_b), (names[3], ms[3], rest_b), (names[4], ms[4], 16 * C * n // D),
              ("AM demod: k_iir_scan + k_fir_dec" if n_am else "", ms[5], 16 * n_am * n // D)]
    ks, roof = kernel_lines(groups)
    if (fs, C, k) == (2048000, 256, 8):  # configs[2] exactly as the committed PMC passes ran it (tools/pmc_bank.py 2)
        attach_measured_traffic(ks, roof, ("r03_traffic_configs2.json", "r02_traffic_configs2.json"))
    elif (fs, C, k) == (100000000, 512, 1):  # the configs[3] shard (tools/pmc_bank.py 3)
        attach_measured_traffic(ks, roof, ("r03_traffic_configs3.json",))
    t_ms = elapsed / bank_steps * 1e3
    comp = 8 * n + 8 * C * n // D
    actual = sum(v["algorithmic_bytes"] for v in ks.values())
    out = {"workload": name, "fs": fs, "channels_per_gpu": C, "channels_total": G, "input_samples_per_step": n,
           "chain": "%s (D = %d)" % (", ".join(("cic3" if t == 0 else "hb%d" % t) + ("x%d" % s if s > 2 else "") for t, s in chain), D),
           "ms_per_step": round(t_ms, 4), "steps": bank_steps, "settle_steps": settled, "channel_Msamples_per_s": round(C * world * n / (t_ms * 1e-3) / 1e6, 1),
           "input_Msamples_per_s": round(n / (t_ms * 1e-3) / 1e6, 1),
           "bytes_compulsory": comp, "bytes_moved_by_kernels": actual, "moved_over_compulsory": round(actual / comp, 2),
           "compulsory_GBps": round(comp / (t_ms * 1e-3) / 1e9, 1), "frac_of_peak_on_compulsory_bytes": round(comp / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "kernels": ks, "roofline": roof}
    rx.close()
    buf.free()
    return out


def bank_batch_sweep(P, fs, C, modes, ks, device, steps):
    """configs[2]'s chain at several batch sizes (super-frames per call): the whole call and the decimator kernel alone.  Separates
    what a call's fixed costs and the decimator's per-chunk warm-up take from the kernels' rate."""
    rows = []
    for k in ks:
        rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=k, device=device)
        freqs = []
        for c in range(C):
            rx.set_mode(c, modes[c % len(modes)])
            f = bank_plan(fs, C, c)
            freqs.append(f)
            rx.set_mixer(c, f)
            rx.set_bandpass(c, 300, 3000)
        n = k * rx.superframe
        x = make_bank_input(fs, n, freqs, 3)
        buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x), device)
        del x
        settle(lambda: rx.process_device(buf.ptr, n), rx.synchronize, max_s=0.3)
        rx.synchronize()
        calls = max(steps, 1600 // k)  # (two overlapping stages per call: enough calls that filling and draining the pipeline do not show)
        t0 = time.perf_counter()
        for _ in range(calls):
            rx.process_device(buf.ptr, n)
        rx.synchronize()
        t_ms = (time.perf_counter() - t0) / calls * 1e3
        rx.set_profiling(True)
        for _ in range(4):
            rx.process_device(buf.ptr, n)
        rx.synchronize()
        rows.append({"superframes_per_call": k, "input_samples": n, "calls": calls, "ms_per_call": round(t_ms, 4),
                     "channel_Msamples_per_s": round(C * n / (t_ms * 1e-3) / 1e6, 1),
                     "decimator_kernel": rx.kernel_name(2), "decimator_ms": round(rx.mean_ms(2, 3), 4), "fastfir_ms": round(rx.mean_ms(4, 3), 4),
                     "decimator_channel_Msamples_per_s": round(C * n / (rx.mean_ms(2, 3) * 1e-3) / 1e6, 1)})
        rx.close()
        buf.free()
    return rows


def run_streambank(P, rank, world, device, barrier, args, dist):
    """BASELINE configs[4] shard: 128 streams per GPU, FastFIR 2048/1025 at the stream rate + 65536-point spectrum."""
    S, N, F = C4_PER_GPU, 65536, 4
    rng = np.random.default_rng(4 + rank)
    x = np.empty((S, F * N), dtype=np.complex64)
    for s in range(S):
        x[s] = (rng.standard_normal(F * N, dtype=np.float32) + 1j * rng.standard_normal(F * N, dtype=np.float32)) * np.float32(0.1)
    sb = P.StreamBank(2.0e6, S, frame=N, spectrum_bins=N, max_frames=F, device=device)
    for c in range(S):
        sb.set_bandpass(c, -50e3, 50e3)
    buf = P.DeviceBuffer.from_array(x.view(np.float32), device)
    del x
    settled = settle(lambda: sb.process_device(buf.ptr, F * N), sb.synchronize)
    for _ in range(max(2, args.warmup)):
        sb.process_device(buf.ptr, F * N)
    sb.synchronize()
    elapsed = timed_steps(lambda: sb.process_device(buf.ptr, F * N), barrier, args.steps, dist)
    bp, sp = [], []
    for _ in range(4):
        sb.process_device(buf.ptr, F * N)
        bp.append(sb.last_ms(1))
        sp.append(sb.last_ms(2))
    n = S * F * N
    ks, roof = kernel_lines([("k_fastfir_t128", float(np.mean(bp[1:])), 16 * n), (sb.spectrum_kernels(), float(np.mean(sp[1:])), 12 * n)])
    attach_measured_traffic(ks, roof, ("r03_traffic_configs4.json",))
    t_ms = elapsed / args.steps * 1e3
    out = {"workload": "configs[4] shard: %d streams/GPU x %d frames of 65536, FastFIR 2048/1025 + 65536-point spectrum" % (S, F),
           "streams_per_gpu": S, "streams_total": S * world, "samples_per_step_per_gpu": n, "ms_per_step": round(t_ms, 4), "settle_steps": settled,
           "Msamples_per_s": round(n * world / (t_ms * 1e-3) / 1e6, 1), "bytes_compulsory": 28 * n,
           "compulsory_GBps": round(28 * n / (t_ms * 1e-3) / 1e9, 1), "frac_of_peak_on_compulsory_bytes": round(28 * n / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "kernels": ks, "roofline": roof}
    sb.close()
    buf.free()
    return out


def pcie_inclusive(P, rx, n, device):
    """What the headline workload runs at when the host hands over pageable host buffers (PCIe both ways).  Never `value`."""
    x = P.binding.to_f32_iq(make_input(n, 1000))
    raw = np.clip(np.round(np.asarray(x).view(np.float32).ravel() * 128), -128, 127).astype(np.int8)
    dbuf, rbuf = P.DeviceBuffer(x.nbytes, device), P.DeviceBuffer(raw.nbytes, device)

    def best(f, k=3):
        b = 1e9
        for _ in range(k):
            t0 = time.perf_counter()
            f()
            b = min(b, time.perf_counter() - t0)
        return b

    def f_float():
        dbuf.upload(x)
        rx.process_device(dbuf.ptr, n)
        rx.audio()

    def f_raw():
        rbuf.upload(raw)
        rx.process_raw_device(rbuf.ptr, n, 0, 0, 1.0)
        rx.audio()

    f_float()
    f_raw()
    a, b = best(f_float), best(f_raw)
    # the same int8 batches through the library's pinned double buffer (pebblegpu_receiver_ingest_*): the upload of the next batch
    # crosses PCIe on a copy stream while this one computes and its audio is read.  (A device plugin writes its samples straight into
    # the slots; here both are filled once, outside the timed loop.)
    for slot in (0, 1):
        rx.ingest_buffer(slot, raw.nbytes)[:] = raw
    rx.ingest_submit(0, raw.nbytes)
    k_steps = 6

    def pipelined():
        for k in range(k_steps):
            s = k & 1
            rx.process_ingested(s, n, 0, 0, 1.0)
            rx.ingest_buffer(s ^ 1, raw.nbytes)   # (blocks until the other slot's last call is over: it is)
            rx.ingest_submit(s ^ 1, raw.nbytes)   # the next batch travels while this call computes
            rx.audio()
    pipelined()
    t0 = time.perf_counter()
    pipelined()
    c = (time.perf_counter() - t0) / k_steps
    rx.synchronize()
    dbuf.free()
    rbuf.free()
    return {"float2_in_audio_out": {"ms": round(a * 1e3, 3), "Msamples_per_s": round(n / a / 1e6, 1)},
            "int8_in_audio_out": {"ms": round(b * 1e3, 3), "Msamples_per_s": round(n / b / 1e6, 1)},
            "int8_pinned_double_buffered_audio_out": {"ms": round(c * 1e3, 3), "Msamples_per_s": round(n / c / 1e6, 1),
                                                      "how": "pebblegpu_receiver_ingest_acquire / _submit / process_ingested, two pinned slots, %d batches back to back" % k_steps},
            "note": "pageable host memory, hipMemcpy each way, spectra left on the device"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--superframes", type=int, default=256, help="super-frames (131072 samples) per step per GPU")
    ap.add_argument("--full", action="store_true",
                    help="also the un-settled rate, the spectrum kernel alone, the copy peak, socket power, the CPU baseline, the configs[2..4] "
                         "legs, the raw-int8 leg and the PCIe-inclusive rates (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's audio and a seeded sample of its spectrum rows to DIR/*.npy (float32; rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--headline-only", action="store_true", help="with --full: skip the configs[2..4] legs, the raw-int8 leg and the PCIe-inclusive rates")
    ap.add_argument("--control-plane-only", action="store_true",
                    help="CPU rehearsal of the N>1 launch path (rendezvous, barriers, max-over-ranks, aggregation, shard ranges): "
                         "the GPU step is replaced by a rank-dependent sleep; used by tests/test_multirank_gloo.py")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        import torch  # noqa: F401
        import torch.distributed as dist  # control plane only: barrier + max of a CPU scalar (gloo)
        dist.init_process_group(backend="gloo")
    assert world == args.gpus or world == 1, "launch one rank per GPU (torch.distributed.run --nproc-per-node N)"

    if args.control_plane_only:
        return control_plane_rehearsal(args, rank, world, dist)

    import pebblesdr_amd as P
    L = P.load_library()
    ndev = L.pebblegpu_device_count()
    if ndev <= 0:
        raise SystemExit("bench.py needs an MI355X: libpebblegpu has no CPU path")
    if ndev < world or local_rank >= ndev:
        # never two ranks on one GPU: that run would be labelled n_gpus = N while measuring something else
        sys.stderr.write("bench.py: %d ranks but only %d HIP device(s) visible; refusing to oversubscribe\n" % (world, ndev))
        sys.stderr.flush()
        os._exit(3)
    device = local_rank

    rx = P.ReceiverBank(FS, n_channels=1, shared_input=True, wfm=True, spectrum_bins=BINS,
                        max_superframes=args.superframes, device=device)
    rx.set_mixer(0, MIX_HZ)
    sf = rx.superframe
    n = args.superframes * sf
    x = make_input(n, 1000 * (rank + 1))
    dbuf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x), device)  # inputs resident in HBM before timing
    raw_leg = args.full and not args.headline_only and world == 1
    raw8 = np.clip(np.round(x.view(np.float32) * 128), -128, 127).astype(np.int8) if raw_leg else None  # the same samples as HackRF int8 pairs
    del x

    def barrier():
        P.binding.check(L, L.pebblegpu_device_synchronize(device))
        if dist is not None:
            dist.barrier()

    def step():
        rx.process_device(dbuf.ptr, n)  # queued on the library's stream; no host sync per step

    for _ in range(args.warmup):
        step()
    rx.synchronize()
    if args.full:
        # the K steps right behind the driver's W warm-ups, before any settling: what the flags alone measure (inside the clocks' ramp)
        elapsed_unsettled = timed_steps(step, barrier, args.steps, dist)
    settled = settle(step, rx.synchronize)  # untimed: the clocks' ramp after set-up is not the workload's rate
    if args.full:
        # untimed, for reference only: the dominant kernel alone on the device (per-kernel profiling keeps the whole call on one
        # stream); in the timed steps the chain's first, memory-bound kernel runs beside it on a second stream
        rx.set_profiling(True)
        for _ in range(3):
            rx.process_device(dbuf.ptr, n)
        rx.synchronize()
        alone_ms = rx.mean_ms(1, 3)
        alone = {w: rx.mean_ms(w, 3) for w in (2, 3, 5)}
        alone_names = {w: rx.kernel_name(w) for w in (2, 3, 5)}
        alone_spec_name = rx.kernel_name(1)  # (with nothing beside it the library launches the transform's all-registers variant)
        rx.set_profiling(False)
    # re-tuning resets the oscillator's phase (Mixer::setFrequency); after this untimed call the chain's state no longer depends
    # on how many steps settle() ran, so the timed steps compute the same from run to run
    rx.set_mixer(0, MIX_HZ)
    rx.process_device(dbuf.ptr, n)
    rx.synchronize()

    for _ in range(args.warmup):
        step()
    rx.synchronize()
    elapsed = timed_steps(step, barrier, args.steps, dist)
    # HIP events the library recorded on its stream around each kernel group of the timed steps (ring of 64 calls)
    k_ev = min(args.steps, 64)
    spec_ms = rx.mean_ms(1, k_ev)
    chain_ms = rx.mean_ms(0, k_ev) - spec_ms
    if args.dump_outputs and rank == 0:
        dump_outputs(rx, args.dump_outputs)

    extra, raw_line, pcie = {}, None, None
    if args.full and not args.headline_only:
        if world == 1:
            # the headline fed in the device's own sample format (2 B/sample in): normalizeIQ runs on the device
            rbuf = P.DeviceBuffer.from_array(raw8, device)
            settle(lambda: rx.process_raw_device(rbuf.ptr, n, 0, 0, 1.0), rx.synchronize)
            for _ in range(2):
                rx.process_raw_device(rbuf.ptr, n, 0, 0, 1.0)
            rx.synchronize()
            el = timed_steps(lambda: rx.process_raw_device(rbuf.ptr, n, 0, 0, 1.0), barrier, args.steps, dist)
            raw_line = {"entry": "pebblegpu_receiver_process_raw(PEBBLEGPU_IQ_S8)", "bytes_in_per_sample": 2,
                        "ms_per_step": round(el / args.steps * 1e3, 4), "Msamples_per_s": round(n * args.steps / el / 1e6, 1)}
            rbuf.free()
            pcie = pcie_inclusive(P, rx, n, device)
    del raw8
    rx_info = {"frames": n // NF}
    power = socket_power(step, rx.synchronize) if (args.full and rank == 0 and world == 1 and not args.headline_only) else None
    copy_gbps = None
    if args.full and rank == 0:
        try:
            copy_gbps = round(P.binding.probe_copy_gbps(16, 1 << 30, 10, device), 1)  # measured float4 streaming copy, read+write
        except Exception:
            copy_gbps = None
    rx.close()
    dbuf.free()
    if args.full and not args.headline_only:
        if world == 1:
            extra["configs[2]"] = run_bank(P, "configs[2]: 2.048 Msps shared stream -> 256 tuned USB channels, mixer + decimate + FastFIR 2048/1025 (300-3000 Hz), 8 super-frames per step",
                                           2_048_000, 256, [P.DM_USB], 8, rank, world, device, barrier, args, dist)
            extra["configs[2]"]["batch_sweep"] = bank_batch_sweep(P, 2_048_000, 256, [P.DM_USB], (8, 32, 128), device, max(5, args.steps // 2))
        extra["configs[3] shard"] = run_bank(P, "configs[3] shard: 100 Msps shared stream -> %d AM/USB channels per GPU (global channels [%d r, %d r + %d)), 1 super-frame (4 194 304 samples) per step"
                                             % (C3_PER_GPU, C3_PER_GPU, C3_PER_GPU, C3_PER_GPU), 100_000_000, C3_PER_GPU, [P.DM_AM, P.DM_USB], 1, rank, world, device, barrier, args, dist)
        extra["configs[4] shard"] = run_streambank(P, rank, world, device, barrier, args, dist)

    if rank == 0:
        frames = rx_info["frames"]
        algo_bytes = frames * (8 * NF + 4 * BINS)  # 8*N + 4*bins per frame
        achieved = algo_bytes / (spec_ms * 1e-3) / 1e9
        traffic, traffic_src = pmc_traffic(args.superframes)
        out = {
            "metric": "IQ Msamples/s through full ProcessBlock chain",
            "value": round(aggregate_msps(n * args.steps, world, elapsed), 2),
            "unit": "Msamples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "settle_steps": settled,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        }
        if args.full:
            out.update({
                "value_unsettled": round(aggregate_msps(n * args.steps, world, elapsed_unsettled), 2),
                "ms_per_step_unsettled": round(elapsed_unsettled / args.steps * 1e3, 4),
                "unsettled_note": "the same K steps timed right after the W warm-up steps, before the untimed settle phase (`value` is the settled rate)",
            })
        out.update({
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": "configs[1]: 20 Msps int8-shape IQ (values k/128, resident in HBM as float2), 1 channel/GPU, mixer+decimate(D=64)+WFM mono demod + 8192-bin SignalSpectrum per 2048-sample frame",
                       "samples_per_step_per_gpu": n, "frames_per_buffer": NF, "spectrum_bins": BINS,
                       "parallelism": "independent channel per GPU, no collectives"},
        })
        roof = {"bound": "hbm", "kernel": "k_spectrum_t128", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src}
        if args.full:
            roof.update({"measured_copy_peak_GBs": copy_gbps, "socket_power": power})
        roof.update({"algorithmic_bytes_per_launch": algo_bytes, "avg_launch_ms": round(spec_ms, 4),
                     "rest_of_chain_ms": round(chain_ms, 4),
                     "co_scheduled": "the chain runs on a second stream beside this kernel (its first stage needs no LDS)"})
        if args.full:
            roof.update({"avg_launch_ms_alone": round(float(alone_ms), 4), "kernel_alone": alone_spec_name,
                         "frac_alone": round(algo_bytes / (alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                         "chain_kernels_alone_ms": {alone_names[w]: round(alone[w], 4) for w in alone if alone_names[w]}})
        out["roofline"] = roof
        if "configs[2]" in extra:
            c2 = extra["configs[2]"]
            # the one single-GPU workload that runs the whole chain the metric names (mixer -> decimate -> FastFIR -> demod), lifted
            out["full_chain"] = {"workload": c2["workload"], "ms_per_step": c2["ms_per_step"], "channel_Msamples_per_s": c2["channel_Msamples_per_s"],
                                 "input_Msamples_per_s": c2["input_Msamples_per_s"], "roofline_kernel": c2["roofline"]["kernel"] if c2["roofline"] else None,
                                 "roofline_frac": c2["roofline"]["frac"] if c2["roofline"] else None,
                                 "frac_of_peak_on_compulsory_bytes": c2["frac_of_peak_on_compulsory_bytes"],
                                 "batch_sweep": c2.get("batch_sweep")}
        if raw_line:
            out["raw_int8"] = raw_line
        if pcie:
            out["pcie_inclusive"] = pcie
        if extra:
            out["configs"] = extra
        if args.full and not args.no_cpu_baseline and world == 1:  # rank 0 at N = 1 only
            out["cpu_baseline"] = cpu_baseline(1, 8, "configs[1] (20 Msps WFM mono + 8192-bin spectrum per frame; one channel per thread, as one channel per GPU)")
            if not args.headline_only:
                for key, wl, what in (("configs[2]", 2, "the 256-channel bank"), ("configs[3] shard", 3, "the 512-channel shard, a 64-frame sample of its 2048-frame super-frame"),
                                      ("configs[4] shard", 4, "the 128-stream shard")):
                    if key in extra:
                        extra[key]["cpu_baseline"] = cpu_baseline(wl, 2.5, what)
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
