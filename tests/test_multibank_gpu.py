"""GPU tier (-m gpu): the multibank (pebblegpu_multibank_*), a bank's channels sharded across devices from one process.

The yardstick of every equality here is one plain ReceiverBank per shard -- created with that shard's channel count, tuned to that
shard's channels and fed the same calls -- and the comparison is np.array_equal, bit for bit: a shard IS that receiver (same kernels,
same shapes, same inputs), and two equal banks agree bit for bit (tests/test_morse_gpu.py relies on it too).  The single banks are held
to the oracle by the parity tests; the multibank inherits that through the equality.  Nothing is compared with one bank of all C
channels: a 40-channel bank and a 20-channel bank take different decimator kernels.

device_ids = [0, 0] puts two shards on one device: the rig for a one-GPU machine.  2.048 Msps, 2048-sample frames, max_superframes 2:
the super-frame is 65536 samples."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import morse_ref as M
from tests.signals import lcg_noise, tones

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, NF, MAX_SF, SF = 2048000, 2048, 2, 65536
CALLS = [1, 2, 2, 1, 2]
E_INVALID, E_SIZE = -1, -5


def centres(C):
    return [-800e3 + 1600e3 * (c + 0.5) / C for c in range(C)]


@functools.lru_cache(maxsize=None)
def shared_stream(C, n_sf):
    """a tone 1 kHz above every channel's centre over LCG noise, n_sf super-frames"""
    n = n_sf * SF
    x = tones(FS, n, [(0.5 / C, f + 1000.0, 0.1 * k) for k, f in enumerate(centres(C))]) + lcg_noise(n, 7 + C, 1e-3)
    x.setflags(write=False)
    return x


def tune(rx, fcs, mode, lo=300, hi=3000):
    for c, f in enumerate(fcs):
        rx.set_mode(c, mode)
        rx.set_mixer(c, f)
        rx.set_bandpass(c, lo, hi)


def make(P, C, devices, flags=0, shared=True, bins=0, mode=None):
    """the multibank and its yardsticks, tuned alike: (mb, [bank per shard], [(first, count)])"""
    mode = P.DM_USB if mode is None else mode
    mb = P.MultiBank(FS, C, devices, flags=flags, shared_input=shared, spectrum_bins=bins, frames_per_buffer=NF, max_superframes=MAX_SF)
    assert mb.superframe == SF
    plan = P.multibank_plan(C, len(devices))
    assert mb.ranges == plan and mb.devices == list(devices)
    fcs = centres(C)
    for c in range(C):
        mb.set_mode(c, mode)
        mb.set_mixer(c, fcs[c])
        mb.set_bandpass(c, 300, 3000)
    banks = []
    for g, (first, count) in enumerate(plan):
        b = P.ReceiverBank(FS, count, shared, False, bins if (g == 0 or not flags & P.MULTIBANK_SPECTRUM_SHARD0) else 0,
                           frames_per_buffer=NF, max_superframes=MAX_SF, device=devices[g])
        tune(b, fcs[first:first + count], mode)
        banks.append(b)
    return mb, banks, plan


def close_all(*things):
    for t in things:
        t.close()


def calls_of(x, sizes):
    pos = 0
    for k in sizes:
        yield x[..., pos * SF:(pos + k) * SF]
        pos += k


def bank_audio(banks, plan, seg, shared=True):
    return np.concatenate([b.process(seg if shared else seg[first:first + count])[0] for b, (first, count) in zip(banks, plan)], axis=0)


def run_shape(P, C, devices):
    mb, banks, plan = make(P, C, devices)
    x = shared_stream(C, sum(CALLS))
    for i, seg in enumerate(calls_of(x, CALLS)):
        got = mb.process(seg)
        want = bank_audio(banks, plan, seg)
        assert got.shape == (C, seg.shape[-1] // mb.D) and np.abs(want).max() > 0
        assert np.array_equal(got, want), (C, i)
    names = [(mb.shard(g).kernel_name(2), banks[g].kernel_name(2)) for g in range(len(plan))]
    print("C = %d on %s: front kernels %s, last_ms %.4f" % (C, devices, names, mb.last_ms()))
    for a, b in names:
        assert a == b and a
    close_all(mb, *banks)


@pytest.mark.parametrize("C", [2, 5, 40])
def test_shard_shapes(gpu_lib, C):
    """1 + 1 (the one-channel routes), 2 + 3 (uneven, the general kernels), 20 + 20 (the banks' front end, oscillators advanced on the
    device, two-stage calls): the audio of every channel equals the per-shard banks', and the shards ran the kernels those banks ran"""
    import pebblesdr_amd as P
    run_shape(P, C, [0, 0])


@pytest.mark.parametrize("flag", [False, True])
def test_spectrum_and_the_flag(gpu_lib, flag):
    import pebblesdr_amd as P
    C, bins = 4, 2048
    mb, banks, plan = make(P, C, [0, 0], flags=P.MULTIBANK_SPECTRUM_SHARD0 if flag else 0, bins=bins)
    assert mb.shard(0).bins == bins and mb.shard(1).bins == (0 if flag else bins)
    x = shared_stream(C, sum(CALLS))
    for i, seg in enumerate(calls_of(x, CALLS)):
        got = mb.process(seg)
        want, specs = [], []
        for b in banks:
            a, s = b.process(seg)
            want.append(a)
            specs.append(s)
        assert np.array_equal(got, np.concatenate(want, axis=0)), i
        s0 = mb.shard(0).spectrum()
        assert s0.shape == (1, seg.shape[-1] // NF, bins)
        assert np.array_equal(s0, specs[0]), i
        if not flag:
            assert np.array_equal(mb.shard(1).spectrum(), s0) and np.array_equal(specs[1], s0), i
        else:
            assert specs[1] is None
    close_all(mb, *banks)


def test_independent_streams(gpu_lib):
    """shared_input = 0: four streams, each shard is fed its two rows"""
    import pebblesdr_amd as P
    C = 4
    mb, banks, plan = make(P, C, [0, 0], shared=False)
    n = sum(CALLS) * SF
    x = np.stack([tones(FS, n, [(0.3, f + 1000.0 + 50.0 * c)]) + lcg_noise(n, 31 + c, 1e-3) for c, f in enumerate(centres(C))])
    rows = []
    for i, seg in enumerate(calls_of(x, CALLS)):
        got = mb.process(seg)
        assert np.array_equal(got, bank_audio(banks, plan, seg, shared=False)), i
        rows.append(got)
    a = np.concatenate(rows, axis=1)
    assert all(not np.array_equal(a[c], a[d]) for c in range(C) for d in range(c))  # (the streams really differ)
    close_all(mb, *banks)


def test_raw_and_ingest(gpu_lib):
    """int8 pairs: process_raw from device buffers equals the banks' process_raw_device; the same stream through the pinned slots,
    alternating over six calls, equals it too; a process_ingested on a slot nothing was submitted to is refused and harms nothing"""
    import pebblesdr_amd as P
    C, sizes = 5, [1, 2, 2, 1, 2, 1]
    x = shared_stream(C, sum(sizes))
    raw = np.stack([np.clip(np.round(x.real * 128), -128, 127), np.clip(np.round(x.imag * 128), -128, 127)], axis=-1).astype(np.int8)
    mb, banks, plan = make(P, C, [0, 0])
    want = []
    pos = 0
    for i, k in enumerate(sizes):
        seg = raw[pos * SF:(pos + k) * SF]
        pos += k
        buf = P.DeviceBuffer.from_array(seg, 0)
        mb.process_raw_device([buf.ptr, buf.ptr], k * SF, P.binding.IQ_S8)
        got = mb.audio()
        rows = []
        for b in banks:
            b.process_raw_device(buf.ptr, k * SF, P.binding.IQ_S8)
            rows.append(b.audio())
        buf.free()
        want.append(np.concatenate(rows, axis=0))
        assert np.abs(want[-1]).max() > 0 and np.array_equal(got, want[-1]), i
    close_all(mb, *banks)

    mb, unused, _ = make(P, C, [0, 0])  # a fresh multibank: the same stream again, from host memory
    close_all(*unused)
    for slot in (0, 1):
        with pytest.raises(P.PebbleGpuError) as e:
            mb.process_ingested(slot, SF, P.binding.IQ_S8)
        assert e.value.code == E_SIZE
    mb.ingest_buffer(1, 2 * SF)  # acquired, but nothing submitted
    with pytest.raises(P.PebbleGpuError) as e:
        mb.process_ingested(1, SF, P.binding.IQ_S8)
    assert e.value.code == E_SIZE
    pos = 0
    for i, k in enumerate(sizes):
        seg = raw[pos * SF:(pos + k) * SF]
        pos += k
        slot = i & 1
        h = mb.ingest_buffer(slot, seg.nbytes)
        h[:] = seg.ravel()
        mb.ingest_submit(slot, seg.nbytes)
        mb.process_ingested(slot, k * SF, P.binding.IQ_S8)
        if i == 0:  # the slot is in flight until it is acquired again
            for call in (lambda: mb.ingest_submit(slot, seg.nbytes), lambda: mb.process_ingested(slot, k * SF, P.binding.IQ_S8)):
                with pytest.raises(P.PebbleGpuError) as e:
                    call()
                assert e.value.code == E_INVALID
        assert np.array_equal(mb.audio(), want[i]), i
    mb.close()


def test_routing(gpu_lib):
    """setters routed by global channel between two calls, the same on the per-shard banks with local indices"""
    import pebblesdr_amd as P
    C = 6
    mb, banks, plan = make(P, C, [0, 0])
    fcs = centres(C)
    owner = {}
    for g, (first, count) in enumerate(plan):
        for c in range(count):
            owner[first + c] = (g, c)
    for ch in range(C):
        assert mb.locate(ch) == owner[ch]
    for ch in (C, C + 1, 2 ** 31):
        with pytest.raises(P.PebbleGpuError) as e:
            mb.locate(ch)
        assert e.value.code == E_INVALID
    x = shared_stream(C, sum(CALLS))
    for i, seg in enumerate(calls_of(x, CALLS)):
        if i == 2:
            mb.set_mixer(4, fcs[0] + 500.0)
            mb.set_mode(1, P.DM_AM)
            mb.set_bandpass(5, -3000, -300)
            mb.set_mode(5, P.DM_LSB)
            g, c = owner[4]
            banks[g].set_mixer(c, fcs[0] + 500.0)
            g, c = owner[1]
            banks[g].set_mode(c, P.DM_AM)
            g, c = owner[5]
            banks[g].set_bandpass(c, -3000, -300)
            banks[g].set_mode(c, P.DM_LSB)
        got = mb.process(seg)
        assert np.array_equal(got, bank_audio(banks, plan, seg)), i
    close_all(mb, *banks)


def test_morse_across_the_split(gpu_lib):
    """the modem on global channels 2 and 3 -- the last channel of shard 0 and the first of shard 1 -- both keyed at 25 WPM, 24 calls of
    two super-frames: events and status through the routed getters equal the per-shard banks'"""
    import pebblesdr_amd as P
    C, calls = 6, 24
    n = calls * 2 * SF
    fcs = [-960e3 + 7.5e3 * c for c in range(C)]
    x = lcg_noise(n, 21, 2e-4)
    for ch, text in ((2, "TEST"), (3, "CQ")):
        env = M.keying(text, 25, FS)[:n]
        x[:len(env)] += 0.002 * env * np.exp(2j * np.pi * (fcs[ch] + 1000.0) * np.arange(len(env)) / FS)
    mb = P.MultiBank(FS, C, [0, 0], frames_per_buffer=NF, max_superframes=MAX_SF)
    plan = P.multibank_plan(C, 2)
    assert plan == [(0, 3), (3, 3)]
    banks = [P.ReceiverBank(FS, count, True, False, 0, frames_per_buffer=NF, max_superframes=MAX_SF) for _, count in plan]
    for ch in range(C):
        g, c = ch // 3, ch % 3
        for rx, k in ((mb, ch), (banks[g], c)):
            rx.set_mixer(k, fcs[ch])
            rx.set_bandpass(k, 300, 3000)
            if ch in (2, 3):
                rx.set_morse(k, True)
            rx.set_mode(k, P.DM_CWU)  # after the enable: the modem follows the mode
    got = {2: [], 3: []}
    want = {2: [], 3: []}

    def ev(e):
        return [(int(r["sample"]), int(r["token"]), int(r["kind"])) for r in e]

    for i in range(calls):
        seg = x[i * 2 * SF:(i + 1) * 2 * SF]
        a = mb.process(seg)
        assert np.array_equal(a, bank_audio(banks, plan, seg)), i
        if i % 5 == 4 or i == calls - 1:
            for ch in (2, 3):
                got[ch] += ev(mb.morse_events(ch))
                want[ch] += ev(banks[ch // 3].morse_events(ch % 3))
    for ch in (2, 3):
        assert len(want[ch]) >= 1 and got[ch] == want[ch], (ch, got[ch], want[ch])
        assert mb.morse_status(ch) == banks[ch // 3].morse_status(ch % 3)
    with pytest.raises(P.PebbleGpuError):
        mb.morse_status(4)  # (its modem is off: refused as on a single bank)
    close_all(mb, *banks)


def test_refusals_and_teardown(gpu_lib):
    import pebblesdr_amd as P
    C = 5
    mb, banks, plan = make(P, C, [0, 0])
    x = shared_stream(C, sum(CALLS))
    buf = P.DeviceBuffer.from_array(P.binding.to_f32_iq(x[:2 * SF]), 0)
    for n in (SF + NF, SF - 1, 3 * SF):  # not whole super-frames; above max_superframes
        with pytest.raises(P.PebbleGpuError) as e:
            mb.process_device([buf.ptr, buf.ptr], n)
        assert e.value.code == E_SIZE, n
    with pytest.raises(P.PebbleGpuError) as e:
        mb.process_device([buf.ptr, 0], SF)  # a null entry
    assert e.value.code == E_INVALID
    # no shard had queued anything: the stream starts here for all of them
    for i, seg in enumerate(calls_of(x, CALLS[:3])):
        assert np.array_equal(mb.process(seg), bank_audio(banks, plan, seg)), i
    # destroy right behind a queued call, no synchronize in between
    mb.process_device([buf.ptr, buf.ptr], 2 * SF)
    mb.close()
    close_all(*banks)
    # a second multibank afterwards works
    mb, banks, plan = make(P, C, [0, 0])
    seg = x[:2 * SF]
    assert np.array_equal(mb.process(seg), bank_audio(banks, plan, seg))
    mb.process_device([buf.ptr, buf.ptr], SF)
    mb.synchronize()
    close_all(mb, *banks)
    buf.free()


def test_two_real_devices(gpu_lib):
    """the 20 + 20 case with the shards on devices 0 and 1, against single banks on device 0 and on device 1"""
    import pebblesdr_amd as P
    if gpu_lib.pebblegpu_device_count() < 2:
        pytest.skip("needs two devices")
    run_shape(P, 40, [0, 1])


def test_the_c_host(gpu_lib, tmp_path):
    """examples/multibank_host.c, one thread of plain C: default device list 0,0 -> exit status 0 and a checksum line per shard"""
    src, exe = os.path.join(ROOT, "examples", "multibank_host.c"), str(tmp_path / "multibank_host")
    lib = os.path.join(ROOT, "pebblesdr_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lpebblegpu", "-Wl,-rpath," + lib, "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "checksum" in ln]
    assert len(lines) == 2 and lines[0].startswith("shard 0") and lines[1].startswith("shard 1"), r.stdout
