"""bench.py's command line: what a plain run prints, and what --dump-outputs writes (CPU: the file layout; GPU: two runs with the
same arguments write the same outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeReceiver:
    """audio() / spectrum() of a ReceiverBank, host arrays only"""

    def __init__(self, n_audio, frames, bins):
        rng = np.random.default_rng(5)
        self.a = (rng.standard_normal((1, n_audio)) + 1j * rng.standard_normal((1, n_audio))).astype(np.complex64)
        self.s = rng.standard_normal((1, frames, bins)).astype(np.float32)

    def audio(self):
        return self.a.copy()

    def spectrum(self):
        return self.s.copy()


def test_dump_outputs_layout(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    rx = _FakeReceiver(300, 2000, 64)
    bench.dump_outputs(rx, str(tmp_path / "a"))
    bench.dump_outputs(rx, str(tmp_path / "b"))
    a = np.load(tmp_path / "a" / "audio.npy")
    s = np.load(tmp_path / "a" / "spectrum_sample.npy")
    assert a.dtype == np.float32 and a.shape == (1, 300, 2)
    assert np.array_equal(a[..., 0] + 1j * a[..., 1], rx.a)
    assert s.dtype == np.float32 and s.shape == (1, bench.DUMP_SPECTRUM_ROWS, 64)
    # a fixed sample: the same rows every time, in order, each one a row of the call's spectrum
    pick = np.sort(np.random.default_rng(0).choice(2000, bench.DUMP_SPECTRUM_ROWS, replace=False))
    assert np.array_equal(s, rx.s[:, pick])
    assert np.array_equal(s, np.load(tmp_path / "b" / "spectrum_sample.npy"))
    # calls with no more rows than the sample: all of them
    small = _FakeReceiver(10, 100, 64)
    bench.dump_outputs(small, str(tmp_path / "c"))
    assert np.array_equal(np.load(tmp_path / "c" / "spectrum_sample.npy"), small.s)
    # the default geometry (256 super-frames: 524 288 audio samples, 16 384 rows of 8192 bins) stays well under 64 MB
    total = 1 * (256 * 131072 // 64) * 2 * 4 + 1 * bench.DUMP_SPECTRUM_ROWS * bench.BINS * 4
    assert total <= 32 << 20


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--superframes", "16", "--dump-outputs", str(tmp_path / run)],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["ms_per_step"] > 0 and d["value"] > 0
        assert abs(d["value"] - 16 * 131072 / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * d["value"]
        for key in ("configs", "raw_int8", "pcie_inclusive", "cpu_baseline", "value_unsettled"):
            assert key not in d  # --full only
    for name, shape in (("audio.npy", (1, 16 * 131072 // 64, 2)), ("spectrum_sample.npy", (1, 512, 8192))):
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype == np.float32 and x.shape == shape, (name, x.dtype, x.shape)
        assert np.isfinite(x).all() and np.abs(x).max() > 0
        assert np.array_equal(x, y), name
