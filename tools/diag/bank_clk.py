"""Clock counts of k_mix_dec_mfma's waves on configs[2]'s geometry (PEBBLEGPU_BANK_CLK=1, read when a receiver is created, makes the
library print them for every launch of that receiver).  A receiver without it warms the device up first; the measured receiver's
first call runs inside the oscillators' start-up transient and takes the two-kernel route, so its three later calls report."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pebblesdr_amd as P  # noqa: E402

k = int(sys.argv[1]) if len(sys.argv) > 1 else 8
fs, C = (int(sys.argv[2]) if len(sys.argv) > 2 else 2048000), 256


def make():
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=k)
    for c in range(C):
        rx.set_mode(c, P.DM_USB); rx.set_mixer(c, (-0.45 + 0.9 * c / C) * fs); rx.set_bandpass(c, 300, 3000)
    return rx


os.environ["PEBBLEGPU_BANK_CLK"] = "0"
warm = make()
os.environ["PEBBLEGPU_BANK_CLK"] = "1"
rx = make()
n = k * rx.superframe
rng = np.random.default_rng(1)
x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.05).astype(np.complex64)
buf = P.DeviceBuffer.from_array(x.view(np.float32))
for _ in range(200):
    warm.process_device(buf.ptr, n)
warm.synchronize()
for _ in range(4):
    rx.process_device(buf.ptr, n)
rx.synchronize()
