"""CPU tier: host logic that needs no device -- input generators, sharding arithmetic, bench JSON contract."""
import json
import os
import subprocess
import sys

import numpy as np

from tests.signals import lcg_noise, lcg_uniform, tones

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lcg_matches_scalar_recurrence():
    s, want = 7, []
    for _ in range(10000):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        want.append(s / 2 ** 32)
    assert np.array_equal(lcg_uniform(10000, 7), np.array(want))
    z = lcg_noise(5, 3, 2.0)
    u = lcg_uniform(10, 3)
    assert np.allclose(z, 2.0 * ((u[0::2] - 0.5) + 1j * (u[1::2] - 0.5)))


def test_tones_phase_continuity():
    a = tones(1e6, 100, [(1.0, 12345.0)])
    b = tones(1e6, 50, [(1.0, 12345.0)], n0=50)
    assert np.allclose(a[50:], b)


def test_bench_shard_arithmetic():
    sys.path.insert(0, ROOT)
    import bench
    # weak scaling: every rank owns its own stream(s); nothing is exchanged
    for world in (1, 2, 4, 8):
        shards = [bench.shard_streams(world, r, per_rank=1) for r in range(world)]
        flat = [s for sh in shards for s in sh]
        assert flat == list(range(world))
    assert bench.aggregate_msps(samples_per_rank=10_000_000, world=4, seconds=0.5) == 80.0


def test_scan_transition_powers_of_a_pole_at_one_minus_2e_6(tmp_path):
    """design::m2_pow feeds the scan kernels their transition powers M^(8 * 2^k).  For DCRemoval's 10 Hz high-pass at 20 Msps (poles at
    1 - 2e-6) M^256 is [[257, -256], [256, -255]] minus terms of 1e-3, and the scan multiplies direct-form-2 states of 5e8 by it: 8e-10 in
    an entry (what squaring in double leaves) is 4e-7 of drift in the filter's output, 0.25 dB at the DC bins
    (test_conditioners_gpu.test_dc_removal_at_20_msps_on_the_wfm_receiver).  Against exact rational powers of the same double
    coefficients the entries must hold 2e-12: one rounding of 256 is 3e-14, long double squaring measures 6.5e-13, double 7.6e-10."""
    from fractions import Fraction
    src = tmp_path / "m2.cpp"
    src.write_text('#include <cstdio>\n#include "design.h"\nint main() {\n'
                   '    const pg::design::Biquad h = pg::design::biquad_highpass(10, 0.7071, 20e6);\n'
                   '    const pg::design::M2 p = pg::design::m2_pow(pg::design::M2{-h.a1, -h.a2, 1.0, 0.0}, 256);\n'
                   '    std::printf("%a %a %a %a %a %a\\n", h.a1, h.a2, p.a, p.b, p.c, p.d);\n    return 0;\n}\n')
    csrc = os.path.join(ROOT, "pebblesdr_amd", "csrc")
    exe = str(tmp_path / "m2")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + csrc, str(src), os.path.join(csrc, "design.cpp"), "-o", exe])
    a1, a2, *got = [float.fromhex(v) for v in subprocess.check_output([exe], text=True).split()]
    m = [[Fraction(-a1), Fraction(-a2)], [Fraction(1), Fraction(0)]]
    for _ in range(8):
        m = [[m[0][0] * m[0][0] + m[0][1] * m[1][0], m[0][0] * m[0][1] + m[0][1] * m[1][1]],
             [m[1][0] * m[0][0] + m[1][1] * m[1][0], m[1][0] * m[0][1] + m[1][1] * m[1][1]]]
    err = max(abs(float(Fraction(g) - w)) for g, w in zip(got, (m[0][0], m[0][1], m[1][0], m[1][1])))
    print("m2_pow(M, 256) against exact: %.3e" % err)
    assert err <= 2e-12
