"""CPU tier of the test bench (generator + taps): the restatement's pins, the library's host-side sweep plan against them, the reference's
two call sites compiled against include/pebblegpu_steps.hpp, and a C host without a device."""
import os
import subprocess

import numpy as np
import pytest

from tests import testbench_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (fs, start, stop, rate) of the issue's three sweeps and their leg lengths
SWEEPS = [((20e6, -1e6, 1e6, 4e9), 10000), ((20e6, -1e6, 1e6, 300000001.0), 133334), ((2.048e6, -0.5e6, 0.7e6, 123456789.0), 19907)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd as P
    return P.load_library()


def test_pulse_timer_numbers():
    """the serial double sum decides the edges: 0.01 * 2.048e6 is 20480.0 exactly, and increment 20480 is the first ABOVE the width"""
    assert R.pulse_numbers(2.048e6, 0.01, 0.5) == (1024001, 20480)
    assert R.pulse_numbers(20e6, 0.01, 0.5) == (10000001, 200001)


@pytest.mark.parametrize("sw,leg", SWEEPS)
def test_leg_lengths(sw, leg):
    n, frac = R.leg_length(*sw)
    assert n == leg
    assert frac == 0.0 or 0.01 <= frac <= 0.99
    _, s = R.serial_sweep(sw[0], 3 * leg + 5, 2048, start=sw[1], stop=sw[2], rate=sw[3], sweep_type=R.REPEAT)
    assert s.resets == [leg, 2 * leg, 3 * leg]


def test_repeat_reverse_returns_to_the_start_frequency():
    fs, a, b, r = SWEEPS[2][0]
    leg = SWEEPS[2][1]
    s = R.SerialSweep(fs, a, b, r, sweep_type=R.REPEAT_REVERSE)
    s.gen(leg)
    assert (s.f, s.up, s.start, s.stop) == (b, False, b, a)   # swapped, running down from the old stop frequency
    s.gen(leg)
    assert (s.f, s.up, s.start, s.stop) == (a, True, a, b)
    assert s.resets == [leg, 2 * leg]


def test_single_holds_the_stop_frequency():
    fs, a, b, r = SWEEPS[0][0]     # rate / fs = 200 Hz per sample: every sum is exact
    s = R.SerialSweep(fs, a, b, r, sweep_type=R.SINGLE)
    s.gen(SWEEPS[0][1] + 4096)
    assert s.f == b and s.inc == 0.0 and s.resets == [SWEEPS[0][1]]
    x = s.gen(4096)
    d = np.angle(x[1:] * np.conj(x[:-1]))
    assert np.allclose(d, 2 * np.pi * b / fs, atol=1e-9)


def test_pulse_gates_the_restatement_at_the_pinned_samples():
    x, _ = R.serial_sweep(2.048e6, 1024001 + 30000, 2048, start=1000.0, stop=2000.0, rate=0.0, pulse_width=0.01, pulse_period=0.5)
    on = np.abs(x) > 0.5
    # samples 0 .. 20478 see increments 1 .. 20479 (timer <= width); the period's last sample sees the reset timer
    assert on[:20479].all() and not on[20479:1024000].any() and on[1024000] and on[1024001:1024001 + 20479].all() and not on[1024001 + 20479:].any()


def test_noise_restatement_shape():
    z, r, att = R.noise(1234, 0, 0, 1 << 16)
    assert (att < R.NOISE_ATTEMPTS).all() and 0.75 < (att == 0).mean() < 0.82       # pi / 4 of the attempts are accepted
    assert (r < 2 ** 31).all()
    z2, r2, _ = R.noise(1234, 0, 1000, 100)
    assert np.array_equal(z2, z[1000:1100]) and np.array_equal(r2, r[1000:1100])     # a sample's noise is a function of its number
    assert not np.array_equal(R.noise(1234, 1, 0, 100)[0], z[:100]) and not np.array_equal(R.noise(1235, 0, 0, 100)[0], z[:100])
    assert abs(z.real.var() - 1.0) < 0.03 and abs(z.imag.var() - 1.0) < 0.03


def test_library_plan_matches_the_restatement(lib):
    """pebblegpu_sweep_plan needs no device: the host side of the generator (leg length, the serial pulse timer) against the pins"""
    import pebblesdr_amd as P
    for (fs, a, b, r), leg in SWEEPS:
        assert P.sweep_plan(fs, P.sweep(a, b, r))[0] == leg
        assert P.sweep_plan(fs, P.sweep(b, a, r))[0] == leg   # downwards
    assert P.sweep_plan(2.048e6, P.sweep(0, 1, 0.0, pulse_width_s=0.01, pulse_period_s=0.5)) == (0, 1024001, 20479)
    assert P.sweep_plan(20e6, P.sweep(0, 1, 0.0, pulse_width_s=0.01, pulse_period_s=0.5)) == (0, 10000001, 200000)
    assert P.sweep_plan(2.048e6, P.sweep(0, 1e5, 1e6)) == (204800, 0, 0)
    with pytest.raises(P.PebbleGpuError) as e:
        P.sweep_plan(2.048e6, P.sweep(0, 10, 2.048e6))          # a leg of 10 samples
    assert e.value.code == -6
    with pytest.raises(P.PebbleGpuError) as e:
        P.sweep_plan(2.048e6, P.sweep(0, 10, 1.0, sweep_type=3))
    assert e.value.code == -1
    bad = P.sweep(0, 10, 1.0)
    bad.struct_size = 8
    with pytest.raises(P.PebbleGpuError) as e:
        P.sweep_plan(2.048e6, bad)
    assert e.value.code == -1


CALL_SITES = r'''
#include <vector>
#include "pebblegpu_steps.hpp"
using namespace pebblegpu;
struct Global { TestBench *testBench; } globalObj, *global = &globalObj;
// application/receiver.cpp:797-798 and :803, as written there
static void head_of_chain(int numSamples, CPX *nextStep, double m_sampleRate, Receiver &rx)
{
    global->testBench->genSweep(numSamples, nextStep);
    global->testBench->genNoise(numSamples, nextStep);
    (void)m_sampleRate; (void)rx;
}
int main()
{
    TestBench tb(2048000, 2048);
    global->testBench = &tb;
    tb.initSweep(-500000.0, 700000.0, 123456789.0, 0.01, 0.5, TestBench::REPEAT);
    tb.setNoise(0.001, 7);
    std::vector<CPX> frame(2048);
    Receiver rx(2048000, 2048, false, 0, [](CPX *, uint16_t) {});
    pebblegpu_sweep s = {};
    s.struct_size = sizeof(s);
    rx.setTestBenchSweep(&s);
    rx.setTestBenchNoise(0.0, 0);
    rx.setTaps(1u << PEBBLEGPU_TAP_MODEM, [](int, CPX *, double, int) {});
    head_of_chain(2048, frame.data(), 2048000.0, rx);
    return tb.lastStatus() == PEBBLEGPU_E_NO_DEVICE || tb.lastStatus() == 0 ? 0 : 1;
}
'''

C_HOST = r'''
#include <stdio.h>
#include <string.h>
#include "pebblegpu.h"
int main(void)
{
    pebblegpu_siggen *g = NULL;
    pebblegpu_sweep s;
    uint64_t leg = 0, period = 0, on = 0;
    int rc;
    memset(&s, 0, sizeof s);
    s.struct_size = sizeof s;
    s.sweep_type = 1; s.start_hz = -1e6; s.stop_hz = 1e6; s.rate_hz_per_s = 4e9; s.amplitude = 1.0; s.mix = 1;
    rc = pebblegpu_sweep_plan(20e6, &s, &leg, &period, &on);
    printf("plan %d %llu\n", rc, (unsigned long long)leg);
    rc = pebblegpu_siggen_create(0, 20e6, 2048, &g);
    printf("create %d devices %d\n", rc, pebblegpu_device_count());
    printf("null %d %d %d\n", pebblegpu_siggen_set_sweep(NULL, &s), pebblegpu_set_testbench_noise(NULL, 1.0, 1), pebblegpu_receiver_set_taps(NULL, 2));
    printf("tap %d\n", pebblegpu_receiver_tap(NULL, 1, NULL, NULL, NULL) == NULL);
    pebblegpu_siggen_destroy(g);
    return 0;
}
'''


def _compile(tmp_path, name, text, cxx):
    src = str(tmp_path / name)
    out = src.rsplit(".", 1)[0]
    with open(src, "w") as f:
        f.write(text)
    libdir = os.path.join(ROOT, "pebblesdr_amd")
    cmd = (["g++", "-std=c++14"] if cxx else ["gcc", "-std=c99"]) + ["-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lpebblegpu",
                                                                      "-Wl,-rpath," + libdir, "-o", out]
    subprocess.check_call(cmd)
    return out


def test_reference_call_sites_compile_and_run(lib, tmp_path):
    exe = _compile(tmp_path, "tb_sites.cpp", CALL_SITES, True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_c_host_without_a_device_gets_no_device(lib, tmp_path):
    exe = _compile(tmp_path, "tb_host.c", C_HOST, False)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict((ln.split()[0], ln.split()[1:]) for ln in r.stdout.splitlines())
    assert out["plan"] == ["0", "10000"]
    devices = int(out["create"][2])
    assert int(out["create"][0]) == (0 if devices > 0 else -2)
    assert out["null"] == ["-1", "-1", "-1"] and out["tap"] == ["1"]


def test_python_face_reports_no_device(lib):
    import pebblesdr_amd as P
    if lib.pebblegpu_device_count() > 0:
        g = P.SigGen(2048000)
        g.close()
        return
    with pytest.raises(P.PebbleGpuError) as e:
        P.SigGen(2048000)
    assert e.value.code == -2
