"""DigitalModemInterface-shaped call sites (setSampleRate, setDemodMode, processBlock) and Receiver::setDigitalModem compiled against
include/pebblegpu_steps.hpp.  CPU tier: they compile and link.  GPU tier: they run end to end against the restatement."""
import os
import subprocess

import numpy as np
import pytest

from tests import morse_ref as M
from tests.signals import lcg_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include <vector>
#include "pebblegpu_steps.hpp"
using namespace pebblegpu;

// plugins/DigitalModemInterface's processing members, as the receiver calls them (receiver.cpp:653-654, :979-980, :1108)
struct DigitalModemInterface {
    virtual ~DigitalModemInterface() {}
    virtual void setSampleRate(int sampleRate, int sampleCount) = 0;
    virtual void setDemodMode(DemodMode mode) = 0;
    virtual CPX *processBlock(CPX *in) = 0;
};
struct MorsePlugin : DigitalModemInterface {
    Morse m;
    void setSampleRate(int r, int n) override { m.setSampleRate(r, n); }
    void setDemodMode(DemodMode d) override { m.setDemodMode(d); }
    CPX *processBlock(CPX *in) override { return m.processBlock(in); }
};

static void print(const char *who, const std::vector<MorseEvent> &ev)
{
    for (const MorseEvent &e : ev)
        std::printf("%s %llu %u %u %s\n", who, (unsigned long long)e.sample, e.token, e.kind, e.kind == PEBBLEGPU_MORSE_CHAR ? Morse::dotDash(e.token).c_str() : "_");
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const int rate = std::atoi(argv[2]), frame = std::atoi(argv[3]);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    std::vector<CPX> x;
    CPX v;
    while (std::fread(&v, sizeof(v), 1, f) == 1) x.push_back(v);
    std::fclose(f);
    MorsePlugin plugin;
    DigitalModemInterface *modem = &plugin;
    modem->setSampleRate(rate, frame);
    modem->setSampleRate(rate, frame);  // every powerOn calls it again: the same object, a fresh decoder
    modem->setDemodMode(dmCWU);
    for (size_t i = 0; i + frame <= x.size(); i += frame)
        if (modem->processBlock(&x[i]) != &x[i]) return 3;
    print("step", plugin.m.events());
    MorseReport r = plugin.m.getStatus();
    std::printf("status %d %d %d %u %u\n", r.wpm, r.above_range, r.below_range, r.modem_rate, r.samples_per_result);
    if (argc > 4) {  // a wideband stream through the Receiver adapter with the modem on
        const uint32_t fs = (uint32_t)std::atoi(argv[4]);
        std::vector<CPX> wide;
        f = std::fopen(argv[5], "rb");
        if (!f) return 1;
        while (std::fread(&v, sizeof(v), 1, f) == 1) wide.push_back(v);
        std::fclose(f);
        Receiver rx(fs, 2048, false, 0, [](CPX *, uint16_t) {});
        rx.mixerChanged(std::atoi(argv[6]));
        rx.filterChanged(300, 3000);
        rx.setMorse(true);
        rx.demodModeChanged(dmCWU);
        for (size_t i = 0; i + 2048 <= wide.size(); i += 2048) rx.processIQData(&wide[i], 2048);
        print("rx", rx.morseEvents());
        if (rx.lastStatus()) return 4;
    }
    return plugin.m.lastStatus() ? 4 : 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    d = tmp_path_factory.mktemp("morse_cpp")
    src, out = str(d / "morse_sites.cpp"), str(d / "morse_sites")
    with open(src, "w") as f:
        f.write(SRC)
    lib = os.path.join(ROOT, "pebblesdr_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lpebblegpu",
                           "-Wl,-rpath," + lib, "-o", out])
    return out


def test_modem_call_sites_compile(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_modem_call_sites_run_end_to_end(exe, tmp_path, oracle_mod):
    fs = 64000
    env = M.keying("CQ CQ", 20, fs)
    n = ((len(env) + 2047) // 2048) * 2048
    t = np.arange(n) / fs
    x = np.zeros(n, dtype=np.complex128)
    x[:len(env)] = 0.05 * env * np.exp(2j * np.pi * 1000 * t[:len(env)])
    x += lcg_noise(n, 61, 2e-3)
    p = str(tmp_path / "x.bin")
    x.tofile(p)
    # the receiver's input: 2.048 Msps, the keyed tone 1 kHz above a 100 kHz mixer frequency
    fw, fc = 2048000, 100000
    sf = 32 * 2048
    nw = ((int(2.2 * fw) + sf - 1) // sf) * sf
    tw = np.arange(nw) / fw
    envw = M.keying("CQ CQ", 20, fw)[:nw]
    w = lcg_noise(nw, 62, 2e-4)
    w[:len(envw)] += 0.01 * envw * np.exp(2j * np.pi * (fc + 1000) * tw[:len(envw)])
    pw = str(tmp_path / "w.bin")
    w.tofile(pw)
    r = subprocess.run([exe, p, str(fs), "2048", str(fw), pw, str(fc)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    ref = M.MorseRef(fs, 2048)
    ref.set_demod_mode(M.DM_CWU)
    for k in range(n // 2048):
        ref.process(x[k * 2048:(k + 1) * 2048])
    step = [(int(a[1]), int(a[2]), int(a[3])) for a in lines if a[0] == "step"]
    assert step == ref.events and len(step) > 0
    assert [a[4] for a in lines if a[0] == "step" and a[3] == "0"] == [M.morse_dotdash(a[2]) for a in lines if a[0] == "step" and a[3] == "0"]
    st = [a for a in lines if a[0] == "status"][0]
    assert [int(v) for v in st[1:]] == [ref.status()[k] for k in ("wpm", "above_range", "below_range", "modem_rate", "samples_per_result")]
    from tests.test_morse_gpu import ref_events
    rx = [(int(a[1]), int(a[2]), int(a[3])) for a in lines if a[0] == "rx"]
    assert rx == ref_events(oracle_mod, w, fw, float(fc)).events and len(rx) > 0
