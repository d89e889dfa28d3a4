"""The reference's MorseGen call sites (setParams, setTextOut, one generate per frame in place of the nextOutputSample loop) and
Receiver::setMorseStations compiled against include/pebblegpu_steps.hpp.  CPU tier: they compile and link.  GPU tier: the adapter's
frames are the C ABI's, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import morsegen_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pebblegpu_steps.hpp"
using namespace pebblegpu;

int main(int argc, char **argv)
{
    if (argc < 8) return 2;
    const double fs = std::atof(argv[2]), freq = std::atof(argv[3]), db = std::atof(argv[4]);
    const uint32_t wpm = (uint32_t)std::atoi(argv[5]), rise = (uint32_t)std::atoi(argv[6]);
    const int frames = std::atoi(argv[7]);
    std::vector<uint16_t> tokens;
    for (int i = 8; i < argc; i++) tokens.push_back((uint16_t)std::atoi(argv[i]));
    // MorseGenDevice's set-up order (morsegendevice.cpp: setParams, then setTextOut) and its generate() with one station
    MorseGen gen(fs);
    gen.setParams(freq, db, wpm, rise);
    gen.setTextOut(tokens);
    if (!gen.hasOutputSamples()) return 3;
    FILE *out = std::fopen(argv[1], "wb");
    if (!out) return 1;
    std::vector<CPX> frame(2048);
    for (int k = 0; k < frames; k++) {
        for (CPX &v : frame) v = CPX(0.25, -0.5);   // generate() adds to what is there
        gen.generate(frame.data(), 2048);
        std::fwrite(frame.data(), sizeof(CPX), frame.size(), out);
    }
    std::fclose(out);
    // the same station at the head of a receiver: accepted, and switched off again
    pebblegpu_morse_station st;
    std::memset(&st, 0, sizeof(st));
    st.struct_size = sizeof(st);
    st.wpm = wpm; st.ms_rise = rise; st.frequency_hz = freq; st.amplitude = 0.1;
    st.tokens = tokens.data(); st.n_tokens = (uint32_t)tokens.size();
    Receiver rx((uint32_t)fs, 2048, false, 0, [](CPX *, uint16_t) {});
    rx.setMorseStations(&st, 1);
    if (rx.lastStatus()) return 5;
    rx.setMorseStations(nullptr, 0);
    if (rx.lastStatus()) return 6;
    return gen.lastStatus() ? 4 : 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    d = tmp_path_factory.mktemp("morsegen_cpp")
    src, out = str(d / "morsegen_sites.cpp"), str(d / "morsegen_sites")
    with open(src, "w") as f:
        f.write(SRC)
    lib = os.path.join(ROOT, "pebblesdr_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lpebblegpu",
                           "-Wl,-rpath," + lib, "-o", out])
    return out


def test_morsegen_call_sites_compile(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_adapter_frames_equal_the_c_abi(exe, tmp_path, gpu_lib):
    import pebblesdr_amd as P
    fs, freq, db, wpm, rise, frames = 2048000.0, 101000.0, -26.0, 50, 5, 6
    toks = G.text_tokens("E T ")
    p = str(tmp_path / "out.bin")
    r = subprocess.run([exe, p, repr(fs), repr(freq), repr(db), str(wpm), str(rise), str(frames)] + [str(t) for t in toks], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(p, dtype=np.complex128)
    assert len(got) == frames * 2048
    g = P.SigGen(fs, 2048)
    g.set_morse([P.morse_station(freq, 10.0 ** (db / 20.0), wpm, rise, toks)], mix=True)
    want = np.concatenate([g.generate(np.full(2048, 0.25 - 0.5j, dtype=np.complex128)) for _ in range(frames)])
    g.close()
    assert np.array_equal(got, want)
    ref = G.station_sum(fs, [(freq, G.db_to_amplitude(db), wpm, rise, toks)], frames * 2048)[0]
    assert np.abs(ref).max() > 0.04 and np.sqrt(np.mean(np.abs(got - (0.25 - 0.5j) - ref) ** 2)) <= 1e-5 * np.sqrt(np.mean(np.abs(ref + 0.25 - 0.5j) ** 2))
