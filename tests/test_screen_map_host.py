"""CPU tier of the screen mapping (FFT::mapFFTToScreen, pebblelib/fft.cpp:411-534).

The numpy restatement in tests/screen_map_ref.py is pinned on hand-worked answers for each quirk that decides an output, and
against a pixel-by-pixel loop on random cases (tests/test_screen_cases_host.py holds both to the oracle's serial loop, which the
mapscreen_* reference pins hold to the reference's compiled code); the C++ adapter is shown to take SignalSpectrum's call sites as written
(application/signalspectrum.cpp:58-59, 111, 146) by compiling them against include/pebblegpu_steps.hpp and linking libpebblegpu.so."""
import os
import subprocess

import numpy as np
import pytest

from tests import screen_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flat(fft=2048, value=-100.0):
    return np.full(fft, value)


def test_pixel_one_is_never_averaged_and_the_window_is_last_to_current():
    # 2048 bins at 1 bin/Hz over the whole spectrum, 512 pixels: 4 bins per pixel, pixel i reads bin 4 i
    db = flat()
    db[4], db[8] = -20.0, -40.0
    out = R.map_scalar(db, 2048, 2048.0, 120, 512, 0.0, -120.0, -1024, 1024)  # yScaleFactor = -1: y = -powerdB - 1
    # pixel 0: bin 0, direct: -100 -> 99
    # pixel 1: bin 4 with lastFftBin = 0, and the rule is lastFftBin > 0: direct, db[4] = -20 -> 19 (averaging [0, 4) would give 99)
    # pixel 2: bins [4, 8) -- the previous pixel's bin, not its own: 10 log10((1e-2 + 3e-10) / 4) = -26.02 -> -26 -> 25
    # pixel 3: bins [8, 12): 10 log10((1e-4 + 3e-10) / 4) = -46.02 -> -46 -> 45
    assert list(out[:5]) == [99, 19, 25, 45, 99]
    got, v, alt = R.map_fft_to_screen(db, 2048, 2048.0, 120, 512, 0.0, -120.0, -1024, 1024)
    assert np.array_equal(got, out)
    assert np.isnan(v[0]) and np.isnan(v[1]) and abs(v[2] - 10 * np.log10((1e-2 + 3e-10) / 4)) < 1e-12


def test_out_of_range_is_min_db_without_the_max_db_offset():
    # stop at the spectrum's low edge: binLow = -1024, binHigh = 0, 1024 bins on 1024 pixels (repeat branch), every bin negative
    out = R.map_scalar(flat(), 2048, 2048.0, 120, 1024, -10.0, -130.0, -2048, -1024)
    assert set(out.tolist()) == {119}  # powerdB = -120 (not -120 - maxdB = -110 -> 109): y = 120 - 1


def test_a_slightly_negative_float_bin_truncates_to_bin_zero():
    # binLow = -1025 + 1024 = -1, 100 bins on 400 pixels: pixelsPerBin = 4, pixel i reads (int)(-1 + i / 4.0f)
    db = flat()
    db[0] = -30.0
    out = R.map_scalar(db, 2048, 2048.0, 120, 400, 0.0, -120.0, -1025, -925)
    assert out[0] == 119          # bin -1: out of range
    assert list(out[1:8]) == [29] * 7  # -0.75 .. -0.25 and 0 .. 0.75 truncate to bin 0
    assert out[8] == 99           # bin 1


def test_start_freq_is_rounded_to_float_at_100_msps():
    # (float)-49999998 = -5e7 (spacing 4 there, tie to even); * (8192.0f / 1e8f) = -4096.0002 -> -4096: binLow 0.  Unrounded the
    # product is -4095.9998 -> -4095: binLow 1
    g = R.geometry(8192, 100e6, -49999998, 49999998, 1024)
    assert g["bin_low"] == 0
    assert int(np.trunc(-49999998 * np.float64(np.float32(8192) / np.float32(100e6)))) + 4096 == 1


def test_quint16_span_wraps_like_x86_64():
    assert R.zoom_edges(48000, 1.0) == (-24000, 24000)
    assert R.zoom_edges(48000, 1.0, 500) == (-24500, 23500)
    assert R.zoom_edges(48000, 1.5) == (-3232, 3232)          # 72000 & 0xffff = 6464
    assert R.zoom_edges(48000, 1.5, 500) == (-3732, 2732)
    assert R.zoom_edges(48000, 1e6) == (0, 0)                 # 4.8e10 overflows int32: INT_MIN, low 16 bits 0
    assert R.zoom_edges(65535, 1.0) == (-32767, 32767)        # -span/2 truncates toward zero


def test_waterfall_height_255():
    # yScaleFactor = (float)(-255 / 120.0) = -2.125; y = (int)(-2.125 * powerdB - 1), bounded to 0..254
    assert float(R.y_scale(255, 0.0, -120.0)) == -2.125
    assert int(R.to_y(np.int32(-50), R.y_scale(255, 0.0, -120.0), 255)) == 105   # 105.25
    assert int(R.to_y(np.int32(-120), R.y_scale(255, 0.0, -120.0), 255)) == 254  # 254 -> yPixels - 1
    assert int(R.to_y(np.int32(0), R.y_scale(255, 0.0, -120.0), 255)) == 0       # -1 -> 0
    db = flat(4096, -50.0)
    assert set(R.map_scalar(db, 4096, 4096.0, 255, 400, 0.0, -120.0, -100, 100).tolist()) == {105}  # repeat branch: direct reads
    # averaged, 10 log10 of the mean of equal powers lands within an ulp of -50, on either side: the parity bar's exception
    _, v, alt = R.map_fft_to_screen(db, 4096, 4096.0, 255, 64, 0.0, -120.0, -2048, 2048)
    a = ~np.isnan(v)
    assert a.sum() == 62 and np.all(np.abs(v[a] + 50.0) < 1e-12)


def test_start_above_stop_and_empty_ranges_follow_the_reference():
    db = np.linspace(-110, -10, 2048)
    for start, stop in [(500, -500), (0, 0), (5000, 6000), (-9000, -8000)]:
        a = R.map_scalar(db, 2048, 2048.0, 255, 37, 0.0, -120.0, start, stop)
        b, _, _ = R.map_fft_to_screen(db, 2048, 2048.0, 255, 37, 0.0, -120.0, start, stop)
        assert np.array_equal(a, b), (start, stop)


@pytest.mark.parametrize("seed", range(6))
def test_vectorised_restatement_matches_the_pixel_loop(seed):
    rng = np.random.default_rng(seed)
    fft = int(rng.choice([2048, 4096]))
    fs = float(rng.choice([2048e3, 10e6, 100e6, 62500.0]))
    db = rng.uniform(-120, 0, fft)
    for _ in range(8):
        xp = int(rng.choice([1, 7, 100, 333, 1024, 3000]))
        span = float(rng.uniform(0.05, 1.5)) * fs
        ctr = float(rng.uniform(-0.4, 0.4)) * fs
        start, stop = int(ctr - span / 2), int(ctr + span / 2)
        yp = int(rng.choice([255, 600]))
        mx = float(rng.choice([0.0, -10.0]))
        a = R.map_scalar(db, fft, fs, yp, xp, mx, -120.0, start, stop)
        b, _, _ = R.map_fft_to_screen(db, fft, fs, yp, xp, mx, -120.0, start, stop)
        assert np.array_equal(a, b), (fft, fs, xp, start, stop)


# the reference's call sites, as written in application/signalspectrum.cpp (58-59, 111, 146), against the adapter
CALL_SITES = r"""
#include <cstdio>
#include "pebblegpu_steps.hpp"
using namespace pebblegpu;
using qint32 = int32_t;
using quint32 = uint32_t;
struct DB { static constexpr double maxDb = 0.0; };

struct SignalSpectrumShape {
    FFT *m_fftUnprocessed = new FFT();
    quint32 m_numSpectrumBins = 4096, sampleRate = 2048000;
    int numSamples = 2048;
    double *m_unprocessedSpectrum = new double[4096]();
    bool m_isOverload = false;
    ~SignalSpectrumShape() { delete m_fftUnprocessed; delete[] m_unprocessedSpectrum; }
    void setSampleRate()
    {
        m_fftUnprocessed->fftParams(m_numSpectrumBins, DB::maxDb, sampleRate, numSamples, WindowFunction::BLACKMANHARRIS);
    }
    void makeSpectrum(FFT *fft, CPX *in, double *sOut, int _numSamples)
    {
        m_isOverload = fft->fftSpectrum(in, sOut, _numSamples);
    }
    bool mapFFTToScreen(qint32 maxHeight, qint32 maxWidth, double maxdB, double mindB, qint32 startFreq, qint32 stopFreq, qint32 *outBuf)
    {
        if (m_fftUnprocessed!=NULL)
            return m_fftUnprocessed->mapFFTToScreen(m_unprocessedSpectrum, maxHeight,maxWidth,maxdB,mindB,startFreq,stopFreq,outBuf);
        else
            return false;
    }
};

int main()
{
    SignalSpectrumShape s;
    s.setSampleRate();
    const int bh = s.m_fftUnprocessed->lastStatus();
    FFT other;
    other.fftParams(4096, DB::maxDb, 2048000, 2048, WindowFunction::HANNING);
    qint32 px[16];
    const bool r = other.mapFFTToScreen(nullptr, 255, 16, 0.0, -120.0, -1024000, 1024000, px);  // no handle: false, nothing written
    std::printf("%d %d %d %d %d\n", bh, other.lastStatus(), other.getFFTSize(), (int)r, (int)WindowFunction::BLACKMANHARRIS);
    return 0;
}
"""


def test_signal_spectrum_call_sites_compile_against_the_adapter(tmp_path):
    import __graft_entry__ as g
    lib = g.build()
    src, exe = tmp_path / "call_sites.cpp", tmp_path / "call_sites"
    src.write_text(CALL_SITES)
    libdir = os.path.dirname(lib)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir,
                           "-lpebblegpu", "-Wl,-rpath," + libdir, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    bh, other, size, ret, code = map(int, r.stdout.split())
    assert bh in (0, -2)       # created (a device is visible) or PEBBLEGPU_E_NO_DEVICE: never E_UNSUPPORTED
    assert other == -6         # PEBBLEGPU_E_UNSUPPORTED, no handle
    assert size == 0 and ret == 0
    assert code == 12          # windowfunction.h:10-11
