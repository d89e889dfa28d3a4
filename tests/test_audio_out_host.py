"""CPU tier: the host twins of the two egress kernels (pebblegpu_audio_out_convert, pebblegpu_iq_record_convert) against the reference's
sample rules written out here in numpy, the argument refusals that need no device, and that the plain-C host example compiles and links.

The twins run the same inline functions the kernels run (pebblesdr_amd/csrc/egress.h); tests/test_audio_out_gpu.py holds the kernels to
the twins bit for bit.

Audio::SendToOutput, pebblelib/audiopa.cpp:304-343 (CPX is complex<double>, gain a float, maxOutput a float 0.9999):
    out[i] *= (gain / 100);  temp = out[i].real();  if (temp > maxOutput) temp = maxOutput; else if (temp < -maxOutput) temp = -maxOutput;
WavFile::WriteSamples, pebblelib/wavfile.cpp:386-388 (pcmData.left is a qint16):
    pcmData.left = buf[i].real() * 32767;
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
F32 = np.float32
MAXOUT = F32(0.9999)
GAINS = [0.0, 37.0, 100.0, 250.0]


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd
    return pebblesdr_amd


def rule_clip(a, gain):
    """audiopa.cpp:323-330 on float32 samples: the product in double, narrowed to float, clipped in float"""
    g = F32(gain) / F32(100)
    t = (np.asarray(a, dtype=F32).astype(np.float64) * np.float64(g)).astype(F32)
    return np.where(t > MAXOUT, MAXOUT, np.where(t < -MAXOUT, -MAXOUT, t)).astype(F32)


def rule_s16(t):
    """wavfile.cpp:387-388: double product, truncating conversion"""
    return np.trunc(np.asarray(t, dtype=F32).astype(np.float64) * 32767.0).astype(np.int16)


def rule_record(v):
    """the same conversion on unclipped samples; saturating where the reference's is undefined, NaN -> 0"""
    d = np.asarray(v, dtype=F32).astype(np.float64) * 32767.0
    d = np.where(np.isnan(d), 0.0, np.clip(d, -32767.0, 32767.0))
    return np.trunc(d).astype(np.int16)


def ulps(v, k):
    """v moved k float32 steps (k < 0: towards -inf)"""
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf) if k > 0 else F32(-np.inf))
    return v


def s16_edges():
    """nextafter(float32(k / 32767), 0) and its neighbour above, for a spread of k: where an fp32 product rounds up to k and a double one does not"""
    ks = np.concatenate([np.arange(1, 40), np.arange(1000, 33000, 997), np.arange(32700, 32767)])
    v = (ks.astype(np.float64) / 32767.0).astype(F32)
    below = np.nextafter(v, F32(0))
    return np.concatenate([below, np.nextafter(below, F32(1)), v, np.nextafter(v, F32(1)), -below, -v, -np.nextafter(v, F32(1))]).astype(F32)


def audio_inputs(gain):
    vals = [0.0, -0.0, 1.0, -1.0, 0.5, 3.0, -7.5, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754944e-38, 1e30, -1e30]
    g = F32(gain) / F32(100)
    if g > 0:  # samples whose product lands at, one ulp inside and one ulp outside +-0.9999f (and a few steps around)
        base = F32(MAXOUT / g)
        for k in range(-4, 5):
            vals += [ulps(base, k), -ulps(base, k)]
    for k in (-1, 0, 1):
        vals += [ulps(MAXOUT, k), -ulps(MAXOUT, k)]
    rng = np.random.default_rng(5)
    a = np.concatenate([np.asarray(vals, dtype=F32), s16_edges(), rng.uniform(-1.5, 1.5, 4001).astype(F32)])
    if len(a) % 2:
        a = a[:-1]
    return a.reshape(-1, 2)  # (L, R) pairs; odd and even positions both carry every kind of value after the shuffle below


@pytest.mark.parametrize("gain", GAINS)
def test_audio_twin_follows_the_reference_rule(P, gain):
    lr = audio_inputs(gain)
    lr = np.concatenate([lr, lr[:, ::-1]])
    want = rule_clip(lr, gain)
    got = P.audio_out_convert(P.AUDIO_F32, gain, False, lr)
    assert got.dtype == np.float32 and got.shape == lr.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))  # bit for bit, the sign of zero included
    if gain >= 100.0:
        assert (np.abs(want) == MAXOUT).any() and (np.abs(want) < MAXOUT).any()
    s = P.audio_out_convert(P.AUDIO_S16, gain, False, lr)
    assert s.dtype == np.int16 and np.array_equal(s, rule_s16(want))
    m = P.audio_out_convert(P.AUDIO_S16_MONO, gain, False, lr)
    assert m.shape == (len(lr),) and np.array_equal(m, rule_s16(want[:, 0]))
    assert np.abs(s.astype(np.int32)).max() <= 32763  # trunc(0.9999f * 32767)
    for fmt in (P.AUDIO_F32, P.AUDIO_S16, P.AUDIO_S16_MONO):
        z = P.audio_out_convert(fmt, gain, True, lr)
        assert not z.any()


def test_the_s16_edges_are_the_ones_fp32_gets_wrong(P):
    """the inputs really exercise the double product: a float32 multiply truncates differently on some of them"""
    v = s16_edges()
    want = rule_s16(rule_clip(v, 100.0))
    fp32 = np.trunc((rule_clip(v, 100.0) * F32(32767)).astype(np.float64)).astype(np.int16)
    assert (fp32 != want).any()
    got = P.audio_out_convert(P.AUDIO_S16_MONO, 100.0, False, np.stack([v, v], axis=1))
    assert np.array_equal(got, want)


def test_record_twin(P):
    v = np.concatenate([np.asarray([1.0, -1.0, 1.5, -1.5, np.nan, 0.0, -0.0, 1e-45, 1.00001, -1.00001, 32768.0 / 32767.0, -32768.0 / 32767.0,
                                    np.inf, -np.inf, 1e30], dtype=F32), s16_edges(), np.random.default_rng(6).uniform(-1.2, 1.2, 3000).astype(F32)])
    if len(v) % 2:
        v = v[:-1]
    iq = v.reshape(-1, 2)
    got = P.iq_record_convert(iq)
    assert got.dtype == np.int16 and got.shape == iq.shape
    assert np.array_equal(got, rule_record(iq))
    head = P.iq_record_convert(np.asarray([[1.0, -1.0], [1.5, -1.5], [np.nan, 0.25]], dtype=F32))
    assert head.tolist() == [[32767, -32767], [32767, -32767], [0, 8191]]
    c = (0.25 - 0.5j) * np.ones(3, dtype=np.complex64)
    assert P.iq_record_convert(c).tolist() == [[8191, -16383]] * 3


def test_refusals_without_a_device(P):
    L = P.load_library()
    lr = np.zeros((4, 2), dtype=F32)
    for bad in (lambda: P.audio_out_convert(3, 100.0, False, lr), lambda: P.audio_out_convert(-1, 100.0, False, lr),
                lambda: P.audio_out_convert(P.AUDIO_F32, -1.0, False, lr), lambda: P.audio_out_convert(P.AUDIO_F32, float("nan"), False, lr),
                lambda: P.audio_out_convert(P.AUDIO_F32, float("inf"), False, lr)):
        with pytest.raises(P.PebbleGpuError) as e:
            bad()
        assert e.value.code == E_INVALID
    blk = P.AudioBlock()
    blk.struct_size = C.sizeof(P.AudioBlock)
    n = C.c_uint64()
    assert C.sizeof(P.AudioBlock) == 48
    assert L.pebblegpu_receiver_audio_out_open(None, 0, None, 0, 4) == E_INVALID
    assert L.pebblegpu_receiver_audio_out_close(None) == E_INVALID
    assert L.pebblegpu_set_audio_level(None, 0, 100.0, 0) == E_INVALID
    assert L.pebblegpu_receiver_audio_out_next(None, 0, C.byref(blk)) == E_INVALID
    assert L.pebblegpu_receiver_audio_out_release(None, 0) == E_INVALID
    assert L.pebblegpu_receiver_audio_out_dropped(None, C.byref(n)) == E_INVALID
    assert L.pebblegpu_receiver_record_open(None, 4) == E_INVALID
    assert L.pebblegpu_receiver_record_close(None) == E_INVALID
    assert L.pebblegpu_receiver_record_next(None, 0, C.byref(blk)) == E_INVALID
    assert L.pebblegpu_receiver_record_release(None, 0) == E_INVALID
    assert L.pebblegpu_audio_out_convert(0, 100.0, 0, None, 4, None) == E_INVALID
    assert L.pebblegpu_iq_record_convert(None, 4, None) == E_INVALID
    assert L.pebblegpu_iq_record_convert(None, 0, None) == 0  # nothing to convert


def test_c_host_example_compiles_and_links(P, tmp_path):
    """compile and link only: running it needs a device"""
    src, exe = os.path.join(ROOT, "examples", "audio_out_host.c"), str(tmp_path / "audio_out_host")
    libdir = os.path.join(ROOT, "pebblesdr_amd")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lpebblegpu", "-Wl,-rpath," + libdir,
                        "-lm", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(exe)
