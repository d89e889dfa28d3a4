"""CPU tier: what of the multibank (pebblegpu_multibank_*, include/pebblegpu.h) needs no device -- the partition rule, the argument
checks create makes before it touches a device, and that the plain-C host example compiles and links against the built library."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd as P
    return P.load_library()


def plan(L, c, g):
    first, count = (C.c_uint32 * 16)(), (C.c_uint32 * 16)()
    rc = L.pebblegpu_multibank_plan(c, g, first, count)
    return rc, [(int(first[i]), int(count[i])) for i in range(min(g, 16))]


def test_plan_is_the_integer_rule(lib):
    import pebblesdr_amd as P
    assert plan(lib, 4096, 8) == (0, [(512 * g, 512) for g in range(8)])
    assert plan(lib, 5, 2) == (0, [(0, 2), (2, 3)])
    assert plan(lib, 16, 16) == (0, [(g, 1) for g in range(16)])
    assert P.multibank_plan(5, 2) == [(0, 2), (2, 3)]
    for g in range(1, 17):
        for c in range(g, 41):
            rc, r = plan(lib, c, g)
            assert rc == 0 and len(r) == g
            assert r == [(k * c // g, (k + 1) * c // g - k * c // g) for k in range(g)], (c, g)
            pos = 0
            for first, count in r:  # contiguous, none empty, covering [0, C)
                assert first == pos and count >= 1, (c, g, r)
                pos += count
            assert pos == c


def test_plan_refusals(lib):
    first, count = (C.c_uint32 * 16)(), (C.c_uint32 * 16)()
    assert lib.pebblegpu_multibank_plan(8, 2, None, count) == E_INVALID
    assert lib.pebblegpu_multibank_plan(8, 2, first, None) == E_INVALID
    assert lib.pebblegpu_multibank_plan(8, 0, first, count) == E_INVALID
    assert lib.pebblegpu_multibank_plan(32, 17, first, count) == E_INVALID
    assert lib.pebblegpu_multibank_plan(3, 4, first, count) == E_INVALID
    assert lib.pebblegpu_last_error()


def config(n_channels=8):
    from pebblesdr_amd.binding import Config
    cfg = Config()
    cfg.struct_size = C.sizeof(Config)
    cfg.sample_rate = 2048000.0
    cfg.frames_per_buffer = 2048
    cfg.n_channels = n_channels
    cfg.shared_input = 1
    cfg.max_superframes = 2
    return cfg


def test_create_checks_its_arguments_before_any_device(lib):
    """every PEBBLEGPU_E_INVALID case is decided without a device: -1 here, where none exists (-2 would mean the probe came first)"""
    ids = (C.c_int32 * 17)(*([0] * 17))
    h = C.c_void_p()
    cfg = config()
    create = lib.pebblegpu_multibank_create
    assert create(None, ids, 2, 0, C.byref(h)) == E_INVALID
    assert create(C.byref(cfg), None, 2, 0, C.byref(h)) == E_INVALID
    assert create(C.byref(cfg), ids, 2, 0, None) == E_INVALID
    bad = config()
    bad.struct_size -= 4
    assert create(C.byref(bad), ids, 2, 0, C.byref(h)) == E_INVALID
    assert create(C.byref(cfg), ids, 0, 0, C.byref(h)) == E_INVALID
    big = config(64)
    assert create(C.byref(big), ids, 17, 0, C.byref(h)) == E_INVALID
    assert create(C.byref(cfg), ids, 9, 0, C.byref(h)) == E_INVALID   # 8 channels, 9 shards
    assert create(C.byref(cfg), ids, 2, 2, C.byref(h)) == E_INVALID   # unknown flag bit
    assert create(C.byref(cfg), ids, 2, 0x80000001, C.byref(h)) == E_INVALID
    assert not h.value
    # the other entry points refuse a null handle
    n = C.c_uint32()
    assert lib.pebblegpu_multibank_shards(None, C.byref(n)) == E_INVALID
    assert lib.pebblegpu_multibank_locate(None, 0, C.byref(n), C.byref(n)) == E_INVALID
    assert lib.pebblegpu_multibank_process(None, None, 65536) == E_INVALID
    assert lib.pebblegpu_multibank_synchronize(None) == E_INVALID
    assert lib.pebblegpu_multibank_destroy(None) == 0


def test_no_device_is_a_loud_failure(lib):
    import pebblesdr_amd as P
    if lib.pebblegpu_device_count() > 0:
        pytest.skip("a device is visible")
    ids = (C.c_int32 * 2)(0, 0)
    h = C.c_void_p()
    cfg = config()
    assert lib.pebblegpu_multibank_create(C.byref(cfg), ids, 2, 0, C.byref(h)) == E_NO_DEVICE
    assert lib.pebblegpu_multibank_create(C.byref(cfg), ids, 2, P.MULTIBANK_SPECTRUM_SHARD0, C.byref(h)) == E_NO_DEVICE
    with pytest.raises(P.PebbleGpuError) as e:
        P.MultiBank(2048000, 8, [0, 0], max_superframes=2)
    assert e.value.code == E_NO_DEVICE


def test_c_host_example_compiles_and_links(lib, tmp_path):
    """compile and link only: running it needs a device (tests/test_multibank_gpu.py)"""
    src, exe = os.path.join(ROOT, "examples", "multibank_host.c"), str(tmp_path / "multibank_host")
    libdir = os.path.join(ROOT, "pebblesdr_amd")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lpebblegpu", "-Wl,-rpath," + libdir,
                        "-lm", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(exe)


ADAPTER_SRC = r"""
#include "pebblegpu_steps.hpp"
int main()
{
    pebblegpu_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.sample_rate = 2048000;
    cfg.n_channels = 4;
    cfg.shared_input = 1;
    pebblegpu::MultiBank mb(cfg, std::vector<int>{0, 0});
    const int created = mb.lastStatus();
    mb.setMixer(1, 1e3);
    mb.setBandPass(1, 300, 3000);
    mb.setDemodMode(1, pebblegpu::dmUSB);
    std::vector<const void *> p(2, nullptr);
    mb.process(p, 65536);
    mb.processRaw(PEBBLEGPU_IQ_S8, PEBBLEGPU_IQO_IQ, 1.0, p, 65536);
    mb.ingestAcquire(0, 16);
    mb.ingestSubmit(0, 16);
    mb.processIngested(0, PEBBLEGPU_IQ_S8, PEBBLEGPU_IQO_IQ, 1.0, 65536);
    mb.synchronize();
    std::printf("%d %u %p\n", created, mb.shards(), (void *)mb.shard(0));
    return 0;
}
"""


def test_cpp_adapter_compiles_and_fails_loudly_without_a_device(lib, tmp_path):
    """pebblegpu::MultiBank (include/pebblegpu_steps.hpp): every member compiles; with no device the constructor reports
    PEBBLEGPU_E_NO_DEVICE and the members are harmless"""
    src, exe = tmp_path / "mb_adapter.cpp", str(tmp_path / "mb_adapter")
    src.write_text(ADAPTER_SRC)
    libdir = os.path.join(ROOT, "pebblesdr_amd")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lpebblegpu",
                        "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if lib.pebblegpu_device_count() > 0:
        return  # (running it would drive a device: the GPU tier does that through the C ABI)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[:2] == [str(E_NO_DEVICE), "0"], r.stdout + r.stderr
