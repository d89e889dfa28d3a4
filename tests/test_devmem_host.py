"""CPU tier of csrc/devmem.h: DevBuf / PinnedBuf compiled with g++ into a stand-alone program whose own hipMalloc, hipFree, ...
count what is live and can be told to fail on the k-th call.  Built with AddressSanitizer and UBSan: a double free, a leak or a
use after a move ends the program with a non-zero status.  Each scenario checks the live allocation count AND the library's byte
counters (what pebblegpu_live_bytes reports) against the sum of live sizes at every step."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")

MAIN = r"""
#define __HIP_PLATFORM_AMD__ 1
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>
#include "devmem.h"

// ---- the stand-in runtime: every allocation is a malloc, recorded with its size ----
static std::map<void *, size_t> g_dev, g_pin;
static int g_calls[8];                       // per entry point
static int g_fail_fn = -1, g_fail_at = 0;    // entry point `g_fail_fn` fails on its g_fail_at-th call from now
enum { MALLOC, FREE, HMALLOC, HFREE, MEMSET, MEMCPY, SYNC };
static bool failing(int fn)
{
    g_calls[fn]++;
    if (fn != g_fail_fn) return false;
    return --g_fail_at == 0;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { if (failing(MALLOC)) return hipErrorOutOfMemory; *p = n ? std::malloc(n) : nullptr; if (n) g_dev[*p] = n; return hipSuccess; }
hipError_t hipFree(void *p) { failing(FREE); if (!g_dev.count(p)) { std::printf("hipFree of an unknown pointer\n"); std::exit(1); } g_dev.erase(p); std::free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { if (failing(HMALLOC)) return hipErrorOutOfMemory; *p = n ? std::malloc(n) : nullptr; if (n) g_pin[*p] = n; return hipSuccess; }
hipError_t hipHostFree(void *p) { failing(HFREE); if (!g_pin.count(p)) { std::printf("hipHostFree of an unknown pointer\n"); std::exit(1); } g_pin.erase(p); std::free(p); return hipSuccess; }
hipError_t hipMemset(void *p, int v, size_t n) { if (failing(MEMSET)) return hipErrorInvalidValue; std::memset(p, v, n); return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { if (failing(MEMCPY)) return hipErrorInvalidValue; std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { if (failing(SYNC)) return hipErrorInvalidValue; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stand-in error"; }
}
namespace pg {
static char g_msg[512];
int fail(int code, const char *fmt, ...) { va_list ap; va_start(ap, fmt); std::vsnprintf(g_msg, sizeof(g_msg), fmt, ap); va_end(ap); return code; }
}

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
static size_t sum(const std::map<void *, size_t> &m) { size_t s = 0; for (auto &kv : m) s += kv.second; return s; }
// n_dev / n_pin live allocations, and the byte counters equal to the sum of what is live
#define LIVE(n_dev, n_pin) do { CHECK(g_dev.size() == (size_t)(n_dev)); CHECK(g_pin.size() == (size_t)(n_pin)); \
    CHECK(pg::g_live_device.load() == sum(g_dev)); CHECK(pg::g_live_pinned.load() == sum(g_pin)); } while (0)

template <template <class> class B>
static void basics(bool pinned)
{
    const int d = pinned ? 0 : 1, p = pinned ? 1 : 0;
    {
        B<float> a;
        CHECK(a.get() == nullptr && a.size() == 0);
        a.release();  // empty: harmless
        LIVE(0, 0);
        CHECK(a.alloc(100) == 0);
        CHECK(a.get() != nullptr && a.size() == 100);
        LIVE(d, p);
        B<float> b(std::move(a));  // move-construct: the source is empty, nothing was allocated or freed
        CHECK(a.get() == nullptr && a.size() == 0 && b.size() == 100);
        LIVE(d, p);
        B<float> c;
        CHECK(c.alloc(7) == 0);
        LIVE(2 * d, 2 * p);
        c = std::move(b);  // move-assign: what c held is freed
        CHECK(b.get() == nullptr && c.size() == 100);
        LIVE(d, p);
        c.release();
        LIVE(0, 0);
        c.release();  // a second release is harmless
        LIVE(0, 0);
        CHECK(c.alloc(3) == 0);
        float *first = c.get();
        CHECK(c.alloc(5) == 0);  // allocating into a held buffer frees the old one first
        CHECK(!g_dev.count(first) && !g_pin.count(first) && c.size() == 5);
        LIVE(d, p);
        std::vector<B<double>> v;  // a vector of owners: growth moves them
        for (int i = 0; i < 9; i++) { B<double> t; CHECK(t.alloc_zero(i + 1) == 0); v.push_back(std::move(t)); LIVE(d + (i + 1) * d, p + (i + 1) * p); }
        for (int i = 0; i < 9; i++) { CHECK(v[i].size() == (size_t)i + 1); CHECK(v[i][i] == 0.0); }
    }
    LIVE(0, 0);  // the destructors freed the rest
}

static void failures()
{
    pg::DevBuf<int> a;
    g_fail_fn = MALLOC; g_fail_at = 1;
    CHECK(a.alloc(10) == -3 && a.get() == nullptr && a.size() == 0);
    LIVE(0, 0);
    // the memset behind a successful malloc fails: the status comes back and nothing stays allocated
    g_fail_fn = MEMSET; g_fail_at = 1;
    CHECK(a.alloc_zero(10) == -3 && a.get() == nullptr);
    CHECK(std::strstr(pg::g_msg, "hipMemset") && std::strstr(pg::g_msg, "40 bytes"));
    LIVE(0, 0);
    const int h[4] = {1, 2, 3, 4};
    g_fail_fn = MEMCPY; g_fail_at = 1;
    CHECK(a.upload(h, 4) == -3 && a.get() == nullptr);
    LIVE(0, 0);
    g_fail_fn = -1;
    CHECK(a.upload(h, 4) == 0 && a[3] == 4);
    LIVE(1, 0);
    // a failed allocation into a held buffer: the old one is gone (freed first), the buffer is empty
    g_fail_fn = MALLOC; g_fail_at = 1;
    CHECK(a.alloc(8) == -3 && a.get() == nullptr && a.size() == 0);
    LIVE(0, 0);
    g_fail_fn = HMALLOC; g_fail_at = 1;
    pg::PinnedBuf<char> p;
    CHECK(p.alloc(64) == -3 && p.get() == nullptr);
    LIVE(0, 0);
    g_fail_fn = -1;
}

static void grow()
{
    pg::DevBuf<float> y;
    hipStream_t s = nullptr;
    CHECK(y.grow(s, 100) == 0 && y.size() == 100);
    CHECK(g_calls[SYNC] == 1 && g_calls[MALLOC] == 1 && g_calls[FREE] == 0);
    LIVE(1, 0);
    float *p = y.get();
    CHECK(y.grow(s, 100) == 0 && y.grow(s, 1) == 0 && y.grow(s, 0) == 0);  // covered: no synchronisation, no allocation
    CHECK(y.get() == p && g_calls[SYNC] == 1 && g_calls[MALLOC] == 1 && g_calls[FREE] == 0);
    CHECK(y.grow(s, 101) == 0 && y.size() == 101);  // larger: synchronise, free, allocate -- in that order
    CHECK(g_calls[SYNC] == 2 && g_calls[MALLOC] == 2 && g_calls[FREE] == 1);
    LIVE(1, 0);
    g_fail_fn = SYNC; g_fail_at = 1;  // the wait fails: nothing is freed
    CHECK(y.grow(s, 500) == -3 && y.size() == 101);
    LIVE(1, 0);
    g_fail_fn = MALLOC; g_fail_at = 1;
    CHECK(y.grow(s, 500) == -3 && y.size() == 0 && y.get() == nullptr);
    LIVE(0, 0);
    g_fail_fn = -1;
    CHECK(y.grow(s, 500) == 0 && y.size() == 500);
    LIVE(1, 0);
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!std::strcmp(what, "device")) basics<pg::DevBuf>(false);
    else if (!std::strcmp(what, "pinned")) basics<pg::PinnedBuf>(true);
    else if (!std::strcmp(what, "failures")) failures();
    else if (!std::strcmp(what, "grow")) grow();
    else return 2;
    LIVE(0, 0);
    std::printf("ok\n");
    return 0;
}
"""


def _rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    hipcc = shutil.which("hipcc")
    assert hipcc, "no ROCm headers found"
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("devmem")
    src = d / "devmem_main.cpp"
    src.write_text(MAIN)
    exe = str(d / "devmem_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing has to be loaded ahead of it
                           "-I" + CSRC, "-I" + _rocm_include(), str(src), "-o", exe])
    return exe


def test_header_compiles_without_sanitizers_and_warnings(tmp_path):
    """devmem.h alone, plain g++ -Wall -Werror: no device code, no common.h"""
    src = tmp_path / "only.cpp"
    src.write_text('#define __HIP_PLATFORM_AMD__ 1\n#include "devmem.h"\npg::DevBuf<float> *a; pg::PinnedBuf<int> *b;\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-I" + _rocm_include(), "-c", str(src), "-o", str(tmp_path / "only.o")])


@pytest.mark.parametrize("scenario", ["device", "pinned", "failures", "grow"])
def test_owning_buffers(program, scenario):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, scenario], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", (r.returncode, r.stdout, r.stderr)
