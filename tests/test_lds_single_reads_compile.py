"""The exchange gathers stay single 8-byte LDS reads after compilation.

lds_gather_b64 (csrc/fft_lds.h) exists because the compiler merges two 8-byte LDS reads off one base into one pair read wherever their
distance allows, and a pair read costs twice what its two halves cost as single reads (profiles/lds_pair_reads_isa_rates.txt).  A
later edit that goes back to plain loads in a gather would be re-paired without a word: this test compiles a few kernels that
instantiate the helper and fft2048_t128 for gfx950 (device side only, a few seconds -- not cores.hip) and counts the LDS reads in
their bodies with tools/isa_mix.py's parser.  No GPU is needed; skipped where there is no hipcc.
"""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")

SRC = r"""
#include "fft_t128.h"
using namespace pg;

// the transform as k_spectrum_t128 uses it: twiddles in registers, so every LDS read in the body is one of its two gathers
__global__ __launch_bounds__(128) void probe_fft_t128(const float2 *__restrict__ in, float2 *__restrict__ out, const Tw128Regs *__restrict__ w)
{
    __shared__ float2 lds[FftLds<2048>::kSlots];
    const int t = threadIdx.x;
    float2 v[16];
#pragma unroll
    for (int m = 0; m < 16; m++) v[m] = in[blockIdx.x * 2048 + t + 128 * m];
    fft2048_t128<void (*)(), true, true, true, false, 0>(v, lds, nullptr, t, [] { __syncthreads(); }, w[t]);
#pragma unroll
    for (int m = 0; m < 16; m++) out[blockIdx.x * 2048 + t + 128 * m] = v[m];
}

// the helper alone at its three block counts, at strides the compiler would pair (adjacent; 64 apart) and one it would not
template <int N, int S> __device__ __forceinline__ void probe(const float2 *in, float2 *out)
{
    __shared__ float2 lds[N * S + 256];
    for (int i = threadIdx.x; i < N * S + 256; i += 256) lds[i] = in[i];
    __syncthreads();
    float2 v[N];
    lds_gather_b64<N, LdsStride<S>>(v, lds + threadIdx.x);
#pragma unroll
    for (int m = 0; m < N; m++) out[threadIdx.x + 256 * m] = v[m];
}
__global__ __launch_bounds__(256) void probe_gather8(const float2 *in, float2 *out) { probe<8, 1>(in, out); }
__global__ __launch_bounds__(256) void probe_gather16(const float2 *in, float2 *out) { probe<16, 64>(in, out); }
__global__ __launch_bounds__(256) void probe_gather32(const float2 *in, float2 *out) { probe<32, 136>(in, out); }
"""

# kernel -> single 8-byte reads expected in its body (fft2048_t128: pass B's sixteen and pass C's sixteen)
EXPECTED = {"probe_fft_t128": 32, "probe_gather8": 8, "probe_gather16": 16, "probe_gather32": 32}
PAIR_READS = ("ds_read2_b64", "ds_read2st64_b64")


def _isa_mix():
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def mixes(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("lds_single_reads")
    src = d / "probe.hip"
    src.write_text(SRC)
    asm = d / "probe.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I" + CSRC, str(src), "-o", str(asm)])
    found = _isa_mix().kernel_mix(asm.read_text(), tuple(EXPECTED))
    return {k: c for name, c in found.items() for k in EXPECTED if k in name}


@pytest.mark.parametrize("kernel", sorted(EXPECTED))
def test_gathers_compile_to_single_reads(mixes, kernel):
    assert kernel in mixes, sorted(mixes)
    c = mixes[kernel]
    print(kernel, {k: v for k, v in c.items() if k.startswith("ds_")})
    for op in PAIR_READS:
        assert c[op] == 0, (kernel, op, c[op])
    assert c["ds_read_b64"] == EXPECTED[kernel], (kernel, c["ds_read_b64"])
