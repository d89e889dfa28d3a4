"""LDS bank conflicts of the transforms' exchanges, enumerated on the host from the padding functions of csrc/fft_lds.h.

A small host program (compiled against the header: lpad, lpad4, lpad_sel are __host__ __device__) lists the byte address of every
lane for every scatter and gather of the two-wave 2048-point transform (fft_t128.h: A -> B, B -> C), of the 2048-point plan of
fft_regs (256 work-items, radix 4 * 8 * 8 * 8) and of k_spectrum_t128's frame gather with and without the DEC padding, and prices
each instruction by the grouping rule of the instruction the kernels issue for it:

  single 8-byte read (ds_read_b64, lds_gather_b64):  two groups of 32 lanes, bank = (a / 4) mod 64
  8-byte store and pair read (ds_write_b64, ds_write2_b64, ds_read2_b64):  four groups of 16 lanes, bank = (a / 4) mod 32

The degree of a group is the largest number of distinct dwords on one bank (equal addresses broadcast); an instruction costs its
groups' degrees added up, so "degree 1" below means no extra LDS cycle anywhere.  Expected: 1 everywhere, except the one
gather that DESIGN.md section 4 ("pair reads") accepts at 2:

  * the frame gather with the DEC padding -- one pad slot per 8 samples for the decimator's stride-8 reads: 32 lanes span 36
    slots, the last three wrap onto busy banks.  That instance is not on any default route.

The image between passes A and B of the two-wave transform is the transposed one (t128_slot_ab, fft_t128.h) for that reason: on
the padded layout it replaced (lpad4, one pad slot per 16) pass B's gather is two-way conflicted under the single-read rule --
`t128_gather_B_lpad4` below pins that, so the reason for the layout stays checked.

fft_regs keeps the compiler's pair reads (its kernels were not changed), so its gathers are priced by the pair rule.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")

MAIN = r"""
#include "fft_t128.h"
#include <cstdio>
#include <set>
#include <vector>
using namespace pg;

// worst group degree of one wave64 instruction: lane l touches the two dwords at slot[l] * 2
static int degree(const int *slot, int group, int banks)
{
    int worst = 0;
    for (int g = 0; g < 64; g += group) {
        std::vector<std::set<int>> on(banks);
        for (int l = g; l < g + group; l++)
            for (int d = 0; d < 2; d++) on[(2 * slot[l] + d) % banks].insert(2 * slot[l] + d);
        for (auto &s : on) worst = (int)s.size() > worst ? (int)s.size() : worst;
    }
    return worst;
}
static int worst;
template <class F> static void instr(int T, bool single_read, F slot_of)  // slot_of(t): float2 slot of work-item t
{
    for (int w = 0; w < T / 64; w++) {
        int slot[64];
        for (int l = 0; l < 64; l++) slot[l] = slot_of(64 * w + l);
        const int d = single_read ? degree(slot, 32, 64) : degree(slot, 16, 32);
        worst = d > worst ? d : worst;
    }
}
static void report(const char *name)
{
    std::printf("%s %d\n", name, worst);
    worst = 0;
}

template <int R, int P, bool FIRST, bool LAST> static void regs_pass(const char *gname, const char *sname)
{
    constexpr int N = 2048, T = 256, E = N / T, Q = E / R;
    constexpr int PAD_IN = (!FIRST && P == 4) ? kPad1per16 : kPad4per32;
    constexpr int PAD_OUT = (FIRST && R == 4) ? kPad1per16 : kPad4per32;
    if (!FIRST) {
        for (int m = 0; m < E; m++) instr(T, false, [&](int t) { return lpad_sel<PAD_IN>(t) + lpad_sel<PAD_IN>(T * m); });
        report(gname);
    }
    if (!LAST) {
        for (int q = 0; q < Q; q++)
            for (int r = 0; r < R; r++)
                instr(T, false, [&](int t) {
                    const int jbase = (t - (t & (P - 1))) * R + (t & (P - 1));
                    return lpad_sel<PAD_OUT>(jbase) + lpad_sel<PAD_OUT>(T * R * q) + lpad_sel<PAD_OUT>(r * P);
                });
        report(sname);
    }
}

int main()
{
    // ---- fft2048_t128 ----
    for (int k = 0; k < 16; k++) instr(128, false, [&](int t) { return t + kT128Pitch * k; });
    report("t128_scatter_A");
    for (int m = 0; m < 16; m++) instr(128, true, [&](int t) { return t128_slot_ab(t) + 8 * m; });
    report("t128_gather_B");
    for (int m = 0; m < 16; m++) instr(128, true, [&](int t) { return lpad4(t) + 136 * m; });
    report("t128_gather_B_lpad4");
    for (int q = 0; q < 2; q++)
        for (int r = 0; r < 8; r++)
            instr(128, false, [&](int t) { const int k = t & 15; return lpad((t - k) * 8 + k) + lpad(1024 * q) + lpad(16 * r); });
    report("t128_scatter_B");
    for (int m = 0; m < 16; m++) instr(128, true, [&](int t) { return lpad(t) + 144 * m; });
    report("t128_gather_C");
    // the helper's offsets are the padded positions of the elements the passes want
    for (int t = 0; t < 128; t++)
        for (int m = 0; m < 16; m++)
            if (t128_slot_ab(t) + LdsStride<8>::at(m) != t128_slot_ab(t + 128 * m) || lpad(t) + LdsStride<144>::at(m) != lpad(t + 128 * m)) return 1;
    // ... the scatter's too, and no two elements share a slot of the transposed image
    {
        std::set<int> slots;
        for (int t = 0; t < 128; t++)
            for (int k = 0; k < 16; k++) {
                if (t + kT128Pitch * k != t128_slot_ab(16 * t + k)) return 2;
                slots.insert(t128_slot_ab(16 * t + k));
            }
        if (slots.size() != 2048 || *slots.rbegin() >= FftLds<2048>::kSlots) return 3;
    }
    // ---- k_spectrum_t128's frame gather: sample t + 128 m in region m / 4 (REGION slots each), slot XOFF + fslot((t + 128 m) % 512) ----
    for (int dec = 0; dec < 2; dec++) {
        const int REGION = FftLds<2048>::kSlots, RSTEP = dec ? 144 : 128;
        for (int m = 0; m < 16; m++) instr(128, true, [&](int t) { return t + (dec ? t >> 3 : 0) + (m / 4) * REGION + (m % 4) * RSTEP; });
        report(dec ? "frame_gather_dec" : "frame_gather");
    }
    // ---- fft_regs<2048>, 256 work-items: radix 4 * 8 * 8 * 8 ----
    regs_pass<4, 1, true, false>("", "regs_scatter_P1");
    regs_pass<8, 4, false, false>("regs_gather_P4", "regs_scatter_P4");
    regs_pass<8, 32, false, false>("regs_gather_P32", "regs_scatter_P32");
    regs_pass<8, 256, false, true>("regs_gather_P256", "");
    return 0;
}
"""

EXPECTED = {
    "t128_scatter_A": 1,
    "t128_gather_B": 1,
    "t128_gather_B_lpad4": 2,  # the layout that was replaced: see the module docstring
    "t128_scatter_B": 1,
    "t128_gather_C": 1,
    "frame_gather": 1,
    "frame_gather_dec": 2,  # accepted: see the module docstring
    "regs_scatter_P1": 1,
    "regs_gather_P4": 1,
    "regs_scatter_P4": 1,
    "regs_gather_P32": 1,
    "regs_scatter_P32": 1,
    "regs_gather_P256": 1,
}


@pytest.fixture(scope="module")
def degrees(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: fft_lds.h needs the HIP headers and a compiler that knows __device__")
    d = tmp_path_factory.mktemp("lds_banks")
    src = d / "banks_main.hip"
    src.write_text(MAIN)
    exe = str(d / "banks_main")
    # host side only: nothing is compiled for a device and the program makes no HIP call
    subprocess.check_call([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-Wno-unused-result", "-I" + CSRC, str(src), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return {name: int(v) for name, v in (line.split() for line in r.stdout.splitlines())}


def test_every_exchange_is_enumerated(degrees):
    assert sorted(degrees) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_conflict_degree(degrees, name):
    print(name, "degree", degrees[name], "expected", EXPECTED[name])
    assert degrees[name] == EXPECTED[name]
