"""CPU tier of the modem hook ring at a modem rate (pebblegpu_modem_rate_plan, pebblegpu_receiver_modem_out_open_rate): the plan against
the oracle's Decimator (pinned to the reference's class) for the table of chains and for other demodulator rates, the look-back against
its formula and against the oracle (H samples in front of a segment reproduce the stream, H - 1 do not), every refusal that needs no
device with its code, the block layout for decimated sizes, the info struct against its declaration, and that the C example and the C++
adapter compile.  tests/test_modem_rate_gpu.py holds the ring itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import modem_out_cases as MC
from tests import modem_rate_cases as RC
from tests import tail_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd as P
    return P


@pytest.fixture(scope="module")
def O(P):
    import oracle
    return oracle


def code_of(P, fn, *args):
    with pytest.raises(P.PebbleGpuError) as e:
        fn(*args)
    return e.value.code, str(e.value)


@pytest.mark.parametrize("chain", sorted(RC.CHAINS) + [RC.EMPTY], ids=lambda c: "%d-%d" % c)
def test_plan_against_the_oracle_for_the_table(P, O, chain):
    bw, mn = chain
    info = P.modem_rate_plan(TC.RATE, TC.SPF, bw, mn)
    dec = O.Decimator(TC.RATE, bw, mn)
    stages, D = RC.CHAINS.get(chain, ([], 1))
    assert info.chain() == dec.chain() == stages
    assert info.total_decimation == dec.total_decimation == D and info.n_stages == len(stages)
    assert float(info.rate) == float(dec.rate) and info.rate_int == int(dec.rate) == TC.RATE // D
    assert info.samples_per_superframe == TC.SPF // D
    assert info.lookback == RC.lookback(stages) == RC.LOOKBACK.get(chain, 0)
    assert info.struct_size == C.sizeof(P.ModemRateInfo)
    assert all(info.taps[j] == 0 and info.stride[j] == 0 for j in range(len(stages), P.MODEM_RATE_MAX_STAGES))


@pytest.mark.parametrize("rate", RC.OTHER_RATES)
def test_plan_against_the_oracle_at_other_demodulator_rates(P, O, rate):
    """39062 and 48828 (receivers whose rate is no integer: the cast of morse.cpp:193) and the 48 kHz receiver without a decimator, for
    every (max_bw, min_rate) of the table and for min_rate 0 (the reference's minDecimatedSampleRate)"""
    seen = set()
    for bw, mn in sorted(RC.CHAINS) + [RC.EMPTY, (1000, 0), (3000, 0)]:
        info = P.modem_rate_plan(rate, 2048, bw, mn)
        dec = O.Decimator(rate, bw, mn)
        assert info.chain() == dec.chain(), (rate, bw, mn)
        assert float(info.rate) == float(dec.rate) and info.rate_int == int(dec.rate) and info.total_decimation == dec.total_decimation
        assert info.lookback == RC.lookback(dec.chain()) and info.samples_per_superframe * info.total_decimation == 2048
        seen.add(info.rate_int)
    assert {39062: 4882, 48828: 6103, 48000: 6000}[rate] in seen   # (1000, 8000)
    assert P.modem_rate_plan(rate, 2048, 1000, 8000).chain() == {39062: [(11, 2), (15, 2), (19, 2)]}.get(rate, [(11, 4), (15, 2)])


@pytest.mark.parametrize("chain", sorted(RC.CHAINS), ids=lambda c: "%d-%d" % c)
def test_lookback_is_what_the_stream_depends_on(P, O, chain):
    """the claim the kernel rests on, on the oracle alone: a fresh Decimator that sees nothing older than the H demodulator samples in
    front of a segment gives exactly the streaming decimator's outputs of that segment (difference 0.0: the missing terms are products
    with zeros); with the oldest of those H samples zeroed as well it does not.  The third super-frame is run again on its own, its first
    `lead` samples (H rounded up to a multiple of D) serving as the look-back of the rest"""
    bw, mn = chain
    stages, D = RC.CHAINS[chain]
    H = P.modem_rate_plan(TC.RATE, TC.SPF, bw, mn).lookback
    rng = np.random.default_rng(3)
    x = rng.standard_normal(3 * TC.SPF) + 1j * rng.standard_normal(3 * TC.SPF)
    stream = np.concatenate(RC.decimated(O, TC.RATE, bw, mn, [x[j * TC.SPF:(j + 1) * TC.SPF] for j in range(3)]))
    lead = -(-H // D) * D
    seg = stream[(2 * TC.SPF + lead) // D:]

    def rerun(keep):
        y = x[2 * TC.SPF:].copy()
        y[:lead - keep] = 0.0
        return RC.decimated(O, TC.RATE, bw, mn, [y])[0][lead // D:]

    with_h, without = float(np.max(np.abs(rerun(H) - seg))), float(np.max(np.abs(rerun(H - 1) - seg)))
    print("(%d Hz, %d Hz): H = %d: difference %.3e with H samples of look-back, %.3e with H - 1" % (bw, mn, H, with_h, without))
    assert len(seg) == (TC.SPF - lead) // D and with_h == 0.0 and without > 0.0


def test_refusals_with_their_codes(P):
    L = P.load_library()
    plan = P.modem_rate_plan
    code, text = code_of(P, plan, TC.RATE, TC.SPF, RC.CIC3[0], RC.CIC3[1])
    assert code == RC.E_UNSUPPORTED and "CIC3" in text and "not built" in text
    assert code_of(P, plan, TC.RATE, TC.SPF, 0, 8000)[0] == RC.E_INVALID                  # max_bw == 0
    assert code_of(P, plan, 0, TC.SPF, 1000, 8000)[0] == RC.E_INVALID
    assert code_of(P, plan, TC.RATE, 100, 1000, 8000)[0] == RC.E_SIZE                     # 100 is no multiple of D = 8
    assert code_of(P, plan, TC.RATE, 2044, 1000, 8000)[0] == RC.E_SIZE
    code, text = code_of(P, plan, TC.RATE, 8, 1000, 8000)                                 # the 11-tap stage would get 8 inputs
    assert code == RC.E_SIZE and "11-tap" in text
    code, text = code_of(P, plan, TC.RATE, 56, 1000, 8000)                                # ... and the 15-tap stage 14
    assert code == RC.E_SIZE and "15-tap" in text
    code, text = code_of(P, plan, TC.RATE, 64, 1000, 8000)                                # every stage is fed, but H = 66 > 64
    assert code == RC.E_SIZE and "66" in text
    assert P.modem_rate_plan(TC.RATE, 72, 1000, 8000).samples_per_superframe == 9         # the smallest super-frame that passes
    assert code_of(P, plan, TC.RATE, 136, 3000, 8000)[0] == RC.E_SIZE                     # H = 142 > 136
    assert P.modem_rate_plan(TC.RATE, 144, 3000, 8000).lookback == 142
    info = P.ModemRateInfo()
    assert L.pebblegpu_modem_rate_plan(TC.RATE, TC.SPF, 1000, 8000, None) == RC.E_INVALID
    assert L.pebblegpu_modem_rate_plan(TC.RATE, TC.SPF, 1000, 8000, C.byref(info)) == RC.E_INVALID      # struct_size not set
    assert L.pebblegpu_receiver_modem_out_open_rate(None, MC.F32, None, 0, 4, 1000, 8000) == RC.E_INVALID
    assert b"null" in L.pebblegpu_last_error()


def test_layout_for_decimated_sizes(P):
    """the block layout is the plain ring's function at the decimated sizes: rows of k * (2048 / D) samples, padded to 16 bytes, the
    trailer right behind them -- for D = 4 and 8, odd row counts, and a super-frame of 9 modem samples (odd rows in both formats)"""
    seen = set()
    for fmt in (MC.F32, MC.S16):
        for D in (4, 8):
            for rows in (1, 5, 6, 16, 70):
                for k in (1, 2, 3):
                    for m in (TC.SPF // D, 9):
                        n = k * m
                        pitch, off, nbytes = P.modem_out_layout(fmt, rows, n, k)
                        assert (pitch, off, nbytes) == MC.layout_ref(fmt, rows, n, k)
                        seen.add((pitch != n * MC.BYTES[fmt], nbytes != rows * k))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_info_struct_matches_its_declaration(P, tmp_path):
    fields = [f for f, _ in P.ModemRateInfo._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pebblegpu.h"', 'int main(void) {', 'printf("%zu\\n", sizeof(pebblegpu_modem_rate_info));']
    lines += ['printf("%%zu\\n", offsetof(pebblegpu_modem_rate_info, %s));' % f for f in fields]
    lines += ['printf("%d\\n", PEBBLEGPU_MODEM_RATE_MAX_STAGES);', 'return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(P.ModemRateInfo)] + [getattr(P.ModemRateInfo, f).offset for f in fields] + [P.MODEM_RATE_MAX_STAGES]


def test_the_c_host_the_feeder_and_the_adapter_compile(P, tmp_path):
    lib = os.path.join(ROOT, "pebblesdr_amd")
    inc = "-I" + os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", inc, os.path.join(ROOT, "examples", "modem_rate_host.c"), "-L" + lib, "-lpebblegpu",
                           "-Wl,-rpath," + lib, "-lm", "-lpthread", "-o", str(tmp_path / "modem_rate_host")])
    for name, text in (("feeder", RC.rate_feeder_cpp()), ("adapter", RC.ADAPTER_CPP)):
        src = tmp_path / (name + ".cpp")
        src.write_text(text)
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", inc, str(src), "-L" + lib, "-lpebblegpu", "-Wl,-rpath," + lib, "-o", str(tmp_path / name)])


def test_header_and_documents_state_the_semantics():
    hdr = open(os.path.join(ROOT, "include", "pebblegpu.h")).read()
    for phrase in ("pebblegpu_receiver_modem_out_open_rate", "decimator.cpp:64-149", "morse.cpp:174-193", "stands still", "DROPPED", "EMPTY CHAIN",
                   "CIC3", "minDecimatedSampleRate", "k_modem_rate_pack"):
        assert phrase in hdr, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_modem_rate_pack" in design and "pebblegpu_receiver_modem_out_open_rate" in design
    assert "modemOutOpenRate" in open(os.path.join(ROOT, "include", "pebblegpu_steps.hpp")).read()
    assert "pebblegpu_receiver_modem_out_open_rate" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
