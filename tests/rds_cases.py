"""The coverage statement for the dmFMS branch (csrc/kernels_demod.h: k_wfm_pilot, k_wfm_lmr_fir; csrc/kernels_rds.h: k_rds_discrim,
k_rds_hilbert_mix, k_rds_fir, k_rds_pll, k_rds_matched, k_rds_bits; csrc/rds.hip: RdsCore::run's head-room refresh and RdsCore::collect's
replay of the reference's 100-entry group queue): one table of rows, call-length scripts and inputs, used by the CPU tier
(tests/test_rds_geometry_host.py: the design table pinned from csrc/design.cpp, a plain fp64 model of the branch held to the oracle,
the inputs shown to be ones on which deliberately wrong models cannot pass, the decoder paths input B and C are there for shown to be
reached) and by the GPU tier (tests/test_rds_geometry_gpu.py: the same rows through P.Demod and P.ReceiverBank against the oracle).
No row sets an environment switch, no kernel is launched directly.

design::rds_design builds one decimate-by-2 chain per demodulator rate (CDownConvert::SetDataRate(rate, 8000)): two, three or four
stages at the rows below, which between them carry the stage designs 1, 2, 3, 4, 5, 7 and 11 (the fixed 11-tap class, the generic
class from 15 to 51 taps; k_rds_fir takes the tap count as an argument, a rate between the rows only picks another table).  NOT
reachable, and so not covered:
  - k_rds_fir's `newest = 1` case (the CIC3, design 0): no row's chain has a stage of design 0, and no rate at which dmFMS is
    accepted (WfmCore::set_stereo needs the one-kernel path) gets one -- the host tier pins both; as k_copy, it has no caller;
  - the wrap of the 4096-entry event log (RdsCore::collect's `total - from > log_cap`): at three groups a second that is twenty
    minutes of signal between two reads.

Bars: m_RdsData (P.Demod.rdsData) of every call at 1e-6, the audio of every call at 1e-5 in both channels, lengths, lock flags,
groups and `changed` flags exact.  The error of a call is the RMS of its difference over the larger of that call's reference RMS and
the reference RMS over the whole script (call_errors): an 18-sample call can lie where m_RdsData passes through zero.
"""
from collections import namedtuple
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests import rds_signal as rs
from tests.demod_cases import CSRC, MIN_CALL, E_SIZE, rms, wfm_design  # noqa: F401  (E_SIZE, wfm_design: for the tiers)

RDS_TOL = 1e-6       # tests/test_parity_gpu.py::test_wfm_stereo_rds_branch_against_the_oracle's bar (it measured 5e-8)
AUDIO_TOL = 1e-5     # BASELINE.json north_star
MODEL_TOL = 1e-9     # the plain model against the oracle: a thousandth of the device's bar
CAP = 8192           # the handle's capacity in the geometry rows
Q_SIZE = 100         # RDS_Q_SIZE: m_RdsGroupQueue's entries


# ------------------------------------------------------------------------------------------------
# comparison, the same function in both tiers
# ------------------------------------------------------------------------------------------------
def call_errors(got, ref):
    """got, ref: one array per call.  -> per call RMS(got - ref) / max(RMS(ref of the call), RMS(ref of all calls)); lengths must agree"""
    whole = rms(np.concatenate([np.asarray(r) for r in ref]))
    out = []
    for g, r in zip(got, ref):
        g, r = np.asarray(g), np.asarray(r)
        assert len(g) == len(r), (len(g), len(r))
        out.append(rms(g - r) / max(rms(r), whole, 1e-300))
    return out


# ------------------------------------------------------------------------------------------------
# what csrc/design.cpp designs, asked with g++ (no device)
# ------------------------------------------------------------------------------------------------
_PROGRAM = r'''
#include <cstdio>
#include "design.h"
using namespace pg::design;
static void vec(const char *name, const double *v, size_t n)
{
    std::printf("%s %zu", name, n);
    for (size_t i = 0; i < n; i++) std::printf(" %.17g", v[i]);
    std::printf("\n");
}
int main()
{
    double rate;
    while (std::scanf("%lf", &rate) == 1) {
        const RdsDesign d = rds_design(rate);
        const WfmPilotDesign p = wfm_pilot_design(rate);
        double amp[1024];
        oscillator_amplitudes(amp, 1024);
        const double sc[12] = {d.rate, d.osc_turns, d.nco_lo, d.nco_hi, d.alpha, d.beta, d.bitsync.b0, d.bitsync.b1, d.bitsync.b2, d.bitsync.a1,
                               d.bitsync.a2, (double)d.stages.size()};
        vec("scalars", sc, 12);
        for (int s : d.stages) {
            const std::vector<double> h = downconvert_stage_response(s);
            std::printf("design %d %d\n", s, downconvert_stage_taps(s));
            vec("stage", h.data(), h.size());
        }
        vec("lp", d.lp.data(), d.lp.size());
        vec("matched", d.matched.data(), d.matched.size());
        vec("hilbert", p.hilb, 122);
        vec("amp", amp, 1024);
    }
    return 0;
}
'''

RdsDesignFacts = namedtuple("RdsDesignFacts", "rate rds_rate osc_turns nco_lo nco_hi alpha beta bitsync stages stage_taps stage_h lp matched hilb_i hilb_q amp")


@functools.lru_cache(maxsize=None)
def _design_exe():
    d = tempfile.mkdtemp(prefix="rds_design_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "rds_design.cpp"), os.path.join(d, "rds_design")
    with open(src, "w") as f:
        f.write(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, src, os.path.join(CSRC, "design.cpp"), "-o", exe])
    return exe


@functools.lru_cache(maxsize=None)
def rds_design(rate):
    """design::rds_design, wfm_pilot_design's Hilbert pair and oscillator_amplitudes at this demodulator rate -> RdsDesignFacts.
    stage_h: the taps RdsCore::init uploads per stage (oldest sample first); lp, matched: y[i] = sum_k h[k] x[i - k]"""
    lines = subprocess.run([_design_exe()], input=("%.17g\n" % rate).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    vecs, stages, taps, sh = {}, [], [], []
    for ln in lines:
        w = ln.split()
        if w[0] == "design":
            stages.append(int(w[1])); taps.append(int(w[2]))
            continue
        v = np.array([float(t) for t in w[2:]])
        assert len(v) == int(w[1])
        if w[0] == "stage":
            sh.append(v)
        else:
            vecs[w[0]] = v
    sc = vecs["scalars"]
    assert int(sc[11]) == len(stages)
    for v in sh + list(vecs.values()):
        v.setflags(write=False)
    return RdsDesignFacts(float(rate), sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], tuple(sc[6:11]), tuple(stages), tuple(taps), tuple(sh), vecs["lp"], vecs["matched"],
                          vecs["hilbert"][:61], vecs["hilbert"][61:], vecs["amp"])


def rds_min_call(des):
    """RdsCore::check restated: the shortest multiple of D whose length in front of every stage is at least that stage's tap count"""
    D = 1 << len(des.stages)
    n = D
    while any((n >> j) < len(h) for j, h in enumerate(des.stage_h)):
        n += D
    return n


# ------------------------------------------------------------------------------------------------
# rows: P.Demod(64000, rate, CAP), DM_FMS, against oracle.DemodWFM(rate)
# ------------------------------------------------------------------------------------------------
# stages: (design, taps) per decimate-by-2 stage; mtaps: matched filter; rds_min: RdsCore::check's shortest call.  All pinned by the host
# tier against rds_design(rate).  mb is the shortest call the handle takes: rds_min, or WfmCore::run's 80 (common.h kMaxTaps, the rule
# tests/demod_cases.py covers) rounded up to a multiple of D where that is more -- at 125 000 only (72 -> 80).
RdsRow = namedtuple("RdsRow", "name rate stages D rds_rate mtaps rds_min mb groups why")


def _row(rate, stages, rds_rate, mtaps, rds_min, groups, why):
    D = 1 << len(stages)
    mb = max(rds_min, -(-MIN_CALL // D) * D)
    return RdsRow("rds-%d" % rate, rate, stages, D, rds_rate, mtaps, rds_min, mb, groups, why)


RDS_ROWS = [
    _row(100000, ((4, 23), (11, 51)), 25000.0, 42, 104, 24, "two stages, the 51-tap design 11; the shortest matched filter but one"),
    _row(125000, ((3, 19), (7, 35)), 31250.0, 52, 72, 24, "two stages; the RDS chain would take 72 samples, the WFM demodulator takes 80"),
    _row(256000, ((2, 15), (3, 19), (7, 35)), 32000.0, 52, 144, 24, "three stages (the chain the equal-call tests run at 250 000)"),
    _row(312500, ((2, 15), (3, 19), (5, 27)), 39062.5, 64, 112, 24, "three stages, design 5, the longest matched filter"),
    _row(384000, ((1, 11), (2, 15), (4, 23), (11, 51)), 24000.0, 40, 416, 24, "four stages, the fixed 11-tap design 1 in front, design 11 last"),
    _row(512000, ((1, 11), (2, 15), (3, 19), (7, 35)), 32000.0, 52, 288, 24, "four stages, the highest rate the one-kernel WFM rows cover"),
]
ROW_BY_RATE = {r.rate: r for r in RDS_ROWS}
ALL_STAGE_DESIGNS = (1, 2, 3, 4, 5, 7, 11)

# a script entry: (length, accepted).  Refused entries consume no input.
Call = namedtuple("Call", "n ok")


def _cycle(row):
    D, mb = row.D, row.mb
    c = [4096, mb, mb, 3 * mb + D, 2048, mb + D, CAP - D, mb, 1024 + 3 * D, 4096]
    return [n - n % D for n in c]


def refused_lengths(row):
    """below the shortest call, not a multiple of D, above the capacity"""
    return [row.mb - row.D, 2048 + row.D // 2 + 1, CAP + row.D]


def rds_script(row, n_input):
    """The cycle 4096, mb, mb, 3 mb + D, 2048, mb + D, 8192 - D, mb, 1024 + 3 D, 4096 (each rounded down to a multiple of D) until the
    input is used up; one call of exactly the capacity behind the first cycle; the three refused calls between valid calls of the first
    cycle (behind its calls 2, 5 and 8: short after short, long after short, short after the longest)."""
    cyc, out, used, k = _cycle(row), [], 0, 0
    ref = dict(zip((2, 5, 8), refused_lengths(row)))
    while True:
        n = cyc[k % len(cyc)]
        if used + n > n_input:
            break
        out.append(Call(n, True)); used += n; k += 1
        if k in ref:
            out.append(Call(ref[k], False))
        if k == len(cyc) and used + CAP <= n_input:
            out.append(Call(CAP, True)); used += CAP
    return out


def equal_script(n_input, blk=4096):
    return [Call(blk, True)] * (n_input // blk)


def offsets(script):
    """[(offset, n)] of the accepted calls"""
    out, at = [], 0
    for c in script:
        if c.ok:
            out.append((at, c.n)); at += c.n
    return out


def _as_uploaded(x):
    """both sides are handed the same single-precision samples, the step's upload format"""
    x = x.astype(np.complex64).astype(np.complex128)
    x.setflags(write=False)
    return x


def _n_for(groups, rate, lead_bits=40, tail_bits=20):
    return int(rate * (groups * 104 + lead_bits + tail_bits) / 1187.5)


# ------------------------------------------------------------------------------------------------
# input A: geometry
# ------------------------------------------------------------------------------------------------
# At 384 000 the reference's decoder finds no block A in a multiplex at fm_multiplex's default levels (24 000 Hz behind the chain, 20
# samples per bit): the row and the 384 000 receiver get a stronger subcarrier under quieter audio, on which it decodes 19 of 24 groups.
A_LEVELS = {384000: dict(rds_level=0.2, audio_level=0.1)}


@functools.lru_cache(maxsize=None)
def input_a(row):
    """a broadcast multiplex of row.groups groups, the subcarrier 14 Hz off three times the pilot (the loop's residual rotation keeps
    m_RdsData moving through its zero crossings)"""
    g = rs.make_groups(row.groups, seed=11)
    return _as_uploaded(rs.fm_multiplex(g, float(row.rate), _n_for(row.groups, row.rate), subcarrier_offset_hz=-14.0, **A_LEVELS.get(row.rate, {})))


def script_a(row):
    return rds_script(row, len(input_a(row)))


# ------------------------------------------------------------------------------------------------
# input B: the block synchroniser's error paths, at 256 000
# ------------------------------------------------------------------------------------------------
B_RATE, B_GROUPS, B_LEAD = 256000, 40, 40
B_ONE_BIT = (5, 8)            # groups with one wrong bit in block C (bit 60 and bit 55 of the group's 104: information bits)
B_BURST = 11                  # a group with bits 30 .. 32 (block B) wrong
B_NOISE = range(16, 24)       # eight groups of random bits
B_TRIPLE = 31                 # this group is sent three times (31, 32, 33)
B_DAMAGED = tuple(B_ONE_BIT) + (B_BURST,)


def groups_b():
    g = rs.make_groups(B_GROUPS, seed=31)
    g[B_TRIPLE + 1] = g[B_TRIPLE + 2] = g[B_TRIPLE]
    return g


def _alter_b(bits):
    at = lambda k, b: B_LEAD + 104 * k + b  # noqa: E731
    bits[at(B_ONE_BIT[0], 60)] ^= 1
    bits[at(B_ONE_BIT[1], 55)] ^= 1
    for b in (30, 31, 32):
        bits[at(B_BURST, b)] ^= 1
    lo, hi = at(B_NOISE[0], 0), at(B_NOISE[-1] + 1, 0)
    bits[lo:hi] = np.random.default_rng(77).integers(0, 2, hi - lo)
    return bits


@functools.lru_cache(maxsize=None)
def input_b():
    n = _n_for(B_GROUPS, B_RATE, B_LEAD)
    return _as_uploaded(rs.fm_multiplex(groups_b(), float(B_RATE), n, subcarrier_offset_hz=-14.0, alter=_alter_b, lead_bits=B_LEAD))


def scripts_b():
    """the two call patterns: equal 4096-sample calls, and the 256 000 row's mixed script (without its refused calls)"""
    n = len(input_b())
    return {"equal": equal_script(n), "mixed": [c for c in rds_script(ROW_BY_RATE[B_RATE], n) if c.ok]}


# ------------------------------------------------------------------------------------------------
# input C: the 100-entry queue overrun, at 256 000
# ------------------------------------------------------------------------------------------------
C_RATE, C_GROUPS, C_CALL, C_CALLS = 256000, 190, 65536, 65


@functools.lru_cache(maxsize=None)
def input_c():
    g = rs.make_groups(C_GROUPS, seed=41)
    x = rs.fm_multiplex(g, float(C_RATE), C_CALL * C_CALLS, subcarrier_offset_hz=-14.0)
    return _as_uploaded(x)


def groups_c():
    return rs.make_groups(C_GROUPS, seed=41)


# ------------------------------------------------------------------------------------------------
# the oracle over a script, shared by the tests of a tier
# ------------------------------------------------------------------------------------------------
OracleRun = namedtuple("OracleRun", "audio data bits locks popped pushed")


def run_oracle(oracle_mod, rate, x, script, pop=True):
    """oracle.DemodWFM(rate) in dmFMS over the accepted calls -> OracleRun: per call the audio, m_RdsData, the lock flag; the bit
    sequence; what Demod::fmStereo's one getNextRdsGroupData per call popped [((a, b, c, d), changed)]; the groups pushed per call"""
    ref = oracle_mod.DemodWFM(float(rate))
    audio, data, locks, popped, pushed = [], [], [], [], []
    for o, n in offsets(script):
        a, lk = ref.process_stereo(x[o:o + n])
        audio.append(a); locks.append(lk)
        data.append(ref.rds_last()[0])
        pushed.append([tuple(int(v) for v in g) for g in ref.rds_pushed()])
        if pop:
            p = ref.next_rds_group()
            if p is not None:
                popped.append(p)
    return OracleRun(audio, data, ref.rds_bits(), locks, popped, pushed)
