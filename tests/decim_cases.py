"""The coverage statement for the general decimator routes (csrc/kernels_frontend.h: k_mix_dec1, k_mix_hb11_bank, k_mix_hb11_lean,
k_mix_cic_hb, k_fir_dec as the peeled second stage, k_cascade): what DecimCore::run (csrc/cores.hip) launches when the call is not one
k_mix_dec_mfma launch.  One table of rows, used by the CPU tier (tests/test_decimator_routes_host.py: every row's chain is the
oracle's, its route is what route() -- the rule of csrc/decim_route.h stated on its own below -- says, the union of the rows reaches what this
statement claims, a plain fp64 model agrees with the oracle and nine deliberately wrong models cannot pass) and by the GPU tier
(tests/test_decimator_routes_gpu.py: the same rows through P.ReceiverBank at the POST_MIXER tap, and the step rows through
P.Decimator, against the oracle).  No row sets an environment switch, no kernel is launched directly.

Reached (instance: rows, by the host tier's union check):
  k_mix_dec1, halfband loop         first stages hb27, hb19, hb15 (stride 2) and hb11 x 2, 4, 8, 16, 32; C = 1, 2, 5, 15; WFM C = 3;
                                    17 independent streams on an (11,4) chain (a bank of >= 16 falls to it per channel)
  k_mix_hb11_bank<false,false>      cl_log2 4 (C = 16), 5 (C = 17, 32): steady state of banks whose triple has no matrix instance
  k_mix_hb11_bank<false,true>       C = 33, 64, 65 (scalar loads), strides 2, 4, 8 and 32
  k_mix_hb11_bank<true,false>       cl_log2 0 (one channel beside the display transform, call 0), 4, 5: call 0
  k_mix_hb11_bank<true,true>        C = 33, 64, 65: call 0
  k_mix_hb11_lean<-1>               strides 2, 8, 32: calls 1.. of the one-channel rows with spectrum_bins = 8192
  k_mix_cic_hb<false,false>         cl_log2 0 .. 5 (C = 1, 2, 3, 8/9, 16, 17), S0 = 2, 4, 8, 16, 32, S1 = 16 and 32; 17 independent
                                    streams (in + c * in_pitch; cl_log2 5 there, and 6 without the scalar loads is NOT a row: 33 streams
                                    at 10 Msps is 70 M samples a run)
  k_mix_cic_hb<false,true>          C = 33, 65 at 16 Msps, C = 33 behind (0,2),(11,32)
  k_mix_cic_hb<true,false|true>     call 0 of each of those, and the call behind the retune of cic-16M-c17-retune
  k_cascade<15,19,31>               behind k_mix_dec1, k_mix_hb11_bank, k_mix_hb11_lean and k_mix_cic_hb
  k_cascade<15,23,47>               100 Msps narrow (cic-s0x16), 200 Msps
  k_cascade<0,0,0>                  nst = 1 ((19,2),(31,2); WFM 1 Msps), 2 (500 kHz; WFM 2.048 Msps), 3 ((15,23,59), (15,27,59),
                                    (19,27,59), (15,23,51) ...), behind a bank (bank-1.4M-*, bank-2.8M-*) too; nst = 0 is the single-stage
                                    rows, whose first-stage buffer is the output and whose first.gain is the gain restore
  k_cascade tiles                   every receiver call is a multiple of 2048 outputs and outb (init's rule) is 256 for every chain the
                                    ladder produces, so NO receiver row has a last tile shorter than outb; the P.Decimator step rows
                                    (1, 3, 255, 257, 513 outputs) have
Unreachable through the ladder (the host tier sweeps 60 kHz .. 250 MHz at both bandwidths and asserts this list; no row forces them):
  k_mix_dec1's two CIC3 paths (merged, cg = 8 or 1; S = 2) and the `wide && !fused_front` launch of k_fir_dec: every CIC3 front is
  followed by hb11 x 16 or x 32, so fused_front always holds and k_mix_cic_hb takes the call.  A wide second stage occurs only there.
Every row is compared at the tap (rel-RMS on the channels plan() lists: all of them up to 4 Msps, the group edges above); none had to go behind the band-pass (the tap leaves the kernel names as route() predicts them).

Bar: rel-RMS <= TOL = 1e-5 per 2048-output frame of every call, the first included, against the oracle's Mixer -> Decimator times
the receiver's gain restore (10^(2 stages / 20) narrow, 1 for WFM as receiver.cpp has it).  Step rows: per 256 consecutive outputs of
the concatenated stream (a call of one or three outputs alone would hold fp32 against a sample that may lie near zero).

Inputs.  Every frequency is a multiple of df = fs / (Q * 2048 * D), Q = the run's super-frames (3 or 7, a prime), so a call's input is
synthesised on its own by inverse FFTs and every tone falls on a bin of the Q * 2048-point FFT of the run's output.  Channel c is
tuned to fc_idx[c] * df (channel `zero` to exactly 0 Hz, the mixer's pass-through; no other index is a multiple of Q, so an oscillator
whose phase restarts at a call shows at every call start) and carries one tone bins[c] steps from its centre, spread over +-0.45 of
the output rate: most lie outside +-15 kHz, where only the last stage's transition band shapes them.  One more tone, the sentinel,
sits (the first halfband's output rate - bandwidth / 4) above channel 0: in that stage's stop band when its stride is 2, it folds to
-bandwidth / 4, inside every later stage's pass band, if the stage's taps or stride are wrong (a merged hb11 x S lets it through as
it does the other channels; behind a CIC3 it sits 0.06 .. 0.28 of the input rate up instead, see plan()); its level is raised where
the first halfband's outer tap is small (see plan()).
Peak check, on EVERY channel of every row (a lane that received another channel's data shows no tone of its own): the largest bin of
the FFT of the channel's whole run is its own tone's.  The hb11 and CIC3 first stages do not reject the other channels
over the whole output band (one 11-tap halfband at stride S, none at all when merged; at stride 2 its stop band covers +-15 kHz of the
output only, and with 15 and 33 channels the oracle itself shows a neighbour above the channel's own tone at dec1-hb11x2 and
bank-700k-c33): their tones fold into a channel near full level, each on a bin the plan predicts; on those rows the check leaves the
predicted bins out and asks that the largest of all the others is the channel's own.  Behind a longer first halfband (hb15 .. hb27 at
stride 2: the rows below 1.024 Msps and the WFM rows) nothing is left out.  The host tier holds the oracle's own output to the same check on every channel.
Each wrong model runs on the first modelled channel it applies to (channel 0 where it can); last-group-clamped runs on every modelled
channel of the last group but the last one.

Measured by the host tier (printed there; rel-RMS per frame, worst over rows, calls and modelled channels):
  plain fp64 model against the oracle: 6.6e-9 at the worst row (cic-s0x32: the oracle's oscillator is a recurrence over 25 M samples,
  the model's a closed form); 3e-10 and under at every other row (bar / 100 = 1e-7)
  smallest miss of each wrong model, in bars, over every row and call it applies to:
    history zeroed at a call start 3808, history one sample off 2337, one outer tap of the first halfband dropped 195 (dec1-single-stage),
    the neighbouring channel's oscillator 116276, phase restarted per call 86777, gain restore one stage short 20567, stride-32 front
    computed as stride 16 122545, last channel group's lanes clamped to the last channel 117056, CIC3 pair order swapped 5237
Measured by the GPU tier on an MI355X (worst rel-RMS per 2048-output frame of each row, bar 1e-5): 1.6e-6 at dec1-single-stage and
dec1-wfm-1M (the two rows whose sentinel is raised 31 times: its fp32 rounding), 1.5e-7 .. 1.1e-6 at every other row; the step rows
7e-8 .. 1.4e-7 per 256 outputs.  No row failed: the routes that had never run on a device compute what the oracle computes.
"""
from collections import namedtuple
import functools
import os
import re

import numpy as np

from tests.signals import lcg_noise, lcg_uniform

TOL = 1e-5     # BASELINE.json north_star, as tests/test_parity_gpu.py
MARGIN = 100   # tests/demod_cases.py's margin
FRAME = 2048   # outputs per super-frame (narrow: lcm(2048, 2048 - 1024); WFM: the frame itself)
STEP_CHUNK = 256
K_FRONT_T1 = 11   # common.h kFrontT1
K_AMP_TAB = 512   # common.h kAmpTab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")


# ------------------------------------------------------------------------------------------------
# what the sources say: halfband taps (hb_taps.inc) and k_mix_dec_mfma's instances (decim_route.h PG_BANK_DEC_INSTANCES)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def halfband_taps():
    """ntaps -> fp64 taps of csrc/hb_taps.inc"""
    text = open(os.path.join(CSRC, "hb_taps.inc")).read()
    out = {}
    for m in re.finditer(r'\{ "hb(\d+)", (\d+), [0-9.]+, \{([^}]*)\} \}', text):
        h = np.array([float(v) for v in m.group(3).split(",")])
        assert len(h) == int(m.group(2)) == int(m.group(1))
        out[len(h)] = h
    return out


@functools.lru_cache(maxsize=None)
def bank_instances():
    """{(NP, T1, T2, T3): MINW} of PG_BANK_DEC_INSTANCES in csrc/decim_route.h: the one list the planner looks a chain up in and
    cores.hip instantiates k_mix_dec_mfma from.  The only reader of that list on the test side."""
    text = open(os.path.join(CSRC, "decim_route.h")).read()
    body = text[text.index("#define PG_BANK_DEC_INSTANCES(X)"):]
    body = body[:body.index("\n\n")]
    found = [tuple(int(v) for v in m) for m in re.findall(r"\bX\((\d+), (\d+), (\d+), (\d+), (\d+)\)", body)]
    assert len(found) == len({f[:4] for f in found}) and body.count("X(") == len(found), body  # (every entry read, none twice)
    return {f[:4]: f[4] for f in found}


def bank_variants():
    """{(NP, T1, T2, T3)} of that list"""
    return frozenset(bank_instances())


_ladder = {}


def ladder_rates():
    """every rate 60 kHz .. 250 MHz in 0.1 % steps, the rows' rates and the round rates"""
    return sorted({int(60000 * 1.001 ** k) for k in range(8340)} | {r.fs for r in ROWS} | {k * 100_000 for k in range(1, 2501)})


def ladder_chains(oracle_mod):
    """{chain: (first rate, bandwidth) that gives it} over ladder_rates() at both bandwidths (computed once per session)"""
    if not _ladder:
        for bw in (30000, 200000):
            for fs in ladder_rates():
                _ladder.setdefault(tuple(oracle_mod.Decimator(fs, bw).chain()), (fs, bw))
    return _ladder


# ------------------------------------------------------------------------------------------------
# The route of a DecimCore::run call, stated here on its own for a chain with at least one stage and the default tuning.  The library
# plans it in csrc/decim_route.h (plan_decim_shape, plan_decim_route); tests/test_decim_route_host.py holds the two to each other over
# the whole ladder, the GPU tier holds kernel_name() to this one.
# ------------------------------------------------------------------------------------------------
Route = namedtuple("Route", "front rest front_inst cl_log2 dec1_branch fir_dec cascade_inst nst outb tiles last_tile")


def cascade_outb(casc):
    """init: the largest power-of-two tile of final outputs whose two ping-pong buffers fit 48 KiB -> (outb, c0, c1)"""
    outb = 256
    while True:
        c0, c1 = outb, 0
        for t, s in reversed(casc):
            c1 = c0
            c0 = c0 * s + t - 1
        if (c0 + c1) * 8 <= 48 * 1024 or outb == 1:
            return outb, c0, c1
        outb //= 2


def route(chain, C, shared_input, lds_free, transient, n_out):
    """the kernels one DecimCore::run call of n_out final outputs launches.  lds_free: DecimCall::lds_free as the receiver sets it
    (lds_free_call()); transient: OscBank::any_transient() at the call"""
    chain = [tuple(s) for s in chain]
    ns = len(chain)
    assert ns >= 1
    t0, s0 = chain[0]
    cic3 = t0 == 0
    bank_front = (not cic3) and t0 == K_FRONT_T1 and (C >= 16 or C == 1)
    wide = ns >= 3 and chain[1][1] >= 8 and chain[1][0] > 0
    fused_front = wide and cic3 and chain[1][0] == K_FRONT_T1
    casc = chain[2:] if wide else chain[1:]
    nst = len(casc)
    three2 = nst == 3 and all(s == 2 for _, s in casc)
    hb_front = bank_front and C >= 16 and not wide and s0 <= 16
    cic_front = fused_front and C >= 16 and chain[1][1] == 16
    triple = tuple(t for t, _ in casc)
    fused_all = hb_front and three2 and triple == (15, 19, 31)
    bank_mfma = three2 and (hb_front or cic_front) and ((12 if cic_front else 4,) + triple) in bank_variants()
    if (fused_all or bank_mfma) and shared_input and not transient:
        if bank_mfma and n_out >= 64:  # (the 32-bit offset limits hold for every row here)
            return Route("k_mix_dec_mfma", "", "k_mix_dec_mfma<%d,%d,%d,%d>" % ((12 if cic_front else 4,) + triple), None, None, False, None, nst, None, 0, 0)
        if fused_all:
            return Route("k_mix_dec_fused", "", "k_mix_dec_fused<15,19,31>", None, None, False, None, nst, None, 0, 0)
    cl_log2 = 0
    while (1 << cl_log2) < C and cl_log2 < 6:
        cl_log2 += 1
    tf = lambda b: "true" if b else "false"
    branch, fir_dec = None, False
    if fused_front:
        uni = cl_log2 == 6 and shared_input
        front, inst, cl = "k_mix_cic_hb", "k_mix_cic_hb<%s,%s>" % (tf(transient), tf(uni)), cl_log2
    else:
        if bank_front and C == 1 and lds_free and not transient:
            front, inst, cl = "k_mix_hb11_lean", "k_mix_hb11_lean<-1>", None
        elif bank_front and (shared_input if C >= 16 else lds_free):
            front, inst, cl = "k_mix_hb11_bank", "k_mix_hb11_bank<%s,%s>" % (tf(transient), tf(cl_log2 == 6)), cl_log2
        else:
            front, inst, cl = "k_mix_dec1", "k_mix_dec1", None
            branch = ("cic3-merged-cg%d" % (8 if shared_input else 1)) if (cic3 and s0 > 2) else "cic3-s2" if cic3 else "halfband"
        fir_dec = wide
    rest = "k_fir_dec" if fir_dec else ""
    cinst, outb, tiles, last = None, None, 0, 0
    if nst > 0:
        rest = "k_fir_dec + k_cascade" if fir_dec else "k_cascade"
        cinst = "k_cascade<15,23,47>" if three2 and triple == (15, 23, 47) else "k_cascade<15,19,31>" if three2 and triple == (15, 19, 31) else "k_cascade<0,0,0>"
        outb = cascade_outb(casc)[0]
        tiles = -(-n_out // outb)
        last = n_out - (tiles - 1) * outb
    return Route(front, rest, inst, cl, branch, fir_dec, cinst, nst, outb, tiles, last)


# ------------------------------------------------------------------------------------------------
# the rows
# ------------------------------------------------------------------------------------------------
Row = namedtuple("Row", "name fs wfm C shared_input spectrum_bins calls retune_before why")
SCRIPT = (1, 2, 1, 3)   # super-frames per call (max_superframes = 3) on rows up to 20 Msps; (1, 1, 1) above


def _row(name, fs, C, why, wfm=False, shared=True, spectrum_bins=0, retune_before=None):
    return Row(name, fs, wfm, C, shared, spectrum_bins, SCRIPT if fs <= 20_000_000 else (1, 1, 1), retune_before, why)


ROWS = [
    # ---- k_mix_dec1, halfband first stage ----
    _row("dec1-single-stage", 140_000, 1, "[(27,2)]: buf0 is the output, first.gain = last_gain, no cascade"),
    _row("dec1-two-stage", 250_000, 2, "[(19,2),(31,2)]: casc.nst == 1"),
    _row("dec1-hb15x2", 500_000, 5, "(15,2) front, two more stages: the generic k_cascade with nst = 2"),
    _row("dec1-hb11x2", 1_024_000, 15, "(11,2) front, 15 channels: under a bank's 16, k_cascade<15,19,31>"),
    _row("dec1-hb11x4", 1_400_000, 1, "(11,4) front, one channel without a spectrum; (15,23,59) behind: generic k_cascade, nst = 3"),
    _row("dec1-hb11x8", 2_800_000, 2, "(11,8) front"),
    _row("dec1-hb11x16", 5_000_000, 5, "(11,16) front: the widest stride the LDS tile saw before"),
    _row("dec1-hb11x32", 9_800_000, 15, "(11,32) front: the tile of 256 * 32 + 10 samples"),
    _row("dec1-wfm-1M", 1_000_000, 3, "WFM [(27,2),(59,2)]: gain 1, nst = 1", wfm=True),
    _row("dec1-wfm-2048k", 2_048_000, 3, "WFM [(15,2),(27,2),(59,2)]: three stages, neither fixed-tap k_cascade", wfm=True),
    _row("dec1-17-streams-hb11x4", 2_048_000, 17, "17 independent streams: bank_front holds but the streams are not shared", shared=False),
    _row("cic-17-streams", 10_000_000, 17, "17 independent streams behind CIC3: k_mix_cic_hb reads in + c * in_pitch", shared=False),
    # ---- k_mix_hb11_bank in steady state: triples with no matrix instance ----
    _row("bank-1.4M-c16", 1_400_000, 16, "(11,4),(15,23,59): cl_log2 4"),
    _row("bank-2.8M-c17", 2_800_000, 17, "(11,8),(15,23,59): cl_log2 5, 17 live lanes of 32"),
    _row("bank-2.95M-c32", 2_950_000, 32, "(11,8),(15,23,51): cl_log2 5, a full group"),
    _row("bank-700k-c33", 700_000, 33, "(11,2),(15,23,59): scalar loads, stride 2 (outputs 0 .. 4 reach into the history)"),
    _row("bank-1.4M-c64", 1_400_000, 64, "scalar loads, one full group of 64"),
    _row("bank-2.8M-c65", 2_800_000, 65, "scalar loads, a second group with one live lane"),
    _row("bank-hb11x32-c33", 9_800_000, 33, "(11,32) front: hb_front needs stride <= 16, so the bank never leaves the general route"),
    _row("lean-x2", 1_024_000, 1, "one channel beside the 8192-bin transform: k_mix_hb11_bank (cl_log2 0) in the transient, then k_mix_hb11_lean", spectrum_bins=8192),
    _row("lean-x8", 2_800_000, 1, "the same at stride 8", spectrum_bins=8192),
    _row("lean-x32", 9_800_000, 1, "the same at stride 32", spectrum_bins=8192),
    # ---- k_mix_cic_hb: every cl_log2 at 16 Msps ((0,2),(11,16),(15,19,31): no matrix instance behind a CIC3) ----
    _row("cic-16M-c1", 16_000_000, 1, "cl_log2 0"),
    _row("cic-16M-c2", 16_000_000, 2, "cl_log2 1"),
    _row("cic-16M-c3", 16_000_000, 3, "cl_log2 2, three live lanes of four"),
    _row("cic-16M-c8", 16_000_000, 8, "cl_log2 3, full"),
    _row("cic-16M-c9", 16_000_000, 9, "cl_log2 4"),
    _row("cic-16M-c16", 16_000_000, 16, "cl_log2 4, full: a bank, general route in steady state"),
    _row("cic-16M-c17-retune", 16_000_000, 17, "cl_log2 5; a channel retuned before the third call: the transient instance again", retune_before=2),
    _row("cic-16M-c33", 16_000_000, 33, "scalar loads"),
    _row("cic-16M-c65", 16_000_000, 65, "scalar loads, a second group with one live lane"),
    # ---- k_mix_cic_hb: every S0, and S1 = 32 ----
    _row("cic-s0x2", 10_000_000, 3, "S0 = 2"),
    _row("cic-s0x4", 20_000_000, 2, "S0 = 4"),
    _row("cic-s0x8", 40_000_000, 3, "S0 = 8"),
    _row("cic-s0x16", 100_000_000, 2, "S0 = 16, k_cascade<15,23,47>"),
    _row("cic-s0x32", 200_000_000, 2, "S0 = 32"),
    _row("cic-hb11x32-c1", 19_500_000, 1, "(0,2),(11,32): cic_front needs wide_stride == 16"),
    _row("cic-hb11x32-c33", 19_500_000, 33, "(0,2),(11,32) with scalar loads"),
    _row("cic-wfm-95M-c17", 95_000_000, 17, "WFM bank near 100 Msps whose triple (15,19,39) has no matrix instance (96 .. 104 Msps have one)", wfm=True),
]


def protect_bw(row):
    return 200000 if row.wfm else 30000


def decimation(chain):
    return int(np.prod([s for _, s in chain]))


def lds_free_call(row, chain):
    """plan_call_route (csrc/call_route.h): the call runs beside the display transform when there is one and the decimator's first
    kernel can leave LDS alone (DecimCore::front_is_lds_free); nothing else that decides it is set by any row"""
    t0 = chain[0][0]
    fused_front = len(chain) >= 3 and t0 == 0 and chain[1][1] >= 8 and chain[1][0] == K_FRONT_T1
    bank_front = t0 == K_FRONT_T1 and (row.C >= 16 or row.C == 1)
    return row.spectrum_bins > 0 and row.C == 1 and (fused_front or bank_front)


def transient_call(row, k):
    """a super-frame is longer than the oscillators' 512-sample amplitude transient: only the first call of a handle and the call
    behind a retune find an oscillator inside it"""
    return k == 0 or k == row.retune_before


def routes(row, chain):
    """-> [Route] per call"""
    return [route(chain, row.C, row.shared_input, lds_free_call(row, chain), transient_call(row, k), row.calls[k] * FRAME) for k in range(len(row.calls))]


def gain_restore(row, chain):
    """receiver.cpp:935-938: "restore gain lost in decimation", 2 dB per halving, on the narrow branch only"""
    return 1.0 if row.wfm else 10 ** (2 * int(round(np.log2(decimation(chain)))) / 20.0)


# ------------------------------------------------------------------------------------------------
# tunings, tones, inputs
# ------------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "D Q P1 period NB df zero fc_idx bins tone_idx retuned extra_fc_idx extra_bin sentinel_idx sentinel_amp amp "
                          "drop_stage compare merged")


def drop_stage(chain):
    """the stage whose outer tap the dropped-tap model leaves out: the first halfband"""
    return 1 if chain[0][0] == 0 else 0


def plan(row, chain):
    C, D = row.C, decimation(chain)
    Q = sum(row.calls)
    assert Q in (3, 7)
    P1 = FRAME * D
    period, NB = Q * P1, Q * FRAME
    df = row.fs / period
    zero = C // 2 if C > 1 else None
    spacing = int(round(0.7 * period / (C + 2)))

    def tune(k):  # carrier k places from channel `zero`; never a multiple of Q away from it
        i = k * spacing if C > 1 else int(round(0.17 * period))
        return i + 1 if i % Q == 0 and i != 0 else i
    fc_idx = [tune(c - (zero or 0)) for c in range(C)]
    extra_fc = tune(C + 1 - (zero or 0))
    assert max(abs(fc_idx[0]), abs(extra_fc)) * df < 0.47 * row.fs
    # own tones: golden-ratio spread over +-0.45 of the output rate, every tone's index distinct modulo NB, so that in every channel
    # every tone of the run lands on a bin of its own
    used, bins = set(), []

    def place(fc, u):
        b = int(round((-0.45 + 0.9 * u) * NB))
        while b == 0 or (fc + b) % NB in used:
            b += 1
        used.add((fc + b) % NB)
        return b
    sb = int(round(0.25 * protect_bw(row) / df))
    ds = drop_stage(chain)
    if chain[0][0] == 0:
        # behind a CIC3 (stride S0) the sentinel sits (k + 1/8) fs / S0 up, k = S0 // 4: a multiple of the merged front's output rate
        # (it folds to -bandwidth / 4), an eighth of the hb11's input rate after the CIC3 (which that halfband passes), and 0.06 ..
        # 0.28 of the input rate, so that the two samples of a pair differ by a good part of a turn: that is what shows a swapped
        # pair (the channels' own tones, close to 0 Hz at a pair, do not: 57 .. 87 bars without this tone)
        s0 = int(chain[0][1])
        sentinel = fc_idx[0] + (8 * (s0 // 4) + 1) * period // (8 * s0) - sb
    else:
        sentinel = fc_idx[0] + period // int(chain[0][1]) - sb  # (the first halfband's output rate, in steps of df)
    used.add(sentinel % NB)
    for c in range(C):
        bins.append(place(fc_idx[c], (0.37 + 0.6180339887 * c) % 1.0))
    extra_bin = place(extra_fc, 0.77)
    # the dropped-tap model leaves out h[0] of the first halfband: what it loses is h[0] times that stage's whole input, which must
    # come to 100 bars (1e-3) of the channel's output.  hb11's 6e-3 does that on any input; behind hb15 .. hb27 (1.4e-3 .. 6e-5) the
    # sentinel is raised to 2e-3 / h[0] times a channel's tone (31 times at hb27: fp32 rounding of the sentinel, 6e-8 of it, stays
    # under a fifth of the bar)
    h0 = abs(halfband_taps()[chain[ds][0]][0])
    ratio = max(1.0, 2e-3 / h0)
    amp = min(0.05, 0.5 / np.sqrt(C), 0.5 / ratio)
    retuned = None
    if row.retune_before is not None:
        retuned = (C // 2 + 5) % C
    if row.fs <= 4_000_000:
        compare = list(range(C))
    else:
        edges = {0, C - 1}
        for g in (8, 16, 32, 64):
            for e in range(g, C, g):
                edges |= {e - 1, e}
        pick = {int(u * C) for u in lcg_uniform(3, C)}
        compare = sorted(c for c in edges | pick | ({retuned} if retuned is not None else set()) | ({zero} if zero is not None else set()) if 0 <= c < C)
    return Plan(D, Q, P1, period, NB, df, zero, fc_idx, bins, [f + b for f, b in zip(fc_idx, bins)], retuned, extra_fc, extra_bin,
                sentinel, amp * ratio, amp, ds, compare, chain[0][0] == 0 or chain[0][0] == K_FRONT_T1)


def tone_table(row, p):
    """[(index, amplitude)] of every tone of the run"""
    t = [(i, p.amp) for i in p.tone_idx] + [(p.sentinel_idx, p.sentinel_amp)]
    if p.retuned is not None:
        t.append((p.extra_fc_idx + p.extra_bin, p.amp))
    return t


def own_bin(row, p, c):
    """bin of the Q * 2048-point FFT of the run's whole output on which channel c's own tone lies at the end of the run"""
    return (p.extra_bin if c == p.retuned else p.bins[c]) % p.NB


def foreign_bins(row, p, c):
    """the bins the peak check leaves out in channel c.  Behind an hb11 or CIC3 front: the bins on which the run's other
    tones land in the channel (wherever it was tuned during the run), at whatever level.  Behind a longer first halfband (hb15 .. hb59
    at stride 2), which does reject the other channels: none, so that a neighbour's tone leaking in shows"""
    if not p.merged:
        return []
    fcs = [p.fc_idx[c]] + ([p.extra_fc_idx] if c == p.retuned else [])
    own = (fcs[-1] + (p.extra_bin if c == p.retuned else p.bins[c]))
    return sorted({(i - f) % p.NB for i, _ in tone_table(row, p) for f in fcs if i != own} - {own_bin(row, p, c)})


def peak_bin(y, exclude):
    """the largest bin of the FFT of a channel's whole run, the listed bins left out"""
    s = np.abs(np.fft.fft(np.asarray(y, dtype=np.complex128)))
    s[list(exclude)] = 0.0
    return int(np.argmax(s))


def call_start(row, p, k):
    return sum(row.calls[:k]) * p.P1


def synth_tones(table, period, Q, start, n):
    """sum over (m, a) in table of a exp(2j pi m (start + i) / period), i = 0 .. n - 1, where period divides Q n: the tones whose
    Q n m / period is r mod Q are bins of an n-point inverse FFT, turned by the slow ramp exp(2j pi r i / (Q n))"""
    assert (Q * n) % period == 0
    j = Q * n // period
    spec = {}
    for m, a in table:
        q, r = divmod(m * j, Q)
        spec.setdefault(r, np.zeros(n, dtype=np.complex128))[q % n] += a * np.exp(2j * np.pi * ((m * start) % period) / period)
    x = np.zeros(n, dtype=np.complex128)
    base = np.exp(2j * np.pi * np.arange(n, dtype=np.float64) / (float(Q) * n))
    ramp = None
    for r in range(Q):  # (the ramp of residue r is the r-th power of the first: one product per residue instead of an exponential)
        if r in spec:
            y = np.fft.ifft(spec[r]) * n
            x += y * ramp if r else y
        ramp = base if ramp is None else ramp * base
    return x


def direct_tones(table, period, start, n):
    """synth_tones() evaluated tone by tone (the host tier compares the two)"""
    t = np.arange(n, dtype=np.int64) + start
    x = np.zeros(n, dtype=np.complex128)
    for m, a in table:
        x += a * np.exp(2j * np.pi * ((m * t) % period) / period)
    return x


def call_input(row, p, k):
    """the shared stream of call k alone: the run's tones over the call's samples + LCG noise of the call's own seed"""
    n = row.calls[k] * p.P1
    return synth_tones(tone_table(row, p), p.period, p.Q, call_start(row, p, k), n) + lcg_noise(n, 11 + k, 1e-3)


def stream_turn(row, c):
    """independent streams: stream c is the shared stream turned by a phase of its own, so a kernel that reads another channel's
    stream is off by that turn"""
    return 1.0 if row.shared_input else np.exp(2j * np.pi * (c + 1) / (row.C + 3.0))


# ------------------------------------------------------------------------------------------------
# the oracle of one channel
# ------------------------------------------------------------------------------------------------
class OracleChannel:
    """Mixer -> Decimator -> gain restore of channel c, fed whole super-frames, call by call"""

    def __init__(self, oracle_mod, row, p, c, chain):
        self.row, self.p, self.c = row, p, c
        self.mix = oracle_mod.Mixer(row.fs)
        self.mix.set_frequency(p.fc_idx[c] * p.df)
        self.dec = oracle_mod.Decimator(row.fs, protect_bw(row))
        assert self.dec.chain() == [tuple(s) for s in chain]
        self.gain = gain_restore(row, chain)

    def call(self, k, x):
        if k == self.row.retune_before and self.c == self.p.retuned:
            self.mix.set_frequency(self.p.extra_fc_idx * self.p.df)  # (Mixer::setFrequency starts the oscillator again)
        x = x * stream_turn(self.row, self.c)
        return np.concatenate([self.dec.process(self.mix.process(x[i:i + self.p.P1])) for i in range(0, len(x), self.p.P1)]) * self.gain


# ------------------------------------------------------------------------------------------------
# the plain fp64 model, and its deliberately wrong variants
# ------------------------------------------------------------------------------------------------
WRONG = ("zero-history", "history-one-off", "dropped-outer-tap", "neighbour-oscillator", "phase-restart", "gain-restore-short",
         "stride-32-as-16", "last-group-clamped", "cic3-pair-swapped")


@functools.lru_cache(maxsize=None)
def osc_amplitudes():
    """Mixer::processBlock's amplitude stabiliser in closed form: |osc| of the i-th sample after a retune, a_{i+1} = (1.95 - a_i^2) a_i
    from 1, settled at sqrt(0.95) long before K_AMP_TAB"""
    a = np.empty(K_AMP_TAB)
    v = 1.0
    for i in range(K_AMP_TAB):
        a[i] = v
        v = (1.95 - v * v) * v
    return a, float(np.sqrt(0.95))


def applies(wrong, row, p, chain, c, k):
    """does this wrong model differ from the right one at channel c, call k of the row?"""
    later = k >= 1
    fc = p.extra_fc_idx if (c == p.retuned and k >= row.retune_before) else p.fc_idx[c]
    if wrong in ("zero-history", "history-one-off"):
        return later
    if wrong == "dropped-outer-tap":
        return True
    if wrong == "neighbour-oscillator":
        return row.C >= 2
    if wrong == "phase-restart":
        # (the retuned channel's oscillator did restart at the call of the retune; a later start shows like any other)
        since = sum(row.calls[row.retune_before:k]) if (c == p.retuned and k >= row.retune_before) else sum(row.calls[:k])
        return later and fc != 0 and (fc * since) % p.Q != 0
    if wrong == "gain-restore-short":
        return not row.wfm
    if wrong == "stride-32-as-16":
        return any(s == 32 and t > 0 for t, s in chain)
    if wrong == "last-group-clamped":
        r = route(chain, row.C, row.shared_input, False, False, FRAME)
        return r.cl_log2 is not None and r.cl_log2 > 0 and c != row.C - 1 and (c >> r.cl_log2) == ((row.C - 1) >> r.cl_log2)
    if wrong == "cic3-pair-swapped":
        return chain[0][0] == 0
    raise ValueError(wrong)


class Model:
    """mixer -> each stage (y[o] = sum_p m[o S + p - (T - 1)] h[p]; CIC3 as decimator.cpp:719-737 merges it) -> gain restore, in fp64
    numpy, one channel, call by call"""

    def __init__(self, row, p, chain, c, wrong=None, mixed=None):
        """mixed: a dict the models of one row share, so that the mixer's output of a channel and call is computed once"""
        self.row, self.p, self.chain, self.c, self.wrong = row, p, [tuple(s) for s in chain], c, wrong
        self.mixed, self.k = mixed, None
        self.fc = p.fc_idx[c]
        self.origin, self.pos = 0, 0
        self.hist = [np.zeros(max(t - 1, 0), dtype=np.complex128) for t, _ in self.chain]
        self.pair = [0j, 0j]  # CIC3: m_xEven, m_xOdd
        self.gain = gain_restore(row, chain)
        if wrong == "gain-restore-short":
            self.gain /= 10 ** (2 / 20.0)

    def _osc_fc(self):
        C = self.row.C
        if self.wrong == "neighbour-oscillator":
            return self.p.fc_idx[self.c + 1 if self.c + 1 < C else self.c - 1]
        if self.wrong == "last-group-clamped":
            return self.p.fc_idx[C - 1]
        return self.fc

    def _mix(self, x, idx, what="all"):
        """the mixed samples at the call's sample indices idx"""
        if self.mixed is None:
            return self._mix_now(x, idx)
        key = (self.c, self._osc_fc(), self.wrong == "phase-restart", self.origin, self.k, what)
        if key not in self.mixed:
            self.mixed[key] = self._mix_now(x, idx)
        return self.mixed[key]

    def _mix_now(self, x, idx):
        fc = self._osc_fc()
        x = x[idx] * stream_turn(self.row, self.c)
        if fc == 0:
            return x  # mixer.cpp:48-52: frequency 0 passes the samples through
        since = idx + (self.pos - self.origin)
        ph_i = idx if self.wrong == "phase-restart" else since
        tab, a_inf = osc_amplitudes()
        amp = np.where(since < K_AMP_TAB, tab[np.minimum(since, K_AMP_TAB - 1)], a_inf)
        ph = ((-fc) * (ph_i + 1)) % self.p.period
        return amp * np.exp(2j * np.pi * ph / self.p.period) * x

    def call(self, k, x):
        row, p = self.row, self.p
        if k == row.retune_before and self.c == p.retuned:
            self.fc, self.origin = p.extra_fc_idx, self.pos
        n = len(x)
        self.k = k
        t0, s0 = self.chain[0]
        if t0 == 0:  # merged CIC3 reads the pair o S, o S + 1 only
            o = np.arange(n // s0, dtype=np.int64) * s0
            ev, od = self._mix(x, o, "even"), self._mix(x, o + 1, "odd")
            if self.wrong == "cic3-pair-swapped":
                ev, od = od, ev
            pe, po = self.pair
            if self.wrong == "zero-history" and k >= 1:
                pe, po = 0j, 0j
            pev, pod = np.concatenate([[pe], ev[:-1]]), np.concatenate([[po], od[:-1]])
            y = .125 * (od + pev + 3.0 * (pod + ev))
            self.pair = [ev[-1], od[-1]]
            rest = list(enumerate(self.chain))[1:]
        else:
            y = self._mix(x, np.arange(n, dtype=np.int64))
            rest = list(enumerate(self.chain))
        for s, (T, S) in rest:
            h = halfband_taps()[T].copy()
            if self.wrong == "dropped-outer-tap" and s == p.drop_stage:
                h[0] = 0.0
            hist = self.hist[s]
            if k >= 1 and self.wrong == "zero-history":
                hist = np.zeros_like(hist)
            if k >= 1 and self.wrong == "history-one-off":
                hist = np.concatenate([[0j], hist[:-1]])
            xx = np.concatenate([hist, y])
            self.hist[s] = xx[len(xx) - (T - 1):]
            nout = len(y) // S
            step = 16 if (self.wrong == "stride-32-as-16" and S == 32) else S
            acc = np.zeros(nout, dtype=np.complex128)
            for q in np.nonzero(h)[0]:
                acc += h[q] * xx[q:q + step * (nout - 1) + 1:step]
            y = acc
        self.pos += n
        return y * self.gain


def frame_errors(got, ref):
    """rel-RMS of every 2048-output frame of a call"""
    assert len(got) == len(ref) and len(ref) % FRAME == 0, (len(got), len(ref))
    g, r = np.asarray(got).reshape(-1, FRAME), np.asarray(ref).reshape(-1, FRAME)
    return np.sqrt(np.mean(np.abs(g - r) ** 2, axis=1)) / np.maximum(np.sqrt(np.mean(np.abs(r) ** 2, axis=1)), 1e-12)


def model_channels(row, p):
    """the channels the host tier models: the ends, the 0 Hz channel, the retuned one, the last but one (inside the last channel group)"""
    want = [0, row.C - 1, row.C - 2, p.zero, p.retuned]
    return sorted({c for c in want if c is not None and 0 <= c < row.C})


# ------------------------------------------------------------------------------------------------
# P.Decimator step rows
# ------------------------------------------------------------------------------------------------
StepRow = namedtuple("StepRow", "name fs bw why")
STEP_OUTPUTS = (1, 1, 3, 255, 256, 257, 1, 513)   # call lengths in outputs; n = outputs * total decimation
STEP_ROWS = [
    StepRow("step-single-stage", 140_000, 30000, "[(27,2)]: calls shorter than the stage's look-back keep part of the old history"),
    StepRow("step-hb11x8", 2_800_000, 30000, "(11,8) front; the cascade's look-back (15,23,59) is 290 first-stage outputs: seven of the calls are shorter"),
    StepRow("step-cic-s0x4", 20_000_000, 30000, "(0,4),(11,16): k_mix_cic_hb at cl_log2 0 with calls of one output"),
    StepRow("step-hb11x32", 9_800_000, 30000, "(11,32) front"),
    StepRow("step-wfm-2048k", 2_048_000, 200000, "[(15,2),(27,2),(59,2)]"),
]


def step_input(row, D):
    """three tones (in band, a quarter of the output rate up, far out of band) + noise; the step has no mixer"""
    n = sum(STEP_OUTPUTS) * D
    t = np.arange(n) / float(row.fs)
    out = row.fs / D
    x = 0.3 * np.exp(2j * np.pi * 1000.0 * t) + 0.2 * np.exp(1j * (2 * np.pi * (-0.26 * out) * t + 0.4)) + 0.2 * np.exp(2j * np.pi * (0.31 * row.fs) * t)
    return x + lcg_noise(n, 31 + STEP_ROWS.index(row), 1e-3)


def step_route(chain, n_out):
    """P.Decimator: one channel, its own stream, no display transform; the oscillator is off (frequency 0)"""
    return route(chain, 1, False, False, False, n_out)


def chunk_errors(got, ref, size=STEP_CHUNK):
    """rel-RMS per `size` consecutive outputs of the whole stream; a rest shorter than a quarter chunk joins the chunk before it"""
    assert len(got) == len(ref)
    k = len(ref) // size
    b = [(i * size, (i + 1) * size) for i in range(k)]
    rest = len(ref) - k * size
    if rest and 4 * rest < size and b:
        b[-1] = (b[-1][0], len(ref))
    elif rest:
        b.append((k * size, len(ref)))
    return [float(np.sqrt(np.mean(np.abs(got[lo:hi] - ref[lo:hi]) ** 2)) / max(np.sqrt(np.mean(np.abs(ref[lo:hi]) ** 2)), 1e-12)) for lo, hi in b]
