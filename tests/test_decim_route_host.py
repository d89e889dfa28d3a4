"""CPU tier of a decimator call's route: plan_decim_shape() and plan_decim_route() of csrc/decim_route.h, compiled here with g++.

 - over every distinct chain of the ladder sweep, crossed with bank sizes, stream layouts and call kinds, the planner agrees field for
   field with decim_cases.route(), the independent statement of the rule that the GPU tier compares kernel_name() with: this is what
   ties that statement to the code DecimCore::run runs,
 - the facts route() does not model (the two tuning switches, the 32-bit offset limits, the lean front's edge launch and raw formats,
   the empty chain's two routes and their hand-over) select what DESIGN.md section 4, "Routes of a decimator call", says,
 - the shape of each of the nine k_mix_dec_mfma instances carries FusedDecGeom's figures, written out here.
"""
import os
import subprocess

import pytest

from tests import decim_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")

TUNING = ["no_fused_dec", "bank_dec"]
FACTS = ["n", "shared_input", "transient", "lds_free", "raw_fmt", "mix_in_consumer", "in_aligned", "out_pitch", "lean_edge_launch", "ovl_pending"]
SHAPE = ["zero_stage", "bank_front", "wide", "fused_front", "wide_stride", "nst", "three2", "fused_all", "bank_mfma", "bank_np", "fused_hy", "bank_nstate",
         "bank_minw", "xh_depth", "outb", "lds_half", "casc_lds_bytes", "halo0", "later", "total"]
ROUTE = ["front", "len0", "len1", "len_out", "transient", "uniform", "cl_log2", "R", "grid_x", "grid_y", "raw_fmt", "edge_launch", "cg", "rest", "cascade_inst",
         "tiles", "ovl_from_row", "ovl_pending"]
# enum class DecimFront / DecimRest, in the header's order
NONE, IN_CONSUMER, MIXER, BANK_MFMA, FUSED, CIC_HB, LEAN, HB11_BANK, DEC1, IN_SPECTRUM = range(10)
REST_NONE, FIR_DEC, CASCADE, FIR_DEC_CASCADE = range(4)
CASCADE_INST = ["k_cascade<0,0,0>", "k_cascade<15,23,47>", "k_cascade<15,19,31>"]

MAIN = """#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "decim_route.h"
int main()
{
    char line[4096];
    while (std::fgets(line, sizeof(line), stdin)) {
        pg::DecimStageDesc st[pg::kMaxCascade + 1];
        int ns = 0;
        long long C = 1;
        pg::DecimTuningFacts t;
        pg::DecimCallFacts f;
        for (char *tok = std::strtok(line, " \\n"); tok; tok = std::strtok(nullptr, " \\n")) {
            char *eq = std::strchr(tok, '=');
            if (!eq) return 2;
            *eq = 0;
            if (!std::strcmp(tok, "chain")) {  // T:S/T:S/... ("-": no stage)
                for (char *p = eq + 1; *p && *p != '-';) {
                    if (ns > pg::kMaxCascade) return 2;
                    st[ns].ntaps = (int)std::strtol(p, &p, 10);
                    if (*p++ != ':') return 2;
                    st[ns++].stride = (int)std::strtol(p, &p, 10);
                    if (*p == '/') p++;
                }
                continue;
            }
            long long v = 0;
            if (std::sscanf(eq + 1, "%%lld", &v) != 1) return 2;
            bool known = !std::strcmp(tok, "C");
            if (known) C = v;
%s
            if (!known) { std::fprintf(stderr, "unknown fact %%s\\n", tok); return 3; }
        }
        const pg::DecimShape s = pg::plan_decim_shape(st, ns, (unsigned)C, t);
        const pg::DecimRoute r = pg::plan_decim_route(s, f);
%s
        std::printf("%%d %%d|%%s|%%s\\n", (int)s.front_is_lds_free(), (int)s.raw_front(), r.front_name(), r.rest_name());
    }
    return 0;
}
"""


def chain_text(chain):
    return "/".join("%d:%d" % (t, s) for t, s in chain) or "-"


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("decim_route")
    src = d / "route.cpp"
    sets = "\n".join('            if (!std::strcmp(tok, "%s")) { %s.%s = (decltype(%s.%s))v; known = true; }' % (k, o, k, o, k)
                     for o, names in (("t", TUNING), ("f", FACTS)) for k in names)
    prints = "\n".join('        std::printf("%%lld ", (long long)%s.%s);' % (o, k) for o, names in (("s", SHAPE), ("r", ROUTE)) for k in names)
    src.write_text(MAIN % (sets, prints))
    exe = str(d / "route")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])

    def plan(rows):
        """rows: a list of (chain, {C / tuning fact / call fact: value}); returns one (shape dict, route dict) per row"""
        text = "".join("chain=%s %s\n" % (chain_text(ch), " ".join("%s=%d" % (k, int(v)) for k, v in facts.items())) for ch, facts in rows)
        out = subprocess.check_output([exe], input=text, text=True).strip().split("\n")
        assert len(out) == len(rows)
        res = []
        for line in out:
            nums, front_name, rest_name = line.split("|")
            v = [int(x) for x in nums.split()]
            assert len(v) == len(SHAPE) + len(ROUTE) + 2
            s = dict(zip(SHAPE, v))
            r = dict(zip(ROUTE, v[len(SHAPE):]))
            s["front_is_lds_free"], s["raw_front"] = v[-2:]
            r["front_name"], r["rest_name"] = front_name, rest_name
            res.append((s, r))
        return res

    def one(chain, **facts):
        return plan([(chain, facts)])[0]

    one.many = plan
    return one


def as_route(chain, s, r, n_out):
    """the planner's answer in the form of decim_cases.Route (dec1_branch: route()'s own name for a branch inside k_mix_dec1, not planned)"""
    tf = lambda b: "true" if b else "false"
    triple = tuple(t for t, _ in chain[len(chain) - s["nst"]:])
    front = r["front"]
    inst = {BANK_MFMA: "k_mix_dec_mfma<%d,%s>" % (s["bank_np"], ",".join(str(t) for t in triple)), FUSED: "k_mix_dec_fused<15,19,31>",
            CIC_HB: "k_mix_cic_hb<%s,%s>" % (tf(r["transient"]), tf(r["uniform"])), LEAN: "k_mix_hb11_lean<%d>" % r["raw_fmt"],
            HB11_BANK: "k_mix_hb11_bank<%s,%s>" % (tf(r["transient"]), tf(r["uniform"])), DEC1: "k_mix_dec1"}[front]
    casc = r["rest"] in (CASCADE, FIR_DEC_CASCADE)
    assert r["len_out"] == n_out
    return dc.Route(r["front_name"], r["rest_name"], inst, r["cl_log2"] if front in (CIC_HB, HB11_BANK) else None, None, r["rest"] in (FIR_DEC, FIR_DEC_CASCADE),
                    CASCADE_INST[r["cascade_inst"]] if casc else None, s["nst"], s["outb"] if casc else None, r["tiles"],
                    n_out - (r["tiles"] - 1) * s["outb"] if casc else 0)


COMPARED = ("front", "front_inst", "cl_log2", "rest", "fir_dec", "cascade_inst", "nst", "outb", "tiles", "last_tile")
BANK_SIZES = (1, 2, 15, 16, 17, 33, 64, 65)


def call_lengths(chain):
    """final outputs per call: a call of 63 * 1024 input samples rounded down to a whole number of outputs (15 outputs at the deepest
    chains, thousands at the shallowest: on both sides of k_mix_dec_mfma's 64-output minimum), 63 and 64 themselves, and a frame"""
    return sorted({max(1, 63 * 1024 // dc.decimation(chain)), 63, 64, dc.FRAME})


def test_the_planner_is_the_restated_rule_over_the_ladder(oracle_mod, planner):
    """every distinct chain of the ladder sweep x bank size x stream layout x lds_free x transient x call length: a disagreement is a
    finding about one of the two statements (cores.hip at the parent commit is the authority)"""
    chains = [list(ch) for ch in dc.ladder_chains(oracle_mod) if ch]
    rows, want = [], []
    for ch in chains:
        D = dc.decimation(ch)
        for C in BANK_SIZES:
            for shared in (True, False):
                for lds_free in (False, True):
                    for transient in (False, True):
                        for n_out in call_lengths(ch):
                            rows.append((ch, dict(C=C, n=n_out * D, shared_input=shared, lds_free=lds_free, transient=transient, out_pitch=n_out + 2048)))
                            want.append((dc.route(ch, C, shared, lds_free, transient, n_out), n_out))
    got = planner.many(rows)
    bad = []
    for (ch, facts), (s, r), (w, n_out) in zip(rows, got, want):
        g = as_route(ch, s, r, n_out)
        if any(getattr(g, k) != getattr(w, k) for k in COMPARED):
            bad.append((ch, facts, g, w))
    print("chains %d, calls compared %d, disagreements %d" % (len(chains), len(rows), len(bad)))
    assert not bad, bad[:3]
    # (k_mix_dec_fused: calls of fewer than 64 outputs behind hb11 x S, hb15, hb19, hb31 only)
    assert len(chains) >= 40 and {r["front"] for _, r in got} == {BANK_MFMA, FUSED, CIC_HB, LEAN, HB11_BANK, DEC1}
    assert {r["front"] for (ch, f), (_, r) in zip(rows, got) if f["n"] // dc.decimation(ch) >= 64} == {BANK_MFMA, CIC_HB, LEAN, HB11_BANK, DEC1}


def test_lds_free_front_is_what_the_rows_assume(oracle_mod, planner):
    chains = [list(ch) for ch in dc.ladder_chains(oracle_mod) if ch]
    rows = [(ch, dict(C=C, n=dc.decimation(ch))) for ch in chains for C in BANK_SIZES]
    for (ch, facts), (s, _) in zip(rows, planner.many(rows)):
        row = dc._row("x", 0, facts["C"], "", spectrum_bins=8192)
        assert bool(s["front_is_lds_free"]) == dc.lds_free_call(row, ch), (ch, facts)
        assert s["total"] == dc.decimation(ch)


# chains of the ladder by the matrix instance a bank takes behind them (tests/bank_cases.py names rates for each)
HB4 = lambda t: [(11, 4)] + [(x, 2) for x in t]
CIC12 = lambda t: [(0, 4), (11, 16)] + [(x, 2) for x in t]
BANK = dict(C=33, shared_input=1, out_pitch=4096)


def chain_of(inst):
    return (CIC12 if inst[0] == 12 else HB4)(inst[1:])


def test_the_two_switches(planner):
    """PEBBLEGPU_NO_FUSED_DEC=1: no one-kernel route; PEBBLEGPU_BANK_DEC=0: k_mix_dec_fused exactly for (4, 15, 19, 31)"""
    for inst in sorted(dc.bank_instances()):
        ch = chain_of(inst)
        n = 2048 * dc.decimation(ch)
        s, r = planner(ch, n=n, **BANK)
        assert (r["front"], s["bank_mfma"], s["bank_np"]) == (BANK_MFMA, 1, inst[0]), inst
        s, r = planner(ch, n=n, no_fused_dec=1, **BANK)
        assert r["front"] == (CIC_HB if inst[0] == 12 else HB11_BANK) and not s["fused_all"] and not s["bank_mfma"], inst
        assert (s["xh_depth"], s["fused_hy"]) == (16, 0)
        s, r = planner(ch, n=n, bank_dec=0, **BANK)
        assert r["front"] == (FUSED if inst == (4, 15, 19, 31) else CIC_HB if inst[0] == 12 else HB11_BANK), inst
        assert s["fused_all"] == (inst == (4, 15, 19, 31)) and not s["bank_mfma"]
    # ... and the four-wave kernel's own grid: a workgroup per 64 channels
    _, r = planner(HB4((15, 19, 31)), n=2048 * 32, bank_dec=0, **dict(BANK, C=65))
    assert (r["front"], r["grid_y"], r["rest"], r["front_name"], r["rest_name"]) == (FUSED, 2, REST_NONE, "k_mix_dec_fused", "")


def test_what_leaves_the_matrix_route(planner):
    ch, other = HB4((15, 19, 31)), HB4((15, 23, 47))
    n = 2048 * 32
    assert planner(ch, n=n, **BANK)[1]["front"] == BANK_MFMA
    # an input pointer off its 8-byte alignment, an output or an input past the 32-bit byte offsets, fewer than 64 outputs, a transient,
    # streams of their own: the predecessor where it exists, the two-kernel route elsewhere
    limit = 0xFFF00000
    for change in (dict(in_aligned=0), dict(out_pitch=limit // (8 * 33) + 1), dict(n=63 * 32), dict(n=(limit // 8 // 32 + 1) * 32)):
        assert planner(ch, **{**BANK, "n": n, **change})[1]["front"] == FUSED, change
        assert planner(other, **{**BANK, "n": n, **change})[1]["front"] == HB11_BANK, change
    assert planner(ch, **dict(BANK, n=n, out_pitch=limit // (8 * 33)))[1]["front"] == BANK_MFMA
    assert planner(ch, **dict(BANK, n=64 * 32))[1]["front"] == BANK_MFMA
    for change in (dict(transient=1), dict(shared_input=0)):
        assert planner(ch, **{**BANK, "n": n, **change})[1]["front"] in (HB11_BANK, DEC1), change


def test_the_lean_front(planner):
    ch = [(11, 8), (15, 2), (23, 2), (47, 2)]
    n = 2048 * 64
    base = dict(C=1, n=n, lds_free=1, shared_input=1)
    s, r = planner(ch, **base)
    assert (r["front"], r["raw_fmt"], r["edge_launch"], r["R"], r["len0"]) == (LEAN, -1, 0, 8, n // 8) and s["raw_front"]
    assert r["grid_x"] == -(-(n // 8) // (4 * 8 * 64)) + 1  # (one more workgroup for the edges)
    assert (r["rest"], r["cascade_inst"], r["front_name"], r["rest_name"]) == (CASCADE, 1, "k_mix_hb11_lean", "k_cascade")
    _, e = planner(ch, lean_edge_launch=1, **base)
    assert (e["front"], e["edge_launch"], e["grid_x"]) == (LEAN, 1, r["grid_x"] - 1)
    for fmt in range(8):  # every raw format has its instance; an unknown one takes the last
        _, x = planner(ch, raw_fmt=fmt, **base)
        assert (x["front"], x["raw_fmt"]) == (LEAN, min(fmt, 4)), fmt
    # inside a transient, or when the call keeps LDS: not this kernel
    assert planner(ch, **dict(base, transient=1))[1]["front"] == HB11_BANK
    assert planner(ch, **dict(base, lds_free=0))[1]["front"] == DEC1
    # a bank has no raw front
    assert not planner(ch, **dict(base, C=33))[0]["raw_front"]


def test_the_empty_chain(planner):
    """k_mixer or the mixing band-pass, and the hand-over of the mixed overlap between them in both directions"""
    s, r = planner([], C=3, n=4096)
    assert (s["zero_stage"], s["front_is_lds_free"], s["raw_front"], s["nst"], s["total"]) == (1, 1, 0, 0, 1)
    assert (r["front"], r["front_name"], r["rest_name"], r["len_out"], r["grid_x"], r["grid_y"], r["rest"]) == (MIXER, "k_mixer", "", 4096, 4, 3, REST_NONE)
    pending, seen = 0, []
    for mix in (0, 1, 1, 0, 0, 1):
        _, r = planner([], C=3, n=4096, mix_in_consumer=mix, ovl_pending=pending)
        assert r["front"] == (IN_CONSUMER if mix else MIXER)
        assert r["front_name"] == ("k_fastfir_t128 (mixing)" if mix else "k_mixer")
        seen.append((mix, r["ovl_from_row"], r["ovl_pending"]))
        pending = r["ovl_pending"]
    # (mixes in the consumer, the overlap in front of the call lies in the consumer's row, ... and behind the call)
    assert seen == [(0, 0, 0),   # k_mixer: its tail job refreshes buf0's head-room
                    (1, 0, 1),   # the consumer behind k_mixer reads that head-room and leaves its own row
                    (1, 1, 1),   # ... which the next such call reads
                    (0, 1, 0),   # k_mixer behind the consumer first copies the row into the head-room
                    (0, 0, 0),
                    (1, 0, 1)]


@pytest.mark.parametrize("inst", sorted(dc.bank_instances()))
def test_the_shape_of_every_matrix_instance(planner, inst):
    """FusedDecGeom<T1, T2, T3> written out: halo = (T1 - 1) + 2 (T2 - 1) + 4 (T3 - 1) first-stage outputs, HY = 8 (halo / 8) + 8,
    running sums (T1 + 1) / 2 + 3, (T2 + 1) / 2 + 1, (T3 + 1) / 2; the cascade tile by init's 48 KiB rule"""
    np_, t1, t2, t3 = inst
    ch = chain_of(inst)
    s, _ = planner(ch, n=2048 * dc.decimation(ch), **BANK)
    halo = (t1 - 1) + 2 * (t2 - 1) + 4 * (t3 - 1)
    hy = 8 * (halo // 8) + 8
    assert s["fused_hy"] == hy and s["halo0"] == max(halo, hy) == hy
    assert s["bank_nstate"] == ((t1 + 1) // 2 + 3) + ((t2 + 1) // 2 + 1) + (t3 + 1) // 2
    assert s["bank_minw"] == dc.bank_instances()[inst]
    assert s["xh_depth"] == (512 if np_ == 12 else 16)
    outb, c0, c1 = dc.cascade_outb(ch[-3:])
    assert (s["outb"], s["lds_half"], s["casc_lds_bytes"]) == (outb, c0, 8 * (c0 + c1)) and outb == 256
    assert (s["nst"], s["three2"], s["later"], s["wide"], s["fused_front"], s["wide_stride"]) == (3, 1, 8, np_ == 12, np_ == 12, 16 if np_ == 12 else 1)
    # without the one-kernel routes the head-room is the cascade's own look-back
    assert planner(ch, n=2048 * dc.decimation(ch), no_fused_dec=1, **BANK)[0]["halo0"] == halo


def test_the_grid_of_every_general_front(oracle_mod, planner):
    """what route() does not model of the launches: channels across a wave's lanes, outputs per lane and the grid of k_mix_cic_hb and
    k_mix_hb11_bank (the rule the two share, over the outputs of the hb11 stage), k_mix_dec1's and k_cascade's, written out here"""
    cdiv = lambda a, b: -(-a // b)
    chains = [list(ch) for ch in dc.ladder_chains(oracle_mod) if ch]
    forced = [[(0, 4), (27, 2)], [(0, 2), (15, 2)], [(0, 4), (15, 8), (19, 2)]]  # CIC3 fronts no rate gives: k_mix_dec1's channel groups, the peeled wide stage
    rows = [(ch, dict(C=C, n=n_out * dc.decimation(ch), shared_input=shared, lds_free=C == 1, transient=transient))
            for ch in chains + forced for C in BANK_SIZES for shared in (1, 0) for transient in (1, 0) for n_out in (1, 257, dc.FRAME)]
    seen = set()
    for (ch, f), (s, r) in zip(rows, planner.many(rows)):
        C, n = f["C"], f["n"]
        len0 = n // ch[0][1]
        assert r["len0"] == len0 and r["len_out"] == n // dc.decimation(ch), (ch, f)
        if r["front"] in (CIC_HB, HB11_BANK):
            outs = len0 // ch[1][1] if r["front"] == CIC_HB else len0
            cl = min(6, (C - 1).bit_length())
            R = 16 if cl == 6 else 8
            assert (r["cl_log2"], r["R"], r["grid_x"], r["grid_y"]) == (cl, R, cdiv(outs + 1, 4 * R * (64 >> cl)), cdiv(C, 1 << cl)), (ch, f)
            assert r["len1"] == (outs if r["front"] == CIC_HB else 0)
        elif r["front"] == DEC1:
            cg = 8 if ch[0][0] == 0 and ch[0][1] > 2 and f["shared_input"] else 1
            assert (r["cg"], r["grid_x"], r["grid_y"]) == (cg, cdiv(len0, 256), cdiv(C, cg)), (ch, f)
            assert r["len1"] == (len0 // ch[1][1] if r["rest"] in (FIR_DEC, FIR_DEC_CASCADE) else 0)
        elif r["front"] == LEAN:
            assert (r["R"], r["grid_x"], r["grid_y"]) == (8, cdiv(len0, 4 * 8 * 64) + 1, 1), (ch, f)
        if r["rest"] in (CASCADE, FIR_DEC_CASCADE):
            assert r["tiles"] == cdiv(r["len_out"], s["outb"]), (ch, f)
        seen.add((r["front"], r["cg"], r["rest"]))
    assert {(DEC1, 8, CASCADE), (DEC1, 1, CASCADE), (DEC1, 8, FIR_DEC_CASCADE), (CIC_HB, 1, CASCADE), (HB11_BANK, 1, CASCADE), (LEAN, 1, CASCADE)} <= seen
