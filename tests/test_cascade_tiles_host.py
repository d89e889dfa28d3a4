"""CPU tier of k_cascade's tiles: the plan of csrc/decim_route.h (plan_decim_shape, plan_decim_route, cascade_fixed_tile and the
four-plane index map of the fixed-tap instances), compiled here with g++ and walked for every chain of the ladder sweep of
tests/decim_cases.py, its rows' chains, the headline's (hb11 x 8, 15, 23, 47) and configs[2]'s (hb11 x 4, 15, 19, 31).

Every chain with a cascade:
  - the tile's input count (lds_half) against a brute-force walk of the stages, and the first intermediate's;
  - LDS bytes within the plan's budget: 48 KiB for the generic form;
  - tiles * outb >= outputs, and the last tile's counts, for calls of outb - 1, outb, outb + 1 and 3 outb + 2 outputs.
Every chain the fixed-tap form is planned for (three stages at stride 2), the same and:
  - LDS bytes within kCascadeFixedLdsCap (32 KiB: five workgroups per CU's 160 KiB, what the generic form's 27.4 KiB gave), at 256
    work-items of 55 registers a workgroup, neither of which binds before LDS does;
  - a ragged last tile's loads end exactly where the call's data ends and start inside the head-room (halo0);
  - the index map is a bijection of the tile into its buffer, for the tile and both intermediates, with the slack slot the last
    work-item's unused second window reaches inside the buffer;
  - every LDS access of the tile load and the three stages is conflict-free: loads and stage outputs under the 8-byte store rule,
    window and centre reads under BOTH read rules of tests/test_lds_exchange_banks_host.py (the compiler emits the reads as a mix of
    single and pair reads), enumerated in that file's style: the worst group degree of every instruction of every wave.

Not here: the issue's "all tiles of the one-channel headline call resident at once".  That piece (a tile small enough for eight
workgroups per CU, or half as many tiles of twice the size) was not built: the tile stays 256 outputs, five workgroups per CU, 1280
resident of the headline's 2048.
"""
import os
import subprocess

import pytest

from tests import decim_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")

HEADLINE = ((11, 8), (15, 2), (23, 2), (47, 2))
CONFIGS2 = ((11, 4), (15, 2), (19, 2), (31, 2))

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
#include "decim_route.h"
using namespace pg;

// worst group degree of one wave64 instruction: lane l touches the two dwords at slot[l] * 2 (tests/test_lds_exchange_banks_host.py)
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
static int worst_single, worst_pair;
// one instruction of a 256-work-item workgroup; slot_of(t): float2 slot of work-item t
template <class F> static void instr(F slot_of)
{
    for (int w = 0; w < 4; w++) {
        int slot[64];
        for (int l = 0; l < 64; l++) slot[l] = slot_of(64 * w + l);
        const int a = degree(slot, 32, 64), b = degree(slot, 16, 32);
        worst_single = a > worst_single ? a : worst_single;
        worst_pair = b > worst_pair ? b : worst_pair;
    }
}
static void take(int &single, int &pair)
{
    single = worst_single;
    pair = worst_pair;
    worst_single = worst_pair = 0;
}

int main()
{
    char line[4096];
    while (std::fgets(line, sizeof(line), stdin)) {
        DecimStageDesc st[kMaxCascade + 1];
        int ns = 0;
        char *p = line;
        long long C = std::strtoll(p, &p, 10), n_out = std::strtoll(p, &p, 10);
        while (*p == ' ') p++;
        while (*p && *p != '\n' && *p != '-') {
            if (ns > kMaxCascade) return 2;
            st[ns].ntaps = (int)std::strtol(p, &p, 10);
            if (*p++ != ':') return 2;
            st[ns++].stride = (int)std::strtol(p, &p, 10);
            if (*p == '/') p++;
        }
        const DecimShape s = plan_decim_shape(st, ns, (unsigned)C, DecimTuningFacts{});
        DecimCallFacts f;
        f.n = n_out * s.total;
        const DecimRoute r = plan_decim_route(s, f);
        std::printf("nst=%d three2=%d outb=%d lds_half=%d lds=%zu fixed_lds=%zu halo0=%lld later=%lld cascade=%d inst=%d tiles=%u cap=%d", s.nst, (int)s.three2, s.outb,
                    s.lds_half, s.casc_lds_bytes, s.casc_fixed_lds_bytes, s.halo0, s.later, (int)r.cascade(), r.cascade_inst, r.tiles, kCascadeFixedLdsCap);
        if (s.three2) {
            const int *T = s.casc_ntaps;
            const CascadeFixedTile g = cascade_fixed_tile(s.outb, T[0], T[1], T[2]);
            const long long o_last = (long long)(r.tiles - 1) * s.outb;
            const CascadeFixedTile last = cascade_fixed_tile((int)(n_out - o_last), T[0], T[1], T[2]);
            std::printf(" c0=%d c1=%d c2=%d pa=%d pb=%d tile_lds=%d last_c0=%d last_c1=%d last_c2=%d last_first=%lld first0=%lld", g.c0, g.c1, g.c2, g.pitch_a, g.pitch_b,
                        g.lds_bytes, last.c0, last.c1, last.c2, cascade_fixed_first(o_last, T[0], T[1], T[2]), cascade_fixed_first(0, T[0], T[1], T[2]));
            // the index map: distinct slots inside the buffer for the counts + the slack input
            const int cnt[3] = {g.c0, g.c1, g.c2}, pitch[3] = {g.pitch_a, g.pitch_b, g.pitch_a};
            int bij = 1;
            for (int b = 0; b < 3; b++) {
                std::set<int> seen;
                for (int i = 0; i <= cnt[b]; i++) {
                    const int sl = cascade_plane_slot(i, pitch[b]);
                    if (sl < 0 || sl >= 4 * pitch[b] || !seen.insert(sl).second) bij = 0;
                    if (sl != cascade_plane_base(i & 3, pitch[b]) + (i >> 2)) bij = 0;
                }
            }
            std::printf(" bijection=%d", bij);
            // the tile load: lane v of a sweep stores inputs 2v and 2v + 1 (every sweep: v0 a multiple of 256)
            int a, b;
            for (int v0 = 0; 2 * v0 < g.c0; v0 += 256)
                for (int h = 0; h < 2; h++) instr([&](int t) { return cascade_plane_slot(2 * (v0 + t) + h, g.pitch_a); });
            take(a, b);
            std::printf(" load_store=%d", b);
            // the stages: work-item u = t + 256 * sweep makes outputs 2u, 2u + 1 of `outs` from (TT + 3) / 2 even inputs and two centres
            const int outs[3] = {g.c1, g.c2, s.outb};
            for (int sg = 0; sg < 3; sg++) {
                const int TT = T[sg], CC = (TT - 1) / 2, NE = (TT + 3) / 2, qs = pitch[sg], qd = pitch[(sg + 1) % 3];
                for (int u0 = 0; 2 * u0 < outs[sg]; u0 += 256) {
                    for (int k = 0; k < NE; k++) instr([&](int t) { return cascade_plane_base((2 * k) & 3, qs) + (u0 + t) + (k >> 1); });
                    for (int rr = 0; rr < 2; rr++) instr([&](int t) { return cascade_plane_base((CC + 2 * rr) & 3, qs) + (u0 + t) + ((CC + 2 * rr) >> 2); });
                }
                take(a, b);
                std::printf(" read%d_single=%d read%d_pair=%d", sg, a, sg, b);
                // ... and these are the inputs the outputs want
                int ok = 1;
                for (int u = 0; 2 * u < outs[sg]; u++) {
                    for (int k = 0; k < NE; k++) ok &= cascade_plane_base((2 * k) & 3, qs) + u + (k >> 1) == cascade_plane_slot(4 * u + 2 * k, qs);
                    for (int rr = 0; rr < 2; rr++) ok &= cascade_plane_base((CC + 2 * rr) & 3, qs) + u + ((CC + 2 * rr) >> 2) == cascade_plane_slot(2 * (2 * u + rr) + CC, qs);
                }
                std::printf(" window%d=%d", sg, ok);
                if (sg < 2) {
                    for (int u0 = 0; 2 * u0 < outs[sg]; u0 += 256)
                        for (int rr = 0; rr < 2; rr++) instr([&](int t) { return cascade_plane_slot(2 * (u0 + t) + rr, qd); });
                    take(a, b);
                    std::printf(" store%d=%d", sg, b);
                }
            }
        }
        std::printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    d = tmp_path_factory.mktemp("cascade_tiles")
    src = d / "tiles.cpp"
    src.write_text(MAIN)
    exe = str(d / "tiles")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])

    def plan(rows):
        """rows: [(chain, C, n_out)] -> one dict of the program's figures per row"""
        text = "".join("%d %d %s\n" % (C, n_out, "/".join("%d:%d" % ts for ts in ch) or "-") for ch, C, n_out in rows)
        out = subprocess.check_output([exe], input=text, text=True).strip().split("\n")
        assert len(out) == len(rows)
        return [{k: int(v) for k, v in (tok.split("=") for tok in line.split())} for line in out]

    return plan


@pytest.fixture(scope="module")
def chains(oracle_mod):
    found = {tuple(tuple(s) for s in ch) for ch in dc.ladder_chains(oracle_mod) if ch}
    for row in dc.ROWS:
        found.add(tuple(oracle_mod.Decimator(row.fs, dc.protect_bw(row)).chain()))
    for row in dc.STEP_ROWS:
        found.add(tuple(oracle_mod.Decimator(row.fs, row.bw).chain()))
    found |= {HEADLINE, CONFIGS2}
    return sorted(ch for ch in found if ch)


def cascade_of(chain):
    """the stages k_cascade fuses (decim_cases.route's rule: a wide second stage is peeled off)"""
    wide = len(chain) >= 3 and chain[1][1] >= 8 and chain[1][0] > 0
    return list(chain[2:] if wide else chain[1:])


def walk(casc, o0, n):
    """brute force: the inputs of each stage that final outputs o0 .. o0 + n - 1 touch, as index sets, outermost first
    (y_s[j] = sum_p y_{s-1}[j S + p - (T - 1)] h[p]); a stage's span runs through the end of its last output's stride, S - 1 inputs
    past the last one read, so that the tiles of a row abut and every span is a whole number of sample pairs"""
    need = [set(range(o0, o0 + n))]
    for t, s in reversed(casc):
        touched = {j * s + p - (t - 1) for j in need[-1] for p in range(t)}
        assert max(touched) == max(need[-1]) * s
        need.append(touched | set(range(max(touched), max(touched) + s)))
    need.reverse()
    for x in need:
        assert len(x) == max(x) - min(x) + 1  # (contiguous: counts are spans)
    return need


def test_every_chain_is_planned_as_the_stages_say(tiles, chains):
    """input counts, LDS budgets, tiles x outb >= outputs and the last tile's counts"""
    rows = [(ch, C, n_out) for ch in chains for C in (1, 3) for n_out in (255, 256, 257, 3 * 256 + 2)]
    got = tiles(rows)
    fixed, generic = set(), set()
    for (ch, C, n_out), g in zip(rows, got):
        casc = cascade_of(ch)
        assert g["nst"] == len(casc), ch
        if not casc:
            assert not g["cascade"]
            continue
        outb = g["outb"]
        assert outb == 256 and n_out in (outb - 1, outb, outb + 1, 3 * outb + 2)
        need = walk(casc, 0, outb)
        assert g["lds_half"] == len(need[0]) and g["lds"] == 8 * (len(need[0]) + len(need[1])) <= 48 * 1024, ch
        assert g["halo0"] >= -min(need[0]) == sum((t - 1) * p for (t, _), p in zip(casc, [dc.decimation(casc[:k]) for k in range(len(casc))]))
        assert g["tiles"] * outb >= n_out > (g["tiles"] - 1) * outb, (ch, n_out)
        three2 = len(casc) == 3 and all(s == 2 for _, s in casc)
        assert g["three2"] == three2
        triple = tuple(t for t, _ in casc)
        assert g["inst"] == ({(15, 23, 47): 1, (15, 19, 31): 2}.get(triple, 0) if three2 else 0)
        if not three2:
            generic.add(ch)
            assert g["fixed_lds"] == 0
            continue
        fixed.add(triple)
        assert (g["c0"], g["c1"], g["c2"]) == tuple(len(x) for x in need[:3]), ch
        assert g["fixed_lds"] == g["tile_lds"] == 8 * 4 * (g["pa"] + g["pb"]) <= g["cap"] == 32 * 1024, ch
        assert 5 * g["fixed_lds"] <= 160 * 1024
        # the buffers hold the counts and the slack input, plane by plane
        assert g["pa"] >= -(-(g["c0"] + 1) // 4) and g["pb"] >= -(-(g["c1"] + 1) // 4) and g["pa"] % 16 == 8 and g["pb"] % 16 == 8
        # the last tile: its counts by the walk, its loads from inside the head-room to the end of the call's data and no further
        o_last = (g["tiles"] - 1) * outb
        last = walk(casc, o_last, n_out - o_last)
        assert (g["last_c0"], g["last_c1"], g["last_c2"]) == tuple(len(x) for x in last[:3]), (ch, n_out)
        assert g["last_first"] == min(last[0]) and g["last_first"] + g["last_c0"] == n_out * g["later"] == max(last[0]) + 1, (ch, n_out)
        assert g["first0"] == min(need[0]) >= -g["halo0"] and g["last_first"] % 2 == 0 and g["last_c0"] % 2 == 0  # (16-byte loads)
    print("chains %d, fixed-tap triples %s, generic cascades %d" % (len(chains), sorted(fixed), len(generic)))
    assert {(15, 23, 47), (15, 19, 31)} <= fixed and generic


def test_the_four_plane_map_is_a_bijection_and_the_windows_are_the_inputs(tiles, chains):
    rows = [(ch, 1, 256) for ch in chains]
    seen = 0
    for (ch, _, _), g in zip(rows, tiles(rows)):
        if g["three2"]:
            seen += 1
            assert g["bijection"] == 1 and g["window0"] == g["window1"] == g["window2"] == 1, ch
    assert seen >= 2


ACCESSES = ("load_store", "read0_single", "read0_pair", "store0", "read1_single", "read1_pair", "store1", "read2_single", "read2_pair")


@pytest.mark.parametrize("access", ACCESSES)
def test_every_lds_access_is_conflict_free(tiles, chains, access):
    """worst group degree over every instruction of every wave of every sweep, at every three-stage chain: 1"""
    rows = [(ch, 1, 256) for ch in chains]
    worst = {ch: g[access] for (ch, _, _), g in zip(rows, tiles(rows)) if g["three2"]}
    print(access, "degree", sorted(set(worst.values())), "over", len(worst), "chains")
    assert HEADLINE in worst and CONFIGS2 in worst
    assert set(worst.values()) == {1}, {ch: d for ch, d in worst.items() if d != 1}


def test_the_per_output_form_is_two_way_conflicted():
    """why the planes: the form this replaced read src + 2 j + p, consecutive lanes 16 bytes apart -- 32 lanes over 64 slots of 8
    bytes, two on every bank under the single-read rule (and 16 lanes over 32 slots under the pair rule)"""
    for group, banks in ((32, 64), (16, 32)):
        for p in range(0, 47, 2):
            on = {}
            for lane in range(group):
                for d in range(2):
                    on.setdefault((2 * (2 * lane + p) + d) % banks, set()).add(2 * (2 * lane + p) + d)
            assert max(len(v) for v in on.values()) == 2
