"""CPU tier of the k_mix_dec_mfma coverage table (tests/bank_cases.py): every instance the library's list ships has a multi-group
row, every row reaches the instance and the chunk geometry it claims (bank_geometry() of csrc/bank_geom.h, compiled here with
g++), the table as a whole covers the strides, chunk lengths and launch shapes it is there for, and the oracle puts every
compared channel's peak into the bin the lane-mapping check of the GPU tier expects."""
import os
import subprocess

import numpy as np
import pytest

from tests import bank_cases as B
from tests import decim_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")


def shipped_variants():
    """{(NP, T1, T2, T3): MINW} of the library's instance list (csrc/decim_route.h)"""
    return dict(decim_cases.bank_instances())


@pytest.fixture(scope="module")
def chains(oracle_mod):
    return {r.name: oracle_mod.Decimator(r.fs, B.protect_bw(r)).chain() for r in B.ROWS}


@pytest.fixture(scope="module")
def geometry(tmp_path_factory, chains):
    """{(row name, call): (waves, L, pairs, n_wg)} of every k_mix_dec_mfma call of the table, by the library's own function with
    the default tuning fields (bank_waves 0, fused_l <= 0, four history workgroups per quad of channel groups)"""
    d = tmp_path_factory.mktemp("bank_geom")
    src = d / "geom.cpp"
    src.write_text('#include <cstdio>\n#include "bank_geom.h"\n#include "tuning.h"\n'
                   'int main()\n{\n    long long len_out, C;\n    int cic, warm, minw, fin2;\n    pg::Tuning t;\n    t.fused_l = -16;  // what read_tuning() leaves with nothing set\n'
                   '    while (std::scanf("%lld %lld %d %d %d %d", &len_out, &C, &cic, &warm, &minw, &fin2) == 6) {\n'
                   '        const pg::BankGeom g = pg::bank_geometry(len_out, C, cic != 0, warm, minw, fin2 != 0, t.bank_waves, t.fused_l, t.bank_hsplit);\n'
                   '        std::printf("%d %lld %lld %u\\n", g.waves, g.L, g.pairs, g.n_wg);\n    }\n    return 0;\n}\n')
    exe = str(d / "geom")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    minw = shipped_variants()
    keys, lines = [], []
    for r in B.ROWS:
        inst = B.instance_of(chains[r.name])
        for k in B.mfma_calls(r):
            keys.append((r.name, k))
            lines.append("%d %d %d %d %d %d" % (r.calls[k] * B.FRAME, r.C, inst[0] == 12, B.warm_blocks(inst), minw[inst], B.has_two_stage_calls(r)))
    out = subprocess.check_output([exe], input="\n".join(lines) + "\n", text=True).split("\n")
    return {key: tuple(int(v) for v in line.split()) for key, line in zip(keys, out)}


def test_rows_are_well_formed():
    assert len({r.name for r in B.ROWS}) == len(B.ROWS)
    for r in B.ROWS:
        assert len(r.calls) == len(r.geometry) and max(r.calls) <= r.max_superframes, r.name
        # the first call and the call after a retune lie in the oscillators' transient: the two-kernel route
        other = {0} | ({r.retune_before} if r.retune_before is not None else set())
        assert {k for k, g in enumerate(r.geometry) if g is None} == other, r.name
        assert r.C >= 16, r.name


def test_every_row_takes_the_instance_it_names(chains):
    shipped = shipped_variants()
    for r in B.ROWS:
        assert B.instance_of(chains[r.name]) == r.instance, (r.name, chains[r.name])
        assert r.instance in shipped, r.name


def test_every_shipped_instance_has_a_multi_group_row(chains):
    shipped = shipped_variants()
    multi = {B.instance_of(chains[r.name]) for r in B.ROWS if (r.C + 31) // 32 >= 2}
    assert set(shipped) - multi == set(), "k_mix_dec_mfma instances without a row of two or more channel groups in tests/bank_cases.py"
    # ... a ragged one of five groups, the second quad with one live wave
    ragged = {B.instance_of(chains[r.name]) for r in B.ROWS if r.C == 133}
    assert set(shipped) - ragged == set()


def test_rows_reach_the_geometry_they_claim(geometry):
    for r in B.ROWS:
        for k in B.mfma_calls(r):
            assert geometry[(r.name, k)][:2] == r.geometry[k], (r.name, k, geometry[(r.name, k)])


def test_the_table_covers_what_it_is_there_for(chains, geometry):
    rows = {r.name: r for r in B.ROWS}
    cic = {n: B.instance_of(chains[n])[0] == 12 for n in rows}
    # front strides: hb11 x 2 and x 16; CIC3 at 8 and 32 (2, 4 and 16 run in tests/test_parity_gpu.py)
    assert {2, 16} <= {B.front_stride(chains[n]) for n in rows if not cic[n]}
    assert {8, 32} <= {B.front_stride(chains[n]) for n in rows if cic[n]}
    for front in (False, True):
        # at least three chunk lengths per front kind, and one handle whose calls change it
        ls = {geometry[(n, k)][1] for n, r in rows.items() if cic[n] == front for k in B.mfma_calls(r)}
        assert len(ls) >= 3, (front, ls)
        assert any(len({geometry[(n, k)][1] for k in B.mfma_calls(r)}) >= 2 for n, r in rows.items() if cic[n] == front), front
        # a retune in the middle of a run: a launch without running sums after another route, then one with them
        assert any(r.retune_before is not None and r.geometry[r.retune_before + 1] and r.geometry[r.retune_before + 2]
                   for n, r in rows.items() if cic[n] == front), front
    assert any(r.instance[3] == 59 and r.retune_before is not None for r in rows.values() if r.instance[0] == 4)
    # two waves per SIMD on both instances named, without and with the running sums
    for inst in ((4, 15, 23, 43), (4, 15, 19, 31)):
        assert any(r.instance == inst and sum(geometry[(n, k)][0] == 2 for k in B.mfma_calls(r)) >= 2 for n, r in rows.items()), inst
    # chunk pairs that do not fill a stretch of eight workgroups, behind a CIC3 front
    assert any(cic[n] and geometry[(n, k)][2] < 8 for n, r in rows.items() for k in B.mfma_calls(r))
    # WFM through the kernel; a 0 Hz channel in the middle of a group of every row
    assert any(r.wfm and r.C >= 33 for r in rows.values())
    for r in B.ROWS:
        p = B.plan(r, chains[r.name])
        assert p.fc[p.zero] == 0.0 and 0 < p.zero % 32 < 31 and p.zero in p.compare, r.name
        want = {0, 1, 30, 31, 32, 33, 63, 64, 127, 128, r.C - 2, r.C - 1, 2047, 2048}
        assert {c for c in want if 0 <= c < r.C} <= set(p.compare), r.name
        if r.retune_before is not None:
            assert p.retuned in p.compare and p.retuned // 32 != p.zero // 32
        if r.C <= B.DENSE:
            assert len(set(B.final_bins(r, p))) == r.C, r.name
        assert all(300.0 <= lo < b * p.df < hi <= 3000.0 for b, (lo, hi) in zip(B.final_bins(r, p), p.band)), r.name


def test_a_call_synthesised_on_its_own_is_the_run_evaluated_tone_by_tone():
    period = 3 * 2048 * 4
    idx = [5, -7, 1234, 3 * 2048 * 4 - 1, 3000, 3001, 3002]
    for start, n in ((0, 8192), (8192, 8192), (3 * 8192, 2 * 8192), (5 * 8192, 3 * 8192)):
        a, b = B.synth_tones(idx, period, start, n), B.direct_tones(idx, period, start, n)
        assert np.max(np.abs(a - b)) <= 1e-9, (start, n)


@pytest.mark.parametrize("name", ["hb11x2", "wfm-20M"])
def test_the_oracle_puts_every_compared_peak_where_the_tuning_predicts(oracle_mod, chains, name):
    """the lane-mapping condition of the GPU tier is one the reference meets (the two cheapest rows: 33 channels, D = 16 narrow
    and D = 64 WFM)"""
    r = {r.name: r for r in B.ROWS}[name]
    p = B.plan(r, chains[name])
    xs = [B.call_input(r, p, k) for k in range(len(r.calls))]
    y = np.array([B.oracle_channel(oracle_mod, r, p, c, xs, chains[name]) for c in p.compare])
    got = (B.peak_bins_wfm if r.wfm else B.peak_bins)(y)
    want = [B.final_bins(r, p)[c] for c in p.compare]
    assert list(got) == want
