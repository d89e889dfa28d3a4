"""CPU tier of the display transforms' chain table (tests/spectrum_cases.py): every row and call reaches the kernel family and the
chain geometry it claims -- spectrum_geometry() of csrc/spectrum_geom.h, compiled here with g++: should a threshold move, these
assertions fail instead of the GPU tier quietly walking chains of one frame again -- and the input is one on which a chain that
averaged with the wrong predecessor cannot pass: on the oracle alone, for every frame the GPU tier compares."""
import os
import re
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from tests import spectrum_cases as SC
from tests.signals import lcg_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")
TOL_DB = 0.1  # tests/test_parity_gpu.py's bar (that module is GPU-only)
FAMILIES = ["q128", "waves", "t128", "t128_one", "w64", "any", "big"]

Geom = namedtuple("Geom", "G chains per_wg wgs surplus")


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """(family, F, S, bins, frame, batch) -> Geom, by the library's own function"""
    d = tmp_path_factory.mktemp("spectrum_geom")
    src = d / "geom.cpp"
    src.write_text('#include <cstdio>\n#include "spectrum_geom.h"\n'
                   'int main()\n{\n    int fam;\n    long long F, S, bins, frame, batch;\n'
                   '    while (std::scanf("%d %lld %lld %lld %lld %lld", &fam, &F, &S, &bins, &frame, &batch) == 6) {\n'
                   '        const pg::SpectrumGeom g = pg::spectrum_geometry((pg::SpecFamily)fam, F, S, bins, frame, batch);\n'
                   '        std::printf("%d %lld %d %u %lld\\n", g.G, g.chains, g.chains_per_wg, g.wgs, g.surplus);\n    }\n    return 0;\n}\n')
    exe = str(d / "geom")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    # the enumerators in the header's order
    hdr = open(os.path.join(CSRC, "spectrum_geom.h")).read()
    body = hdr[hdr.index("enum class SpecFamily {"):]
    names = re.findall(r"^\s*(\w+),", body[:body.index("};")], flags=re.M)
    assert names == FAMILIES

    def many(queries):
        """[(family, F, S, bins, frame, batch)] -> [Geom], one process for all"""
        text = "".join("%d %d %d %d %d %d\n" % ((FAMILIES.index(q[0]),) + tuple(q[1:])) for q in queries)
        out = subprocess.check_output([exe], input=text, text=True).split("\n")
        return [Geom(*(int(v) for v in line.split())) for line in out[:len(queries)]]

    def geom(family, F, S, bins, frame, batch=None):
        return many([(family, F, S, bins, frame, S if batch is None else batch)])[0]
    geom.many = many
    return geom


def launches(row, geometry):
    """per call of the row's bank: (rows computed, Geom)"""
    return [(len(sel), geometry(row.family, len(sel), row.S, row.bins, row.frame)) for sel in SC.computed_frames(row)]


def inline_arithmetic(family, F, S, bins, frame, batch):
    """(G, grid.x) as SpectrumCore::run, run_any and run_list_big computed them inline before spectrum_geom.h took the arithmetic over"""
    def cdiv(a, b):
        return (a + b - 1) // b

    def clamp(g, hi):
        return max(1, min(hi, g))
    if family == "q128":
        zp = bins // frame
        G = clamp(F * S * zp // 2048, 32)
        return G, 8 * zp * cdiv(cdiv(F, G), 8)
    if family == "waves":
        groups = 4 // (bins // frame)
        G = clamp(F * S // (1024 * groups), 16)
        return G, cdiv(F, G * groups)
    if family in ("t128", "t128_one"):
        G = clamp(F * S // 512, 32)
        return G, cdiv(cdiv(F, G), 2) if family == "t128" else cdiv(F, G)
    if family == "w64":
        G = clamp(cdiv(F * S, 512), 32)
        return G, cdiv(F, G)
    if family == "any":
        M = 256
        while M < frame:
            M *= 2
        zp = bins // M
        G = clamp(F * S * zp // 1024, 32)
        return G, cdiv(F, G) * zp
    G = clamp(F * batch * 8 // 512, 16)
    return G, cdiv(F, G) * 8


def test_the_header_launches_the_grids_the_inline_arithmetic_launched(geometry):
    shapes = [("q128", 2048, 2048), ("q128", 16384, 2048), ("q128", 32768, 2048), ("waves", 4096, 2048), ("waves", 2048, 2048),
              ("t128", 8192, 2048), ("t128_one", 8192, 2048), ("w64", 8192, 2048), ("any", 8192, 1024), ("any", 4096, 3000), ("any", 16384, 4096),
              ("any", 32768, 16384), ("big", 65536, 65536)]
    fs = list(range(1, 140)) + [255, 256, 257, 511, 512, 513, 515, 1023, 1024, 1025, 4095, 4096, 16384, 16385, 65536, 100000]
    queries = [(fam, F, S, bins, frame, batch) for fam, bins, frame in shapes for S in (1, 2, 3, 4, 8, 16, 64, 128) for F in fs
               for batch in ((S,) if fam != "big" else sorted({1, max(1, S // 3), S}))]
    got = geometry.many(queries)
    assert len(got) == len(queries) > 10000
    for q, g in zip(queries, got):
        assert (g.G, g.wgs) == inline_arithmetic(*q), (q, g)
        assert g.chains == -(-q[1] // g.G) and g.surplus >= 0 and (g.chains + g.surplus) % g.per_wg == 0, (q, g)


def test_rows_are_well_formed():
    assert len({r.name for r in SC.ROWS}) == len(SC.ROWS)
    for r in SC.ROWS:
        assert r.family in FAMILIES and r.fmt in (None, 0) and r.bins >= r.frame, r.name
        assert sum(SC.chunks(r)) == sum(SC.calls(r)) and max(SC.chunks(r)) <= r.chunk, r.name
        assert len(SC.streams(r)) >= 2 and {0, r.S - 1} <= set(SC.streams(r)), r.name


def test_every_row_takes_the_kernel_family_it_names():
    """SpectrumCore::init's selection, restated: 65536 / 65536 is `big`; 2048-sample frames with 2048, 16384 or 32768 bins take
    k_spectrum_q128, with 4096 k_spectrum<2>, with 8192 k_spectrum_t128 (two chains per workgroup: the stagger defaults to 3); every
    other frame length the general kernel.  (k_spectrum_1to1 is unreachable: 2048 bins always take k_spectrum_q128.)"""
    src = open(os.path.join(CSRC, "cores.hip")).read()
    assert "per_q = !big && !any && (bins == 2048 || bins > 8192 || tun.spectrum_perq);" in src
    assert re.search(r"int t128_stagger = 3;", open(os.path.join(CSRC, "tuning.h")).read())
    for r in SC.ROWS:
        if r.frame == 65536 and r.bins == 65536:
            fam = "big"
        elif r.frame != 2048:
            fam = "any"
        else:
            fam = {2048: "q128", 4096: "waves", 8192: "t128", 16384: "q128", 32768: "q128"}[r.bins]
        assert r.family == fam, r.name
        assert r.kernel.startswith({"q128": "k_spectrum_q128", "waves": "k_spectrum<2>", "t128": "k_spectrum_t128", "any": "k_spectrum_any",
                                    "big": "k_big256_cols"}[fam]), r.name
        assert ("raw s8" in r.kernel) == (r.fmt == 0) and ("_list" in r.kernel) == (r.ups is not None), r.name


def test_rows_reach_the_chains_they_claim(geometry):
    for r in SC.ROWS:
        ls = launches(r, geometry)
        (n1, g1), (n2, g2), (n3, g3) = ls
        # the long calls walk chains of two frames or more, several per stream; the short call between them degenerates to G = 1
        for n, g in ((n1, g1), (n3, g3)):
            assert g.G >= 2 and g.chains > 1 and g.chains == -(-n // g.G), (r.name, n, g)
        assert g2.G == 1 and n2 >= 2, (r.name, n2, g2)
        assert [g.G for _, g in ls] == [SC.chain_length(r, k) for k in range(3)], r.name
        assert (g1.G, g1.chains, n1 - (g1.chains - 1) * g1.G, g1.surplus) == (r.G, r.chains, r.last_live, r.surplus), (r.name, n1, g1)
        if r.ups is None:
            assert n1 == n3 == r.F and n2 == SC.SHORT and g3 == g1, r.name
        else:
            assert n1 >= 9 and n3 >= 9 and n1 < r.F, (r.name, n1, n3)  # about every second frame
        # the second bank, fed the same frames in calls of `chunk`, never walks a chain longer than one frame
        for sel in SC.computed_frames(r, SC.chunks(r)):
            assert geometry(r.family, max(1, len(sel)), r.S, r.bins, r.frame).G == 1, r.name
        assert sum(SC.computed_frames(r, SC.chunks(r)), []) == sum(SC.computed_frames(r), []), r.name


def test_the_table_covers_what_it_is_there_for(geometry):
    rows = {r.name: r for r in SC.ROWS}
    geo = {n: launches(r, geometry)[0][1] for n, r in rows.items()}
    ragged = {n: launches(r, geometry)[0][0] % geo[n].G != 0 for n, r in rows.items()}
    # every family the default build launches, each with a ragged last chain
    for fam in ("q128", "waves", "t128", "any", "big"):
        assert any(r.family == fam and ragged[n] for n, r in rows.items()), fam
    # k_spectrum_q128: surplus chain slots with and without zero-padding, chains of three, ZP = 16
    q = [n for n, r in rows.items() if r.family == "q128"]
    assert any(geo[n].surplus > 0 and rows[n].bins == 2048 for n in q) and any(geo[n].surplus > 0 and rows[n].bins > 2048 for n in q)
    assert any(geo[n].G == 3 and launches(rows[n], geometry)[0][0] % 3 == 1 for n in q) and any(rows[n].bins == 32768 for n in q)
    # two chains per workgroup: a last workgroup whose second chain is half dead (k_spectrum<2>) and one whose second chain is wholly dead (t128)
    w = geo["waves-4096"]
    assert w.per_wg == 2 and w.surplus == 0 and w.chains % 2 == 0 and rows["waves-4096"].F % w.G == 1 and w.wgs * 2 == w.chains
    for n in ("t128-float", "t128-s8"):
        assert geo[n].per_wg == 2 and geo[n].chains % 2 == 1 and geo[n].surplus == 1 and rows[n].F % geo[n].G == 1, n
    assert rows["t128-s8"].fmt == 0 and rows["t128-float"].fmt is None
    # the general kernel: ZP 1 (a frame that is no power of two), 4 and 8
    assert {(r.frame, r.bins) for r in rows.values() if r.family == "any"} >= {(1024, 8192), (3000, 4096), (4096, 16384)}
    # the 65536-point transform: more frames than a chain holds, every frame and listed frames (int8)
    assert geo["big"].chains == 5 and rows["big"].F > geo["big"].G and rows["big"].ups is None
    assert rows["big-listed-s8"].ups is not None and rows["big-listed-s8"].fmt == 0 and geo["big-listed-s8"].chains >= 5


def test_the_noise_of_a_frame_made_on_its_own_is_the_stream_s():
    for seed, k, n in ((7, 0, 10), (7, 5000, 100), (12345, 2 * 3 * 65536, 64)):
        a = lcg_noise(n, SC.lcg_jump(seed, 2 * k), 1.0)
        assert np.array_equal(a, lcg_noise(k + n, seed, 1.0)[k:]), (seed, k)
    r = SC.ROWS[0]
    assert np.array_equal(SC.frames_input(r, 1, 3, 4)[2 * r.frame:3 * r.frame], SC.frame_input(r, 1, 5))
    r = {r.name: r for r in SC.ROWS}["t128-s8"]
    raw = SC.bank_input(r, 5, 2)  # (frame 5 is a full-level one)
    assert raw.dtype == np.int8 and raw.shape == (r.S, 2 * r.frame, 2) and np.array_equal(SC.convert(raw[1]), SC.frames_input(r, 1, 5, 2))
    assert np.abs(raw.astype(int)).max() > 60


def test_levels_step_by_12_db_or_more():
    lv = SC.level_db(np.arange(40))
    assert np.abs(np.diff(lv)).min() >= 12.0 and lv.min() == -24.0 and lv.max() == 0.0
    for r in SC.ROWS:
        for s in SC.streams(r):
            k = SC.tone_index(r, s, np.arange(3 * SC.PERIOD))
            assert np.abs(k).max() < 0.49 * r.frame and len(set(k[:SC.PERIOD])) == SC.PERIOD, r.name
            assert np.abs(k[1:] - k[:-1]).min() >= 37 * (r.frame // 256) and np.abs(k[2:] - k[:-2]).min() >= 74 * (r.frame // 256), r.name


@pytest.mark.parametrize("name", [r.name for r in SC.ROWS])
def test_a_wrong_predecessor_moves_every_compared_frame_by_1_db(oracle_mod, geometry, name):
    """for every frame the GPU tier compares: the oracle's average with the frame two back, with the frame itself and with nothing
    differs from the true one by at least 1 dB (ten times TOL_DB) at the frame's own peak or at its true predecessor's"""
    r = {r.name: r for r in SC.ROWS}[name]
    done = worst = 0
    flat = sum(SC.computed_frames(r), [])  # (under a gate the predecessor is the previous LISTED frame)
    at = {g: i for i, g in enumerate(flat)}
    for k, (sel, (n, geo)) in enumerate(zip(SC.computed_frames(r), launches(r, geometry))):
        assert geo.G == SC.chain_length(r, k)
        for i in SC.compared_rows(r, k, n, geo.G):
            g = sel[i]
            j = at[g]
            assert j >= 1
            pred, pred2 = flat[j - 1], flat[j - 2] if j >= 2 else None
            for s in SC.streams(r):
                x = SC.frame_input(r, s, g).astype(np.complex128)
                sp = SC.new_oracle(oracle_mod, r)
                alone = sp.process(x)                       # averaged with the start-up zeros
                twice = sp.process(x)                       # averaged with itself
                true = SC.oracle_pair(oracle_mod, r, s, pred, g)
                pk, pk_pred = int(np.argmax(alone)), int(np.argmax(_alone(oracle_mod, r, s, pred)))
                assert abs(pk - SC.tone_bin(r, s, g)) <= 1 and abs(pk_pred - SC.tone_bin(r, s, pred)) <= 1 and pk != pk_pred, (name, k, i, s)
                assert true[pk] > -110 and true[pk_pred] > -110  # (bins the GPU tier's db_err looks at)
                wrong = {"zeros": alone, "itself": twice}
                if pred2 is not None:
                    wrong["two back"] = SC.oracle_pair(oracle_mod, r, s, pred2, g)
                for what, w in wrong.items():
                    moved = max(abs(w[pk] - true[pk]), abs(w[pk_pred] - true[pk_pred]))
                    assert moved >= 10 * TOL_DB, (name, k, i, s, what, moved)
                    worst = moved if not done else min(worst, moved)
                    done += 1
    assert done >= 3 * 40
    print("%s: %d wrong predecessors, the least moves the result by %.2f dB" % (name, done, worst))


def _alone(oracle_mod, r, s, g):
    return SC.new_oracle(oracle_mod, r).process(SC.frame_input(r, s, g).astype(np.complex128))
