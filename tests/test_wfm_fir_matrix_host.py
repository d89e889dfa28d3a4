"""k_wfm_fir's audio FIR as a banded-Toeplitz matrix product (csrc/wfm_fir_geom.h), on the host: the header and its tap-table builder
are compiled with g++, and the blocked product is emulated in numpy exactly as the kernel walks it -- column group by column group,
K half by K half (the wave split), group of 16 k by group, every operand taken through the header's index functions and the
instruction's lane maps (A: row = lane & 15, k = lane >> 4; B: k = lane >> 4, column = lane & 15; C/D: column = lane & 15, row =
4 (lane >> 4) + register) -- against np.convolve in fp64, for every L4 in 16 .. 1536 step 16 and Llp in {1, 47, 62} (Llp moves where
`db` lies in LDS).  Bar: 1e-12 of the largest output (both sides sum the same fp64 products of fp32-rounded taps in another
order: a few 1e-16 per term over at most 1536 terms).  Also: the padded K holds every tap of every row exactly once, the halves
partition the groups, every LDS read stays inside `db` and `db` inside the allocation, 16-byte aligned.  The low-pass in front of
the discriminator (phase 2) is the same product on a plane of samples: emulated job by job against np.convolve at every L4 and
Llp as well, with its planes' places in LDS."""
import subprocess

import numpy as np
import pytest

from tests import demod_cases as DC

L4S = list(range(16, 1536 + 1, 16))
LLPS = (1, 47, 62)
OUTB = DC.K_WFM_OUTB
LP_TILES_MAX = (OUTB + L4S[-1] + 8 + 255) // 256   # tiles of 256 low-pass outputs at the longest response

_PROGRAM = r'''
#include <cstdio>
#include <vector>
#include "wfm_fir_geom.h"
using namespace pg;
static void put(const std::vector<int> &v) { std::fwrite(v.data(), sizeof(int), v.size(), stdout); }
int main()
{
    // constants
    put({kWfmMxTile, kWfmMxColGroups, kWfmMxHalves, kWfmMxGroupK, kWfmLpGroupsMax});
    // the B operand's db index [cg][g][lane][j] for the most groups any L4 has, and the result's output index [cg][lane][r]
    const int Gmax = wfm_mx_groups(L4_MAX);
    std::vector<int> m;
    for (int cg = 0; cg < kWfmMxColGroups; cg++)
        for (int g = 0; g < Gmax; g++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 4; j++) m.push_back(wfm_mx_db(cg, g, lane, j));
    put(m);
    m.clear();
    for (int cg = 0; cg < kWfmMxColGroups; cg++)
        for (int lane = 0; lane < 64; lane++)
            for (int r = 0; r < 4; r++) m.push_back(wfm_mx_out(cg, lane, r));
    put(m);
    // the low-pass: per Llp the groups and the A operand's tap index + 1 [g][lane][j] (0 = none); the B operand's sample index
    // [tile][g][lane][j] for the most tiles and groups
    for (int Llp : {1, 47, 62}) {
        put({wfm_lp_groups(Llp)});
        m.clear();
        for (int g = 0; g < kWfmLpGroupsMax; g++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 4; j++) m.push_back(wfm_lp_tap(Llp, g, lane, j) + 1);
        put(m);
    }
    m.clear();
    for (int t = 0; t < LP_TILES_MAX; t++)
        for (int g = 0; g < kWfmLpGroupsMax; g++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 4; j++) m.push_back(wfm_lp_x(t, g, lane, j));
    put(m);
    // per L4: G, the halves' bounds, the db offset per Llp, then the table wfm_mx_fill_taps builds from h[p] = p + 1 (so an entry
    // names its tap, 0 = a zero of the band's corners)
    for (int L4 = 16; L4 <= L4_MAX; L4 += 16) {
        const int G = wfm_mx_groups(L4);
        put({G, wfm_mx_half_begin(G, 0), wfm_mx_half_begin(G, 1), wfm_mx_half_begin(G, 2), wfm_mx_table_floats(L4),
             wfm_fir_db_offset(OUTB, L4, 1), wfm_fir_db_offset(OUTB, L4, 47), wfm_fir_db_offset(OUTB, L4, 62),
             wfm_fir_lp_offset(OUTB, L4, 1), wfm_fir_lp_offset(OUTB, L4, 47), wfm_fir_lp_offset(OUTB, L4, 62),
             wfm_lp_jobs((OUTB + L4 + 1 + 7) & ~7), wfm_lp_plane(((OUTB + L4 + 1 + 7) & ~7) + 46)});
        std::vector<float> h(L4), t(wfm_mx_table_floats(L4));
        for (int p = 0; p < L4; p++) h[p] = (float)(p + 1);
        wfm_mx_fill_taps(h.data(), L4, t.data());
        std::vector<int> ti(t.begin(), t.end());
        put(ti);
    }
    return 0;
}
'''


def _lds_bytes(L4, Llp):
    """kernels_demod.h wfm_fir_lds_bytes"""
    nd = OUTB + L4
    nl = (nd + 1 + 7) & ~7
    nx = nl + Llp - 1
    return (nx + nx // 8 + 1) * 8 + (nl + 1) * 8 + nd * 4


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    d = tmp_path_factory.mktemp("wfm_fir_geom")
    src, exe = d / "geom.cpp", str(d / "geom")
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + DC.CSRC, "-DL4_MAX=%d" % L4S[-1], "-DOUTB=%d" % OUTB, "-DLP_TILES_MAX=%d" % LP_TILES_MAX, str(src), "-o", exe])
    a = np.frombuffer(subprocess.check_output([exe]), dtype=np.int32)
    tile, ncg, nh, gk, lpg = (int(v) for v in a[:5])
    assert (tile, ncg, nh, gk) == (16, 4, 2, 16) and ncg * tile * tile == OUTB
    at = 5
    gmax = L4S[-1] // 16 + 1
    db = a[at:at + ncg * gmax * 256].reshape(ncg, gmax, 64, 4); at += db.size
    out = a[at:at + ncg * 256].reshape(ncg, 64, 4); at += out.size
    lp = {}
    for llp in LLPS:
        g = int(a[at]); at += 1
        lp[llp] = (g, a[at:at + lpg * 256].reshape(lpg, 64, 4)); at += lpg * 256
    lpx = a[at:at + LP_TILES_MAX * lpg * 256].reshape(LP_TILES_MAX, lpg, 64, 4); at += lpx.size
    per = {}
    for L4 in L4S:
        G, h0, h1, h2, nt = (int(v) for v in a[at:at + 5])
        off = {llp: int(v) for llp, v in zip(LLPS, a[at + 5:at + 8])}
        lpoff = {llp: int(v) for llp, v in zip(LLPS, a[at + 8:at + 11])}
        jobs, plane47 = int(a[at + 11]), int(a[at + 12])
        at += 13
        assert nt == G * 256
        per[L4] = (G, (h0, h1, h2), off, a[at:at + nt].reshape(G, 64, 4), lpoff, jobs, plane47)
        at += nt
    assert at == len(a)
    return {"db": db, "out": out, "per": per, "lp": lp, "lpx": lpx, "lpg": lpg}


def test_the_kernels_constants_are_the_ones_this_file_assumes():
    k = DC._header_constants()
    assert k["kWfmOutB"] == OUTB and k["kWfmIrMax"] == L4S[-1] and k["kWfmLpMax"] >= max(LLPS)


def test_padded_k_holds_every_tap_of_every_row_exactly_once(geom):
    lane = np.arange(64)
    for L4 in L4S:
        G, (h0, h1, h2), _, table = geom["per"][L4][:4]
        assert G * 16 == L4 + 16
        assert 0 == h0 < h1 <= h2 == G and h1 - h0 >= h2 - h1 >= h1 - h0 - 1, "the halves partition the groups, sizes within one"
        for b in range(16):
            taps = table[:G, lane[(lane & 15) == b], :].ravel()     # the k run of row b: 16 G entries
            taps = taps[taps != 0] - 1
            assert len(taps) == L4 and np.array_equal(np.sort(taps), np.arange(L4)), (L4, b)
        # a lane's four A operands of a group are consecutive taps (descending) wherever the band is not cut
        full = (table[:G] != 0).all(axis=2)
        assert (np.diff(table[:G][full], axis=1) == -1).all()


def test_operand_reads_stay_inside_db_and_db_inside_the_allocation(geom):
    db, out = geom["db"], geom["out"]
    assert np.array_equal(np.sort(out.ravel()), np.arange(OUTB)), "every output of the workgroup comes from exactly one register"
    assert (np.diff(out, axis=2) == 1).all() and (out[:, :, 0] % 4 == 0).all(), "a lane's four results are consecutive outputs"
    assert (db[:, :, :, 0] % 4 == 0).all() and (np.diff(db, axis=3) == 1).all(), "a lane's four B operands: one aligned 16-byte read"
    # a wave's 64 reads of a group are 1024 contiguous bytes: conflict-free whatever the bank count
    assert np.array_equal(np.sort(db[:, :, :, 0], axis=2) - db[:, :, :1, 0], np.broadcast_to(4 * np.arange(64), db.shape[:3]))
    for L4 in L4S:
        G = geom["per"][L4][0]
        assert db[:, :G].min() == 0 and db[:, :G].max() == OUTB + L4 - 1, "ND = kWfmOutB + L4 samples, all used, none beyond"
        for llp in LLPS:
            off = geom["per"][L4][2][llp]                      # floats from the start of the dynamic allocation
            nd = OUTB + L4
            nl = (nd + 1 + 7) & ~7
            nx = nl + llp - 1
            lpoff = geom["per"][L4][4][llp]                    # the low-passed planes: 2 NL floats directly in front of db
            planes = 2 * ((nx + 3) & ~3)                       # the sample planes, from the start of the allocation
            assert off % 4 == 0 and lpoff % 4 == 0 and planes <= lpoff and lpoff + 2 * nl == off and 4 * (off + nd) <= _lds_bytes(L4, llp), (L4, llp)
            assert 4 * planes >= 8 * OUTB, "the K halves' fp64 partial sums (4 x 256 doubles) fit in the sample planes"


def test_low_pass_product_equals_the_convolution(geom):
    """phase 2: the same product with the low-pass response on a plane of samples, job by job (a tile of 256 outputs), zeros read
    from the end of the plane on, results kept where o < NL; against np.convolve in fp64, at every L4 (NL = outputs + L4 + 1
    rounded up to 8) and Llp"""
    rng = np.random.default_rng(21)
    lane = np.arange(64)
    worst = 0.0
    for llp in LLPS:
        Glp, tapi = geom["lp"][llp]
        assert Glp * 16 >= llp + 15 > (Glp - 1) * 16 and Glp <= geom["lpg"]
        for b in range(16):
            taps = tapi[:Glp, lane[(lane & 15) == b], :].ravel()
            assert np.array_equal(np.sort(taps[taps != 0] - 1), np.arange(llp)), "every tap of every row exactly once"
        assert not tapi[Glp:].any()
        hl = rng.standard_normal(llp).astype(np.float32).astype(np.float64)
        tv = np.where(tapi > 0, hl[np.maximum(tapi - 1, 0)], 0.0)
        for L4 in L4S:
            nl = (OUTB + L4 + 1 + 7) & ~7
            nx = nl + llp - 1
            nxp = (nx + 3) & ~3
            jobs = geom["per"][L4][5]
            assert jobs == 2 * ((nl + 255) // 256)
            assert llp != 47 or geom["per"][L4][6] == nxp, "wfm_lp_plane"
            plane = np.concatenate([rng.standard_normal(nx), np.zeros(nxp - nx)])
            want = np.convolve(hl, plane[:nx])[llp - 1:llp - 1 + nl]      # l[o] = sum_m hlp[m] x[o + Llp - 1 - m]
            got = np.full(nl, np.nan)
            for t in range(jobs // 2):
                acc = np.zeros((16, 16))
                for g in range(Glp):
                    idx = geom["lpx"][t, g]                               # [lane][j]
                    assert (idx[:, 0] % 4 == 0).all() and (np.diff(idx, axis=1) == 1).all()
                    ok = idx[:, :1] < nxp
                    B = np.where(ok, plane[np.where(ok, idx, 0)], 0.0).reshape(4, 16, 4)   # [kq][a][j]
                    acc += np.einsum("kbj,kaj->ba", tv[g].reshape(4, 16, 4), B)
                o = geom["out"][0] + 256 * t                               # wfm_mx_out(t, lane, r)
                y = acc[(4 * (lane >> 4))[:, None] + np.arange(4)[None, :], (lane & 15)[:, None]]
                keep = o[:, 0] < nl
                got[o[keep]] = y[keep]
            assert not np.isnan(got).any(), "every output below NL is written"
            e = float(np.abs(got - want).max() / np.abs(want).max())
            worst = max(worst, e)
            assert e <= 1e-12, (L4, llp, e)
    print("low-pass product against np.convolve: worst error %.2e of the largest output" % worst)


def test_blocked_product_equals_the_convolution(geom):
    """tile by tile and half by half, in fp64, with the taps rounded to fp32 as uploaded"""
    rng = np.random.default_rng(20)
    worst = 0.0
    for L4 in L4S:
        G, (h0, h1, h2), offs, table = geom["per"][L4][:4]
        h = (rng.standard_normal(L4) * np.exp(-np.arange(L4) / 200.0)).astype(np.float32).astype(np.float64)
        tv = np.where(table > 0, h[np.maximum(table - 1, 0)], 0.0)   # what wfm_mx_fill_taps uploads for this response
        lane = np.arange(64)
        for llp in LLPS:
            nd = OUTB + L4
            lds = rng.standard_normal(_lds_bytes(L4, llp) // 4 + 4)     # the whole allocation as floats; db is a part of it
            dbv = lds[offs[llp]:offs[llp] + nd]
            want = np.convolve(h, dbv)[L4:L4 + OUTB]                     # y[o] = sum_p h[p] db[L4 + o - p]
            got = np.zeros(OUTB)
            for cg in range(4):
                part = []
                for lo, hi in ((h0, h1), (h1, h2)):                       # the K halves: waves cg and cg + 4
                    acc = np.zeros((16, 16))                              # [row b][column a], the fp64 fold of the groups' results
                    for g in range(lo, hi):
                        # step j of the group: A[b][kq] = table[g][b + 16 kq][j], B[kq][a] = db[index of lane a + 16 kq]
                        A = tv[g].reshape(4, 16, 4)                        # [kq][b][j]
                        B = lds[offs[llp] + geom["db"][cg, g]].reshape(4, 16, 4)  # [kq][a][j]
                        acc += np.einsum("kbj,kaj->ba", A, B)
                    part.append(acc)
                y = part[0] + part[1]                                      # the halves meet in LDS
                got[geom["out"][cg]] = y[(4 * (lane >> 4))[:, None] + np.arange(4)[None, :], (lane & 15)[:, None]]
            e = float(np.abs(got - want).max() / np.abs(want).max())
            worst = max(worst, e)
            assert e <= 1e-12, (L4, llp, e)
    print("blocked product against np.convolve: worst error %.2e of the largest output over %d (L4, Llp)" % (worst, len(L4S) * len(LLPS)))
