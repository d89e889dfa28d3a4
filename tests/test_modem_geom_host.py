"""CPU tier of tests/modem_geom_cases.py (the geometry of the modem ring at a modem rate, k_modem_rate_pack):
 - every row of the table against pebblegpu_modem_rate_plan, oracle.Decimator(...).chain() and csrc/modem_rate_geom.h compiled here with
   the host compiler; the refusals with their codes; the arithmetic facts the coverage statement's unreachable paths rest on;
 - a plain fp64 model of the kernel's algorithm, written from the comment above the kernel, equal to oracle.Decimator fed the present
   pairs on every row under three presence patterns;
 - six wrong models, one line of that model each, which miss the device's bar tenfold on a named row and pattern, on the oracle alone;
 - the signal condition: no compared pair is near-silent.
tests/test_modem_geom_gpu.py holds the device to the same rows."""
import os
import subprocess

import numpy as np
import pytest

from tests import decim_cases as DC
from tests import modem_geom_cases as GC
from tests import modem_out_cases as MC
from tests import tail_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")
NAMES = list(GC.ROWS)


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


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """csrc/modem_rate_geom.h through the host compiler -> f(D, H, out_spf, taps0, stride0) = (tile, lds_a, lds_b) or None"""
    d = tmp_path_factory.mktemp("modem_geom")
    src, exe = d / "geom.cpp", str(d / "geom")
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "modem_rate_geom.h"\n'
                   'int main(int argc, char **argv) {\n'
                   '    for (int i = 1; i + 4 < argc; i += 5) {\n'
                   '        pg::ModemRateGeom g;\n'
                   '        if (pg::modem_rate_geometry(strtoull(argv[i], 0, 10), strtoull(argv[i + 1], 0, 10), strtoull(argv[i + 2], 0, 10), atoi(argv[i + 3]),\n'
                   '                                    (uint32_t)atoi(argv[i + 4]), &g)) printf("%u %u %u\\n", g.tile, g.lds_a, g.lds_b);\n'
                   '        else printf("none\\n");\n'
                   '    }\n    return 0;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])

    def ask(cases):
        args = [str(int(v)) for c in cases for v in c]
        lines = subprocess.check_output([exe] + args, text=True).splitlines()
        assert len(lines) == len(cases)
        return [None if ln == "none" else tuple(int(v) for v in ln.split()) for ln in lines]
    return ask


def code_of(P, fn, *args):
    with pytest.raises(P.PebbleGpuError) as e:
        fn(*args)
    return e.value.code, str(e.value)


# ------------------------------------------------------------------------------------------------
# 1. the table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_row_against_the_plan_the_oracle_and_the_header(P, O, header, name):
    row = GC.ROWS[name]
    rate = GC.demod_rate(row)
    L = row.fft - row.taps + 1
    assert L in GC.BLOCKS and row.spf == GC.lcm(row.nf, L) and row.nf % GC.front(row) == 0
    info, dec = P.modem_rate_plan(rate, row.spf, row.bw, row.mn), O.Decimator(rate, row.bw, row.mn)
    assert info.chain() == dec.chain() == row.chain
    assert info.total_decimation == dec.total_decimation == row.D and info.lookback == GC.lookback(row.chain) == row.H
    assert info.samples_per_superframe == row.m == row.spf // row.D and row.spf % row.D == 0
    assert O.Decimator(row.fs, 30000, 0).total_decimation == GC.front(row) and int(O.Decimator(row.fs, 30000, 0).rate) == rate
    geom = header([(row.D, row.H, row.m, row.chain[0][0], row.chain[0][1])])[0]
    assert geom is not None and geom == GC.tile_rule(row.D, row.H, row.m, *row.chain[0])
    tile, lds_a, lds_b = geom
    assert tile == row.tile and row.m % tile == row.ragged
    assert tile * row.D + row.H <= lds_a <= 4096 and lds_a % 2 == 0 and lds_b % 2 == 0
    if len(row.chain) > 1:   # the first stage's outputs of the widest span land in the second buffer
        assert (tile * row.D + row.H - row.chain[0][0]) // row.chain[0][1] + 1 <= lds_b
    else:
        assert tile <= lds_b
    assert 3 <= row.C <= 5 and len(set(row.sel)) == len(row.sel) < row.C and row.sel != sorted(row.sel) and max(row.sel) < row.C
    assert max(GC.CALLS) == GC.MAX_SF and sorted(GC.CALLS) == sorted(GC.RECUT) and GC.CALLS != GC.RECUT


def test_the_rows_reach_what_they_are_there_for():
    R = GC.ROWS
    tiles = lambda r: -(-r.m // r.tile)
    assert [R[n].ragged for n in ("d4-l1792", "d8-ragged")] == [192, 128] and all(R[n].tile == 256 for n in ("d4-l1792", "d8-ragged"))
    r = R["d16-t64"]
    assert r.tile == 64 == r.m and 128 * r.D + r.H <= 4096                      # halved by out_spf, not by the span
    r = R["d32-ragged"]
    assert r.tile == 64 < r.m and 128 * r.D + r.H > 4096 and r.ragged == 32     # halved by the span
    r = R["d64-one-tile"]
    assert tiles(r) == 1 and 2 * r.H > r.tile * r.D > r.H
    r = R["d64-four"]
    assert len(r.chain) == 4 and tiles(r) == 2 and r.ragged == 16 and r.ragged * r.D < r.H
    for n in ("d128", "d128-l1792", "d128-s16-scalar"):
        r = R[n]
        assert r.tile == 8 and r.tile * r.D < r.H and all(o0 * r.D - r.H < 0 for o0 in range(0, min(r.m, 24), r.tile))
    assert R["d128"].ragged == 0 and tiles(R["d128"]) == 3 and R["d128-l1792"].ragged == 4
    r = R["d128-s16-scalar"]
    assert r.m % 4 == 2 and r.tile % 4 == 0                                      # S16 sample by sample, F32 by pairs
    assert all(R[n].m % 4 == 0 for n in R if n != "d128-s16-scalar")
    r = R["d64-48k"]
    assert r.chain[-1][0] == 59 and r.tile * r.D < r.H and r.fs == 48000 and GC.front(r) == 1
    assert max(len(r.chain) for r in R.values()) == 4 and {r.tile for r in R.values()} == {256, 64, 32, 16, 8}


def test_refusals_with_their_codes(P, O, header):
    for rate, spf, bw, mn, code, word in GC.REFUSALS:
        got, text = code_of(P, P.modem_rate_plan, rate, spf, bw, mn)
        assert got == code and word in text, (rate, spf, bw, mn, got, text)
    rate, spf, bw, mn = GC.REFUSALS[2][:4]
    chain = O.Decimator(rate, bw, mn).chain()
    D = int(np.prod([s for _, s in chain]))
    assert spf % D == 0 and GC.lookback(chain) <= spf and 4 * D + GC.lookback(chain) > 4096   # nothing but the tile refuses it
    assert header([(D, GC.lookback(chain), spf // D, chain[0][0], chain[0][1])]) == [None]
    assert GC.tile_rule(D, GC.lookback(chain), spf // D, *chain[0]) is None


def test_what_the_unreachable_scalar_paths_rest_on(P, O, header):
    """the coverage statement's arithmetic: every design's tap count is odd (H even); wherever the plan accepts a chain at a receiver's
    rate on a super-frame of the three band-pass sizes, D <= 128 and even, spf a multiple of 256, so m is even and every quantity of
    vec_in is even; and the header agrees with the restated tile rule over the whole sweep"""
    assert all(T % 2 == 1 for T in DC.halfband_taps())
    spfs = sorted({GC.lcm(nf, L) for nf in (256, 512, 768, 1024, 1536, 2048, 4096) for L in GC.BLOCKS})
    assert all(s % 256 == 0 for s in spfs)
    asked, accepted, seen_d = [], 0, set()
    for rate in GC.RECEIVER_RATES:
        for bw in (100, 150, 200, 300, 500, 1000, 3000, 5000, 12000):
            for mn in (125, 250, 500, 1000, 2000, 4000, 8000, 16000, 0):
                dec = O.Decimator(rate, bw, mn)
                chain, D = dec.chain(), dec.total_decimation
                for spf in spfs:
                    try:
                        info = P.modem_rate_plan(rate, spf, bw, mn)
                    except P.PebbleGpuError:
                        continue
                    if not info.n_stages:
                        continue
                    accepted += 1
                    seen_d.add(D)
                    H, m = int(info.lookback), int(info.samples_per_superframe)
                    assert D % 2 == 0 and D <= 128 and H % 2 == 0 and m % 2 == 0 and m * D == spf, (rate, bw, mn, spf)
                    asked.append((D, H, m, chain[0][0], chain[0][1]))
    asked = sorted(set(asked))
    got = []
    for i in range(0, len(asked), 200):
        got += header(asked[i:i + 200])
    for a, g in zip(asked, got):
        assert g is not None and g == GC.tile_rule(*a), a
        D, H, m = a[:3]
        for o0 in range(0, m, g[0]):
            tn = min(g[0], m - o0)
            assert (o0 * D - H) % 2 == 0 and (tn * D + H) % 2 == 0 and tn * D + H <= g[1]
    print("%d accepted plans, %d distinct geometries, D in %s" % (accepted, len(asked), sorted(seen_d)))
    assert accepted > 100 and max(seen_d) == 128


# ------------------------------------------------------------------------------------------------
# 2. the model against the oracle; the signal condition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_oracle_fed_the_present_pairs(O, name):
    row = GC.ROWS[name]
    for pattern, present in GC.PATTERNS.items():
        for ch in (row.sel[0], row.sel[-1]):
            x = GC.host_stream(name, ch)
            want, gains = GC.oracle_pairs(O, row, x, present)
            got = GC.model(row, x, present)
            fig, k, j = GC.worst(got, want)
            print("%s, %s, channel %d: model against the oracle %.3e (call %d super-frame %d); output / input RMS %.3f .. %.3f"
                  % (name, pattern, ch, fig, k, j, min(gains), max(gains)))
            assert fig <= GC.MODEL_BAR
            assert min(gains) >= GC.MIN_GAIN                                      # the signal condition
            for gc, wc, pc in zip(got, want, present):
                for g, w, p in zip(gc, wc, pc):
                    assert len(g) == row.m and (p or not g.any()) and (w is None) == (not p)


def test_the_oracle_takes_whole_superframes(O):
    """oracle.Decimator grows its buffers with the frame (po_grow, oracle/pebble_oracle.c): a super-frame of 5376 or 3584 samples in
    one call equals the same samples in pieces of at most 2048, exactly"""
    for name in ("d128-s16-scalar", "d128-l1792"):
        row = GC.ROWS[name]
        x = GC.host_stream(name, 0)[:3 * row.spf]
        whole, pieces = O.Decimator(64000, row.bw, row.mn), O.Decimator(64000, row.bw, row.mn)
        for j in range(3):
            seg = x[j * row.spf:(j + 1) * row.spf]
            a = whole.process(seg)
            b = np.concatenate([pieces.process(seg[i:i + 1792]) for i in range(0, row.spf, 1792)])
            assert len(a) == row.m and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------
# 3. the wrong models
# ------------------------------------------------------------------------------------------------
def _miss(O, name, pattern, wrong):
    row = GC.ROWS[name]
    worst = 0.0
    for ch in (row.sel[0], row.sel[-1]):
        x = GC.host_stream(name, ch)
        want, _ = GC.oracle_pairs(O, row, x, GC.PATTERNS[pattern])
        worst = max(worst, GC.worst(GC.model(row, x, GC.PATTERNS[pattern], wrong=wrong), want)[0])
    return worst / MC.PAIR_BAR


@pytest.mark.parametrize("wrong", GC.WRONG)
def test_wrong_model_misses_the_bar_tenfold(O, wrong):
    name, pattern = GC.MISSES[wrong]
    bars = _miss(O, name, pattern, wrong)
    print("wrong model %s on %s, %s: %.3g bars" % (wrong, name, pattern, bars))
    assert bars >= 10.0


def test_where_a_wrong_model_cannot_be_told_apart(O):
    """a wrong model is exactly the model where the row does not reach its line: (b) without a ragged tile; (c) where the last tile's own
    samples cover H; (d) and (e) under a pattern without an absent pair in front of a present one, or without an empty launch"""
    same = [("b", "d128", "all"), ("b", "d16-t64", "gap"), ("c", "d64-one-tile", "all"), ("c", "d8-ragged", "gap"), ("d", "d128", "all"),
            ("e", "d64-four", "gap"), ("e", "d64-four", "all")]
    for wrong, name, pattern in same:
        row = GC.ROWS[name]
        x = GC.host_stream(name, row.sel[0])
        a, b = GC.model(row, x, GC.PATTERNS[pattern]), GC.model(row, x, GC.PATTERNS[pattern], wrong=wrong)
        assert all(np.array_equal(u, v) for ca, cb in zip(a, b) for u, v in zip(ca, cb)), (wrong, name, pattern)
    assert "absent-call" in GC.PATTERNS and not any(GC.PATTERNS["absent-call"][2])
    assert GC.PATTERNS["gap"][1] == [1, 0, 1] and GC.PATTERNS["gap"][3][0] == 0


def test_the_reopen_chains_are_other_chains_the_plan_accepts(P):
    for name in GC.STATE_ROWS:
        row = GC.ROWS[name]
        (bw, mn), sel = GC.REOPEN[name]
        info = P.modem_rate_plan(GC.demod_rate(row), row.spf, bw, mn)
        assert info.n_stages and info.chain() != row.chain and info.total_decimation != row.D
        assert sel != row.sel and len(set(sel)) == len(sel) and max(sel) < row.C


def test_the_gate_script_holds_on_frames_of_1536(O):
    """tail_cases' thresholds were set on frames of 2048: on the gated row's frames of 1536 the oracle's fdEstimate avgDb of every
    super-frame's last raw frame (the spectrum the gate reads, receiver.cpp:959-965) still lies 5 dB or more on the keyed side of each
    selected channel's threshold, and channel 0's first call is present-absent-present"""
    row, x, nf, sfw = TC.ROWS["gate"], GC.gate_input(), GC.GATE_NF, GC.GATE_SFW
    assert sfw == 49152 == TC.D * GC.ROWS["d64-four"].spf and row.calls[0] == 3 and TC.GATE_KEYS[0][:3] == (1, 0, 1) and 0 in GC.GATE_SEL
    sp, last = O.Spectrum(row.bins, nf), []   # (run on every frame, as the Receiver runs it)
    for f in range(len(x) // nf):
        db = sp.process(x[f * nf:(f + 1) * nf])
        if (f + 1) % (sfw // nf) == 0:
            last.append(db)
    for ch in GC.GATE_SEL:
        c = row.chans[ch]
        for j, key in enumerate(TC.GATE_KEYS[ch]):
            level = float(O.fd_estimate(last[j], TC.FS, np.float32(c.band[0]), np.float32(c.band[1]), c.fc)[1])
            print("channel %d super-frame %d key %d: %.1f dB, threshold %.1f" % (ch, j, key, level, c.squelch))
            assert (level - c.squelch >= 5.0) if key else (c.squelch - level >= 5.0), (ch, j, key, level, c.squelch)


def test_documents_state_the_coverage():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for phrase in ("modem_rate_geom.h", "tests/modem_geom_cases.py", "d128-s16-scalar"):
        assert phrase in design, phrase
    assert "modem_rate_geom.h" in open(os.path.join(CSRC, "egress.hip")).read()
    doc = GC.__doc__
    for phrase in ("vec_in == false: NOT reachable", "HistBuf::alloc", "d128-s16-scalar, in its present and its absent pairs", "k_modem_pack"):
        assert phrase in doc, phrase
