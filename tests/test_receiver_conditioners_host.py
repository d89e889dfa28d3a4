"""CPU tier of the receiver's input-conditioner table (tests/cond_cases.py; no device): the rows are well formed and reach what their
"why" says, the margin condition holds on every row that compares blanker decisions, every call of every row plans the route the table
names (csrc/call_route.h compiled here, as tests/test_call_route_host.py does), the oracle driver is the stream bank's Chain and the
oracle Receiver's own conditioner block, and every wrong model misses the GPU tier's comparison -- rel-RMS per chunk of 512 consecutive
samples of pebblegpu_receiver_conditioned() at TOL -- by a factor of WRONG_FACTOR or more on a row it is held to.

For every wrong model the factor by which it moves the OLD observables is measured too and printed: the audio of a 2.7 kHz USB pass band
(rel-RMS at TOL) and the spectrum rows (0.1 dB), all the suite looked at before the sample-exact view existed.  Nothing is asserted of
those factors but that they are finite; DESIGN.md, "Receiver input conditioners: stream lists, frame sizes, call routes" has the table."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import cond_cases as CC
from tests.spectrum_gate_ref import GateTimer
from tests.test_call_route_host import planner  # noqa: F401  (the fixture: plan_call_route() built with g++)
from tests.test_parity_gpu import TOL, TOL_DB
from tests.test_streambank_conditioners_host import MARGIN, Chain, smallest_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
DEVICE_FACTS = ["dec_lds_free_front", "dec_raw_front", "spec_raw_ready", "spec_dec_ready", "dec_triple_out", "dec_fuse_shape", "osc_transient"]


# ------------------------------------------------------------------------------------------------
# the accessor: declared, bound, exported, and NULL without a handle
# ------------------------------------------------------------------------------------------------
def test_the_accessor_is_declared_bound_and_exported():
    import pebblesdr_amd as P
    from pebblesdr_amd.binding import SYMBOLS
    header = open(os.path.join(ROOT, "include", "pebblegpu.h")).read()
    assert len(re.findall(r"\bpebblegpu_receiver_conditioned\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))) == 1
    assert SYMBOLS.count("pebblegpu_receiver_conditioned") == 1
    L = P.load_library()
    assert L.pebblegpu_receiver_conditioned.argtypes is not None and hasattr(P.ReceiverBank, "conditioned")
    n, pitch = C.c_uint64(7), C.c_uint64(7)
    assert L.pebblegpu_receiver_conditioned(None, C.byref(n), C.byref(pitch)) is None
    assert (n.value, pitch.value) == (0, 0)
    assert L.pebblegpu_receiver_conditioned(None, None, None) is None
    assert L.pebblegpu_set_conditioners(None, 0, 2, float("nan"), 0.0) == E_INVALID
    assert "pebblegpu_receiver_conditioned" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
def test_the_table_is_well_formed():
    assert list(CC.ROWS) == ["flags", "lists", "frame4096", "switching", "negative_gain", "two_stage", "raw", "generator", "gated", "downstream", "recording", "wfm"]
    assert CC.WRONG_FACTOR == 100 and (CC.TOL, CC.TOL_DB, CC.MARGIN) == (TOL, TOL_DB, MARGIN) == (1e-5, 0.1, 1e-4)
    for row in CC.ROWS.values():
        assert row.why and len(row.levels) == len(row.calls) and max(row.calls) <= row.max_sf
        assert row.sf % row.nf == 0 and row.S == (1 if row.shared else row.C)
        assert row.sf == (CC.WFM_D * row.nf if row.wfm else CC.D * math.lcm(row.nf, 1024))   # design::superframe_len
        for c, s, f, g, p in row.script:
            assert 0 <= c < len(row.calls) and 0 <= s < row.S and 0 <= f <= 15 and np.isfinite([g, p]).all()
        x = CC.row_input(row.name)
        assert x.shape == (row.S, CC.total(row)) and x.dtype == np.complex64 and np.isfinite(x).all()
        assert row.fs == (CC.WFM_FS if row.name == "wfm" else CC.FS)
    for model, (rows, what) in CC.WRONG.items():
        assert what and rows and all(r in CC.ROWS for r in rows)
    assert len(CC.WRONG) == 15


def test_every_row_reaches_what_it_is_there_for():
    R = CC.ROWS
    fl = {name: CC.flags_during(R[name]) for name in R}
    # flags: every stage alone and together; three of four calls shorter than the copy's pitch
    r = R["flags"]
    assert fl["flags"][0] == [0, 1, 2, 4, 8, 15] and sum(n < r.max_sf * r.sf for _, n in CC.call_bounds(r)) == 3
    assert len({(CC.GAINS6[s], CC.PHASES6[s]) for s in range(6)}) == 6
    # lists: a second workgroup of k_noise_blank with blankers in it, list positions that are not ids, a rebuilt list
    r = R["lists"]
    assert r.S > 64 and -(-r.S // 64) == 2 and any(fl["lists"][0][s] & 12 for s in range(64, r.S)) and any(fl["lists"][0][s] & 12 for s in range(64))
    assert CC.dc_list(r, 0) == [1, 64, 65] and CC.dc_list(r, 1) == [63, 64, 65]
    assert all(s != pos for pos, s in enumerate(CC.dc_list(r, 0))) and CC.dc_list(r, 0)[0] != CC.dc_list(r, 1)[0]
    assert sorted(s for s in range(r.S) if fl["lists"][0][s]) == [0, 1, 63, 64, 65] and len({fl["lists"][0][s] for s in (0, 1, 63, 64, 65)}) == 5
    assert fl["lists"][1][1] & 1 == 0 and fl["lists"][0][63] & 1 == 0 and fl["lists"][1][63] & 1 == 1
    # frame4096: frames of 4096 with IQ balance on both streams
    r = R["frame4096"]
    assert r.nf == 4096 and all(f & 2 for f in fl["frame4096"][0]) and fl["frame4096"][0] == [2, 15]
    # switching
    r = R["switching"]
    assert fl["switching"] == [[15, 13], [0, 1], [15, 15], [15, 15], [3, 0]] and r.levels[:3] == (1.0, 0.5, 2.0)
    again = CC.setters_before(r, 3)
    assert [a[1] for a in again] == [15, 15] and [a[2:] for a in again] != [a[2:] for a in CC.setters_before(r, 2)]   # the setter with the flags on, another gain
    # negative_gain
    assert [(f, g) for _, f, g, _ in CC.setters_before(R["negative_gain"], 0)] == [(2, -0.97), (15, -0.97)]
    # two_stage: no display transform, three channels off one stream, flags on for call 2 alone
    r = R["two_stage"]
    assert (r.bins, r.C, r.S, r.shared) == (0, 3, 1, True) and [f[0] for f in fl["two_stage"]] == [0, 0, 15, 0, 0, 0]
    # raw
    assert (R["raw"].S, fl["raw"][0], len(R["raw"].calls)) == (3, [15, 0, 5], 3) and CC.row_raw("raw").dtype == np.int16
    assert any(n < R["raw"].max_sf * R["raw"].sf for _, n in CC.call_bounds(R["raw"]))
    # gated: the timer lists some frames of every call, not all
    r = R["gated"]
    t = GateTimer(r.nf, r.fs)
    t.set_updates(CC.GATE_UPS)
    for _, n in CC.call_bounds(r):
        sel = t.call(n // r.nf)
        assert 2 <= len(sel) < n // r.nf // 2
    assert fl["gated"][0] == [5, 5] and any(n < r.max_sf * r.sf for _, n in CC.call_bounds(r))   # in_pitch = cap differs from n
    assert (R["downstream"].hires, fl["downstream"][0]) == (2048, [1]) and CC.band_of(R["downstream"])[0] < -CC.mixer_of(R["downstream"], 0) < CC.band_of(R["downstream"])[1]
    assert np.abs(CC.row_input("recording")).max() < 1.0   # the PCM16 conversion does not saturate
    assert (R["wfm"].fs, R["wfm"].wfm, R["wfm"].calls, fl["wfm"][0]) == (20000000, True, (1, 2), [15])
    # every row that runs NB1: a spike within 6 samples in front of every call boundary (the count crosses it), spikes around every frame
    # boundary, the run of 40 across the second call's start; a quiet stream beside a stream that keeps the -3 spike
    for name, r in R.items():
        nb1 = [s for s in range(r.S) if any(f[s] & 4 for f in fl[name])]
        if not nb1:
            continue
        x = np.abs(CC.row_input(name))
        keeps = [s for s in nb1 if s not in r.quiet]
        assert keeps, name
        for s in nb1:
            pos = CC.spike_positions(r, s)
            for e in range(r.nf, CC.total(r), r.nf):
                call_edge = e in [lo for lo, _ in CC.call_bounds(r)]
                want = (2, 5) if (call_edge and s in r.quiet) else (-3, 2, 5)
                assert all(e + o in pos for o in want) and ((e - 3 in pos) == (-3 in want)), (name, s, e)
                assert all(x[s, e + o] > 0.5 * min(r.levels) for o in want), (name, s, e)   # (the tones and the offset: 0.08 of the level)
            b = CC.call_bounds(r)[1][0]
            assert CC.run_start(r) == b - 20 and (x[s, b - 20:b + 20] > 0.5 * min(r.levels)).all()
    assert R["flags"].quiet == (3,) and R["switching"].quiet == (1,) and R["raw"].quiet == (2,)


# ------------------------------------------------------------------------------------------------
# the oracle driver
# ------------------------------------------------------------------------------------------------
def test_the_model_is_the_stream_banks_chain(oracle_mod):
    """Model (whole calls) against Chain (frame by frame) with the same setter calls: the same bits, and the same recorded blanker inputs"""
    row = CC.ROWS["switching"]
    x = CC.oracle_input(row.name)
    got, ms = CC.right(oracle_mod, row.name)
    for s in range(row.S):
        ch = Chain(oracle_mod, row.fs, row.nf)
        for k, (lo, n) in enumerate(CC.call_bounds(row)):
            for st, f, g, p in CC.setters_before(row, k):
                if st == s:
                    ch.set(f, g, p)
            want = ch.process(x[s, lo:lo + n]) if ch.flags else x[s, lo:lo + n]
            assert np.array_equal(got[k][s], want), (s, k)
        assert abs(smallest_margin(ch.nb_in) - smallest_margin(ms[s].nb_in)) <= 1e-12


def test_the_python_restatement_of_nb1_is_the_oracles(oracle_mod):
    """the `nb1_six` model restates NB1 in Python to change its blanking length; with the reference's 7 it is the oracle's NB1 bit for bit,
    across a call boundary"""
    row = CC.ROWS["flags"]
    x = CC.oracle_input("flags")[5, :2 * row.nf + 100]
    m = CC.Model(oracle_mod, row.fs, row.nf)
    m.set(4)
    nb = oracle_mod.NoiseBlanker()
    nb.enable(1)
    for lo, hi in ((0, row.nf + 1), (row.nf + 1, len(x))):
        a, b = m._nb1_python(x[lo:hi], 7), nb.process(x[lo:hi], which=1)
        assert np.array_equal(a, b) and np.count_nonzero(b == 0) > 20
    assert m.py["avg"] == float(nb.s.nb_avg_mag) and m.py["cnt"] == nb.s.spike_count


def test_the_chain_then_a_plain_receiver_is_the_receiver_with_conditioners(oracle_mod):
    """what the old observables are computed from: the right chain's output fed to an oracle Receiver WITHOUT conditioners gives the
    audio and the spectrum rows of the oracle Receiver given the script through set_conditioners, bit for bit"""
    row = CC.ROWS["switching"]
    cond, _ = CC.right(oracle_mod, row.name)
    audio, rows = CC.observables(oracle_mod, row, cond)
    calls = CC.receiver_oracles(oracle_mod, row)
    for c in range(row.C):
        assert np.array_equal(audio[c], np.concatenate([a[c] for a, _ in calls]))
        assert np.array_equal(rows[c], np.concatenate([r[c] for _, r in calls]))


# ------------------------------------------------------------------------------------------------
# the margin condition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, r in CC.ROWS.items() if any(f & 12 for _, _, f, _, _ in r.script)])
def test_the_margin_condition_holds(oracle_mod, name):
    """a condition on the INPUT (tests/test_streambank_conditioners_host.py).  Seeds that miss it are noted at the rows (cond_cases.ROWS), as
    that file notes them: `lists` with seed 300, 4.5e-6"""
    _, ms = CC.right(oracle_mod, name)
    CC.assert_margin(ms, name)
    zeros = sum(int(np.count_nonzero(c == 0)) for c in CC.right(oracle_mod, name)[0] if c is not None)
    print("%s: %d exact zeros in the oracle's conditioned streams" % (name, zeros))
    if any(f & 4 for _, _, f, _, _ in CC.ROWS[name].script):
        assert zeros > 100


# ------------------------------------------------------------------------------------------------
# routes
# ------------------------------------------------------------------------------------------------
def test_every_call_plans_the_route_the_table_names(planner):  # noqa: F811
    """with a conditioner on or a change pending: no side, no bank_pipe, no plain, no raw_fused, whatever the cores could do; staged where
    the row is raw or generated.  The two_stage row: bank_pipe before the change (plain from its second call on) and after it again"""
    seen = set()
    for row in CC.ROWS.values():
        for k in range(len(row.calls)):
            facts, want = CC.call_facts(row, k), CC.route_of(row, k)
            for bits in range(1 << len(DEVICE_FACTS)):
                f = dict(facts, pipeline=1, **{d: (bits >> i) & 1 for i, d in enumerate(DEVICE_FACTS)})
                got = planner(**f)
                assert {key: got[key] for key in want} == want, (row.name, k, f, got)
            seen.add((row.name, want["bank_pipe"], want["plain"], want["staged"]))
    assert [CC.route_of(CC.ROWS["two_stage"], k)["bank_pipe"] for k in range(6)] == [1, 1, 0, 0, 1, 1]
    assert [CC.route_of(CC.ROWS["two_stage"], k)["plain"] for k in range(6)] == [0, 1, 0, 0, 1, 1]
    assert ("raw", 0, 0, 1) in seen and ("generator", 0, 0, 1) in seen and ("flags", 0, 0, 0) in seen


# ------------------------------------------------------------------------------------------------
# the wrong models
# ------------------------------------------------------------------------------------------------
_GOOD_OBS = {}


def _good_obs(O, name):
    if name not in _GOOD_OBS:
        _GOOD_OBS[name] = CC.observables(O, CC.ROWS[name], CC.right(O, name)[0])
    return _GOOD_OBS[name]


@pytest.mark.parametrize("model", list(CC.WRONG))
def test_every_wrong_model_misses_the_new_comparison(oracle_mod, model):
    """each model is one change to the oracle chain, compared with the right chain by the comparison the GPU tier makes of conditioned()
    (spectrum_raw: of the spectrum rows, the one thing it changes).  New: bars of that comparison; old: bars of the USB audio and of the
    spectrum rows"""
    best = 0.0
    for name in CC.WRONG[model][0]:
        row = CC.ROWS[name]
        good, _ = CC.right(oracle_mod, name)
        if model == "spectrum_raw":
            bad = good
            old = CC.old_factor(_good_obs(oracle_mod, name), CC.observables(oracle_mod, row, good, spectrum_raw=True))
            new = old[1]
        else:
            bad, _ = CC.conditioned(oracle_mod, row, model)
            new = CC.new_factor(row, good, bad)
            old = CC.old_factor(_good_obs(oracle_mod, name), CC.observables(oracle_mod, row, bad))
        print("wrong model %-18s row %-14s new comparison %10.3g bars | old observables: audio %10.3g bars, spectrum %10.3g bars" % (model, name, new, old[0], old[1]))
        assert np.isfinite(new) and np.isfinite(old).all()
        best = max(best, new)
    assert best >= CC.WRONG_FACTOR, (model, best)
