"""CPU tier of the dmFMS coverage statement (tests/rds_cases.py): no device.

  1. the path table: csrc/design.cpp's RDS chain, tap counts, matched-filter length and shortest call per row, WfmCore::init's rule
     giving the one-kernel path at every row, no stage of design 0 anywhere dmFMS is accepted;
  2. the plain fp64 model (tests/rds_ref.py) against oracle.DemodWFM on every row and script: m_RdsData of every call to 1e-9 with
     the device tier's metric, the bit sequence exactly.  Measured: 2.4e-14 (100 000), 1.4e-11 (125 000), 1.2e-11 (256 000),
     1.8e-11 (312 500), 1.1e-12 (384 000), 3.3e-12 (512 000);
  3. the wrong models: every fault of rds_ref.FAULTS in front of the bit slicer misses m_RdsData by at least 100 bars on some call of
     every row's script (measured: 0.18 .. 170, i.e. 1.8e5 bars and more), losing the slicer's state changes the bits, folding the PLL's
     phase somewhere else than at the call's end stays inside the bar;
  4. input B reaches the block synchroniser's error paths and input C overruns the 100-entry queue, in the oracle."""
import numpy as np
import pytest

import oracle as O
from tests import rds_cases as RC
from tests import rds_ref as RR
from tests.demod_cases import MIN_CALL


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle_mod):
    """(conftest's fixture builds the oracle's library; the module-level import below is the same module)"""
    assert oracle_mod is O


_CACHE = {}


def oracle_a(row):
    if row.name not in _CACHE:
        _CACHE[row.name] = RC.run_oracle(O, row.rate, RC.input_a(row), RC.script_a(row))
    return _CACHE[row.name]


# ------------------------------------------------------------------------------------------------
# 1. the path table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", RC.RDS_ROWS, ids=lambda r: r.name)
def test_row_is_what_design_cpp_builds(row):
    des = RC.rds_design(row.rate)
    assert tuple(zip(des.stages, des.stage_taps)) == row.stages
    assert [len(h) for h in des.stage_h] == [t for _, t in row.stages]          # what RdsCore::init uploads
    assert 1 << len(des.stages) == row.D
    assert des.rds_rate == row.rds_rate == row.rate / row.D
    assert len(des.matched) == row.mtaps
    assert len(des.lp) == 75 and len(des.hilb_i) == 61
    assert RC.rds_min_call(des) == row.rds_min
    assert row.mb == max(row.rds_min, -(-MIN_CALL // row.D) * row.D) and row.mb % row.D == 0
    assert RC.wfm_design(row.rate).fused                                        # WfmCore::set_stereo refuses dmFMS otherwise
    assert O.DemodWFM(float(row.rate)).rds_rate == row.rds_rate                 # the oracle's chain is as long


def test_rows_cover_every_stage_design_in_use_and_none_is_the_cic3():
    seen = sorted({s for row in RC.RDS_ROWS for s, _ in row.stages})
    assert tuple(seen) == RC.ALL_STAGE_DESIGNS and 0 not in seen
    # k_rds_fir's newest = 1 (design 0) has no caller: wherever the one-kernel path exists, the chain is made of half-bands only
    fused = [r for r in range(50000, 3000001, 12500) if RC.wfm_design(r).fused]
    assert len(fused) >= 20 and all(r in fused for r in (100000, 125000, 250000, 312500, 387500, 512500))
    for r in fused:
        st = RC.rds_design(r).stages
        assert 0 not in st and len(st) >= 1, (r, st)            # (rates between the rows pick other half-bands: 3, 8 at 112 500)


@pytest.mark.parametrize("row", RC.RDS_ROWS, ids=lambda r: r.name)
def test_script_has_the_geometries_it_is_there_for(row):
    sc = RC.script_a(row)
    ok = [c.n for c in sc if c.ok]
    des = RC.rds_design(row.rate)
    assert all(n % row.D == 0 and row.mb <= n <= RC.CAP for n in ok)
    assert ok.count(RC.CAP) == 1 and len(ok) >= 3 * 10 + 1                       # the capacity once, three cycles and more
    look_back = max(len(des.lp) - 1, len(des.matched) - 1)
    assert row.mb // row.D < min(len(des.lp) - 1, len(des.matched) - 1)         # n < hist in the low-pass row and in mag
    pairs = list(zip(ok, ok[1:]))
    assert any(a // row.D >= look_back > b // row.D for a, b in pairs)          # short after long
    assert any(b // row.D >= look_back > a // row.D for a, b in pairs)          # long after short
    assert any(a // row.D < look_back and b // row.D < look_back for a, b in pairs)  # short after short
    bad = [c.n for c in sc if not c.ok]
    assert bad == RC.refused_lengths(row)
    assert bad[0] < row.mb and bad[0] % row.D == 0 and bad[1] % row.D != 0 and row.mb < bad[1] < RC.CAP and bad[2] > RC.CAP and bad[2] % row.D == 0
    for i, c in enumerate(sc):                                                  # every refused call sits between two valid ones
        if not c.ok:
            assert 0 < i < len(sc) - 1 and sc[i - 1].ok and sc[i + 1].ok
    assert sum(ok) > 0.95 * len(RC.input_a(row))


# ------------------------------------------------------------------------------------------------
# 2. the plain model against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", RC.RDS_ROWS, ids=lambda r: r.name)
def test_plain_model_is_the_oracle(row):
    ref = oracle_a(row)
    data, bits = RR.run_model(RC.rds_design(row.rate), RC.input_a(row), RC.offsets(RC.script_a(row)))
    e = RC.call_errors(data, ref.data)
    print("%s: model against oracle, worst call %.3e (call %d of %d), %d bits" % (row.name, max(e), int(np.argmax(e)), len(e), len(bits)))
    assert max(e) <= RC.MODEL_TOL
    assert len(bits) > 2000 and np.array_equal(bits, ref.bits)
    assert len(ref.popped) >= 4                              # the decoder works on every row's input


# ------------------------------------------------------------------------------------------------
# 3. the wrong models
# ------------------------------------------------------------------------------------------------
def _first_miss(row, fault, stage=0):
    """runs the wrong model call by call until a call misses the oracle's m_RdsData by 100 bars -> (error, call index) or None"""
    ref = oracle_a(row)
    whole = RC.rms(np.concatenate(ref.data))
    m = RR.RdsModel(RC.rds_design(row.rate), (fault,), stage)
    x = RC.input_a(row)
    for k, (o, n) in enumerate(RC.offsets(RC.script_a(row))):
        e = RC.rms(m.process(x[o:o + n]) - ref.data[k]) / max(RC.rms(ref.data[k]), whole)    # call_errors, one call at a time
        if e >= 100 * RC.RDS_TOL:
            return e, k
    return None


SIGNAL_FAULTS = [f for f in RR.FAULTS if f not in ("slicer_state", "pll_fold_block")]


@pytest.mark.parametrize("fault", SIGNAL_FAULTS)
@pytest.mark.parametrize("row", RC.RDS_ROWS, ids=lambda r: r.name)
def test_wrong_model_misses_the_bar(row, fault):
    for stage in (range(len(row.stages)) if fault == "stage_hist" else (0,)):
        miss = _first_miss(row, fault, stage)
        assert miss is not None, (fault, stage)
        print("%s %s stage %d: %.2e at call %d" % (row.name, fault, stage, miss[0], miss[1]))


def test_the_metric_of_the_wrong_models_is_the_shared_one():
    """_first_miss restates call_errors for one call; hold the two together"""
    row = RC.RDS_ROWS[0]
    ref = oracle_a(row)
    got = [d * (1 + 1e-5) for d in ref.data[:20]] + list(ref.data[20:])
    e = RC.call_errors(got, ref.data)
    whole = RC.rms(np.concatenate(ref.data))
    for k in (0, 1, 19, 20):
        assert e[k] == RC.rms(got[k] - ref.data[k]) / max(RC.rms(ref.data[k]), whole)
    assert max(e[:20]) <= 1e-5 * (1 + 1e-9) and max(e[20:]) == 0.0


@pytest.mark.parametrize("row", RC.RDS_ROWS, ids=lambda r: r.name)
def test_lost_slicer_state_changes_the_bits(row):
    ref = oracle_a(row)
    data, bits = RR.run_model(RC.rds_design(row.rate), RC.input_a(row), RC.offsets(RC.script_a(row)), ("slicer_state",))
    assert max(RC.call_errors(data, ref.data)) <= RC.MODEL_TOL                    # m_RdsData lies in front of the slicer
    assert not np.array_equal(bits, ref.bits)


@pytest.mark.parametrize("row", RC.RDS_ROWS, ids=lambda r: r.name)
def test_folding_the_pll_phase_elsewhere_stays_inside_the_bar(row):
    """the reference folds the phase at the end of a call; the device folds at the end of every reference-sized block of a longer call"""
    ref = oracle_a(row)
    data, bits = RR.run_model(RC.rds_design(row.rate), RC.input_a(row), RC.offsets(RC.script_a(row)), ("pll_fold_block",))
    e = max(RC.call_errors(data, ref.data))
    print("%s: folded every 7 samples, worst call %.3e" % (row.name, e))
    assert e <= RC.RDS_TOL / 100 and np.array_equal(bits, ref.bits)


# ------------------------------------------------------------------------------------------------
# 4. inputs B and C reach what they are there for
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["equal", "mixed"])
def test_input_b_reaches_the_error_paths(pattern):
    sent = RC.groups_b()
    r = RC.run_oracle(O, RC.B_RATE, RC.input_b(), RC.scripts_b()[pattern])
    pushed = [g for call in r.pushed for g in call]
    # (a) the three damaged groups are pushed, corrected: checkBlock's Meggitt decoder ran and found the burst
    for k in RC.B_DAMAGED:
        assert tuple(sent[k]) in pushed, k
    # (b) one zero group: more than five block errors in the noise, the queue cleared (STATE_GROUPRESYNC lies on the way there: the
    #     first five errors each skip to the next group)
    assert pushed.count((0, 0, 0, 0)) == 1
    zero_at = pushed.index((0, 0, 0, 0))
    assert all(tuple(sent[k]) not in pushed for k in RC.B_NOISE)
    # (c) getNextRdsGroupData returns changed = 0 twice: the group sent three times
    flags = [c for _, c in r.popped]
    assert flags.count(False) == 2
    same = [g for g, c in r.popped if not c]
    assert same == [tuple(sent[RC.B_TRIPLE])] * 2
    # (d) decoding resumes: groups from behind the noise are pushed behind the zero group, in order
    later = [sent.index(g) for g in pushed[zero_at + 1:]]
    assert later == sorted(later) and later[0] > RC.B_NOISE[-1] and len(later) >= 12
    assert [g for g, _ in r.popped] == pushed[:len(r.popped)]


def test_input_c_overruns_the_group_queue():
    sent = RC.groups_c()
    r = RC.run_oracle(O, RC.C_RATE, RC.input_c(), RC.equal_script(len(RC.input_c()), RC.C_CALL))
    assert len(r.audio) == RC.C_CALLS
    per_call = [len(c) for c in r.pushed]
    assert sum(per_call) > RC.Q_SIZE + RC.C_CALLS and max(per_call) == 3        # about three pushed, one popped per call
    idx = [sent.index(g) for g, _ in r.popped]
    jumps = [(i, b - a) for i, (a, b) in enumerate(zip(idx, idx[1:])) if b - a != 1]
    print("input C: %d popped, sequence breaks %r" % (len(idx), jumps))
    assert len(jumps) == 1 and jumps[0][1] == RC.Q_SIZE + 1                     # head has lapped tail: 100 groups are gone
    assert jumps[0][0] >= 40 and len(idx) - jumps[0][0] >= 8                    # ... with groups read on both sides of the gap
