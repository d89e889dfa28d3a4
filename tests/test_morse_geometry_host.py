"""CPU tier of the Morse geometry table (tests/morse_cases.py): no device.

1. The table against literals: chain, total decimation, modem rate, N, frames, modem samples a call, and which rows complete no block in
   most calls, end every call on a block boundary or give more than 64 results a call -- every row sits on the path it is there for.
2. Call-split invariance of the restatement: MorseRef fed frame by frame equals MorseRef fed the whole stream in one frame (two, around
   the mode change): events and decisions identical, powers within 1e-12 relative.  The device's design -- state carried between calls
   in the stage tails, the Goertzel sums and the clock -- rests on this.
3. Discrimination: each deliberately wrong model (morse_cases.WrongRef) fails the GPU tier's own comparison (morse_cases.check_against:
   counts, decisions, powers at 1e-5, events, status) on the rows named in WRONG_ROWS, and the stage-by-stage decimator those models are
   built on passes it when nothing is wrong.
"""
import numpy as np
import pytest

from tests import morse_cases as MC
from tests import morse_ref as M

# rate: (chain, total, chain rate, modem rate, N, frames (min, N total, (N+1) total, 67 N total))
TABLE = {
    8000: ([], 1, 8000.0, 8000, 80, (8, 80, 81, 5360)),
    12000: ([(15, 2)], 2, 6000.0, 6000, 60, (16, 120, 122, 8040)),
    31250: ([(11, 2), (15, 2)], 4, 7812.5, 7812, 78, (32, 312, 316, 20904)),
    37500: ([(11, 2), (15, 2), (19, 2)], 8, 4687.5, 4687, 46, (80, 368, 376, 24656)),
    48000: ([(11, 4), (15, 2)], 8, 6000.0, 6000, 60, (64, 480, 488, 32160)),
    64000: ([(11, 4), (15, 2)], 8, 8000.0, 8000, 80, (64, 640, 648, 42880)),
    96000: ([(11, 8), (15, 2)], 16, 6000.0, 6000, 60, (128, 960, 976, 64320)),
    256000: ([(11, 16), (15, 2)], 32, 8000.0, 8000, 80, (256, 2560, 2592, 171520)),
}
# modem samples a call at the four frames
PER_CALL = {8000: (8, 80, 81, 5360), 12000: (8, 60, 61, 4020), 31250: (8, 78, 79, 5226), 37500: (10, 46, 47, 3082),
            48000: (8, 60, 61, 4020), 64000: (8, 80, 81, 5360), 96000: (8, 60, 61, 4020), 256000: (8, 80, 81, 5360)}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


def test_the_table_against_literals(oracle_mod):
    assert MC.RATES == list(TABLE)
    assert len(MC.rows()) == 32
    for rate, (chain, total, chain_rate, modem, n, frames) in TABLE.items():
        d = oracle_mod.Decimator(rate, 1000, 8000)
        assert d.chain() == chain and d.rate == chain_rate, rate
        assert MC.geometry(rate) == (chain, total, modem, n), rate
        assert tuple(MC.frames(rate)) == frames, rate
        assert tuple(MC.per_call(rate, f)[0] for f in frames) == PER_CALL[rate], rate
        # min: the limit of MorseCore::check -- one multiple of the decimation less starves a stage (8000 has none: any frame would do)
        if chain:
            ln, starved = frames[0] - total, False
            for t, s in chain:
                starved = starved or ln < t
                ln //= s
            assert starved and frames[0] % total == 0, rate
        m = PER_CALL[rate]
        # min: 8 or 10 modem samples a call, under a quarter of a block: at least three calls in four complete none
        assert m[0] in (8, 10) and m[0] * 4 < n, rate
        # N total: every call ends on a block boundary; (N+1) total: the phase moves by one and N + 1 is coprime to N, so it takes
        # every position; 67 N total: 67 results a call, more than the 64 lanes, and on a boundary too
        assert m[1] == n and m[2] == n + 1 and m[3] == 67 * n, rate
    # every form of the chain: none, one, two and three stages; strides 2, 4, 8, 16; a fractional rate truncated, twice
    assert sorted(len(v[0]) for v in TABLE.values()) == [0, 1, 2, 2, 2, 2, 2, 3]
    assert {s for v in TABLE.values() for _, s in v[0]} == {2, 4, 8, 16}
    assert [r for r, v in TABLE.items() if v[2] != v[3]] == [31250, 37500]


@pytest.mark.parametrize("row", MC.REFUSALS, ids=lambda r: "%d-%d" % r[:2])
def test_the_refusal_rows_are_refusals(oracle_mod, row):
    """why MorseCore::init / check must refuse each: worked from the oracle's chain, not from the library"""
    rate, frame, code = row
    d = oracle_mod.Decimator(rate, 1000, 8000)
    chain = d.chain()
    if rate == 390625:
        assert chain[0][0] == 0 and code == "E_UNSUPPORTED"       # the CIC stage
    elif rate == 50:
        assert chain == [] and M.best_n(int(d.rate)) == 0 and code == "E_UNSUPPORTED"
    elif frame == 60:
        assert frame % d.total_decimation != 0 and code == "E_SIZE"
    else:
        assert frame % d.total_decimation == 0 and frame // chain[0][1] == 14 < chain[1][0] and code == "E_SIZE"


def test_every_row_decodes_with_margin():
    """the condition of every row (no tolerance): every restated decision at least 1e-4 of the power away from its thresholds, the
    stream decoded, and more calls than the event log has entries at the min frame"""
    worst = {}
    for rate, frame in MC.rows():
        ref = MC.reference(rate, frame)
        assert min(ref.margins) > MC.MARGIN, (rate, frame, min(ref.margins))
        got = [(k, t) for _, t, k in ref.events]
        assert got[-len(M.text_tokens(MC.TEXT2)):] == M.text_tokens(MC.TEXT2), (rate, frame)
        worst[rate] = min(worst.get(rate, 1.0), min(ref.margins))
        x, _ = MC.stream(rate, frame)
        if frame == MC.frames(rate)[0]:
            assert len(x) // frame > 1024 + 2, (rate, frame)
    print("smallest margin per rate:", {r: "%.2e" % v for r, v in worst.items()})


@pytest.mark.parametrize("rate", MC.RATES)
def test_call_split_invariance_of_the_restatement(rate):
    """frame by frame == in one piece (the stream in two calls, split where the mode changes), at all four frames of the rate"""
    for frame in MC.frames(rate):
        ref = MC.reference(rate, frame)
        x, n1 = MC.stream(rate, frame)
        whole = M.MorseRef(rate, len(x))
        whole.process(x[:n1])
        whole.set_demod_mode(M.DM_CWU)
        whole.process(x[n1:])
        assert whole.events == ref.events and len(ref.events) > 0, (rate, frame)
        assert whole.tones == ref.tones, (rate, frame)
        a, b = np.array(whole.powers), np.array(ref.powers)
        assert len(a) == len(b) == len(x) // (MC.geometry(rate)[1] * MC.geometry(rate)[3])
        assert np.max(np.abs(a - b) / np.maximum(b, 1e-300)) <= 1e-12, (rate, frame)
        assert whole.status() == ref.status()


# model -> [(rate, frame, stage)]: the rows on which it must fail the GPU tier's comparison
WRONG_ROWS = {
    # (a) shows wherever calls do not end on block boundaries: the min and the sliding frames
    "goertzel_reset": [(37500, 80, None), (12000, 122, None), (8000, 8, None)],
    # (b) shows everywhere, the boundary rows included (cnt0 = 0 there at every call)
    "phase_late": [(8000, 80, None), (64000, 42880, None)],
    "phase_early": [(8000, 80, None), (64000, 42880, None)],
    # (c) one model per stage index of the one-, two- and three-stage chains, at the min frame (nearly every tap from the tail) and
    # at the largest (one call start in 67 blocks)
    "stage_zeroed": [(12000, 16, 0), (37500, 80, 0), (37500, 80, 1), (37500, 80, 2), (256000, 256, 0), (256000, 256, 1),
                     (31250, 20904, 0), (31250, 20904, 1), (37500, 24656, 2)],
    # (d) shows at the two fractional rates
    "rate_untruncated": [(31250, 316, None), (31250, 32, None), (37500, 24656, None), (37500, 368, None)],
    # (e) N = 59 at a modem rate of 6000
    "usec_rounded": [(12000, 120, None), (48000, 488, None), (96000, 64320, None)],
    # (f), (g) show at the min frames only
    "clock_skips_empty_calls": [(8000, 8, None), (37500, 80, None), (256000, 256, None)],
    "log_not_drained": [(8000, 8, None), (31250, 32, None), (256000, 256, None)],
}
WRONG_CASES = [(w, r, f, j) for w, rows in WRONG_ROWS.items() for r, f, j in rows]


def test_every_wrong_model_has_its_rows():
    assert set(WRONG_ROWS) == set(MC.WRONG)
    assert all((r, f) in MC.rows() for _, r, f, _ in WRONG_CASES)
    assert {r for r, _, _ in WRONG_ROWS["rate_untruncated"]} == {31250, 37500}
    assert {r for r, _, _ in WRONG_ROWS["usec_rounded"]} == {12000, 48000, 96000}
    # every stage index of every chain length
    assert {(len(MC.geometry(r)[0]), j) for r, _, j in WRONG_ROWS["stage_zeroed"]} == {(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)}


@pytest.mark.parametrize("wrong,rate,frame,stage", WRONG_CASES, ids=lambda v: str(v))
def test_wrong_models_fail_the_gpu_tiers_comparison(wrong, rate, frame, stage):
    ref = MC.reference(rate, frame)
    model = MC.wrong_run(rate, frame, wrong, stage)
    with pytest.raises(AssertionError):
        MC.check_model(ref, model)


@pytest.mark.parametrize("rate,frame", sorted({(r, f) for r, f, _ in WRONG_ROWS["stage_zeroed"]}))
def test_the_stage_model_with_nothing_wrong_passes(rate, frame):
    """the fp64 stage-by-stage decimator (k_morse_fir's indexing) against the oracle's Decimator, through the same comparison"""
    MC.check_model(MC.reference(rate, frame), MC.wrong_run(rate, frame, None, stage_model=True))


def test_models_that_need_a_geometry_pass_elsewhere():
    """why the table needs its rows: the defects a boundary-aligned call hides, and the ones only a fractional rate, a modem rate of 6000
    or a call without a result shows"""
    for wrong, rate, frame in (("goertzel_reset", 64000, 640), ("goertzel_reset", 8000, 5360), ("rate_untruncated", 64000, 648),
                               ("usec_rounded", 64000, 648), ("usec_rounded", 31250, 316), ("clock_skips_empty_calls", 12000, 122),
                               ("log_not_drained", 48000, 488)):
        MC.check_model(MC.reference(rate, frame), MC.wrong_run(rate, frame, wrong))
