"""GPU tier (-m gpu) of tests/modem_geom_cases.py: k_modem_rate_pack at every tile, chain depth and carry path the plan accepts at a
receiver's rate -- ragged and halved tiles, D up to 128, four stages, spans that are mostly look-back, a carry whose samples come from
the look-back, the sample-by-sample store.  The table, the streams and the coverage statement: tests/modem_geom_cases.py; the CPU tier
(tests/test_modem_geom_host.py) holds the table to the plan and the header and a plain model of the algorithm to the oracle.

As tests/test_modem_rate_gpu.py: the bank with the rate ring runs beside a twin with the plain F32 ring (modem_rate_cases.hold_row);
flags equal the twin's, absent pairs are zeros, every present pair -- the very first included -- is within modem_out_cases.PAIR_BAR of
oracle.Decimator fed the twin's present pairs; S16 rows are exactly the host twin of the F32 ring's rows; audio and kernel names are a
bank's without a ring.  Every test prints its worst figure."""
import numpy as np
import pytest

from tests import modem_geom_cases as GC
from tests import modem_out_cases as MC
from tests import modem_rate_cases as RC
from tests import tail_cases as TC
from tests.test_modem_rate_gpu import close_all, hold_blocks, refused

pytestmark = pytest.mark.gpu


def signal_holds(O, twin, rows, rate, bw, mn, spf, label):
    """the signal condition: the oracle's output RMS of every present pair is at least MIN_GAIN of the pair's input RMS"""
    low = 1e9
    for r in range(rows):
        fed = [y for _, _, p, y in RC.pairs_of(twin, r, spf) if p]
        for y, z in zip(fed, RC.decimated(O, rate, bw, mn, fed)):
            low = min(low, GC.rms(z) / GC.rms(y))
    print("%s: output / input RMS of a present pair at least %.3f (>= %.2f)" % (label, low, GC.MIN_GAIN))
    assert low >= GC.MIN_GAIN, (label, low)


def s16_is_the_twin_of(P, got16, got):
    for k, (b16, b32) in enumerate(zip(got16, got)):
        assert b16[2].dtype == np.int16 and b16[2].shape == b32[2].shape
        want = np.stack([P.modem_out_convert(MC.S16, b32[2][r]) for r in range(b32[2].shape[0])])
        assert b16[2].tobytes() == want.tobytes(), "call %d: the S16 rows are not the host twin of the F32 rows" % k
        assert np.array_equal(b16[3], b32[3]) and (b16[0], b16[1], b16[4]) == (b32[0], b32[1], b32[4])


# ------------------------------------------------------------------------------------------------
# 1. every row, both formats
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.ROWS))
def test_every_row_in_both_formats(gpu_lib, oracle_mod, name):
    import pebblesdr_amd as P
    row = GC.ROWS[name]
    rate, sfw, sel = GC.demod_rate(row), row.spf * GC.front(row), row.sel
    a, s, b, n = (GC.bank(P, row) for _ in range(4))   # F32 rate ring; S16 rate ring; plain F32 ring; no ring
    try:
        assert a.superframe == sfw and int(a.info.demod_rate_int) == rate and a.D == GC.front(row)
        info = P.modem_rate_plan(rate, row.spf, row.bw, row.mn)
        assert info.chain() == row.chain and info.total_decimation == row.D and info.samples_per_superframe == row.m
        x = GC.wide_stream(row, sum(GC.CALLS))
        a.modem_out_open_rate(row.bw, row.mn, MC.F32, sel, 4)
        s.modem_out_open_rate(row.bw, row.mn, MC.S16, sel, 4)
        b.modem_out_open(MC.F32, sel, 4)
        got, got16, twin, at = [], [], [], 0
        for ns in GC.CALLS:
            seg = x[at * sfw:(at + ns) * sfw]
            at += ns
            want = n.process(seg)[0]
            for rx in (a, s, b):
                assert np.array_equal(rx.process(seg)[0], want), "the ring changed the audio"
            got += MC.drain(a, 1); got16 += MC.drain(s, 1); twin += MC.drain(b, 1)
            for w in range(1, 7):
                assert a.kernel_name(w) == s.kernel_name(w) == n.kernel_name(w), (w, a.kernel_name(w), n.kernel_name(w))
        if row.fs == 48000:
            assert "mixing" in a.kernel_name(2), a.kernel_name(2)
        for k, (call, dropped, rows, present, r_) in enumerate(got):
            assert (call, dropped, r_) == (k, 0, int(info.rate_int))
            assert rows.shape == (len(sel), GC.CALLS[k] * row.m, 2) and rows.dtype == np.float32
            assert present.shape == (len(sel), GC.CALLS[k]) and present.all()
        hold_blocks(oracle_mod, list(enumerate(got)), twin, len(sel), rate, row.bw, row.mn, row.spf, row.D, name)
        signal_holds(oracle_mod, twin, len(sel), rate, row.bw, row.mn, row.spf, name)
        s16_is_the_twin_of(P, got16, got)
        assert all(g[2].any() for g in got16)
        assert a.modem_out_next(False) is None and a.modem_out_dropped() == 0
        a.modem_out_close()
    finally:
        close_all(a, s, b, n)


# ------------------------------------------------------------------------------------------------
# 2. the state paths at the small tiles
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.STATE_ROWS)
def test_a_channel_in_dmnone(gpu_lib, oracle_mod, name):
    """block row 0 sits out the middle call of the first three, block row 1 one whole call of three super-frames: their streams equal the
    oracle's with those pairs cut, after a decimator run through the zeros and one restarted at every call have both missed the bar
    tenfold on the pair that follows; the S16 ring's rows -- the absent pairs' zeros among them, in slots that held samples before -- are
    the host twin of the F32 ring's"""
    import pebblesdr_amd as P
    row = GC.ROWS[name]
    rate, sfw, sel, calls = GC.demod_rate(row), row.spf * GC.front(row), row.sel, (2, 1, 2, 3, 1)
    a, s, b = (GC.bank(P, row) for _ in range(3))
    script = {1: (sel[0], P.DM_NONE), 2: (sel[0], P.DM_USB), 3: (sel[1], P.DM_NONE), 4: (sel[1], P.DM_USB)}

    def before(k):
        if k in script:
            for rx in (a, s, b):
                rx.set_mode(*script[k])
    try:
        x = GC.wide_stream(row, sum(calls))
        a.modem_out_open_rate(row.bw, row.mn, MC.F32, sel, 2)
        s.modem_out_open_rate(row.bw, row.mn, MC.S16, sel, 2)
        b.modem_out_open(MC.F32, sel, 2)
        got, got16, twin, at = [], [], [], 0
        for k, ns in enumerate(calls):
            before(k)
            seg = x[at * sfw:(at + ns) * sfw]
            at += ns
            for rx in (a, s, b):
                rx.process(seg)
            got += MC.drain(a, 1); got16 += MC.drain(s, 1); twin += MC.drain(b, 1)
        assert [int(t[3][0].all()) for t in twin] == [1, 0, 1, 1, 1] and [int(t[3][0].any()) for t in twin] == [1, 0, 1, 1, 1]
        assert [int(t[3][1].any()) for t in twin] == [1, 1, 1, 0, 1] and all(t[3][2:].all() for t in twin)
        for r, where in ((0, {(2, 0)}), (1, {(4, 0)})):
            truth, w1, w2 = RC.wrong_models(oracle_mod, twin, r, rate, row.bw, row.mn, row.spf)
            f1, f2 = RC.miss_factor(truth, w1, where), RC.miss_factor(truth, w2, where)
            print("%s, block row %d: run through the absent pairs %.0f bars, restarted at every call %.0f bars" % (name, r, f1, f2))
            assert f1 >= 10.0 and f2 >= 10.0
        hold_blocks(oracle_mod, list(enumerate(got)), twin, len(sel), rate, row.bw, row.mn, row.spf, row.D, name + ", dmNONE")
        s16_is_the_twin_of(P, got16, got)
        assert not got16[1][2][0].any() and not got16[3][2][1].any() and got16[3][2][0].any()
    finally:
        close_all(a, s, b)


@pytest.mark.parametrize("name", GC.STATE_ROWS)
def test_a_two_slot_ring_drops_two_blocks(gpu_lib, oracle_mod, name):
    """two slots, never released: calls 2 and 3 (two super-frames each) are dropped and counted; what follows is the decimation of the
    delivered pairs only; the bank's audio is a bank's without a ring"""
    import pebblesdr_amd as P
    row = GC.ROWS[name]
    rate, sfw, K = GC.demod_rate(row), row.spf * GC.front(row), 6
    a, b, c = (GC.bank(P, row) for _ in range(3))   # rate ring, 2 slots; plain ring; no ring
    try:
        x = GC.wide_stream(row, 2 * K)
        a.modem_out_open_rate(row.bw, row.mn, MC.F32, row.sel, 2)
        b.modem_out_open(MC.F32, row.sel, 8)
        got = []
        for k in range(K):
            seg = x[2 * k * sfw:2 * (k + 1) * sfw]
            if k == 4:
                first = [a.modem_out_next(True), a.modem_out_next(True)]
                assert [(blk[0], blk[1]) for blk in first] == [(0, 0), (1, 0)] and a.modem_out_next(True) is None and a.modem_out_dropped() == 2
                for blk in first:
                    got.append((blk[0], blk))
                    a.modem_out_release(blk[0])
            audio = a.process(seg)[0]
            b.process(seg)
            assert np.array_equal(audio, c.process(seg)[0]), k
        twin = MC.drain(b, K)
        for blk in MC.drain(a, 2):
            got.append((blk[0], blk))
        assert [(k, blk[1]) for k, blk in got] == [(0, 0), (1, 0), (4, 2), (5, 0)] and a.modem_out_dropped() == 2
        for r in (0, len(row.sel) - 1):   # the wrong model: a decimator that was fed the dropped calls as well
            pairs = lambda ks: [MC.as_complex(twin[k][2])[r][j * row.spf:(j + 1) * row.spf] for k in ks for j in range(2)]
            truth = RC.decimated(oracle_mod, rate, row.bw, row.mn, pairs((0, 1, 4, 5)))
            fed_all = RC.decimated(oracle_mod, rate, row.bw, row.mn, pairs(range(K)))
            assert MC.rel_rms(fed_all[8], truth[4]) >= 10.0 * MC.PAIR_BAR
        hold_blocks(oracle_mod, got, twin, len(row.sel), rate, row.bw, row.mn, row.spf, row.D, name + ", drops")
    finally:
        close_all(a, b, c)


@pytest.mark.parametrize("name", GC.STATE_ROWS)
def test_the_same_stream_cut_into_other_calls(gpu_lib, oracle_mod, name):
    """tests/test_modem_rate_gpu.py's rule: the plain ring's rows are not bit-identical between two cuts of a stream for every channel,
    so a plain twin runs the other cut as well, and every pair whose input -- its own super-frame and the one in front of it, where its
    look-back lies (H <= spf) -- is bit-identical between the cuts must be bit-identical behind the decimator, whether its look-back comes
    from the carry in one cut and from the call's own rows in the other or not"""
    import pebblesdr_amd as P
    row = GC.ROWS[name]
    rate, sfw, sel, m = GC.demod_rate(row), row.spf * GC.front(row), row.sel, row.m
    a, b, c, d = (GC.bank(P, row) for _ in range(4))
    try:
        x = GC.wide_stream(row, sum(GC.CALLS))
        for rx in (a, c):
            rx.modem_out_open_rate(row.bw, row.mn, MC.F32, sel, 4)
        for rx in (b, d):
            rx.modem_out_open(MC.F32, sel, 4)
        blocks = []
        for rxs, cut in (((a, b), GC.CALLS), ((c, d), GC.RECUT)):
            at, out = 0, ([], [])
            for ns in cut:
                for i, rx in enumerate(rxs):
                    rx.process(x[at * sfw:(at + ns) * sfw])
                    out[i].extend(MC.drain(rx, 1))
                at += ns
            blocks.append(out)
        (got, twin), (other, other_twin) = blocks
        hold_blocks(oracle_mod, list(enumerate(other)), other_twin, len(sel), rate, row.bw, row.mn, row.spf, row.D, name + ", other calls")
        one, two = (np.concatenate([g[2] for g in blk], axis=1) for blk in (got, other))
        in_one, in_two = (np.concatenate([g[2] for g in blk], axis=1) for blk in (twin, other_twin))
        assert one.shape == two.shape == (len(sel), sum(GC.CALLS) * m, 2) and in_one.shape == in_two.shape
        n_sf, held, carried = sum(GC.CALLS), 0, 0
        starts = lambda cut: {sum(cut[:i]) for i in range(len(cut))}
        moved = starts(GC.CALLS) ^ starts(GC.RECUT)
        for r in range(len(sel)):
            same = [in_one[r, j * row.spf:(j + 1) * row.spf].tobytes() == in_two[r, j * row.spf:(j + 1) * row.spf].tobytes() for j in range(n_sf)]
            assert same[0]
            for j in range(n_sf):
                if same[j] and (j == 0 or same[j - 1]):
                    assert one[r, j * m:(j + 1) * m].tobytes() == two[r, j * m:(j + 1) * m].tobytes(), "row %d super-frame %d: other call lengths change the rows" % (r, j)
                    held += 1
                    carried += j in moved
        print("%s: %d of %d pairs held bit for bit between the cuts, %d of them with the look-back from the carry in one cut only"
              % (name, held, len(sel) * n_sf, carried))
        assert moved and held >= len(sel) and carried >= 1
    finally:
        close_all(a, b, c, d)


@pytest.mark.parametrize("name", GC.STATE_ROWS)
def test_close_mid_stream_and_reopen_with_another_chain(gpu_lib, oracle_mod, name):
    """calls of 2 and 1 super-frames on the row's chain -- refused opens in between leave the open ring untouched: the second call continues
    the first's stream, and a decimator restarted there misses the bar tenfold -- then close, a refused open, and an open with another chain
    on another selection: the first pair equals a FRESH oracle's, call indices start again, and a decimator of the new chain that had seen
    the stream so far misses the bar tenfold"""
    import pebblesdr_amd as P
    row = GC.ROWS[name]
    rate, sfw = GC.demod_rate(row), row.spf * GC.front(row)
    (bw2, mn2), sel2 = GC.REOPEN[name]
    info2 = P.modem_rate_plan(rate, row.spf, bw2, mn2)
    D2 = int(info2.total_decimation)
    assert info2.chain() != row.chain and info2.n_stages and sel2 != row.sel
    a, b = GC.bank(P, row), GC.bank(P, row)
    try:
        x = GC.wide_stream(row, 7)
        a.modem_out_open_rate(row.bw, row.mn, MC.F32, row.sel, 4)
        b.modem_out_open(MC.F32, None, 8)
        a.process(x[:2 * sfw]); b.process(x[:2 * sfw])
        refused(P, RC.E_INVALID, a.modem_out_open_rate, bw2, mn2, MC.F32, sel2, 4)            # a second open
        refused(P, RC.E_UNSUPPORTED, a.modem_out_open_rate, RC.CIC3[0], RC.CIC3[1])           # a refused plan
        refused(P, RC.E_INVALID, a.modem_out_open, MC.F32, None, 4)
        a.process(x[2 * sfw:3 * sfw]); b.process(x[2 * sfw:3 * sfw])
        got = MC.drain(a, 2)
        a.modem_out_close()
        refused(P, RC.E_UNSUPPORTED, a.modem_out_open_rate, RC.CIC3[0], RC.CIC3[1])
        refused(P, RC.E_INVALID, a.modem_out_next, False)                                     # nothing is open
        a.modem_out_open_rate(bw2, mn2, MC.S16 if name == "d128" else MC.F32, sel2, 4)
        a.modem_out_close()                                                                   # (opened and closed without a call)
        a.modem_out_open_rate(bw2, mn2, MC.F32, sel2, 4)
        a.process(x[3 * sfw:6 * sfw]); b.process(x[3 * sfw:6 * sfw])
        a.process(x[6 * sfw:7 * sfw]); b.process(x[6 * sfw:7 * sfw])
        again = MC.drain(a, 2)
        whole = MC.drain(b, 4)
        view = lambda s: [(c, d, rows[s], present[s], r_) for c, d, rows, present, r_ in whole]
        assert [(g[0], g[1], g[4]) for g in got] == [(0, 0, rate // row.D), (1, 0, rate // row.D)]
        assert [(g[0], g[1], g[4]) for g in again] == [(0, 0, int(info2.rate_int)), (1, 0, int(info2.rate_int))]
        assert again[0][2].shape == (len(sel2), 3 * row.spf // D2, 2) and again[0][3].all()
        for r in range(len(row.sel)):
            truth, _, w2 = RC.wrong_models(oracle_mod, view(row.sel)[:2], r, rate, row.bw, row.mn, row.spf)
            assert RC.miss_factor(truth, w2, {(1, 0)}) >= 10.0
        hold_blocks(oracle_mod, list(enumerate(got)), view(row.sel), len(row.sel), rate, row.bw, row.mn, row.spf, row.D, name + ", before the close")
        for r in range(len(sel2)):
            pairs = [y for _, _, _, y in RC.pairs_of(view(sel2), r, row.spf)]
            fresh = RC.decimated(oracle_mod, rate, bw2, mn2, pairs[3:])
            stale = RC.decimated(oracle_mod, rate, bw2, mn2, pairs)
            assert MC.rel_rms(stale[3], fresh[0]) >= 10.0 * MC.PAIR_BAR
        hold_blocks(oracle_mod, [(2, again[0]), (3, again[1])], view(sel2), len(sel2), rate, bw2, mn2, row.spf, D2, name + ", reopened (%d Hz, %d Hz)" % (bw2, mn2))
        a.modem_out_close()
    finally:
        close_all(a, b)


# ------------------------------------------------------------------------------------------------
# 3. under the bank gate: tail_cases' `gate` script on the d64-four geometry
# ------------------------------------------------------------------------------------------------
def test_under_the_bank_gate_with_several_tiles_per_superframe(gpu_lib, oracle_mod):
    """the carriers, keys, thresholds and calls of tail_cases' row `gate` on frames of 1536 (super-frames of 3072 demodulator samples, two
    tiles each through the four-stage chain): flags equal the plain twin's, with a present-absent-present pattern inside a call, absent pairs
    are zeros, present pairs within the bar of the oracle fed present pairs only -- after both wrong models have missed it tenfold"""
    import pebblesdr_amd as P
    geo, row = GC.ROWS["d64-four"], TC.ROWS["gate"]
    x, sfw = GC.gate_input(), GC.GATE_SFW
    ring, plain = GC.gate_bank(P), GC.gate_bank(P)
    try:
        assert ring.superframe == sfw and sfw == geo.spf * TC.D
        ring.modem_out_open_rate(geo.bw, geo.mn, MC.F32, GC.GATE_SEL, 4)
        plain.modem_out_open(MC.F32, GC.GATE_SEL, 4)
        blocks, twin = [], []
        for s0, ns in TC.call_offsets(row):
            seg = x[s0 * sfw:(s0 + ns) * sfw]
            assert np.array_equal(ring.process(seg)[0], plain.process(seg)[0]), "the rate ring changed the bank's audio"
            blocks += MC.drain(ring, 1); twin += MC.drain(plain, 1)
        for r, ch in enumerate(GC.GATE_SEL):
            flags = [int(v) for b in twin for v in b[3][r]]
            assert flags == list(TC.GATE_KEYS[ch]), (ch, flags)
        assert [int(v) for v in twin[0][3][GC.GATE_SEL.index(0)]] == [1, 0, 1]
        through = restarted = 0.0
        for r in range(len(GC.GATE_SEL)):
            where = RC.reopened(twin, r)
            truth, w1, w2 = RC.wrong_models(oracle_mod, twin, r, TC.RATE, geo.bw, geo.mn, geo.spf)
            through, restarted = max(through, RC.miss_factor(truth, w1, where)), max(restarted, RC.miss_factor(truth, w2, where))
        print("gate on d64-four: run through the absent pairs %.0f bars, restarted at every call %.0f bars" % (through, restarted))
        assert through >= 10.0 and restarted >= 10.0
        hold_blocks(oracle_mod, list(enumerate(blocks)), twin, len(GC.GATE_SEL), TC.RATE, geo.bw, geo.mn, geo.spf, geo.D, "gate on d64-four")
        signal_holds(oracle_mod, twin, len(GC.GATE_SEL), TC.RATE, geo.bw, geo.mn, geo.spf, "gate on d64-four")
    finally:
        close_all(ring, plain)
