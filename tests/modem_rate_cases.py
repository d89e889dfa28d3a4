"""What the two tiers of the modem hook ring at a modem rate (pebblegpu_receiver_modem_out_open_rate, pebblegpu_modem_rate_plan) share: the
table of chains, the look-back formula restated, the reference for a block row and the two deliberately wrong models of its state.

Geometry: tail_cases' own (tests/modem_out_cases.py): 1.024 Msps, D = 16, demodulator rate 64 000, super-frames of 2048 demodulator
samples, at most 6 channels -- but a 5-of-6 and a 70-of-70 selection for the trailer's padding.

The definition (include/pebblegpu.h): the stream of one selected channel is what ONE oracle.Decimator(demodulator rate, max_bw, min_rate)
-- pinned to the reference's class -- produces when it is fed, in order, exactly the (channel, super-frame) pairs the ring delivers as
present.  The input it is fed here are the present pairs of a TWIN bank's plain F32 ring rows: existing code, identical input, bit for bit
the hook's rows.  The oracle is fed one pair -- one whole super-frame -- at a time, whatever its length: its buffers grow with the
frame (po_grow, oracle/pebble_oracle.c), and tests/test_modem_geom_host.py holds a super-frame of 5376 samples in one call to the same
samples in pieces, exactly.  (An earlier version of this text said that a frame over 2048 overruns the oracle's allocation: it does not.)

Other geometries -- ragged and halved tiles, D up to 128, four stages, spans that are mostly look-back, the sample-by-sample store --
are the table of tests/modem_geom_cases.py, which reuses hold_row and the wrong models below on super-frames of other lengths.

Bar per present pair: modem_out_cases.PAIR_BAR, the project's 1e-5 relative RMS; not taken from the code under test.  S16 rows against
the host twin of a twin's F32 rows, the empty chain against the plain ring, and the same stream cut into other calls: exact.

Not reachable with any chain the ladder can build, and therefore tested nowhere: the refusal of more than 16 stages (the ladder has one
CIC3 and eleven halfband designs, and a repeated pick merges into the stage before it)."""
import numpy as np

from tests import modem_out_cases as MC
from tests import tail_cases as TC

E_INVALID, E_SIZE, E_UNSUPPORTED = -1, -5, -6

# (max_bw, min_rate) -> ([(taps, stride)], D) on a 64 kHz bank: read off the oracle, and asserted against it by the host tier
CHAINS = {
    (1000, 8000): ([(11, 4), (15, 2)], 8),
    (3000, 8000): ([(11, 2), (15, 2), (27, 2)], 8),
    (5000, 16000): ([(15, 2), (23, 2)], 4),
    (12000, 8000): ([(27, 2), (59, 2)], 4),      # stops at 16 kHz: out of filters
}
EMPTY = (1000, 64000)                            # min_rate at the demodulator rate: no stage, the plain ring
CIC3 = (100, 8000)                               # [(cic3, 2), (hb11, 4)]: refused
LOOKBACK = {(1000, 8000): 66, (3000, 8000): 142, (5000, 16000): 58, (12000, 8000): 142}
OTHER_RATES = (39062, 48828, 48000)              # demodulator rates of other receivers: (1000, 8000) there


def lookback(chain):
    """H = sum_j (T_j - 1) prod_{i<j} stride_i: how many demodulator samples in front of a segment its outputs depend on"""
    h, scale = 0, 1
    for taps, stride in chain:
        h += (taps - 1) * scale
        scale *= stride
    return h


def decimated(O, rate, bw, mn, pairs):
    """one fresh oracle Decimator fed the given pairs (complex arrays of one super-frame each) in order -> [array per pair]"""
    dec = O.Decimator(rate, bw, mn)
    out = []
    for y in pairs:
        out.append(dec.process(np.asarray(y, dtype=np.complex128)))
    return out


def pairs_of(blocks, r, spf):
    """a drained ring's blocks -> [(call, super-frame, present, complex row of that pair)] of block row r, in stream order"""
    out = []
    for k, (_, _, rows, present, _) in enumerate(blocks):
        z = MC.as_complex(rows)[r] if rows.shape[1] else np.zeros(0, dtype=np.complex64)
        for j in range(present.shape[1]):
            out.append((k, j, bool(present[r][j]), z[j * spf:(j + 1) * spf]))
    return out


def hold_row(O, got, twin, r, rate, bw, mn, spf, D, label=""):
    """block row r of a rate ring's blocks against the oracle fed the present pairs of the twin's plain blocks.  `got` may hold fewer
    blocks than `twin` (dropped ones): got = [(twin's block index, block)].  Flags equal the twin's, absent pairs are all-zero, present
    pairs within PAIR_BAR -> [(rel-RMS, call, super-frame)] of the present pairs"""
    m = spf // D
    fed, where = [], []
    for k, blk in got:
        tp = [p for p in pairs_of([twin[k]], r, spf)]
        gp = [p for p in pairs_of([blk], r, m)]
        assert len(tp) == len(gp), (label, r, k)
        for (_, j, t_present, t_row), (_, _, g_present, g_row) in zip(tp, gp):
            assert g_present == t_present, "%s row %d call %d super-frame %d: flag %d, the plain ring's %d" % (label, r, k, j, g_present, t_present)
            if not t_present:
                assert not g_row.any(), "%s row %d call %d super-frame %d is absent: zeros" % (label, r, k, j)
                continue
            fed.append(t_row)
            where.append((k, j, g_row))
    ref = decimated(O, rate, bw, mn, fed)
    figs = []
    for y, (k, j, g_row) in zip(ref, where):
        assert len(y) == m == len(g_row), (label, len(y), m, len(g_row))
        figs.append((MC.rel_rms(g_row, y), k, j))
    return figs


def wrong_models(O, twin, r, rate, bw, mn, spf):
    """two wrong models of the state, on the oracle alone, for block row r of the twin's plain blocks -> (truth, through, restarted), each
    [(call, super-frame, array)] over the present pairs:
      through    a decimator that ran through the absent pairs as well (it is fed what the plain ring holds there: zeros);
      restarted  a decimator restarted from zero history at every call"""
    pairs = pairs_of(twin, r, spf)
    truth = decimated(O, rate, bw, mn, [y for _, _, p, y in pairs if p])
    through = decimated(O, rate, bw, mn, [y for _, _, _, y in pairs])
    through = [y for y, (_, _, p, _) in zip(through, pairs) if p]
    restarted = []
    for k in range(len(twin)):
        restarted += decimated(O, rate, bw, mn, [y for kk, _, p, y in pairs if p and kk == k])
    keys = [(k, j) for k, j, p, _ in pairs if p]
    return ([(k, j, y) for (k, j), y in zip(keys, truth)], [(k, j, y) for (k, j), y in zip(keys, through)],
            [(k, j, y) for (k, j), y in zip(keys, restarted)])


def reopened(twin, r):
    """the present pairs of block row r that follow an absent pair or start a call, after the row has delivered something -> {(call, sf)}"""
    out, seen, prev = set(), False, True
    for k, (_, _, _, present, _) in enumerate(twin):
        for j in range(present.shape[1]):
            p = bool(present[r][j])
            if p and seen and (not prev or j == 0):
                out.add((k, j))
            seen = seen or p
            prev = p
    return out


def miss_factor(truth, wrong, where):
    """the worst rel-RMS of a wrong model against the truth over the pairs in `where`, in bars"""
    worst = 0.0
    for (k, j, t), (_, _, w) in zip(truth, wrong):
        if (k, j) in where:
            worst = max(worst, MC.rel_rms(w, t) / MC.PAIR_BAR)
    return worst


# ------------------------------------------------------------------------------------------------
# the C++ feeder of modem_out_cases on a ring at a modem rate: the same program, the ring opened at (1000, 8000) and the frame the modem's
# ------------------------------------------------------------------------------------------------
def rate_feeder_cpp():
    src = MC.FEEDER_CPP
    a = "CHECK(pebblegpu_receiver_modem_out_open(rx, format, nullptr, 0, 4));"
    b = "const uint32_t demodFrames = (uint32_t)(cfg.frames_per_buffer / info.total_decimation);"
    assert src.count(a) == 1 and src.count(b) == 1
    src = src.replace(a, "CHECK(pebblegpu_receiver_modem_out_open_rate(rx, format, nullptr, 0, 4, 1000, 8000));")
    return src.replace(b, "const uint32_t demodFrames = (uint32_t)(cfg.frames_per_buffer / info.total_decimation) / 8;   // the modem's frame: D = 8")


ADAPTER_CPP = r"""
// pebblegpu::Receiver::modemOutOpenRate and feedModemBlock at the modem's frame length compile against the header
#include "pebblegpu_steps.hpp"
int main()
{
    pebblegpu::Receiver rx(1024000, 2048, false, 0, nullptr);
    int rc = rx.modemOutOpenRate(PEBBLEGPU_AUDIO_S16, 4, 1000, 8000);
    pebblegpu_modem_block b;
    rx.modemOutNext(false, &b);
    unsigned long long n = pebblegpu::feedModemBlock(b, 16, [](uint32_t, pebblegpu::CPX *, uint32_t) {});
    rx.modemOutClose();
    return rc == 0 && n == 0 ? 0 : 1;
}
"""
