"""CPU tier of the receivers' S-meter: the window table of tests/strength_cases.py through the oracle's SignalStrength::fdEstimate and
through the host twin pebblegpu_signal_strength_row, which ends in the same strength_finish (params.h) as the receivers' k_signal_strength
and the stream bank's k_stream_strength.  tests/test_receiver_smeter_gpu.py runs the same table on the device;
tests/test_reference_pins.py holds the oracle to the reference's own code on the same rows, bit for bit.

Bounds: the twin is the reference's serial loop in double over the same libm and reports float, so the oracle's doubles are narrowed the
same way before the comparison: 1e-9 dB (as tests/test_streambank_smeter_host.py).  A value that the row's class makes a bound (-120, 0)
is exact.  Nothing is NaN or inf.
"""
import numpy as np
import pytest

from tests import strength_cases as S


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    import pebblesdr_amd
    return pebblesdr_amd


def test_every_class_is_present_and_every_row_reaches_its_edge():
    assert {r[6] for r in S.ROWS} == set(S.CLASSES) and len(set(S.NAMES)) == len(S.ROWS)
    for r in S.ROWS:
        w = S.check_class(r)
        assert 0 <= w["nlo"] <= r[2] and 0 <= w["nhi"] <= r[2]
    visited = {S.check_class(r)["visited"] for r in S.ROWS if r[6] in ("centred", "clipped_low_partial")}
    assert {61, 64, 65, 67, 601} <= visited and min(visited) < 61          # under, at and over a wave's stride, and several strides
    assert {r[2] for r in S.ROWS} == {2048, 4096}
    assert {(48000, 2048), (2400000, 4096)} <= {(r[1], r[2]) for r in S.ROWS if r[6] == "truncating"}
    for name in ("mixer_at_half_rate", "mixer_beyond_half_rate"):           # mixer = +fs/2, and beyond it
        r = S.row(name)
        assert (r[5] == r[1] / 2) == (name == "mixer_at_half_rate") and r[5] >= r[1] / 2


def test_the_restated_windows_are_the_device_windows(P):
    """strength_windows (params.h) against the restatement, through the twin: a row that is -110 dB everywhere but -10 dB at one bin gives
    peak -10 dB exactly when that bin is in band, and a floor above -109 dB exactly when it is a noise bin; the bins tried are the ones on
    either side of every edge of the window"""
    for r in S.ROWS:
        name, rate, bins, lo, hi, mixer, _ = r
        w = S.windows(rate, bins, lo, hi, mixer)
        last = min(w["nhi"], bins - 1)
        for i in sorted({0, w["nlo"] - 1, w["nlo"], w["lo"] - 1, w["lo"], w["hi"], w["hi"] + 1, last, last + 1, bins - 1}):
            if not 0 <= i < bins:
                continue
            row = np.full(bins, -110.0, dtype=np.float32)
            row[i] = -10.0
            got = P.signal_strength_row(row, rate, lo, hi, mixer)
            in_band = w["lo"] <= i <= w["hi"] and i >= w["nlo"] and i <= last
            noise = (not in_band) and w["nlo"] <= i <= last
            assert (got[0] == np.float32(-10.0)) == in_band, (name, i, got, w)
            if w["noise"]:
                assert (got[3] > -109.0) == noise, (name, i, got, w)


def test_twin_equals_the_oracle_over_the_table(P, oracle_mod):
    for r in S.ROWS:
        name, rate, bins, lo, hi, mixer, cls = r
        sp = S.row_spectrum(name)
        want = oracle_mod.fd_estimate(sp, rate, np.float32(lo), np.float32(hi), mixer)
        got = P.signal_strength_row(sp.astype(np.float32), rate, lo, hi, mixer)
        print("%-30s oracle %s twin %s" % (name, want, got))
        assert np.isfinite(want).all() and np.isfinite(got).all(), (name, want, got)
        assert np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max() <= 1e-9, (name, got, want)
        for k, v in S.expected(cls).items():
            assert want[k] == v and got[k] == np.float32(v), (name, k, want, got)
        assert -120.0 <= want[[0, 1, 3]].min() and want[[0, 1, 3]].max() <= 0.0 and 0.0 <= want[2] <= 120.0
        if cls not in S.DEGENERATE:                                         # a real measurement: nothing sits on a bound by accident
            assert -120.0 < want[1] < 0.0 and -120.0 < want[3] < 0.0 and -120.0 < want[0] < 0.0, (name, want)


def test_the_oracle_receiver_squelch_closes_on_a_clamped_mixer(oracle_mod):
    """po_receiver's squelch reads po_fd_estimate's avg: with the mixer's bin clamped to `bins` it is -120, under any threshold above
    -120 (m_avgDb < m_squelchDb, receiver.cpp:959-965): no audio.  With bpBins == 0 and a bin in band it is 0 dB: open even at -1."""
    from tests.signals import lcg_noise, tones
    fs, n, F = 2048000, 2048, 48            # (the band-pass hands out its first block after 1024 / 64 = 16 frames)
    x = tones(fs, F * n, [(0.1, 101e3)]) + lcg_noise(F * n, 3, 1e-3)
    for mixer, (lo, hi), threshold, audio in ((1.2e6, S.USB, -60.0, False), (100e3, (100.0, 200.0), -1.0, True), (100e3, S.USB, -119.0, True)):
        ref = oracle_mod.Receiver(fs, n, 2048)
        ref.set_mode(oracle_mod.USB)
        ref.set_mixer(mixer)
        ref.set_filter(lo, hi)
        ref.set_squelch(threshold)
        got = sum(len(ref.process(x[f * n:(f + 1) * n])[0]) for f in range(F))
        assert (got > 0) == audio, (mixer, lo, hi, threshold, got)
