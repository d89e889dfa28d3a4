"""CPU tier of the receiver frame-size table (tests/frame_cases.py); no device.  What the GPU tier (tests/test_receiver_frames_gpu.py) relies on:

  1. every narrow row's super-frame is total * lcm(nf, L), and oracle.Receiver releases per demodulator-rate frame what the row's `why` says;
  2. a plain model of the LIBRARY's partition of a call -- oracle.Mixer -> Decimator -> gain -> FastFIR over the whole call, the demodulator
     once per call with Demod_NFM's wraps placed by k_pll_demod's rule restated (frame_cases.wrap_points) -- is oracle.Receiver fed frame by
     frame, on every never-gated channel of every narrow row, within reference_cases.MAX_BAR (1e-9; it measures 0): the rule IS the
     reference's wherever the block does not divide the frame;
  3. wrong models miss that bar by a factor of ten at least on a row where they place a wrap elsewhere: a wrap every nf samples, at every
     block, at the call's end only; on w-256 a history merge that drops the old part misses the WFM bar by ten; a stereo block as long
     as the call can NOT be told apart on any row, and a test of its own says why instead of passing silently;
  4. the resampler's partition: ResampCore takes off its time sum what each reference frame released, and then delivers the oracle's count
     per call and its samples; in frames of nf it delivers 17641, 35280 outputs where the reference delivers 17640, 35280 (the defect this
     table found: Receiver::init handed ResampCore frames of nf);
  5. the dmFMS frame rule's verdicts, from design::rds_design through rds_cases' design program, at every rate of rds_cases and seven frames;
  6. where a stream starts, frame_cases.stream_chunks joins or leaves out only what the oracle's own parts lose under the band-pass's
     fp32 floor, and every chunk that is compared holds its bar there;
  7. the keyed row's threshold sits midway with 10 dB to either side; the lock flags of the dmFMS rows come from a chain that is the
     Receiver; the CDownConvert model is the oracle wherever the oracle streams exactly."""
import numpy as np
import pytest

from tests import demod_cases as DC
from tests import frame_cases as FC
from tests import rds_cases as RC
from tests import tail_cases as TC
from tests import test_demod_geometry_host as DH
from tests.reference_cases import MAX_BAR

NARROW = [r.name for r in FC.NARROW]
FMN_ROWS = [r.name for r in FC.NARROW if r.chans[0].mode == "FMN"]
WFM = {r.name: r for r in FC.wfm_rows()}


def _stream(calls):
    return np.concatenate(calls)


# ------------------------------------------------------------------------------------------------
# 1. the rows
# ------------------------------------------------------------------------------------------------
def test_rows_are_well_formed(oracle_mod):
    assert len(FC.NARROW_BY_NAME) == len(FC.NARROW) == 7 and len(WFM) == 6
    for name in ("AM", "SAM", "FMN", "FMM", "FMS", "USB", "NONE"):
        assert FC.MODE[name] == getattr(oracle_mod, name)
    want_sf = {"n-512": 16384, "n-1536": 49152, "n-3072": 49152, "n-2048-t257": 229376, "n-4096-f4096": 65536, "n-300-48k": 76800, "n-512-gate": 16384}
    for row in FC.NARROW:
        r = oracle_mod.Receiver(row.fs, row.nf, row.bins, row.fft, row.taps)
        assert (r.demod_rate(), 1 << r.dec_stages()) == (row.rate, row.total), row.name
        assert FC.n_superframe(row) == want_sf[row.name] and FC.n_spf(row) % FC.CHUNK == 0
        assert FC.n_input(row.name).shape == (sum(row.calls) * FC.n_superframe(row),)
        fcs = [ch.fc for ch in row.chans]
        assert len(set(fcs)) == len(fcs) and max(abs(ch.fc + e) for ch in row.chans for e in TC.BAND[ch.mode]) < row.fs / 2
        assert row.release is None or list(row.release) == FC.expected_release(row), row.name
    assert FC.NARROW_BY_NAME["n-512-gate"].calls == TC.GATE_CALLS and len(FC.GATE_KEY) == sum(TC.GATE_CALLS) and FC.GATE_KEY[0] == 0
    rel = FC.expected_release(FC.NARROW_BY_NAME["n-300-48k"])
    assert len(rel) == 256 and sum(rel) == 75 and set(rel) == {0, 1} and rel[:7] == [0, 0, 0, 1, 0, 0, 1]
    assert FC.resampler_parts(FC.NARROW_BY_NAME["n-300-48k"]) == [1024] * 75
    assert FC.resampler_parts(FC.NARROW_BY_NAME["n-1536"]) == [1024, 2048] and FC.resampler_parts(FC.NARROW_BY_NAME["n-2048-t257"]) == [1792] * 6 + [3584]
    for row in WFM.values():
        assert max(row.calls) <= 3 and DC.wfm_design(row.fs // row.total).fused
    d = DC.wfm_design(256000)
    assert d.L4 + d.Llp == FC.WFM_LX_256K
    w = WFM["w-256"]
    assert [k * w.nf < FC.WFM_LX_256K for k in w.calls] == [True, True, False, True, True]       # short, short, long, short after long, short
    assert WFM["w-600"].nf - FC.WFM_LX_256K == 7 and WFM["w-dec-512"].nf < FC.WFM_LX_256K < 2 * WFM["w-dec-512"].nf
    assert -(-WFM["w-65535"].nf // FC.WFM_CHUNK) == 64 and WFM["w-65535"].nf % FC.WFM_CHUNK == FC.WFM_CHUNK - 1


@pytest.mark.parametrize("name", NARROW)
def test_oracle_releases_what_the_row_says(oracle_mod, name):
    """per demodulator-rate frame (`total` input frames) the never-gated channels' Receiver delivers expected_release blocks of L"""
    row = FC.NARROW_BY_NAME[name]
    c = max(i for i, ch in enumerate(row.chans) if ch.key is None)
    lens = FC.n_oracle(oracle_mod, name, c, resample=False)[2]
    per = [sum(lens[i:i + row.total]) for i in range(0, len(lens), row.total)]
    assert all(v == 0 for i, v in enumerate(lens) if i % row.total != row.total - 1)       # only the frame that fills the buffer delivers
    want = [r * FC.n_block(row) for r in FC.expected_release(row)] * sum(row.calls)
    assert per == want, (name, per[:8], want[:8])
    print("%s: %d frames per super-frame release %s blocks of %d" % (name, len(FC.expected_release(row)), sorted(set(FC.expected_release(row))), FC.n_block(row)))


# ------------------------------------------------------------------------------------------------
# 2. the model of the library's partition, 3. the wrong wrap models
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NARROW)
def test_partition_model_is_the_oracle_receiver(oracle_mod, name):
    row, worst = FC.NARROW_BY_NAME[name], 0.0
    for c, ch in enumerate(row.chans):
        if ch.key is not None:
            continue
        want, got = FC.n_oracle(oracle_mod, name, c, resample=False)[0], FC.n_model(oracle_mod, name, c, resample=False)
        assert [len(g) for g in got] == [len(w) for w in want]
        worst = max(worst, max(FC.rel_rms(g, w) for g, w in zip(got, want)))
    print("%s: model of the library's partition against the Receiver fed frame by frame, worst call %.3e" % (name, worst))
    assert worst <= MAX_BAR


def test_wrap_rule_on_the_rows_edges():
    """the rule at the places the rows are there for: every block where the frame is shorter than the block; one wrap per frame and none
    inside a double release; p + blk_len == frame end (L = 1792: 12544 + 1792 = 14336 = 7 * 2048) is NOT a wrap, the double release's end is"""
    w = lambda name, n: FC.wrap_points(FC.NARROW_BY_NAME[name], n)  # noqa: E731
    assert w("n-512", 4096) == [1024, 2048, 3072, 4096]
    assert w("n-1536", 6144) == [1024, 3072, 4096, 6144]
    assert w("n-3072", 6144) == [3072, 6144]
    assert w("n-2048-t257", 14336) == [1792, 3584, 5376, 7168, 8960, 10752, 14336]
    assert w("n-4096-f4096", 8192) == [4096, 8192]
    assert w("n-300-48k", 3072) == [1024, 2048, 3072]
    stock = FC.NARROW_BY_NAME["n-512"]._replace(nf=2048)
    assert FC.wrap_points(stock, 6144) == [2048, 4096, 6144]       # the stock sizes: every frame


@pytest.mark.parametrize("wrong", FC.WRAP_MODELS)
def test_wrong_wrap_models_miss_the_bar_by_ten(oracle_mod, wrong):
    """Each wrong placement on every FMN row: where it places the wraps of every call as the rule does it must change nothing (and the test
    says at which rows that is); where it does not, the stream misses MAX_BAR by a factor of ten at least.  The carriers sit off tune, so
    the float phase passes 2 pi between any two wraps and a wrap moved is an output changed.  Seen by none: no such model."""
    told = {}
    for name in FMN_ROWS:
        row = FC.NARROW_BY_NAME[name]
        same = all(FC.model_wraps(row, n // row.total, wrong) == FC.model_wraps(row, n // row.total) for _, n in FC.n_calls(row))
        want = _stream(FC.n_oracle(oracle_mod, name, 0, resample=False)[0])
        got = _stream(FC.n_model(oracle_mod, name, 0, wrong=wrong, resample=False))
        e = FC.rel_rms(got, want)
        told[name] = e
        if same:
            assert e <= MAX_BAR, (name, e)
        else:
            assert e >= 10 * MAX_BAR, (name, e)
    print("wraps %s: %s" % (wrong, "  ".join("%s %.1e" % (k, v) for k, v in told.items())))
    apart = [k for k, v in told.items() if v >= 10 * MAX_BAR]
    assert len(apart) >= 3, apart
    assert {"every_nf": "n-512", "every_block": "n-1536", "call_end": "n-2048-t257"}[wrong] in apart


# ------------------------------------------------------------------------------------------------
# 3b. the WFM wrong models
# ------------------------------------------------------------------------------------------------
def _mixed(oracle_mod, row, c):
    x, calls = FC.w_input(row.name)
    m = oracle_mod.Mixer(row.fs); m.set_frequency(row.fc)
    return [m.process(x[c, o:o + n]) for o, n in calls]


@pytest.mark.parametrize("name", ["w-256", "w-600"])
def test_wfm_history_merge_that_drops_the_old_part_misses_the_bar(oracle_mod, name):
    """k_wfm_fir in fp64 (test_demod_geometry_host.FoldedWfm) call by call on the row's calls: with the merge it holds the GPU tier's bar
    against the Receiver on every chunk; with a merge that keeps [zeros | the call] (demod_cases' model d) the call behind a short call
    misses it by a factor of ten at least on w-256 (channels 0 and 1: 12 and 13 bars; channel 2, whose 2.4 and 9.1 kHz tones leave less of
    the quiet calls quiet: 6) -- and changes nothing on w-600, whose calls all cover the history"""
    row = WFM[name]
    des = DC.wfm_design(row.fs)
    last = []
    for c in range(len(row.chans)):
        want = FC.w_oracle(oracle_mod, name, c)[0]
        calls = _mixed(oracle_mod, row, c)
        right, wrong = DH.FoldedWfm(des), DH.FoldedWfm(des, "merge")
        e_right = [max(DC.chunk_errors(right.process(x), w, FC.WFM_CHUNK)) for x, w in zip(calls, want)]
        e_wrong = [max(DC.chunk_errors(wrong.process(x), w, FC.WFM_CHUNK)) for x, w in zip(calls, want)]
        print("%s channel %d: one-kernel design against the Receiver, per call %s; merge without the old part %s"
              % (name, c, " ".join("%.1e" % e for e in e_right), " ".join("%.1e" % e for e in e_wrong)))
        assert max(e_right) <= DC.TOL
        if name == "w-256":
            # the last call (512 quiet samples behind the quiet call of 256, the loud call of 768 in front of both): ten bars and more.  The
            # calls in front of it cannot tell: at full level the response 256 samples back is under a thousandth of a bar
            assert row.calls == (1, 2, 3, 1, 2) and FC.W_QUIET[name] == (3, 4)
            assert e_wrong[4] >= 5 * DC.TOL and max(e_wrong[:4]) <= DC.TOL / 1000
            last.append(e_wrong[4])
        else:
            assert e_wrong == e_right
    if name == "w-256":
        assert sorted(last)[-2] >= 10 * DC.TOL, last


def test_stereo_block_as_long_as_the_call_cannot_be_told_apart_on_this_row(oracle_mod):
    """w-1024-fms: oracle.DemodWFM handed every CALL as one processDataStereo block (WfmCore::stereo_block = the call's length) instead of
    frames of 1024, the queue polled once per call, not once per frame.  NO ROW OF THIS TABLE CAN TELL THE TWO APART, and this test says
    so instead of passing silently: the reference's pilot loop ends its first block without lock and never returns (tests/test_oracle_pins.py),
    so no block's (L - R) part depends on where the blocks end; everything else in processDataStereo streams sample by sample; and at one
    group per 87 ms against a poll every 4 ms the queue never holds two groups, so fewer polls deliver the same groups with the same flags.
    The audio is bit for bit the same and the polled lists are equal.  What the block length is good for is held by the step's tests
    (tests/test_rds_geometry_gpu.py, input C: the queue overrun).  Should an input be found on which they differ, this test fails and
    becomes the wrong model's test."""
    row = WFM["w-1024-fms"]
    want, (want_g, want_c) = FC.w_oracle(oracle_mod, row.name, 0)
    x, calls = FC.w_input(row.name)
    m, d = oracle_mod.Mixer(row.fs), oracle_mod.DemodWFM(float(row.fs))
    m.set_frequency(row.fc)
    audio, popped = [], []
    for o, n in calls:
        audio.append(d.process_stereo(m.process(x[0, o:o + n]))[0])
        p = d.next_rds_group()
        if p is not None:
            popped.append(p)
    e = max(RC.call_errors([a.real for a in audio], [w.real for w in want]))
    n_polls_frames, n_polls_calls = sum(n // row.nf for _, n in calls), len(calls)
    # what a reader sees between two reads every 7 calls (the GPU tier's rhythm)
    per_frame = list(zip([tuple(int(v) for v in g) for g in want_g], [bool(v) for v in want_c]))
    per_call = [(tuple(int(v) for v in g), bool(ch)) for g, ch in popped]
    print("stereo block = call: audio worst call %.3e; %d polls instead of %d; %d groups polled against %d" % (e, n_polls_calls, n_polls_frames, len(per_call), len(per_frame)))
    assert n_polls_calls < n_polls_frames
    assert e == 0.0 and per_call == per_frame and len(per_frame) >= 10


# ------------------------------------------------------------------------------------------------
# 4. the resampler's partition
# ------------------------------------------------------------------------------------------------
def test_resampler_partition_follows_what_each_frame_released(oracle_mod):
    name = "n-300-48k"
    row = FC.NARROW_BY_NAME[name]
    assert (row.rate, row.audio_rate) == (48000, 11025) and 147 * 640 == 11025 * 640 // 75 and 48000 * 147 == 11025 * 640
    for c, ch in enumerate(row.chans):
        want = FC.n_oracle(oracle_mod, name, c)[0]
        got = FC.n_model(oracle_mod, name, c)
        assert [len(g) for g in got] == [len(w) for w in want] == [17640, 35280]
        e = max(FC.rel_rms(g, w) for g, w in zip(got, want))
        old = FC.n_model(oracle_mod, name, c, rs_partition="frames")
        print("%s channel %d (%s): released blocks %s outputs, worst call %.3e; frames of 300: %s outputs" % (name, c, ch.mode, [len(g) for g in got], e, [len(g) for g in old]))
        assert e <= FC.TOL / 10
        # the partition the library had: one output early.  (Should a change of the input move this, the counts above are what matters.)
        assert [len(g) for g in old] == [17641, 35280]


# ------------------------------------------------------------------------------------------------
# 5. the dmFMS frame rule
# ------------------------------------------------------------------------------------------------
def test_refusal_verdicts_from_the_design_program():
    rates = [r.rate for r in RC.RDS_ROWS]
    assert rates == [100000, 125000, 256000, 312500, 384000, 512000]
    got = {(rate, nf): FC.fms_verdict(rate, nf) for rate in rates for nf in FC.VERDICT_FRAMES}
    for fs, nf, reason in FC.REFUSALS:
        assert got[(fs, nf)] == reason, (fs, nf, got[(fs, nf)])
    refused = {k: v for k, v in got.items() if v is not None}
    D = {r.rate: r.D for r in RC.RDS_ROWS}
    assert {k for k, v in refused.items() if v == "not a multiple of D"} == {(r, nf) for r in rates for nf in FC.VERDICT_FRAMES if nf % D[r]}
    assert {k for k, v in refused.items() if v == "stage shorter than its taps"} == {(384000, 256), (512000, 256)}
    assert {k for k, v in refused.items() if v == "below 2 (T - 1)"} == {(256000, 256), (384000, 512), (384000, 768), (512000, 512)}
    assert all(got[(r, 2048)] is None and got[(r, 1024)] is None for r in rates)
    # RdsCore::check's rule (what the stand-alone step streams) is the weaker one: rds_min_call accepts what the receiver refuses
    for r in RC.RDS_ROWS:
        assert RC.rds_min_call(RC.rds_design(float(r.rate))) == r.rds_min and FC.fms_verdict(r.rate, r.rds_min) in (None, "below 2 (T - 1)")
    edge = WFM["w-384k-fms"].nf
    assert edge == FC.fms_edge_nf(384000) and edge % 16 == 0 and FC.fms_verdict(384000, edge) is None and FC.fms_verdict(384000, edge - 16) is not None
    des = RC.rds_design(384000.0)
    assert des.stage_taps == (11, 15, 23, 51) and (edge >> 3) == 2 * (51 - 1)
    assert FC.fms_verdict(256000, WFM["w-1024-fms"].nf) is None


# ------------------------------------------------------------------------------------------------
# 6. where a stream starts
# ------------------------------------------------------------------------------------------------
FLOOR_SEEDS = (1, 2, 3)


@pytest.mark.parametrize("name", NARROW)
def test_where_a_stream_starts_only_what_the_oracle_loses_is_joined_or_left_out(oracle_mod, name):
    """the oracle's parts fed the band-passed call plus tail_cases.FLOOR of white noise (n_model's floor_seed), three seeds: every compared
    chunk holds its bar (USB's first, 0.6 of it, is the closest: tail_cases.compared_chunks reads 0.5 .. 0.7 there); every chunk joined to the one behind it loses its bar alone; of an FMN channel's outputs that are left out,
    those of the acquisition (the first 512) lose TOL_NFM_WRAP and some chunk up to the first compared one loses TOL"""
    row = FC.NARROW_BY_NAME[name]
    for c, ch in enumerate(row.chans):
        if ch.key is not None:
            continue
        want = _stream(FC.n_oracle(oracle_mod, name, c)[0])
        size = FC.RS_CHUNK if row.audio_rate else FC.CHUNK
        kept = FC.stream_chunks(row, c, len(want))
        assert kept[-1][1] == len(want) and all(a[1] == b[0] for a, b in zip(kept, kept[1:]))
        worst, alone_min, left = 0.0, None, None
        for seed in FLOOR_SEEDS:
            got = _stream(FC.n_model(oracle_mod, name, c, floor_seed=seed))
            f = lambda lo, hi: FC.rel_rms(FC.form(ch, got[lo:hi]), FC.form(ch, want[lo:hi]))  # noqa: E731
            worst = max(worst, max(f(lo, hi) / bar for lo, hi, bar in kept))
            lo0, hi0, bar0 = kept[0]
            if ch.mode == "FMN":
                assert lo0 > 0 and bar0 == TC.TOL_NFM_WRAP and kept[1][2] == FC.TOL
                out = [f(lo, lo + size) for lo in range(0, lo0, size)]
                assert out[0] >= TC.TOL_NFM_WRAP and max(out) >= FC.TOL
                left = lo0
            else:
                assert lo0 == 0
                joined = [k for k in kept if k[1] - k[0] > size]
                assert len(joined) == (1 if (FC.joined_at_start(row, ch) or (ch.agc is not None and ch.agc[0] != TC.AGC_OFF)) else 0), (name, c)
                for lo, hi, bar in joined:
                    alone = [f(a, a + size) for a in range(lo, hi - size, size) if np.abs(want[a:a + size]).max() > 0]   # (all but the last; zeros of an AGC's delay line are equal)
                    assert alone and all(e >= bar for e in alone), (name, c, seed, alone)
                    alone_min = min(alone + ([alone_min] if alone_min else []))
        print("%s channel %d (%s): compared chunks hold %.2f of their bar under the floor%s%s"
              % (name, c, ch.mode, worst, "" if alone_min is None else "; a joined chunk alone reads %.1e at least" % alone_min,
                 "" if left is None else "; compared from output %d" % left))
        assert worst <= 1.0


def test_fmn_rows_start_behind_the_first_wrap_past_the_acquisition():
    assert {n: FC.fmn_first_compared(FC.NARROW_BY_NAME[n]) for n in FMN_ROWS} == \
        {"n-512": 2048, "n-1536": 3072, "n-3072": 3072, "n-2048-t257": 3584, "n-4096-f4096": 4096, "n-300-48k": 2048}


# ------------------------------------------------------------------------------------------------
# 7. the keyed row, the lock flags' chain, the CDownConvert model
# ------------------------------------------------------------------------------------------------
def test_gate_threshold_sits_midway_with_10_db_to_either_side(oracle_mod):
    row = FC.NARROW_BY_NAME["n-512-gate"]
    ch, sf = row.chans[0], FC.n_superframe(row)
    assert sf // row.nf == 32 and row.bins // row.nf == 4       # 32 raw frames per super-frame, zero-padded four times
    x, sp, lv = FC.n_input(row.name), oracle_mod.Spectrum(row.bins, row.nf), []
    for j in range(sum(row.calls)):
        for i in range(j * sf, (j + 1) * sf, row.nf):
            db = sp.process(x[i:i + row.nf])
        lv.append(float(oracle_mod.fd_estimate(db, row.fs, np.float32(TC.BAND["AM"][0]), np.float32(TC.BAND["AM"][1]), ch.fc)[1]))
    lv, key = np.array(lv), np.asarray(FC.GATE_KEY)
    on, off = lv[key > 0], lv[key == 0]
    print("n-512-gate: open %.1f .. %.1f dB, closed %.1f .. %.1f dB, threshold %.1f" % (on.min(), on.max(), off.min(), off.max(), ch.squelch))
    assert on.min() >= ch.squelch + 10 and off.max() <= ch.squelch - 10 and abs((on.mean() + off.mean()) / 2 - ch.squelch) <= 1.0
    opened = [o for call in FC.n_oracle(oracle_mod, row.name, 0)[1] for o in call]
    assert opened == [bool(k) for k in FC.GATE_KEY]
    assert all(o for call in FC.n_oracle(oracle_mod, row.name, 1)[1] for o in call)


@pytest.mark.parametrize("name", ["w-1024-fms", "w-384k-fms"])
def test_lock_flags_come_from_a_chain_that_is_the_receiver(oracle_mod, name):
    locks, audio = FC.w_locks(oracle_mod, name, with_audio=True)
    want, (groups, changed) = FC.w_oracle(oracle_mod, name, 0)
    assert len(locks) == len(want) and all(np.array_equal(a, w) for a, w in zip(audio, want))
    assert len(groups) >= (10 if name == "w-1024-fms" else 4) and len(groups) == len(changed)
    row = WFM[name]
    assert sorted({n // row.nf for _, n in FC.w_input(name)[1]}) == sorted(set(row.calls))
    print("%s: %d calls, %d groups, %d calls end locked" % (name, len(locks), len(groups), sum(locks)))


def test_downconvert_model_is_the_oracle_where_the_oracle_streams(oracle_mod):
    """one call of the whole input: the model is the oracle (and so the reference, tests/test_reference_pins.py).  In the GPU tier's calls of
    32 .. 96 samples the oracle, like the reference, drops into CHalfBandDecimateBy2's safety net (downconvert.cpp:361-362) and is no
    reference for a step that promises exact history: the model is."""
    fs, bw, f0, taps = FC.DC_STEP
    x = FC.dc_step_input()
    assert tuple(len(h) for h in FC.dc_design(fs, bw)[0]) == taps and len(x) % 32 == 0 and sum(FC.dc_step_calls()) == len(x)
    assert FC.dc_step_calls()[:3] == [32, 64, 96] and FC.dc_step_calls()[3:] == [32] * 41
    want = FC.downconvert_model(fs, bw, f0, x)
    d = oracle_mod.DownConvert()
    assert d.set_data_rate(fs, bw) == fs / 32 and d.chain() == list(taps)
    d.set_frequency(f0)
    e = FC.rel_rms(want, d.process(x))
    print("CDownConvert model against the oracle, one call of %d samples: %.3e" % (len(x), e))
    assert e <= MAX_BAR and np.abs(want).max() > 0.05
    d2 = oracle_mod.DownConvert(); d2.set_data_rate(fs, bw); d2.set_frequency(f0)
    short, at = [], 0
    for n in FC.dc_step_calls():
        short.append(d2.process(x[at:at + n])); at += n
    assert FC.rel_rms(np.concatenate(short), want) > 0.1
