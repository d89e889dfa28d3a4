"""GPU tier (-m gpu) of the dmFMS coverage statement (tests/rds_cases.py): k_wfm_pilot, k_wfm_lmr_fir, the six kernels of
csrc/kernels_rds.h and RdsCore's queue replay through P.Demod and P.ReceiverBank against the oracle, at every row and call geometry.
No environment switch is set, no kernel is launched directly.

  1. call geometry on input A: every row's script through P.Demod(64000, rate, 8192) in dmFMS against oracle.DemodWFM call by call:
     rdsData() of every call at 1e-6, both audio channels at 1e-5, lengths and lock flags exact, the popped groups and `changed` flags
     bit for bit; the three refused calls fail with the size code and leave the handle bit-identical to a twin that never saw them;
  2. input B (the block synchroniser's error paths) with equal and with mixed calls, groups read every few calls;
  3. input C (the 100-entry queue overrun), groups read every few calls and once at the end;
  4. receivers: dmFMS at 250 000 and 384 000 without a decimator and at 2.5 Msps, calls of 1, 3 and 2 super-frames; a 192 000
     receiver refuses dmFMS and goes on in dmFMM;
  5. a dmFMS bank channel that leaves for dmFMM and returns, beside another station's channel and alone: its RDS groups, and -- leaving
     while its pilot loop is still locked -- its audio, which shows what is left in the (L - R) rows.
"""
import numpy as np
import pytest

from tests import rds_cases as RC
from tests import rds_signal as rs
from tests.signals import lcg_noise

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle_run(oracle_mod, key, rate, x, script):
    if key not in _ORACLE:
        _ORACLE[key] = RC.run_oracle(oracle_mod, rate, x, script)
    return _ORACLE[key]


def tuples(g):
    return [tuple(int(v) for v in r) for r in g]


# ------------------------------------------------------------------------------------------------
# 1. call geometry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", RC.RDS_ROWS, ids=lambda r: r.name)
def test_call_geometry_against_the_oracle(gpu_lib, oracle_mod, row):
    import pebblesdr_amd as P
    x, script = RC.input_a(row), RC.script_a(row)
    ref = oracle_run(oracle_mod, row.name, row.rate, x, script)
    d, twin = P.Demod(64000, row.rate, RC.CAP), P.Demod(64000, row.rate, RC.CAP)
    d.setDemodMode(P.DM_FMS); twin.setDemodMode(P.DM_FMS)
    audio, data, at, k, refused = [], [], 0, 0, 0
    prev_lock = True
    for c in script:
        fr = x[at:at + c.n]
        if not c.ok:
            with pytest.raises(P.PebbleGpuError) as ei:
                d.processBlock(fr)
            assert ei.value.code == RC.E_SIZE, (c.n, ei.value)
            refused += 1
            continue
        g, gd, lock = d.processBlock(fr), d.rdsData(), d.getStereoLock()
        tg, td, tlock = twin.processBlock(fr), twin.rdsData(), twin.getStereoLock()
        assert np.array_equal(g, tg) and np.array_equal(gd, td) and lock == tlock, (k, c.n, refused)
        assert len(g) == c.n and len(gd) == len(ref.data[k]) == c.n // row.D, (k, c.n)
        assert lock == (ref.locks[k], ref.locks[k] != prev_lock), (k, lock)
        prev_lock = ref.locks[k]
        audio.append(g); data.append(gd)
        at += c.n; k += 1
    assert refused == 3 and k == len(ref.data)
    e_rds = RC.call_errors(data, ref.data)
    e_l = RC.call_errors([a.real for a in audio], [a.real for a in ref.audio])
    e_r = RC.call_errors([a.imag for a in audio], [a.imag for a in ref.audio])
    w = int(np.argmax(e_rds))
    print("%s: %d calls; rdsData worst %.3e (call %d, %d samples); audio worst left %.3e right %.3e; %d groups popped"
          % (row.name, k, e_rds[w], w, len(data[w]), max(e_l), max(e_r), len(ref.popped)))
    assert max(e_rds) <= RC.RDS_TOL, (w, e_rds[w])
    assert max(e_l) <= RC.AUDIO_TOL and max(e_r) <= RC.AUDIO_TOL
    got_g, got_c = d.getNextRdsGroupData()
    twin_g, twin_c = twin.getNextRdsGroupData()
    assert len(ref.popped) >= 4                                     # (no row compares an empty list with an empty list)
    assert tuples(got_g) == [g for g, _ in ref.popped] and list(got_c) == [c for _, c in ref.popped]
    assert np.array_equal(got_g, twin_g) and np.array_equal(got_c, twin_c)
    assert d.getNextRdsGroupData()[0].shape == (0, 4)


# ------------------------------------------------------------------------------------------------
# 2. input B, 3. input C
# ------------------------------------------------------------------------------------------------
def _device_groups(P, rate, cap, x, script, read_every):
    d = P.Demod(64000, rate, cap)
    d.setDemodMode(P.DM_FMS)
    got_g, got_c = [], []

    def read():
        g, c = d.getNextRdsGroupData()
        got_g.extend(tuples(g)); got_c.extend(bool(v) for v in c)
    for k, (o, n) in enumerate(RC.offsets(script)):
        d.processBlock(x[o:o + n])
        if read_every and k % read_every == read_every - 1:
            read()
    read()
    return got_g, got_c


@pytest.mark.parametrize("pattern", ["equal", "mixed"])
def test_decoder_error_paths_on_input_b(gpu_lib, oracle_mod, pattern):
    """the Meggitt correction, STATE_GROUPRESYNC, the queue clear with its zero group (event flag 1 and RdsCore::collect's branch for
    it), getNextRdsGroupData's changed = 0: tests/test_rds_geometry_host.py shows that the oracle takes them on this input"""
    import pebblesdr_amd as P
    x, script = RC.input_b(), RC.scripts_b()[pattern]
    ref = oracle_run(oracle_mod, "B-" + pattern, RC.B_RATE, x, script)
    got_g, got_c = _device_groups(P, RC.B_RATE, RC.CAP, x, script, 7)
    want_g, want_c = [g for g, _ in ref.popped], [c for _, c in ref.popped]
    sent = RC.groups_b()
    assert all(tuple(sent[k]) in got_g for k in RC.B_DAMAGED)           # corrected
    assert got_g.count((0, 0, 0, 0)) == 1                               # the queue clear
    assert got_c.count(False) == 2                                      # the group sent three times
    assert got_g == want_g and got_c == want_c                          # ... and every other group, bit for bit


@pytest.mark.parametrize("read_every", [4, 0], ids=["read every 4 calls", "read once at the end"])
def test_group_queue_overrun_on_input_c(gpu_lib, oracle_mod, read_every):
    """about three groups pushed and one popped per call: after 33 calls head runs into tail and the reference loses the 100 groups in
    the ring; RdsCore::collect replays that from the event log, whenever it is asked"""
    import pebblesdr_amd as P
    x = RC.input_c()
    script = RC.equal_script(len(x), RC.C_CALL)
    ref = oracle_run(oracle_mod, "C", RC.C_RATE, x, script)
    got_g, got_c = _device_groups(P, RC.C_RATE, RC.C_CALL, x, script, read_every)
    want_g = [g for g, _ in ref.popped]
    sent = RC.groups_c()
    idx = [sent.index(g) for g in got_g]
    assert max(b - a for a, b in zip(idx, idx[1:])) == RC.Q_SIZE + 1     # the gap is there
    assert got_g == want_g and got_c == [c for _, c in ref.popped]


# ------------------------------------------------------------------------------------------------
# 4. receivers
# ------------------------------------------------------------------------------------------------
CALL_SF = (1, 3, 2)     # super-frames per call, in turn


def call_plan(n, sf):
    """[(offset, length)] of calls of 1, 3 and 2 super-frames in turn over n samples (n a multiple of 6 super-frames)"""
    out, at, k = [], 0, 0
    while at < n:
        m = CALL_SF[k % 3] * sf
        out.append((at, m)); at += m; k += 1
    assert at == n
    return out


@pytest.mark.parametrize("fs,fc,min_groups", [(250000, 10e3, 4), (384000, 20e3, 4), (2500000, 250e3, 4)])
def test_receiver_rds_with_calls_of_changing_length(gpu_lib, oracle_mod, fs, fc, min_groups):
    """dmFMS receivers -- at the input rate (250 000: the three-stage chain; 384 000: the four-stage one, on the levels of that row's
    input, at which the reference decodes) and behind the 2.5 Msps decimator -- against oracle.Receiver fed frame by frame.  A WFM
    receiver without a decimator has one route (k_mixer in front of the demodulator)."""
    import pebblesdr_amd as P
    nf, ng = 2048, 16
    rx = P.ReceiverBank(fs, 1, True, True, 0, max_superframes=3)
    rx.set_mode(0, P.DM_FMS); rx.set_mixer(0, fc)
    sf = rx.superframe
    n = int(fs * (ng * 104 + 60) / 1187.5)
    n -= n % (6 * sf)
    x = rs.fm_multiplex(rs.make_groups(ng, seed=12), float(fs), n, subcarrier_offset_hz=-14.0, **RC.A_LEVELS.get(fs, {})) \
        * np.exp(2j * np.pi * fc * np.arange(n) / fs)
    ref = oracle_mod.Receiver(fs, nf, 0)
    ref.set_mode(oracle_mod.FMS); ref.set_mixer(fc)
    for f in range(n // nf):
        ref.process(x[f * nf:(f + 1) * nf], want_spectrum=False)
    want_g, want_c = ref.rds_polled()
    got_g, got_c = [], []
    for k, (o, m) in enumerate(call_plan(n, sf)):
        rx.process(x[o:o + m])
        if k % 5 == 4:
            g, c = rx.rds_groups(0)
            got_g += tuples(g); got_c += list(c)
    g, c = rx.rds_groups(0)
    got_g += tuples(g); got_c += list(c)
    if fs < 500000:
        assert rx.chain() == [] and rx.kernel_name(2) == "k_mixer"
    print("%d Hz receiver: %d groups" % (fs, len(want_g)))
    assert len(want_g) >= min_groups
    assert got_g == tuples(want_g) and got_c == list(want_c)
    rx.close()


def test_receiver_at_192000_refuses_stereo_and_goes_on_in_mono(gpu_lib, oracle_mod):
    """192 000 runs the sequential WFM path, which has no dmFMS: the mode change is refused and the channel stays what it was"""
    import pebblesdr_amd as P
    fs, fc, nf = 192000, 20e3, 2048
    rx = P.ReceiverBank(fs, 1, True, True, 0, max_superframes=3)
    rx.set_mixer(0, fc)
    ref = oracle_mod.Receiver(fs, nf, 0)
    ref.set_mode(oracle_mod.FMM); ref.set_mixer(fc)
    sf = rx.superframe
    n = 12 * sf
    t = np.arange(n) / fs
    x = 0.5 * np.exp(1j * (2 * np.pi * fc * t + 40.0 * np.sin(2 * np.pi * 1000 * t))) + lcg_noise(n, 2, 1e-3)
    want = [ref.process(x[f * nf:(f + 1) * nf], want_spectrum=False)[0] for f in range(n // nf)]
    got = []
    for k, (o, m) in enumerate(call_plan(n, sf)):
        if k in (0, 2):
            with pytest.raises(P.PebbleGpuError):
                rx.set_mode(0, P.DM_FMS)
        a = rx.process(x[o:o + m])[0][0]
        got += [a[i:i + nf] for i in range(0, len(a), nf)]
    assert len(got) == len(want)
    e = RC.call_errors(got, want)
    print("192000 Hz receiver in dmFMM: worst frame %.3e" % max(e))
    assert max(e) <= RC.AUDIO_TOL
    assert len(rx.rds_groups(0)[0]) == 0
    rx.close()


# ------------------------------------------------------------------------------------------------
# 5. leave and return
# ------------------------------------------------------------------------------------------------
LR_FS, LR_NF = 2500000, 2048
LR_TUNE = (250e3, -600e3)
LR_GROUPS = 22
LR_LEAVE, LR_RETURN = 48, 63           # channel 1 is in dmFMM during the calls [LR_LEAVE, LR_RETURN): 30 super-frames, about two groups
LR_LEAD = 40


def lr_input(sf):
    n = int(LR_FS * (LR_GROUPS * 104 + 60) / 1187.5)
    n -= n % (6 * sf)
    t = np.arange(n) / LR_FS
    ga, gb = rs.make_groups(LR_GROUPS, seed=21), rs.make_groups(LR_GROUPS, seed=22, pi=0x1234)
    x = rs.fm_multiplex(ga, float(LR_FS), n, subcarrier_offset_hz=-14.0, seed=5) * np.exp(2j * np.pi * LR_TUNE[0] * t) \
        + 0.7 * rs.fm_multiplex(gb, float(LR_FS), n, subcarrier_offset_hz=-13.0, seed=6) * np.exp(2j * np.pi * LR_TUNE[1] * t)
    return x, ga, gb


def lr_oracle(oracle_mod, x, plan, tune, switches):
    """oracle.Receiver fed frame by frame with the mode switches at the calls' borders -> the polled (groups, flags) per phase"""
    ref = oracle_mod.Receiver(LR_FS, LR_NF, 0)
    ref.set_mode(oracle_mod.FMS); ref.set_mixer(tune)
    phases = []
    for k, (o, m) in enumerate(plan):
        if switches and k in (LR_LEAVE, LR_RETURN):
            g, c = ref.rds_polled()
            phases.append((tuples(g), list(c)))
            ref.set_mode(oracle_mod.FMM if k == LR_LEAVE else oracle_mod.FMS)
        for f in range(o, o + m, LR_NF):
            ref.process(x[f:f + LR_NF], want_spectrum=False)
    g, c = ref.rds_polled()
    phases.append((tuples(g), list(c)))
    return phases


def lr_device(P, x, plan, tunes, away_channel):
    """a WFM bank of len(tunes) dmFMS channels; `away_channel` is in dmFMM during [LR_LEAVE, LR_RETURN) -> per channel the
    (groups, flags) per phase, and that channel's audio of every call"""
    C = len(tunes)
    rx = P.ReceiverBank(LR_FS, C, True, True, 0, max_superframes=3)
    for c in range(C):
        rx.set_mode(c, P.DM_FMS); rx.set_mixer(c, tunes[c])
    phases, audio = [[] for _ in range(C)], []

    def read():
        for c in range(C):
            g, ch = rx.rds_groups(c)
            phases[c].append((tuples(g), list(ch)))
    for k, (o, m) in enumerate(plan):
        if k in (LR_LEAVE, LR_RETURN):
            read()
            rx.set_mode(away_channel, P.DM_FMM if k == LR_LEAVE else P.DM_FMS)
        audio.append(rx.process(x[o:o + m])[0][away_channel].copy())
    read()
    rx.close()
    return phases, audio


def lr_transient_samples(oracle_mod):
    """how long one wrong sample at the demodulator's input stays in m_RdsData, in input samples: the look-back of the Hilbert pair,
    of every decimate-by-2 stage, of the low-pass and of the matched filter, from the design at the receiver's demodulator rate"""
    dec = oracle_mod.Decimator(LR_FS, 200000).total_decimation
    des = RC.rds_design(LR_FS / dec)
    at_demod = 60 + sum((len(h) - 1) << j for j, h in enumerate(des.stage_h)) + ((len(des.lp) - 1 + len(des.matched) - 1) << len(des.stage_h))
    return at_demod * dec


def test_bank_channel_that_leaves_stereo_and_returns(gpu_lib, oracle_mod):
    """Channel 1 of a two-station bank goes to dmFMM for 15 calls of changing length and comes back; the same channel does the same alone
    in a one-channel bank, where no kernel of the RDS branch runs while it is away.  Its rows must be what it left them: RdsCore::run
    refreshes the head-room of the listed channels only.  The first group compared with the oracle is the first that began after the
    switch transient (test_wfm_stereo_mode_is_the_reference_from_the_first_block: the reference carries the discriminator's last
    sample across the switch, the device reads the input's history) had left the branch's filters, counted in the oracle's list.
    Groups are a coarse observable: a library that refreshed every channel's RDS rows passed this test too (the stale head-room is four
    bits long, inside the stretch in which the block synchroniser resynchronises behind the gap anyway)."""
    import pebblesdr_amd as P
    probe = P.ReceiverBank(LR_FS, 1, True, True, 0, max_superframes=3)
    sf = probe.superframe
    probe.close()
    x, ga, gb = lr_input(sf)
    plan = call_plan(len(x), sf)
    assert len(plan) > LR_RETURN + 40 and len({m for _, m in plan[LR_LEAVE:LR_RETURN]}) == 3
    both, both_audio = lr_device(P, x, plan, LR_TUNE, 1)
    alone, alone_audio = lr_device(P, x, plan, LR_TUNE[1:], 0)
    want1 = lr_oracle(oracle_mod, x, plan, LR_TUNE[1], True)
    want0 = lr_oracle(oracle_mod, x, plan, LR_TUNE[0], False)
    print("leave and return: channel 1 groups per phase: bank %r, alone %r, oracle %r; channel 0: %d"
          % ([len(p[0]) for p in both[1]], [len(p[0]) for p in alone[0]], [len(p[0]) for p in want1], len(want0[0][0])))
    # channel 0 never notices
    got0 = ([g for p in both[0] for g in p[0]], [c for p in both[0] for c in p[1]])
    assert len(want0[0][0]) >= 8 and got0 == want0[0]
    # nothing is popped while away; the two setups agree in every phase, bit for bit
    assert both[1][1] == ([], []) and alone[0][1] == ([], []) and want1[1] == ([], [])
    assert both[1] == alone[0]
    assert all(np.array_equal(a, b) for a, b in zip(both_audio, alone_audio))   # (the audio too; the pilot loop has dropped out long before,
    # so the (L - R) rows are zero here: test_channel_that_leaves_while_its_pilot_is_locked is the case that looks at them)
    # before leaving: the oracle's groups
    assert both[1][0] == want1[0] and len(want1[0][0]) >= 2
    # after the return: from the first group that began behind the transient
    start = plan[LR_RETURN][0] + lr_transient_samples(oracle_mod)
    begins = {tuple(g): (LR_LEAD + 104 * k) / 1187.5 * LR_FS for k, g in enumerate(gb)}
    wg, wc = want1[2]
    first = next(i for i, g in enumerate(wg) if begins.get(g, -1) >= start)
    assert len(wg) - first >= 4, (first, len(wg))
    gg, gc = both[1][2]
    assert gg[first:] == wg[first:] and gc[first:] == wc[first:], (first, gg, wg)


def test_channel_that_leaves_while_its_pilot_is_locked(gpu_lib, oracle_mod):
    """The (L - R) rows.  A channel whose pilot loop is still locked (the first block of this stream is demultiplexed) goes to dmFMM
    for one call and comes back: while it is away the (L - R) part it left with must ring out of the audio response as it does in the
    reference's shared filter -- zeros go into its row -- whether another channel is still in dmFMS (WfmCore::run refreshes every
    row) or none is (it flushes the rows).  The returning channel's audio is bit-identical between the two setups in every call; a
    library without the flush hands the one-channel bank's first 656 returning samples the (L - R) tail of the block it left with."""
    import pebblesdr_amd as P
    from tests.test_parity_gpu import _fm_stereo_mpx
    fs, nf, K = 2500000, 2048, 5

    def run(C, away):
        rx = P.ReceiverBank(fs, C, True, True, 0, max_superframes=1)
        for c in range(C):
            rx.set_mode(c, P.DM_FMS); rx.set_mixer(c, 250e3)
        sf = rx.superframe
        x = _fm_stereo_mpx(fs, K * sf) * np.exp(2j * np.pi * 250e3 * np.arange(K * sf) / fs) + lcg_noise(K * sf, 4, 1e-4)
        out = []
        for k in range(K):
            if k in (1, 2):
                rx.set_mode(away, P.DM_FMM if k == 1 else P.DM_FMS)
            out.append(rx.process(x[k * sf:(k + 1) * sf])[0][away].copy())
        rx.close()
        return out, x, sf
    both, x, sf = run(2, 1)
    alone, _, _ = run(1, 0)
    ref = oracle_mod.Receiver(fs, nf, 0)
    ref.set_mode(oracle_mod.FMS); ref.set_mixer(250e3)
    want = []
    for k in range(K):
        if k in (1, 2):
            ref.set_mode(oracle_mod.FMM if k == 1 else oracle_mod.FMS)
        blocks = [ref.process(x[f:f + nf], want_spectrum=False)[0] for f in range(k * sf, (k + 1) * sf, nf)]
        want.append(np.concatenate([b for b in blocks if len(b)]))
    assert not np.array_equal(want[0].real, want[0].imag)          # the channel leaves locked: its (L - R) rows are not zero
    assert max(RC.call_errors([both[0].real, both[0].imag], [want[0].real, want[0].imag])) <= RC.AUDIO_TOL
    for k in range(K):
        assert np.array_equal(both[k], alone[k]), (k, int(np.argmax(both[k] != alone[k])))
    # against the oracle: every call, the two behind a switch from their 1024th sample on as test_wfm_stereo_mode_is_the_reference_
    # from_the_first_block compares them (the switch transient: the reference's one filter rings on with what the other mode left in
    # it -- here also the (L - R) tail of the locked block, which the device's dmFMM output does not carry -- for the ~700 taps of
    # the audio response)
    lo = [0, 1024, 1024, 0, 0]
    e = RC.call_errors([g[o:] for g, o in zip(both, lo)], [w[o:] for w, o in zip(want, lo)])
    print("leaves locked: against the oracle per call %r" % ["%.1e" % v for v in e])
    assert max(e) <= RC.AUDIO_TOL
