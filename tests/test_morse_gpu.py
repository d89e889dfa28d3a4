"""GPU tier (-m gpu): the Morse digital modem on the device (pebblegpu_morse_*, pebblegpu_set_morse) against the restatement in
tests/morse_ref.py, which decimates through the unchanged oracle.Decimator."""
import numpy as np
import pytest

from tests import morse_ref as M
from tests.signals import lcg_noise

pytestmark = pytest.mark.gpu


def keyed(text, wpm, fs, n, freq, amp, start=0):
    """amp * keying envelope * tone at freq, placed at sample `start` of an n-sample stream"""
    env = M.keying(text, wpm, fs)[: max(0, n - start)]
    t = (np.arange(len(env)) + start) / fs
    out = np.zeros(n, dtype=np.complex128)
    out[start:start + len(env)] = amp * env * np.exp(2j * np.pi * freq * t)
    return out


def events_of(ev):
    return [(int(e["sample"]), int(e["token"]), int(e["kind"])) for e in ev]


# ------------------------------------------------------------------------------------------------
# stand-alone step: Morse::setSampleRate + setDemodMode + processBlock
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [2048, 512])
@pytest.mark.parametrize("wpm", [15, 25, 40])
def test_step_against_the_restatement(gpu_lib, oracle_mod, wpm, frame):
    """CWL on enable (tone at -1000 Hz), then CWU from the middle of the stream on (the tone moves to +1000 Hz): events and per-result
    decisions identical, powers within 1e-5 relative on results above -100 dB."""
    import pebblesdr_amd as P
    fs = 64000
    n1 = (int(2.2 * fs) // frame) * frame
    n = n1 + (int(4.6 * fs) // frame) * frame
    x = keyed("TEST", wpm, fs, n, -1000.0, 0.05) + keyed("MORSE", wpm, fs, n, 1000.0, 0.05, start=n1) + lcg_noise(n, 11 + wpm, 2e-3)
    ref = M.MorseRef(fs, frame)
    step = P.Morse(fs, frame, keep_results=True)
    for k in range(n // frame):
        if k * frame == n1:
            ref.set_demod_mode(M.DM_CWU)
            step.setDemodMode(P.DM_CWU)
        fr = x[k * frame:(k + 1) * frame]
        assert step.processBlock(fr) is fr  # processBlock returns `in`
        ref.process(fr)
    p, tone = step.results()
    assert len(p) == len(ref.powers) > 0
    rp = np.array(ref.powers)
    # "identical" means something only if no restated decision sits within the device's rounding of a threshold
    assert min(ref.margins) > 1e-4, min(ref.margins)
    assert tone.tolist() == ref.tones
    m = 10 * np.log10(np.maximum(rp, 1e-300)) > -100
    assert np.max(np.abs(p[m] - rp[m]) / rp[m]) <= 1e-5
    ev = events_of(step.events())
    assert ev == ref.events
    assert [(k, t) for _, t, k in ev][-len(M.text_tokens("MORSE")):] == M.text_tokens("MORSE")
    assert step.status() == ref.status()
    assert len(step.events()) == 0  # drained
    step.close()


def test_step_set_sample_rate_keeps_the_wpm_estimate(gpu_lib, oracle_mod):
    """setSampleRate again mid-stream (every powerOn of the reference): a fresh decoder in dmCWL that starts from the current WPM
    estimate, not from 20; without keep_results the step collects no read-out"""
    import pebblesdr_amd as P
    fs, frame = 64000, 2048
    n1 = (int(3.0 * fs) // frame) * frame
    n = n1 + (int(3.0 * fs) // frame) * frame
    x = keyed("VVV TEST", 40, fs, n, 1000.0, 0.05) + keyed("EST", 40, fs, n, 1000.0, 0.05, start=n1) + lcg_noise(n, 71, 2e-3)
    ref = M.MorseRef(fs, frame)
    step = P.Morse(fs, frame)
    ref.set_demod_mode(M.DM_CWU)
    step.setDemodMode(P.DM_CWU)
    for k in range(n // frame):
        if k * frame == n1:
            assert step.status()["wpm"] == ref.wpm != 20
            ref.set_sample_rate(fs, frame)
            step.setSampleRate(fs, frame)
            assert step.status() == ref.status()  # init(m_wpmSpeedCurrent)
            ref.set_demod_mode(M.DM_CWU)
            step.setDemodMode(P.DM_CWU)
        fr = x[k * frame:(k + 1) * frame]
        step.processBlock(fr)
        ref.process(fr)
    assert events_of(step.events()) == ref.events
    assert step.status() == ref.status()
    assert len(step.results()[0]) == 0
    step.close()


# ------------------------------------------------------------------------------------------------
# receiver banks
# ------------------------------------------------------------------------------------------------
def oracle_pre_agc(oracle_mod, x, fs, fc, lo, hi):
    """Receiver::processIQData up to the modem hook, ANF off: Mixer -> Decimator -> gain restore -> FastFIR (receiver.cpp:910-974)"""
    mx = oracle_mod.Mixer(fs)
    mx.set_frequency(fc)
    d = oracle_mod.Decimator(int(fs), 30000, 0)
    y = d.process(mx.process(x)) * 10.0 ** (2 * d.dec_by2_stages / 20.0)
    ff = oracle_mod.FastFIR()
    ff.setup(lo, hi, 0.0, float(int(d.rate)))
    return ff.process(y), int(d.rate)


def ref_events(oracle_mod, x, fs, fc, mode=M.DM_CWU, cut=None):
    """the restatement fed the oracle chain's pre-AGC signal; cut = (a, b): demodulator samples [a, b) never reach the modem"""
    a, rate = oracle_pre_agc(oracle_mod, x, fs, fc, 300, 3000)
    if cut:
        a = np.concatenate([a[:cut[0]], a[cut[1]:]])
    r = M.MorseRef(rate, 2048)
    r.set_demod_mode(mode)
    for k in range(len(a) // 2048):
        r.process(a[k * 2048:(k + 1) * 2048])
    return r


MSGS = ["TEST", "CQ", "DE", "K1A", "EST", "SOS", "RST", "QTH"]


def config2_input(n, fs, C, keyed_ch):
    fcs = [-960e3 + 7.5e3 * c for c in range(C)]
    x = lcg_noise(n, 21, 2e-4)
    for i, c in enumerate(keyed_ch):
        wpm = 18 + 3 * (i % 8)
        x += keyed(MSGS[i % len(MSGS)], wpm, fs, n, fcs[c] + 1000.0 + 2.0 * (i % 5), 0.002)
    return x, fcs


def bank(P, fs, C, fcs, morse, max_sf, none_ch=(), off_ch=()):
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=max_sf)
    for c in range(C):
        rx.set_mixer(c, fcs[c])
        rx.set_bandpass(c, 300, 3000)
        if morse and c not in off_ch:
            rx.set_morse(c, True)
        rx.set_mode(c, P.DM_NONE if c in none_ch else P.DM_CWU)  # after the enable: the modem follows the mode (CWL -> CWU)
    return rx


def test_config2_bank_against_the_restatement(gpu_lib, oracle_mod):
    """2.048 Msps shared stream, 256 CWU channels with the modem on every one, 32 keyed with distinct messages and speeds, 8 calls of 8
    super-frames.  Events per channel equal the restatement fed the oracle chain's pre-AGC signal; other call lengths give the same
    events; the audio rows are bit-identical to a run with the modem off; channels that are off or in dmNONE emit nothing."""
    import pebblesdr_amd as P
    fs, C = 2048000, 256
    keyed_ch = [8 * i + 3 for i in range(32)]
    none_ch, off_ch = (5,), (6,)
    sf = 32 * 2048
    K = 8
    n = K * 8 * sf
    x, fcs = config2_input(n, fs, C, keyed_ch + [5, 6])
    on = bank(P, fs, C, fcs, True, 8, none_ch, off_ch)
    off = bank(P, fs, C, fcs, False, 8, none_ch)
    assert on.superframe == sf
    got = {c: [] for c in range(C)}
    for k in range(K):
        seg = x[k * 8 * sf:(k + 1) * 8 * sf]
        a_on = on.process(seg)[0]
        a_off = off.process(seg)[0]
        assert np.array_equal(a_on, a_off), k
        if k % 3 == 0:  # reads between some calls only: nothing is lost however many calls run between two reads
            for c in range(C):
                got[c] += events_of(on.morse_events(c))
    for c in range(C):
        got[c] += events_of(on.morse_events(c))
    assert got[5] == [] and got[6] == []
    with pytest.raises(P.PebbleGpuError):
        on.morse_status(6)
    for i, c in enumerate(keyed_ch):
        r = ref_events(oracle_mod, x, fs, fcs[c])
        assert got[c] == r.events, (c, got[c], r.events)
        assert on.morse_status(c) == r.status()
    assert sum(len(got[c]) for c in keyed_ch) > 32
    # the same stream in calls of 1, 2, 5, ... super-frames
    other = bank(P, fs, C, fcs, True, 8, none_ch, off_ch)
    got2 = {c: [] for c in range(C)}
    pos, sizes = 0, [1, 2, 5, 8, 3, 7, 4, 6, 8, 8, 8, 4]
    assert sum(sizes) == K * 8
    for s in sizes:
        other.process(x[pos * sf:(pos + s) * sf])
        pos += s
    for c in range(C):
        got2[c] = events_of(other.morse_events(c))
    assert got2 == got
    for r in (on, off, other):
        r.close()


def test_config3_shard_against_the_restatement(gpu_lib, oracle_mod):
    """100 Msps shared stream, 512 channels, modem on every one; a few keyed channels at 40 WPM against the restatement"""
    import pebblesdr_amd as P
    fs, C = 100e6, 512
    rx = P.ReceiverBank(fs, C, True, False, 0, max_superframes=1)
    sf = rx.superframe
    K = 10
    n = K * sf
    fcs = [-45e6 + 175e3 * c + 1e3 * (c % 7) for c in range(C)]
    kc = [3, 200, 511]
    x = lcg_noise(n, 31, 2e-4)
    for i, c in enumerate(kc):
        x += keyed(["EE", "TE", "ET"][i], 40, fs, n, fcs[c] + 1000.0, 0.003)
    for c in range(C):
        rx.set_mixer(c, fcs[c])
        rx.set_bandpass(c, 300, 3000)
        rx.set_morse(c, True)
        rx.set_mode(c, P.DM_CWU)
    for k in range(K):
        rx.process(x[k * sf:(k + 1) * sf])
    for c in kc:
        r = ref_events(oracle_mod, x, fs, fcs[c])
        assert events_of(rx.morse_events(c)) == r.events, c
        assert rx.morse_status(c) == r.status()
        assert r.status()["modem_rate"] == 6103 and r.status()["samples_per_result"] == 61
        assert len(r.events) > 0
    rx.close()


def test_process_iq_drives_the_modem(gpu_lib, oracle_mod):
    """pebblegpu_process_iq (CB_ProcessIQData frames) runs the modem like pebblegpu_receiver_process does"""
    import pebblesdr_amd as P
    fs = 2048000
    fc = 100e3
    a = P.ReceiverBank(fs, 1, True, False, 0)
    b = P.ReceiverBank(fs, 1, True, False, 0)
    for r in (a, b):
        r.set_mixer(0, fc)
        r.set_bandpass(0, 300, 3000)
        r.set_morse(0, True)
        r.set_mode(0, P.DM_CWU)
    sf = a.superframe
    n = 24 * sf
    x = keyed("EE", 30, fs, n, fc + 1000.0, 0.01) + lcg_noise(n, 41, 2e-4)
    for k in range(n // 2048):
        a.process_iq(x[k * 2048:(k + 1) * 2048])
    for k in range(n // sf):
        b.process(x[k * sf:(k + 1) * sf])
    ea, eb = events_of(a.morse_events(0)), events_of(b.morse_events(0))
    assert ea == eb and len(ea) > 0
    assert ea == ref_events(oracle_mod, x, fs, fc).events
    a.close()
    b.close()


def test_refusals_leave_the_handle_usable(gpu_lib):
    import pebblesdr_amd as P
    fs = 2048000
    w = P.ReceiverBank(20e6, 1, True, True, 0)
    with pytest.raises(P.PebbleGpuError) as e:
        w.set_morse(0, True)  # the WFM branch has no modem hook
    assert e.value.code == -6
    w.close()
    rx = P.ReceiverBank(fs, 4, True, False, 2048, max_superframes=1)
    for c in range(4):
        rx.set_mixer(c, 10e3 * c)
        rx.set_mode(c, P.DM_USB)
    with pytest.raises(P.PebbleGpuError):
        rx.set_morse(4, True)  # channel out of range
    rx.set_morse(1, True)
    with pytest.raises(P.PebbleGpuError) as e:
        rx.set_squelch(2, -60.0)  # a bank's per-channel squelch with the modem on
    assert e.value.code == -6
    x = lcg_noise(rx.superframe, 51, 1e-3)
    rx.process(x)
    rx.set_morse(1, False)
    rx.set_squelch(2, -60.0)
    with pytest.raises(P.PebbleGpuError) as e:
        rx.set_morse(3, True)  # ... the other way round
    assert e.value.code == -6
    rx.process(x)
    rx.close()


def test_dmnone_and_a_second_enable_in_a_bank(gpu_lib, oracle_mod):
    """A channel in dmNONE for two calls leaves its modem untouched (no input, no state change: the restatement never sees those
    samples); pebblegpu_set_morse on a channel whose modem is on gives a fresh decoder from the current WPM estimate"""
    import pebblesdr_amd as P
    fs, C = 2048000, 4
    sf = 32 * 2048
    K, spc = 8, 8
    n = K * spc * sf
    x, fcs = config2_input(n, fs, C, [0, 1, 2, 3])
    rx = bank(P, fs, C, fcs, True, spc)
    nd = spc * sf // 32
    got = {c: [] for c in range(C)}
    for k in range(K):
        if k == 2:
            rx.set_mode(1, P.DM_NONE)
        if k == 4:
            rx.set_mode(1, P.DM_CWU)
        if k == 5:
            got[2] += events_of(rx.morse_events(2))
            rx.set_morse(2, True)  # setDigitalModem -> setSampleRate: dmCWL again, init(m_wpmSpeedCurrent)
            rx.set_mode(2, P.DM_CWU)
        rx.process(x[k * spc * sf:(k + 1) * spc * sf])
    for c in range(C):
        got[c] += events_of(rx.morse_events(c))
    r0 = ref_events(oracle_mod, x, fs, fcs[0])
    assert got[0] == r0.events and len(r0.events) > 0
    r1 = ref_events(oracle_mod, x, fs, fcs[1], cut=(2 * nd, 4 * nd))
    assert got[1] == r1.events and rx.morse_status(1) == r1.status()
    a, rate = oracle_pre_agc(oracle_mod, x, fs, fcs[2], 300, 3000)
    r2 = M.MorseRef(rate, 2048)
    r2.set_demod_mode(M.DM_CWU)
    for j in range(len(a) // 2048):
        if j * 2048 == 5 * nd:
            r2.set_sample_rate(rate, 2048)
            r2.set_demod_mode(M.DM_CWU)
        r2.process(a[j * 2048:(j + 1) * 2048])
    assert got[2] == r2.events and rx.morse_status(2) == r2.status()
    rx.close()


def test_one_channel_squelch_leaves_the_modem_untouched(gpu_lib, oracle_mod):
    """The reference's own shape (one channel, one super-frame per call): calls closed by the squelch return before the hook, so the
    modem never sees their samples and its state does not move"""
    import pebblesdr_amd as P
    fs, fc = 2048000, 100e3
    rx = P.ReceiverBank(fs, 1, True, False, 2048, max_superframes=1)
    rx.set_mixer(0, fc)
    rx.set_bandpass(0, 300, 3000)
    rx.set_morse(0, True)
    rx.set_mode(0, P.DM_CWU)
    sf = rx.superframe
    K = 64
    n = K * sf
    x = keyed("TEST TEST", 25, fs, n, fc + 1000.0, 0.01) + lcg_noise(n, 81, 2e-4)
    for k in range(K):
        if k == 20:
            rx.set_squelch(0, 50.0)  # closes every call: m_avgDb < m_squelchDb
        if k == 30:
            rx.set_squelch(0, -120.0)
        a, _ = rx.process(x[k * sf:(k + 1) * sf])
        assert a.shape[1] == (0 if 20 <= k < 30 else sf // 32), k
    nd = sf // 32
    r = ref_events(oracle_mod, x, fs, fc, cut=(20 * nd, 30 * nd))
    got = events_of(rx.morse_events(0))
    assert got == r.events and len(got) > 0
    assert rx.morse_status(0) == r.status()
    rx.close()
