"""CPU tier: the Morse modem restatement (tests/morse_ref.py) pinned by hand-worked answers.  The plugin's own compiled decoder holds it
too, on clean and on hard keying: tests/test_reference_pins.py (cases morse_hard_*, morse_stream_64000), tests/test_morse_hard_host.py."""
import numpy as np
import pytest

from tests import morse_ref as M
from tests.signals import lcg_noise


@pytest.fixture(scope="module")
def oracle_built(oracle_mod):
    return oracle_mod


@pytest.mark.parametrize("demod_rate,chain,rate", [(64000, [(11, 4), (15, 2)], 8000),   # configs[2]: 2.048 Msps / 32
                                                   (48828, [(11, 4), (15, 2)], 6103)])  # configs[3]: 100 Msps / 2048, int 48828
def test_modem_chain_and_rate(oracle_built, demod_rate, chain, rate):
    d = oracle_built.Decimator(demod_rate, 1000, 8000)
    assert d.chain() == chain
    # 48828 / 8 = 6103.5 is truncated to int (morse.cpp:193)
    assert M.modem_rate(demod_rate) == rate


def test_goertzel_n():
    # (1200000 / 30 = 40000 us / 4) / (quint32)(1e6 / rate)
    assert M.best_n(8000) == 80       # 10000 / 125
    assert M.best_n(6103) == 61       # 10000 / 163 (1e6 / 6103 = 163.85)


def test_init_thresholds_at_20_wpm(oracle_built):
    m = M.MorseRef(64000, 2048)
    # updateThresholds(60000, true): dot 60000, dash 180000, dot-dash threshold (60000 + 180000) / 2 = 120000 (the filter primes)
    assert (m.wpm, m.ddt, m.element, m.char_thr, m.word_thr) == (20, 120000, 15000, 120000, 240000)
    dot = m.ddt // 2
    assert dot == 60000 and int(dot * 0.5) == 30000   # the spike and fade thresholds (set, never compared)
    assert m.shortest == 21818                        # 1200000 / (50 * 1.10)
    assert m.state == M.IDLE and m.sma is None        # init resets the dot-dash filter after priming it


def test_first_result_always_reads_as_a_tone(oracle_built):
    for amp in (0.0, 1e-6, 1.0, 30.0):
        m = M.MorseRef(8000, 80)
        m.process_modem(np.full(80, amp, dtype=np.complex128))
        assert m.tones == [True], amp
        assert m.state == M.MARK_TIMING


def test_cwl_on_enable(oracle_built):
    m = M.MorseRef(64000, 2048)
    assert m.mode == M.DM_CWL
    # -1000 Hz moves up by the modem rate: 7000 / 8000 of a turn per sample
    b, c, d = M.goertzel_coeffs(7000, 80, 8000)
    assert (m.B, m.C, m.D) == (b, c, d)
    # a +1000 Hz tone sits outside the CWL bin: what reaches it is leakage, two orders of magnitude down
    fs = 64000
    env = M.keying("E E", 20, fs)
    t = np.arange(len(env)) / fs
    x = 0.1 * env * np.exp(2j * np.pi * 1000 * t)
    x = np.concatenate([x, np.zeros((-len(x)) % 2048)])
    x = x + lcg_noise(len(x), 5, 1e-4)  # (on digital silence every power is 0 >= a threshold of 0: one endless mark)
    for i in range(0, len(x), 2048):
        m.process(x[i:i + 2048])
    m2 = M.MorseRef(64000, 2048)
    m2.set_demod_mode(M.DM_CWU)
    for i in range(0, len(x), 2048):
        m2.process(x[i:i + 2048])
    assert [(k, tok) for _, tok, k in m2.events] == M.text_tokens("E E")
    assert max(m.powers) < 1e-2 * max(m2.powers)


@pytest.mark.parametrize("wpm,expect_wpm", [(20, 20), (35, 36)])  # 35 WPM: marks are timed in 10 ms results
def test_clean_keyed_tone_decodes(oracle_built, wpm, expect_wpm):
    fs = 64000
    text = "CQ DE K1ABC"
    # the decoder starts from 20 WPM thresholds: at another speed its first marks are mis-timed until the dot-dash pairs have moved
    # them, so a "VVV" goes first and only what follows it is pinned
    env = M.keying("VVV " + text, wpm, fs)
    t = np.arange(len(env)) / fs
    x = 0.05 * env * np.exp(2j * np.pi * 1000 * t)
    x = np.concatenate([x, np.zeros((-len(x)) % 2048)])
    x = x + lcg_noise(len(x), 6, 1e-4)
    m = M.MorseRef(fs, 2048)
    m.set_demod_mode(M.DM_CWU)
    for i in range(0, len(x), 2048):
        m.process(x[i:i + 2048])
    want = M.text_tokens(text)
    got = [(k, tok) for _, tok, k in m.events]
    assert got[-len(want):] == want
    if wpm == 20:
        assert got == M.text_tokens("VVV " + text)
    assert m.status() == {"wpm": expect_wpm, "above_range": 0, "below_range": 0, "modem_rate": 8000, "samples_per_result": 80}
    # events carry the modem-rate sample count, increasing
    s = [e[0] for e in m.events]
    assert s == sorted(s) and s[-1] <= len(x) // 8


def test_token_helpers():
    assert M.dotdash_token(".-") == 0b101
    assert M.dotdash_token("-...") == 0b11000
    import pebblesdr_amd as P
    for dd in ITU_VALUES:
        assert P.morse_token_to_dotdash(M.dotdash_token(dd)) == dd


ITU_VALUES = sorted(set(M.ITU.values()))
