"""CPU tier of the narrow-bank tail table (tests/tail_cases.py); no device.  It holds four things the GPU tier (tests/test_narrow_tail_gpu.py)
relies on: the rows are well formed; every row reaches the channel lists and workgroup counts it is there for; the oracle Receiver is the
chain of its own parts (so each wrong model differs from it in one thing only); and every wrong model -- the deferred AM refresh over a stale
row, state advanced through what a channel sits out, another channel's state blocks, a shifted gate row, a closed super-frame let through --
misses the GPU tier's bar by a factor of 100 or more on the first chunk of 512 outputs it changes, at every row it applies to."""
import numpy as np
import pytest

from tests import tail_cases as TC


def _cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------
# the rows
# ------------------------------------------------------------------------------------------------
def test_rows_are_well_formed(oracle_mod):
    assert len(TC.ROWS) == len({r.name for r in TC.ROWS.values()}) == 7
    for name in ("AM", "SAM", "FMN", "USB", "NONE"):
        assert TC.MODE[name] == getattr(oracle_mod, name)
    r = oracle_mod.Receiver(TC.FS, TC.FRAME, 0)
    assert (r.demod_rate(), r.dec_stages(), oracle_mod.Decimator(TC.FS, 30000).total_decimation) == (TC.RATE, 4, TC.D)
    assert TC.SF == TC.D * TC.SPF
    for row in TC.ROWS.values():
        assert max(row.calls) <= row.max_sf and min(row.calls) >= 1
        fcs = [fc for fc, _, _ in row.carriers]
        assert len(set(fcs)) == len(fcs) and max(abs(f) for f in fcs) + 10e3 < TC.FS / 2
        for fc, _, key in row.carriers:
            assert key is None or len(key) == sum(row.calls)
        for ch in row.chans:
            assert len(ch.modes) == len(row.calls) and ch.fc in fcs
            assert ch.squelch is None or row.bins
        for k, c, kind, args in row.actions:
            assert 0 < k < len(row.calls) and 0 <= c < len(row.chans) and kind in ("bandpass", "squelch")
        assert TC.row_input(row.name).shape == (sum(row.calls) * TC.SF,)
    m = TC.ROWS["modes"]
    assert m.calls == (2, 1, 3, 1, 2, 1) and m.max_sf == 3 and m.bins == 0
    # channel 0 sits out calls of other lengths than its last AM call, and the twin differs from it in the one set_bandpass only
    assert m.chans[0].modes == m.chans[5].modes == ("AM", "USB", "USB", "AM", "AM", "AM")
    assert [m.calls[k] for k in (1, 2)] == [1, 3] and m.calls[0] == 2
    assert m.actions == [(3, 5, "bandpass", (-5000.0, 5000.0))]
    assert TC.ROWS["gate"].calls == TC.ROWS["gate-one"].calls == TC.ROWS["gate-11025"].calls == (3, 1, 2, 2)
    assert TC.ROWS["gate-11025"].audio_rate == 11025 and len(TC.ROWS["gate-one"].chans) == 1 and TC.ROWS["gate-one"].max_sf == 3


def test_lists_row_tunes_neighbours_in_every_list_to_different_carriers():
    """a lane-to-channel or list-to-channel mix-up changes the audio: channel c differs from c +- 1, c +- 3 (its neighbours in its own list)
    and c +- 64 (the same lane of the next workgroup)"""
    row = TC.ROWS["lists"]
    fcs = sorted(fc for fc, _, _ in row.carriers)
    assert len(fcs) == 12 and np.allclose(np.diff(fcs), 80e3)
    kinds = {fc: sig[0] for fc, sig, _ in row.carriers}
    assert sorted(kinds.values()) == ["am"] * 6 + ["fm"] * 6
    assert len({sig for _, sig, _ in row.carriers}) == 12
    C = len(row.chans)
    assert C == TC.LISTS_C == 200
    for c, ch in enumerate(row.chans):
        assert ch.modes[0] == ("FMN", "SAM", "AM")[c % 3] and kinds[ch.fc] == ("fm" if c % 3 == 0 else "am")
        for d in (1, 3, 64):
            for o in (c - d, c + d):
                if 0 <= o < C:
                    assert row.chans[o].fc != ch.fc, (c, o)
    used = {ch.fc for ch in row.chans}
    assert used == set(fcs)


def test_every_row_reaches_the_lists_it_is_there_for():
    m = TC.ROWS["modes"]
    per_call = [TC.mode_lists(m, k) for k in range(len(m.calls))]
    assert [p["AM"] for p in per_call] == [[0, 1, 5], [1], [1, 2], [0, 1, 5], [0, 1, 5], [0, 1, 5]]
    assert [p["SAM"] for p in per_call] == [[2], [2], [], [2], [], [2]]
    assert [p["FMN"] for p in per_call] == [[3], [], [3], [3], [2], [3]]
    assert all(p["ANF"] == [4] and p["AGC"] == [4] for p in per_call)
    ls = TC.ROWS["lists"]
    for k in range(len(ls.calls)):
        p = TC.mode_lists(ls, k)
        assert [len(p[n]) for n in ("FMN", "SAM", "AM", "AGC", "ANF")] == [67, 67, 66, 160, 0]
        for n in ("FMN", "SAM", "AM", "AGC"):
            assert len(p[n]) > 64 and len(p[n]) % 64 != 0
        # k_pll_demod and k_agc: one lane per entry, 64 per workgroup
        assert (_cdiv(len(p["FMN"]), 64), _cdiv(len(p["SAM"]), 64), _cdiv(len(p["AGC"]), 64)) == (2, 2, 3)
        assert all(c in p["AGC"] for c in TC.LISTS_MANUAL) and p["AGC"] == [c for c in range(200) if c % 5]
        assert {ls.chans[c].agc for c in p["AGC"]} == {(TC.AGC_FAST, 20), (TC.AGC_MED, 30), (TC.AGC_SLOW, 30), (TC.AGC_OFF, 30)}
        # the two manual channels sit in different workgroups of k_agc
        assert {p["AGC"].index(c) // 64 for c in TC.LISTS_MANUAL} == {0, 1}
    a = TC.ROWS["anf-list"]
    assert [TC.mode_lists(a, k)["ANF"] for k in range(3)] == [[1, 3, 4], [1, 4], [1, 3, 4]]
    for name in ("gate", "gate-thr", "gate-11025"):
        p = TC.mode_lists(TC.ROWS[name], 0)
        assert (p["AM"], p["SAM"], p["FMN"], p["ANF"], p["AGC"]) == ([0, 1], [2], [3], [1, 4], [0, 1, 4])
        assert {TC.ROWS[name].chans[c].agc for c in p["AGC"]} == {(TC.AGC_SLOW, 30), (TC.AGC_FAST, 20), (TC.AGC_MED, 30)}
    p = TC.mode_lists(TC.ROWS["gate-one"], 0)
    assert (p["AM"], p["AGC"]) == ([0], [0])


def _runs(bits, v):
    out, n = [], 0
    for b in list(bits) + [None]:
        if b == v:
            n += 1
        elif n:
            out.append(n)
            n = 0
    return out


def test_every_keyed_pattern_has_the_runs_and_steps_it_is_there_for():
    bounds = {s0 for s0, _ in TC.call_offsets(TC.ROWS["gate"])}
    assert len({tuple(k) for k in TC.GATE_KEYS}) == 5
    for key in TC.GATE_KEYS:
        closed = _runs(key, 0)
        assert 1 in closed and max(closed) >= 2
        steps = [j for j in range(1, len(key)) if not key[j - 1] and key[j]]   # closed -> open
        assert any(j in bounds for j in steps) and any(j not in bounds for j in steps), key


@pytest.mark.parametrize("name", ["gate", "gate-thr", "gate-one"])
def test_thresholds_sit_midway_with_10_db_to_either_side(oracle_mod, name):
    """the oracle's fdEstimate avgDb of every super-frame's last frame in both keyed states, and what its Receiver then delivers"""
    row = TC.ROWS[name]
    calls = TC.call_offsets(row)
    for c, ch in enumerate(row.chans):
        key = {fc: k for fc, _, k in row.carriers}[ch.fc]
        lv = np.array(TC.gate_levels(oracle_mod, row, c))
        got = [len(a) for call in TC.cached_rows(oracle_mod, name, c) for a in call]
        if ch.squelch is None:
            assert got == [TC.SPF] * len(lv)
            continue
        thr = ch.squelch
        want = [TC.SPF if op else 0 for call in TC.script_opened(row, c) for op in call]
        raised = any(kind == "squelch" and args[0] > 0 for k, cc, kind, args in row.actions if cc == c)
        on = lv if key is None else lv[np.asarray(key) > 0]
        print("%s channel %d (%s): open %.1f .. %.1f dB, threshold %.1f" % (name, c, ch.modes[0], on.min(), on.max(), thr), end="")
        assert on.min() >= thr + 10.0
        if key is not None:
            off = lv[np.asarray(key) == 0]
            print(", closed %.1f .. %.1f dB" % (off.min(), off.max()), end="")
            assert off.max() <= thr - 10.0
            assert abs((on.mean() + off.mean()) / 2 - thr) <= 1.0
        else:
            assert raised and on.max() <= 50.0 - 10.0
        print()
        assert got == want


# ------------------------------------------------------------------------------------------------
# the oracle Receiver is the chain of its own parts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["modes", "lists", "anf-list", "gate", "gate-thr", "gate-one"])
def test_oracle_receiver_is_the_chain_of_its_parts(oracle_mod, name):
    """oracle.Anf, Agc, DemodAM / DemodSAM / DemodNFM fed the USB / AGC-off receiver's output as the band-passed row, asleep through tune-only
    calls, other modes and closed super-frames, give what the Receiver gives, on every channel of every row"""
    row, worst = TC.ROWS[name], 0.0
    for c in range(len(row.chans)):
        full = TC.cached_rows(oracle_mod, name, c)
        got = TC.compose(oracle_mod, row, c, TC.cached_rows(oracle_mod, name, c, "open"), TC.opened_of(full))
        for wc, gc in zip(full, got):
            for w, g in zip(wc, gc):
                assert len(w) == len(g) and len(w) in (0, TC.SPF)
                if len(w):
                    worst = max(worst, TC.rel_rms(g, w))
    print("%s: the composed chain against the Receiver, worst rel-RMS %.3e" % (name, worst))
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------------------
# the wrong models
# ------------------------------------------------------------------------------------------------
def _aw(*parts):
    return ("awake", parts)


_GATED = ("gate_shift",), ("let_through",)
WRONG = [
    # the defect the deferred refresh had: channel 0's AM delay line before its return (call 3) is the end of super-frame 0 of its last AM call
    ("modes", 0, ("stale_am", 3, TC.SPF)),
    # state advanced through a call the channel sat out: another mode, tune-only
    ("modes", 0, _aw("AM")), ("modes", 2, _aw("SAM")), ("modes", 3, _aw("FMN")), ("anf-list", 3, _aw("ANF")),
    # ... a closed gate
    ("gate", 0, _aw("AM")), ("gate", 0, _aw("AGC")), ("gate", 1, _aw("ANF")), ("gate", 1, _aw("AGC")), ("gate", 1, _aw("AM")), ("gate", 2, _aw("SAM")),
    ("gate", 3, _aw("FMN")), ("gate", 4, _aw("ANF")), ("gate", 4, _aw("AGC")),
    ("gate-thr", 0, _aw("AM")), ("gate-thr", 1, _aw("ANF")), ("gate-thr", 2, _aw("SAM")), ("gate-thr", 3, _aw("FMN")), ("gate-thr", 4, _aw("AGC")),
    ("gate-one", 0, _aw("AM")), ("gate-one", 0, _aw("AGC")),
    # two channels' state blocks exchanged for one call (list index used as channel index): neighbours in the FMN, SAM and AM lists
    ("lists", 3, ("foreign", 1, 6)), ("lists", 4, ("foreign", 1, 7)), ("lists", 5, ("foreign", 1, 8)), ("lists", 198, ("foreign", 1, 195)),
    ("modes", 0, ("foreign", 3, 1)), ("gate", 0, ("foreign", 3, 1)), ("anf-list", 3, ("foreign", 2, 4)),
    # channel c >= 64 given the state of c - 64 (the lane's number used as the channel's)
    ("lists", 64, ("foreign", 1, 0)), ("lists", 66, ("foreign", 1, 2)), ("lists", 131, ("foreign", 1, 67)), ("lists", 199, ("foreign", 1, 135)),
] + [(name, c, w) for name in ("gate", "gate-thr") for c in range(5) for w in _GATED if not (name == "gate-thr" and w[0] == "gate_shift")] \
  + [("gate-one", 0, w) for w in _GATED]
# (gate-thr has no shifted-row model: its thresholds change between calls, so all rows of a call agree and the shift changes nothing)


def _wrong_id(w):
    name, c, wrong = w
    return "%s-ch%d-%s" % (name, c, "-".join(str(v) for v in (wrong[:1] + tuple(wrong[1]) if wrong[0] == "awake" else wrong)))


@pytest.mark.parametrize("case", WRONG, ids=_wrong_id)
def test_wrong_models_miss_the_bar_by_a_factor_of_100(oracle_mod, case):
    name, c, wrong = case
    row = TC.ROWS[name]
    full = TC.cached_rows(oracle_mod, name, c)
    if wrong[0] == "foreign":
        o = wrong[2]
        wrong = wrong + (TC.cached_rows(oracle_mod, name, o, "open"), TC.opened_of(TC.cached_rows(oracle_mod, name, o)))
    got = TC.compose(oracle_mod, row, c, TC.cached_rows(oracle_mod, name, c, "open"), TC.opened_of(full), wrong)
    miss = TC.first_miss(row, c, full, got)
    assert miss is not None, "the model changes nothing at this row"
    k, j, b, e, bar = miss
    print("%s channel %d, %s: first changed chunk is call %d super-frame %d outputs %d..%d, rel-RMS %.3e = %.0f bars of %.0e"
          % (name, c, case[2][:3], k, j, b[0], b[1], e, e / bar, bar))
    assert e >= TC.WRONG_FACTOR * bar


# ------------------------------------------------------------------------------------------------
# where the stream starts: the chunks the GPU tier compares are as fine as the reference's own response to the band-pass's fp32 floor allows
# ------------------------------------------------------------------------------------------------
FLOOR_SEEDS = (1, 2, 3)


def _under_floor(oracle_mod, name, c, seed):
    """the oracle's parts fed the channel's band-passed rows plus white noise of FLOOR rms on I and on Q -> (outputs, the oracle's) of the first two super-frames"""
    row = TC.ROWS[name]
    full = TC.cached_rows(oracle_mod, name, c)
    bp = [[a + TC.lcg_noise(len(a), seed, TC.FLOOR * 12 ** 0.5) for a in call] for call in TC.cached_rows(oracle_mod, name, c, "open")]
    got = TC.compose(oracle_mod, row, c, bp, TC.opened_of(full))
    flat = lambda rows: [a for call in rows for a in call][:2]
    return flat(got), flat(full)


@pytest.mark.parametrize("name", ["modes", "lists", "anf-list", "gate", "gate-thr", "gate-one"])
def test_where_the_stream_starts_only_chunks_the_oracle_itself_loses_are_joined(oracle_mod, name):
    """tail_cases.compared_chunks joins chunk 0 of an AM channel, and chunk 1 behind a running AGC, to the chunk behind it in the stream's first
    super-frame, and leaves out an FMN channel's first super-frame.  Every channel of every row that is compared with the oracle chain and
    delivers that super-frame: the oracle's own parts, fed the oracle's band-passed row plus FLOOR (3e-8, absolute) of white noise, LOSE the
    channel's bar on each chunk that is joined, alone, with every seed; HOLD it, with every seed, on every chunk that is compared there, and
    with a factor of 3 to spare on every chunk of the super-frame behind it (an FMN channel's chunk 0 there: see the test below)."""
    row = TC.ROWS[name]
    second = (0, 1) if row.calls[0] > 1 else (1, 0)
    seen = {}
    for c, ch in enumerate(row.chans):
        if TC.via_twin(row, c) or not TC.script_opened(row, c)[0][0]:
            continue
        kept = TC.compared_chunks(row, c, 0, 0)
        if ch.modes[0] == "FMN":
            assert kept == []
            continue
        assert kept[0][0] == 0 and kept[-1][1] == TC.SPF and all(a[1] == b[0] for a, b in zip(kept, kept[1:]))   # nothing is left out
        # a chunk of 1024 is (the chunk the oracle loses alone, the chunk behind it)
        exempt = [(lo, lo + TC.CHUNK) for lo, hi in kept if hi - lo != TC.CHUNK]
        assert all(hi - lo in (TC.CHUNK, 2 * TC.CHUNK) for lo, hi in kept) and len(exempt) <= 1
        bar, sam = TC.chan_bar(row, c)
        kind = (ch.modes[0], "AGC" if TC.agc_running(ch) else "-")
        assert [b[0] // TC.CHUNK for b in exempt] == {("AM", "-"): [0]}.get(kind, [1] if kind[1] == "AGC" else []), kind
        for seed in FLOOR_SEEDS:
            got, want = _under_floor(oracle_mod, name, c, seed)
            alone = TC.chunk_figures(got[0], want[0], sam, exempt)
            held = TC.chunk_figures(got[0], want[0], sam, kept)
            nxt = TC.chunk_figures(got[1], want[1], sam, TC.compared_chunks(row, c, *second)) if TC.script_opened(row, c)[second[0]][second[1]] else []
            assert all(e >= bar for e in alone), (name, c, seed, alone)
            assert all(e <= bar for e in held), (name, c, seed, held)
            assert all(e <= bar / 3 for e in nxt), (name, c, seed, nxt)
            s = seen.setdefault(kind, [bar, [], []])
            s[1] += [e / bar for e in alone]
            s[2] += [e / bar for e in held]
    for kind, (bar, alone, held) in sorted(seen.items()):
        print("%s %s%s (bar %.0e): joined chunk alone %s bars; the chunks compared at most %.3f bars"
              % (name, kind[0], " behind a running AGC" if kind[1] == "AGC" else "", bar,("%.2f .. %.2f" % (min(alone), max(alone))) if alone else "(none)", max(held)))


def test_behind_an_fmn_acquisition_chunk_0_is_held_to_the_oracles_own_transient(oracle_mod):
    """tail_cases.chunk_bar: chunk 0 of the super-frame behind an FMN channel's acquisition is compared at TOL_NFM_WRAP.  Every such channel of
    every row, the oracle's parts under FLOOR: the worst chunk 0 is at most a third of that bar and at least ten times TOL (so TOL cannot be asked
    there); the transient still stands over TOL in the chunk's second half for some (so no cut inside the chunk would do); and chunks 1-3
    hold TOL with a factor of 3 to spare."""
    first, half, rest = [], [], []
    rows = [(name, c) for name in ("modes", "lists", "gate-thr") for c, ch in enumerate(TC.ROWS[name].chans)
            if ch.modes[0] == "FMN" and TC.script_opened(TC.ROWS[name], c)[0][0]]
    assert len(rows) == 1 + 67 + 1
    for name, c in rows:
        row = TC.ROWS[name]
        k, j = (0, 1) if row.calls[0] > 1 else (1, 0)
        assert TC.compared_chunks(row, c, 0, 0) == [] and TC.compared_chunks(row, c, k, j) == TC.FOUR
        bar = TC.chan_bar(row, c)[0]   # TOL, or TOL_AGC_STARTUP behind a running AGC
        assert [TC.chunk_bar(row, c, k, j, lo) for lo, _ in TC.FOUR] == [TC.TOL_NFM_WRAP] + [bar] * 3
        for seed in FLOOR_SEEDS:
            got, want = _under_floor(oracle_mod, name, c, seed)
            f = TC.chunk_figures(got[1], want[1], False, TC.FOUR + [(256, 512)])
            first.append(f[0]); half.append(f[4]); rest.append(max(f[1:4]) / bar)
    print("FMN, second super-frame of the stream under that floor: chunk 0 %.1e .. %.1e, its second half at most %.1e, chunks 1-3 at most %.3f of their bar"
          % (min(first), max(first), max(half), max(rest)))
    assert max(rest) <= 1 / 3
    assert 10 * TC.TOL <= max(first) <= TC.TOL_NFM_WRAP / 3 * 1.2   # three times the worst, rounded: 1.1e-3 -> 3e-3
    assert max(half) >= 2 * TC.TOL
    # and the gate row's FMN channel, closed at the start, acquires at a reopened super-frame inside a call: all four chunks at TOL
    g = TC.ROWS["gate"]
    assert not TC.script_opened(g, 3)[0][0] and all(TC.chunk_bar(g, 3, k, j, 0) == TC.TOL for k, (_, ns) in enumerate(TC.call_offsets(g)) for j in range(ns))


def test_nfm_phase_wrapped_once_per_call_misses_the_bar(oracle_mod):
    """Found by the `modes` row: Demod_NFM wraps its float phase at the end of every processBlock (demod_nfm.cpp:253), one 2048-sample block per
    frame (receiver.cpp:929), and k_pll_demod wrapped once per CALL.  The model -- DemodNFM fed a call's super-frames as one block -- differs only
    where a phase of 2 pi or more meets a block end inside a call: behind the acquisition in the stream's first super-frame, whose run-up the
    second super-frame of the same call then carries unwrapped, at a float resolution of 3e-5 rad.  That is 2 bars on chunks 1-3 of that
    super-frame (the ones held to TOL), not 100: the defect's size IS the float phase's resolution, so no signal makes it larger without
    making the reference's own figure as large.  A regression of the wrap shows in the GPU tier at about 2 bars on those three chunks only."""
    row = TC.ROWS["modes"]
    c = 3
    assert row.chans[c].modes[0] == "FMN" and row.calls[0] == 2 and row.chans[c].agc is None and not row.chans[c].anf
    full = TC.cached_rows(oracle_mod, "modes", c)
    got = oracle_mod.DemodNFM(TC.RATE).process(np.concatenate(TC.cached_rows(oracle_mod, "modes", c, "open")[0]))
    assert np.array_equal(got[:TC.SPF], full[0][0])
    bounds = TC.FOUR[1:]
    assert TC.compared_chunks(row, c, 0, 1) == TC.FOUR and [TC.chunk_bar(row, c, 0, 1, lo) for lo, _ in bounds] == [TC.TOL] * 3
    figs = TC.chunk_figures(got[TC.SPF:], full[0][1], False, bounds)
    print("modes channel 3, one wrap per call: second super-frame, chunks 1-3: %s" % " ".join("%.2e" % e for e in figs))
    assert min(figs) >= 1.5 * TC.TOL
