"""CPU tier of the general decimator routes (tests/decim_cases.py): no device.

 - every row's chain is oracle.Decimator's and its route is what decim_cases.route() gives (tests/test_decim_route_host.py holds that
   statement to the planner DecimCore::run reads, csrc/decim_route.h): the rows really sit on
   the kernels, channel-lane layouts and k_cascade instances the coverage statement claims,
 - a sweep of the ladder shows which branches no rate reaches; that list is asserted,
 - the plain fp64 model of mixer -> stages -> gain restore is the oracle at every row (100 times under the GPU bar),
 - nine deliberately wrong models each miss the GPU bar 100 times on every row and call they apply to,
 - the oracle's own output has EVERY channel's peak on the bin the plan predicts.
"""
import numpy as np
import pytest

from tests import decim_cases as dc

ROW_IDS = [r.name for r in dc.ROWS]
_measured = {}


@pytest.fixture(scope="module")
def chains(oracle_mod):
    return {r.name: oracle_mod.Decimator(r.fs, dc.protect_bw(r)).chain() for r in dc.ROWS}


def test_rows_are_well_formed(chains):
    assert len(set(ROW_IDS)) == len(ROW_IDS)
    for r in dc.ROWS:
        assert r.calls == (dc.SCRIPT if r.fs <= 20_000_000 else (1, 1, 1)), r.name
        assert len(chains[r.name]) >= 1, r.name
        p = dc.plan(r, chains[r.name])
        assert len({i % p.NB for i, _ in dc.tone_table(r, p)}) == len(dc.tone_table(r, p)), r.name  # every tone on a bin of its own in every channel
        assert all(f % p.Q for c, f in enumerate(p.fc_idx) if c != p.zero) and (p.zero is None or p.fc_idx[p.zero] == 0), r.name
        assert any(abs(b) * p.df > 15000.0 for b in p.bins) or r.C == 1, r.name
        assert set(p.compare) == set(range(r.C)) or r.fs > 4_000_000, r.name


def test_matrix_instances_are_the_ones_the_statement_was_written_against():
    assert dc.bank_variants() == {(4, 15, 19, 31), (4, 15, 23, 43), (4, 15, 23, 47), (4, 15, 19, 35), (4, 15, 27, 59), (4, 19, 27, 59),
                                  (12, 15, 23, 47), (12, 15, 19, 35), (12, 15, 27, 59)}


def test_every_row_takes_the_route_it_is_there_for(oracle_mod, chains):
    by = {r.name: dc.routes(r, chains[r.name]) for r in dc.ROWS}
    for r in dc.ROWS:
        print("%-26s %-48s %s" % (r.name, chains[r.name], " | ".join("%s%s + %s" % (x.front_inst, "" if x.cl_log2 is None else "@%d" % x.cl_log2, x.cascade_inst or "-") for x in by[r.name])))
        for x in by[r.name]:
            assert x.front != "k_mix_dec_mfma" and x.front != "k_mix_dec_fused", r.name  # the general route on every call
            assert not x.fir_dec, r.name
            assert x.nst == 0 or (x.outb == 256 and x.last_tile == 256), r.name  # (no receiver call has a short last tile)
    front = {n: {(x.front_inst, x.cl_log2) for x in v} for n, v in by.items()}
    name = lambda prefix: [n for n in ROW_IDS if n.startswith(prefix)]
    strides = lambda names: {chains[n][0][1] for n in names}
    # k_mix_dec1
    dec1 = [n for n in ROW_IDS if front[n] == {("k_mix_dec1", None)}]
    assert {n for n in name("dec1-")} == set(dec1)
    assert {(chains[n][0], len(chains[n])) for n in dec1} >= {((27, 2), 1), ((19, 2), 2), ((15, 2), 3), ((11, 2), 4), ((11, 4), 4), ((11, 8), 4), ((11, 16), 4), ((11, 32), 4), ((27, 2), 2)}
    assert {r.C for r in dc.ROWS if r.name in dec1 and not r.wfm and r.shared_input} == {1, 2, 5, 15}
    assert [r.C for r in dc.ROWS if r.name in dec1 and not r.shared_input] == [17]
    assert chains["dec1-17-streams-hb11x4"][0] == (11, 4) and chains["cic-17-streams"][0][0] == 0
    # k_mix_hb11_bank: steady state at every lane layout, the scalar-load instance at every stride; the transient instances on call 0
    steady = {}
    for r in dc.ROWS:
        for k, x in enumerate(by[r.name]):
            if k >= 1 and x.front == "k_mix_hb11_bank":
                steady.setdefault(x.front_inst, set()).add((r.C, chains[r.name][0][1], x.cl_log2))
    assert {c for c, _, _ in steady["k_mix_hb11_bank<false,false>"]} == {16, 17, 32} and {l for _, _, l in steady["k_mix_hb11_bank<false,false>"]} == {4, 5}
    assert {c for c, _, _ in steady["k_mix_hb11_bank<false,true>"]} == {33, 64, 65} and {s for _, s, _ in steady["k_mix_hb11_bank<false,true>"]} == {2, 4, 8, 32}
    assert all(by[n][0].front_inst == "k_mix_hb11_bank<true,%s>" % ("true" if by[n][0].cl_log2 == 6 else "false") for n in name("bank-") + name("lean-"))
    for n in name("lean-"):
        assert [x.front_inst for x in by[n]] == ["k_mix_hb11_bank<true,false>"] + ["k_mix_hb11_lean<-1>"] * 3 and by[n][0].cl_log2 == 0
    assert strides(name("lean-")) == {2, 8, 32}
    # k_mix_cic_hb
    cic = [n for n in ROW_IDS if all(x.front == "k_mix_cic_hb" for x in by[n])]
    assert set(cic) == set(name("cic-"))
    assert {x.cl_log2 for n in cic for x in by[n][1:] if x.front_inst == "k_mix_cic_hb<false,false>"} == {0, 1, 2, 3, 4, 5}
    assert {r.C for r in dc.ROWS if r.name in cic and by[r.name][1].front_inst == "k_mix_cic_hb<false,true>"} == {33, 65}
    assert {x.front_inst for n in cic for x in by[n]} == {"k_mix_cic_hb<%s,%s>" % (a, b) for a in ("true", "false") for b in ("true", "false")}
    assert strides(cic) == {2, 4, 8, 16, 32} and {chains[n][1] for n in cic} == {(11, 16), (11, 32)}
    assert {r.C for r in dc.ROWS if r.name in cic and chains[r.name][1] == (11, 32)} == {1, 33}
    retune = [r for r in dc.ROWS if r.retune_before is not None]
    assert len(retune) == 1 and by[retune[0].name][2].front_inst == "k_mix_cic_hb<true,false>" and by[retune[0].name][3].front_inst == "k_mix_cic_hb<false,false>"
    assert [r.C for r in dc.ROWS if r.name in cic and not r.shared_input] == [17]
    assert any(r.wfm and r.C >= 16 and 90e6 <= r.fs <= 110e6 for r in dc.ROWS if r.name in cic)
    # k_cascade: the three instantiations, the generic one with 1, 2 and 3 stages and behind a bank
    casc = {(x.cascade_inst, x.nst) for v in by.values() for x in v}
    assert casc >= {("k_cascade<15,19,31>", 3), ("k_cascade<15,23,47>", 3), ("k_cascade<0,0,0>", 1), ("k_cascade<0,0,0>", 2), ("k_cascade<0,0,0>", 3), (None, 0)}
    assert all(by[n][1].cascade_inst == "k_cascade<0,0,0>" for n in name("bank-"))
    # the step rows: the cascade's last tile is shorter than outb
    short = 0
    for s in dc.STEP_ROWS:
        ch = oracle_mod.Decimator(s.fs, s.bw).chain()
        for n_out in dc.STEP_OUTPUTS:
            x = dc.step_route(ch, n_out)
            assert x.front in ("k_mix_dec1", "k_mix_cic_hb") and (x.cl_log2 or 0) == 0
            short += x.nst > 0 and x.last_tile < x.outb
    assert short >= 4 * 6


def test_ladder_sweep_leaves_these_branches_dead(oracle_mod):
    """Every rate 60 kHz .. 250 MHz (0.1 % steps and the round rates) at both bandwidths, every bank size class, stream layout, call kind:
    the branches of DecimCore::run and k_mix_dec1 that never come up.  A change to the ladder that makes one live fails here."""
    rates = dc.ladder_rates()
    assert rates[0] == 60000 and rates[-1] >= 249_000_000
    seen_dec1, seen_fir, seen_front, behind_cic, outbs, triples = set(), set(), set(), set(), set(), {4: set(), 12: set()}
    chains = dc.ladder_chains(oracle_mod)  # (both bandwidths at every rate)
    for ch in chains:
        if not ch:
            continue
        if ch[0][0] == 0:
            behind_cic.add(ch[1])
        if len(ch) == 4 and ch[0][0] == 11 and ch[0][1] <= 16:
            triples[4].add(tuple(t for t, _ in ch[1:]))
        if len(ch) == 5 and ch[0][0] == 0 and ch[1] == (11, 16):
            triples[12].add(tuple(t for t, _ in ch[2:]))
        for C in (1, 2, 15, 16, 17, 33, 64, 65):
            for shared in (True, False):
                for lds_free in (False, True):
                    for transient in (False, True):
                        x = dc.route(list(ch), C, shared, lds_free and C == 1, transient, dc.FRAME)
                        seen_front.add(x.front)
                        seen_fir.add(x.fir_dec)
                        if x.front == "k_mix_dec1":
                            seen_dec1.add(x.dec1_branch)
                        if x.outb is not None:
                            outbs.add(x.outb)
    print("chains:", len(chains), "behind a CIC3:", sorted(behind_cic))
    print("triples behind hb11 x S without a matrix instance:", sorted(t for t in triples[4] if (4,) + t not in dc.bank_variants()))
    print("triples behind CIC3 + hb11 x 16 without one:", sorted(t for t in triples[12] if (12,) + t not in dc.bank_variants()))
    assert behind_cic == {(11, 16), (11, 32)}          # so fused_front always holds behind a CIC3 ...
    assert seen_dec1 == {"halfband"}                   # ... and k_mix_dec1's CIC3 paths (merged cg = 8 / 1, S = 2) are dead,
    assert seen_fir == {False}                         # as is the `wide && !fused_front` launch of k_fir_dec
    assert seen_front == {"k_mix_dec1", "k_mix_hb11_bank", "k_mix_hb11_lean", "k_mix_cic_hb", "k_mix_dec_mfma"}  # (k_mix_dec_fused: behind a switch only)
    assert outbs == {256}
    assert {t for t in triples[4] if (4,) + t not in dc.bank_variants()} == {(15, 19, 27), (15, 19, 39), (15, 23, 39), (15, 23, 51), (15, 23, 59)}
    assert {t for t in triples[12] if (12,) + t not in dc.bank_variants()} == {(15, 19, 27), (15, 19, 31), (15, 19, 39), (15, 23, 39), (15, 23, 43), (15, 23, 51), (15, 23, 59)}  # ((19,27,59) comes behind (11,32) only)


def test_inverse_fft_synthesis_is_the_tones_themselves():
    table = [(5, 0.3), (-77, 0.2), (1234, 0.1), (7 * 90 + 3, 0.05)]
    for Q in (3, 7):
        period = Q * 512
        for start, n in ((0, 512), (512, 1024), (3 * 512, 512)):
            assert np.max(np.abs(dc.synth_tones(table, period, Q, start, n) - dc.direct_tones(table, period, start, n))) < 1e-11


def test_oscillator_amplitudes_settle_inside_the_table():
    tab, a_inf = dc.osc_amplitudes()
    assert tab[0] == 1.0 and abs(tab[-1] - a_inf) < 1e-15


def _measure(oracle_mod, chains, name):
    """one row, computed once per session whichever test asks first -> (routes, worst distance of the plain model, channels whose peak
    the oracle does not put on the planned bin, [(wrong model, channel, call, miss in bars)])"""
    if name in _measured:
        return _measured[name]
    row = dc.ROWS[ROW_IDS.index(name)]
    chain = chains[name]
    p = dc.plan(row, chain)
    inputs = [dc.call_input(row, p, k) for k in range(len(row.calls))]
    chans = dc.model_channels(row, p)
    ref, off_peak = {}, []
    for c in range(row.C):  # EVERY channel: the input lights it where the plan says
        o = dc.OracleChannel(oracle_mod, row, p, c, chain)
        y = [o.call(k, x) for k, x in enumerate(inputs)]
        assert [len(v) for v in y] == [k * dc.FRAME for k in row.calls]
        if dc.peak_bin(np.concatenate(y), dc.foreign_bins(row, p, c)) != dc.own_bin(row, p, c):
            off_peak.append(c)
        if c in chans:
            ref[c] = y
    worst, mixed = 0.0, {}
    for c in chans:
        m = dc.Model(row, p, chain, c, mixed=mixed)
        for k, x in enumerate(inputs):
            worst = max(worst, float(dc.frame_errors(m.call(k, x), ref[c][k]).max()))
    misses = []
    for wrong in dc.WRONG:
        cands = [c for c in chans if any(dc.applies(wrong, row, p, chain, c, k) for k in range(len(row.calls)))]
        for c in cands if wrong == "last-group-clamped" else cands[:1]:
            m = dc.Model(row, p, chain, c, wrong, mixed=mixed)
            for k, x in enumerate(inputs):
                e = float(dc.frame_errors(m.call(k, x), ref[c][k]).max())
                if dc.applies(wrong, row, p, chain, c, k):
                    misses.append((wrong, c, k, e / dc.TOL))
    text = " | ".join("%s + %s" % (x.front_inst, x.cascade_inst or "-") for x in dc.routes(row, chain))
    _measured[name] = (text, worst, off_peak, misses)
    return _measured[name]


@pytest.mark.parametrize("name", ROW_IDS)
def test_plain_model_is_the_oracle_and_wrong_models_are_not(oracle_mod, chains, name):
    text, worst, off_peak, misses = _measure(oracle_mod, chains, name)
    print("%s: %s; plain model against the oracle %.2e" % (name, text, worst))
    assert not off_peak, (name, off_peak)
    assert worst <= dc.TOL / dc.MARGIN
    for wrong, c, k, bars in misses:
        assert bars >= dc.MARGIN, (name, wrong, c, k, bars)


def test_summary_of_the_measured_distances(oracle_mod, chains):
    """the figures of the coverage statement, over every row (rows that have not run in this session are computed here)"""
    res = {n: _measure(oracle_mod, chains, n) for n in ROW_IDS}
    n, w = max(((n, r[1]) for n, r in res.items()), key=lambda t: t[1])
    print("plain model against the oracle, worst row: %.2e (%s); bar / %d = %.0e" % (w, n, dc.MARGIN, dc.TOL / dc.MARGIN))
    assert w <= dc.TOL / dc.MARGIN
    for wrong in dc.WRONG:
        hits = [(bars, n, c, k) for n, r in res.items() for wr, c, k, bars in r[3] if wr == wrong]
        assert hits, wrong  # every wrong model applies to some row
        bars, n, c, k = min(hits)
        print("%-22s smallest miss %10.0f bars (%s, channel %d, call %d), %d rows" % (wrong, bars, n, c, k, len({h[1] for h in hits})))
        assert bars >= dc.MARGIN
