"""CPU tier of the receivers without a decimator: the route facts call_route.h gained for them (compiled here with g++, as
tests/test_call_route_host.py compiles the header) and the chain / super-frame arithmetic of csrc/design.cpp at the rates whose
chain is empty, against oracle.Decimator."""
import math
import os
import subprocess

import pytest

from tests.test_call_route_host import FACTS, FUSE, PIPE, RAW, ROUTE, SIDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")
NEW_FACTS = ["dec_mix_in_consumer", "tap_post_mixer"]

ROUTE_MAIN = """#include <cstdio>
#include <cstring>
#include "call_route.h"
int main()
{
    char line[4096];
    while (std::fgets(line, sizeof(line), stdin)) {
        pg::CallFacts f;
        for (char *tok = std::strtok(line, " \\n"); tok; tok = std::strtok(nullptr, " \\n")) {
            char *eq = std::strchr(tok, '=');
            if (!eq) return 2;
            *eq = 0;
            unsigned long long v = 0;
            if (std::sscanf(eq + 1, "%%llu", &v) != 1) return 2;
            bool known = false;
%s
            if (!known) return 3;
        }
        const pg::CallRoute r = pg::plan_call_route(f);
        std::printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\\n", r.side, r.bank_pipe, r.plain, r.raw_fused, r.staged, r.fuse_dec, r.rot3, r.mid, r.done_in_kernel,
                    r.timed_handover, r.tail == pg::CallTail::Narrow ? 0 : r.tail == pg::CallTail::BankGated ? 1 : 2, r.tune_only, r.mix_in_bandpass);
    }
    return 0;
}
"""

CHAIN_MAIN = """#include <cstdio>
#include "design.h"
int main()
{
    unsigned fs, bw, frame, fft, taps, wfm;
    while (std::scanf("%u %u %u %u %u %u", &fs, &bw, &frame, &fft, &taps, &wfm) == 6) {
        const pg::design::Chain c = pg::design::build_chain(fs, bw, 0);
        std::printf("%zu %u %u %d %llu\\n", c.stages.size(), c.total, c.dec_by2, (int)c.rate,
                    (unsigned long long)pg::design::superframe_len(c, frame, fft, taps, wfm != 0));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("no_decimator_route")
    src = d / "route.cpp"
    sets = "\n".join('            if (!std::strcmp(tok, "%s")) { f.%s = (decltype(f.%s))v; known = true; }' % (k, k, k) for k in FACTS + NEW_FACTS)
    src.write_text(ROUTE_MAIN % sets)
    exe = str(d / "route")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])

    def plan(**facts):
        text = " ".join("%s=%d" % (k, int(v)) for k, v in facts.items()) + "\n"
        out = subprocess.check_output([exe], input=text, text=True).split()
        return dict(zip(ROUTE + ["mix_in_bandpass"], (int(v) for v in out)))

    return plan


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    d = tmp_path_factory.mktemp("no_decimator_chain")
    src = d / "chain.cpp"
    src.write_text(CHAIN_MAIN)
    exe = str(d / "chain")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC, str(src), os.path.join(CSRC, "design.cpp"), "-o", exe])

    def run(rows):
        text = "".join("%d %d %d %d %d %d\n" % r for r in rows)
        out = subprocess.check_output([exe], input=text, text=True).strip().split("\n")
        return [dict(zip(("stages", "total", "dec_by2", "rate", "superframe"), (int(v) for v in line.split()))) for line in out]

    return run


# a 48 kHz bank: a chain, an LDS-free front (k_mixer uses none), the band-pass can mix in its loads
NARROW48 = dict(with_chain=1, C=5, S=1, n=2048, dec_lds_free_front=1, dec_mix_in_consumer=1)


def test_the_mixing_band_pass_is_the_route_of_an_empty_chain(planner):
    r = planner(**NARROW48)
    assert r["mix_in_bandpass"] == 1 and r["bank_pipe"] == 0 and r["fuse_dec"] == 0 and r["raw_fused"] == 0 and r["side"] == 0
    # beside a display transform the chain still goes to its own stream: `side` stays available
    r = planner(**NARROW48, with_spectrum=1)
    assert r["mix_in_bandpass"] == 1 and r["side"] == 1
    # raw input is staged through normalizeIQ (no converting loads on these routes), and then mixed in the band-pass as float2 input is
    r = planner(**NARROW48, with_spectrum=1, raw=1, spec_raw_ready=1)
    assert (r["mix_in_bandpass"], r["raw_fused"], r["staged"]) == (1, 0, 1)
    # the one-value squelch, the generator, conditioners, the recording ring and the other taps leave the mixed rows unread
    for fact in ("squelch_set", "generator", "cond_any", "recording", "taps", "gated", "touched", "ch0_tune_only"):
        assert planner(**NARROW48, **{fact: 1})["mix_in_bandpass"] == 1, fact


@pytest.mark.parametrize("fact,value", [("zoom_bins", 2048), ("tap_post_mixer", 1), ("bank_gate", 1), ("profiling", 1), ("wfm", 1)])
def test_what_needs_the_mixed_rows_takes_the_mixer(planner, fact, value):
    assert planner(**NARROW48, **{fact: value})["mix_in_bandpass"] == 0


def test_without_the_variant_or_the_chain_there_is_nothing_to_mix_into(planner):
    f = dict(NARROW48)
    del f["dec_mix_in_consumer"]
    assert planner(**f)["mix_in_bandpass"] == 0   # a chain with stages, the 4096 / 8192-point band-pass, PEBBLEGPU_NO_FUSED_DEC=1
    f = dict(NARROW48, with_spectrum=1)
    del f["with_chain"]
    assert planner(**f)["mix_in_bandpass"] == 0   # a spectrum-only call


def test_the_new_facts_move_no_existing_route(planner):
    """every row of tests/test_call_route_host.py's bases, with the new facts at their defaults and set: the fields that existed before
    are the same, and without the new facts no call mixes in the band-pass"""
    bases = [dict(), SIDE, PIPE, RAW, FUSE, dict(SIDE, pipeline=1), dict(PIPE, dec_triple_out=1), dict(with_chain=1, wfm=1), dict(with_chain=1, bank_gate=1, C=33),
             dict(with_chain=1, C=1, ch0_tune_only=1), dict(SIDE, generator=1), {k: 1 for k in FACTS}]
    for base in bases:
        old = planner(**base)
        assert old["mix_in_bandpass"] == 0, base
        for extra in (dict(dec_mix_in_consumer=1), dict(tap_post_mixer=1), dict(dec_mix_in_consumer=1, tap_post_mixer=1)):
            new = planner(**base, **extra)
            assert {k: new[k] for k in ROUTE} == {k: old[k] for k in ROUTE}, (base, extra)


EMPTY = [(48000, 30000), (44100, 30000), (192000, 200000), (250000, 200000), (300000, 200000), (384000, 200000), (48000, 200000)]


def test_chains_at_the_rates_without_a_decimator(chains, oracle_mod):
    """no halfband design has fs >= bw / wPass below 75 kHz narrow, below 500 kHz WFM: no stage, D = 1, the demodulator at the input
    rate, as oracle.Decimator builds it; the first rates above those floors get their one stage"""
    rows = [(fs, bw, 2048, 2048, 1025, int(bw == 200000)) for fs, bw in EMPTY]
    for (fs, bw), got in zip(EMPTY, chains(rows)):
        d = oracle_mod.Decimator(fs, bw)
        assert d.total_decimation == 1 and got["stages"] == 0 and got["total"] == 1 and got["dec_by2"] == 0 and got["rate"] == fs, (fs, bw, got)
        assert got["superframe"] == 2048
    for fs, bw in ((96000, 30000), (500000, 200000)):
        got = chains([(fs, bw, 2048, 2048, 1025, int(bw == 200000))])[0]
        assert got["stages"] == 1 and got["total"] == 2 == oracle_mod.Decimator(fs, bw).total_decimation, (fs, bw, got)


@pytest.mark.parametrize("frame,fft,taps", [(2048, 2048, 1025), (2048, 4096, 1025), (2048, 2048, 513), (1024, 2048, 1025), (4096, 8192, 4097), (2048, 2048, 2)])
def test_superframe_of_an_empty_chain(chains, frame, fft, taps):
    """lcm(frame, L) narrow with L = fft - (taps - 1), the frame itself for WFM; the formula of the chains with stages, at D = 1
    (and at 2.048 Msps, D = 32, unchanged)"""
    L = fft - (taps - 1)
    lcm = frame * L // math.gcd(frame, L)
    narrow, wfm, stock = chains([(48000, 30000, frame, fft, taps, 0), (250000, 200000, frame, fft, taps, 1), (2048000, 30000, frame, fft, taps, 0)])
    assert narrow["superframe"] == lcm
    assert wfm["superframe"] == frame
    assert stock["total"] == 32 and stock["superframe"] == 32 * lcm
