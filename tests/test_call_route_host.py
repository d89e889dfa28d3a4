"""CPU tier of a receiver call's route: plan_call_route() of csrc/call_route.h, compiled here with g++, against the table of routes
and the facts that select them ("Routes of a receiver call").  Every row says "with everything else at its
default"; a change to one route that moves another fails here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")

FACTS = ["with_spectrum", "with_chain", "raw", "n", "C", "S", "nf", "zoom_bins", "wfm", "bank_pipe_ok", "profiling", "squelch_set", "bank_gate",
         "gated", "touched", "cond_any", "cond_dirty", "generator", "taps", "recording", "ch0_tune_only", "dec_lds_free_front", "dec_raw_front",
         "dec_double_out", "dec_triple_out", "dec_long_call", "dec_fuse_shape", "osc_transient", "spec_raw_ready", "spec_dec_ready", "pipeline",
         "fuse_dec", "bank_pipe_extev", "bank_pipe_timed_ev"]
ROUTE = ["side", "bank_pipe", "plain", "raw_fused", "staged", "fuse_dec", "rot3", "mid", "done_in_kernel", "timed_handover", "tail", "tune_only"]
NARROW, BANK_GATED, WFM = 0, 1, 2

MAIN = """#include <cstdio>
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
            if (!known) { std::fprintf(stderr, "unknown fact %%s\\n", tok); return 3; }
        }
        const pg::CallRoute r = pg::plan_call_route(f);
        std::printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\\n", r.side, r.bank_pipe, r.plain, r.raw_fused, r.staged, r.fuse_dec, r.rot3, r.mid, r.done_in_kernel,
                    r.timed_handover, r.tail == pg::CallTail::Narrow ? 0 : r.tail == pg::CallTail::BankGated ? 1 : 2, r.tune_only);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("call_route")
    src = d / "route.cpp"
    sets = "\n".join('            if (!std::strcmp(tok, "%s")) { f.%s = (decltype(f.%s))v; known = true; }' % (k, k, k) for k in FACTS)
    src.write_text(MAIN % sets)
    exe = str(d / "route")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])

    def plan(rows):
        """rows: a list of {fact: value}; returns one {route field: value} per row"""
        text = "".join(" ".join("%s=%d" % (k, int(v)) for k, v in row.items()) + "\n" for row in rows)
        out = subprocess.check_output([exe], input=text, text=True).strip().split("\n")
        assert len(out) == len(rows)
        return [dict(zip(ROUTE, (int(v) for v in line.split()))) for line in out]

    def one(**facts):
        return plan([facts])[0]

    one.many = plan
    return one


def without(facts, *names, **changed):
    f = {k: v for k, v in facts.items() if k not in names}
    f.update(changed)
    return f


# one channel, a spectrum, a chain, an LDS-free front, nothing else on
SIDE = dict(with_spectrum=1, with_chain=1, C=1, S=1, n=131072, dec_lds_free_front=1)
# no spectrum, a chain, a handle made for two-stage calls, two output buffers
PIPE = dict(with_spectrum=0, with_chain=1, C=33, S=1, n=32768, bank_pipe_ok=1, dec_double_out=1)
# raw input into a side-by-side call whose first kernels both convert in their loads
RAW = dict(SIDE, raw=1, spec_raw_ready=1, dec_raw_front=1)
# everything the decimator inside the display transform needs
FUSE = dict(SIDE, fuse_dec=1, spec_dec_ready=1, dec_fuse_shape=1, nf=2048)


def test_the_header_is_plain_cpp_and_every_fact_is_settable(planner):
    r = planner()
    assert r == dict(side=0, bank_pipe=0, plain=0, raw_fused=0, staged=0, fuse_dec=0, rot3=0, mid=0, done_in_kernel=0, timed_handover=0, tail=NARROW, tune_only=0)
    assert planner(**{k: 1 for k in FACTS})["tail"] == WFM


def test_side_by_side(planner):
    for pipeline in (0, 1):
        for touched in (0, 1):
            r = planner(**SIDE, pipeline=pipeline, touched=touched)
            assert r["side"] == 1 and r["bank_pipe"] == 0
            assert r["plain"] == int(pipeline and not touched), (pipeline, touched)
    assert planner(**without(SIDE, "with_chain"))["side"] == 0
    assert planner(**without(SIDE, "with_spectrum"))["side"] == 0


@pytest.mark.parametrize("fact", ["profiling", "squelch_set", "bank_gate", "cond_any", "cond_dirty"])
def test_what_switches_side_off(planner, fact):
    assert planner(**SIDE, **{fact: 1})["side"] == 0


def test_a_front_that_needs_lds_switches_side_off(planner):
    assert planner(**without(SIDE, "dec_lds_free_front"))["side"] == 0


def test_two_stage_bank_call(planner):
    for touched in (0, 1):
        for pipeline in (0, 1):  # (PEBBLEGPU_PIPELINE is about side-by-side calls only)
            r = planner(**PIPE, touched=touched, pipeline=pipeline)
            assert r["bank_pipe"] == 1 and r["side"] == 0
            assert r["plain"] == int(not touched)
    assert planner(**without(PIPE, "bank_pipe_ok"))["bank_pipe"] == 0
    assert planner(**without(PIPE, "dec_double_out"))["bank_pipe"] == 0
    assert planner(**without(PIPE, "with_chain"))["bank_pipe"] == 0


@pytest.mark.parametrize("fact", ["taps", "recording", "generator", "zoom_bins", "profiling", "squelch_set", "cond_any", "cond_dirty", "bank_gate", "with_spectrum"])
def test_what_switches_bank_pipe_off(planner, fact):
    r = planner(**without(PIPE, fact, **{fact: 2048 if fact == "zoom_bins" else 1}))
    assert r["bank_pipe"] == 0 and r["plain"] == 0 and r["rot3"] == 0


def test_the_generator_keeps_side_and_is_never_plain(planner):
    base = dict(SIDE, pipeline=1, touched=0)
    r = planner(**base)
    assert r["side"] == 1 and r["plain"] == 1
    r = planner(**base, generator=1)
    assert r["side"] == 1 and r["plain"] == 0 and r["staged"] == 1 and r["raw_fused"] == 0


def test_raw_fusing(planner):
    r = planner(**RAW)
    assert r["side"] == 1 and r["raw_fused"] == 1 and r["staged"] == 0
    missing = [without(RAW, "spec_raw_ready"), without(RAW, "dec_raw_front"), dict(RAW, S=2), dict(RAW, osc_transient=1), dict(RAW, generator=1),
               dict(RAW, profiling=1), without(RAW, "dec_lds_free_front"), without(RAW, "with_spectrum")]  # (the last three: not side)
    for f, r in zip(missing, planner.many(missing)):
        assert r["raw_fused"] == 0 and r["staged"] == 1, f
    # float2 input is never staged unless the generator is on
    r = planner(**without(RAW, "raw"))
    assert r["raw_fused"] == 0 and r["staged"] == 0


def test_three_buffer_rotation(planner):
    for triple in (0, 1):
        for long_call in (0, 1):
            for pipe in (0, 1):
                f = dict(PIPE, dec_triple_out=triple, dec_long_call=long_call, bank_pipe_ok=pipe)
                r = planner(**f)
                assert r["bank_pipe"] == pipe
                assert r["rot3"] == int(pipe and triple and not long_call), f
    assert planner(**SIDE, dec_triple_out=1)["rot3"] == 0


def test_decimator_inside_the_transform(planner):
    r = planner(**FUSE)
    assert r["side"] == 1 and r["fuse_dec"] == 1
    missing = [without(FUSE, "fuse_dec"), dict(FUSE, profiling=1), dict(FUSE, pipeline=1), dict(FUSE, gated=1), dict(FUSE, S=2), dict(FUSE, nf=4096),
               without(FUSE, "spec_dec_ready"), without(FUSE, "dec_fuse_shape"), dict(FUSE, osc_transient=1)]
    for f, r in zip(missing, planner.many(missing)):
        assert r["fuse_dec"] == 0, f
    # the input's format does not take part: a raw call, fused or staged, may have its decimator inside the transform
    assert planner(**FUSE, raw=1)["fuse_dec"] == 1
    r = planner(**FUSE, raw=1, spec_raw_ready=1, dec_raw_front=1)
    assert (r["fuse_dec"], r["raw_fused"], r["staged"]) == (1, 1, 0)


def test_the_mid_record(planner):
    assert planner(with_chain=1)["mid"] == 0
    assert planner(with_chain=1, with_spectrum=1)["mid"] == 1
    assert planner(with_chain=1, profiling=1)["mid"] == 1
    assert planner(**SIDE)["mid"] == 1
    assert planner(**PIPE)["mid"] == 0


def test_the_hand_over_switches_act_on_two_stage_calls_only(planner):
    for base, pipe in ((PIPE, 1), (SIDE, 0)):
        r = planner(**base, bank_pipe_extev=1, bank_pipe_timed_ev=1)
        assert (r["done_in_kernel"], r["timed_handover"]) == (pipe, pipe)
        r = planner(**base)
        assert (r["done_in_kernel"], r["timed_handover"]) == (0, 0)


def test_which_tail(planner):
    assert planner(with_chain=1, wfm=1)["tail"] == WFM
    assert planner(with_chain=1, wfm=1, bank_gate=1)["tail"] == WFM
    assert planner(with_chain=1, bank_gate=1, C=33)["tail"] == BANK_GATED
    assert planner(with_chain=1, C=33)["tail"] == NARROW
    assert planner(**SIDE)["tail"] == NARROW
    assert planner(**PIPE)["tail"] == NARROW
    for C in (1, 2):
        for wfm in (0, 1):
            for none in (0, 1):
                r = planner(with_chain=1, C=C, wfm=wfm, ch0_tune_only=none)
                assert r["tune_only"] == int(C == 1 and not wfm and none), (C, wfm, none)
