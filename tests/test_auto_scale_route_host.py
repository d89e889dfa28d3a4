"""CPU tier: the display ring's recalc as a stage of a receiver call's planned route -- CallRoute::rescale of csrc/call_route.h, compiled
here with g++ as tests/test_call_route_host.py compiles the rest of the table.  The stage is planned for a call that computes the
unprocessed spectrum while a recalc is requested, moves no other field of the route, and no other call gets it."""
import itertools
import subprocess

import pytest

from tests.test_call_route_host import CSRC, FACTS, SIDE, PIPE

MAIN = """#include <cstdio>
#include "call_route.h"
int main()
{
    for (int m = 0; m < 8; m++) {
        pg::CallFacts f;
        f.with_chain = true;
        f.scale_pending = m & 1;
        f.with_spectrum = m & 2;
        f.gated = m & 4;
        std::printf("%d %d %d %d\\n", (int)f.scale_pending, (int)f.with_spectrum, (int)f.gated, (int)pg::plan_call_route(f).rescale);
    }
    // the request moves nothing else: the side-by-side and the two-stage call with and without it
    for (int shape = 0; shape < 2; shape++) {
        pg::CallFacts f;
        f.with_chain = true;
        if (shape == 0) { f.with_spectrum = true; f.dec_lds_free_front = true; f.pipeline = true; }
        else { f.C = 33; f.bank_pipe_ok = true; f.dec_double_out = true; }
        pg::CallRoute r[2];
        for (int p = 0; p < 2; p++) { f.scale_pending = p; r[p] = pg::plan_call_route(f); }
        const bool same = r[0].side == r[1].side && r[0].bank_pipe == r[1].bank_pipe && r[0].plain == r[1].plain && r[0].raw_fused == r[1].raw_fused &&
                          r[0].staged == r[1].staged && r[0].fuse_dec == r[1].fuse_dec && r[0].rot3 == r[1].rot3 && r[0].mid == r[1].mid &&
                          r[0].done_in_kernel == r[1].done_in_kernel && r[0].timed_handover == r[1].timed_handover && r[0].tail == r[1].tail &&
                          r[0].tune_only == r[1].tune_only;
        std::printf("same %d %d %d %d %d\\n", (int)same, (int)r[1].side, (int)r[1].bank_pipe, (int)r[0].rescale, (int)r[1].rescale);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("auto_scale_route")
    src, exe = d / "route.cpp", str(d / "route")
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])
    return subprocess.check_output([exe], text=True).strip().split("\n")


def test_the_recalc_stage_needs_a_request_and_a_spectrum(lines):
    got = {tuple(int(v) for v in ln.split()[:3]): int(ln.split()[3]) for ln in lines[:8]}
    for pending, spectrum, gated in itertools.product((0, 1), repeat=3):
        # (a gated call is planned with the stage too: whether its timer selects a row is decided after the route)
        assert got[(pending, spectrum, gated)] == int(pending and spectrum), (pending, spectrum, gated)


def test_the_request_moves_no_other_field(lines):
    assert lines[8].split() == ["same", "1", "1", "0", "0", "1"]   # side by side, with a spectrum: the stage is planned
    assert lines[9].split() == ["same", "1", "0", "1", "0", "0"]   # two-stage call, no spectrum: never
    assert SIDE["with_spectrum"] == 1 and PIPE["with_spectrum"] == 0 and "scale_pending" not in FACTS
