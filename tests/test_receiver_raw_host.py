"""CPU tier of raw device-format input into a receiver (tests/raw_cases.py is the coverage statement).

1. The loaders of csrc/raw_load.h -- raw_load, raw_load1, raw_fetch4 + raw_convert4 (raw_load4) and raw_load4_even -- compiled for the
   host with g++ and run against raw_cases.host_convert_parts bit for bit: every format x IQ order, all 65536 byte pairs of the 8-bit
   formats, all 65536 values in either component of the 16-bit ones, a float set with signed zeros, denormals, large values and NaN
   payloads; raw_load4_even from every even offset modulo 8.
2. plan_call_route() of csrc/call_route.h, compiled as tests/test_call_route_host.py does, on the facts every call of every row
   implies: call 0 staged, calls 1..3 raw-fused, and what takes raw_fused away.
3. The table's own claims as literals, and the rows' inputs (extreme codes at every quad position, a negative value in every shift
   lane, I and Q distinct).
4. Wrong conversions on the oracle alone: each moves the oracle-tied comparison of every row of its format by >= 100 bars; the ones
   only the bit-for-bit twin comparison can see are named as such.
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import decim_cases, raw_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")

LOADERS_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "raw_load.h"
using namespace pg;

static void put(const std::vector<float2> &o) { std::fwrite(o.data(), sizeof(float2), o.size(), stdout); }

template <int F>
static void run(const RawSrc &r, long long n)
{
    std::vector<float2> o((size_t)n);
    float2 q[4];
    for (long long i = 0; i < n; i++) o[i] = raw_load(r, i);
    put(o);
    for (long long i = 0; i < n; i++) o[i] = raw_load1<F>(r, i);
    put(o);
    for (long long i = 0; i + 4 <= n; i += 4) {
        RawQuad<F> w;
        raw_fetch4<F>(r, i, w);
        raw_convert4<F>(r, w, q);
        for (int k = 0; k < 4; k++) o[i + k] = q[k];
    }
    put(o);
    for (long long i = 0; i + 4 <= n; i += 4) {
        raw_load4<F>(r, i, q);
        for (int k = 0; k < 4; k++) o[i + k] = q[k];
    }
    put(o);
    for (int e = 0; e < 8; e += 2) {  // windows from every even offset modulo 8
        std::memset(o.data(), 0, sizeof(float2) * o.size());
        for (long long i = e; i + 4 <= n; i += 8) {
            raw_load4_even<F>(r, i, q);
            for (int k = 0; k < 4; k++) o[i + k] = q[k];
        }
        put(o);
    }
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const int fmt = std::atoi(argv[1]), order = std::atoi(argv[2]);
    const double gain = std::strtod(argv[3], nullptr);
    const long long n = std::atoll(argv[4]);
    if (fmt < 0 || fmt > 4 || n % 8) return 2;
    const size_t bytes = (size_t)n * kRawPairBytes[fmt];
    void *buf = std::aligned_alloc(64, (bytes + 63) / 64 * 64);
    if (std::fread(buf, 1, bytes, stdin) != bytes) return 3;
    const RawSrc r{buf, fmt, order, raw_scale(fmt, gain), 0};
    switch (fmt) {
    case 0: run<0>(r, n); break;
    case 1: run<1>(r, n); break;
    case 2: run<2>(r, n); break;
    case 3: run<3>(r, n); break;
    default: run<4>(r, n); break;
    }
    std::free(buf);
    return 0;
}
"""
N_BLOCKS = 8   # raw_load, raw_load1, fetch4 + convert4, raw_load4, raw_load4_even x 4 offsets


@pytest.fixture(scope="module")
def loaders(tmp_path_factory):
    d = tmp_path_factory.mktemp("raw_load")
    src = d / "loaders.cpp"
    src.write_text(LOADERS_MAIN)
    exe = str(d / "loaders")
    # -ffp-contract=off: the header's host stand-in for __fmul_rn is a plain product
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I" + CSRC, str(src), "-o", exe])

    def run(raw, fmt, order, gain):
        """-> uint32 [N_BLOCKS, n, 2]: the bits of what every loader gave"""
        n = raw.shape[0]
        out = subprocess.check_output([exe, str(fmt), str(order), float(gain).hex(), str(n)], input=np.ascontiguousarray(raw).tobytes())
        return np.frombuffer(out, dtype=np.uint32).reshape(N_BLOCKS, n, 2)

    return run


def exhaustive_input(fmt):
    """[n, 2] components: every byte pair (8-bit), every value in either component (16-bit), the float corners"""
    dtype = rc.FORMATS[fmt][0]
    if dtype in (np.int8, np.uint8):
        v = np.arange(65536, dtype=np.uint32)
        return np.stack([v & 0xFF, v >> 8], axis=-1).astype(np.uint8).view(dtype)
    if dtype == np.int16:
        v = np.arange(65536, dtype=np.uint32)
        second = (v * 40503 + 12345) & 0xFFFF   # (an odd multiplier: a permutation of all 65536 values, out of step with the first)
        return np.stack([v, second], axis=-1).astype(np.uint16).view(np.int16)
    bits = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000, 0xBF800000, 0x3FC00000,
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC54321, 0x7FA00001, 0xFF812345,
            0x3DCCCCCD, 0xC2F6E979, 0x4B800000, 0x00012345]
    rng = np.random.default_rng(3)
    a = np.array(bits + list(rng.integers(0, 1 << 32, 40, dtype=np.uint64)), dtype=np.uint32)
    b = np.roll(a, 7)
    return np.stack([a, b], axis=-1).view(np.float32)


@pytest.mark.parametrize("fmt,order", list(itertools.product(range(5), range(4))))
def test_every_loader_is_host_convert_bit_for_bit(loaders, fmt, order):
    raw = exhaustive_input(fmt)
    n = raw.shape[0]
    assert n % 8 == 0
    if fmt != 3:
        assert len({(int(a), int(b)) for a, b in raw[:: max(1, n // 4096)]}) > 1000
        for comp in (0, 1):
            assert len(np.unique(raw[:, comp])) == (256 if fmt < 2 else 65536)
        if fmt < 2:
            assert len(np.unique(raw.view(np.uint16))) == 65536
    gain = rc.GAIN[fmt]
    want = rc.host_convert_parts(raw, fmt, order, gain).view(np.uint32)
    got = loaders(raw, fmt, order, gain)
    names = ["raw_load", "raw_load1", "raw_fetch4 + raw_convert4", "raw_load4"]
    for k, name in enumerate(names):
        bad = np.nonzero((got[k] != want).any(axis=1))[0]
        assert bad.size == 0, "%s: %d samples differ, first at %d: raw %r" % (name, bad.size, bad[0], raw[bad[0]])
    for j, e in enumerate(range(0, 8, 2)):
        idx = (np.arange(e, n - 3, 8)[:, None] + np.arange(4)).reshape(-1)
        assert idx.size >= n // 2 - 8
        bad = np.nonzero((got[4 + j][idx] != want[idx]).any(axis=1))[0]
        assert bad.size == 0, "raw_load4_even from offset %d: %d samples differ, first at %d" % (e, bad.size, idx[bad[0]])


def test_the_float_set_holds_what_it_claims():
    raw = exhaustive_input(3)
    bits = raw.view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 0).any()
    expo, frac = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    assert ((expo == 0) & (frac != 0)).sum() >= 8                # denormals
    assert ((expo == 255) & (frac != 0)).sum() >= 8              # NaNs, quiet and signalling, with payloads
    assert ((expo == 255) & (frac == 0)).sum() >= 4              # infinities
    assert (np.abs(raw[np.isfinite(raw)]) > 1e30).any()


def test_host_convert_is_the_order_select_of_one_product():
    """the reference every comparison of both tiers rests on, spelled out once on literals"""
    raw = np.array([[-128, 127], [1, -2]], dtype=np.int8)
    s = np.float32(0.7 / 128.0)
    i, q = raw[:, 0].astype(np.float32) * s, raw[:, 1].astype(np.float32) * s
    for order, (re, im) in enumerate(((i, q), (q, i), (i, i), (q, q))):
        p = rc.host_convert_parts(raw, 0, order, 0.7)
        assert np.array_equal(p[:, 0], re) and np.array_equal(p[:, 1], im)
        x = rc.host_convert(raw, 0, order, 0.7)
        assert x.dtype == np.complex64 and np.array_equal(x.real, re) and np.array_equal(x.imag, im)
    u = rc.host_convert_parts(np.array([[0, 255]], dtype=np.uint8), 1, 0, 1.0)
    assert u.tolist() == [[-1.0, 127.0 / 128.0]]
    z = rc.host_convert_parts(np.array([[-0.0, 1e-40]], dtype=np.float32), 3, 0, 0.9)
    assert np.signbit(z[0, 0]) and z[0, 0] == 0 and 0 < z[0, 1] < 1e-40


# ------------------------------------------------------------------------------------------------
# the routes
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    from tests import test_call_route_host as T
    d = tmp_path_factory.mktemp("raw_route")
    src = d / "route.cpp"
    sets = "\n".join('            if (!std::strcmp(tok, "%s")) { f.%s = (decltype(f.%s))v; known = true; }' % (k, k, k) for k in T.FACTS)
    src.write_text(T.MAIN % sets)
    exe = str(d / "route")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe])

    def plan(rows):
        text = "".join(" ".join("%s=%d" % (k, int(v)) for k, v in row.items()) + "\n" for row in rows)
        out = subprocess.check_output([exe], input=text, text=True).strip().split("\n")
        assert len(out) == len(rows)
        return [dict(zip(T.ROUTE, (int(v) for v in line.split()))) for line in out]

    return plan


def test_call_0_is_staged_and_calls_1_to_3_are_raw_fused(planner):
    facts = [rc.call_facts(row, k) for row in rc.ROWS for k in range(len(rc.SCRIPT))]
    routes = planner(facts)
    for f, r in zip(facts, routes):
        assert r["side"] == 1, f
        if f["osc_transient"]:
            assert (r["raw_fused"], r["staged"]) == (0, 1), f
        else:
            assert (r["raw_fused"], r["staged"]) == (1, 0), f
    for row in rc.ROWS:
        assert [rc.input_route(row, k) for k in range(4)] == ["k_normalize_iq"] + ["raw " + rc.TAG[row.fmt]] * 3
        assert [rc.front_kernel(row, k) for k in range(4)] == ["k_mix_hb11_bank"] + ["k_mix_hb11_lean"] * 3


def test_what_takes_raw_fused_away(planner):
    """the hand-over tests of the GPU tier lean on these: two streams, two channels (no LDS-free front), another number of bins (no
    converting display kernel), conditioners, the generator, per-kernel profiling, a squelch value"""
    base = rc.call_facts(rc.ROWS[0], 1)
    assert planner([base])[0]["raw_fused"] == 1
    two_channels = {k: v for k, v in base.items() if k not in ("dec_lds_free_front", "dec_raw_front")}
    two_channels["C"] = 2
    other_bins = {k: v for k, v in base.items() if k != "spec_raw_ready"}
    off = [dict(base, S=2), two_channels, other_bins, dict(base, cond_any=1), dict(base, cond_dirty=1), dict(base, generator=1),
           dict(base, profiling=1), dict(base, squelch_set=1)]
    for f, r in zip(off, planner(off)):
        assert (r["raw_fused"], r["staged"]) == (0, 1), f


# ------------------------------------------------------------------------------------------------
# the table's own claims
# ------------------------------------------------------------------------------------------------
def test_the_rows_are_what_the_statement_says():
    rows = rc.ROWS
    assert len(rows) == 13 and len({r.name for r in rows}) == 13
    assert {(r.fmt, r.stride) for r in rows} == {(0, 8), (0, 2), (0, 32), (1, 2), (1, 8), (2, 32), (2, 8), (3, 8), (3, 2), (4, 8), (4, 2)}
    for fmt in range(5):
        mine = [r for r in rows if r.fmt == fmt]
        assert len({r.stride for r in mine}) >= 2, fmt
        assert any(r.order != 0 for r in mine), fmt
    assert {r.order for r in rows} == {0, 1, 2, 3}
    assert {r.fs for r in rows} == {1_024_000, 2_800_000, 9_800_000, 20_000_000}
    assert {r.fs: r.stride for r in rows} == {1_024_000: 2, 2_800_000: 8, 9_800_000: 32, 20_000_000: 8}
    assert all(r.wfm == (r.fs == 20_000_000) for r in rows)
    # every one of the eight instances that only int8 had reached, by name
    assert {rc.lean_instance(r) for r in rows} == {"k_mix_hb11_lean<%d>" % f for f in range(5)}
    assert {rc.spectrum_instance(r) for r in rows} == {"k_spectrum_t128<2, %d>" % f for f in range(5)}
    assert rc.SCRIPT == (1, 2, 1, 3) and rc.MAX_SF == 3 and rc.BINS == 8192
    assert rc.GAIN == {0: 0.7, 1: 1.0, 2: 1.3, 3: 0.9, 4: 0.5}
    assert np.log2(rc.GAIN[4]) % 1 == 0   # a power of two where the normaliser is 32767
    assert rc.PAIR_BYTES == {0: 2, 1: 2, 2: 4, 3: 8, 4: 4}
    # the oracle tie: one row per rate at the least, all five formats
    orows = [rc.ROW[n] for n in rc.ORACLE_ROWS]
    assert {r.fs for r in orows} == {r.fs for r in rows} and {r.fmt for r in orows} == set(range(5)) and len(orows) == 5
    assert {rc.ROW[n].fmt for n in rc.GATED_ROWS} == set(range(5)) and len(rc.GATED_ROWS) == 5
    assert {rc.ROW[n].fmt for n in rc.RECORD_ROWS} == set(range(5)) and sum(rc.ROW[n].order != 0 for n in rc.RECORD_ROWS) >= 3


@pytest.fixture(scope="module")
def chains(oracle_mod):
    return {fs: oracle_mod.Decimator(fs, 200000 if fs == rc.WFM_FS else 30000).chain() for fs in rc.FC}


def test_the_chains_and_kernels_behind_the_rows(chains):
    want = {1_024_000: (2, 5, "k_cascade<15,19,31>"), 2_800_000: (8, 2, "k_cascade<0,0,0>"), 9_800_000: (32, 1, None), 20_000_000: (8, 2, "k_cascade<15,23,47>")}
    for row in rc.ROWS:
        chain = [tuple(s) for s in chains[row.fs]]
        stride, j_first, casc = want[row.fs]
        assert chain[0] == (11, stride) == (11, row.stride), row.name
        assert (10 + stride - 1) // stride == j_first
        for k, nsf in enumerate(rc.SCRIPT):
            r = decim_cases.route(chain, 1, True, True, k == 0, nsf * rc.FRAME)
            assert r.front == rc.front_kernel(row, k), (row.name, k)
            assert r.front_inst == ("k_mix_hb11_bank<true,false>" if k == 0 else "k_mix_hb11_lean<-1>")  # (route() knows the float2 instance only)
            if casc:
                assert r.cascade_inst == casc, row.name
        sf = rc.superframe(chain)
        assert sf % rc.FRAME == 0 and (sf * rc.PAIR_BYTES[row.fmt]) % rc.RAW_ALIGN == 0   # every call of a run starts aligned


def test_the_header_and_the_table_agree_on_the_constants():
    import re
    text = open(os.path.join(CSRC, "raw_load.h")).read()
    m = re.search(r"kRawPairBytes\[5\] = \{([^}]*)\}", text)
    assert [int(v) for v in m.group(1).split(",")] == [rc.PAIR_BYTES[f] for f in range(5)]
    pub = open(os.path.join(ROOT, "include", "pebblegpu.h")).read()
    assert int(re.search(r"#define\s+PEBBLEGPU_RAW_ALIGN\s+(\d+)", pub).group(1)) == rc.RAW_ALIGN
    assert "PEBBLEGPU_RAW_ALIGN" in pub[pub.index("The same call fed with the device's own sample format"):pub.index("int pebblegpu_receiver_process_raw(")]


# ------------------------------------------------------------------------------------------------
# the rows' inputs
# ------------------------------------------------------------------------------------------------
SMALL_SF = 32768   # the checks on the arrays do not depend on the row's super-frame: the smallest one (1.024 Msps) for all


@pytest.mark.parametrize("name", [r.name for r in rc.ROWS])
def test_row_inputs_carry_the_edges(name):
    row = rc.ROW[name]
    dtype, off, norm = rc.FORMATS[row.fmt]
    raw = rc.row_raw(name, SMALL_SF)
    assert raw.dtype == dtype and raw.shape == (sum(rc.SCRIPT) * SMALL_SF, 2) and not raw.flags.writeable
    bits = np.ascontiguousarray(raw).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[raw.itemsize])
    codes = np.array(rc.extremes(row.fmt)).view(bits.dtype)
    assert len(set(codes.tolist())) == (4 if row.fmt == 3 else 2)
    for lo, n in rc.call_bounds(SMALL_SF):
        call = bits[lo:lo + n]
        for pos in range(4):
            for comp in range(2):
                lane = call[pos::4, comp]
                for code in codes:
                    assert (lane == code).any(), (name, lo, pos, comp, hex(int(code)))
    # the edges of the format's range really are its edges
    if row.fmt != 3:
        info = np.iinfo(dtype)
        assert raw.min() == info.min and raw.max() == info.max
        centred = raw.astype(np.int32) - int(off)
    else:
        assert raw.max() > 1.0 and raw.min() < -1.0
        assert (bits == 0x80000000).any() and (((bits & 0x7F800000) == 0) & ((bits & 0x007FFFFF) != 0)).any()   # -0.0f, a denormal
        centred = raw
    # a negative value in every shift lane of raw_convert4 / raw_load4_even (4 quad positions x 2 components), in every call
    for lo, n in rc.call_bounds(SMALL_SF):
        for pos in range(4):
            for comp in range(2):
                assert (centred[lo + pos:lo + n:4, comp] < 0).mean() > 0.3
    # the noise fills the range
    for comp in range(2):
        assert np.percentile(np.abs(centred[:, comp].astype(np.float64)), 99.9) > 0.85 * norm
    # I and Q are distinct: every order gives another stream
    x = [rc.host_convert(raw[:8192], row.fmt, o, rc.GAIN[row.fmt]) for o in range(4)]
    for a, b in itertools.combinations(range(4), 2):
        assert (x[a] != x[b]).mean() > 0.9, (a, b)


# ------------------------------------------------------------------------------------------------
# wrong conversions on the oracle alone
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_truth(oracle_mod, chains):
    """name -> (raw of the row's first super-frame, the oracle's audio and spectra on the right conversion), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            row = rc.ROW[name]
            sf = rc.superframe(chains[row.fs])
            raw = rc.row_raw(name, sf)[:sf]
            cache[name] = (raw,) + rc.oracle_run(oracle_mod, row, rc.host_convert(raw, row.fmt, row.order, rc.GAIN[row.fmt]))
        return cache[name]

    return get


def test_the_reference_of_the_9_8_msps_rows_is_the_oracle_receiver(oracle_mod, oracle_truth, chains):
    """At 9.8 Msps a 2048-sample frame hands the decimator's 59-tap last stage 16 samples: the reference falls back to sample
    skipping there (decimator.cpp:602-625), the oracle does as it does, the library streams with exact history.  Those rows take
    their audio from oracle_narrow_audio at 8192-sample frames.  Here: that chain is oracle.Receiver sample for sample on the narrow
    rows where nothing falls back, and at 9.8 Msps 2048-sample frames do give another stream than 8192-sample ones."""
    assert {fs: rc.oracle_frame(chains[fs]) for fs in rc.FC} == {1_024_000: 2048, 2_800_000: 2048, 9_800_000: 8192, 20_000_000: 2048}
    for name in ("u8-x2-iq", "wav16-x8-qi"):
        row = rc.ROW[name]
        raw, ra, _ = oracle_truth(name)
        x = rc.host_convert(raw, row.fmt, row.order, rc.GAIN[row.fmt])
        own = rc.oracle_narrow_audio(oracle_mod, row, x, 2048)
        assert own.shape == ra.shape and np.abs(ra).max() > 1e-3 and np.array_equal(own, ra), name
        # ... and the decimator is frame-invariant where nothing falls back: 8192-sample frames give the same stream
        assert rc.rel_rms(rc.oracle_narrow_audio(oracle_mod, row, x, 8192), ra) < 1e-12, name
    row = rc.ROW["s16-x32-qi"]
    raw, ra, _ = oracle_truth(row.name)
    x = rc.host_convert(raw, row.fmt, row.order, rc.GAIN[row.fmt])
    assert np.array_equal(rc.oracle_narrow_audio(oracle_mod, row, x, 8192), ra)
    assert rc.rel_rms(rc.oracle_narrow_audio(oracle_mod, row, x, 16384), ra) < 1e-12
    assert rc.rel_rms(rc.oracle_narrow_audio(oracle_mod, row, x, 2048), ra) > 1e-2


@pytest.mark.parametrize("wrong", rc.WRONG)
def test_wrong_conversions_cannot_pass_the_oracle_tie(oracle_mod, oracle_truth, wrong):
    """each wrong conversion, on every row of its format: the first super-frame through the oracle, held to the oracle on the right
    conversion with the bars of the GPU tier's oracle tie"""
    rows = [r for r in rc.ROWS if rc.applies(wrong, r)]
    assert rows
    worst = None
    for row in rows:
        raw, ra, rs = oracle_truth(row.name)
        x = rc.wrong_convert(wrong, raw, row.fmt, row.order, rc.GAIN[row.fmt])
        a, s = rc.oracle_run(oracle_mod, row, x)
        b, wa, wd = rc.bars(a, s, ra, rs)
        print("%-22s %-16s %12.0f bars (audio rel-RMS %.3e, spectrum %.3f dB)" % (wrong, row.name, b, wa, wd))
        worst = b if worst is None else min(worst, b)
        assert b >= rc.MARGIN, (wrong, row.name, b)
    print("%-22s smallest miss %.0f bars over %d rows" % (wrong, worst, len(rows)))


def test_the_right_conversion_is_zero_bars_and_wav_by_32768_is_for_the_twin(oracle_mod, oracle_truth):
    """WAV PCM16 normalised by 32768 instead of 32767 is 3e-5 relative: a few bars of the oracle tie at the most, far under the
    margin -- only np.array_equal against the twin sees it (TWIN_ONLY), and it does: most samples differ in their last bits"""
    assert rc.TWIN_ONLY == ("wav-by-32768",)
    for row in [r for r in rc.ROWS if r.fmt == 4]:
        raw, ra, rs = oracle_truth(row.name)
        b0, _, _ = rc.bars(*rc.oracle_run(oracle_mod, row, rc.host_convert(raw, 4, row.order, rc.GAIN[4])), ra, rs)
        assert b0 == 0.0
        x = rc.wrong_convert("wav-by-32768", raw, 4, row.order, rc.GAIN[4])
        b, wa, wd = rc.bars(*rc.oracle_run(oracle_mod, row, x), ra, rs)
        print("wav-by-32768           %-16s %12.2f bars (audio rel-RMS %.3e, spectrum %.5f dB)" % (row.name, b, wa, wd))
        assert b < rc.MARGIN
        right = rc.host_convert(raw, 4, row.order, rc.GAIN[4])
        assert (x != right).mean() > 0.5
