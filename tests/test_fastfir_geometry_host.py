"""CPU tier of the band-pass geometry table (tests/fastfir_cases.py).

 - At every row the oracle (the reference's sample-at-a-time loop, restated) IS the convolution with its own designed taps, in fp64
   direct form: the reference binary cannot say so (tests/test_reference_pins.py: its sizes are #defines), this does.
 - Beyond overlap <= L it is not -- which is why the library refuses those sizes.
 - The rows satisfy the size rules the library enforces and reach the grid shapes they are there for.
 - The input is adequate: two deliberately wrong overlap-saves miss the GPU tier's bar by a factor of 100 on the chunks they reach.
 - design::fastfir_design (compiled here with g++) designs what the oracle designs.
"""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import fastfir_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pebblesdr_amd", "csrc")
EXACT = 1e-12        # fp64 against fp64: transforms of 8192 points against sums of 4097 products
MARGIN = 100 * FC.TOL


# ------------------------------------------------------------------------------------------------
# plain numpy
# ------------------------------------------------------------------------------------------------
def taps_of(ref):
    """the oracle's designed taps in the time domain: ifft(coef())[:taps] * fft (1/fft is folded into coef, fastfir.cpp:244-245)"""
    h = np.fft.ifft(ref.coef()) * ref.fft_size
    assert np.abs(h[ref.fir_size:]).max() <= 1e-15 * max(1.0, np.abs(h).max())  # (the transform's direction is numpy's)
    return h[:ref.fir_size].copy()


class OverlapSave:
    """Overlap-save that carries TRUE history: the last `ov` input samples, whatever the block length.  ov = taps - 1 is right.
    Two deliberate mistakes: zero_carry forgets the carried samples at the start of every call after the first; ov = taps is a kernel
    told `overlap = taps` by a host that still places blocks L apart: its window starts one sample early and ends one early, it
    discards one output too many, and the last output of every block is never written (zero here)."""

    def __init__(self, fft, taps, ov=None, zero_carry=False):
        self.fft, self.ov = fft, taps - 1 if ov is None else ov
        self.hop = fft - (taps - 1)
        self.hist = np.zeros(self.ov, dtype=np.complex128)
        self.pend = np.zeros(0, dtype=np.complex128)
        self.zero_carry, self.calls = zero_carry, 0
        self.H = np.zeros(fft, dtype=np.complex128)

    def set_taps(self, h):
        self.H = np.fft.fft(h, self.fft)

    def process(self, x):
        if self.zero_carry and self.calls:
            self.hist[:] = 0
        self.calls += 1
        self.pend = np.concatenate([self.pend, np.asarray(x, dtype=np.complex128)])
        out = []
        while len(self.pend) >= self.hop:
            new = self.pend[:self.hop]
            y = np.fft.ifft(np.fft.fft(np.concatenate([self.hist, new[:self.fft - self.ov]])) * self.H)[self.ov:]
            out.append(np.concatenate([y, np.zeros(self.hop - len(y), dtype=np.complex128)]))
            both = np.concatenate([self.hist, new])
            self.hist = both[len(both) - self.ov:]
            self.pend = self.pend[self.hop:]
        return np.concatenate(out) if out else np.zeros(0, dtype=np.complex128)


def direct(x, h, lo, hi):
    """y[n] = sum_j h[j] x[n - j] for lo <= n < hi, x zero before its first sample: fp64 direct form"""
    if hi <= lo:
        return np.zeros(0, dtype=np.complex128)
    back = len(h) - 1
    seg = x[max(0, lo - back):hi]
    if lo < back:
        seg = np.concatenate([np.zeros(back - lo, dtype=np.complex128), seg])
    return np.convolve(seg, h, mode="valid")


def fit(w, n):
    """a wrong model's call output against the oracle's n samples: cut or padded with zeros (its count is part of the mistake)"""
    return w[:n] if len(w) >= n else np.concatenate([w, np.zeros(n - len(w), dtype=np.complex128)])


class Stream:
    """one filter stream of a row: the oracle, the right model and the two wrong ones, all given the same taps and calls"""

    def __init__(self, oracle_mod, fft, taps):
        self.fft, self.taps, self.L = fft, taps, FC.geometry(fft, taps)[1]
        self.ref = oracle_mod.FastFIR(fft, taps)
        self.models = {"right": OverlapSave(fft, taps), "no carry": OverlapSave(fft, taps, zero_carry=True), "overlap = taps": OverlapSave(fft, taps, ov=taps)}
        self.h = np.zeros(taps, dtype=np.complex128)
        self.x = np.zeros(0, dtype=np.complex128)
        self.emitted = 0
        self.worst_exact = 0.0
        self.least = {"no carry": np.inf, "overlap = taps": np.inf}
        self.reached = {"no carry": 0, "overlap = taps": 0}

    def setup(self, lo, hi, offset, rate):
        ok = self.ref.setup(lo, hi, offset, rate) == 0
        self.h = taps_of(self.ref)
        for m in self.models.values():
            m.set_taps(self.h)
        return ok

    def call(self, x):
        """one call: the oracle's output is the convolution (and the right model's); every chunk the GPU tier compares is one the wrong
        models miss -- `no carry` where it reaches: the first chunk of a call that starts with carried samples other than zero"""
        carried = bool(np.any(self.models["right"].hist))
        self.x = np.concatenate([self.x, np.asarray(x, dtype=np.complex128)])
        r = self.ref.process(x)
        w = {k: m.process(x) for k, m in self.models.items()}
        if not len(r):
            return r
        y = direct(self.x, self.h, self.emitted, self.emitted + len(r))
        silent = not np.any(self.h)
        if silent:
            assert not np.any(r) and not np.any(w["right"])
        else:
            self.worst_exact = max([self.worst_exact] + FC.chunk_errors(r, y, self.L) + FC.chunk_errors(w["right"], y, self.L))
            for k in self.least:
                e = FC.chunk_errors(fit(w[k], len(r)), r, self.L)
                if k == "no carry":
                    if not carried:
                        continue
                    e = e[:1]
                self.least[k] = min([self.least[k]] + e)
                self.reached[k] += len(e)
        self.emitted += len(r)
        return r


# ------------------------------------------------------------------------------------------------
# the rows, stream by stream
# ------------------------------------------------------------------------------------------------
def run_step(oracle_mod, row, b):
    st = Stream(oracle_mod, row.fft, row.taps)
    outs = FC.run_script(FC.step_script(row, b), FC.step_input(row), st.setup, st.call)
    return st, outs


_decimated = {}


def decimated(oracle_mod, c):
    """the receiver's band-pass input of channel c over the rows' four super-frames: mixer and decimator in 2048-sample frames"""
    if c not in _decimated:
        n = sum(FC.RX_CALLS) * FC.rx_superframe(FC.RX_ROWS[0])
        x = FC.rx_input(n)
        mix, dec = oracle_mod.Mixer(FC.RX_FS), oracle_mod.Decimator(FC.RX_FS, 30000)
        mix.set_frequency(FC.RX_CHANNELS[c][3])
        z = np.concatenate([dec.process(mix.process(x[i:i + FC.RX_FRAME])) for i in range(0, n, FC.RX_FRAME)])
        assert len(z) == n // FC.RX_D
        _decimated[c] = z
    return _decimated[c]


def run_rx(oracle_mod, row, c):
    """the band-pass stage of channel c: calls of 1, 2 and 1 super-frames at the demodulator's rate"""
    st = Stream(oracle_mod, row.fft, row.taps)
    _, lo, hi, _ = FC.RX_CHANNELS[c]
    assert st.setup(lo, hi, 0.0, float(FC.RX_FS // FC.RX_D))
    z, at, outs = decimated(oracle_mod, c), 0, []
    for k in FC.RX_CALLS:
        n = k * FC.rx_superframe(row) // FC.RX_D
        outs.append(st.call(z[at:at + n]))
        assert len(outs[-1]) == n
        at += n
    return st, outs


def run_sb(oracle_mod, row, fmt, s):
    st = Stream(oracle_mod, row.fft, row.taps)
    assert st.setup(FC.SB_BANDS[s][0], FC.SB_BANDS[s][1], 0.0, FC.FS)
    x = FC.sb_input(row, fmt, oracle_mod)[1][s]
    n, outs = FC.sb_call_samples(row), []
    for k in range(FC.SB_CALLS):
        outs.append(st.call(x[k * n:(k + 1) * n]))
        assert len(outs[-1]) == n
    return st, outs


def all_streams(oracle_mod):
    """(label, Stream) of every stream of every row, run"""
    for row, b in FC.step_cases():
        yield "%s band %s" % (row.name, b), run_step(oracle_mod, row, b)[0]
    for row in FC.RX_ROWS:
        for c in range(len(FC.RX_CHANNELS)):
            yield "%s channel %d" % (row.name, c), run_rx(oracle_mod, row, c)[0]
    for row, fmt in FC.sb_cases():
        for s in range(FC.SB_S):
            yield "%s %s stream %d" % (row.name, "float2" if fmt is None else FC.FORMATS[fmt][0], s), run_sb(oracle_mod, row, fmt, s)[0]


@pytest.fixture(scope="module")
def streams(oracle_mod):
    return list(all_streams(oracle_mod))


def test_the_oracle_is_the_convolution_at_every_row(streams):
    """oracle.FastFIR.process over the row's calls (and the plain overlap-save beside it) against fp64 direct convolution with
    ifft(coef())[:taps] * fft, per chunk of max(L, 1024) outputs.  Measured worst over the table's 64 streams: 7.0e-16."""
    worst = 0.0
    for label, st in streams:
        assert st.emitted > 0, label
        assert st.worst_exact <= EXACT, (label, st.worst_exact)
        worst = max(worst, st.worst_exact)
    print("oracle against direct convolution, worst chunk over %d streams: %.2e" % (len(streams), worst))


def test_a_lost_or_miscounted_overlap_misses_the_bar_by_100(streams):
    """Input adequacy.  Two wrong overlap-saves against the oracle, on the chunks the GPU tier compares (per call, consecutive chunks of
    max(L, 1024) outputs):
     - `overlap = taps` (the kernel's index arithmetic one off against the host's block placement: one output per block lost) is off by
       at least 100 TOL on EVERY chunk;
     - `no carry` (the carried overlap zeroed at the start of every call after the first) can only touch the first taps - 1 outputs of a
       call, and only when the carried samples were not zero anyway: it is off by at least 100 TOL on the first chunk of every such call.
    A row that fails this needs another input, not another margin."""
    for label, st in streams:
        if not np.any(st.h):  # the constructor row: all-zero taps, the output is zero whatever is carried
            continue
        for k, least in st.least.items():
            assert st.reached[k] >= 2, (label, k)
            assert least >= MARGIN, (label, k, least)
    live = [st for _, st in streams if np.any(st.h)]
    print("least miss of a wrong overlap-save: no carry %.2e, overlap = taps %.2e (bar %.0e)"
          % (min(st.least["no carry"] for st in live), min(st.least["overlap = taps"] for st in live), MARGIN))


def test_step_scripts_redesign_refuse_and_repeat(oracle_mod):
    """what the scripts are there for, on the oracle: the repeat changes nothing, the invalid pair is refused and changes nothing, the
    redesign changes the taps; the constructor's parameters design nothing"""
    for row, b in FC.step_cases():
        ref = oracle_mod.FastFIR(row.fft, row.taps)
        seen = []
        for e in FC.step_script(row, b):
            if e[0] == "setup":
                assert (ref.setup(*e[1]) == 0) == e[2]
                seen.append(ref.coef())
        if row.ctor:
            assert len(seen) == 1 and not np.any(seen[0])
            continue
        first, repeat, invalid, redesign = seen
        assert np.any(first) and np.array_equal(first, repeat) and np.array_equal(first, invalid) and not np.array_equal(first, redesign)
        assert FC.step_calls(row)[-1] > 64 * row.L and (sum(FC.step_calls(row)[3:])) % row.L == 6  # (past the device buffer, a ragged rest)


def test_beyond_overlap_equal_block_the_reference_is_no_convolution(oracle_mod):
    """Why the library refuses taps > fft/2 + 1.  The reference refills only the last L samples of its overlap buffer per block
    (fastfir.cpp:312-316), so with overlap > L the front of the next block's overlap is stale: at 2048/1026 (L = 1023, one stale
    sample under a window that is almost zero there) the oracle departs from the convolution of its own taps by more than 1e-9, at
    2048/1537 (overlap = 3 L) by more than 0.1 -- while a plain overlap-save that carries the true history is exact at both.  Nothing
    pins behaviour there: the reference fixes 2048/1025 by #define."""
    n = 14 * 2048
    x = FC.tones(FC.FS, n, FC.TONES) + FC.lcg_noise(n, 7, FC.SIGMA)
    for taps, least in ((1026, 1e-9), (1537, 0.1)):
        assert not FC.accepted(2048, taps)
        ref = oracle_mod.FastFIR(2048, taps)
        assert ref.setup(300.0, 3000.0, 700.0, FC.FS) == 0
        h = taps_of(ref)
        plain = OverlapSave(2048, taps)
        plain.set_taps(h)
        r, p = ref.process(x), plain.process(x)
        assert len(r) == len(p) >= 10 * (2048 - taps + 1)
        y = direct(x, h, 0, len(r))
        assert FC.rel_rms(p, y) <= EXACT
        assert FC.rel_rms(r, y) > least, (taps, FC.rel_rms(r, y))
        print("2048/%d: oracle against convolution %.2e, plain overlap-save %.2e" % (taps, FC.rel_rms(r, y), FC.rel_rms(p, y)))
    # ... and at the edge of what is accepted the oracle is exact
    assert FC.accepted(2048, 1025) and FC.accepted(4096, 2049) and FC.accepted(8192, 4097) and not FC.accepted(2048, 1)


def test_rows_satisfy_the_size_rules_and_reach_their_grids():
    """FastFirCore::init (2 <= taps <= fft/2 + 1), Receiver::create (super-frame = total decimation * lcm(frame, L)), the stream bank
    (frame % L == 0) and the XCD-ordered grid of k_fastfir_t128 (nb * C workgroups rounded up to a multiple of 8)."""
    names = [r.name for r in FC.STEP_ROWS + FC.RX_ROWS + FC.SB_ROWS]
    assert len(set(names)) == len(names)
    for r in FC.STEP_ROWS + FC.RX_ROWS + FC.SB_ROWS:
        ov, L = FC.geometry(r.fft, r.taps)
        assert FC.accepted(r.fft, r.taps) and L == r.L and ov <= L and ov + L == r.fft, r.name
    # the step's pairs: the three stock ones and, at each transform size, ones with overlap < L
    assert [(r.fft, r.taps) for r in FC.STEP_ROWS if not r.ctor] == [(2048, 2), (2048, 129), (2048, 1024), (2048, 1025), (4096, 1025), (4096, 2049),
                                                                    (8192, 1025), (8192, 4097)]
    assert any(r.taps - 1 != r.L for r in FC.STEP_ROWS) and any(r.L & (r.L - 1) for r in FC.STEP_ROWS) and any(r.L % 2 for r in FC.STEP_ROWS)
    grids = []
    for r in FC.RX_ROWS:
        sf = FC.rx_superframe(r)
        assert sf == FC.RX_D * math.lcm(FC.RX_FRAME, r.L) == 32 * 6144 and sf % FC.RX_FRAME == 0 and (sf // FC.RX_D) % r.L == 0, r.name
        assert max(FC.RX_CALLS) == 2  # max_superframes
        if r.fft == 2048:
            grids += [FC.rx_blocks(r, k) * len(FC.RX_CHANNELS) for k in FC.RX_CALLS]
    for r in FC.SB_ROWS:
        assert r.frame % r.L == 0 and FC.sb_call_samples(r) >= r.taps - 1, r.name
        assert r.bins >= r.frame and r.bins & (r.bins - 1) == 0, r.name
        assert (r.kernel == "k_fastfir_t128") == (r.fft == 2048), r.name
        assert all(f is None or r.fft == 2048 for f in r.fmts), r.name  # (only the 2048-point plan has converting loads)
        if r.fft == 2048:
            grids.append(FC.sb_blocks(r) * FC.SB_S)
    assert sorted(grids) == [6, 12, 12, 12, 24]
    assert any(g % 8 for g in grids) and any(g < 8 for g in grids) and any(g % 8 == 0 for g in grids)
    # the one-dimensional grid's map, restated (kernels_fastfir.h): every (channel, block) exactly once, the surplus workgroups leave
    for nb, C in ((4, 3), (8, 3), (2, 3)):
        total, per = nb * C, (nb * C + 7) // 8
        seen = []
        for wg in range(8 * per):
            q = (wg & 7) * per + (wg >> 3)
            if q < total:
                seen.append(divmod(q, nb))
        assert sorted(seen) == [(c, b) for c in range(C) for b in range(nb)]
    assert {f for r in FC.SB_ROWS for f in r.fmts} == {None, 0, 1, 2, 3, 4}


def test_the_oracle_receiver_hands_out_two_blocks_from_one_frame(oracle_mod):
    """2048/513 fed 2048-sample frames: L = 1536, so the band-pass delivers 1536, 1536 and then 3072 samples -- more than a frame.  The
    Python face's output array has room for it (it once had max(frame, fft) = 2048), and the USB channel is the decimated stream times
    the restored gain through oracle.FastFIR, sample for sample."""
    row = FC.RX_ROWS[0]
    sf = FC.rx_superframe(row)
    x = FC.rx_input(sum(FC.RX_CALLS) * sf)[:sf]
    mode, lo, hi, fc = FC.RX_CHANNELS[0]
    assert (row.fft, row.taps, mode) == (2048, 513, "USB")
    r = oracle_mod.Receiver(FC.RX_FS, FC.RX_FRAME, 0, row.fft, row.taps)
    r.set_mode(oracle_mod.USB); r.set_mixer(fc); r.set_filter(lo, hi)
    outs = [r.process(x[i:i + FC.RX_FRAME], want_spectrum=False)[0] for i in range(0, sf, FC.RX_FRAME)]
    assert [len(o) for o in outs if len(o)] == [1536, 1536, 3072] and r.cap >= 3072
    z = decimated(oracle_mod, 0)[:sf // FC.RX_D]
    f = oracle_mod.FastFIR(row.fft, row.taps)
    assert f.setup(float(np.float32(lo)), float(np.float32(hi)), 0.0, 64000.0) == 0
    gain = 10.0 ** (oracle_mod.Decimator(FC.RX_FS, 30000).dec_by2_stages * 2 / 20.0)
    assert FC.rel_rms(np.concatenate(outs), f.process(z * gain)) <= EXACT


def test_raw_inputs_fill_their_formats(oracle_mod):
    for row, fmt in FC.sb_cases():
        fed, x, gain = FC.sb_input(row, fmt, oracle_mod)
        n = FC.SB_CALLS * FC.sb_call_samples(row)
        assert x.shape == (FC.SB_S, n) and x.dtype == np.complex128
        if fmt is None:
            assert fed.shape == (FC.SB_S, n) and fed.dtype == np.complex64
            continue
        _, dtype, off, full, g = FC.FORMATS[fmt]
        assert fed.shape == (FC.SB_S, n, 2) and fed.dtype == dtype and g == gain
        span = np.abs(fed.astype(np.float64) - off).max()
        assert 0.6 * full <= span <= full, (row.name, fmt, span)
        assert not np.array_equal(fed[0], fed[1]) and not np.array_equal(fed[1], fed[2])


# ------------------------------------------------------------------------------------------------
# the library's design against the oracle's
# ------------------------------------------------------------------------------------------------
def design_queries():
    q = set()
    for row, b in FC.step_cases():
        for e in FC.step_script(row, b):
            if e[0] == "setup" and e[2] and e[1] != FC.CTOR:
                q.add((row.fft, row.taps) + e[1])
    for r in FC.RX_ROWS:
        for _, lo, hi, _ in FC.RX_CHANNELS:
            q.add((r.fft, r.taps, float(np.float32(lo)), float(np.float32(hi)), 0.0, float(FC.RX_FS // FC.RX_D)))
    for r in FC.SB_ROWS:
        for lo, hi in FC.SB_BANDS:
            q.add((r.fft, r.taps, lo, hi, 0.0, FC.FS))
    return sorted(q)


@pytest.fixture(scope="module")
def library_design(tmp_path_factory):
    """(fft, taps, lo, hi, offset, rate) -> H of design::fastfir_design, or None where it refuses"""
    d = tmp_path_factory.mktemp("fastfir_design")
    src = d / "ffdesign.cpp"
    src.write_text('#include <cstdio>\n#include "design.h"\n'
                   'int main()\n{\n    unsigned fft, taps;\n    double lo, hi, off, fs;\n'
                   '    while (std::scanf("%u %u %lf %lf %lf %lf", &fft, &taps, &lo, &hi, &off, &fs) == 6) {\n'
                   '        std::vector<std::complex<double>> H;\n'
                   '        const unsigned ok = pg::design::fastfir_design(fft, taps, lo, hi, off, fs, H) ? 1u : 0u;\n'
                   '        std::fwrite(&ok, sizeof ok, 1, stdout);\n'
                   '        if (ok) std::fwrite(H.data(), sizeof(std::complex<double>), H.size(), stdout);\n    }\n    return 0;\n}\n')
    exe = str(d / "ffdesign")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, str(src), os.path.join(CSRC, "design.cpp"),
                           "-o", exe])  # (-ffp-contract=off as oracle/Makefile: no fused multiply-adds on either side)

    def many(queries):
        text = "".join("%d %d %.17g %.17g %.17g %.17g\n" % q for q in queries)
        blob = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout
        out, at = [], 0
        for q in queries:
            (ok,) = struct.unpack_from("I", blob, at)
            at += 4
            if ok:
                out.append(np.frombuffer(blob, dtype=np.complex128, count=q[0], offset=at).copy())
                at += 16 * q[0]
            else:
                out.append(None)
        assert at == len(blob)
        return out
    return many


DESIGN_BAR = 10 * 0.0  # ten times the measured worst (0.0: see the test), under the ceiling of 1e-9


def test_the_library_designs_what_the_oracle_designs(oracle_mod, library_design):
    """design::fastfir_design against oracle.FastFIR.coef() for every (fft, taps, lo, hi, offset, rate) of the table, rel-RMS over the
    fft frequency-domain points.  Both are fp64 with a transform of their own (design.cpp's against pebble_oracle.c's); equality was not
    assumed but measured: worst rel-RMS over the table's 37 designs 0.0e+00 -- the two compute the same taps and run the same radix-2
    recurrence, both compiled without contraction into fused multiply-adds.  The bar is ten times the measured worst, so 0.  The refused
    pair and the constructor's parameters are refused by both."""
    qs = design_queries()
    assert len(qs) >= 3 * 8 + 3 * 3  # (the stream bank's designs partly coincide with the receiver's)
    worst = 0.0
    for q, H in zip(qs, library_design(qs)):
        ref = oracle_mod.FastFIR(q[0], q[1])
        assert ref.setup(*q[2:]) == 0 and H is not None, q
        e = FC.rel_rms(H, ref.coef())
        worst = max(worst, e)
        assert e <= DESIGN_BAR, (q, e)
    print("design::fastfir_design against the oracle over %d designs: worst rel-RMS %.2e" % (len(qs), worst))
    bad = [(2048, 1025) + FC.INVALID, (2048, 1025, -1.0 + 1.0, 1.0 + 1.0, 0.0, 1.0)]  # (the constructor's values, offset applied: hi >= rate / 2)
    assert library_design(bad) == [None, None]
    assert oracle_mod.FastFIR(2048, 1025).setup(*FC.INVALID) != 0
