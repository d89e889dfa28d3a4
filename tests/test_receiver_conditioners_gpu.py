"""GPU tier of the receiver's input-conditioner table (tests/cond_cases.py): every row through P.ReceiverBank, call by call, against the
oracle chain -- which tests/test_receiver_conditioners_host.py shows to be the stream bank's Chain and the oracle Receiver's own
conditioner block, and on whose rows it shows every wrong model (a wrong restart of IQ balance, state by list position, DC or blanker
state dropped, kept awake or reset at the wrong time, stages out of order, the copy read at the wrong pitch, a negative gain taken for
'off') to miss the first bar below by a factor of 100 or more.

Bars, all the suite's own (tests/test_parity_gpu.py):
  - pebblegpu_receiver_conditioned() against the oracle chain: rel-RMS <= TOL (1e-5) per chunk of 512 consecutive samples of every stream
    and call, the first call included; NB1's exact-zero positions identical to the oracle's; rows of streams with flags 0 bit for bit the
    input; None after every call that conditioned nothing;
  - audio <= TOL per channel and call (USB, no AGC; WFM);
  - spectrum rows <= TOL_DB (0.1 dB) from the run's second row on; the S-meter and the zoomed rows the same (`downstream`);
  - the same row run twice gives the same bits.
Every test prints its figures before it asserts.  Measured figures: DESIGN.md, "Receiver input conditioners: stream lists, frame sizes,
call routes"."""
import numpy as np
import pytest

from tests import cond_cases as CC
from tests.demod_cases import E_SIZE
from tests.spectrum_gate_ref import GateTimer
from tests.test_parity_gpu import TOL, TOL_DB, db_err, rel_rms

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_rx(P, row):
    rx = P.ReceiverBank(row.fs, row.C, row.shared, row.wfm, row.bins, frames_per_buffer=row.nf, max_superframes=row.max_sf, hires_bins=row.hires)
    assert rx.superframe == row.sf and rx.n_streams == row.S and rx.D == (CC.WFM_D if row.wfm else CC.D)
    for c in range(row.C):
        rx.set_mixer(c, CC.mixer_of(row, c))
        if not row.wfm:
            rx.set_mode(c, P.DM_USB)
            rx.set_bandpass(c, *CC.band_of(row))
    return rx


def run_row(P, row, rx, script=True, raw=False, after_call=None):
    """the row's calls with its setter calls -> [call] dict(audio, spec, cond, names); after_call(k, rx, out) adds what a row reads besides"""
    x, res = CC.row_input(row.name), []
    for k, (lo, n) in enumerate(CC.call_bounds(row)):
        if script:
            for s, f, g, p in CC.setters_before(row, k):
                rx.set_conditioners(s, f, g, p)
        if raw:
            buf = P.DeviceBuffer.from_array(np.ascontiguousarray(CC.row_raw(row.name)[:, lo:lo + n]), 0)
            try:
                rx.process_raw_device(buf.ptr, n, CC.RAW_FMT, 0, CC.RAW_GAIN)
                a, s = rx.audio(), (rx.spectrum() if row.bins else None)
            finally:
                buf.free()
        else:
            a, s = rx.process(x[:, lo:lo + n])
        cond = rx.conditioned()
        out = dict(audio=a, spec=s, cond=None if cond is None else cond.copy(), names=tuple(rx.kernel_name(w) for w in (2, 3, 4, 6)))
        if after_call:
            after_call(k, rx, out)
        res.append(out)
    return res


def check_view(row, res, want, label=""):
    """conditioned() of every call against the oracle chain; prints the worst chunk, then asserts"""
    x, fl = CC.row_input(row.name), CC.flags_during(row)
    figs, zeros = [], 0
    for k, (lo, n) in enumerate(CC.call_bounds(row)):
        got = res[k]["cond"]
        if want[k] is None:
            assert got is None, "%s call %d conditioned nothing" % (row.name, k)
            continue
        assert got is not None and got.shape == (row.S, n) and got.dtype == np.complex64
        e, (s, i), same = CC.view_figures(got, want[k])
        figs.append((e, k, s, i, same))
        zeros += int(np.count_nonzero(want[k] == 0))
        for s in range(row.S):
            if fl[k][s] == 0:
                assert np.array_equal(bits(got[s]), bits(x[s, lo:lo + n])), "%s call %d: stream %d has no flag" % (row.name, k, s)
    e, k, s, i, _ = max(figs)
    print("%s%s: conditioned() against the oracle chain: worst of %d calls x %d streams, per chunk of %d: %.3e (call %d stream %d chunk %d); %d exact zeros, positions %s"
          % (row.name, label, len(figs), row.S, CC.CHUNK, e, k, s, i, zeros, "identical" if all(f[4] for f in figs) else "DIFFER"))
    assert e <= TOL
    assert all(f[4] for f in figs)
    if any(f & 4 for call in fl for f in call):
        assert zeros > 100
    return e


def check_audio_and_spectrum(row, res, want, label="", spec=True):
    """every call's audio per channel, and the spectrum rows of every stream from the run's second row on"""
    ea, ed = [], []
    for k, (wa, ws) in enumerate(want):
        a = res[k]["audio"]
        assert a.shape == (row.C, len(wa[0]))
        ea += [(rel_rms(a[c], wa[c]), k, c) for c in range(row.C)]
        if spec and row.bins:
            s = res[k]["spec"]
            assert s.shape == (row.S,) + ws[0].shape
            ed += [(db_err(s[st][f], ws[st][f]), k, st, f) for st in range(row.S) for f in range(1 if k == 0 else 0, len(ws[st]))]
    print("%s%s: audio worst rel-RMS %.3e (call %d channel %d)%s" % ((row.name, label) + max(ea) + (("; spectrum rows worst %.4f dB (call %d stream %d row %d)" % max(ed)) if ed else "",)))
    assert max(ea)[0] <= TOL
    if ed:
        assert max(ed)[0] <= TOL_DB


def same_bits(res_a, res_b):
    for a, b in zip(res_a, res_b):
        for key in ("audio", "spec", "cond"):
            if (a[key] is None) != (b[key] is None) or (a[key] is not None and not np.array_equal(bits(a[key]), bits(b[key]))):
                return False
    return True


# ------------------------------------------------------------------------------------------------
# the rows that need nothing but the script
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flags", "lists", "frame4096", "switching", "negative_gain", "wfm"])
def test_row_against_the_oracle_chain(gpu_lib, oracle_mod, name):
    """flags: flags 0, 1, 2, 4, 8, 15 with calls of 1, 2, 1, 3 super-frames on a handle made for 3 (n < cap).  lists: 66 streams, the DC
    list {1, 64, 65} then {63, 64, 65}.  frame4096: IQ balance per 4096.  switching: five calls, (15, 13), (0, 1), (15, 15), the setter
    again with the flags on and another gain, (3, 0), at levels x1, x0.5, x2.  negative_gain: iq_gain = -0.97.  wfm: 20 Msps."""
    import pebblesdr_amd as P
    row = CC.ROWS[name]
    want, ms = CC.right(oracle_mod, name)
    if any(m.nb_in for m in ms):
        CC.assert_margin(ms, name)
    runs = []
    for _ in range(2):
        rx = make_rx(P, row)
        try:
            runs.append(run_row(P, row, rx))
        finally:
            rx.close()
    check_view(row, runs[0], want)
    check_audio_and_spectrum(row, runs[0], CC.receiver_oracles(oracle_mod, row))
    again = same_bits(runs[0], runs[1])
    print("%s: the row run twice: same bits %s" % (name, again))
    assert again
    if name == "negative_gain":   # the stage ran: stream 0 (IQ balance alone) is not its input, and its real part changed sign
        c, x = runs[0][0]["cond"][0], CC.row_input(name)[0, :row.sf]
        assert not np.array_equal(c, x) and float(np.sum(c.real * x.real)) < -0.9 * 0.97 * float(np.sum(x.real * x.real))


# ------------------------------------------------------------------------------------------------
# two-stage calls -> conditioned -> cleared -> two-stage again
# ------------------------------------------------------------------------------------------------
def test_two_stage_calls_around_a_conditioned_one(gpu_lib, oracle_mod):
    """a bank without a display transform, three USB channels off one stream, six calls: none, none, flags 15, cleared, none, none.  Calls 0-1
    are bit for bit a twin that was never given a conditioner, and so are calls 4-5, which name the kernels calls 0-1 named; conditioned() is the oracle chain's
    after call 2 and None after every other; every call's audio against the oracle (the route facts: the CPU tier)"""
    import pebblesdr_amd as P
    row = CC.ROWS["two_stage"]
    want, ms = CC.right(oracle_mod, row.name)
    CC.assert_margin(ms, row.name)
    rx, twin = make_rx(P, row), make_rx(P, row)
    try:
        res, plain = run_row(P, row, rx), run_row(P, row, twin, script=False)
    finally:
        rx.close(); twin.close()
    assert [r["cond"] is not None for r in res] == [False, False, True, False, False, False] and all(r["cond"] is None for r in plain)
    same = [bool(np.array_equal(bits(a["audio"]), bits(b["audio"]))) for a, b in zip(res, plain)]
    names = [r["names"] for r in res]
    print("two_stage: audio bit for bit the never-conditioned twin's per call: %s; kernels per call %s" % (same, names))
    # call 3 starts on the decimator history call 2's conditioned samples left; call 4 starts on call 3's unconditioned ones, the twin's
    assert same == [True, True, False, False, True, True]
    assert names[0] == names[1] == names[4] == names[5] == plain[0]["names"] and all(p["names"] == plain[0]["names"] for p in plain)
    assert names[0][3] == "float2" and names[0][2] == "k_fastfir_t128"
    check_view(row, res, want)
    check_audio_and_spectrum(row, res, CC.receiver_oracles(oracle_mod, row))


# ------------------------------------------------------------------------------------------------
# raw input
# ------------------------------------------------------------------------------------------------
def test_raw_calls_are_staged_then_copied_at_the_capacitys_pitch(gpu_lib, oracle_mod):
    """three independent streams of int16 pairs through process_raw_device, flags 15 / 0 / 5, calls of 1, 2, 1 super-frames on a handle made
    for 2: conditioned(), audio and spectrum bit for bit those of a twin handed host_convert(raw) through process; input_route() says staged"""
    import pebblesdr_amd as P
    row = CC.ROWS["raw"]
    want, ms = CC.right(oracle_mod, row.name)
    CC.assert_margin(ms, row.name)
    rx, twin = make_rx(P, row), make_rx(P, row)
    try:
        res, conv = run_row(P, row, rx, raw=True), run_row(P, row, twin)
    finally:
        rx.close(); twin.close()
    routes = [(a["names"][3], b["names"][3]) for a, b in zip(res, conv)]
    same = same_bits(res, conv)
    print("raw: bit for bit the twin handed the converted samples: %s; input routes (raw, float2) per call %s" % (same, routes))
    assert same and routes == [("k_normalize_iq", "float2")] * len(row.calls)
    check_view(row, res, want)
    check_audio_and_spectrum(row, res, CC.receiver_oracles(oracle_mod, row))


# ------------------------------------------------------------------------------------------------
# the test bench's generator
# ------------------------------------------------------------------------------------------------
def test_the_generators_staging_buffer_is_what_is_conditioned(gpu_lib, oracle_mod):
    """noise and a sweep mixed into the input on the device, flags 15, the RAW_IQ tap on: the oracle is fed what the tap returned (the
    margin condition is asserted on that), and conditioned() is its chain's output -- not the caller's input conditioned"""
    import pebblesdr_amd as P
    row = CC.ROWS["generator"]
    a, b, rate, amp = CC.GEN_SWEEP
    taps = []
    rx = make_rx(P, row)
    try:
        rx.set_testbench_sweep(P.sweep(a, b, rate, amplitude=amp, mix=True))
        rx.set_testbench_noise(*CC.GEN_NOISE)
        rx.set_taps([P.TAP_RAW_IQ])
        res = run_row(P, row, rx, after_call=lambda k, r, out: taps.append(r.tap(P.TAP_RAW_IQ)[0].copy()))
    finally:
        rx.close()
    tap = np.concatenate(taps, axis=1)
    x = CC.row_input(row.name)
    assert tap.shape == x.shape and all(r["names"][0].startswith("k_testbench + ") for r in res)
    stand_in = rel_rms(tap[0], CC.oracle_input(row.name)[0])
    print("generator: the RAW_IQ tap against the input plus the restated injection: %.3e; against the input alone: %.3e" % (stand_in, rel_rms(tap[0], x[0])))
    assert stand_in <= TOL and rel_rms(tap[0], x[0]) > 1000 * TOL
    fed = tap.astype(np.complex128)
    want, ms = CC.conditioned(oracle_mod, row, x=fed)
    CC.assert_margin(ms, row.name + " (the tap)")
    for k, (lo, n) in enumerate(CC.call_bounds(row)):   # (the flags-0 check of check_view has nothing to look at: the one stream has 15)
        assert not np.array_equal(res[k]["cond"], tap[:, lo:lo + n])
    check_view(row, res, want)
    check_audio_and_spectrum(row, res, CC.receiver_oracles(oracle_mod, row, x=fed))


# ------------------------------------------------------------------------------------------------
# the spectrum's update gate
# ------------------------------------------------------------------------------------------------
def test_listed_frames_are_read_at_the_copys_pitch(gpu_lib, oracle_mod):
    """set_spectrum_updates(100) on two streams with flags 5, calls of 1 and 2 super-frames on a handle made for 3: the listed frames are
    the timer model's, their rows the oracle spectrum's of the CONDITIONED streams fed the listed frames alone"""
    import pebblesdr_amd as P
    row = CC.ROWS["gated"]
    want, ms = CC.right(oracle_mod, row.name)
    CC.assert_margin(ms, row.name)
    frames = []
    rx = make_rx(P, row)
    try:
        rx.set_spectrum_updates(CC.GATE_UPS)
        res = run_row(P, row, rx, after_call=lambda k, r, out: frames.append(list(r.spectrum_frames())))
    finally:
        rx.close()
    t = GateTimer(row.nf, row.fs)
    t.set_updates(CC.GATE_UPS)
    listed, worst = [], (0.0, 0, 0, 0)
    sp = [oracle_mod.Spectrum(row.bins, row.nf) for _ in range(row.S)]
    raw_sp = [oracle_mod.Spectrum(row.bins, row.nf) for _ in range(row.S)]
    apart, first = 0.0, True
    x = CC.oracle_input(row.name)
    for k, (lo, n) in enumerate(CC.call_bounds(row)):
        assert frames[k] == t.call(n // row.nf) and 2 <= len(frames[k]) < n // row.nf and res[k]["spec"].shape == (row.S, len(frames[k]), row.bins)
        for j, f in enumerate(frames[k]):
            for s in range(row.S):
                r = sp[s].process(want[k][s, f * row.nf:(f + 1) * row.nf])
                u = raw_sp[s].process(x[s, lo + f * row.nf:lo + (f + 1) * row.nf])
                if not first:
                    worst = max(worst, (db_err(res[k]["spec"][s][j], r), k, s, f))
                    apart = max(apart, db_err(u, r))
            first = False
        listed.append(len(frames[k]))
    print("gated: rows per call %s; worst %.4f dB (call %d stream %d frame %d); the unconditioned input's rows lie %.1f dB away" % ((listed,) + worst + (apart,)))
    assert apart > 100 * TOL_DB
    assert worst[0] <= TOL_DB
    check_view(row, res, want)
    check_audio_and_spectrum(row, res, CC.receiver_oracles(oracle_mod, row), spec=False)


# ------------------------------------------------------------------------------------------------
# the zoomed transform, the S-meter and the chain
# ------------------------------------------------------------------------------------------------
def test_downstream_reads_the_conditioned_rows(gpu_lib, oracle_mod):
    """DC removal on, a 0.01 offset under a 0.004 tone, a band-pass across 0 Hz (the design of stream-bank test 6): the S-meter, the zoomed
    spectrum of the decimated frames and the audio are the oracle's for the CONDITIONED stream"""
    import pebblesdr_amd as P
    row = CC.ROWS["downstream"]
    want, _ = CC.right(oracle_mod, row.name)
    sm, zoom = [], []

    def read(k, r, out):
        sm.append(r.signal_strength())
        zoom.append(r.zoom_spectrum())

    rx = make_rx(P, row)
    try:
        rx.enable_signal_strength(True)
        stages = sum(int(np.log2(st)) for _, st in rx.chain())
        res = run_row(P, row, rx, after_call=read)
    finally:
        rx.close()
    check_view(row, res, want)
    oracles = CC.receiver_oracles(oracle_mod, row)
    check_audio_and_spectrum(row, res, oracles)
    sm, zoom = np.concatenate(sm, axis=1)[0], np.concatenate(zoom, axis=1)[0]
    rows = np.concatenate([ws[0] for _, ws in oracles])
    lo, hi = CC.band_of(row)
    fc = CC.mixer_of(row, 0)
    est = lambda db: oracle_mod.fd_estimate(db, row.fs, np.float32(lo), np.float32(hi), fc)
    want_sm = np.array([est(r) for r in rows])
    x = CC.oracle_input(row.name)[0]
    raw_sp = oracle_mod.Spectrum(row.bins, row.nf)
    raw_sm = np.array([est(raw_sp.process(x[i:i + row.nf])) for i in range(0, len(x), row.nf)])
    assert sm.shape == want_sm.shape
    e_sm, apart = float(np.abs(sm[1:] - want_sm[1:]).max()), float(abs(raw_sm[-1, 0] - want_sm[-1, 0]))
    cond = np.concatenate([w[0] for w in want])
    mix = oracle_mod.Mixer(row.fs); mix.set_frequency(fc)
    dec = oracle_mod.Decimator(row.fs, 30000)
    z = np.concatenate([dec.process(mix.process(cond[i:i + 8192])) for i in range(0, len(cond), 8192)]) * 10 ** (2 * stages / 20.0)
    zs = oracle_mod.Spectrum(row.hires, row.nf)
    zref = np.array([zs.process(z[f * row.nf:(f + 1) * row.nf]) for f in range(len(z) // row.nf)])
    assert zoom.shape == zref.shape and len(zref) == sum(row.calls)
    e_zoom = max(db_err(zoom[f], zref[f]) for f in range(1, len(zref)))
    print("downstream: S-meter %.4f dB over %d rows (the unconditioned peak of the last row lies %.1f dB away), zoomed rows %.4f dB over %d"
          % (e_sm, len(sm) - 1, apart, e_zoom, len(zref) - 1))
    assert apart > 10 * TOL_DB
    assert e_sm <= TOL_DB and e_zoom <= TOL_DB


# ------------------------------------------------------------------------------------------------
# the recording ring
# ------------------------------------------------------------------------------------------------
def test_the_ring_records_the_unconditioned_input(gpu_lib, oracle_mod):
    """the recording ring open, flags 15: every block is the truncating PCM16 conversion of the INPUT (WavFile::WriteSamples ahead of the
    conditioners), which is not that of conditioned()"""
    import pebblesdr_amd as P
    row = CC.ROWS["recording"]
    want, ms = CC.right(oracle_mod, row.name)
    CC.assert_margin(ms, row.name)
    blocks = []

    def read(k, r, out):
        blk = r.record_next(True)
        assert blk is not None and (blk[0], blk[1]) == (k, 0)
        blocks.append(blk[2].copy())
        r.record_release(blk[0])

    rx = make_rx(P, row)
    try:
        rx.record_open(4)
        res = run_row(P, row, rx, after_call=read)
    finally:
        rx.close()
    x = CC.row_input(row.name)
    differ = []
    for k, (lo, n) in enumerate(CC.call_bounds(row)):
        assert blocks[k].dtype == np.int16 and blocks[k].shape == (1, n, 2)
        assert np.array_equal(blocks[k][0], P.iq_record_convert(x[0, lo:lo + n])), "call %d: the block is not the input" % k
        differ.append(int(np.count_nonzero(blocks[k][0] != P.iq_record_convert(res[k]["cond"][0]))))
    print("recording: blocks equal the input's PCM16; components that differ from conditioned()'s PCM16 per call: %s" % differ)
    assert all(d > 1000 for d in differ)
    check_view(row, res, want)
    check_audio_and_spectrum(row, res, CC.receiver_oracles(oracle_mod, row))


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(gpu_lib, oracle_mod):
    """every refusal is followed by a good call of one super-frame, checked against the oracle chain: the stream went on where it was.
    Flags 3 (DC removal and IQ balance: no decision, no margin condition), gain 1.02, phase 0.03 throughout: a refused setter changed nothing"""
    import pebblesdr_amd as P
    L = P.load_library()
    row = CC.ROWS["switching"]
    x = np.tile(CC.row_input(row.name)[:1], (1, 3))   # fifteen super-frames of one stream
    rx = P.ReceiverBank(row.fs, 1, True, False, row.bins, max_superframes=2)
    rx.set_mode(0, P.DM_USB); rx.set_mixer(0, CC.mixer_of(row, 0)); rx.set_bandpass(0, *CC.band_of(row))
    m = CC.Model(oracle_mod, row.fs, row.nf)
    at, sf, figs = [0], row.sf, []

    def good(what):
        seg = x[:, at[0]:at[0] + sf]
        a, _ = rx.process(seg)
        got, want = rx.conditioned(), m.call(seg[0])
        assert got is not None and got.shape == (1, sf) and np.isfinite(a).all()
        figs.append((CC.view_figures(got, want[None, :])[0], what))
        at[0] += sf

    def refused(code, fn, *args):
        with pytest.raises(P.PebbleGpuError) as e:
            fn(*args)
        assert e.value.code == code, (e.value.code, code)

    try:
        assert rx.conditioned() is None                       # before any call
        rx.process(x[:, :sf]); at[0] += sf
        assert rx.conditioned() is None                       # a call with no flag
        rx.set_conditioners(0, 3, 1.02, 0.03); m.set(3, 1.02, 0.03)
        good("the first conditioned call")
        buf = P.DeviceBuffer.from_array(np.ascontiguousarray(x[:, :3 * sf]), 0)
        try:
            refused(E_SIZE, rx.process_device, buf.ptr, sf + 100)     # n % nf != 0
            assert rx.conditioned() is None                       # a refused call conditioned nothing
            good("n % nf != 0")
            refused(E_SIZE, rx.process_device, buf.ptr, 3 * sf)       # n > cap
            assert rx.conditioned() is None
            good("n > cap")
        finally:
            buf.free()
        for what, args in (("stream >= S", (1, 3, 1.02, 0.03)), ("flags 16", (0, 16, 1.02, 0.03)), ("flags -1", (0, -1, 1.02, 0.03)),
                           ("NaN gain", (0, 3, float("nan"), 0.03)), ("inf gain", (0, 3, float("inf"), 0.03)),
                           ("NaN phase", (0, 3, 1.02, float("nan"))), ("-inf phase", (0, 3, 1.02, float("-inf")))):
            assert L.pebblegpu_set_conditioners(rx.h, *args) == E_INVALID, what
            good(what)
        refused(E_UNSUPPORTED, rx.process_iq, x[0, :row.nf].astype(np.complex128))
        assert rx.conditioned() is None
        good("process_iq")
        rx.set_conditioners(0, 0)
        rx.process(x[:, at[0]:at[0] + sf])
        assert rx.conditioned() is None                       # cleared again
    finally:
        rx.close()
    print("refusals: conditioned() of the good call behind each, worst chunk of 512: %s" % ["%s %.2e" % (w, e) for e, w in figs])
    assert all(np.isfinite(e) and e <= TOL for e, _ in figs)
