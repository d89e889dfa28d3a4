"""The window table of the receivers' S-meter (SignalStrength::fdEstimate, application/signalstrength.cpp:287-380), shared by
tests/test_receiver_smeter_host.py, tests/test_receiver_smeter_gpu.py and the "fdestimate_*" cases of tests/reference_cases.py.

A row is (name, sample rate, bins, bp_lo, bp_hi, mixer, class).  windows() restates signalstrength.cpp:308-335 in plain integers --
written from the reference's text, not from the device's strength_windows (params.h) -- and check_class() asserts from its result
that the row reaches the edge its class names, so the table proves that each edge is reached:

  binWidth = rate / bins                      both integers: the quotient truncates, then widens to double
  mixerBin = qBound(0, int(bins / 2 + mixer / binWidth), bins)
  lo, hi   = qBound(0, int(mixerBin + bp / binWidth), bins)       (bp is a float; int() truncates towards zero)
  bpBins   = hi - lo
  nlo, nhi = qBound(0, lo - bpBins, bins), qBound(0, hi + bpBins, bins)
  for i in 0 .. bins - 1: skip i < nlo; lo <= i <= hi is in band, else nlo <= i <= nhi is noise; leave after i >= nhi

A window centred in the spectrum visits nhi - nlo + 1 = 3 bpBins + 1 bins -- 61, 64, 67 ..., never 65 -- so the 65-bin window (one
bin more than a wave's stride) is a clipped one: clipped_low_65.

What the values must be, where the class makes them a bound (expected()): avg of a window with bpBins == 0 and a bin in band is
x / 0 = +inf -> 0 dB; 0 / 0 (no noise bin, or no bin at all) is NaN, which the reference's qBound returns as its LOWER bound: -120 dB
for peak, avg and floor, 0 for snr.  Nothing is ever NaN.
"""
import numpy as np

from tests.signals import lcg_uniform

USB, LSB, CW, WFM = (300.0, 3000.0), (-3000.0, -300.0), (-1250.0, -250.0), (-100000.0, 100000.0)

# (name, sample rate, bins, bp_lo, bp_hi, mixer, class)
ROWS = [
    # centred: the loop visits 10, 61, 64, 67 and 601 bins (k_signal_strength strides by 64 lanes)
    ("usb_centred", 2048000, 2048, USB[0], USB[1], 100e3, "centred"),
    ("centred_61", 2048000, 2048, -10000.0, 10000.0, -300e3, "centred"),
    ("centred_64", 2048000, 2048, -10000.0, 11000.0, 250e3, "centred"),
    ("centred_67", 2048000, 2048, -11000.0, 11000.0, 0.0, "centred"),
    ("wfm_centred_601", 2048000, 2048, WFM[0], WFM[1], 200e3, "centred"),
    ("usb_centred_4096", 2048000, 4096, USB[0], USB[1], -412345.0, "centred"),
    # clipped, with part of the lower noise window left: 65 bins, one more than a wave's stride
    ("clipped_low_65", 2048000, 2048, 300.0, 27000.0, -1014000.0, "clipped_low_partial"),
    # clipped: the noise window exists on one side only
    ("lsb_clipped_low", 2048000, 2048, LSB[0], LSB[1], -1021000.0, "clipped_low"),
    ("usb_clipped_high", 2048000, 2048, USB[0], USB[1], 1020000.0, "clipped_high"),
    ("wfm_clipped_high", 2048000, 2048, WFM[0], WFM[1], 950e3, "clipped_high"),
    ("wfm_250k_clipped_both", 250000, 2048, WFM[0], WFM[1], 0.0, "clipped_both"),
    # nhi == bins: noise above the band-pass up to the last bin, where the loop ends without reaching nhi
    ("usb_nhi_bins", 2048000, 2048, USB[0], USB[1], 1018000.0, "nhi_bins"),
    # bpBins == 0 with one bin in band
    ("lsb_lower_edge_one_bin", 2048000, 2048, LSB[0], LSB[1], -1023500.0, "bp0_one_bin"),
    ("narrow_one_bin", 2048000, 2048, 100.0, 200.0, 0.0, "bp0_one_bin"),
    ("cw_one_bin", 2048000, 2048, -1000.0, -500.0, 77e3, "bp0_one_bin"),
    # bpBins == 0 with no bin: the mixer's bin clamped to `bins`
    ("mixer_at_half_rate", 2048000, 2048, USB[0], USB[1], 1024000.0, "bp0_no_bin"),
    ("mixer_beyond_half_rate", 2048000, 2048, USB[0], USB[1], 1.2e6, "bp0_no_bin"),
    ("mixer_beyond_half_rate_4096", 2048000, 4096, USB[0], USB[1], 1.2e6, "bp0_no_bin"),
    # every bin in band: no noise bin (WFM on a 192 kHz device)
    ("wfm_192k_all_in_band", 192000, 2048, WFM[0], WFM[1], 0.0, "all_in_band"),
    # negative frequencies: int() truncates towards zero, which moves a window below the mixer DOWN a bin
    ("lsb_negative", 2048000, 2048, LSB[0], LSB[1], 100e3, "negative"),
    ("cw_negative_4096", 2048000, 4096, CW[0], CW[1], -300e3, "negative"),
    # an integer bin width that truncates: 48000 / 2048 = 23 (23.4375), 2400000 / 4096 = 585 (585.9375)
    ("usb_48k_truncating", 48000, 2048, USB[0], USB[1], 5000.0, "truncating"),
    ("usb_2m4_truncating_4096", 2400000, 4096, USB[0], USB[1], 700e3, "truncating"),
    # lo >= hi: CFastFIR stores a refused pair before its check (fastfir.cpp:200-203) and fdEstimate reads the stored pair
    ("refused_inverted", 2048000, 2048, 3000.0, 300.0, 100e3, "inverted"),
    ("refused_inverted_at_edge", 2048000, 2048, 3000.0, -3000.0, -1022000.0, "inverted"),
]
CLASSES = ["centred", "clipped_low_partial", "clipped_low", "clipped_high", "clipped_both", "nhi_bins", "bp0_one_bin", "bp0_no_bin", "all_in_band", "negative",
           "truncating", "inverted"]
NAMES = [r[0] for r in ROWS]


def row(name):
    return next(r for r in ROWS if r[0] == name)


def _qbound(lo, v, hi):
    return max(lo, min(hi, v))


def windows(rate, bins, bp_lo, bp_hi, mixer, exact_width=False):
    """signalstrength.cpp:308-356 -> dict(nlo, lo, hi, nhi, bp_bins, in_band, noise_below, noise_above, visited); exact_width: what an
    untruncated bin width would give (only to show that a "truncating" row tells the two apart)"""
    bin_width = float(rate) / bins if exact_width else float(int(rate) // int(bins))
    assert bin_width > 0
    mixer_bin = _qbound(0, int(bins // 2 + float(mixer) / bin_width), bins)
    lo = _qbound(0, int(mixer_bin + float(np.float32(bp_lo)) / bin_width), bins)
    hi = _qbound(0, int(mixer_bin + float(np.float32(bp_hi)) / bin_width), bins)
    bp_bins = hi - lo
    nlo, nhi = _qbound(0, lo - bp_bins, bins), _qbound(0, hi + bp_bins, bins)
    in_band = below = above = visited = 0
    for i in range(bins):
        if i < nlo:
            continue
        visited += 1
        if lo <= i <= hi:
            in_band += 1
        elif nlo <= i <= nhi:
            if i < lo:
                below += 1
            else:
                above += 1
        if i >= nhi:
            break
    return dict(mixer_bin=mixer_bin, nlo=nlo, lo=lo, hi=hi, nhi=nhi, bp_bins=bp_bins, in_band=in_band, noise_below=below, noise_above=above,
                noise=below + above, visited=visited)


def check_class(r):
    """asserts that the row reaches the edge its class names; -> its windows"""
    name, rate, bins, lo, hi, mixer, cls = r
    w = windows(rate, bins, lo, hi, mixer)
    inside = 0 < w["nlo"] and w["nhi"] < bins - 1
    if cls == "centred":
        assert inside and w["bp_bins"] > 0 and w["visited"] == 3 * w["bp_bins"] + 1 and w["noise_below"] == w["noise_above"] == w["bp_bins"], (name, w)
    elif cls in ("clipped_low", "clipped_low_partial"):
        assert w["nlo"] == 0 and w["lo"] - w["bp_bins"] < 0 and w["bp_bins"] > 0 and w["nhi"] < bins - 1 and w["noise_above"] == w["bp_bins"], (name, w)
        assert w["noise_below"] == 0 if cls == "clipped_low" else 0 < w["noise_below"] < w["bp_bins"], (name, w)
    elif cls == "clipped_high":
        assert w["nhi"] == bins and w["hi"] >= bins - 1 and w["nlo"] > 0 and w["bp_bins"] > 0, (name, w)
        assert w["noise_above"] == 0 and w["noise_below"] == w["bp_bins"], (name, w)
    elif cls == "clipped_both":
        assert w["nlo"] == 0 and w["nhi"] == bins and 0 < w["noise_below"] < w["bp_bins"] and 0 < w["noise_above"] < w["bp_bins"], (name, w)
    elif cls == "nhi_bins":
        assert w["nhi"] == bins and w["hi"] < bins - 1 and 0 < w["noise_above"] == bins - 1 - w["hi"] and w["nlo"] > 0, (name, w)
    elif cls == "bp0_one_bin":
        assert w["bp_bins"] == 0 and w["in_band"] == 1 and w["noise"] == 0 and w["visited"] == 1, (name, w)
    elif cls == "bp0_no_bin":
        assert w["mixer_bin"] == bins and w["bp_bins"] == 0 and w["nlo"] == bins and w["visited"] == 0, (name, w)
    elif cls == "all_in_band":
        assert (w["lo"], w["hi"], w["in_band"], w["noise"]) == (0, bins, bins, 0), (name, w)
    elif cls == "negative":
        assert inside and hi < 0 and w["hi"] < w["mixer_bin"] and w["bp_bins"] > 0 and w["noise_below"] == w["noise_above"] == w["bp_bins"], (name, w)
    elif cls == "truncating":
        exact = windows(rate, bins, lo, hi, mixer, exact_width=True)
        assert rate % bins != 0 and inside and (w["lo"], w["hi"]) != (exact["lo"], exact["hi"]), (name, w, exact)
    elif cls == "inverted":
        assert lo >= hi and w["bp_bins"] < 0 and w["in_band"] == 0 and w["noise"] == 0, (name, w)
    else:
        raise AssertionError("unknown class %r" % cls)
    if name.endswith(("_61", "_64", "_65", "_67", "_601")):
        assert w["visited"] == int(name.rsplit("_", 1)[1]), (name, w)
    return w


def expected(cls):
    """{index of (peak, avg, snr, floor): the exact value the class forces}"""
    return {"bp0_one_bin": {1: 0.0, 2: 0.0, 3: -120.0}, "bp0_no_bin": {0: -120.0, 1: -120.0, 2: 0.0, 3: -120.0},
            "all_in_band": {2: 0.0, 3: -120.0}, "inverted": {0: -120.0, 1: -120.0, 2: 0.0, 3: -120.0}}.get(cls, {})


DEGENERATE = ("bp0_one_bin", "bp0_no_bin", "all_in_band", "inverted")


def db_row(bins, seed):
    """float64 [bins] dB: a ragged floor near -100 dB (6 dB of ripple), a -30 dB bin every 97 bins (so that every window of a few bins
    or more holds one, and the one-bin windows mostly do not) and -55 dB shoulders; every value is a float32"""
    sp = -100.0 + 6.0 * (lcg_uniform(bins, seed) - 0.5)
    sp[5::97] = -30.0
    sp[6::97] = -55.0 - 3.0 * lcg_uniform(len(sp[6::97]), seed + 1)
    sp[0], sp[bins - 1] = -98.25, -97.5
    return sp.astype(np.float32).astype(np.float64)


def row_spectrum(name):
    """the dB row the host tier and the reference pins feed row `name`"""
    r = row(name)
    return db_row(r[2], 7000 + NAMES.index(name))
