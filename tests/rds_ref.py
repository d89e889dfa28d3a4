"""A plain NumPy fp64 model of the RDS branch of Demod_WFM::processDataStereo as far as m_RdsData and the bit slicer
(application/demod/demod_wfm.cpp:258-263, 268, 296-353), every stage carrying its state from call to call the way a streaming
implementation has to: discriminator, the 61-tap Hilbert pair, CDownConvert's oscillator and product, each decimate-by-2 stage as an
np.convolve, the 2400 Hz low-pass, the PLL, the matched filter, the bit-rate resonator and the slope detector.  The taps and constants
come from csrc/design.cpp (tests/rds_cases.py: rds_design).  tests/test_rds_geometry_host.py holds it to oracle.DemodWFM.

`faults` switches on what a device implementation can plausibly get wrong (FAULTS); the host tier shows that each of them misses the
bar on every row's script, with the metric the device tier uses.

The oscillator: the reference turns a phasor by (cos inc, sin inc) per sample and pulls its length back with 1.95 - |z|^2.  What that
recurrence turns by is the angle of the ROUNDED pair, not inc: after 5e5 samples the two are 1e-10 rad apart, and m_RdsData -- the
imaginary part of a signal whose real part can be hundreds of times larger -- shows it at 5e-8 (the figure the device, which uses
the closed form (n + 1) inc, measures against the oracle).  The model's own agreement has to be a thousand times better than the
device's bar, so it takes the angle of the rounded pair, in extended precision, times the sample count; the length is the table of
the recurrence's first 1024 values, converged to sqrt(0.95) long before its end."""
import numpy as np

FAULTS = (
    "discrim_prev",      # the discriminator's previous sample is not carried: every call starts from (0, 0)
    "hilbert_hist",      # the Hilbert pair's look-back is zeroed at a call start
    "osc_frozen",        # the oscillator's sample count is not advanced: every call starts at sample 0
    "osc_wrong_n",       # ... is advanced by the call's length behind the chain instead of in front of it
    "stage_hist",        # stage `fault_stage` starts every call with an empty delay line
    "lp_hist",           # the low-pass starts every call with an empty delay line
    "short_headroom",    # a call shorter than a look-back leaves only itself (zeros in front) as the next call's history
    "pll_phase",         # the PLL's phase is reset per call
    "pll_freq",          # the PLL's frequency is reset per call
    "matched_hist",      # the matched filter's look-back is lost
    "slicer_state",      # resonator, slope and last-bit state are lost at a call border (judged by the bits)
    "pll_fold_block",    # the PLL's phase is folded every 7 samples, not per call (must stay inside the bar)
)


def _fir_hist(x_hist, x, h, hist_len, short_headroom):
    """y[i] = sum_k h[k] x[i - k] over [history | call]; -> (y of the call, the next history)"""
    ext = np.concatenate([x_hist, x])
    y = np.convolve(ext, h)[hist_len:hist_len + len(x)]
    if short_headroom and len(x) < hist_len:
        nxt = np.concatenate([np.zeros(hist_len - len(x), dtype=ext.dtype), x])
    else:
        nxt = ext[len(ext) - hist_len:]
    return y, nxt


class RdsModel:
    def __init__(self, des, faults=(), fault_stage=0):
        assert all(f in FAULTS for f in faults), faults
        self.d, self.f, self.fault_stage = des, frozenset(faults), fault_stage
        self.prev = 0j
        self.raw_hist = np.zeros(60)
        self.n0 = 0
        self.st_hist = [np.zeros(len(h) - 1, dtype=np.complex128) for h in des.stage_h]
        self.lp_hist = np.zeros(len(des.lp) - 1, dtype=np.complex128)
        self.ph = self.fq = 0.0
        self.mag_hist = np.zeros(len(des.matched) - 1)
        self.w1 = self.w2 = self.last_sync = self.last_slope = self.last_data = 0.0
        self.last_bit = 0
        self.bits = []
        # the angle the reference's recurrence turns by per sample (see the module's docstring)
        inc = 6.28318530717958647692528676656 * (57000.0 / des.rate)   # po_downconvert_set_frequency: TWOPI * freq / rate
        self.inc_eff = np.arctan2(np.longdouble(np.sin(inc)), np.longdouble(np.cos(inc)))

    def _oscillator(self, n):
        m = self.n0 + np.arange(n)
        ph = (m + 1).astype(np.longdouble) * self.inc_eff
        a = self.d.amp[np.minimum(m, len(self.d.amp) - 1)]
        return a * (np.cos(ph).astype(np.float64) + 1j * np.sin(ph).astype(np.float64))

    def process(self, x):
        """one processDataStereo call -> m_RdsData of it; the bits it hands to processNewRdsBit are appended to self.bits"""
        d, f = self.d, self.f
        x = np.asarray(x, dtype=np.complex128)
        n = len(x)
        short = "short_headroom" in f
        # :258-263
        xp = np.concatenate([[0j if "discrim_prev" in f else self.prev], x[:-1]])
        raw = 0.25 * np.arctan2(xp.real * x.imag - x.real * xp.imag, xp.real * x.real + xp.imag * x.imag)
        self.prev = x[-1]
        # :268, CFir real in / complex out
        rh = np.zeros(60) if "hilbert_hist" in f else self.raw_hist
        yi, nxt = _fir_hist(rh, raw, d.hilb_i, 60, short)
        yq, _ = _fir_hist(rh, raw, d.hilb_q, 60, short)
        self.raw_hist = nxt
        # CDownConvert::ProcessData: oscillator, product, the stages
        if "osc_frozen" in f:
            self.n0 = 0
        z = (yi + 1j * yq) * self._oscillator(n)
        self.n0 += (n >> len(d.stage_h)) if "osc_wrong_n" in f else n
        for j, h in enumerate(d.stage_h):
            T = len(h)
            hist = self.st_hist[j]
            if "stage_hist" in f and j == self.fault_stage:
                hist = np.zeros(T - 1, dtype=np.complex128)
            ext = np.concatenate([hist, z])
            # output m from ext[2 m .. 2 m + T - 1], h oldest sample first
            full = np.convolve(ext, h[::-1])
            self.st_hist[j] = ext[len(ext) - (T - 1):]
            z = full[T - 1:T - 1 + len(z):2]
        # :301
        lh = np.zeros(len(d.lp) - 1, dtype=np.complex128) if "lp_hist" in f else self.lp_hist
        z, self.lp_hist = _fir_hist(lh, z, d.lp, len(d.lp) - 1, short)
        # processRdsPll, :542-569
        if "pll_phase" in f:
            self.ph = 0.0
        if "pll_freq" in f:
            self.fq = 0.0
        mag = np.empty(len(z))
        ph, fq = self.ph, self.fq
        two_pi = 6.28318530717958647692528676656
        zr, zi = z.real.tolist(), z.imag.tolist()
        import math
        for i in range(len(z)):
            sn, cs = math.sin(ph), math.cos(ph)
            tr = cs * zr[i] - sn * zi[i]
            ti = cs * zi[i] + sn * zr[i]
            err = -_arctan2(ti, tr)
            fq += d.beta * err
            if fq > d.nco_hi:
                fq = d.nco_hi
            elif fq < d.nco_lo:
                fq = d.nco_lo
            ph += fq + d.alpha * err
            mag[i] = ti
            if "pll_fold_block" in f and i % 7 == 6:
                ph = math.fmod(ph, two_pi)
        self.ph, self.fq = math.fmod(ph, two_pi), fq
        # m_RdsMatchedFilter
        mh = np.zeros(len(d.matched) - 1) if "matched_hist" in f else self.mag_hist
        data, self.mag_hist = _fir_hist(mh, mag, d.matched, len(d.matched) - 1, short)
        # :312-353
        if "slicer_state" in f:
            self.w1 = self.w2 = self.last_sync = self.last_slope = self.last_data = 0.0
            self.last_bit = 0
        b0, b1, b2, a1, a2 = d.bitsync
        w1, w2, last_sync, last_slope, last_data, last_bit = self.w1, self.w2, self.last_sync, self.last_slope, self.last_data, self.last_bit
        for v in data.tolist():
            w0 = v * v - a1 * w1 - a2 * w2
            sync = b0 * w0 + b1 * w1 + b2 * w2
            w2, w1 = w1, w0
            slope = sync - last_sync
            last_sync = sync
            if slope < 0.0 and last_slope * slope < 0.0:
                bit = 1 if last_data >= 0 else 0
                self.bits.append(bit ^ last_bit)
                last_bit = bit
            last_data = v
            last_slope = slope
        self.w1, self.w2, self.last_sync, self.last_slope, self.last_data, self.last_bit = w1, w2, last_sync, last_slope, last_data, last_bit
        return data


def _arctan2(y, x):
    """Demod_WFM::arctan2, :792-821, constants as written"""
    two_pi, pi = 6.28318530717958647692528676656, 3.14159265358979323846
    if x == 0.0:
        return two_pi if y > 0.0 else (0.0 if y == 0.0 else -two_pi)
    z = y / x
    if abs(z) < 1.0:
        ang = z / (1.0 + 0.2854 * z * z)
        if x < 0.0:
            return ang - pi if y < 0.0 else ang + pi
        return ang
    ang = two_pi - z / (z * z + 0.2854)
    return ang - pi if y < 0.0 else ang


def run_model(des, x, script_offsets, faults=(), fault_stage=0):
    """-> ([m_RdsData per call], bits)"""
    m = RdsModel(des, faults, fault_stage)
    data = [m.process(x[o:o + n]) for o, n in script_offsets]
    return data, np.array(m.bits, dtype=np.uint8)
