"""Restatement of the reference's test-bench generator (pebblelib/nco.cpp), plain numpy, for the generator parity tests.

  SerialSweep   NCO::initSweep + NCO::genSweep (nco.cpp:119-212) as the reference runs them: the frequency, the phase and the pulse timer
                are accumulated by sequential double additions (numpy's cumsum adds in order, one rounding per step, exactly the loop's
                `+=`), the phase is folded by fmod once per genSweep call.
  pulse_numbers the pulse timer's period and width in samples.
  noise_*       NCO::genNoise (nco.cpp:87-116) with rand() replaced by the library's counter-based draw (the reference's rand() is
                libc-specific and unseeded: there is nothing to keep parity with).  This file DEFINES that draw; the device must reproduce
                its integers.
"""
import numpy as np

TWOPI = 6.28318530717958647692528676656  # pebblelib/cpx.h:17
SINGLE, REPEAT, REPEAT_REVERSE = 0, 1, 2  # NCO::SweepType, nco.h:52


def leg_length(fs, start, stop, rate):
    """samples from the start frequency until the SERIAL frequency reaches the stop frequency (0: never), and the fractional part of
    |stop - start| / (rate / fs): near 0 or 1 the serial sum's rounding decides the last step and a closed form may disagree by one"""
    inc = rate / fs
    if not inc > 0:
        return 0, 0.5
    f, n = start, 0
    up = start < stop
    span = abs(stop - start) / inc
    # serial, in blocks
    while True:
        seq = np.cumsum(np.concatenate(([f], np.full(1 << 16, inc if up else -inc))))
        hit = seq[1:] >= stop if up else seq[1:] <= stop
        if hit.any():
            return n + int(np.argmax(hit)) + 1, span - np.floor(span)
        n += 1 << 16
        f = seq[-1]


def pulse_numbers(fs, width, period):
    """(period, first_off): the timer is reset by its increment number `period` (the first that leaves it above the period); increment
    `first_off` is the first that leaves it above the width.  Sample i of a period sees the timer after increment i + 1 (nco.cpp:151-155)."""
    dt = 1.0 / fs
    t, n, first_off = 0.0, 0, 0
    while True:
        seq = np.cumsum(np.concatenate(([t], np.full(1 << 20, dt))))[1:]
        if not first_off:
            w = seq > width
            if w.any():
                first_off = n + int(np.argmax(w)) + 1
        p = seq > period
        if p.any():
            return n + int(np.argmax(p)) + 1, first_off
        n += 1 << 20
        t = seq[-1]


class SerialSweep:
    """NCO with initSweep called; gen(n) is one NCO::genSweep(_in, n, amp, mix) call and returns what it adds to (or puts in place of) _in"""

    def __init__(self, fs, start, stop, rate, pulse_width=0.0, pulse_period=0.0, sweep_type=REPEAT):
        self.fs = float(fs)
        self.start, self.stop, self.f = float(start), float(stop), float(start)  # nco.cpp:122-124
        self.acc = 0.0
        self.inc = rate / self.fs            # m_sweepRateInc
        self.norm = TWOPI / self.fs          # m_sweepFreqNorm
        self.width, self.period, self.timer = float(pulse_width), float(pulse_period), 0.0
        self.type = sweep_type
        self.up = self.start < self.stop     # nco.cpp:136
        self.resets = []                     # absolute sample numbers after which the frequency was set back / held / reversed
        self.n = 0

    def _amp(self, n, amp):
        a = np.full(n, float(amp))
        if not self.width > 0.0:             # nco.cpp:149
            return a
        dt = 1.0 / self.fs
        i = 0
        while i < n:
            seq = np.cumsum(np.concatenate(([self.timer], np.full(n - i, dt))))[1:]
            over = seq > self.period
            m = int(np.argmax(over)) + 1 if over.any() else n - i
            t = seq[:m].copy()
            if over.any():
                t[m - 1] = 0.0               # nco.cpp:152-153
            a[i:i + m][t > self.width] = 0.0  # nco.cpp:154-155
            self.timer = float(t[m - 1])
            i += m
        return a

    def gen(self, n, amp=1.0):
        a = self._amp(n, amp)
        ph = np.empty(n)
        i = 0
        while i < n:
            m = n - i
            seg, reached = m, False
            if self.inc > 0:                 # nco.cpp:181
                fseq = np.cumsum(np.concatenate(([self.f], np.full(m, self.inc if self.up else -self.inc))))
                hit = fseq[1:] >= self.stop if self.up else fseq[1:] <= self.stop  # nco.cpp:188-189
                if hit.any():
                    seg, reached = int(np.argmax(hit)) + 1, True
            else:
                fseq = np.full(m + 1, self.f)
            accs = np.cumsum(np.concatenate(([self.acc], fseq[:seg] * self.norm)))  # nco.cpp:180
            ph[i:i + seg] = accs[:seg]
            self.acc = float(accs[seg])
            self.f = float(fseq[seg])
            i += seg
            if reached:
                self.resets.append(self.n + i)
                if self.type == SINGLE:
                    self.inc = 0.0           # nco.cpp:193
                elif self.type == REPEAT:
                    self.f = self.start      # nco.cpp:196
                else:                        # nco.cpp:199-204
                    self.start, self.stop = self.stop, self.start
                    self.up = not self.up
                    self.f = self.start
        self.acc = float(np.fmod(self.acc, TWOPI))  # nco.cpp:211
        self.n += n
        return a * np.cos(ph) + 1j * (a * np.sin(ph))


def serial_sweep(fs, n, frame, amp=1.0, **kw):
    """n samples in genSweep calls of `frame` samples -> (complex128 [n], the SerialSweep)"""
    s = SerialSweep(fs, **kw)
    out = np.empty(n, dtype=np.complex128)
    for i in range(0, n, frame):
        m = min(frame, n - i)
        out[i:i + m] = s.gen(m, amp)
    return out, s


# ---- noise ----
NOISE_ATTEMPTS = 32     # per sample at most; a sample whose attempts all fail gets no noise
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def _mix64(z):
    """splitmix64's finaliser on uint64 arrays (wrapping arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def noise_draw(seed, stream, sample, attempt):
    """the two 31-bit integers of one attempt: a pure function of (seed, stream, absolute sample number, attempt).  sample: uint64 array"""
    with np.errstate(over="ignore"):
        key = _mix64(np.uint64(seed) + _GOLDEN * np.uint64(stream + 1))
        h = _mix64(_mix64(key ^ np.asarray(sample, dtype=np.uint64)) + _GOLDEN * np.uint64(attempt + 1))
    return (h >> np.uint64(33)).astype(np.uint32), ((h >> np.uint64(1)) & np.uint64(0x7FFFFFFF)).astype(np.uint32)


def noise(seed, stream, first, n):
    """NCO::genNoise's samples first .. first + n - 1 at amplitude 1 -> (complex128 [n], accepted draws uint32 [n, 2], accepted attempt uint8 [n])"""
    idx = np.arange(first, first + n, dtype=np.uint64)
    out = np.zeros(n, dtype=np.complex128)
    r = np.zeros((n, 2), dtype=np.uint32)
    att = np.full(n, NOISE_ATTEMPTS, dtype=np.uint8)
    todo = np.arange(n)
    for a in range(NOISE_ATTEMPTS):
        if not todo.size:
            break
        r1, r2 = noise_draw(seed, stream, idx[todo], a)
        u1 = 1.0 - 2.0 * r1.astype(np.float64) / 2147483647.0   # nco.cpp:99-100, RAND_MAX = 2^31 - 1
        u2 = 1.0 - 2.0 * r2.astype(np.float64) / 2147483647.0
        s = u1 * u1 + u2 * u2
        ok = ~((s >= 1.0) | (s == 0.0))                         # nco.cpp:103
        k = todo[ok]
        rad = np.sqrt(-2.0 * np.log(s[ok]) / s[ok])             # nco.cpp:105
        out[k] = u1[ok] * rad + 1j * (u2[ok] * rad)
        r[k, 0], r[k, 1], att[k] = r1[ok], r2[ok], a
        todo = todo[~ok]
    return out, r, att
