"""SpectrumWidget::recalcScale (application/spectrumwidget.cpp:693-734) restated: the reference for pebblegpu_auto_scale_row, k_scale_stats
and the display rings' auto-scale.  recalcScale lives in a Qt widget and cannot be built into oracle/_ref, so this is a line-by-line
restatement: a serial fp64 loop with math.pow / math.log10 / int(), in the reference's order.

The library's spectrum rows are float; each value is widened to double first (the reference's getUnprocessed() is double already).
"""
import math

MIN_DB = -120.0          # DB::minDb (pebblelib/db.cpp)
MIN_DB_LIMIT = -70       # m_minDbScaleLimit, spectrumwidget.h:154
MAX_DB_LIMIT = -50       # m_maxDbScaleLimit, spectrumwidget.h:153
EDGE = 1e-6              # a quantity closer than this to an integer may legitimately truncate either way on another adder / libm


def power_to_db(p):
    """DB::powerTodB, db.h:78-82"""
    return MIN_DB if p == 0 else 10 * math.log10(p)


def c_div5(v):
    """(v / 5) * 5 in C int arithmetic: the division truncates toward zero (spectrumwidget.cpp:716, :724)"""
    q = abs(v) // 5
    return (q if v >= 0 else -q) * 5


def q_bound(lo, v, hi):
    """qBound(lo, v, hi) = max(lo, min(hi, v))"""
    return max(lo, min(hi, v))


def finish_min(q):
    """spectrumwidget.cpp:715-717 from the unrounded powerTodB(avg) - 10: int() truncates as the double -> int conversion does"""
    return q_bound(-120, c_div5(int(q)), MIN_DB_LIMIT)


def finish_max(q):
    """spectrumwidget.cpp:723-725 from the unrounded powerTodB(peak) + 10"""
    return q_bound(MAX_DB_LIMIT, c_div5(int(q)), 0)


def scale_row(db):
    """one row of dB values -> dict(max_db, min_db, avg_power, peak_power, q_avg, q_peak); q_*: the unrounded quantities the ints come from"""
    total = 0.0
    peak = 0.0                                    # double peakPwr = 0, :702
    n = 0
    for v in db:
        pwr = math.pow(10, float(v) / 10.0)       # DB::dBToPower, db.h:72-75 (:706)
        total += pwr                              # :707
        if pwr > peak:                            # :708-709
            peak = pwr
        n += 1
    avg = total / n                               # :711
    q_avg = power_to_db(avg) - 10                 # :715
    q_peak = power_to_db(peak) + 10               # :723
    return dict(max_db=finish_max(q_peak), min_db=finish_min(q_avg), avg_power=avg, peak_power=peak, q_avg=q_avg, q_peak=q_peak)


def is_safe(r):
    """The condition on a test's inputs, from the restatement alone: both quantities farther than EDGE from an integer -- or, for a row
    clipped to the bounds (all -120 dB, a 0 dB peak), both candidates clamping to the same limit."""
    for q, fin, limits in ((r["q_avg"], finish_min, (-120, MIN_DB_LIMIT)), (r["q_peak"], finish_max, (MAX_DB_LIMIT, 0))):
        if abs(q - round(q)) > EDGE:
            continue
        lo, hi = fin(q - 2 * EDGE), fin(q + 2 * EDGE)
        if not (lo == hi and lo in limits):
            return False
    return True


def scale_rows(rows):
    """rows [..., bins] (numpy) -> a list of scale_row results in C order, every one asserted safe: NO row is excluded"""
    flat = rows.reshape(-1, rows.shape[-1])
    out = []
    for i, row in enumerate(flat):
        r = scale_row(row.tolist())
        assert is_safe(r), "row %d: powerTodB(avg) - 10 = %.9f, powerTodB(peak) + 10 = %.9f: within %g of an integer -- pick another seed" % (
            i, r["q_avg"], r["q_peak"], EDGE)
        out.append(r)
    return out
