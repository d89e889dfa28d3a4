"""numpy restatement of FFT::mapFFTToScreen (pebblelib/fft.cpp:411-534) and SignalSpectrum::mapFFTZoomedToScreen's span
(application/signalspectrum.cpp:151-167), for the screen-map tests.

float32 where the reference computes in float, float64 where it computes in double, and float -> int conversions as an x86-64
build performs them (cvttss2si / cvttsd2si: toward zero, INT_MIN for NaN and out of range).  Int sums that overflow wrap.
"""
import numpy as np

MIN_DB = -120  # DB::minDb
INT_MIN = -(1 << 31)


def wrap32(v):
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def trunc_f32(f):
    """float32 (array or scalar) -> int32 like cvttss2si"""
    f = np.asarray(f, dtype=np.float32)
    ok = (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
    out = np.full(f.shape, INT_MIN, dtype=np.int64)
    out[ok] = np.trunc(f[ok].astype(np.float64)).astype(np.int64)
    return out.astype(np.int32)


def trunc_f64(d):
    """float64 (array or scalar) -> int32 like cvttsd2si"""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (d > -2147483649.0) & (d < 2147483648.0)
    out = np.full(d.shape, INT_MIN, dtype=np.int64)
    out[ok] = np.trunc(d[ok]).astype(np.int64)
    return out.astype(np.int32)


def zoom_edges(hires_rate, zoom, mode_offset=0):
    """quint16 span = hiResSampleRate * zoom (x86-64: truncate to int32, keep the low 16 bits); (-span/2 - off, span/2 - off)"""
    span = int(trunc_f64(np.float64(hires_rate) * np.float64(zoom))) & 0xFFFF
    half = -(span // 2)  # -span/2 in C: (-span) / 2 truncates toward zero
    return wrap32(half - mode_offset), wrap32(span // 2 - mode_offset)


def geometry(fft_size, sample_rate, start_freq, stop_freq, x_pixels):
    """-> dict of the per-call values: bin_low, bins_to_plot, pixels_per_bin, bins_per_pixel (float32), averaged"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        bph = np.float32(fft_size) / np.float32(sample_rate)
        lo = int(trunc_f32(np.float32(start_freq) * bph))
        hi = int(trunc_f32(np.float32(stop_freq) * bph))
        bin_low = wrap32(lo + fft_size // 2)
        bin_high = wrap32(hi + fft_size // 2)
        n = wrap32(bin_high - bin_low)
        ppb = np.float32(x_pixels) / np.float32(n)
        bpp = np.float32(n) / np.float32(x_pixels)
    return dict(bin_low=bin_low, bins_to_plot=n, pixels_per_bin=ppb, bins_per_pixel=bpp, averaged=n > x_pixels)


def pixel_bins(g, x_pixels):
    i = np.arange(x_pixels, dtype=np.int64).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        off = i * g["bins_per_pixel"] if g["averaged"] else i / g["pixels_per_bin"]
        return trunc_f32(np.float32(g["bin_low"]) + off.astype(np.float32))


def y_scale(y_pixels, max_db, min_db):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(np.float64(-y_pixels) / (np.float64(max_db) - np.float64(min_db)))


def to_y(power_db, ys, y_pixels):
    with np.errstate(invalid="ignore", over="ignore"):
        y = trunc_f32(ys * np.asarray(power_db, dtype=np.int32).astype(np.float32) - np.float32(1.0))
    return np.clip(y, 0, y_pixels - 1).astype(np.int32)  # qBound(0, y, yPixels - 1)


def map_fft_to_screen(db, fft_size, sample_rate, y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq, tol=1e-9, chunk=256):
    """db: [..., fft_size] dB rows (the doubles FFT::fftSpectrum left in inBuf; float32 rows are widened exactly).

    Returns (out, v, alt), each [..., x_pixels]:
      out  int32: the reference's plot heights;
      v    float64: for averaged pixels the value powerdB truncates (10 log10(mean power) - maxdB), NaN elsewhere;
      alt  int32: for averaged pixels with v within tol * max(1, |v|) of an integer, the height computed from the neighbouring
           powerdB (the other side of that integer); equal to out everywhere else.
    """
    db = np.asarray(db)
    if db.dtype not in (np.float32, np.float64):
        db = db.astype(np.float64)
    lead = db.shape[:-1]
    rows = db.reshape(-1, db.shape[-1])
    assert rows.shape[1] >= fft_size
    g = geometry(fft_size, sample_rate, start_freq, stop_freq, x_pixels)
    b = pixel_bins(g, x_pixels).astype(np.int64)
    last = np.concatenate([[-1], b[:-1]])
    inside = (b >= 0) & (b < fft_size)
    avg = inside & g["averaged"] & (last > 0) & (b != last + 1)
    direct = inside & ~avg
    ys = y_scale(y_pixels, max_db, min_db)
    R = rows.shape[0]
    out = np.empty((R, x_pixels), dtype=np.int32)
    alt = np.empty((R, x_pixels), dtype=np.int32)
    v = np.full((R, x_pixels), np.nan)
    ia = np.nonzero(avg)[0]
    lo, hi = last[ia], b[ia]
    skipped = hi - lo
    idx = np.empty(2 * len(ia), dtype=np.int64)
    idx[0::2], idx[1::2] = lo, np.minimum(hi, fft_size - 1)
    for r0 in range(0, R, chunk):
        blk = rows[r0:r0 + chunk, :fft_size].astype(np.float64)  # (float dB rows widen exactly, a chunk at a time)
        pdb = np.full((blk.shape[0], x_pixels), MIN_DB, dtype=np.int32)
        pdb[:, direct] = trunc_f64(blk[:, b[direct]] - np.float64(max_db))
        pa = pdb.copy()
        if len(ia):
            P = np.power(10.0, blk / 10.0)  # DB::dBToPower
            s = np.add.reduceat(P, idx, axis=1)[:, 0::2] if len(idx) else np.zeros((blk.shape[0], 0))
            s[:, skipped <= 0] = 0.0
            with np.errstate(divide="ignore", invalid="ignore"):
                p = s / skipped.astype(np.float64)
                dbv = np.where(p == 0.0, float(MIN_DB), 10.0 * np.log10(np.where(p == 0.0, 1.0, p)))  # DB::powerTodB
            vv = dbv - np.float64(max_db)
            vv[:, skipped == 0] = np.nan  # 0 / 0 (never met with binsPerPixel >= 1 below 2^24 bins)
            pdb[:, ia] = trunc_f64(vv)
            v[r0:r0 + blk.shape[0], ia] = vv
            d = tol * np.maximum(1.0, np.abs(vv))
            with np.errstate(invalid="ignore"):
                near = np.abs(vv - np.round(vv)) <= d
            lo_t, hi_t = trunc_f64(vv - d), trunc_f64(vv + d)
            other = np.where(lo_t != pdb[:, ia], lo_t, hi_t)
            pa[:, ia] = np.where(near, other, pdb[:, ia])
        out[r0:r0 + blk.shape[0]] = to_y(pdb, ys, y_pixels)
        alt[r0:r0 + blk.shape[0]] = to_y(pa, ys, y_pixels)
    return out.reshape(lead + (x_pixels,)), v.reshape(lead + (x_pixels,)), alt.reshape(lead + (x_pixels,))


def map_scalar(db, fft_size, sample_rate, y_pixels, x_pixels, max_db, min_db, start_freq, stop_freq):
    """the reference's loop, pixel by pixel in plain Python (pins the vectorised restatement above on small cases)"""
    g = geometry(fft_size, sample_rate, start_freq, stop_freq, x_pixels)
    ys = y_scale(y_pixels, max_db, min_db)
    out, last = [], -1
    for i in range(x_pixels):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if g["averaged"]:
                b = int(trunc_f32(np.float32(g["bin_low"]) + np.float32(i) * g["bins_per_pixel"]))
            else:
                b = int(trunc_f32(np.float32(g["bin_low"]) + np.float32(i) / g["pixels_per_bin"]))
        if b < 0 or b >= fft_size:
            pdb = MIN_DB
        elif g["averaged"] and last > 0 and b != last + 1:
            k = b - last
            t = 0.0
            for j in range(k):
                t += 10.0 ** (float(db[last + j]) / 10.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                p = np.float64(t) / np.float64(k)
            pdb = int(trunc_f64((MIN_DB if p == 0.0 else 10.0 * np.log10(p)) - max_db))
        else:
            pdb = int(trunc_f64(float(db[b]) - max_db))
        last = b
        out.append(int(to_y(np.int32(pdb), ys, y_pixels)))
    return np.array(out, dtype=np.int32)
