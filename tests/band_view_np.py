"""NumPy model of the band drivers' view radiances and of the brightness stage, written from the definitions
and not from the kernel: the temperature at which a weighted sum of Planck band radiances (`bands_np.planck_band`) equals a
radiance, by the safeguarded Newton iteration the header states; and the channel sum of per-point view terms."""
import numpy as np

import bands_np as M

T_LO, T_HI, T_START, STOP, MAX_ITERATIONS = 1.0, 1e5, 250.0, 1e-9, 40


def _edge_term(x):
    """x^4 / (e^x - 1); 0 at x = 0."""
    out = np.zeros_like(x)
    pos = x > 0
    with np.errstate(over="ignore"):
        out[pos] = x[pos] ** 2 * x[pos] ** 2 / np.expm1(x[pos])
    return out


def channel(T, lo, hi, w):
    """(f, df/dT) of f(T) = sum_k w[k] B_k(T) at the temperatures T [n]: lo, hi [K]; w [K, n]."""
    f, df = np.zeros_like(T), np.zeros_like(T)
    for k in range(len(lo)):
        B = M.planck_band(T, lo[k], hi[k])
        slope = 4.0 * B / T + (M.RADIANCE * T) * (T * T) * (_edge_term(M.C2 * lo[k] / T) - _edge_term(M.C2 * hi[k] / T))
        f += w[k] * B
        df += w[k] * slope
    return f, df


def brightness_temperature(R, lo, hi, w=None, iterations=False):
    """T_b of the radiances R (any shape) for the bands lo, hi [K] and the weights w: None (ones), [K], or [K] + R.shape.
    NaN where the definition has no root."""
    R = np.asarray(R, dtype=np.float64)
    lo, hi = np.atleast_1d(np.asarray(lo, dtype=np.float64)), np.atleast_1d(np.asarray(hi, dtype=np.float64))
    K = lo.size
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    w = np.broadcast_to(w.reshape((K,) + (1,) * R.ndim) if w.ndim == 1 else w, (K,) + R.shape).reshape(K, -1)
    r = R.reshape(-1)
    out, count = np.full(r.shape, np.nan), np.zeros(r.shape, dtype=int)
    with np.errstate(all="ignore"):
        # the elements that have a root; only they are carried along, and each leaves when it stops
        idx = np.flatnonzero(np.isfinite(r) & (r > 0) & np.all(w >= 0, axis=0) & (w.sum(axis=0) > 0))
        f_lo = channel(np.full(idx.size, T_LO), lo, hi, w[:, idx])[0]
        f_hi = channel(np.full(idx.size, T_HI), lo, hi, w[:, idx])[0]
        idx = idx[(f_lo < r[idx]) & (r[idx] < f_hi)]
        a, b, T = np.full(idx.size, T_LO), np.full(idx.size, T_HI), np.full(idx.size, T_START)
        for it in range(MAX_ITERATIONS):
            if idx.size == 0:
                break
            f, df = channel(T, lo, hi, w[:, idx])
            count[idx] += 1
            a, b = np.where(f < r[idx], T, a), np.where(f > r[idx], T, b)
            # Newton on ln f in u = 1 / T: u' = u - (ln f - ln R) / (d ln f / du), d ln f / du = -T^2 f' / f
            Tn = 1.0 / (1.0 / T + np.log(f / r[idx]) * f / (T * T * df))
            newton = np.isfinite(Tn) & (a <= Tn) & (Tn <= b)
            Tn = np.where(newton, Tn, np.sqrt(a * b))
            stop = newton & (np.abs(Tn - T) <= STOP * Tn)
            out[idx[stop]] = Tn[stop]
            idx, a, b, T = idx[~stop], a[~stop], b[~stop], Tn[~stop]
    out, count = out.reshape(R.shape), count.reshape(R.shape)
    return (out, count) if iterations else out


def channel_sum(points, weight, scale=None):
    """The channel's view term from the per-point ones: points [K, C, nlev, 2V] -> [C, nlev, 2V], `bands_np.band_reduce` over the
    flattened lanes (one fused multiply-add per point, ascending)."""
    p = np.asarray(points, dtype=np.float64)
    K, C = p.shape[:2]
    return M.band_reduce(p.reshape(K, C, -1), weight, scale).reshape(p.shape[1:])
