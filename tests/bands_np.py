"""NumPy model of the band stages, written from the definitions and not from the kernels: the Planck radiance
of a wavenumber band from temperatures, its normalisation per (point, column), and the weighted sum over the spectral points of a
batch with one fused multiply-add per point."""
from fractions import Fraction

import numpy as np

# CODATA 2018 (exact since the 2019 redefinition of the SI)
H, C, K = 6.62607015e-34, 299792458.0, 1.380649e-23
C2 = 100.0 * H * C / K                                          # x = C2 nu / T, nu in cm^-1
RADIANCE = 2.0 * ((K * K) * (K * K)) / ((H * H * H) * (C * C))  # 2 k^4 / (h^3 c^2)
G0 = (np.pi * np.pi) * (np.pi * np.pi) / 15.0                   # G(0) = pi^4 / 15
SIGMA = np.pi * RADIANCE * G0                                   # Stefan-Boltzmann, 5.670374419e-8 W m-2 K-4
# c_k = B_k / ((k + 3) k!), k = 0, 1, 2, 4, .., 16
SERIES = {0: 1.0 / 3.0, 1: -1.0 / 8.0, 2: 1.0 / 60.0, 4: -1.0 / 5040.0, 6: 1.0 / 272160.0, 8: -1.0 / 13305600.0,
          10: 1.60590438368216149e-09, 12: -3.52279342579166215e-11, 14: 7.87208031216745774e-13, 16: -1.78404226122241216e-14}
TAIL_TERMS = 30


def S(x):
    """int_0^x t^3 / (e^t - 1) dt as the series sum c_k x^{k+3} (x < 1), by Horner in x^2 above k = 2."""
    x = np.asarray(x, dtype=np.float64)
    u = x * x
    p = np.full_like(x, SERIES[16])
    for k in (14, 12, 10, 8, 6, 4, 2):
        p = p * u + SERIES[k]
    p = p * x + SERIES[1]
    p = p * x + SERIES[0]
    return (x * u) * p


def G_tail(x):
    """int_x^inf t^3 / (e^t - 1) dt = sum_{n=1}^{30} e^{-n x} (x^3/n + 3 x^2/n^2 + 6 x/n^3 + 6/n^4) (x >= 1): one exp, the powers
    by repeated multiplication, the bracket by Horner in 1/n."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-x)
        x2 = x * x
        a3, a2, a1 = x2 * x, 3.0 * x2, 6.0 * x
        p, g = np.ones_like(x), np.zeros_like(x)
        for n in range(1, TAIL_TERMS + 1):
            r = 1.0 / n
            p = p * e
            g = g + p * (r * (a3 + r * (a2 + r * (a1 + r * 6.0))))
    return g


def G_difference(x_lo, x_hi):
    """G(x_lo) - G(x_hi) in the form that does not cancel (the split is at x = 1)."""
    x_lo, x_hi = np.broadcast_arrays(np.asarray(x_lo, dtype=np.float64), np.asarray(x_hi, dtype=np.float64))
    below = S(np.minimum(x_hi, 1.0)) - S(np.minimum(x_lo, 1.0))
    above = G_tail(np.maximum(x_lo, 1.0)) - G_tail(np.maximum(x_hi, 1.0))
    mixed = (G0 - S(np.minimum(x_lo, 1.0))) - G_tail(np.maximum(x_hi, 1.0))
    return np.where(x_hi < 1.0, below, np.where(x_lo >= 1.0, above, mixed))


def planck_band(T, nu_lo, nu_hi):
    """Band radiance W m-2 sr-1 of a black body at T (kelvin) between the wavenumbers nu_lo < nu_hi (cm^-1); the arguments
    broadcast.  T <= 0 gives NaN."""
    T, lo, hi = np.broadcast_arrays(np.asarray(T, dtype=np.float64), np.asarray(nu_lo, dtype=np.float64),
                                    np.asarray(nu_hi, dtype=np.float64))
    ok = T > 0
    Ts = np.where(ok, T, 1.0)
    t2 = Ts * Ts
    b = ((RADIANCE * t2) * t2) * G_difference((C2 * lo) / Ts, (C2 * hi) / Ts)
    return np.where(ok, b, np.nan)


def planck_bands(T, T_surface, nu_lo, nu_hi, normalise):
    """The Planck stage: T [C, L], T_surface [C], nu_lo / nu_hi [K] -> (planck [K, C, L], planck_surface [K, C], scale [K, C])."""
    T, Ts = np.atleast_2d(np.asarray(T, dtype=np.float64)), np.atleast_1d(np.asarray(T_surface, dtype=np.float64))
    lo, hi = np.atleast_1d(nu_lo).astype(np.float64), np.atleast_1d(nu_hi).astype(np.float64)
    b = planck_band(T[None, :, :], lo[:, None, None], hi[:, None, None])
    bs = planck_band(Ts[None, :], lo[:, None], hi[:, None])
    if not normalise:
        return b, bs, np.ones_like(bs)
    scale = np.fmax(np.fmax.reduce(b, axis=2), bs)
    return b / scale[:, :, None], bs / scale, scale


def planck_nu(T, nu):
    """Planck's spectral radiance per wavenumber, W m-2 sr-1 (cm^-1)^-1: 2 h c^2 nu^3 / (e^{c2 nu / T} - 1) with nu in cm^-1."""
    nu = np.asarray(nu, dtype=np.float64)
    return 2.0 * H * C * C * (100.0 * nu) ** 3 / np.expm1(C2 * nu / T) * 100.0


def planck_band_quadrature(T, nu_lo, nu_hi, nodes=64):
    """The same band radiance as a Gauss-Legendre sum of planck_nu: the independent check of the closed forms."""
    t, w = np.polynomial.legendre.leggauss(nodes)
    nu = 0.5 * (nu_hi + nu_lo) + 0.5 * (nu_hi - nu_lo) * t
    return 0.5 * (nu_hi - nu_lo) * float(np.sum(w * planck_nu(T, nu)))


def fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic, then the correctly rounded conversion)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def band_reduce(x, weight=None, scale=None, out=None):
    """The reduce stage: x [K, C, M], weight / scale [K, C] or None for ones, out [C, M] or None (accumulate = 0):
    acc = fma(w s, x, acc) for k ascending, the product w s rounded once."""
    x = np.asarray(x, dtype=np.float64)
    Kp, Cc, M = x.shape
    w = np.ones((Kp, Cc)) if weight is None else np.asarray(weight, dtype=np.float64)
    s = np.ones((Kp, Cc)) if scale is None else np.asarray(scale, dtype=np.float64)
    acc = np.zeros((Cc, M)) if out is None else np.array(out, dtype=np.float64)
    for k in range(Kp):
        ws = w[k] * s[k]
        for c in range(Cc):
            for m in range(M):
                acc[c, m] = fma(ws[c], x[k, c, m], acc[c, m])
    return acc


# ---- the points of the tests ---------------------------------------------------------------------------------
# thermal: (nu_lo, nu_hi, tauStar_atm, alb_atm, tauStar_aer, alb_aer, orders with the layer, orders without)
THERMAL_POINTS = [(350.0, 500.0, 2.0, 0.0, 0.12, 0.2, 4, 2),
                  (630.0, 700.0, 4.0, 0.0, 0.12, 0.3, 4, 2),
                  (820.0, 980.0, 0.3, 0.0, 0.3, 0.6, 8, 2),
                  (980.0, 1080.0, 1.0, 0.0, 0.3, 0.6, 7, 2),
                  (1180.0, 1390.0, 0.6, 0.1, 0.3, 0.5, 7, 5)]
N_, L_, RHO, Z0, T_SURFACE = 32, 24, 0.1, 120.0, 288.0
OLR_WITH, OLR_WITHOUT = 12.7246, 14.4338                        # band-summed outgoing flux W m-2 of the five points (the oracle)
# solar: (tauStar_atm, alb_atm, tauStar_aer, alb_aer), their weights, and the oracle's orders at mu0 = 0.5 / 0.8
SOLAR_POINTS = [(0.5, 1.0, 0.16, 0.99), (0.124, 1.0, 0.12, 0.97), (0.05, 0.9, 0.09, 0.95), (0.02, 0.6, 0.06, 0.9)]
SOLAR_WEIGHTS = (0.1, 0.4, 0.3, 0.2)
SOLAR_MU0 = (0.5, 0.8)
SOLAR_ORDERS = {True: [(14, 14), (9, 9), (7, 7), (6, 6)], False: [(12, 12), (7, 7), (6, 5), (4, 4)]}   # [with layer][point] = (mu0 0.5, 0.8)
# the longwave bands of the quadrature check: sixteen between 10 and 3250 cm^-1
LW_BANDS = [(10, 100), (100, 350), (350, 500), (500, 630), (630, 700), (700, 820), (820, 980), (980, 1080), (1080, 1180),
            (1180, 1390), (1390, 1480), (1480, 1800), (1800, 2080), (2080, 2250), (2250, 2600), (2600, 3250)]
LW_TEMPERATURES = (180.0, 216.5, 288.0, 320.0)


def temperature_profile(L, z0=Z0):
    """288 K at the ground, -6.5 K km^-1, 216.5 K above, at the levels' altitudes np.linspace(z0, 0, L)."""
    return np.maximum(288.0 - 6.5 * np.linspace(z0, 0, L), 216.5)
