"""Band-integrated fluxes and heating rates: K spectral points x C physical columns solved as K C library
columns, laid out point-major (b = k C + c), and summed over the points on the device.

Every solve of the library is monochromatic.  A band structure -- bands, or the g-points of a k-distribution -- is a weighted
sum of such solves; the caller brings each point's optical depths, albedos and weight.  The drivers here run the points as
batches, take the flux epilogue of every batch on the device and add the points up there (`Solver.band_reduce_device`): only the
summed arrays and the order counts cross PCIe.

The thermal source is normalised on the way in.  The order loop's mu -> 0 search compares second differences of the field with
an absolute threshold of 1e-4, so a Planck source in W m-2 sr-1 (values around 10) runs it off the grid where the same source
divided by its maximum converges in a few orders.  `Solver.planck_bands_device` therefore divides every (point, column) by its
maximum and hands the maximum back as the scale, which re-enters in the weighted sum.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _lib
from . import main
from .thermal import BOLTZMANN_K, LIGHT_C, PLANCK_H

C2 = 100.0 * PLANCK_H * LIGHT_C / BOLTZMANN_K                    # x = C2 nu / T with nu in cm^-1
RADIANCE = 2.0 * ((BOLTZMANN_K * BOLTZMANN_K) * (BOLTZMANN_K * BOLTZMANN_K)) / ((PLANCK_H * PLANCK_H * PLANCK_H) * (LIGHT_C * LIGHT_C))
G0 = (np.pi * np.pi) * (np.pi * np.pi) / 15.0
# c_k = B_k / ((k + 3) k!) for k = 16, 14, .., 2, then 1 and 0
_SERIES_EVEN = (-1.78404226122241216e-14, 7.87208031216745774e-13, -3.52279342579166215e-11, 1.60590438368216149e-09,
                -1.0 / 13305600.0, 1.0 / 272160.0, -1.0 / 5040.0, 1.0 / 60.0)
_TAIL_TERMS = 30
BAND_FIELD_BYTES = 1 << 30          # the default points_per_solve keeps one field buffer [P C, L, 2N] of a solve within this
WANT = ("flux_down", "flux_up", "heating_rate", "net_toa")


def _S(x):
    u = x * x
    p = np.full_like(x, _SERIES_EVEN[0])
    for c in _SERIES_EVEN[1:]:
        p = p * u + c
    p = p * x + -1.0 / 8.0
    p = p * x + 1.0 / 3.0
    return (x * u) * p


def _G(x):
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-x)
        x2 = x * x
        a3, a2, a1 = x2 * x, 3.0 * x2, 6.0 * x
        p, g = np.ones_like(x), np.zeros_like(x)
        for n in range(1, _TAIL_TERMS + 1):
            r = 1.0 / n
            p = p * e
            g = g + p * (r * (a3 + r * (a2 + r * (a1 + r * 6.0))))
    return g


def planck_band(T, nu_lo, nu_hi):
    """Planck radiance of a black body at T (kelvin) integrated over the wavenumber band [nu_lo, nu_hi] (cm^-1), W m-2 sr-1 (host
    NumPy; the arguments broadcast): B = 2 k^4 T^4 / (h^3 c^2) [G(x_lo) - G(x_hi)], x = 100 h c nu / (k T), G(x) = int_x^inf
    t^3 / (e^t - 1) dt -- below x = 1 pi^4/15 minus the Bernoulli series, above it the sum of 30 exponentials, and the difference
    in the form that does not cancel.  nu_lo = 0 is allowed; pi B(0, inf) = sigma T^4.  Within 6e-15 of quadrature for bands of
    10 cm^-1 and more; a band of width dnu loses digits by cancellation (up to 6e-13 relative at 1 cm^-1, 6e-11 at 0.01 cm^-1), so a
    monochromatic source is `thermal.planck_radiance`.  The arithmetic of `Solver.planck_bands_device`."""
    T, lo, hi = np.broadcast_arrays(np.asarray(T, dtype=np.float64), np.asarray(nu_lo, dtype=np.float64),
                                    np.asarray(nu_hi, dtype=np.float64))
    if np.any(~(T > 0)):
        raise ValueError("planck_band needs T > 0 K")
    if np.any(~np.isfinite(lo)) or np.any(~np.isfinite(hi)) or np.any(lo < 0) or np.any(hi <= lo):
        raise ValueError("planck_band needs finite band edges with 0 <= nu_lo < nu_hi (cm^-1)")
    xl, xh = (C2 * lo) / T, (C2 * hi) / T
    below = _S(np.minimum(xh, 1.0)) - _S(np.minimum(xl, 1.0))
    above = _G(np.maximum(xl, 1.0)) - _G(np.maximum(xh, 1.0))
    mixed = (G0 - _S(np.minimum(xl, 1.0))) - _G(np.maximum(xh, 1.0))
    t2 = T * T
    return ((RADIANCE * t2) * t2) * np.where(xh < 1.0, below, np.where(xl >= 1.0, above, mixed))


BRIGHTNESS_BRACKET = (1.0, 1e5)     # kelvin
BRIGHTNESS_START = 250.0
BRIGHTNESS_STOP = 1e-9              # the accepted Newton step that ends the iteration, relative to T
BRIGHTNESS_ITERATIONS = 40
BRIGHTNESS_MAX_BANDS = 64           # the device entry's band edges travel by value


def _slope_term(x):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x2 = x * x
        return np.where(x > 0.0, (x2 * x2) / np.expm1(np.where(x > 0.0, x, 1.0)), 0.0)


def _channel(T, lo, hi, w):
    """f = sum_k w[k] B_k(T) and df/dT, k ascending: T [...], lo / hi [K, 1..], w [K, ...]."""
    f, df = np.zeros_like(T), np.zeros_like(T)
    t3 = (RADIANCE * T) * (T * T)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(lo.shape[0]):
            B = planck_band(T, lo[k], hi[k])
            dB = 4.0 * B / T + t3 * (_slope_term((C2 * lo[k]) / T) - _slope_term((C2 * hi[k]) / T))
            f = f + w[k] * B
            df = df + w[k] * dB
    return f, df


def brightness_temperature(radiance, nu_lo, nu_hi, weights=None, return_iterations=False):
    """BRIGHTNESS TEMPERATURE OF A BAND-SUMMED RADIANCE (host NumPy): the temperature T (kelvin) at which
    f(T) = sum_k weights[k] planck_band(T, nu_lo[k], nu_hi[k]) equals `radiance` (W m-2 sr-1, any shape).  `nu_lo`, `nu_hi`: [K]
    (or scalars: one band) in cm^-1; `weights`: None (ones), [K], or [K, ...] broadcasting against the radiance behind the
    leading K -- g-point weights of one band (equal edges, sum 1) or the response over sub-bands.

    Newton on ln f in u = 1 / T from 250 K, u' = u + ln(f / R) f / (T^2 f'), with dB/dT = 4 B / T + 2 k^4 / (h^3 c^2) T^3
    [x_lo^4 / (e^x_lo - 1) - x_hi^4 / (e^x_hi - 1)]; a bracket [1 K, 1e5 K] that every evaluation tightens, and whose geometric
    mean replaces an iterate that is not finite or leaves it; the first accepted Newton step with |dT| <= 1e-9 T is applied and
    ends the iteration; at most 40 iterations, then NaN.  NaN where the radiance is not finite or <= 0, lies outside
    (f(1 K), f(1e5 K)), or the weights are all zero or one is negative.  The arithmetic of
    `Solver.brightness_temperature_device`; `return_iterations=True`: (T, the evaluations each element took, 0 where NaN from
    the start)."""
    R = np.asarray(radiance, dtype=np.float64)
    lo, hi = np.atleast_1d(np.asarray(nu_lo, dtype=np.float64)), np.atleast_1d(np.asarray(nu_hi, dtype=np.float64))
    if lo.ndim != 1 or lo.shape != hi.shape or lo.size < 1:
        raise ValueError("brightness_temperature needs nu_lo and nu_hi as two arrays [K] of one length")
    if np.any(~np.isfinite(lo)) or np.any(~np.isfinite(hi)) or np.any(lo < 0) or np.any(hi <= lo):
        raise ValueError("brightness_temperature needs finite band edges with 0 <= nu_lo < nu_hi (cm^-1)")
    K = lo.size
    w = np.ones((K,) + (1,) * R.ndim) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.ndim == 1:
        w = w.reshape((-1,) + (1,) * R.ndim)
    try:
        w = np.broadcast_to(w, (K,) + R.shape)
    except ValueError:
        raise ValueError("weights of the shape %s do not broadcast to [K, ...] = %s" % (np.shape(weights), (K,) + R.shape)) from None
    lo, hi = lo.reshape((K,) + (1,) * R.ndim), hi.reshape((K,) + (1,) * R.ndim)
    with np.errstate(invalid="ignore"):
        live = np.isfinite(R) & (R > 0) & np.all(w >= 0, axis=0) & (np.sum(w, axis=0) > 0)
        a, b = np.full(R.shape, BRIGHTNESS_BRACKET[0]), np.full(R.shape, BRIGHTNESS_BRACKET[1])
        live = live & (_channel(a, lo, hi, w)[0] < R) & (R < _channel(b, lo, hi, w)[0])
    T = np.full(R.shape, BRIGHTNESS_START)
    out, its = np.full(R.shape, np.nan), np.zeros(R.shape, dtype=np.int64)
    for it in range(BRIGHTNESS_ITERATIONS):
        if not np.any(live):
            break
        f, df = _channel(T, lo, hi, w)
        a, b = np.where(live & (f < R), T, a), np.where(live & (f > R), T, b)
        with np.errstate(all="ignore"):
            Tn = 1.0 / (1.0 / T + (np.log(f / R) * f) / ((T * T) * df))
            newton = (Tn >= a) & (Tn <= b)
        Tn = np.where(newton, Tn, np.sqrt(a * b))
        with np.errstate(invalid="ignore"):
            stop = live & newton & (np.abs(Tn - T) <= BRIGHTNESS_STOP * Tn)
        T = np.where(live, Tn, T)
        its = its + live
        out = np.where(stop, T, out)
        live = live & ~stop
    return (out, its) if return_iterations else out


def wavenumber_bands(edges_um):
    """(nu_lo [K], nu_hi [K]) in cm^-1 of the K bands between K + 1 wavelength edges in micrometres (strictly ascending or
    descending; band k lies between edges k and k + 1)."""
    e = np.asarray(edges_um, dtype=np.float64)
    if e.ndim != 1 or e.size < 2 or np.any(~(e > 0)) or not (np.all(np.diff(e) > 0) or np.all(np.diff(e) < 0)):
        raise ValueError("wavenumber_bands needs at least two wavelength edges > 0 um, strictly ascending or descending")
    with np.errstate(divide="ignore"):
        nu = 1e4 / e
    return np.minimum(nu[:-1], nu[1:]), np.maximum(nu[:-1], nu[1:])


@dataclass
class BandResult:
    flux_down: Optional[np.ndarray]       # [C, L] sum over the points of weight x (scale x) the point's downward flux
    flux_up: Optional[np.ndarray]         # [C, L]
    heating_rate: Optional[np.ndarray]    # [C, L]
    net_toa: Optional[np.ndarray]         # [C]
    n: np.ndarray                         # [K, C] orders of every point's solve
    status: np.ndarray                    # [K, C]
    scale: Optional[np.ndarray] = None    # [K, C] (thermal) the maximum each point's source was divided by, W m-2 sr-1
    point_net_toa: Optional[np.ndarray] = None   # [K, C] (per_point=True) every point's own net_toa, unweighted, scale applied
    # with view_mu: the channel's radiance at the view lanes, summed over the points like the fluxes
    view_mu_signed: Optional[np.ndarray] = None          # [2V] the lanes (-view_mu, +view_mu)
    I_view_first: Optional[np.ndarray] = None            # [C, nlev, 2V] the first term: emission (thermal) or first order (solar)
    I_view_scattered: Optional[np.ndarray] = None        # [C, nlev, 2V]
    I_view: Optional[np.ndarray] = None                  # [C, nlev, 2V] their sum
    brightness_temperature: Optional[np.ndarray] = None  # [C, nlev, 2V] (thermal, brightness=True) kelvin; NaN where I_view is 0
    point_I_view: Optional[np.ndarray] = None            # [K, C, nlev, 2V] (per_point=True) every point's I_view, unweighted, scale applied


# ---- checks made before any handle exists ---------------------------------------------------------------------------------------
def _refuse(want, beam, azimuths, view_azimuths, devices, first_order, views=False):
    want = tuple(want)
    if "diffusivity" in want:
        raise ValueError("want: 'diffusivity' is a ratio of two integrals of the field, not additive over spectral points; sum "
                         "flux_down and flux_up and form it from them")
    bad = [k for k in want if k not in WANT]
    if bad or (not want and not views):
        raise ValueError("want must name some of %s (got %r)" % (WANT, want))
    if beam != "plane":
        raise ValueError("beam='spherical' is not available in the band drivers: the slant-path first order is solved per batch "
                         "with its own stage; call SOS_Aer_batch(beam='spherical') per point")
    if azimuths is not None or view_azimuths is not None:
        raise ValueError("azimuths / view_azimuths are not available in the band drivers: they sum fluxes, which need only the "
                         "m = 0 mode")
    if devices is not None:
        raise ValueError("devices=[...] is not available in the band drivers: the band sum runs on one device; shard the columns "
                         "and call per device=")
    if first_order != "coded":
        raise ValueError("first_order='readme' is not available in the band drivers (parity of the README first order is unpinned)")
    return want


def _array(a, name):
    try:
        return np.asarray(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s must be numbers" % name) from None


def _widths(K, per_point, per_column, extra=()):
    """C of the call: what the [K, C] per-point arrays, the [C] per-column arrays and `extra` widths agree on (default 1)."""
    seen = set(int(c) for c in extra)
    for name, a in per_point.items():
        if a.ndim == 2:
            seen.add(a.shape[1])
        elif a.ndim > 2:
            raise ValueError("%s has the shape %s: a per-point argument is a scalar, [K] or [K, C]" % (name, a.shape))
    for name, a in per_column.items():
        if a.ndim == 1:
            seen.add(a.shape[0])
        elif a.ndim > 1:
            raise ValueError("%s has the shape %s: a per-column argument is a scalar or [C]" % (name, a.shape))
    seen.discard(1)
    if len(seen) > 1:
        raise ValueError("the arguments do not broadcast to [K, C] = [%d, C]: they name C = %s" % (K, sorted(seen)))
    return seen.pop() if seen else 1


def _per_point(a, K, C, name):
    if a.shape not in ((), (K,), (K, 1), (1, C), (K, C)):
        raise ValueError("%s has the shape %s, which does not broadcast to [K, C] = [%d, %d] (a per-point argument is a scalar, "
                         "[K] or [K, C])" % (name, a.shape, K, C))
    return np.ascontiguousarray(np.broadcast_to(a[:, None] if a.ndim == 1 else a, (K, C)))


def _per_column(a, C, name):
    if a.shape not in ((), (1,), (C,)):
        raise ValueError("%s has the shape %s: a per-column argument is a scalar or [C] = (%d,)" % (name, a.shape, C))
    return np.ascontiguousarray(np.broadcast_to(a, (C,)))


def _gas_points(gas_tau, K, C, L):
    """`gas_tau` of a band call, [K, L] or [K, C, L] -- each spectral point its own cumulative absorption profile -- as [K, C, L],
    or None.  Shape and values are checked here, once, before any handle exists (main._gas_args)."""
    if gas_tau is None:
        return None
    g = _array(gas_tau, "gas_tau")
    if g.shape not in ((K, L), (K, C, L)):
        raise ValueError("gas_tau must have the shape [K, L] = (%d, %d) or [K, C, L] = (%d, %d, %d): the gas absorption profile of "
                         "every spectral point (got %s)" % (K, L, K, C, L, g.shape))
    g = np.ascontiguousarray(np.broadcast_to(g[:, None, :] if g.ndim == 2 else g, (K, C, L)))
    main._gas_args(g.reshape(K * C, L), K * C, L)
    return g


def _points_per_solve(points_per_solve, K, C, L, N):
    if points_per_solve is None:
        return int(max(1, min(K, BAND_FIELD_BYTES // (C * L * 2 * N * 8))))
    P = int(points_per_solve)
    if P < 1:
        raise ValueError("points_per_solve must be >= 1 (got %r)" % (points_per_solve,))
    return min(P, K)


def _view_points(view_mu, view_levels, view_quadrature, L, surface, atm_phase_fun, aer_phase_fun, point_aerosol=None):
    """Checks of `view_mu` in a band call, made before any handle exists: None, or (view_mu [V], levels as row indices,
    quadrature) as `main._view_args` returns them."""
    if view_mu is None:
        return None
    if point_aerosol is not None or isinstance(aer_phase_fun, (list, tuple)):
        raise ValueError("view_mu is not available in the band drivers with a list of aerosols in aer_phase_fun (point_aerosol): "
                         "the view stage reads one aerosol phase function; call per aerosol and add the sums")
    if surface != "specular":
        raise ValueError("view_mu is not available in the band drivers with surface=%r: the first term at the view lanes (the "
                         "emission, the solar first order) is specular / none only, and the Lambertian boundary of the orders "
                         "n >= 2 needs the grid's surface row of every order" % (surface,))
    return main._view_args(view_mu, view_levels, view_quadrature, L, None, None, None, None, surface, None, "coded", None, None,
                           atm_phase_fun, aer_phase_fun)


def _brightness_args(brightness, view, weights, K):
    """Checks of `brightness` in `band_thermal`, made before any handle exists: whether the brightness stage runs."""
    if not isinstance(brightness, (bool, np.bool_)):
        raise ValueError("brightness must be True or False (got %r)" % (brightness,))
    if view is None or not brightness:
        return False
    if K > BRIGHTNESS_MAX_BANDS:
        raise ValueError("brightness=True takes at most %d bands (got K = %d): the sum over the bands sits inside the inversion, "
                         "whose band edges travel by value; pass brightness=False and invert the channel's I_view yourself"
                         % (BRIGHTNESS_MAX_BANDS, K))
    if np.any(~(weights >= 0)) or np.any(~(weights.sum(axis=0) > 0)):
        c = int(np.flatnonzero(np.any(~(weights >= 0), axis=0) | ~(weights.sum(axis=0) > 0))[0])
        raise ValueError("brightness=True needs weights >= 0 that are not all zero in a column (column %d: %s): the channel's "
                         "radiance must increase with temperature; pass brightness=False" % (c, weights[:, c]))
    return True


class _Views:
    """The device side of the band sum of view radiances: the view stage on a chunk's resident field, and the summed first and
    scattered terms [C, nlev, 2V].  The phase rows and p0 rows are built once, at the first (and largest) chunk."""

    def __init__(self, torch, dev, view, phases, device, C, per_point):
        self.vmu, self.vlev, self.vquad = view
        self.phases, self.device, self.dev, self.C = phases, device, dev, C
        shape = (C, len(self.vlev), 2 * len(self.vmu))
        self.M = shape[1] * shape[2]
        self.first = torch.zeros(shape, dtype=torch.float64, device=dev)
        self.scat = torch.zeros(shape, dtype=torch.float64, device=dev)
        self.points = [] if per_point else None
        self.rows = self.cur = None

    def stage(self, s, d_tau, d_I, mu0, thermal=None, sigma=None, profile=False):
        """The view stage on B columns, inside a stream scope: both terms [B, nlev, 2V] stay on the device for `reduce`."""
        import torch
        if self.rows is None:
            d_mu0 = torch.from_numpy(np.array(mu0, dtype=np.float64, order="C")).to(self.dev)
            self.rows = main.view_rows(s, self.vmu, d_mu0, self.phases[:3], self.phases[3:], self.dev)
        self.cur = main.view_radiance(s, d_tau, d_I, mu0, self.vmu, self.vlev, self.vquad, *self.phases, self.device, thermal=thermal,
                                      sigma=sigma, profile=profile, dev=self.dev, keep_device=True, rows=self.rows)

    def reduce(self, s, P, d_weight, d_scale, first):
        for x, o in zip(self.cur, (self.first, self.scat)):
            s.band_reduce_device(x.data_ptr(), o.data_ptr(), self.C, P, self.M, d_weight, d_scale, accumulate=not first)
        if self.points is not None:
            self.points.append(self.cur[0] + self.cur[1])
        self.cur = None


def _view_result(r, vw, d_view, scale=None):
    """The view fields of BandResult `r` from the sums of `vw` and their sum `d_view` [C, nlev, 2V], formed on the device."""
    import torch
    r.view_mu_signed = np.concatenate((-vw.vmu, vw.vmu))
    r.I_view_first, r.I_view_scattered, r.I_view = vw.first.cpu().numpy(), vw.scat.cpu().numpy(), d_view.cpu().numpy()
    if vw.points is not None:
        K = r.n.shape[0]
        p = torch.cat(vw.points).cpu().numpy().reshape((K,) + r.I_view.shape)
        r.point_I_view = p if scale is None else p * scale[:, :, None, None]


def _thermal_inputs(bands, temperature, surface_temperature, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer, weights,
                    surface_emissivity, nb_layers):
    """Every array of a thermal band call at its full shape: (nu_lo [K], nu_hi [K], T [C, L], T_s [C], dict of the per-point
    [K, C] arrays, grd_alb [C], emissivity [C] or None)."""
    L = int(nb_layers)
    if isinstance(bands, tuple) and len(bands) == 2:
        lo, hi = np.atleast_1d(_array(bands[0], "bands")), np.atleast_1d(_array(bands[1], "bands"))
    else:
        b = _array(bands, "bands")
        lo, hi = (b[:, 0], b[:, 1]) if b.ndim == 2 and b.shape[1] == 2 else (b, None)
    if hi is None or lo.ndim != 1 or lo.shape != hi.shape:
        raise ValueError("bands must be a tuple (nu_lo [K], nu_hi [K]) or an array [K, 2] of wavenumber edges in cm^-1")
    K = lo.size
    if K < 1:
        raise ValueError("bands: no band")
    if np.any(~np.isfinite(lo)) or np.any(~np.isfinite(hi)) or np.any(lo < 0):
        raise ValueError("bands: an edge must be finite and >= 0 cm^-1")
    if np.any(hi <= lo):
        k = int(np.flatnonzero(hi <= lo)[0])
        raise ValueError("bands: band %d = [%g, %g] cm^-1 has nu_hi <= nu_lo" % (k, lo[k], hi[k]))
    T = _array(temperature, "temperature")
    if T.ndim not in (1, 2) or T.shape[-1] != L:
        raise ValueError("temperature must have the shape [L] = (%d,) or [C, L] (got %s)" % (L, T.shape))
    pp = dict(tauStar_aer=_array(tauStar_aer, "tauStar_aer"), tauStar_atm=_array(tauStar_atm, "tauStar_atm"),
              alb_atm=_array(alb_atm, "alb_atm"), alb_aer=_array(alb_aer, "alb_aer"),
              weights=_array(1.0 if weights is None else weights, "weights"))
    pc = dict(surface_temperature=_array(surface_temperature, "surface_temperature"), grd_alb=_array(grd_alb, "grd_alb"))
    if surface_emissivity is not None:
        pc["surface_emissivity"] = _array(surface_emissivity, "surface_emissivity")
    C = _widths(K, pp, pc, [T.shape[0]] if T.ndim == 2 else [])
    pp = {k: _per_point(v, K, C, k) for k, v in pp.items()}
    pc = {k: _per_column(v, C, k) for k, v in pc.items()}
    if T.ndim == 2 and T.shape[0] not in (1, C):
        raise ValueError("temperature has the shape %s, the call has C = %d columns" % (T.shape, C))
    T = np.ascontiguousarray(np.broadcast_to(T, (C, L)))
    if np.any(~(T > 0)) or np.any(~(pc["surface_temperature"] > 0)):
        raise ValueError("temperature and surface_temperature must be > 0 K")
    return (np.ascontiguousarray(lo), np.ascontiguousarray(hi), T, pc["surface_temperature"], pp, pc["grd_alb"],
            pc.get("surface_emissivity"))


class _Sum:
    """The device side of a band sum: per-chunk epilogue buffers [P C, M] and the summed outputs [C, M]."""

    def __init__(self, torch, dev, want, per_point, PC, C, L):
        self.names = [k for k in WANT if k in want or (k == "net_toa" and per_point)]
        width = lambda k: 1 if k == "net_toa" else L
        self.buf = {k: torch.empty((PC, width(k)), dtype=torch.float64, device=dev) for k in self.names}
        self.out = {k: torch.zeros((C, width(k)), dtype=torch.float64, device=dev) for k in self.names if k in want}
        self.C, self.per_point = C, per_point

    def ptr(self, k):
        return self.buf[k].data_ptr() if k in self.buf else 0

    def reduce(self, s, P, d_weight, d_scale, first):
        for k, o in self.out.items():
            s.band_reduce_device(self.buf[k].data_ptr(), o.data_ptr(), self.C, P, o.shape[1], d_weight, d_scale, accumulate=not first)

    def result(self):
        host = {k: v.cpu().numpy() for k, v in self.out.items()}
        return {k: (host[k][:, 0] if k == "net_toa" else host[k]) if k in host else None for k in WANT}


def _sum_points(s, device, acc, P, d_weight, d_scale, solve_chunk, epilogue, N, max_orders, views=None, view_stage=None):
    """The chunk loop of both drivers: per chunk of P points `solve_chunk(k0, k1, B)` -> the tensors {"I", "n", "status",
    "tau"} of its B = (k1 - k0) C columns, left on the device; then, with the handle `s` on torch's stream, `epilogue(d, acc,
    B)` into the chunk buffers of `acc` and `band_reduce_device` with the weights d_weight [K, C] (and the scales d_scale
    [K, C], or None), accumulating over the chunks -- the chunks run in ascending order, so the sum adds the points in
    ascending order.  Any non-zero status raises (`N`, `max_orders`: for the message).  Returns (n [K, C], status [K, C], every
    point's net_toa [K, C] or None); the summed arrays are `acc.result()`.  `views` (a `_Views`, with `view_mu`): in the same
    scope `view_stage(d, k0, k1, B)` runs the view stage on the chunk where `solve_chunk` has not (it has under `gas_tau`, while
    the weights were set), and both terms are reduced like the epilogue's buffers; `acc` may then have nothing to sum."""
    import torch
    (K, C), per_point = d_weight.shape, acc.per_point
    n_all, st_all, net_all = [], [], []
    for k0 in range(0, K, P):
        k1 = min(K, k0 + P)
        B = (k1 - k0) * C
        d = solve_chunk(k0, k1, B)
        with main._on_torch_stream(s, device):
            w_ptr, s_ptr = d_weight[k0:k1].data_ptr(), 0 if d_scale is None else d_scale[k0:k1].data_ptr()
            if acc.names:
                epilogue(d, acc, B)
            acc.reduce(s, k1 - k0, w_ptr, s_ptr, k0 == 0)
            if views is not None:
                view_stage(d, k0, k1, B)
                views.reduce(s, k1 - k0, w_ptr, s_ptr, k0 == 0)
            if per_point:
                net_all.append(acc.buf["net_toa"][:B, 0].clone())
        n_all.append(d["n"])
        st_all.append(d["status"])
    n = torch.cat(n_all).cpu().numpy().reshape(K, C)
    status = torch.cat(st_all).cpu().numpy().reshape(K, C)
    main._raise_unconverged(status, N, max_orders)
    point = torch.cat(net_all).cpu().numpy().reshape(K, C) if per_point else None
    return n, status, point


# ---- the thermal driver -------------------------------------------------------------------------------------------------------------
def band_thermal(bands, temperature, surface_temperature, tauStar_aer, grd_alb, *, tauStar_atm, alb_atm, alb_aer, weights=None,
                 surface_emissivity=None, want=WANT, points_per_solve=None, per_point=False, z0=120, z_up=25, z_down=17,
                 nb_layers=200, nb_angles=128, atm_phase_fun="rayleigh", g_atm=0.0, aer_phase_fun="hg", g_aer=0.7, mie_atm=None,
                 mie_aer=None, surface="specular", tol=1e-4, max_orders=256, device=0, beam="plane", azimuths=None,
                 view_azimuths=None, devices=None, first_order="coded", gas_tau=None, view_mu=None, view_levels=(0, -1),
                 view_quadrature="grid", brightness=True) -> BandResult:
    """LONGWAVE FLUXES AND HEATING RATES SUMMED OVER K SPECTRAL POINTS, for C columns: sum_k weights[k] x (the thermal solve of
    point k with the Planck radiance of band k as its source), in W m-2 (the heating rate in the epilogue's unit per W m-2).

    `bands`: (nu_lo [K], nu_hi [K]) in cm^-1 (`wavenumber_bands`) or an array [K, 2].  `temperature` [L] or [C, L] (kelvin, at
    the levels np.linspace(z0, 0, nb_layers)), `surface_temperature`.  Per-point arguments -- tauStar_aer, tauStar_atm, alb_atm,
    alb_aer, weights (default 1; a k-distribution's g-point weights) -- are scalars, [K] or [K, C]; per-column arguments --
    grd_alb, surface_temperature, surface_emissivity (default 1 - grd_alb) -- scalars or [C].  The geometry and phase keywords are
    those of `thermal.thermal_toa_flux`.

    Pipeline, all on the device: `Solver.planck_bands_device` with normalise = 1 (the order loop needs a source of order 1: the
    module's docstring); the thermal solve of P C columns per chunk of P points, the field left on the device;
    `epilogue_emission_device`; `band_reduce_device` with the weights and the Planck stage's scales, accumulating over the
    chunks.  Only the summed arrays, `n`, `status` and `scale` cross PCIe (with per_point=True also every point's net_toa).

    `points_per_solve` = P: the points of one solve.  Default: as many as keep one field buffer P C L 2N 8 bytes within
    BAND_FIELD_BYTES (1 GiB), at least 1, at most K.  The result has the same bits for every P: a column's solve does not depend
    on its batch, and the sum adds the points in ascending order one fused multiply-add each, however they are chunked.

    A status != 0 raises as `thermal_toa_flux` does.  ValueError before any handle exists: `want` with 'diffusivity' (a ratio,
    not additive); beam='spherical', azimuths, view_azimuths, devices, first_order='readme'; shapes that do not broadcast to
    [K, C]; bands with nu_hi <= nu_lo; temperatures <= 0.  ValueError after the Planck stage, before any solve: a (band, column)
    whose radiances all underflow to 0 (a band far in the Wien tail of a cold column, x = 100 h c nu / (k T) above about 745),
    which the stage cannot normalise (scale 0).

    `gas_tau` [K, L] or [K, C, L] (default None, the code path as it was): EVERY SPECTRAL POINT ITS OWN GAS ABSORPTION PROFILE
    (DESIGN section 29), the cumulative absorption optical depth of the gases at the levels for that point -- 0 at the top, finite,
    non-decreasing.  Point k is solved on tau0 + gas_tau[k] with the row weights of `inputs.gas_row_weights` in its emission
    coefficient and its source function (`main.solve_profile`), so the heating rate gets the vertical structure of the gas.

    `view_mu` [V] (default None, the code path as it was): THE CHANNEL'S RADIANCE AT VIEW ANGLES.  Per chunk
    the view stage of `SOS_Aer_batch(source='thermal', view_mu=...)` runs on the resident field -- the emission at the lanes
    plus the scattered term, under `gas_tau` the weighted entries of `gas_view=True`, while the weights are set -- and both terms
    are summed over the points like the fluxes, with the weights and the scales: `view_mu_signed` [2V], `I_view_first`,
    `I_view_scattered` and `I_view` [C, nlev, 2V] in W m-2 sr-1, the lanes and `view_levels` / `view_quadrature` as in
    `SOS_Aer_batch`; the same bits for every `points_per_solve`.  `brightness=True` adds `brightness_temperature` [C, nlev, 2V],
    kelvin, from `Solver.brightness_temperature_device` on the summed `I_view` with `weights` and `bands` (NaN where the radiance
    is 0: the downward lanes at the top).  `per_point=True` adds `point_I_view` [K, C, nlev, 2V].  `want=()` is then allowed: no
    epilogue runs.  Refused before any handle exists: a surface other than 'specular'; what the view stage refuses
    (`main._view_args`); with brightness=True more than 64 bands, and weights that are negative or all zero in a column."""
    view = _view_points(view_mu, view_levels, view_quadrature, int(nb_layers), surface, atm_phase_fun, aer_phase_fun)
    want = _refuse(want, beam, azimuths, view_azimuths, devices, first_order, views=view is not None)
    L, N = int(nb_layers), int(nb_angles)
    lo, hi, T, Ts, pp, rho, es = _thermal_inputs(bands, temperature, surface_temperature, tauStar_aer, grd_alb, tauStar_atm, alb_atm,
                                                 alb_aer, weights, surface_emissivity, L)
    K, C = pp["weights"].shape
    brightness = _brightness_args(brightness, view, pp["weights"], K)
    gas_all = _gas_points(gas_tau, K, C, L)
    P = _points_per_solve(points_per_solve, K, C, L, N)
    import torch
    s = main.get_solver(L, N, P * C, max_orders, device)
    with main._on_torch_stream(s, device) as dev:
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dev)      # (a copy: broadcast inputs are read-only)
        d_pl = torch.empty((K, C, L), dtype=torch.float64, device=dev)
        d_bs = torch.empty((K, C), dtype=torch.float64, device=dev)
        d_scale = torch.empty((K, C), dtype=torch.float64, device=dev)
        d_w, d_T, d_Ts = up(pp["weights"]), up(T), up(Ts)
        d_es = None if es is None else up(np.tile(es, P))
        d_z = up(np.linspace(z0, 0, L)) if "heating_rate" in want else None
        acc = _Sum(torch, dev, want, per_point, P * C, C, L)
        vw = None if view is None else _Views(torch, dev, view, (atm_phase_fun, g_atm, mie_atm, aer_phase_fun, g_aer, mie_aer),
                                              device, C, per_point)
        s.planck_bands_device(d_T.data_ptr(), d_Ts.data_ptr(), lo, hi, d_pl.data_ptr(), d_bs.data_ptr(), d_scale.data_ptr(), C=C)
    scale = d_scale.cpu().numpy()
    if not np.all(scale > 0):
        k, c = [int(i) for i in np.argwhere(~(scale > 0))[0]]
        raise ValueError("band %d = [%g, %g] cm^-1 has no Planck radiance in double precision at the temperatures of column %d "
                         "(every value underflows to 0, scale = %r): there is no source to normalise; leave the band out"
                         % (k, lo[k], hi[k], c, float(scale[k, c])))

    def sources(k0, k1, B):
        return d_pl[k0:k1].reshape(B, L), d_bs[k0:k1].reshape(B), None if d_es is None else d_es[:B]

    def solve_chunk(k0, k1, B):
        flat = lambda a: a[k0:k1].reshape(B)
        # (checked by _gas_points: the namespace _prepare_batch fills, as main._gas_args returns it)
        gas = None if gas_all is None else SimpleNamespace(gas_tau=gas_all[k0:k1].reshape(B, L), tau0=None, w=None)
        _, tau, _, _, _, _, _, _ = main._prepare_batch(
            np.full(B, 0.5), flat(pp["tauStar_aer"]), np.tile(rho, k1 - k0), flat(pp["tauStar_atm"]), flat(pp["alb_atm"]),
            flat(pp["alb_aer"]), z0, z_up, z_down, L, N, atm_phase_fun, g_atm, aer_phase_fun, g_aer, mie_atm, mie_aer, None, None,
            None, None, surface, max_orders, device, gas=gas)
        if gas is not None:
            # the view stage on the resident field, while the weights are set (as gas_view=True of SOS_Aer_batch)
            gas_views = lambda dev, d_tau, d_I, d_sigma, B: vw.stage(s, d_tau, d_I, np.full(B, 0.5), thermal=sources(k0, k1, B),
                                                                     profile=True)
            return main.solve_profile(s, tau, None, None, gas.w, thermal=sources(k0, k1, B), tol=tol, keep_device=True,
                                      device=device, post=None if vw is None else gas_views)
        return main.solve_thermal(s, tau, *sources(k0, k1, B), tol=tol, keep_device=True, device=device)

    def epilogue(d, acc, B):
        s.epilogue_emission_device(d["tau"].data_ptr(), d["I"].data_ptr(), 0 if d_z is None else d_z.data_ptr(),
                                   acc.ptr("flux_down"), acc.ptr("flux_up"), 0, acc.ptr("heating_rate"), acc.ptr("net_toa"), B=B)

    def view_stage(d, k0, k1, B):
        if gas_all is None:
            vw.stage(s, d["tau"], d["I"], np.full(B, 0.5), thermal=sources(k0, k1, B))

    n, status, point = _sum_points(s, device, acc, P, d_w, d_scale, solve_chunk, epilogue, N, max_orders, vw, view_stage)
    r = BandResult(n=n, status=status, scale=scale, point_net_toa=None if point is None else point * scale, **acc.result())
    if vw is not None:
        d_Tb = None
        with main._on_torch_stream(s, device):
            d_view = vw.first + vw.scat
            if brightness:
                d_Tb = torch.empty_like(d_view)
                s.brightness_temperature_device(d_view.data_ptr(), d_Tb.data_ptr(), lo, hi, C, vw.M, d_w.data_ptr())
        _view_result(r, vw, d_view, scale)
        r.brightness_temperature = None if d_Tb is None else d_Tb.cpu().numpy()
    return r


def band_thermal_forcing(bands, temperature, surface_temperature, tauStar_aer, grd_alb, *, tauStar_atm, alb_atm, alb_aer,
                         weights=None, surface_emissivity=None, nb_layers=200, gas_tau=None, **kw):
    """Band-integrated longwave forcing of the aerosol layer, [C] in W m-2: the band-summed outgoing flux of the same columns
    with tauStar_aer = 0 minus the one with the layer -- positive where the layer keeps radiation in, the sign of
    `thermal.thermal_forcing` and `forcing.radiative_forcing`.  The columns with and without the layer are one batch of 2 C
    columns per point (`band_thermal`, its arguments; `want` and `per_point` are the driver's own)."""
    for k in ("want", "per_point"):
        if k in kw:
            raise ValueError("band_thermal_forcing sets %s itself" % k)
    _refuse(("flux_up",), kw.get("beam", "plane"), kw.get("azimuths"), kw.get("view_azimuths"), kw.get("devices"),
            kw.get("first_order", "coded"))
    lo, hi, T, Ts, pp, rho, es = _thermal_inputs(bands, temperature, surface_temperature, tauStar_aer, grd_alb, tauStar_atm, alb_atm,
                                                 alb_aer, weights, surface_emissivity, nb_layers)
    C = rho.size
    two = lambda a: np.concatenate((a, a), axis=-1)
    gas_all = _gas_points(gas_tau, lo.size, C, int(nb_layers))
    if gas_all is not None:
        kw["gas_tau"] = np.concatenate((gas_all, gas_all), axis=1)       # (the columns without the layer keep the gas)
    r = band_thermal((lo, hi), np.concatenate((T, T)), two(Ts), np.concatenate((pp["tauStar_aer"], np.zeros_like(pp["tauStar_aer"])), axis=1),
                     two(rho), tauStar_atm=two(pp["tauStar_atm"]), alb_atm=two(pp["alb_atm"]), alb_aer=two(pp["alb_aer"]),
                     weights=two(pp["weights"]), surface_emissivity=None if es is None else two(es), want=("flux_up",),
                     nb_layers=nb_layers, **kw)
    return r.flux_up[C:, 0] - r.flux_up[:C, 0]


# ---- the solar driver ---------------------------------------------------------------------------------------------------------------
def _solar_inputs(solar_flux, mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer, aer_phase_fun, point_aerosol, beam_norm):
    w = _array(solar_flux, "solar_flux")
    if w.ndim not in (1, 2) or w.shape[0] < 1:
        raise ValueError("solar_flux must be [K] or [K, C]: one weight per spectral point (got shape %s)" % (w.shape,))
    K = w.shape[0]
    if beam_norm not in ("crit", "graphe"):
        raise ValueError("beam_norm must be 'crit' or 'graphe' (got %r)" % (beam_norm,))
    pp = dict(solar_flux=w, tauStar_aer=_array(tauStar_aer, "tauStar_aer"), tauStar_atm=_array(tauStar_atm, "tauStar_atm"),
              alb_atm=_array(alb_atm, "alb_atm"), alb_aer=_array(alb_aer, "alb_aer"))
    pc = dict(mu0=_array(mu0, "mu0"), grd_alb=_array(grd_alb, "grd_alb"))
    C = _widths(K, pp, pc)
    pp = {k: _per_point(v, K, C, k) for k, v in pp.items()}
    pc = {k: _per_column(v, C, k) for k, v in pc.items()}
    sets = None
    if isinstance(aer_phase_fun, (list, tuple)):
        if len(aer_phase_fun) > _lib.MAX_PHASE_SETS:
            raise ValueError("aer_phase_fun names %d aerosols, a batch takes at most MAX_PHASE_SETS = %d" % (len(aer_phase_fun), _lib.MAX_PHASE_SETS))
        if point_aerosol is None:
            raise ValueError("a list of aerosols in aer_phase_fun needs point_aerosol [K]: the aerosol of every spectral point")
        sets = np.asarray(point_aerosol)
        if sets.shape != (K,) or not np.issubdtype(sets.dtype, np.integer):
            raise ValueError("point_aerosol must be [K] = %d integers (got shape %s)" % (K, sets.shape))
        if sets.min() < 0 or sets.max() >= len(aer_phase_fun):
            raise ValueError("point_aerosol names aerosol %d, aer_phase_fun has %d" % (int(sets.max() if sets.max() >= len(aer_phase_fun)
                                                                                           else sets.min()), len(aer_phase_fun)))
    elif point_aerosol is not None:
        raise ValueError("point_aerosol belongs to a list of aerosol names in aer_phase_fun")
    return pp, pc["mu0"], pc["grd_alb"], sets


def band_solar(solar_flux, mu0, tauStar_aer, grd_alb, *, tauStar_atm, alb_atm, alb_aer, beam_norm="crit", want=WANT,
               points_per_solve=None, per_point=False, point_aerosol=None, z0=120, z_up=25, z_down=17, nb_layers=200, nb_angles=128,
               atm_phase_fun="rayleigh", g_atm=0.0, aer_phase_fun="hg", g_aer=0.7, mie_atm=None, mie_aer=None, surface="specular",
               tol=1e-4, max_orders=256, device=0, beam="plane", azimuths=None, view_azimuths=None, devices=None,
               first_order="coded", gas_tau=None, view_mu=None, view_levels=(0, -1), view_quadrature="grid") -> BandResult:
    """SHORTWAVE FLUXES AND HEATING RATES SUMMED OVER K SPECTRAL POINTS, for C columns: sum_k solar_flux[k] x (the epilogue of
    the solar solve of point k).  `solar_flux` [K] or [K, C] is the weight of every point; mu0 and grd_alb are per column
    (scalars or [C]); tauStar_aer, tauStar_atm, alb_atm and alb_aer per point (scalars, [K] or [K, C]).

    The weights multiply the per-point epilogue outputs EXACTLY AS THE EPILOGUE DEFINES THEM (`Solver.epilogue`): the solve
    carries the reference's incident flux F0 = pi / mu0, and `beam_norm` picks one of its two normalisations of the direct beam
    in the fluxes ('crit': crit:377-382, 'graphe': graphe:74-91).  Turning solar_flux[k] into a physical irradiance per unit of
    those outputs (a factor mu0 E_k / pi for a band irradiance E_k on a plane normal to the sun) is left to the caller.

    `aer_phase_fun` may be a list of names (with `g_aer` / `mie_aer` single values or lists of its length) and `point_aerosol`
    [K] the aerosol of every point: the driver makes them the `aer_set` of the batch, at most MAX_PHASE_SETS.  The atmosphere's
    phase function is the same for all points.  Pipeline: `solve_batch_device` of P C columns per chunk, `epilogue_device`,
    `band_reduce_device` (no scale); `points_per_solve`, `per_point`, `want` and the refusals as `band_thermal`.
    `gas_tau` [K, L] or [K, C, L]: every spectral point its own gas absorption profile, as in `band_thermal` (the solar first
    order layer by layer with the weights in its scattering coefficient, the beam terms of the fluxes on the total tau).

    `view_mu` [V] (default None, the code path as it was): THE CHANNEL'S RADIANCE AT VIEW ANGLES, as in
    `band_thermal`: per chunk the view stage of `SOS_Aer_batch(view_mu=...)` on the resident field -- the closed-form first
    order plus the scattered term, under `gas_tau` the weighted entries of `gas_view=True` on sigma = tau / mu0 -- each term summed
    with solar_flux[k, c] exactly as the epilogue outputs are (no scale): `view_mu_signed`, `I_view_first`, `I_view_scattered`,
    `I_view` [C, nlev, 2V], with per_point=True `point_I_view` [K, C, nlev, 2V]; `want=()` is then allowed.  The sums carry the
    solve's F0 = pi / mu0 like the fluxes: the factor mu0 E_k / pi in solar_flux[k] makes them a radiance in the unit of E_k per
    steradian.  No brightness temperature is formed.  Refused besides: a surface other than 'specular', and a list of aerosols
    (`point_aerosol`) -- the view stage reads one aerosol phase function."""
    view = _view_points(view_mu, view_levels, view_quadrature, int(nb_layers), surface, atm_phase_fun, aer_phase_fun, point_aerosol)
    want = _refuse(want, beam, azimuths, view_azimuths, devices, first_order, views=view is not None)
    L, N = int(nb_layers), int(nb_angles)
    pp, mu0c, rho, sets = _solar_inputs(solar_flux, mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer, aer_phase_fun,
                                        point_aerosol, beam_norm)
    K, C = pp["solar_flux"].shape
    gas_all = _gas_points(gas_tau, K, C, L)
    P = _points_per_solve(points_per_solve, K, C, L, N)
    import torch
    s = main.get_solver(L, N, P * C, max_orders, device)
    dev = torch.device("cuda", device)
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dev)      # (a copy: broadcast inputs are read-only)
    d_w = up(pp["solar_flux"])
    d_z = up(np.linspace(z0, 0, L)) if "heating_rate" in want else None
    acc = _Sum(torch, dev, want, per_point, P * C, C, L)
    vw = None if view is None else _Views(torch, dev, view, (atm_phase_fun, g_atm, mie_atm, aer_phase_fun, g_aer, mie_aer), device,
                                          C, per_point)

    def solve_chunk(k0, k1, B):
        flat = lambda a: a[k0:k1].reshape(B)
        tile = lambda a: np.tile(a, k1 - k0)
        # the view stage on the resident field, while the weights are set (as gas_view=True of SOS_Aer_batch)
        gas_views = lambda dev, d_tau, d_I, d_sigma, B: vw.stage(s, d_tau, d_I, tile(mu0c), sigma=d_sigma, profile=True)
        # (the handle's stream, its columns and their aerosol sets are solve_batch_device's to set and to put back)
        return main.solve_batch_device(
            tile(mu0c), flat(pp["tauStar_aer"]), tile(rho), tauStar_atm=flat(pp["tauStar_atm"]), alb_atm=flat(pp["alb_atm"]),
            alb_aer=flat(pp["alb_aer"]), z0=z0, z_up=z_up, z_down=z_down, nb_layers=L, nb_angles=N, atm_phase_fun=atm_phase_fun,
            g_atm=g_atm, aer_phase_fun=aer_phase_fun, g_aer=g_aer, mie_atm=mie_atm, mie_aer=mie_aer, surface=surface, tol=tol,
            max_orders=max_orders, device=device, aer_set=None if sets is None else np.repeat(sets[k0:k1], C),
            gas_tau=None if gas_all is None else gas_all[k0:k1].reshape(B, L),
            profile_post=None if vw is None or gas_all is None else gas_views)[0]

    def epilogue(d, acc, B):
        s.epilogue_device(d["tau"].data_ptr(), d["I"].data_ptr(), 0 if d_z is None else d_z.data_ptr(), beam_norm,
                          acc.ptr("flux_down"), acc.ptr("flux_up"), 0, acc.ptr("heating_rate"), acc.ptr("net_toa"))

    def view_stage(d, k0, k1, B):
        if gas_all is None:
            vw.stage(s, d["tau"], d["I"], np.tile(mu0c, k1 - k0))

    n, status, point = _sum_points(s, device, acc, P, d_w, None, solve_chunk, epilogue, N, max_orders, vw, view_stage)
    r = BandResult(n=n, status=status, point_net_toa=point, **acc.result())
    if vw is not None:
        with main._on_torch_stream(s, device):
            d_view = vw.first + vw.scat
        _view_result(r, vw, d_view)
    return r


def band_solar_forcing(solar_flux, mu0, tauStar_aer, grd_alb, *, tauStar_atm, alb_atm, alb_aer, beam_norm="crit",
                       aer_phase_fun="hg", point_aerosol=None, gas_tau=None, **kw):
    """Band-integrated shortwave forcing of the aerosol layer, [C]: the band-summed TOA net flux with the layer minus the one of
    the same columns with tauStar_aer = 0, the sign of `forcing.radiative_forcing` (the weights as `band_solar` defines them).
    The columns with and without the layer are one batch of 2 C columns per point."""
    for k in ("want", "per_point"):
        if k in kw:
            raise ValueError("band_solar_forcing sets %s itself" % k)
    _refuse(("net_toa",), kw.get("beam", "plane"), kw.get("azimuths"), kw.get("view_azimuths"), kw.get("devices"),
            kw.get("first_order", "coded"))
    pp, mu0c, rho, sets = _solar_inputs(solar_flux, mu0, tauStar_aer, grd_alb, tauStar_atm, alb_atm, alb_aer, aer_phase_fun,
                                        point_aerosol, beam_norm)
    C = rho.size
    two = lambda a: np.concatenate((a, a), axis=-1)
    gas_all = _gas_points(gas_tau, pp["solar_flux"].shape[0], C, int(kw.get("nb_layers", 200)))
    if gas_all is not None:
        kw["gas_tau"] = np.concatenate((gas_all, gas_all), axis=1)       # (the columns without the layer keep the gas)
    r = band_solar(two(pp["solar_flux"]), two(mu0c), np.concatenate((pp["tauStar_aer"], np.zeros_like(pp["tauStar_aer"])), axis=1),
                   two(rho), tauStar_atm=two(pp["tauStar_atm"]), alb_atm=two(pp["alb_atm"]), alb_aer=two(pp["alb_aer"]),
                   beam_norm=beam_norm, aer_phase_fun=aer_phase_fun, point_aerosol=point_aerosol, want=("net_toa",), **kw)
    return r.net_toa[:C] - r.net_toa[C:]
