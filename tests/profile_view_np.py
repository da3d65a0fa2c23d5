"""NumPy model of per-level weights in the view stage, written from the definitions on the existing models
and not from the kernels:

    view_source_profile        the weighted sum of the two constituents of view_np.source (profile_np.split), row by row
    view_first_order_profile   spherical_view_np.view_first_order_beam with q of a ROW (profile_np.row_q's expression on the p0 rows)
    emission_view_profile      thermal_np._sweeps at the view cosines with profile_np.row_eps

View cosines `mu_view` [V] in [0.01, 1]; signed lanes s = (-mu_view, +mu_view), the mirror of lane j is j +- V."""
import numpy as np

import profile_np as P
import spherical_np as S
import thermal_np as T
import view_np as VN


def solve_column_last(O, c, w_atm, w_aer, I1, tol=1e-4, max_orders=10000):
    """profile_np.solve_column's loop, returning what the view stage's node identity needs: (I, the last order I_last, n)."""
    In_1 = I1
    I = I1.copy()
    In = np.ones_like(I1)
    n = 1
    while True:
        r = O.convergence_ratio(In, I, c.N)
        if not (r >= tol) or n >= max_orders:
            break
        n += 1
        In = O.transport(c, P.source_function(O, c, In_1, w_atm, w_aer), literal=False)
        In_1 = In
        I = I + In
    return I, In, n


def view_source_profile(c, rows_atm, rows_aer, Isrc, w_atm, w_aer):
    """S [L, 2V] = w_atm[:, None] view_np.source(c with alb_aer = 0) + w_aer[:, None] view_np.source(c with alb_atm = 0)."""
    ca, cr = P.split(c)
    return (np.asarray(w_atm)[:, None] * VN.source(ca, rows_atm, rows_aer, Isrc)
            + np.asarray(w_aer)[:, None] * VN.source(cr, rows_atm, rows_aer, Isrc))


def row_q_rows(c, p0a, p0r, w_atm, w_aer):
    """q [L][2V] from the p0 rows at the lanes: (omega_atm w_atm,t p0a f_atm + omega_aer w_aer,t p0r f_aer) / 4 pi with the
    fractions of row t's zone (clear: f_atm = 1, no aerosol term)."""
    p0a, p0r = np.asarray(p0a, dtype=np.float64), np.asarray(p0r, dtype=np.float64)
    L = len(c.tau)
    q = np.zeros((L, p0a.size))
    zones, zone_of = c.zones, P.zone_of_rows(c)
    for t in range(L):
        z = zones[zone_of[t]]
        if z.kind != "mix":
            q[t] = (c.alb_atm * w_atm[t]) * p0a / (4 * np.pi)
        else:
            fa, fr = c.zone_fractions(z)
            q[t] = ((c.alb_atm * w_atm[t]) * p0a * fa + (z.alb_aer * w_aer[t]) * p0r * fr) / (4 * np.pi)
    return q


def view_first_order_profile(c, sigma, p0a, p0r, mu_view, w_atm, w_aer, dtype=np.float64):
    """The first order of column `c` on the beam path sigma [L] at the signed lanes of `mu_view`, with q of a row: [L][2V].
    The recurrences, the two exclusions, R and phi of spherical_view_np.view_first_order_beam.  dtype: the type every operation
    runs in (np.longdouble: the same formulas, to measure what float64 loses)."""
    tau, mu0 = np.asarray(c.tau, dtype=dtype), dtype(c.mu0)
    sigma = np.asarray(sigma, dtype=dtype)
    a = np.asarray(mu_view, dtype=dtype)
    L, V = tau.size, a.size
    F0 = dtype(np.pi) / mu0
    Tt = dtype(c.tauStar_tot)
    R = F0 * c.grd_alb * np.exp(-sigma[L - 1] - (Tt - tau[L - 1]) / mu0)
    zones = c.zones
    q = np.asarray(row_q_rows(c, p0a, p0r, w_atm, w_aer), dtype=dtype)
    first_row, last_row = np.zeros(L, dtype=bool), np.zeros(L, dtype=bool)
    for zi, z in enumerate(zones):
        if zi > 0:
            first_row[z.r0] = True               # first row of a zone below the top one
        if zi < len(zones) - 1:
            last_row[z.r1] = True                # last row of a zone above the bottom one
    lo, hi = np.arange(V), V + np.arange(V)
    e_dir = F0 * np.exp(-sigma)
    e_ref = R * np.exp(-(Tt - tau) / mu0)
    out = np.zeros((L, 2 * V), dtype=dtype)
    with np.errstate(all="ignore"):
        Dn = np.zeros(V, dtype=dtype)
        for t in range(1, L):
            dl = tau[t] - tau[t - 1]
            ds = sigma[t] - sigma[t - 1]
            E = np.exp(-dl / a)
            Dn = Dn * E + q[t, lo] * e_dir[t] * (dl / a) * S.phi(dl / a - ds, dtype)
            if not first_row[t]:
                Dn = Dn + q[t, hi] * e_ref[t] * (dl / a) * S.phi((1 / a + 1 / mu0) * dl, dtype)
            out[t, lo] = Dn
        Up = c.grd_alb * out[L - 1, lo]
        out[L - 1, hi] = Up
        for t in range(L - 2, -1, -1):
            dl = tau[t + 1] - tau[t]
            ds = sigma[t + 1] - sigma[t]
            E = np.exp(-dl / a)
            Up = Up * E + q[t, hi] * e_dir[t] * (dl / a) * S.phi(dl / a + ds, dtype)
            if not last_row[t]:
                Up = Up + q[t, lo] * e_ref[t] * (dl / a) * S.phi(dl / a - dl / mu0, dtype)
            out[t, hi] = Up
    return out


def emission_view_profile(c, planck, planck_surface, mu_view, w_atm, w_aer, emissivity=None, dtype=np.float64):
    """[L][2V] on the signed lanes (-mu_view, +mu_view): thermal_np's sweeps at a = mu_view with the emission coefficient of a
    row; specular ground or none."""
    tau = np.asarray(c.tau, dtype=dtype)
    a = np.atleast_1d(np.asarray(mu_view, dtype=dtype))
    es = 1 - c.grd_alb if emissivity is None else float(emissivity)
    if c.surface not in ("specular", None):
        raise ValueError("the view lanes have no Lambertian ground")
    rho = c.grd_alb if c.surface == "specular" else 0.0
    D, U = T._sweeps(tau, np.asarray(planck, dtype=dtype), P.row_eps(c, w_atm, w_aer), a,
                     lambda down: rho * down + es * planck_surface, dtype)
    return np.concatenate((D, U), axis=1)
