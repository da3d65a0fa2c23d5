"""NumPy model of the pseudo-spherical beam at view lanes, written from the definitions of DESIGN section 17
and not from the kernel: the recurrences of spherical_np.first_order_beam with a direction's |mu_m| replaced by the lane's view
cosine.

View cosines `mu_view` [V] in [0.01, 1]; signed lanes s = (-mu_view, +mu_view), the mirror of lane j is j +- V; p0 rows [2V] on
those lanes.  There is no mu = 0 lane and no limit branch: phi is exact where a view cosine equals mu0."""
import dataclasses

import numpy as np

import azimuth_direct as AD
import sos_oracle as O
import spherical_np as S


def zone_q_rows(c, p0a, p0r):
    """q [nz][2V] of the column's zones from the p0 rows at the lanes: clear w_atm p0a / (4 pi); aerosol
    (w_atm p0a f_atm + w_aer p0r f_aer) / (4 pi)."""
    p0a, p0r = np.asarray(p0a, dtype=np.float64), np.asarray(p0r, dtype=np.float64)
    out = []
    for z in c.zones:
        if z.kind != "mix":
            out.append(c.alb_atm * p0a / (4 * np.pi))
        else:
            fa, fr = c.zone_fractions(z)
            out.append((c.alb_atm * p0a * fa + z.alb_aer * p0r * fr) / (4 * np.pi))
    return out


def view_first_order_beam(c, sigma, p0a, p0r, mu_view, dtype=np.float64):
    """The first order of column `c` (oracle.Column) on the beam path sigma [L] at the signed lanes of `mu_view`: [L][2V].
    dtype: the type every operation runs in (np.longdouble: the same formulas, to measure what float64 loses)."""
    tau, mu0 = np.asarray(c.tau, dtype=dtype), dtype(c.mu0)
    sigma = np.asarray(sigma, dtype=dtype)
    a = np.asarray(mu_view, dtype=dtype)
    L, V = tau.size, a.size
    F0 = dtype(np.pi) / mu0
    T = dtype(c.tauStar_tot)
    R = F0 * c.grd_alb * np.exp(-sigma[L - 1] - (T - tau[L - 1]) / mu0)
    zones = c.zones
    qz = [np.asarray(q, dtype=dtype) for q in zone_q_rows(c, p0a, p0r)]
    zone_of = np.zeros(L, dtype=int)
    first_row, last_row = np.zeros(L, dtype=bool), np.zeros(L, dtype=bool)
    for zi, z in enumerate(zones):
        zone_of[z.r0:z.r1 + 1] = zi
        if zi > 0:
            first_row[z.r0] = True               # first row of a zone below the top one
        if zi < len(zones) - 1:
            last_row[z.r1] = True                # last row of a zone above the bottom one
    lo, hi = np.arange(V), V + np.arange(V)      # the downward lanes and their mirrors
    e_dir = F0 * np.exp(-sigma)                  # F0 e^{-sigma_t}
    e_ref = R * np.exp(-(T - tau) / mu0)         # R e^{-(T - tau_t) / mu0}
    out = np.zeros((L, 2 * V), dtype=dtype)
    with np.errstate(all="ignore"):
        # downward, D_0 = 0; layer (t-1, t) takes the q of row t
        Dn = np.zeros(V, dtype=dtype)
        for t in range(1, L):
            q = qz[zone_of[t]]
            dl = tau[t] - tau[t - 1]
            ds = sigma[t] - sigma[t - 1]
            E = np.exp(-dl / a)
            Dn = Dn * E + q[lo] * e_dir[t] * (dl / a) * S.phi(dl / a - ds, dtype)
            if not first_row[t]:
                Dn = Dn + q[hi] * e_ref[t] * (dl / a) * S.phi((1 / a + 1 / mu0) * dl, dtype)
            out[t, lo] = Dn
        # surface and upward; layer (t, t+1) takes the q of row t
        Up = c.grd_alb * out[L - 1, lo]
        out[L - 1, hi] = Up
        for t in range(L - 2, -1, -1):
            q = qz[zone_of[t]]
            dl = tau[t + 1] - tau[t]
            ds = sigma[t + 1] - sigma[t]
            E = np.exp(-dl / a)
            Up = Up * E + q[hi] * e_dir[t] * (dl / a) * S.phi(dl / a + ds, dtype)
            if not last_row[t]:
                Up = Up + q[lo] * e_ref[t] * (dl / a) * S.phi(dl / a - dl / mu0, dtype)
            out[t, hi] = Up
    return out


def sphere_geometry(mu0, L, N):
    """azimuth_direct.three_zone's column with the first order on the sphere's beam path, so that azimuth_direct.mode_fields and
    direct_solve share it: (Geometry, sigma [L])."""
    Z1, Z2 = np.zeros(2 * N), np.zeros((2 * N, 2 * N))
    c = O.make_column(mu0, 120, 25, 17, L, 0.124, 0.3, 0.15, 1.0, 0.95, N, Z1, Z2, Z1, Z2)
    sig = S.slant_path(c.tau, S.altitudes(L), mu0)
    geo = AD.three_zone(mu0, L, N)
    first = lambda P0a, P0r: S.first_order_beam(dataclasses.replace(c, P0_atm=P0a, P0_aer=P0r), sig)
    return dataclasses.replace(geo, first=first), sig
