"""NumPy model of per-level weights on the source function, written from the definitions and not from the
kernels, on the oracle's unchanged functions: the order loop of oracle.solve_column with
    Jn = w_atm[:, None] source_function(c with alb_aer = 0) + w_aer[:, None] source_function(c with alb_atm = 0),
the per-row generalisation of spherical_np.first_order_beam, the per-row generalisation of thermal_np.emission, and the rule
that turns a gas absorption profile into weights."""
import dataclasses

import numpy as np

import spherical_np as S
import thermal_np as T


def _with_albedos(c, alb_atm, aer_scale):
    """Column c with the atmosphere's albedo `alb_atm` and every aerosol albedo times `aer_scale` (its zone table included)."""
    zt = c.zone_table
    if zt is not None:
        zt = [dataclasses.replace(z, alb_aer=z.alb_aer * aer_scale) for z in zt]
    return dataclasses.replace(c, alb_atm=alb_atm, alb_aer=c.alb_aer * aer_scale, zone_table=zt)


def split(c):
    """(c with alb_aer = 0, c with alb_atm = 0): the two constituents of the source function."""
    return _with_albedos(c, c.alb_atm, 0.0), _with_albedos(c, 0.0, 1.0)


def scaled(c, w):
    """The column a constant weight w stands for: both albedos times w, the column unchanged otherwise."""
    return _with_albedos(c, c.alb_atm * w, w)


def source_function(O, c, In_1, w_atm, w_aer):
    ca, cr = split(c)
    return np.asarray(w_atm)[:, None] * O.source_function(ca, In_1) + np.asarray(w_aer)[:, None] * O.source_function(cr, In_1)


def solve_column(O, c, w_atm, w_aer, I1, tol=1e-4, max_orders=10000, literal=False):
    """oracle.solve_column's loop (spec:301-458) with the weighted source function, from the first order I1."""
    In_1 = I1
    I = I1.copy()
    In = np.ones_like(I1)
    n = 1
    while True:
        r = O.convergence_ratio(In, I, c.N)
        if not (r >= tol) or n >= max_orders:
            break
        n += 1
        In = O.transport(c, source_function(O, c, In_1, w_atm, w_aer), literal=literal)
        In_1 = In
        I = I + In
    return O.Solution(I=I, I_saved=np.zeros((0,) + I.shape), n=n)


def zone_of_rows(c):
    zone_of = np.zeros(len(c.tau), dtype=int)
    for zi, z in enumerate(c.zones):
        zone_of[z.r0:z.r1 + 1] = zi
    return zone_of


def row_q(c, w_atm, w_aer, P0_aer_zone=None):
    """q [L][2N]: (omega_atm f_atm w_atm,t P0_atm + omega_aer f_aer w_aer,t P0_aer) / 4 pi with the fractions of row t's zone
    (clear: f_atm = 1, no aerosol term)."""
    L = len(c.tau)
    q = np.zeros((L, 2 * c.N))
    zones, zone_of = c.zones, zone_of_rows(c)
    for t in range(L):
        z = zones[zone_of[t]]
        if z.kind != "mix":
            q[t] = (c.alb_atm * w_atm[t]) * c.P0_atm / (4 * np.pi)
        else:
            fa, fr = c.zone_fractions(z)
            pr = c.P0_aer if P0_aer_zone is None else P0_aer_zone[zone_of[t]]
            q[t] = ((c.alb_atm * w_atm[t]) * c.P0_atm * fa + (z.alb_aer * w_aer[t]) * pr * fr) / (4 * np.pi)
    return q


def first_order_profile(c, sigma, w_atm, w_aer, P0_aer_zone=None, dtype=np.float64):
    """spherical_np.first_order_beam with q of a ROW: the same recurrences, level choices, exclusions, R, phi and mu = 0 lane.
    dtype: the type every operation runs in (np.longdouble: the same formulas, to measure what float64 loses)."""
    tau, mu, N, mu0 = np.asarray(c.tau, dtype=dtype), np.asarray(c.mu, dtype=dtype), c.N, dtype(c.mu0)
    sigma = np.asarray(sigma, dtype=dtype)
    L, D = tau.size, 2 * N
    F0 = dtype(np.pi) / mu0
    Tt = dtype(c.tauStar_tot)
    R = F0 * c.grd_alb * np.exp(-sigma[L - 1] - (Tt - tau[L - 1]) / mu0)
    zones = c.zones
    q = np.asarray(row_q(c, w_atm, w_aer, P0_aer_zone), dtype=dtype)
    first_row, last_row = np.zeros(L, dtype=bool), np.zeros(L, dtype=bool)
    for zi, z in enumerate(zones):
        if zi > 0:
            first_row[z.r0] = True
        if zi < len(zones) - 1:
            last_row[z.r1] = True
    mirror = D - 1 - np.arange(D)
    e_dir = F0 * np.exp(-sigma)
    e_ref = R * np.exp(-(Tt - tau) / mu0)
    I1 = np.zeros((L, D), dtype=dtype)
    with np.errstate(all="ignore"):
        a = np.abs(mu[:N])
        Dn = np.zeros(N, dtype=dtype)
        for t in range(1, L):
            dl = tau[t] - tau[t - 1]
            s = (sigma[t] - sigma[t - 1]) / dl
            E = np.exp(-dl / a)
            Dn = Dn * E + q[t, :N] * e_dir[t] * (dl / a) * S.phi((1 / a - s) * dl, dtype)
            if not first_row[t]:
                Dn = Dn + q[t, mirror[:N]] * e_ref[t] * (dl / a) * S.phi((1 / a + 1 / mu0) * dl, dtype)
            I1[t, :N] = Dn
        a = np.abs(mu[N:])
        Up = c.grd_alb * I1[L - 1, mirror[N:]]
        I1[L - 1, N:] = Up
        for t in range(L - 2, -1, -1):
            dl = tau[t + 1] - tau[t]
            s = (sigma[t + 1] - sigma[t]) / dl
            E = np.exp(-dl / a)
            Up = Up * E + q[t, N:] * e_dir[t] * (dl / a) * S.phi((1 / a + s) * dl, dtype)
            if not last_row[t]:
                Up = Up + q[t, mirror[N:]] * e_ref[t] * (dl / a) * S.phi((1 / a - 1 / mu0) * dl, dtype)
            I1[t, N:] = Up
    for t in range(L):
        for m in (N - 1, N):
            I1[t, m] = q[t, m] * e_dir[t] + q[t, mirror[m]] * e_ref[t]
    return I1


def row_eps(c, w_atm, w_aer):
    """eps [L] = 1 - (omega_atm f_atm w_atm,t + omega_aer f_aer w_aer,t) with the fractions of row t's zone."""
    L = len(c.tau)
    eps = np.zeros(L)
    zones, zone_of = c.zones, zone_of_rows(c)
    for t in range(L):
        z = zones[zone_of[t]]
        if z.kind != "mix":
            eps[t] = 1 - (c.alb_atm * w_atm[t])
        else:
            fa, fr = c.zone_fractions(z)
            eps[t] = 1 - ((c.alb_atm * w_atm[t]) * fa + (z.alb_aer * w_aer[t]) * fr)
    return eps


def emission_profile(c, planck, planck_surface, w_atm, w_aer, emissivity=None, dtype=np.float64):
    """thermal_np.emission with the emission coefficient of a ROW: the same sweeps, the same boundary.  dtype: as in
    first_order_profile."""
    tau, mu, N = np.asarray(c.tau, dtype=dtype), c.mu, c.N
    b = np.asarray(planck, dtype=dtype)
    L = tau.size
    es = 1 - c.grd_alb if emissivity is None else float(emissivity)
    eps = row_eps(c, w_atm, w_aer)
    I0 = np.zeros((L, 2 * N), dtype=dtype)
    a = np.abs(mu[:N - 1])[::-1]

    def ground_of(down):
        full = np.zeros(N, dtype=dtype)
        full[:N - 1] = down[::-1]
        return T.boundary(c, full)[1:] + es * planck_surface

    D, U = T._sweeps(tau, b, eps, a, ground_of, dtype)
    I0[:, :N - 1] = D[:, ::-1]
    I0[:, N + 1:] = U
    I0[:, N - 1] = I0[:, N] = eps * b
    return I0


def gas_weights(tau0, gas):
    """(tau, w) of the rule, level by level: w_t = dtau0_t / (dtau0_t + dgas_t) for t >= 1, w_0 = w_1."""
    tau0, gas = np.asarray(tau0, dtype=np.float64), np.asarray(gas, dtype=np.float64)
    L = tau0.size
    w = np.ones(L)
    for t in range(1, L):
        d0, dg = tau0[t] - tau0[t - 1], gas[t] - gas[t - 1]
        w[t] = d0 / (d0 + dg) if d0 + dg > 0 else 1.0
    w[0] = w[1]
    return tau0 + gas, w


def with_gas(c, gas):
    """(the column on tau0 + gas with tauStar_tot including the gas, w): dtau_atm / dtau_aer stay the scattering column's."""
    tau, w = gas_weights(c.tau, gas)
    return dataclasses.replace(c, tau=tau, tauStar_tot=c.tauStar_tot + float(np.asarray(gas)[-1])), w


def stretched(c, w):
    """The scaled-albedo column of the constant-w identity: both albedos times w, every optical depth divided by w."""
    cs = scaled(c, w)
    zt = cs.zone_table
    if zt is not None:
        zt = [dataclasses.replace(z, dtau_aer=z.dtau_aer / w) for z in zt]
    return dataclasses.replace(cs, tau=c.tau / w, tauStar_tot=c.tauStar_tot / w, dtau_atm=c.dtau_atm / w, dtau_aer=c.dtau_aer / w,
                               zone_table=zt)


# ---- the columns of the tests: Rayleigh + Henyey-Greenstein g = 0.7, the atmosphere of spherical_np ----------------------------
def column(O, N, L, mu0, rho, slabs=None, surface="specular", g=0.7, alb_atm=1.0, alb_aer=0.97):
    c = S.column(O, N, L, mu0, rho, slabs, surface, g, alb_aer)
    return c if alb_atm == 1.0 else _with_albedos(c, alb_atm, 1.0)


def random_weights(c, seed, lo=0.2):
    """(w_atm [L], w_aer [L]) drawn independently in [lo, 1], with a jump exactly at the first and the last row of the first
    aerosol zone, and rows of exact 1.0 and exact 0.0."""
    rng = np.random.default_rng(seed)
    L = len(c.tau)
    wa, wr = rng.uniform(lo, 1.0, L), rng.uniform(lo, 1.0, L)
    z = next(z for z in c.zones if z.kind == "mix")
    wa[z.r0:] *= 0.5                                           # a jump at the zone's first row ...
    wr[z.r1 + 1:] = 1.0                                        # ... and behind its last one
    wa[z.r1] = 0.25 * wa[z.r1 - 1] if z.r1 > z.r0 else wa[z.r1]
    wa[1], wr[z.r0] = 1.0, 1.0
    wa[L - 2], wr[z.r1] = 0.0, 0.0
    return wa, wr
