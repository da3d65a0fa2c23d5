"""NumPy model of the view-radiance stage: what csrc/view.hip implements, written from the definitions
with the oracle's own building blocks (`sos_oracle._azimuth_average`, `np.trapz`, the formulas of `first_order` and
`I1_NumInt`).  tests/test_view_host.py pins it to the oracle at the nodes of the direction grid; tests/test_gpu_view.py
compares the device with it off the grid.

View cosines `mu_view` [V] in [0.01, 1]; signed lanes s = (-mu_view, +mu_view), the mirror of lane j is j +- V; every
output is ordered by j."""
import functools

import numpy as np

import sos_oracle as O

QUAD_GRID, QUAD_LINEAR = 0, 1
_trapz = O._trapz


def signed(mu_view):
    m = np.asarray(mu_view, dtype=np.float64)
    return np.concatenate((-m, m))


def phase_fn(kind, g=0.0, table=None):
    """p(cos Theta) of a kind of the builders ('iso' gives None: its rows are constants)."""
    if kind == "iso":
        return None
    if kind == "rayleigh":
        return lambda c: (3 / 4) * (1 + c * c)
    if kind == "hg":
        return lambda c: (1 - g * g) / ((1 + g * g - 2 * g * c) ** 1.5)
    if kind == "table":
        return lambda c: O.interpolate_table(table[0], table[1], c)
    raise ValueError(kind)


def phase_rows(fn, mu, s):
    """rows[j][n] = 4 ring(s_j, mu_n) / trapz_a ring(mu_a, mu_n): the stored matrix's rows at exit cosines s (phase:116-131)."""
    s = np.asarray(s, dtype=np.float64)
    if fn is None:
        return 2 * np.ones((len(s), len(mu)))
    return 4 * O._azimuth_average(fn, s, mu) / _trapz(O._azimuth_average(fn, mu, mu), mu, axis=0)[None, :]


def phase_p0_rows(fn, mu, mu0, s):
    """p0rows[b][j] = 2 ring(s_j, mu0_b) / trapz_a ring(mu_a, mu0_b) (phase:86-103)."""
    s = np.asarray(s, dtype=np.float64)
    mu0 = np.atleast_1d(np.asarray(mu0, dtype=np.float64))
    if fn is None:
        return np.ones((len(mu0), len(s)))
    return (2 * O._azimuth_average(fn, s, mu0) / _trapz(O._azimuth_average(fn, mu, mu0), mu, axis=0)[None, :]).T


def source(c, rows_atm, rows_aer, Isrc):
    """`oracle.source_function` with the matrices replaced by the rows: S [L, 2V]."""
    L = len(c.tau)
    S = np.zeros((L, rows_atm.shape[0]))
    Ra = rows_atm[:, ::-1]
    Rr = None if rows_aer is None else rows_aer[:, ::-1]
    for z in c.zones:
        for t in range(z.r0, z.r1 + 1):
            if z.kind == "mix":
                fa, fr = c.zone_fractions(z)
                S[t] = (c.alb_atm / 4) * _trapz(Ra * Isrc[t], c.mu, axis=1) * fa + (z.alb_aer / 4) * _trapz(Rr * Isrc[t], c.mu, axis=1) * fr
            else:
                S[t] = (c.alb_atm / 4) * _trapz(Ra * Isrc[t], c.mu, axis=1)
    return S


def linear_weights(x):
    """w0 = 1 - a, w1 = a - E with a = (1 - E) / x, in long double with expm1 (x = 0: both 0)."""
    xl = np.asarray(x, dtype=np.longdouble)
    safe = np.where(xl > 0, xl, 1)
    a = np.where(xl > 0, -np.expm1(-safe) / safe, 1)
    E = np.exp(-xl)
    return np.asarray(1 - a, dtype=np.float64), np.asarray(a - E, dtype=np.float64)


def transport(c, S, mu_view, quadrature, surface="specular"):
    """The two sweeps of S [L, 2V] -> [L, 2V].  surface: 'specular' (rho D[L-1] of the mirror lane) or None (0)."""
    tau = c.tau
    mu = np.asarray(mu_view, dtype=np.float64)
    L, V = len(tau), len(mu)
    out = np.zeros((L, 2 * V))
    Sd, Su = S[:, :V], S[:, V:]

    def step(dt):
        x = dt / mu
        E = np.exp(-x)
        if quadrature == QUAD_LINEAR:
            w0, w1 = linear_weights(x)
            return E, w0, w1
        h = (dt / 2) / mu
        return E, h, h * E

    for t in range(1, L):
        E, wc, wp = step(tau[t] - tau[t - 1])
        out[t, :V] = E * out[t - 1, :V] + (wc * Sd[t] + wp * Sd[t - 1])
    out[L - 1, V:] = c.grd_alb * out[L - 1, :V] if surface == "specular" else 0.0
    gaps = set() if quadrature == QUAD_LINEAR else {z.r1 for z in c.zones[:-1]}
    for t in range(L - 2, -1, -1):
        E, wc, wp = step(tau[t + 1] - tau[t])
        if t in gaps:
            out[t, V:] = E * out[t + 1, V:]
        else:
            out[t, V:] = E * out[t + 1, V:] + (wc * Su[t] + wp * Su[t + 1])
    return out


def first_order(c, p0a, p0r, mu_view):
    """`oracle.first_order` (spec:104-292) at the lanes s_j: p0a, p0r [2V] are the column's rows of `phase_p0_rows`."""
    tau, mu0 = c.tau, c.mu0
    mv = np.asarray(mu_view, dtype=np.float64)
    L, V = len(tau), len(mv)
    F0 = np.pi / mu0
    T = c.tauStar_tot
    R = F0 * c.grd_alb * np.exp(-T / mu0)
    mir = (np.arange(2 * V) + V) % (2 * V)

    def q_of(z):
        if z.kind != "mix":
            return c.alb_atm * p0a / (4 * np.pi)
        fa, fr = c.zone_fractions(z)
        return (c.alb_atm * p0a * fa + z.alb_aer * p0r * fr) / (4 * np.pi)
    I1 = np.zeros((L, 2 * V))
    zones = c.zones
    with np.errstate(all="ignore"):
        md = -mv
        near = np.abs(md + mu0) < 0.0001
        for zi, z in enumerate(zones):
            q = q_of(z)
            qd, qdm = q[:V], q[mir[:V]]
            t_bd, t_bs = (0.0, 0.0) if zi == 0 else (tau[z.r0 - 1], tau[z.r0])
            for t in range(z.r0, z.r1 + 1):
                before = 0.0 if zi == 0 else I1[z.r0 - 1, :V] * np.exp((tau[t] - t_bd) / md)
                direct = (mu0 / (mu0 + md)) * qd * F0 * (np.exp(-tau[t] / mu0) - np.exp(-t_bd / mu0) * np.exp((tau[t] - t_bd) / md))
                direct_near = qd * F0 * np.exp(-tau[t] / mu0) * (tau[t] - t_bd) / mu0
                surf = (mu0 / (mu0 - md)) * qdm * R * (np.exp(-(T - tau[t]) / mu0) - np.exp(-(T - t_bs) / mu0) * np.exp((tau[t] - t_bs) / md))
                I1[t, :V] = before + np.where(near, direct_near, direct) + surf
        mp = mv
        near = np.abs(mp - mu0) < 0.0001
        for zi in range(len(zones) - 1, -1, -1):
            z = zones[zi]
            q = q_of(z)
            qu, qum = q[V:], q[mir[V:]]
            bottom = zi == len(zones) - 1
            if bottom:
                t_bu, t_su = tau[L - 1], T
                B = c.grd_alb * I1[L - 1, mir[V:]]
            else:
                t_bu, t_su = tau[z.r1 + 1], tau[z.r1]
            for t in range(z.r0, z.r1 + 1):
                if not bottom:
                    B = I1[z.r1 + 1, V:]
                before = B * np.exp(-(t_bu - tau[t]) / mp)
                direct = (mu0 / (mu0 + mp)) * qu * F0 * (np.exp(-tau[t] / mu0) - np.exp(-t_bu / mu0) * np.exp(-(t_bu - tau[t]) / mp))
                surf = (mu0 / (mu0 - mp)) * qum * R * (np.exp(-(T - tau[t]) / mu0) - np.exp(-(T - t_su) / mu0) * np.exp(-(t_su - tau[t]) / mp))
                surf_near = qum * R * np.exp(-(T - tau[t]) / mu0) * (t_su - tau[t]) / mu0
                I1[t, V:] = before + direct + np.where(near, surf_near, surf)
    return I1


def first_order_single_slab(tau, tauStar, mu0, alb, p0, mu_view):
    """`oracle.I1_NumInt` (I1_In:13-58) at the lanes s_j."""
    mv = np.asarray(mu_view, dtype=np.float64)
    L, V = len(tau), len(mv)
    I1 = np.zeros((L, 2 * V))
    e0 = np.exp(-tau / mu0)
    eS = np.exp(-tauStar / mu0)
    k = alb / (4 * np.pi)
    md = -mv
    near = np.abs(md + mu0) < 0.0001
    with np.errstate(all="ignore"):
        for t in range(L):
            v = (mu0 / (mu0 + md)) * k * p0[:V] * (e0[t] - np.exp(tau[t] / md))
            I1[t, :V] = np.where(near, k * p0[:V] * e0[t] * tau[t] / mu0, v)
            I1[t, V:] = (mu0 / (mu0 + mv)) * k * p0[V:] * (e0[t] - eS * np.exp(-(tauStar - tau[t]) / mv))
    return I1 * np.pi / mu0


def single_slab_column(tau, mu, N, mu0, alb, tauStar):
    """An oracle Column that `source` / `transport` read as the single slab of I1_In:62-130 (one clear zone, black surface)."""
    z = [O._Zone(0, len(tau) - 1, "atm")]
    return O.Column(tau=np.asarray(tau, dtype=np.float64), mu=mu, N=N, idx_up=0, idx_down=0, mu0=mu0, grd_alb=0.0, alb_atm=alb, alb_aer=0.0,
                    dtau_atm=tauStar / len(tau), dtau_aer=0.0, tauStar_tot=tauStar, P0_atm=None, P_atm=None, P0_aer=None,
                    P_aer=None, surface=None, zone_table=z)


# ---- the grid's own lanes ------------------------------------------------------------------------------------------------
def node_views(mu, N):
    """(mu_view, grid index of every signed lane): all nodes with |mu| >= 0.01, ascending."""
    up = np.array([m for m in range(N + 1, 2 * N) if mu[m] >= O.MU_THRESHOLD])
    mv = mu[up]
    down = 2 * N - 1 - up
    assert np.max(np.abs(mu[down] + mv)) < 4e-16             # (linspace(-1, 0, N) mirrors linspace(0, 1, N) to an ulp, not bit for bit)
    return mv, np.concatenate((down, up))


def rewritten_down(c, lanes_down):
    """[L, V] mask: downward lanes (grid indices) the a4b extrapolation rewrote in each row (spec:342-345,361-364,380-383)."""
    L = len(c.tau)
    m = np.zeros((L, len(lanes_down)), dtype=bool)
    for z, tref in zip(c.zones, c.tau_ref()):
        idx = O.a4b_count(tref, c.N)
        m[z.r0:z.r1 + 1] = (lanes_down >= c.N - idx)[None, :]
    return m


def node_errors(c, sol, surface="specular"):
    """Model GRID on I - I_last at the nodes against I - I1: (|error| / field maximum [L, 2V], mask of the rewritten
    downward lanes [L, V]).  A column without P_aer is a single slab."""
    mv, lanes = node_views(c.mu, c.N)
    V = len(mv)
    Isrc = sol.I - sol.I_saved[-1]
    S = source(c, c.P_atm[lanes], None if c.P_aer is None else c.P_aer[lanes], Isrc)
    got = transport(c, S, mv, QUAD_GRID, surface=surface)
    ref = (sol.I - sol.I_saved[0])[:, lanes]
    return np.abs(got - ref) / np.max(np.abs(ref)), rewritten_down(c, lanes[:V])


def untouched_up(err):
    """Upward lanes whose error stays below 1e-12 on every row; they must be the lanes above some cosine (the blend of
    spec:402-409 rewrites a run of lanes that starts next to mu = 0+)."""
    V = err.shape[1] // 2
    ok = np.max(err[:, V:], axis=0) < 1e-12
    n = int(ok.sum())
    assert np.array_equal(ok, np.arange(V) >= V - n), "the untouched upward lanes are not a run down from mu = 1"
    return ok


# ---- the two cases of the node tests (Rayleigh + Henyey-Greenstein) ----------------------------------------------------------
Z0 = 120


@functools.lru_cache(maxsize=None)
def case_A(mu0=0.6, tauStar_aer=0.3, rho=0.15, L=40, N=64, g=0.7):
    """One slab: L = 40, N = 64, g = 0.7, tauStar_aer = 0.3, mu0 = 0.6, rho = 0.15."""
    mu = O.make_mu(N)
    P0a, Pa = O.phase_rayleigh(N, mu, mu0)
    P0r, Pr = O.phase_hg(N, mu, mu0, g)
    return O.make_column(mu0, Z0, 25, 17, L, 0.124, tauStar_aer, rho, 1.0, 0.95, N, P0a, Pa, P0r, Pr)


@functools.lru_cache(maxsize=None)
def case_B(mu0=0.6, rho=0.15, scale=1.0, L=48, N=64, g=0.6):
    """Two slabs [(25, 17, 0.12, 0.97), (10, 6, 0.2, 0.9)]: L = 48, N = 64, g = 0.6 (`scale` multiplies the aerosol depths)."""
    mu = O.make_mu(N)
    P0a, Pa = O.phase_rayleigh(N, mu, mu0)
    P0r, Pr = O.phase_hg(N, mu, mu0, g)
    return O.make_column_slabs(mu0, Z0, [(25, 17, 0.12 * scale, 0.97), (10, 6, 0.2 * scale, 0.9)], L, 0.124, rho, 1.0, N, P0a, Pa, P0r, Pr)


@functools.lru_cache(maxsize=None)
def solved(case, *args):
    c = case(*args)
    return c, O.solve_column(c, literal=False)
