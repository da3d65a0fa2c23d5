"""NumPy model of thermal emission, written from the definitions and not from the kernels: the field the
layers and the ground emit on the grid's directions and at view cosines, and the epilogue without beam terms.  The full thermal
field is the order loop fed this field as its first order: oracle.solve_column(c, I1=emission(c, ...))."""
import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz


def linear_weights(x, dtype=np.float64):
    """(w0, w1, E) of a source linear in tau over a layer of slant thickness x = Delta / a, attenuated exactly: E = e^{-x},
    A = (1 - E) / x, w0 = 1 - A (the row the sweep arrives at), w1 = A - E (the row it leaves); both 0 at x = 0.  expm1 keeps the
    digits of 1 - E, and below x = 0.25 the two differences are summed as the series sum (-1)^{n+1} x^n / (n+1)! [times n].
    dtype: the type every operation runs in (np.longdouble: the same formulas, to measure what float64 loses)."""
    x = np.asarray(x, dtype=dtype)
    E = np.exp(-x)
    safe = np.where(x == 0, 1.0, x)
    A = -np.expm1(-safe) / safe
    w0, w1 = 1 - A, A - E
    s0, s1, term = np.zeros_like(x), np.zeros_like(x), np.ones_like(x)
    for n in range(1, 20):
        term = term * -x / (n + 1) if n > 1 else x / 2        # (-1)^{n+1} x^n / (n+1)!
        s0 = s0 + term
        s1 = s1 + n * term
    small = x < 0.25
    return np.where(small, s0, w0), np.where(small, s1, w1), E


def zone_eps(c):
    """eps [L]: the emission coefficient of every row's zone: 1 - omega_atm in a clear zone, 1 - (omega_atm f_atm + omega_aer f_aer)
    in an aerosol zone (f of spec:149)."""
    eps = np.zeros(len(c.tau))
    for z in c.zones:
        if z.kind != "mix":
            eps[z.r0:z.r1 + 1] = 1 - c.alb_atm
        else:
            fa, fr = c.zone_fractions(z)
            eps[z.r0:z.r1 + 1] = 1 - (c.alb_atm * fa + z.alb_aer * fr)
    return eps


def boundary(c, down):
    """What the order loop reflects of the downward surface row `down` [N] (oracle._transport): [N] on the upward directions
    N .. 2N-1 (the entry of the mu = 0 node is not used)."""
    N, mu = c.N, c.mu
    out = np.zeros(N, dtype=np.asarray(down).dtype)
    rev = np.arange(N - 2, -1, -1)
    if c.surface == "specular":
        out[1:] = c.grd_alb * down[rev]
    elif c.surface == "lambertian":
        out[1:] = -2 * c.grd_alb * _trapz(down[rev] * mu[rev], mu[rev])
    elif c.surface == "lambertian_readme":
        out[1:] = 2 * c.grd_alb * _trapz(down[rev] * mu[rev], mu[rev])
    return out


def _sweeps(tau, b, eps, a, ground_of, dtype=np.float64):
    """Downward and upward sweeps at the cosines a [K] > 0: (D [L][K], U [L][K]); ground_of(D_{L-1}) -> U_{L-1}."""
    tau, b, eps, a = (np.asarray(x, dtype=dtype) for x in (tau, b, eps, a))
    L = len(tau)
    D, U = np.zeros((L, a.size), dtype=dtype), np.zeros((L, a.size), dtype=dtype)
    for t in range(1, L):
        w0, w1, E = linear_weights((tau[t] - tau[t - 1]) / a, dtype)
        D[t] = D[t - 1] * E + eps[t] * (w0 * b[t] + w1 * b[t - 1])
    U[L - 1] = ground_of(D[L - 1])
    for t in range(L - 2, -1, -1):
        w0, w1, E = linear_weights((tau[t + 1] - tau[t]) / a, dtype)
        U[t] = U[t + 1] * E + eps[t + 1] * (w0 * b[t] + w1 * b[t + 1])
    return D, U


def emission(c, planck, planck_surface, emissivity=None, dtype=np.float64):
    """I_0 [L][2N] of column `c` (oracle.Column): planck [L] at the levels, the ground's planck_surface and emissivity
    (None: 1 - grd_alb).  dtype: as in linear_weights."""
    tau, mu, N = np.asarray(c.tau, dtype=dtype), c.mu, c.N
    b = np.asarray(planck, dtype=dtype)
    L = tau.size
    es = 1 - c.grd_alb if emissivity is None else float(emissivity)
    eps = zone_eps(c)
    I0 = np.zeros((L, 2 * N), dtype=dtype)
    a = np.abs(mu[:N - 1])[::-1]                              # |mu| of directions N-2 .. 0 = mu of directions N+1 .. 2N-1

    def ground_of(down):                                     # down[j]: direction N-2-j
        full = np.zeros(N, dtype=dtype)
        full[:N - 1] = down[::-1]
        return boundary(c, full)[1:] + es * planck_surface

    D, U = _sweeps(tau, b, eps, a, ground_of, dtype)
    I0[:, :N - 1] = D[:, ::-1]
    I0[:, N + 1:] = U
    I0[:, N - 1] = I0[:, N] = eps * b                        # the two mu = 0 nodes
    return I0


def emission_view(c, planck, planck_surface, mu_view, levels, emissivity=None, dtype=np.float64):
    """[nlev][2V] on the signed lanes (-mu_view, +mu_view): the sweeps at a = mu_view; specular ground or none."""
    tau = np.asarray(c.tau, dtype=dtype)
    a = np.atleast_1d(np.asarray(mu_view, dtype=dtype))
    es = 1 - c.grd_alb if emissivity is None else float(emissivity)
    if c.surface not in ("specular", None):
        raise ValueError("the view lanes have no Lambertian ground")
    rho = c.grd_alb if c.surface == "specular" else 0.0
    D, U = _sweeps(tau, np.asarray(planck, dtype=dtype), zone_eps(c), a, lambda down: rho * down + es * planck_surface, dtype)
    lev = np.atleast_1d(levels)
    return np.concatenate((D[lev], U[lev]), axis=1)


def epilogue_emission(I, mu, N, z_profile=None, slabs=None):
    """Fluxes, diffusivity, heating rate and TOA net flux of a field without a direct beam (the arithmetic of oracle.fluxes /
    diffusivity / heating_rate / toa_net_flux with both beam terms absent)."""
    L = I.shape[0]
    sd = np.array([_trapz(I[i, :N] * mu[:N], mu[:N]) for i in range(L)])
    su = np.array([_trapz(I[i, N:] * mu[N:], mu[N:]) for i in range(L)])
    out = {"flux_down": sd, "flux_up": su, "diffusivity": np.array([-_trapz(I[i] * mu, mu) / _trapz(I[i], mu) for i in range(L)]),
           "net_toa": -sd[0] - su[0]}
    if z_profile is not None:
        flux = sd + su
        hr = np.zeros(L)
        for i in range(L - 1):
            hr[i] = -(1 / (1.225 * 1004)) * (flux[i + 1] - flux[i]) / (z_profile[i + 1] - z_profile[i])
        hr[-1] = hr[-2]
        for iu, idn in (slabs or []):
            hr[iu - 1] = hr[iu - 2]
            hr[idn] = hr[idn - 1]
        out["heating_rate"] = hr
    return out


# ---- the columns of the tests: Rayleigh + Henyey-Greenstein g = 0.5, z0 = 120 km, a 17-25 km slab ------------------------------
Z0, G_AER = 120.0, 0.5
TWO_SLABS = [(25, 17, 0.12, 0.97), (10, 6, 0.2, 0.5)]
MU0 = 0.5                                                    # (does not enter the thermal field)
# (N, L, rho, tauStar_atm, alb_atm, tauStar_aer, alb_aer, surface, slabs, orders the oracle's loop takes)
SOLVE_CASES = [(32, 24, 0.1, 1.0, 0.0, 0.3, 0.6, "specular", None, 7),
               (33, 24, 0.3, 0.5, 0.2, 0.3, 0.9, "specular", None, 10),
               (64, 30, 0.1, 1.0, 0.3, 0.5, 0.7, "specular", None, 11),
               (32, 48, 0.2, 1.0, 0.1, None, None, "specular", TWO_SLABS, 8),
               (32, 24, 0.3, 1.0, 0.0, 0.3, 0.6, "lambertian_readme", None, 7),
               (32, 24, 0.3, 1.0, 0.0, 0.3, 0.6, "lambertian", None, 7)]


def altitudes(L, z0=Z0):
    return np.linspace(z0, 0, L)


def planck_profile(L, z0=Z0):
    """b [L] = (T / 288)^4 of a 288 K / -6.5 K km^-1 / 216.5 K temperature profile at the levels' altitudes."""
    T = np.maximum(288.0 - 6.5 * altitudes(L, z0), 216.5)
    return (T / 288.0) ** 4


def column(O, N, L, rho, t_atm, w_atm, t_aer=0.3, w_aer=0.6, surface="specular", slabs=None, mu0=MU0, g=G_AER):
    """An oracle column of the tests' atmosphere (O: the sos_oracle module)."""
    mu = O.make_mu(N)
    P0a, Pa = O.phase_rayleigh(N, mu, mu0)
    P0r, Pr = O.phase_hg(N, mu, mu0, g)
    if slabs:
        return O.make_column_slabs(mu0, Z0, slabs, L, t_atm, rho, w_atm, N, P0a, Pa, P0r, Pr, surface=surface)
    return O.make_column(mu0, Z0, 25, 17, L, t_atm, t_aer, rho, w_atm, w_aer, N, P0a, Pa, P0r, Pr, surface=surface)


def solve_column_case(O, case, mu0=MU0):
    N, L, rho, t_atm, w_atm, t_aer, w_aer, surface, slabs, _ = case
    return column(O, N, L, rho, t_atm, w_atm, t_aer, w_aer, surface, slabs, mu0)
