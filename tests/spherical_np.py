"""NumPy model of the pseudo-spherical direct beam, written from the definitions and not from the kernels:
the slant optical depth of the beam through spherical shells, the layer-by-layer first order on a beam path sigma, and the
flux beam terms on that path.  With the plane path sigma = tau / mu0 the first order is the reference's three-zone first
order (oracle.first_order) and the beam terms are oracle.fluxes."""
import numpy as np

EARTH_RADIUS_KM = 6371.0


def slant_path(tau, z, mu0, earth_radius=EARTH_RADIUS_KM, dtype=np.float64):
    """sigma [L]: sigma_0 = 0, sigma_t = sum_{k=1..t} (tau_k - tau_{k-1}) c_{t,k} with
    c_{t,k} = (r_{k-1} + r_k) / (sqrt(r_{k-1}^2 - p^2) + sqrt(r_k^2 - p^2)), r = R_e + z, p^2 = r_t^2 (1 - mu0^2).
    dtype: the type every operation runs in (np.longdouble: the same formulas, to measure what float64 loses)."""
    tau = np.asarray(tau, dtype=dtype)
    r = dtype(earth_radius) + np.asarray(z, dtype=dtype)
    L = tau.size
    if not (mu0 > 0):
        raise ValueError("mu0 must be > 0")
    mu0 = dtype(mu0)
    sig = np.zeros(L, dtype=dtype)
    d = np.diff(tau)
    for t in range(1, L):
        p2 = r[t] * r[t] * (1.0 - mu0 * mu0)
        s = np.sqrt(r[:t + 1] * r[:t + 1] - p2)
        c = (r[:t] + r[1:t + 1]) / (s[:t] + s[1:t + 1])
        sig[t] = np.sum(d[:t] * c)
    return sig


def plane_path(tau, mu0):
    return np.asarray(tau, dtype=np.float64) / mu0


def slant_uniform_closed_form(z, mu0, kappa, earth_radius=EARTH_RADIUS_KM):
    """Slant optical depth of a medium of uniform extinction kappa (per km) above level t: kappa (sqrt(r_0^2 - p^2) - r_t mu0)."""
    r = float(earth_radius) + np.asarray(z, dtype=np.float64)
    p2 = r * r * (1.0 - mu0 * mu0)
    return kappa * (np.sqrt(r[0] * r[0] - p2) - r * mu0)


def phi(y, dtype=np.float64):
    """-expm1(-y) / y with phi(0) = 1."""
    y = np.asarray(y, dtype=dtype)
    safe = np.where(y == 0, 1.0, y)
    return np.where(y == 0, 1.0, -np.expm1(-safe) / safe)


def zone_q(c, P0_aer_zone=None):
    """q [nz][2N] of the column's zones (spec:149): clear w_atm P0_atm / (4 pi); aerosol (w_atm P0_atm f_atm + w_aer P0_aer f_aer)
    / (4 pi).  P0_aer_zone [nz][2N] (optional) gives every zone its own aerosol P0 (the per-zone layout of the phase sets)."""
    out = []
    for zi, z in enumerate(c.zones):
        if z.kind != "mix":
            out.append(c.alb_atm * c.P0_atm / (4 * np.pi))
        else:
            fa, fr = c.zone_fractions(z)
            pr = c.P0_aer if P0_aer_zone is None else P0_aer_zone[zi]
            out.append((c.alb_atm * c.P0_atm * fa + z.alb_aer * pr * fr) / (4 * np.pi))
    return out


def first_order_beam(c, sigma, P0_aer_zone=None, dtype=np.float64):
    """The first order of column `c` (oracle.Column) on the beam path sigma [L]: I1 [L][2N].  dtype: as in slant_path."""
    tau, mu, N, mu0 = np.asarray(c.tau, dtype=dtype), np.asarray(c.mu, dtype=dtype), c.N, dtype(c.mu0)
    sigma = np.asarray(sigma, dtype=dtype)
    L = tau.size
    D = 2 * N
    F0 = dtype(np.pi) / mu0
    T = dtype(c.tauStar_tot)
    R = F0 * c.grd_alb * np.exp(-sigma[L - 1] - (T - tau[L - 1]) / mu0)
    zones = c.zones
    qz = [np.asarray(q, dtype=dtype) for q in zone_q(c, P0_aer_zone)]
    zone_of = np.zeros(L, dtype=int)
    first_row, last_row = np.zeros(L, dtype=bool), np.zeros(L, dtype=bool)
    for zi, z in enumerate(zones):
        zone_of[z.r0:z.r1 + 1] = zi
        if zi > 0:
            first_row[z.r0] = True               # first row of a zone below the top one
        if zi < len(zones) - 1:
            last_row[z.r1] = True                # last row of a zone above the bottom one
    mirror = D - 1 - np.arange(D)
    e_dir = F0 * np.exp(-sigma)                  # F0 e^{-sigma_t}
    e_ref = R * np.exp(-(T - tau) / mu0)         # R e^{-(T - tau_t) / mu0}
    I1 = np.zeros((L, D), dtype=dtype)
    with np.errstate(all="ignore"):
        a = np.abs(mu[:N])
        # downward, D_0 = 0; layer (t-1, t) takes the q of row t
        Dn = np.zeros(N, dtype=dtype)
        for t in range(1, L):
            q = qz[zone_of[t]]
            dl = tau[t] - tau[t - 1]
            s = (sigma[t] - sigma[t - 1]) / dl
            E = np.exp(-dl / a)
            Dn = Dn * E + q[:N] * e_dir[t] * (dl / a) * phi((1 / a - s) * dl, dtype)
            if not first_row[t]:
                Dn = Dn + q[mirror[:N]] * e_ref[t] * (dl / a) * phi((1 / a + 1 / mu0) * dl, dtype)
            I1[t, :N] = Dn
        # surface and upward; layer (t, t+1) takes the q of row t
        a = np.abs(mu[N:])
        Up = c.grd_alb * I1[L - 1, mirror[N:]]
        I1[L - 1, N:] = Up
        for t in range(L - 2, -1, -1):
            q = qz[zone_of[t]]
            dl = tau[t + 1] - tau[t]
            s = (sigma[t + 1] - sigma[t]) / dl
            E = np.exp(-dl / a)
            Up = Up * E + q[N:] * e_dir[t] * (dl / a) * phi((1 / a + s) * dl, dtype)
            if not last_row[t]:
                Up = Up + q[mirror[N:]] * e_ref[t] * (dl / a) * phi((1 / a - 1 / mu0) * dl, dtype)
            I1[t, N:] = Up
    # the two mu = 0 nodes
    for t in range(L):
        q = qz[zone_of[t]]
        for m in (N - 1, N):
            I1[t, m] = q[m] * e_dir[t] + q[mirror[m]] * e_ref[t]
    return I1


def beam_flux_terms(tau, sigma, mu0, grd_alb, beam_norm="crit"):
    """(downward, upward) beam terms per level: -fb e^{-sigma_t}, +fb rho e^{-sigma_{L-1}} e^{-(tau_{L-1} - tau_t) / mu0}."""
    tau, sigma = np.asarray(tau, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    F0 = np.pi / mu0
    fb = F0 / (4 * np.pi) if beam_norm == "crit" else F0
    return -fb * np.exp(-sigma), fb * grd_alb * np.exp(-sigma[-1]) * np.exp(-(tau[-1] - tau) / mu0)


def epilogue_beam(I, mu, tau, sigma, N, mu0, grd_alb, z_profile=None, slabs=None, beam_norm="crit"):
    """Fluxes, diffusivity, heating rate and TOA net flux of a field with the beam terms on the path sigma (the arithmetic of
    oracle.fluxes / diffusivity / heating_rate / toa_net_flux with the two exponentials replaced)."""
    trapz = getattr(np, "trapezoid", None) or np.trapz
    L = len(tau)
    sd = np.array([trapz(I[i, :N] * mu[:N], mu[:N]) for i in range(L)])
    su = np.array([trapz(I[i, N:] * mu[N:], mu[N:]) for i in range(L)])
    bd, bu = beam_flux_terms(tau, sigma, mu0, grd_alb, beam_norm)
    out = {"flux_down": sd + bd, "flux_up": su + bu,
           "diffusivity": np.array([-trapz(I[i] * mu, mu) / trapz(I[i], mu) for i in range(L)])}
    bd4, bu4 = beam_flux_terms(tau, sigma, mu0, grd_alb, "crit")
    flux = (sd + bd4) + (su + bu4)
    out["net_toa"] = -(sd[0] + bd4[0]) - (su[0] + bu4[0])
    if z_profile is not None:
        hr = np.zeros(L)
        for i in range(L - 1):
            hr[i] = -(1 / (1.225 * 1004)) * (flux[i + 1] - flux[i]) / (z_profile[i + 1] - z_profile[i])
        hr[-1] = hr[-2]
        for iu, idn in (slabs or []):
            hr[iu - 1] = hr[iu - 2]
            hr[idn] = hr[idn - 1]
        out["heating_rate"] = hr
    return out


# ---- the columns of the tests (Rayleigh + Henyey-Greenstein g = 0.7, z0 = 120 km, molecules 0.124, aerosol 0.3 of albedo 0.97 at 17-25 km) ----
Z0, T_ATM, T_AER = 120.0, 0.124, 0.3
TWO_SLABS = [(25, 17, 0.12, 0.97), (10, 6, 0.2, 0.9)]
# (N, L, mu0, rho[, slabs]); every mu0 is at least 1e-3 from a node of its grid, so the reference's approximate limit branch
# (|mu -+ mu0| < 1e-4) is not in play
FIRST_ORDER_CASES = [(32, 24, 0.6, 0.0), (32, 24, 0.6, 0.3), (33, 24, 0.83, 0.5), (32, 24, 0.21, 0.3), (32, 24, 0.05, 0.3),
                     (32, 48, 0.6, 0.3, TWO_SLABS)]
# whole columns on which the reference's unbounded mu -> 0+ search stays on the grid
SOLVE_CASES = [(32, 24, 0.6, 0.3), (32, 24, 0.45, 0.3), (64, 24, 0.3, 0.3), (64, 24, 0.21, 0.3), (64, 30, 0.21, 0.0),
               (64, 24, 0.15, 0.1), (32, 48, 0.6, 0.3, TWO_SLABS)]


def column(O, N, L, mu0, rho, slabs=None, surface="specular", g=0.7, alb_aer=0.97):
    """An oracle column of the tests' atmosphere (O: the sos_oracle module)."""
    mu = O.make_mu(N)
    P0a, Pa = O.phase_rayleigh(N, mu, mu0)
    P0r, Pr = O.phase_hg(N, mu, mu0, g)
    if slabs:
        return O.make_column_slabs(mu0, Z0, slabs, L, T_ATM, rho, 1.0, N, P0a, Pa, P0r, Pr, surface=surface)
    return O.make_column(mu0, Z0, 25, 17, L, T_ATM, T_AER, rho, 1.0, alb_aer, N, P0a, Pa, P0r, Pr, surface=surface)


def altitudes(L, z0=Z0):
    return np.linspace(z0, 0, L)


def node_distance(N, mu0):
    return float(np.min(np.abs(np.abs(np.concatenate((np.linspace(-1, 0, N), np.linspace(0, 1, N)))) - mu0)))
