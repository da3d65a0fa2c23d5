"""NumPy model of the azimuth-resolved view radiance: the view stage of tests/view_np.py run per Fourier mode
of tests/azimuth_np.py, and a DIRECT view radiance that never goes through a mode -- the field of
azimuth_direct.direct_solve on its azimuth nodes, its source formed at (view lane, azimuth) with the physical kernel p(c)
summed over the nodes and the grid, transported by view_np.transport.

Signed lanes s = (-mu_view, +mu_view); c(a, b, phi) = -(mu_a mu_b + s_a s_b cos phi); phi = 0 with an upward mu = mu0 is
back-scatter.  A phase function `fn` None is the isotropic one."""
import numpy as np

import azimuth_direct as AD
import azimuth_np as A
import sos_oracle as O
import view_np as VN

_trapz = A._trapz


# ---- builders ------------------------------------------------------------------------------------------------------------------
def mode_rows(fn, mu, s, ms, nphi):
    """rows^m[j][n] = R^m(s_j, mu_n) / (2 pi) * 4 / Z_n, Z_n = trapz_mu(R^0(., n) / (2 pi)) on the same nphi nodes:
    [len(ms), len(s), 2N].  `azimuth_np.ring_modes` takes any exit cosines; the normaliser stays the grid's."""
    s = np.asarray(s, dtype=np.float64)
    ms = list(ms)
    if fn is None:
        return np.zeros((len(ms), len(s), len(mu)))
    Z = _trapz(A.ring_modes(fn, mu, mu, [0], nphi)[0] / (2 * np.pi), mu, axis=0)[None, :]
    R = A.ring_modes(fn, s, mu, ms, nphi) / (2 * np.pi)
    return np.stack([4 * R[i] / Z for i in range(len(ms))])


def solve_rows(fn, mu, s, ms, nphi):
    """(-1)^m rows^m: what the view source of mode m takes (it pairs rows[j][2N-1-k] with I[k], the fold of the grid)."""
    return np.stack([(-1) ** m * r for m, r in zip(ms, mode_rows(fn, mu, s, ms, nphi))])


def mode_p0_rows(fn, mu, mu0, s, ms, nphi):
    """p0rows^m[b][j] = R^m(s_j, mu0_b) / (4 pi) * 2 / Z0_b, Z0_b = trapz_mu(R^0(., mu0_b) / (4 pi)): [len(ms), B, len(s)]."""
    s = np.asarray(s, dtype=np.float64)
    mu0 = np.atleast_1d(np.asarray(mu0, dtype=np.float64))
    ms = list(ms)
    if fn is None:
        return np.zeros((len(ms), len(mu0), len(s)))
    Z = _trapz(A.ring_modes(fn, mu, mu0, [0], nphi)[0] / (4 * np.pi), mu, axis=0)            # [B]
    R = A.ring_modes(fn, s, mu0, ms, nphi) / (4 * np.pi)                                      # [m, V2, B]
    return np.stack([(R[i] / Z[None, :] * 2).T for i in range(len(ms))])


def p0_exact(fn, mu, mu0, s, phi):
    """p(c(s_j, mu0_b, phi_i)) / Z0_b with the 25-node normaliser of the stored P0 (view_np.phase_p0_rows'): [len(phi), B, len(s)]."""
    s = np.asarray(s, dtype=np.float64)
    mu0 = np.atleast_1d(np.asarray(mu0, dtype=np.float64))
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    if fn is None:
        return np.ones((len(phi), len(mu0), len(s)))
    Z = _trapz(O._azimuth_average(fn, mu, mu0) / (4 * np.pi), mu, axis=0)                     # [B]
    c = -(s[None, None, :] * mu0[None, :, None]
          + np.sqrt(1 - s * s)[None, None, :] * np.sqrt(1 - mu0 * mu0)[None, :, None] * np.cos(phi)[:, None, None])
    return fn(c) / Z[None, :, None]


# ---- the view stage per mode -----------------------------------------------------------------------------------------------------
def mode_scattered(c, fn_atm, fn_aer, Im, m, mu_view, quadrature, nphi, surface="specular"):
    """Transport of the source of the mode-m field Im [L, 2N] at the view lanes: [L, 2V].  Mode 0 takes the stored matrix's
    rows (25 nodes), modes m >= 1 (-1)^m rows^m on `nphi` nodes.  fn_aer None with a single slab: no aerosol rows."""
    sgn = VN.signed(mu_view)
    rows = (lambda fn: VN.phase_rows(fn, c.mu, sgn)) if m == 0 else (lambda fn: solve_rows(fn, c.mu, sgn, [m], nphi)[0])
    three = any(z.kind == "mix" for z in c.zones)
    S = VN.source(c, rows(fn_atm), rows(fn_aer) if three else None, Im)
    return VN.transport(c, S, mu_view, quadrature, surface=surface)


def mode_p0(fn, mu, mu0, mu_view, m, nphi):
    """The first-order rows of mode m for one column: [2V]."""
    sgn = VN.signed(mu_view)
    return VN.phase_p0_rows(fn, mu, [mu0], sgn)[0] if m == 0 else mode_p0_rows(fn, mu, [mu0], sgn, [m], nphi)[0, 0]


def synthesize(vals, phi):
    """sum_m (2 - delta_m0) val^m cos(m phi): vals [M + 1, ...] -> [..., len(phi)], the terms added in ascending m."""
    phi = np.asarray(phi, dtype=np.float64)
    out = np.repeat(np.asarray(vals[0])[..., None], len(phi), axis=-1).astype(np.float64)
    for m in range(1, len(vals)):
        out = out + 2 * np.asarray(vals[m])[..., None] * np.cos(m * phi)
    return out


# ---- direct: no Fourier mode anywhere ----------------------------------------------------------------------------------------------
def direct_source(geo, fn_atm, fn_aer, Iq, s, phi):
    """Source of the field Iq [nq, L, 2N] on the uniform nodes phi_r = 2 pi r / nq at (lane s_j, azimuth phi_i): [len(phi), L,
    len(s)].  The kernel of azimuth_direct._kernels with the exit cosine s_j in place of mu_a,
        K_Delta[j][k] = p(c(s_j, flip k, Delta + pi)) * 4 / Z_{flip k} / nq * w_k,   Delta = phi_i - phi_r
    (the pair (s_j, flip k) at Delta + pi is the physical scattering cosine at Delta), times the row's albedo factor."""
    fn_aer = fn_aer or fn_atm
    mu = geo.mu
    s = np.asarray(s, dtype=np.float64)
    nq, L = Iq.shape[:2]
    wq = np.zeros(len(mu))
    wq[:-1] += np.diff(mu) / 2
    wq[1:] += np.diff(mu) / 2
    sm, ss = np.sqrt(1 - mu * mu), np.sqrt(1 - s * s)
    out = np.zeros((len(phi), L, len(s)))
    for fn, w_rows in ((fn_atm, geo.w_atm), (fn_aer, geo.w_aer)):
        if not np.any(w_rows):
            continue
        Z = _trapz(O._azimuth_average(fn, mu, mu) / (2 * np.pi), mu, axis=0)                  # 25-node normaliser per column b'
        for i, ph in enumerate(phi):
            for r in range(nq):
                delta = ph - 2 * np.pi * r / nq
                c = -(s[:, None] * mu[None, :] + ss[:, None] * sm[None, :] * np.cos(delta + np.pi))
                K = (fn(c) * 4 / Z[None, :] / nq)[:, ::-1] * wq[None, :]
                out[i] += w_rows[:, None] * (Iq[r] @ K.T)
    return out


def direct_view(c, geo, fn_atm, fn_aer, Iq, mu_view, phi, quadrature, scale=1.0, surface="specular"):
    """(first [len(phi), L, 2V], scattered (same shape)) at the view lanes from the direct field Iq of the orders that feed the
    source: the closed-form first order with p0_exact, and the transport of `direct_source`."""
    sgn = VN.signed(mu_view)
    S = direct_source(geo, fn_atm, fn_aer, Iq, sgn, phi)
    scat = np.stack([VN.transport(c, S[i], mu_view, quadrature, surface=surface) for i in range(len(phi))])
    pa = scale * p0_exact(fn_atm, c.mu, [c.mu0], sgn, phi)[:, 0]
    pr = scale * p0_exact(fn_aer or fn_atm, c.mu, [c.mu0], sgn, phi)[:, 0]
    if any(z.kind == "mix" for z in c.zones):
        first = np.stack([VN.first_order(c, pa[i], pr[i], mu_view) for i in range(len(phi))])
    else:
        first = np.stack([VN.first_order_single_slab(c.tau, c.tauStar_tot, c.mu0, c.alb_atm, pa[i], mu_view) for i in range(len(phi))])
    return first, scat


def three_zone(mu0, L, N, tau_aer=0.3):
    """(oracle Column for view_np, azimuth_direct.Geometry) of azimuth_direct.three_zone's column."""
    Z1, Z2 = np.zeros(2 * N), np.zeros((2 * N, 2 * N))
    c = O.make_column(mu0, 120, 25, 17, L, 0.124, tau_aer, 0.15, 1.0, 0.95, N, Z1, Z2, Z1, Z2)
    return c, AD.three_zone(mu0, L, N, tau_aer=tau_aer)


def single_slab(mu0, L, N, tau_star=0.5, alb=0.95):
    """The same of azimuth_direct.single_slab (one phase function, no surface)."""
    tau, mu = np.linspace(0.0, tau_star, L), O.make_mu(N)
    return VN.single_slab_column(tau, mu, N, mu0, alb, tau_star), AD.single_slab(mu0, L, N, tau_star=tau_star, alb=alb)
