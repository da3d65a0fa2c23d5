"""NumPy model of the BRDF ground, written from the definitions and not from the kernels: the azimuth mean
of a BRDF, the reflection operator with the flux quadrature folded in, the beam row, the ground source of a surface row, its
unscattered field with the reference's mu -> 0+ blend, and the series in ground reflections on `oracle.solve_column`.

Lanes: i = 0 .. N-2 is the upward direction N+1+i, j = 0 .. N-2 the downward direction j.  R[i, j] here; the device stores the
transpose (the lanes i of one j contiguous)."""
import copy

import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz

COL_OK, COL_INDEXERROR, COL_MAXORDERS = 0, 1, 2


def rho_lambertian(a, b, phi):
    return np.ones(np.broadcast(a, b, phi).shape)


def rho_rpv(a, b, phi, rho0, k, theta):
    """Rahman-Pinty-Verstraete: rho0 (a b (a + b))^(k-1) F(g) (1 + (1 - rho0) / (1 + G)); phi = 0 is the hot spot.  G^2 =
    tan^2 a + tan^2 b - 2 tan a tan b cos phi vanishes there: written as (tan a - tan b)^2 + 4 tan a tan b sin^2(phi / 2), a sum
    of non-negative terms, it neither cancels nor rounds below 0 (the clamp stays)."""
    sa, sb = np.sqrt(np.maximum(0.0, 1 - a * a)), np.sqrt(np.maximum(0.0, 1 - b * b))
    ta, tb = sa / a, sb / b
    cosg = a * b + sa * sb * np.cos(phi)
    F = (1 - theta * theta) / (1 + 2 * theta * cosg + theta * theta) ** 1.5
    G = np.sqrt(np.maximum(0.0, (ta - tb) ** 2 + 4 * (ta * tb) * np.sin(phi / 2) ** 2))
    return rho0 * (a * b * (a + b)) ** (k - 1) * F * (1 + (1 - rho0) / (1 + G))


def _rho(brdf):
    """brdf: 'lambertian' or ('rpv', rho0, k, theta) -> rho(a, b, phi)"""
    if brdf == "lambertian":
        return rho_lambertian
    assert brdf[0] == "rpv"
    return lambda a, b, c: rho_rpv(a, b, c, *brdf[1:])


def rho_bar(brdf, a, b, nphi=65):
    """(1 / pi) int_0^pi rho(a, b, phi) dphi by the trapezoid rule on nphi nodes, for broadcastable a, b"""
    phi = np.linspace(0, np.pi, nphi)
    a, b = np.asarray(a, dtype=np.float64)[..., None], np.asarray(b, dtype=np.float64)[..., None]
    return _trapz(_rho(brdf)(a, b, phi), phi, axis=-1) / np.pi


def trapezoid_weights(x):
    w = np.zeros(len(x))
    w[:-1] += np.diff(x) / 2
    w[1:] += np.diff(x) / 2
    return w


def operator(mu, N, brdf, nphi=65):
    """R[i, j] = 2 w_j |mu_j| rho_bar(mu[N+1+i], |mu_j|), w the trapezoid weights of mu[0 .. N-2]"""
    up, dn = mu[N + 1:], -mu[:N - 1]
    return 2 * (trapezoid_weights(mu[:N - 1]) * dn)[None, :] * rho_bar(brdf, up[:, None], dn[None, :], nphi)


def beam_row(mu, N, mu0, brdf, nphi=65):
    """r0[i] = rho_bar(mu[N+1+i], mu0)"""
    return rho_bar(brdf, mu[N + 1:], mu0, nphi)


def ground_source(R, I_surface, r0, tau_last, mu0, scale=1.0):
    """S = scale (R I[L-1][0 .. N-2] + r0 exp(-tau[L-1] / mu0)); r0 None: no beam term"""
    S = R @ I_surface[:R.shape[1]]
    if r0 is not None:
        S = S + r0 * np.exp(-tau_last / mu0)
    return scale * S


def blend_small_up(row, mu, N):
    """spec:402-409 on one row, in place; False (row untouched) where the reference raises IndexError"""
    k = N + 1
    while True:
        if k + 2 > 2 * N - 1:
            return False
        if not abs((row[k] - row[k + 1]) - (row[k + 1] - row[k + 2])) > 0.0001:
            break
        k += 1
    k += 1
    for m in range(N + 1, k):
        w = mu[m] / mu[k]
        row[m] = (1 - w) * row[N] + w * row[k]
    return True


def ground_field(S, tau, mu, N, blend=True):
    """(G [L, 2N], status, blended [L, 2N] bool): G[t][N+1+i] = S[i] exp(-(tau[L-1] - tau[t]) / mu_i), lane N and the downward
    lanes 0, then the blend on every row"""
    L = len(tau)
    G = np.zeros((L, 2 * N))
    G[:, N + 1:] = S[None, :] * np.exp(-(tau[-1] - tau)[:, None] / mu[N + 1:][None, :])
    raw = G.copy()
    status = COL_OK
    if blend:
        for t in range(L):
            if not blend_small_up(G[t], mu, N):
                status = COL_INDEXERROR
    return G, status, G != raw


def bounce_ratio(Ik, total, N):
    """the larger of max |Ik| / max |total| on the upward lanes of row 0 and on the downward lanes of row L-1 (0 for a zero row)"""
    out = 0.0
    for a, b in ((Ik[0, N:], total[0, N:]), (Ik[-1, :N], total[-1, :N])):
        d = np.max(np.abs(b))
        out = max(out, np.max(np.abs(a)) / d if d > 0 else 0.0)
    return out


def black(c):
    """the column over a black ground: the specular surface with albedo 0"""
    c = copy.copy(c)
    c.surface, c.grd_alb = "specular", 0.0
    return c


def bounce_solve(O, cols, R, r0, scale, tol=1e-4, max_bounces=32, beam=1.0, blend=True, max_orders=10000):
    """The series in ground reflections for the columns `cols` (their ground is replaced by a black one): R [N-1, N-1], r0
    [B, N-1], scale [B]; `beam` multiplies the beam term (the linear regime scales it with P0).  Every column runs until all
    are below `tol`, as the device driver does.  Returns (I [B, L, 2N], bounces [B], ratio [B], status [B], terms): terms[k][b]
    is the field of bounce k (k = 0: the black solve)."""
    cols = [black(c) for c in cols]
    B, N = len(cols), cols[0].N
    first = [O.solve_column(c, tol=tol, literal=False, max_orders=max_orders).I for c in cols]
    total, prev, terms = [f.copy() for f in first], first, [first]
    bounces, ratio, status = np.zeros(B, dtype=int), np.zeros(B), np.zeros(B, dtype=int)
    for k in range(1, max_bounces + 1):
        cur = []
        for b, c in enumerate(cols):
            S = ground_source(R, prev[b][-1], None if k > 1 else beam * r0[b], c.tau[-1], c.mu0, scale[b])
            G, st, _ = ground_field(S, c.tau, c.mu, N, blend)
            status[b] = status[b] or st
            Ik = O.solve_column(c, tol=tol, literal=False, I1=G, max_orders=max_orders).I
            total[b] = total[b] + Ik
            ratio[b] = bounce_ratio(Ik, total[b], N)
            if bounces[b] == 0 and ratio[b] < tol:
                bounces[b] = k
            cur.append(Ik)
        terms.append(cur)
        prev = cur
        if np.all(ratio < tol):
            break
    status[(bounces == 0) & (status == 0)] = COL_MAXORDERS
    bounces[bounces == 0] = max_bounces
    return np.stack(total), bounces, ratio, status, terms


def experiment_column(O, N=64, L=30, mu0=0.6, rho=0.3, p0_scale=1.0, surface="lambertian_readme"):
    """The column of the CPU experiment behind the feature: Rayleigh with an HG(0.6) slab, tau*_aer = 0.3, omega_aer = 0.9"""
    mu = O.make_mu(N)
    P0a, Pa = O.phase_rayleigh(N, mu, mu0)
    P0r, Pr = O.phase_hg(N, mu, mu0, 0.6)
    return O.make_column(mu0, 120, 25, 17, L, 0.124, 0.3, rho, 1.0, 0.9, N, p0_scale * P0a, Pa, p0_scale * P0r, Pr, surface=surface)
