"""NumPy model of the Ross-Thick / Li-Sparse-Reciprocal ground, written from the definitions and not from the
kernels: the two kernels, the weighted BRDF rho = f_iso + f_vol K_vol + f_geo K_geo, the weighted ground source over operator
terms, the albedos on the grid's trapezoid, and the series in ground reflections with every column's own operator.

Importing this module teaches `brdf_np._rho` -- through which brdf_np, brdf_azimuth_np and brdf_view_np resolve a named BRDF --
the names ('ross_thick', mu_floor), ('li_sparse_r', mu_floor) and ('ross_li', f_iso, f_vol, f_geo[, mu_floor]); every other name
goes to the function it replaced, unchanged."""
import numpy as np

import brdf_np as G

MU_FLOOR = 0.17364817766693033            # cos 80 deg
WHITE_SKY = {"ross_thick": 0.189184, "li_sparse_r": -1.377622}      # Lucht et al. (2000), the kernels' bihemispherical integrals
# |white_sky_albedo on the grid's trapezoid (make_mu(N), 65 azimuth nodes, mu_floor = 0) - WHITE_SKY|, measured with this model on
# the CPU; the tests assert twice these
WHITE_SKY_GRID_DISTANCE = {("ross_thick", 64): 8.64e-4, ("ross_thick", 66): 8.14e-4, ("ross_thick", 128): 2.20e-4,
                           ("li_sparse_r", 64): 1.271e-3, ("li_sparse_r", 66): 1.193e-3, ("li_sparse_r", 128): 2.89e-4}


def _dirs(a, b, mu_floor):
    a, b = np.maximum(np.asarray(a, dtype=np.float64), mu_floor), np.maximum(np.asarray(b, dtype=np.float64), mu_floor)
    sa, sb = np.sqrt(np.maximum(0.0, 1 - a * a)), np.sqrt(np.maximum(0.0, 1 - b * b))
    return a, b, sa, sb


def _cos_xi(a, b, sa, sb, phi):
    return np.clip(a * b + sa * sb * np.cos(phi), -1.0, 1.0)


def k_vol(a, b, phi, mu_floor=MU_FLOOR):
    """Ross-Thick: ((pi/2 - xi) cos xi + sin xi) / (a' + b') - pi/4; phi = 0 with a = b is back-scatter"""
    a, b, sa, sb = _dirs(a, b, mu_floor)
    cx = _cos_xi(a, b, sa, sb, phi)
    xi = np.arccos(cx)
    return ((np.pi / 2 - xi) * cx + np.sin(xi)) / (a + b) - np.pi / 4


def k_geo(a, b, phi, mu_floor=MU_FLOOR):
    """Li-Sparse-Reciprocal with h/b = 2, b/r = 1: O - sec + (1 + cos xi) / (2 a' b').  D^2 in brdf_np.rho_rpv's non-cancelling
    form, and sin^2 phi = hav (2 - hav) from the same hav = 1 - cos phi = 2 sin^2(phi / 2)."""
    a, b, sa, sb = _dirs(a, b, mu_floor)
    ta, tb = sa / a, sb / b
    cx = _cos_xi(a, b, sa, sb, phi)
    sec = 1 / a + 1 / b
    hav = 2 * np.sin(np.asarray(phi, dtype=np.float64) / 2) ** 2
    D2 = np.maximum(0.0, (ta - tb) ** 2 + 2 * (ta * tb) * hav)
    ct = np.clip(2 * np.sqrt(D2 + (ta * tb) ** 2 * (hav * (2 - hav))) / sec, -1.0, 1.0)
    t = np.arccos(ct)
    return (t - np.sin(t) * ct) * sec / np.pi - sec + 0.5 * (1 + cx) / (a * b)


def rho_ross_li(a, b, phi, f_iso, f_vol, f_geo, mu_floor=MU_FLOOR):
    return f_iso + f_vol * k_vol(a, b, phi, mu_floor) + f_geo * k_geo(a, b, phi, mu_floor)


_rho_before = G._rho


def _rho(brdf):
    if isinstance(brdf, tuple) and brdf and brdf[0] == "ross_thick":
        return lambda a, b, c: k_vol(a, b, c, *brdf[1:])
    if isinstance(brdf, tuple) and brdf and brdf[0] == "li_sparse_r":
        return lambda a, b, c: k_geo(a, b, c, *brdf[1:])
    if isinstance(brdf, tuple) and brdf and brdf[0] == "ross_li":
        return lambda a, b, c: rho_ross_li(a, b, c, *brdf[1:])
    return _rho_before(brdf)


G._rho = _rho


def terms(mu_floor=MU_FLOOR):
    """the operator terms of a Ross-Li ground as named BRDFs, in the order of the weights"""
    return ("lambertian", ("ross_thick", mu_floor), ("li_sparse_r", mu_floor))


def ground_source_terms(Rs, I_surface, r0s, tau_last, mu0, weight):
    """S = sum_k weight[k] (R_k I[L-1][0 .. N-2] + r0_k exp(-tau[L-1] / mu0)); Rs [K, N-1, N-1] as R[i, j], r0s [K, N-1] or None"""
    S = 0.0
    for k, w in enumerate(weight):
        S = S + w * G.ground_source(Rs[k], I_surface, None if r0s is None else r0s[k], tau_last, mu0)
    return S


def up_weights(mu, N):
    """2 w_i mu_i on the upward nodes mu[N+1 ..], w their trapezoid weights"""
    return 2 * G.trapezoid_weights(mu[N + 1:]) * mu[N + 1:]


def black_sky_albedo(mu, N, r0s, weight):
    """sum_i 2 w_i mu_i sum_k f_k r0_k[i]; r0s [K, N-1]"""
    return float(up_weights(mu, N) @ np.tensordot(weight, r0s, axes=1))


def white_sky_albedo(mu, N, Rs, weight):
    """sum_i 2 w_i mu_i sum_j sum_k f_k R_k[i, j]; Rs [K, N-1, N-1] as R[i, j]"""
    return float(up_weights(mu, N) @ np.tensordot(weight, Rs, axes=1).sum(axis=1))


def bounce_solve_columns(O, cols, Rs, r0s, tol=1e-4, max_bounces=32, max_orders=10000):
    """brdf_np.bounce_solve with every column's own operator Rs[b] [N-1, N-1] and beam row r0s[b] [N-1] (scale 1).  Every column
    runs until all are below `tol`, as the device driver does.  Returns (I [B, L, 2N], bounces [B], ratio [B], status [B])."""
    cols = [G.black(c) for c in cols]
    B, N = len(cols), cols[0].N
    prev = [O.solve_column(c, tol=tol, literal=False, max_orders=max_orders).I for c in cols]
    total = [f.copy() for f in prev]
    bounces, ratio, status = np.zeros(B, dtype=int), np.zeros(B), np.zeros(B, dtype=int)
    for k in range(1, max_bounces + 1):
        cur = []
        for b, c in enumerate(cols):
            S = G.ground_source(Rs[b], prev[b][-1], None if k > 1 else r0s[b], c.tau[-1], c.mu0)
            Gf, st, _ = G.ground_field(S, c.tau, c.mu, N)
            status[b] = status[b] or st
            Ik = O.solve_column(c, tol=tol, literal=False, I1=Gf, max_orders=max_orders).I
            total[b] = total[b] + Ik
            ratio[b] = G.bounce_ratio(Ik, total[b], N)
            if bounces[b] == 0 and ratio[b] < tol:
                bounces[b] = k
            cur.append(Ik)
        prev = cur
        if np.all(ratio < tol):
            break
    status[(bounces == 0) & (status == 0)] = G.COL_MAXORDERS
    bounces[bounces == 0] = max_bounces
    return np.stack(total), bounces, ratio, status
