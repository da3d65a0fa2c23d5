"""NumPy model of the view radiance over a BRDF ground, written from the definitions and not from the kernels,
on tests/brdf_np.py, brdf_azimuth_np.py, view_np.py and view_azimuth_np.py.

Over a BRDF ground the field is the sum over ground reflections I = sum_k I(k) (section 20), and the radiance at a view lane is

    first order over the black ground  +  the view stage on the summed field  +  the ground's own unscattered radiance,

the last being, on the upward lane of view cosine v,

    sum_k S_k[v] exp(-(tau[L-1] - tau[t]) / v),
    S_k[v] = scale (sum_j Rv[v, j] I(k-1)[L-1][j] + [k = 1] rho_bar(v, mu0) exp(-tau[L-1] / mu0)),   Rv[v, j] = 2 w_j |mu_j| rho_bar(v, |mu_j|),

and 0 on the downward lanes; no view lane is blended.  Per azimuth mode m the same with (-1)^m Rv^m, rho^m and the mode's fields.
Here: the rows and beam rows at view cosines (azimuth mean, modes, exact azimuth), the ground term, the series in ground
reflections with its view hook (on the oracle at natural scale; per mode with fixed counts), and a DIRECT reference on uniform
azimuth nodes in which nothing goes through a mode.  Rows are [v, j] here; the device stores the transpose."""
import numpy as np

import azimuth_direct as D
import azimuth_np as A
import brdf_azimuth_np as BA
import brdf_np as G
import sos_oracle as O
import view_azimuth_np as VA
import view_np as VN


# ---- rows at view cosines ---------------------------------------------------------------------------------------------------------
def _flux_weights(mu, N):
    return 2 * G.trapezoid_weights(mu[:N - 1]) * -mu[:N - 1]


def view_rows(mu, N, mu_view, brdf, nphi=65):
    """Rv[v, j] = 2 w_j |mu_j| rho_bar(mu_view_v, |mu_j|): brdf_np.operator with the view cosines in place of the upward nodes"""
    mv = np.asarray(mu_view, dtype=np.float64)
    return _flux_weights(mu, N)[None, :] * G.rho_bar(brdf, mv[:, None], -mu[:N - 1][None, :], nphi)


def view_rows_modes(mu, N, mu_view, brdf, ms, nphi=65):
    """Rv^m[v, j] = 2 w_j |mu_j| rho^m(mu_view_v, |mu_j|): [len(ms), V, N-1]"""
    mv = np.asarray(mu_view, dtype=np.float64)
    return _flux_weights(mu, N)[None, None, :] * BA.rho_modes(brdf, mv[:, None], -mu[:N - 1][None, :], ms, nphi)


def view_beam_row(mu_view, mu0, brdf, nphi=65):
    """rho_bar(mu_view_v, mu0): [V]"""
    return G.rho_bar(brdf, np.asarray(mu_view, dtype=np.float64), mu0, nphi)


def view_beam_modes(mu_view, mu0, brdf, ms, nphi=65):
    """rho^m(mu_view_v, mu0): [len(ms), V]"""
    return BA.rho_modes(brdf, np.asarray(mu_view, dtype=np.float64), mu0, ms, nphi)


def view_beam_azimuth(mu_view, mu0, brdf, phi):
    """rho(mu_view_v, mu0, phi_q) at the azimuth itself (phi = 0: the hot spot): [len(phi), V]"""
    mv = np.asarray(mu_view, dtype=np.float64)
    return G._rho(brdf)(mv[None, :], mu0, np.atleast_1d(np.asarray(phi, dtype=np.float64))[:, None])


def view_ground(S, tau, mu_view):
    """[L, 2V]: lanes V + v = S[v] exp(-(tau[L-1] - tau[t]) / mu_view_v), lanes v = 0; nothing is blended"""
    mv = np.asarray(mu_view, dtype=np.float64)
    out = np.zeros((len(tau), 2 * len(mv)))
    out[:, len(mv):] = S[None, :] * np.exp(-(tau[-1] - tau)[:, None] / mv[None, :])
    return out


# ---- natural scale: the series in ground reflections on the oracle, with the view hook ------------------------------------------------
def bounce_solve_view(c, brdf, mu_view, scale=1.0, tol=1e-4, max_bounces=32, nphi=65, max_orders=10000):
    """brdf_np.bounce_solve for one column `c` (its ground replaced by a black one) over the named BRDF, keeping what the view stage
    needs.  Returns a dict: I [L, 2N] the sum, last [L, 2N] the sum of every term's last order, ground [L, 2V] the ground's term at
    the view lanes, bounces, orders (of the black solve and of every reflection), status."""
    c = G.black(c)
    mu, N = c.mu, c.N
    R, r0 = G.operator(mu, N, brdf, nphi), G.beam_row(mu, N, c.mu0, brdf, nphi)
    Rv, r0v = view_rows(mu, N, mu_view, brdf, nphi), view_beam_row(mu_view, c.mu0, brdf, nphi)
    sol = O.solve_column(c, tol=tol, literal=False, max_orders=max_orders)
    total, last, prev = sol.I.copy(), sol.I_saved[-1].copy(), sol.I
    ground = np.zeros((len(c.tau), 2 * len(mu_view)))
    orders, status, bounces = [sol.n], 0, 0
    for k in range(1, max_bounces + 1):
        beam = k == 1
        S = G.ground_source(R, prev[-1], r0 if beam else None, c.tau[-1], c.mu0, scale)
        ground += view_ground(G.ground_source(Rv, prev[-1], r0v if beam else None, c.tau[-1], c.mu0, scale), c.tau, mu_view)
        Gf, st, _ = G.ground_field(S, c.tau, mu, N)
        status = status or st
        sk = O.solve_column(c, tol=tol, literal=False, I1=Gf, max_orders=max_orders)
        total, last, prev = total + sk.I, last + sk.I_saved[-1], sk.I
        orders.append(sk.n)
        if G.bounce_ratio(sk.I, total, N) < tol:
            bounces = k
            break
    return dict(I=total, last=last, ground=ground, bounces=bounces, orders=orders, status=status, column=c)


def node_view(c, I_src, mv, lanes):
    """(first, scattered) [L, 2V] of the view stage at the grid's own lanes (view_np.node_views), GRID quadrature, over the black
    column `c` whose P and P0 are the grid's"""
    S = VN.source(c, c.P_atm[lanes], c.P_aer[lanes], I_src)
    return VN.first_order(c, c.P0_atm[lanes], c.P0_aer[lanes], mv), VN.transport(c, S, mv, VN.QUAD_GRID)


def node_pin(c, brdf, scale=1.0, tol=1e-4, nphi=65):
    """The node pin of DESIGN section 22 for one column at natural scale: (distance of I_view from the model's own I on the
    untouched upward lanes in units of the field maximum, the number of those lanes, mask [V] of them, the series).  With
    I_src = I minus every term's last order the three terms reproduce I exactly on every upward lane that no blend rewrote
    (first order, ground rows or upward sweep): those lanes are found that way (< 1e-12 on every row).  With I_src = I, what the
    drivers pass, the stage adds the series' next term: a distance of the order of tol."""
    mv, lanes = VN.node_views(c.mu, c.N)
    V = len(mv)
    r = bounce_solve_view(c, brdf, mv, scale, tol, nphi=nphi)
    cb = r["column"]
    mx = np.max(np.abs(r["I"]))
    first, exact = node_view(cb, r["I"] - r["last"], mv, lanes)
    err = np.abs(first + exact + r["ground"] - r["I"][:, lanes]) / mx
    ok = VN.untouched_up(err)
    _, scat = node_view(cb, r["I"], mv, lanes)
    dist = np.abs(first + scat + r["ground"] - r["I"][:, lanes])[:, V:][:, ok] / mx
    return float(np.max(dist)), int(ok.sum()), ok, r


# ---- the series per azimuth mode with fixed counts, with the view hook ------------------------------------------------------------------
def black_column(mu0, L, N, tau_aer=0.3, alb_aer=0.95, tau_atm=0.124):
    """(oracle Column for view_np, brdf_azimuth_np.Ground) of brdf_azimuth_np.black_three_zone's column over a black ground"""
    Z1, Z2 = np.zeros(2 * N), np.zeros((2 * N, 2 * N))
    c = O.make_column(mu0, 120, 25, 17, L, tau_atm, tau_aer, 0.0, 1.0, alb_aer, N, Z1, Z2, Z1, Z2)
    return c, BA.black_three_zone(mu0, L, N, tau_aer, alb_aer, tau_atm)


def mode_series_view(c, gr, fn_atm, fn_aer, brdf, M, nphi, n, n_bounce, mu_view, quadrature, scale=1.0, brdf_nphi=65,
                     ground_scale=1.0, sign=True, beam_in_modes=True, log=None):
    """brdf_azimuth_np.mode_series with the view stage per mode.  Returns a dict of arrays [M + 1, L, ...]: I the mode fields
    [.., 2N]; first, scattered, ground [.., 2V] at the view lanes -- first: the closed-form first order of the mode's P0 over the
    black ground; scattered: the view stage on the mode's SUMMED field with (-1)^m rows^m; ground: per reflection the ground source
    at the view cosines with (-1)^m Rv^m (sign=False: Rv^m and R^m themselves), attenuated.  beam_in_modes=False leaves the beam's
    single reflection out of `ground` (the drivers' view_first_order='exact' takes it at the azimuth itself: `beam_ground`)."""
    geo = gr.geo
    mu, N, mu0 = geo.mu, geo.N, geo.mu0
    fn_aer = fn_aer or fn_atm
    ms = list(range(M + 1))
    Rm, r0m = BA.operator_modes(mu, N, brdf, ms, brdf_nphi), BA.beam_modes(mu, N, mu0, brdf, ms, brdf_nphi)
    Rvm, r0vm = view_rows_modes(mu, N, mu_view, brdf, ms, brdf_nphi), view_beam_modes(mu_view, mu0, brdf, ms, brdf_nphi)
    out = dict(I=[], first=[], scattered=[], ground=[])
    worst = 0
    for m in ms:
        q = 25 if m == 0 else nphi
        Pa, Pr = A.solve_modes(fn_atm, mu, [m], q)[0], A.solve_modes(fn_aer, mu, [m], q)[0]
        P0a, P0r = A.phase_p0_modes(fn_atm, mu, mu0, [m], q)[0], A.phase_p0_modes(fn_aer, mu, mu0, [m], q)[0]
        total = prev = D.fixed_orders(geo, scale * P0a, Pa, scale * P0r, Pr, n)
        sg = (-1) ** m if sign else 1
        ground = np.zeros((len(gr.tau), 2 * len(mu_view)))
        for k, nk in enumerate(n_bounce, start=1):
            beam = k == 1
            S = G.ground_source(sg * Rm[m], prev[-1], scale * r0m[m] if beam else None, gr.tau[-1], mu0, ground_scale)
            Sv = G.ground_source(sg * Rvm[m], prev[-1], scale * r0vm[m] if beam and beam_in_modes else None, gr.tau[-1], mu0, ground_scale)
            ground += view_ground(Sv, gr.tau, mu_view)
            Gf, status = BA._ground_field(S, gr, log)
            worst = worst or status
            prev = BA.orders_from(geo, Gf, Pa, Pr, int(nk))
            total = total + prev
        out["I"].append(total)
        out["ground"].append(ground)
        out["scattered"].append(VA.mode_scattered(c, fn_atm, fn_aer, total, m, mu_view, quadrature, nphi))
        out["first"].append(VN.first_order(c, scale * VA.mode_p0(fn_atm, mu, mu0, mu_view, m, nphi),
                                           scale * VA.mode_p0(fn_aer, mu, mu0, mu_view, m, nphi), mu_view))
    return {k: np.stack(v) for k, v in out.items()}, worst


def beam_ground(gr, brdf, mu_view, phi, scale=1.0, ground_scale=1.0):
    """The beam's single reflection seen from the view lanes at the azimuths phi themselves: [len(phi), L, 2V]"""
    r = view_beam_azimuth(mu_view, gr.geo.mu0, brdf, phi) * np.exp(-gr.tau[-1] / gr.geo.mu0)
    return np.stack([view_ground(ground_scale * scale * r[i], gr.tau, mu_view) for i in range(len(r))])


# ---- direct: uniform azimuth nodes, no Fourier mode anywhere ----------------------------------------------------------------------------
def direct_view_solve(c, gr, fn_atm, fn_aer, brdf, nq, n, n_bounce, mu_view, quadrature, scale=1.0, ground_scale=1.0, log=None):
    """brdf_azimuth_np.direct_solve with the view stage.  Returns (phi [nq / 2 + 1] the solved half of the nodes 2 pi q / nq,
    dict of first, scattered, ground [nq / 2 + 1, L, 2V], the fields [nq, L, 2N]): the first order from p(c) at (lane, phi_q)
    and the transport of the direct source of the summed fields (view_azimuth_np.direct_view); the ground's radiance at
    (lane, phi_q) per reflection from

        Sv_q[v] = ground_scale ((1 / nq) sum_r sum_j 2 w_j |mu_j| rho(mu_view_v, |mu_j|, phi_q - phi_r + pi) I_r[L-1][j]
                                + [k = 1] scale rho(mu_view_v, mu0, phi_q) exp(-tau* / mu0))."""
    geo = gr.geo
    mu, N, mu0 = geo.mu, geo.N, geo.mu0
    fn_aer = fn_aer or fn_atm
    mv = np.asarray(mu_view, dtype=np.float64)
    phi = 2 * np.pi * np.arange(nq) / nq
    half = np.arange(nq // 2 + 1)
    mirror = np.minimum(np.arange(nq), nq - np.arange(nq))
    Ka, Kr = D._kernels(fn_atm, mu, nq), D._kernels(fn_aer, mu, nq)
    rho = G._rho(brdf)
    up, dn = mu[N + 1:], -mu[:N - 1]
    wj = _flux_weights(mu, N)
    Rd = np.stack([wj[None, :] * rho(up[:, None], dn[None, :], phi[d] + np.pi) for d in range(nq)]) / nq
    Rvd = np.stack([wj[None, :] * rho(mv[:, None], dn[None, :], phi[d] + np.pi) for d in range(nq)]) / nq
    att = np.exp(-gr.tau[-1] / mu0)
    beam = np.stack([rho(up, mu0, phi[q]) for q in half]) * att
    beam_v = np.stack([rho(mv, mu0, phi[q]) for q in half]) * att
    first = np.stack([geo.first(scale * A.p0_direct(fn_atm, mu, mu0, phi[q]), scale * A.p0_direct(fn_aer, mu, mu0, phi[q]))
                      for q in half])
    total = prev = BA._direct_orders(geo, Ka, Kr, first, n, nq)
    ground = np.zeros((len(half), len(gr.tau), 2 * len(mv)))
    for k, nk in enumerate(n_bounce, start=1):
        rows = prev[mirror][:, -1, :N - 1]
        S = np.stack([sum(Rd[(q - r) % nq] @ rows[r] for r in range(nq)) for q in half])
        Sv = np.stack([sum(Rvd[(q - r) % nq] @ rows[r] for r in range(nq)) for q in half])
        if k == 1:
            S, Sv = S + scale * beam, Sv + scale * beam_v
        ground += np.stack([view_ground(ground_scale * Sv[i], gr.tau, mv) for i in range(len(half))])
        Gf = np.stack([BA._ground_field(ground_scale * S[i], gr, log)[0] for i in range(len(half))])
        prev = BA._direct_orders(geo, Ka, Kr, Gf, int(nk), nq)
        total = total + prev
    Iq = total[mirror]
    first_v, scat_v = VA.direct_view(c, geo, fn_atm, fn_aer, Iq, mv, phi[half], quadrature, scale)
    return phi[half], dict(first=first_v, scattered=scat_v, ground=ground), Iq


def project_half(X, M):
    """Fourier modes 0..M of X [nq / 2 + 1, ...] given on the solved half of nq uniform nodes (even in phi): [M + 1, ...]"""
    nh = X.shape[0]
    nq = 2 * (nh - 1)
    return D.project(X[np.minimum(np.arange(nq), nq - np.arange(nq))], M)
