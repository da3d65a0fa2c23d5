"""NumPy model of the azimuth-resolved radiance over a BRDF ground, written from the definitions and not from
the kernels: the Fourier modes in azimuth of a BRDF, of its reflection operator and of its beam row; the series in ground
reflections per mode on the oracle; and a direct azimuth-resolved solve with a phi-resolved BRDF ground, in which nothing goes
through a mode.

phi is the ring angle of DESIGN section 11, the propagation azimuth minus the beam's plus pi, the same for every lane: phi = 0 at
an upward mu = mu0 is back-scatter, which is RPV's hot spot phi = 0.  A down-welling lane at ring angle phi_j is reflected into the
lane at phi_i with the BRDF's relative azimuth phi_i - phi_j + pi; the beam stands at ring angle pi, so its reflection into phi_i
has the relative azimuth phi_i.

    rho^m(a, b) = (1 / pi) int_0^pi rho(a, b, phi) cos(m phi) dphi     (trapezoid rule on nphi nodes of [0, pi])
    S^m = scale ((-1)^m R^m I^m[L-1] + [bounce 1] rho^m(., mu0) exp(-tau* / mu0)),   R^m[i, j] = 2 w_j |mu_j| rho^m(mu_i, |mu_j|)

Lanes and layouts as in tests/brdf_np.py (R[i, j] here; the device stores the transpose)."""
import dataclasses

import numpy as np

import azimuth_direct as D
import azimuth_np as A
import brdf_np as G
import sos_oracle as O

_trapz = G._trapz


def mode_cos(m, nphi):
    """cos(m phi_q) at the nodes phi_q = pi q / (nphi - 1): the nodes are a regular division of the circle, so the angle is taken
    of the integer m q modulo 2 (nphi - 1), folded onto [0, pi] -- cos(m phi) as written loses m ulps of the angle"""
    half = nphi - 1
    r = (int(m) * np.arange(nphi)) % (2 * half)
    r = np.where(r > half, 2 * half - r, r)
    c = np.cos(np.pi * r / half)
    c[2 * r == half] = 0.0
    return c


def rho_modes(brdf, a, b, ms, nphi=65):
    """rho^m for the modes `ms` and broadcastable a, b: [len(ms), ...]"""
    phi = np.linspace(0, np.pi, nphi)
    a, b = np.asarray(a, dtype=np.float64)[..., None], np.asarray(b, dtype=np.float64)[..., None]
    rho = G._rho(brdf)(a, b, phi)
    return np.stack([_trapz(rho * mode_cos(m, nphi), phi, axis=-1) / np.pi for m in ms])


def operator_modes(mu, N, brdf, ms, nphi=65):
    """R^m[i, j] = 2 w_j |mu_j| rho^m(mu[N+1+i], |mu_j|): [len(ms), N-1, N-1]"""
    up, dn = mu[N + 1:], -mu[:N - 1]
    return 2 * (G.trapezoid_weights(mu[:N - 1]) * dn)[None, None, :] * rho_modes(brdf, up[:, None], dn[None, :], ms, nphi)


def beam_modes(mu, N, mu0, brdf, ms, nphi=65):
    """r0^m[i] = rho^m(mu[N+1+i], mu0): [len(ms), N-1]"""
    return rho_modes(brdf, mu[N + 1:], mu0, ms, nphi)


# ---- the columns: three zones over a black ground -------------------------------------------------------------------------------
@dataclasses.dataclass
class Ground:
    """A three-zone column over a black ground as the oracle solves it (azimuth_direct.Geometry) with its optical depths."""
    geo: D.Geometry
    tau: np.ndarray


def black_three_zone(mu0, L, N, tau_aer=0.3, alb_aer=0.95, tau_atm=0.124):
    """The column of azimuth_direct.three_zone (120 km, slab 17-25 km) over a black ground: the specular surface with albedo 0."""
    Z1, Z2 = np.zeros(2 * N), np.zeros((2 * N, 2 * N))
    c = O.make_column(mu0, 120, 25, 17, L, tau_atm, tau_aer, 0.0, 1.0, alb_aer, N, Z1, Z2, Z1, Z2)
    w_atm, w_aer = np.zeros(L), np.zeros(L)
    for z in c.zones:
        fa, fr = c.zone_fractions(z) if z.kind == "mix" else (1.0, 0.0)
        w_atm[z.r0:z.r1 + 1] = c.alb_atm / 4 * fa
        w_aer[z.r0:z.r1 + 1] = z.alb_aer / 4 * fr
    geo = D.Geometry(
        mu=c.mu, N=N, mu0=mu0,
        first=lambda P0a, P0r: O.first_order(dataclasses.replace(c, P0_atm=P0a, P0_aer=P0r)),
        source=lambda Pa, Pr, I: O.source_function(dataclasses.replace(c, P_atm=Pa, P_aer=Pr), I),
        transport=lambda J: O.transport(c, J, literal=False), w_atm=w_atm, w_aer=w_aer)
    return Ground(geo=geo, tau=c.tau)


def orders_from(geo, I1, Pa, Pr, K):
    """Orders 1..K of the oracle's loop started from the field I1, summed (azimuth_direct.fixed_orders with a given first order)"""
    In = I1
    I = I1.copy()
    for _ in range(2, K + 1):
        In = geo.transport(geo.source(Pa, Pr, In))
        I = I + In
    return I


@dataclasses.dataclass
class BlendLog:
    """Whether every search of the mu -> 0+ blend stopped at its first test: the oracle's (azimuth_direct.record_blend) and the
    ground rows' (brdf_np.ground_field blends lane N+1 alone exactly then)."""
    oracle: list = dataclasses.field(default_factory=list)
    ground: list = dataclasses.field(default_factory=list)

    def first_test_everywhere(self):
        return bool(self.oracle) and all(self.oracle) and bool(self.ground) and all(self.ground)


def _ground_field(S, gr, log):
    N = gr.geo.N
    Gf, status, blended = G.ground_field(S, gr.tau, gr.geo.mu, N)
    if log is not None:
        log.ground.append(status == 0 and not blended[:, N + 2:].any())
    return Gf, status


# ---- the series in ground reflections per mode, on the oracle ---------------------------------------------------------------------
def mode_series(gr, fn_atm, fn_aer, brdf, M, nphi, n, n_bounce, scale=1.0, brdf_nphi=65, ground_scale=1.0, sign=True, log=None):
    """I^m [M + 1, L, 2N] over the BRDF ground: per mode the black solve of `n` orders with (-1)^m P^m (mode 0 on the reference's
    25 nodes, modes m >= 1 on `nphi`: azimuth_direct.mode_fields), then the reflections k = 1 .. len(n_bounce) of n_bounce[k - 1]
    orders each with (-1)^m R^m and r0^m on `brdf_nphi` nodes.  `scale` multiplies P0 and the beam row (the linear regime).
    sign=False reflects through R^m itself, without the (-1)^m.  Also returns the worst status of the ground rows."""
    geo = gr.geo
    mu, N, mu0 = geo.mu, geo.N, geo.mu0
    fn_aer = fn_aer or fn_atm
    ms = list(range(M + 1))
    Rm, r0m = operator_modes(mu, N, brdf, ms, brdf_nphi), beam_modes(mu, N, mu0, brdf, ms, brdf_nphi)
    out, worst = [], 0
    for m in ms:
        q = 25 if m == 0 else nphi
        Pa, Pr = A.solve_modes(fn_atm, mu, [m], q)[0], A.solve_modes(fn_aer, mu, [m], q)[0]
        P0a, P0r = A.phase_p0_modes(fn_atm, mu, mu0, [m], q)[0], A.phase_p0_modes(fn_aer, mu, mu0, [m], q)[0]
        total = prev = D.fixed_orders(geo, scale * P0a, Pa, scale * P0r, Pr, n)
        R = (-1) ** m * Rm[m] if sign else Rm[m]
        for k, nk in enumerate(n_bounce, start=1):
            S = G.ground_source(R, prev[-1], scale * r0m[m] if k == 1 else None, gr.tau[-1], mu0, ground_scale)
            Gf, status = _ground_field(S, gr, log)
            worst = worst or status
            prev = orders_from(geo, Gf, Pa, Pr, int(nk))
            total = total + prev
        out.append(total)
    return np.stack(out), worst


# ---- the direct azimuth-resolved solve over a phi-resolved BRDF ground ---------------------------------------------------------------
def _direct_orders(geo, Ka, Kr, In, K, nq):
    """Orders 1..K on the solved half of the nodes, started from In [nq / 2 + 1, L, 2N] (the loop of azimuth_direct.direct_solve)"""
    half = np.arange(nq // 2 + 1)
    mirror = np.minimum(np.arange(nq), nq - np.arange(nq))
    rows_aer = np.flatnonzero(geo.w_aer)
    wa, wr = geo.w_atm[None, :, None], geo.w_aer[None, rows_aer, None]
    I = In.copy()
    for _ in range(2, K + 1):
        full = In[mirror]
        J = np.zeros_like(In)
        for d in range(nq):
            R = full[(half - d) % nq]
            J += wa * (R @ Ka[d].T)
            if len(rows_aer):
                J[:, rows_aer] += wr * (R[:, rows_aer] @ Kr[d].T)
        In = np.stack([geo.transport(J[i]) for i in range(len(half))])
        I = I + In
    return I


def direct_solve(gr, fn_atm, fn_aer, brdf, nq, n, n_bounce, scale=1.0, ground_scale=1.0, log=None):
    """(phi [nq], I [nq, L, 2N]): the azimuth-resolved field on nq uniform nodes phi_q = 2 pi q / nq over the BRDF ground, solved
    directly.  The black solve of `n` orders is azimuth_direct's; reflection k takes the previous term's surface rows of all
    nodes r to the ground source of node q,

        S_q[i] = ground_scale ((1 / nq) sum_r sum_j 2 w_j |mu_j| rho(mu_i, |mu_j|, phi_q - phi_r + pi) I_r[L-1][j]
                               + [k = 1] scale rho(mu_i, mu0, phi_q) exp(-tau* / mu0)),

    its unscattered field with the blend (brdf_np.ground_field) is the first order of n_bounce[k - 1] direct orders, and the
    terms are summed.  The sun lies in the plane phi = 0 and rho is even in phi, so I_q = I_{nq - q}."""
    geo = gr.geo
    mu, N, mu0 = geo.mu, geo.N, geo.mu0
    fn_aer = fn_aer or fn_atm
    phi = 2 * np.pi * np.arange(nq) / nq
    half = np.arange(nq // 2 + 1)
    mirror = np.minimum(np.arange(nq), nq - np.arange(nq))
    Ka, Kr = D._kernels(fn_atm, mu, nq), D._kernels(fn_aer, mu, nq)
    rho = G._rho(brdf)
    up, dn = mu[N + 1:], -mu[:N - 1]
    wj = 2 * G.trapezoid_weights(mu[:N - 1]) * dn
    # Rd[d][i, j]: the operator at the relative azimuth phi_d + pi, d = q - r
    Rd = np.stack([wj[None, :] * rho(up[:, None], dn[None, :], phi[d] + np.pi) for d in range(nq)]) / nq
    beam = np.stack([rho(up, mu0, phi[q]) for q in half]) * np.exp(-gr.tau[-1] / mu0)
    first = np.stack([geo.first(scale * A.p0_direct(fn_atm, mu, mu0, phi[q]), scale * A.p0_direct(fn_aer, mu, mu0, phi[q]))
                      for q in half])
    total = prev = _direct_orders(geo, Ka, Kr, first, n, nq)
    for k, nk in enumerate(n_bounce, start=1):
        rows = prev[mirror][:, -1, :N - 1]                                      # [nq, N-1] the downward surface rows
        S = np.stack([sum(Rd[(q - r) % nq] @ rows[r] for r in range(nq)) for q in half])
        if k == 1:
            S = S + scale * beam
        Gf = np.stack([_ground_field(ground_scale * S[i], gr, log)[0] for i in range(len(half))])
        prev = _direct_orders(geo, Ka, Kr, Gf, int(nk), nq)
        total = total + prev
    return phi, total[mirror]
