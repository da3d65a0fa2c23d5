"""Direct azimuth-resolved solve, the reference the Fourier modes of DESIGN section 11 are tested against.

The field is kept on `nq` uniform azimuth nodes phi_q = 2 pi q / nq, I[q][L][2N].  Its first order is the oracle's with the
phi-resolved single-scattering phase function p(c(mu, mu0, phi_q)) / Z0 (azimuth_np.p0_direct).  Each further order
couples every pair of nodes through the physical scattering kernel: the source of node q is the sum over nodes r of the
column's zone mix of

    S_Delta[a][b'] = p(c(a, b', Delta + pi)) * 4 / Z_b' / nq,    Delta = phi_q - phi_r,

stored for the oracle's fold (its source function reads P[a][flip b]; with the reference's cosine
c(a, b, phi) = -(mu_a mu_b + s_a s_b cos phi), the pair (a, flip b) at Delta + pi is the physical cosine at Delta), with Z the
reference's 25-node mode-0 normaliser.  The transport of every node is the oracle's own.  Nothing here goes through a
Fourier mode, so it checks the convention the mode builders use.

The oracle's mu -> 0+ upward blend (`_blend_small_up`) searches for the first row whose second difference falls to an
absolute 1e-4, so its stopping row depends on the field and the solve is linear in P0 only when every search stops at its
first test.  `record_blend` records that; the exact comparisons scale P0 down (by 1e-6) until it holds."""
import contextlib
import dataclasses

import numpy as np

import azimuth_np as A
import sos_oracle as O

_trapz = getattr(np, "trapezoid", None) or np.trapz


@contextlib.contextmanager
def record_blend():
    """Wraps the oracle's upward blend for the duration; yields a list that gets, per call, whether the search stopped at
    its first test (the oracle itself is not edited)."""
    orig = O._blend_small_up

    def wrapped(row, mu, N):
        k = N + 1
        log.append(not np.abs((row[k] - row[k + 1]) - (row[k + 1] - row[k + 2])) > 0.0001)
        return orig(row, mu, N)
    log = []
    O._blend_small_up = wrapped
    try:
        yield log
    finally:
        O._blend_small_up = orig


@dataclasses.dataclass
class Geometry:
    """One column as the oracle solves it: first order, source function and transport, plus the coefficients of the
    atmosphere and aerosol kernels per row (alb / 4 times the zone's fraction) for the direct source."""
    mu: np.ndarray
    N: int
    mu0: float
    first: object          # (P0_atm, P0_aer) -> I1 [L, 2N]
    source: object         # (P_atm, P_aer, In_1) -> Jn [L, 2N]
    transport: object      # Jn -> In [L, 2N]
    w_atm: np.ndarray
    w_aer: np.ndarray


def three_zone(mu0, L, N, tau_aer=0.3):
    """The column of tests/test_gpu_azimuth.py `_three_zone`: 120 km, slab 17-25 km, tau_atm 0.124, ground albedo 0.15,
    albedos 1.0 / 0.95, specular surface."""
    Z1, Z2 = np.zeros(2 * N), np.zeros((2 * N, 2 * N))
    c = O.make_column(mu0, 120, 25, 17, L, 0.124, tau_aer, 0.15, 1.0, 0.95, N, Z1, Z2, Z1, Z2)
    w_atm, w_aer = np.zeros(L), np.zeros(L)
    for z in c.zones:
        fa, fr = c.zone_fractions(z) if z.kind == "mix" else (1.0, 0.0)
        w_atm[z.r0:z.r1 + 1] = c.alb_atm / 4 * fa
        w_aer[z.r0:z.r1 + 1] = z.alb_aer / 4 * fr
    return Geometry(
        mu=c.mu, N=N, mu0=mu0,
        first=lambda P0a, P0r: O.first_order(dataclasses.replace(c, P0_atm=P0a, P0_aer=P0r)),
        source=lambda Pa, Pr, I: O.source_function(dataclasses.replace(c, P_atm=Pa, P_aer=Pr), I),
        transport=lambda J: O.transport(c, J, literal=False), w_atm=w_atm, w_aer=w_aer)


def single_slab(mu0, L, N, tau_star=0.5, alb=0.95):
    """The reference's single-slab functions (I1_In), one phase function (the atmosphere's), no surface."""
    tau, mu = np.linspace(0.0, tau_star, L), O.make_mu(N)
    return Geometry(
        mu=mu, N=N, mu0=mu0,
        first=lambda P0a, P0r: O.I1_NumInt(tau, mu, tau_star, mu0, P0a, alb, N),
        source=lambda Pa, Pr, I: O.Jn_NumInt(0, I, tau, mu, tau_star, mu0, Pa, alb, N),
        transport=lambda J: O.In_NumInt(0, J, None, tau, mu, tau_star, mu0, None, alb, N, literal=False),
        w_atm=np.full(L, alb / 4), w_aer=np.zeros(L))


def fixed_orders(geo, P0a, Pa, P0r, Pr, K):
    """Orders 1..K of the oracle's loop, summed (no convergence test: a mode has none)."""
    In = geo.first(P0a, P0r)
    I = In.copy()
    for _ in range(2, K + 1):
        In = geo.transport(geo.source(Pa, Pr, In))
        I = I + In
    return I


def mode_fields(geo, fn_atm, fn_aer, M, nphi, K, scale=1.0, fold_sign=True):
    """I^m [M + 1, L, 2N] from the NumPy restatement of the builders (azimuth_np): mode 0 on the reference's 25 nodes,
    modes 1..M on `nphi`, each solved with (-1)^m P^m (azimuth_np.solve_modes).  `fn_aer` None: the atmosphere's function
    for both.  fold_sign=False solves with P^m itself, without the factor of the fold."""
    fn_aer = fn_aer or fn_atm
    mu, mu0 = geo.mu, geo.mu0
    mats = A.solve_modes if fold_sign else A.phase_modes
    out = []
    for m in range(M + 1):
        n = 25 if m == 0 else nphi
        Pa, Pr = mats(fn_atm, mu, [m], n)[0], mats(fn_aer, mu, [m], n)[0]
        P0a, P0r = A.phase_p0_modes(fn_atm, mu, mu0, [m], n)[0], A.phase_p0_modes(fn_aer, mu, mu0, [m], n)[0]
        out.append(fixed_orders(geo, scale * P0a, Pa, scale * P0r, Pr, K))
    return np.stack(out)


def synthesize(Im, phi):
    """sum_m (2 - delta_m0) I^m cos(m phi): [..., len(phi)]."""
    w = np.where(np.arange(len(Im)) == 0, 1.0, 2.0)[:, None] * np.cos(np.arange(len(Im))[:, None] * np.asarray(phi)[None, :])
    return np.einsum("m...,mj->...j", Im, w)


def project(Iq, M):
    """Fourier modes 0..M of a field on uniform nodes, Iq [nq, L, 2N] -> [M + 1, L, 2N]: (1 / nq) sum_q I_q cos(m phi_q)."""
    nq = Iq.shape[0]
    phi = 2 * np.pi * np.arange(nq) / nq
    return np.einsum("q...,mq->m...", Iq, np.cos(np.arange(M + 1)[:, None] * phi[None, :])) / nq


def _kernels(fn, mu, nq):
    """K[d] [2N, 2N] = S_Delta[:, ::-1] times the trapezoid weights of mu, Delta = phi_d: the source of node q is
    sum_d K[d] I_{q - d} (before the row's albedo factor)."""
    Z = _trapz(O._azimuth_average(fn, mu, mu) / (2 * np.pi), mu, axis=0)         # 25-node mode-0 normaliser, per column b'
    wq = np.zeros(len(mu))
    wq[:-1] += np.diff(mu) / 2
    wq[1:] += np.diff(mu) / 2
    s = np.sqrt(1 - mu * mu)
    K = []
    for d in range(nq):
        delta = 2 * np.pi * d / nq
        c = -(mu[:, None] * mu[None, :] + s[:, None] * s[None, :] * np.cos(delta + np.pi))
        S = fn(c) * 4 / Z[None, :] / nq
        K.append(S[:, ::-1] * wq[None, :])
    return np.stack(K)


def direct_solve(geo, fn_atm, fn_aer, nq, K, scale=1.0):
    """(phi [nq], I [nq, L, 2N]): orders 1..K of the azimuth-resolved field on nq uniform nodes, solved directly.  The sun
    lies in the plane phi = 0, so I_q = I_{nq - q}: nodes 0..nq/2 are solved and mirrored to the rest."""
    fn_aer = fn_aer or fn_atm
    mu, mu0 = geo.mu, geo.mu0
    phi = 2 * np.pi * np.arange(nq) / nq
    half = np.arange(nq // 2 + 1)
    mirror = np.minimum(np.arange(nq), nq - np.arange(nq))    # node q -> its solved twin
    Ka, Kr = _kernels(fn_atm, mu, nq), _kernels(fn_aer, mu, nq)
    rows_aer = np.flatnonzero(geo.w_aer)                       # the aerosol kernel feeds the slab rows only
    wa, wr = geo.w_atm[None, :, None], geo.w_aer[None, rows_aer, None]
    In = np.stack([geo.first(scale * A.p0_direct(fn_atm, mu, mu0, phi[q]), scale * A.p0_direct(fn_aer, mu, mu0, phi[q]))
                   for q in half])
    I = In.copy()
    for _ in range(2, K + 1):
        full = In[mirror]
        J = np.zeros_like(In)
        for d in range(nq):
            R = full[(half - d) % nq]                           # R[q] = In[q - d]
            J += wa * (R @ Ka[d].T)
            if len(rows_aer):
                J[:, rows_aer] += wr * (R[:, rows_aer] @ Kr[d].T)
        In = np.stack([geo.transport(J[i]) for i in range(len(half))])
        I = I + In
    return phi, I[mirror]
