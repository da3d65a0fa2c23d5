"""Phase matrices of a chosen rank, and an extended-precision source function with the magnitude sums that bound a float
evaluation of it (test infrastructure, plain NumPy, no GPU).

A phase function given as a Legendre series p(cos T) = sum_l a_l P_l(cos T) has the azimuth average
sum_l a_l (-1)^l P_l(mu) P_l(mu') (addition theorem; the sign is the reference's scattering cosine -(mu mu' + ...)): r terms
are a matrix of rank r, flip-symmetric on the symmetric direction grid, and -- after the reference's column normalisation, a
scaling of the columns -- still of rank r.  That is the input the low-rank form of the plain rows (csrc/jn_gemm_tile.hpp,
lowrank_rows) needs to be driven at every rank it has code for."""
import numpy as np
from numpy.polynomial import legendre as _leg

_trapz = getattr(np, "trapezoid", None) or np.trapz

COEFFS = [1.0, 0.9, 0.5, 0.3, 0.2]      # a_l: terms(r) = COEFFS[:r]; min p = 0.2 > 0 for every r, so columns converge
U64 = 2.0 ** -53                        # unit roundoff, double
U32 = 2.0 ** -24                        # unit roundoff, float


def terms(r):
    return COEFFS[:r]


def legendre_phase(N, mu, a, mu0=None, no_flip=False):
    """P [2N, 2N] of the series `a` with the reference's column normalisation trapz(P[:, n], mu) = 4 (phase:131), and
    P0 [2N] with trapz = 2 (phase:103) when `mu0` is given (else None).  `a` empty: zeros (a zero matrix has no
    normalisation).  no_flip: 0.4 P_1(mu) P_0(mu') is added before normalising -- inside the span of the series' own terms
    when it has two or more, so the rank stays (<= 4 in any case), but P[2N-1-i, 2N-1-j] != P[i, j]."""
    D = 2 * N
    a = np.asarray(a, dtype=np.float64)
    if a.size == 0:
        return (np.zeros((D, D)), np.zeros(D) if mu0 is not None else None)
    sgn = (-1.0) ** np.arange(a.size)
    Pl = _leg.legvander(mu, a.size - 1).T                      # [l, D]
    S = np.einsum("l,li,lj->ij", a * sgn, Pl, Pl)
    if no_flip:
        S = S + 0.4 * np.outer(mu, np.ones(D))
    P = 4 * S / _trapz(S, mu, axis=0)[None, :]
    P0 = None
    if mu0 is not None:
        p0 = (a * sgn * _leg.legvander(np.array([float(mu0)]), a.size - 1)[0]) @ Pl
        if no_flip:
            p0 = p0 + 0.4 * mu
        P0 = p0 / _trapz(p0, mu) * 2
    return P, P0


def factor(W, rmax=4, tol=1e-12):
    """The library's cross approximation (plan.cpp, lowrank_factor) in NumPy: U [D, r], V [r, D]."""
    R = W.copy()
    wmax = np.max(np.abs(W))
    U, V = [], []
    for _ in range(rmax + 1):
        i, j = np.unravel_index(np.argmax(np.abs(R)), R.shape)
        if abs(R[i, j]) <= tol * wmax:
            break
        U.append(R[:, j] / R[i, j])
        V.append(R[i, :].copy())
        R = R - np.outer(U[-1], V[-1])
    assert len(U) <= rmax
    U = np.array(U).T.reshape(W.shape[0], len(U))
    V = np.array(V).reshape(len(V), W.shape[1])
    assert np.max(np.abs(W - U @ V)) <= tol * wmax
    return U, V


def rank_of(W, rmax=4, tol=1e-12):
    """(rank or -1, last pivot / max |W|) of `factor`'s elimination, without its assertions: what sosrt_phase_rank answers."""
    R = W.copy()
    wmax = np.max(np.abs(W))
    if wmax == 0:
        return 0, 0.0
    for r in range(rmax + 1):
        i, j = np.unravel_index(np.argmax(np.abs(R)), R.shape)
        if abs(R[i, j]) <= tol * wmax:
            return r, abs(R[i, j]) / wmax
        if r == rmax:
            return -1, abs(R[i, j]) / wmax
        R = R - np.outer(R[:, j] / R[i, j], R[i, :].copy())


def fold_ld(P, mu):
    """gpu_model.fold_weights in long double: W[k, m] = w_k P[m, D-1-k]."""
    m = np.asarray(mu, dtype=np.longdouble)
    d = np.diff(m)
    w = np.zeros_like(m)
    w[:-1] += d / 2
    w[1:] += d / 2
    return w[:, None] * np.asarray(P, dtype=np.longdouble)[:, ::-1].T


def _magnitude(Xabs, mu, P_atm, P_aer, ca, cr):
    S = np.abs(np.asarray(ca, dtype=np.longdouble))[:, None] * (Xabs @ np.abs(fold_ld(P_atm, mu)))
    if P_aer is not None and np.any(np.asarray(cr) != 0):
        S = S + np.abs(np.asarray(cr, dtype=np.longdouble))[:, None] * (Xabs @ np.abs(fold_ld(P_aer, mu)))
    return S


def source_ld(X, mu, P_atm, P_aer, ca, cr):
    """Jn_NumInt's sum (I1_In:62-74: c trapz(P[:, ::-1] In_1[t], mu, axis=1)) for the rows X [T, D] with every operand in
    long double; ca, cr [T]: the rows' coefficients as gpu_model.source_model takes them (cr = 0: a plain row, which reads
    W_atm alone).  Returns (J [T, D] long double, S [T, D] with S[t, m] = sum_k |c X[t, k] W[k, m]| over the matrices the row
    reads)."""
    ld = np.longdouble
    X = np.asarray(X, dtype=ld)
    d = np.diff(np.asarray(mu, dtype=ld))
    T, D = X.shape
    J = np.zeros((T, D), dtype=ld)
    mats = [(np.asarray(ca, dtype=ld), P_atm)]
    if P_aer is not None and np.any(np.asarray(cr) != 0):
        mats.append((np.asarray(cr, dtype=ld), P_aer))
    for c, P in mats:
        Pf = np.asarray(P, dtype=ld)[:, ::-1]
        for t in range(T):
            if c[t] == 0:
                continue
            f = Pf * X[t][None, :]
            J[t] += c[t] * (((f[:, 1:] + f[:, :-1]) * d[None, :]).sum(axis=1) / 2)
    return J, _magnitude(np.abs(X), mu, P_atm, P_aer, ca, cr)


def mirrored(X):
    """|X[k]| + |X[D-1-k]|: what takes the place of |X[k]| in S for the flip-symmetric form, which sums x +- x' first."""
    A = np.abs(np.asarray(X, dtype=np.longdouble))
    return A + A[..., ::-1]


def lowrank_magnitude(X, U, V, ca):
    """|c| sum_q |V[q, m]| sum_k |X[t, k] U[k, q]|  [T, D]: the magnitude sum of the factored plain rows ca (X U) V."""
    ld = np.longdouble
    M = np.abs(np.asarray(X, dtype=ld)) @ np.abs(np.asarray(U, dtype=ld))
    return np.abs(np.asarray(ca, dtype=ld))[:, None] * (M @ np.abs(np.asarray(V, dtype=ld)))


def bounds(X, mu, P_atm, P_aer, ca, cr, Wa, sym, UV, lowrank_tol=1e-12):
    """(J_ld, {mode: bound [T, D]}) for the rows X [T, D] of one column: the long-double source function and, per contraction
    mode of sosrt_set_contraction, the bound on |J - J_ld| per element.  Derived from the summations, not measured (u = 2^-53):
      f64_full   (D + 8) u S: one rounding of c x, D accumulations of exact products, a few more for the combined slab matrix.
      f64_dense  the same when the flip-symmetric form does not run (`sym` false); else 4 (D + 8) u S' with S' = S for
                 |X[k]| + |X[D-1-k]| in place of |X[k]|: the form sums x +- x' first and multiplies by the sum and the
                 difference of W's mirrored entries; the factor 4 also holds what the form moves the result by when W is
                 flip-symmetric to rounding only (it multiplies by (W[k][m] + W[D-1-k][D-1-m]) / 2: a few u of max |W|).
      f64        slab rows (cr != 0) as f64_dense; plain rows, with the factors `UV` = (U, V) of W_atm (None: no low-rank form,
                 every row as f64_dense), 4 (D + 8) u |c| sum_q |V[q][m]| sum_k |X[k] U[k][q]| plus the certificate of the
                 factors, lowrank_tol max |W_atm| |c| sum_k |X[k]| (sosrt.h).
      f32        (D + 8) 2^-24 S: float operands and a float accumulator.
    Wa: the float64 folded W_atm (what the handle holds: Solver.plan_fold(0))."""
    ld = np.longdouble
    D = X.shape[1]
    ca_, cr_ = np.abs(np.asarray(ca, dtype=ld))[:, None], np.abs(np.asarray(cr, dtype=ld))[:, None]
    J, S = source_ld(X, mu, P_atm, P_aer, ca, cr)
    sumx = np.abs(np.asarray(X, dtype=ld)).sum(axis=1)[:, None]
    out = {"f64_full": (D + 8) * U64 * S, "f32": (D + 8) * U32 * S}
    if sym:
        dense = 4 * (D + 8) * U64 * _magnitude(mirrored(X), mu, P_atm, P_aer, ca, cr)
    else:
        dense = out["f64_full"]
    out["f64_dense"] = dense
    if UV is None:
        out["f64"] = dense
    else:
        plain = 4 * (D + 8) * U64 * lowrank_magnitude(X, UV[0], UV[1], ca) + lowrank_tol * ld(np.max(np.abs(Wa))) * ca_ * sumx
        out["f64"] = np.where((np.asarray(cr) != 0)[:, None], dense, plain)
    return J, out


def worst_ratio(J, J_ld, bound):
    """max over the elements of |J - J_ld| / bound; an element whose bound is zero must be exact (inf otherwise)."""
    err = np.abs(np.asarray(J, dtype=np.longdouble) - J_ld)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))
