"""The shapes of tests/test_gpu_profile_view.py with their inputs and their models' outputs, computed once
per shape, shared by the tests and never changed.

(L, N, B, V): (40, 32, 5, 3); (41, 33, 3, 1) odd in both; (48, 32, 3, 64) two slabs, five zones, all 64 lanes of a workgroup;
(24, 128, 70, 33) more columns than a wave has lanes; (1024, 32, 2, 2) the cap of the stage, 48 KiB of LDS in the first-order
kernel; (300, 32, 2, 2) with all 300 levels requested in shuffled order and one of them twice, so two launches of 256 and 45.
Columns from profile_np.column (five distinct parameter sets, repeated where B > 5 with weights of their own), weights from
profile_np.random_weights: independent w_atm / w_aer, jumps at the slab's first row and behind its last, rows of exact 0.0 and
1.0.  The view cosines of every shape hold 0.6 = mu0 of column 0 (the phi(0) branch) and, between them, 0.01 and 1.0.

Does float64 NumPy hold the tests' bound of 1e-12 at L = 1024?  `float64_gaps()` evaluates the three models a second time in
np.longdouble and measures float64 against it in the tests' measure (of the column's field maximum);
tests/test_profile_view_host.py asserts every gap <= 1e-13, a tenth of the bound, so the bound is the models' to set."""
import functools

import numpy as np

import profile_np as P
import profile_view_np as PV
import sos_oracle as O
import spherical_np as S
import thermal_np as T
import view_np as VN

SHAPES = {"L40-N32-B5-V3": (40, 32, 5, 3, None), "L41-N33-B3-V1": (41, 33, 3, 1, None), "L48-N32-B3-V64-2slabs": (48, 32, 3, 64, S.TWO_SLABS),
          "L24-N128-B70-V33": (24, 128, 70, 33, None), "L1024-N32-B2-V2": (1024, 32, 2, 2, None), "L300-N32-B2-V2": (300, 32, 2, 2, None)}
CAP = "L1024-N32-B2-V2"
# (mu0, rho, alb_atm, alb_aer) of column b (mod 5); rho = 0 stands for "no surface", which the three-zone geometry has no code for
PAR = [(0.6, 0.3, 1.0, 0.97), (0.45, 0.0, 0.9, 0.8), (0.83, 0.5, 1.0, 1.0), (0.3, 0.1, 0.95, 0.9), (0.7, 0.2, 0.8, 0.97)]
G_AER = 0.7
NSETS = 3


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def _column(N, L, par, slabs_key, surface):
    slabs = S.TWO_SLABS if slabs_key else None
    return P.column(O, N, L, par[0], par[1], slabs, surface, G_AER, par[2], par[3])


@functools.lru_cache(maxsize=None)
def columns(name, surface="specular"):
    L, N, B, _, slabs = SHAPES[name]
    return tuple(_column(N, L, PAR[b % 5], slabs is not None, surface) for b in range(B))


@functools.lru_cache(maxsize=None)
def weights(name):
    """(w_atm [B, L], w_aer [B, L]); the last column keeps unit weights on the atmosphere."""
    cols = columns(name)
    w = [P.random_weights(c, 300 + b) for b, c in enumerate(cols)]
    wa, wr = np.stack([x[0] for x in w]), np.stack([x[1] for x in w])
    wa[-1] = 1.0
    return _frozen(wa, wr)


@functools.lru_cache(maxsize=None)
def view_mu(name):
    V = SHAPES[name][3]
    if V == 1:
        return _frozen(np.array([0.6]))
    if V == 2:
        return _frozen(np.array([0.6, 1.0]) if name == CAP else np.array([0.01, 0.6]))
    mv = np.linspace(0.01, 1.0, V)
    mv[V // 2] = 0.6
    return _frozen(mv)


@functools.lru_cache(maxsize=None)
def levels(name):
    L = SHAPES[name][0]
    rng = np.random.default_rng(5)
    if name.startswith("L300"):
        lev = np.concatenate((rng.permutation(L), [137]))      # every level, shuffled, and one twice: launches of 256 and 45
    else:
        z = columns(name)[0].zones[1]
        lev = rng.permutation(np.array([0, 1, z.r0 - 1, z.r0, z.r1, z.r1 + 1, L - 2, L - 1]))
    return _frozen(lev.astype(np.int32))


def sigma_of(cols, path):
    if path == "plane":
        return np.stack([S.plane_path(c.tau, c.mu0) for c in cols])
    return np.stack([S.slant_path(c.tau, S.altitudes(len(c.tau)), c.mu0) for c in cols])


@functools.lru_cache(maxsize=None)
def p0_rows(name):
    """(p0a, p0r) [NSETS][B][2V]: set 0 the phase functions' own rows at the lanes, the others scaled copies with the lanes
    reversed -- the entry is linear in them and reads nothing else of a set."""
    cols = columns(name)
    sgn = VN.signed(view_mu(name))
    mu0 = np.array([c.mu0 for c in cols])
    fa, fr = VN.phase_fn("rayleigh"), VN.phase_fn("hg", G_AER)
    a, r = VN.phase_p0_rows(fa, cols[0].mu, mu0, sgn), VN.phase_p0_rows(fr, cols[0].mu, mu0, sgn)
    return _frozen(np.stack([a, 1.25 * a[:, ::-1], 0.5 * a]), np.stack([r, 0.8 * r, 1.5 * r[:, ::-1]]))


@functools.lru_cache(maxsize=None)
def phase_rows(name):
    """(rows_atm, rows_aer) [2V][2N] at the signed lanes."""
    mu = columns(name)[0].mu
    sgn = VN.signed(view_mu(name))
    return _frozen(VN.phase_rows(VN.phase_fn("rayleigh"), mu, sgn), VN.phase_rows(VN.phase_fn("hg", G_AER), mu, sgn))


@functools.lru_cache(maxsize=None)
def source_field(name):
    """I_src [B][L][2N]: a positive field that varies with the row and the direction."""
    L, N, B, _, _ = SHAPES[name]
    rng = np.random.default_rng(77)
    return _frozen((0.05 + rng.random((B, L, 2 * N))) * (1 + np.arange(2 * N) / N)[None, None, :])


def planck_of(name):
    L, _, B, _, _ = SHAPES[name]
    b = np.arange(B)
    return T.planck_profile(L)[None, :] * (1 + 0.1 * (b % 7)[:, None]), 1 + 0.05 * (b % 7), 0.95 - 0.01 * (b % 7)


# ---- the models' outputs, all L rows: [..][B][L][2V] ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_first(name, path, dtype=np.float64):
    cols = columns(name)
    wa, wr = weights(name)
    sig = sigma_of(cols, path)
    p0a, p0r = p0_rows(name)
    mv = view_mu(name)
    return _frozen(np.stack([np.stack([PV.view_first_order_profile(c, sig[b], p0a[k, b], p0r[k, b], mv, wa[b], wr[b], dtype)
                                       for b, c in enumerate(cols)]) for k in range(NSETS)]))


@functools.lru_cache(maxsize=None)
def model_emission(name, explicit, dtype=np.float64):
    cols = columns(name)
    wa, wr = weights(name)
    pl, bs, es = planck_of(name)
    mv = view_mu(name)
    return _frozen(np.stack([PV.emission_view_profile(c, pl[b], bs[b], mv, wa[b], wr[b], es[b] if explicit else None, dtype)
                             for b, c in enumerate(cols)]))


@functools.lru_cache(maxsize=None)
def model_scattered(name, quad):
    cols = columns(name)
    wa, wr = weights(name)
    ra, rr = phase_rows(name)
    src = source_field(name)
    mv = view_mu(name)
    return _frozen(np.stack([VN.transport(c, PV.view_source_profile(c, ra, rr, src[b], wa[b], wr[b]), mv, quad)
                             for b, c in enumerate(cols)]))


def col_err(got, ref):
    """max over the columns of max |got - ref| / max |ref| (arrays [B][...])."""
    got, ref = np.asarray(got), np.asarray(ref)
    return max(float(np.max(np.abs(np.asarray(got[b] - ref[b], dtype=np.float64))) / np.max(np.abs(np.asarray(ref[b], dtype=np.float64))))
               for b in range(ref.shape[0]))


def float64_gaps():
    """[(model, gap)] at the cap: float64 against the same formulas in long double, in the tests' measure."""
    out = []
    for path in ("plane", "slant"):
        f, l = model_first(CAP, path), model_first(CAP, path, np.longdouble)
        out.append(("profile_view_np.view_first_order_profile %s" % path, max(col_err(f[k], l[k]) for k in range(NSETS))))
    for explicit in (False, True):
        out.append(("profile_view_np.emission_view_profile emissivity %s" % ("given" if explicit else "1 - rho"),
                    col_err(model_emission(CAP, explicit), model_emission(CAP, explicit, np.longdouble))))
    # the scattered term: the transport of a weighted source; its source is a row-wise product, its sweeps are view_np's
    cols = columns(CAP)
    wa, wr = weights(CAP)
    ra, rr = phase_rows(CAP)
    src = source_field(CAP)
    mv = view_mu(CAP)
    for quad, qn in ((VN.QUAD_GRID, "grid"), (VN.QUAD_LINEAR, "linear")):
        ref = []
        for b, c in enumerate(cols):
            Sv = np.asarray(PV.view_source_profile(c, ra, rr, src[b], wa[b], wr[b]), dtype=np.longdouble)
            ref.append(_transport_long(c, Sv, mv, quad))
        out.append(("view_np.transport of view_source_profile, %s" % qn, col_err(model_scattered(CAP, quad), np.stack(ref))))
    return out


def _transport_long(c, S_, mu_view, quad):
    """view_np.transport's two sweeps in long double (the same formulas; the linear weights are long double there already)."""
    ld = np.longdouble
    tau, mu = np.asarray(c.tau, dtype=ld), np.asarray(mu_view, dtype=ld)
    L, V = len(tau), len(mu)
    out = np.zeros((L, 2 * V), dtype=ld)
    Sd, Su = S_[:, :V], S_[:, V:]

    def step(dt):
        x = dt / mu
        E = np.exp(-x)
        if quad == VN.QUAD_LINEAR:
            safe = np.where(x > 0, x, 1)
            a = np.where(x > 0, -np.expm1(-safe) / safe, 1)
            return E, 1 - a, a - E
        h = (dt / 2) / mu
        return E, h, h * E

    for t in range(1, L):
        E, wc, wp = step(tau[t] - tau[t - 1])
        out[t, :V] = E * out[t - 1, :V] + (wc * Sd[t] + wp * Sd[t - 1])
    out[L - 1, V:] = c.grd_alb * out[L - 1, :V]
    gaps = set() if quad == VN.QUAD_LINEAR else {z.r1 for z in c.zones[:-1]}
    for t in range(L - 2, -1, -1):
        E, wc, wp = step(tau[t + 1] - tau[t])
        if t in gaps:
            out[t, V:] = E * out[t + 1, V:]
        else:
            out[t, V:] = E * out[t + 1, V:] + (wc * Su[t] + wp * Su[t + 1])
    return out


if __name__ == "__main__":
    for model, gap in float64_gaps():
        print("%-70s %.1e" % (model, gap))
