"""The cases of tests/test_gpu_brdf_builder_shapes.py: the seven BRDF builder entries (csrc/brdf.hip: k_brdf_pairs<NM, KIND>,
k_brdf_view_beam_azimuth) at the shapes the product ships at and at the limits the header promises, for every kind.  Per case
the directions handed to the device and to the NumPy models alike, and the models' results, built once on the CPU, cached and
never changed.

    shape         (N, B)      nphi: modes                         reaches
    floor         (4, 3)      3: 0..1                             9 pairs in one block; flux_weight with M = 3; m_max = 1
                              256: 0..9, 257: 0..9                exactly one chunk of kPhiChunk nodes; a second chunk of one node
                              65537: 0, 1, 63, 64 alone, 57..64   257 chunks, the last of one node; m q up to 4.2e6 in mode_cos
    headline      (128, 3)    65: 0..63 in one call               eight launches of eight modes; the shape README's timings quote
                              131: 0..64                          nine launches: eight of NM = 8 and one of NM = 1
    shipped-N     (501, 3)    257: 0..8                           250 000 pairs, a partial last block; a launch of eight and of one
    cap-N         (1024, 2)   65: 0..8                            1 046 529 pairs: 4089 blocks, the last with ONE live lane
    many-columns  (130, 70)   65: 0..9                            B (N - 1) = 9030 and B V pairs; 361 x 70 x 64 exact azimuths

L = 24 everywhere (no builder reads L); the suns cycle through stage_shape_cases.SUNS; the view cosines are
stage_shape_cases.view_cosines with V = 33 and 64, and for V = 1 (which that function cannot make: it places three cosines) its
cosine 4e-5 above the sun.

The models are those of the suite -- brdf_np._rho with ross_li_np and cox_munk_np imported resolves every kind to rho(a, b, phi)
-- and the quadrature is brdf_azimuth_np.rho_modes': the trapezoid rule on nphi nodes of [0, pi] against cos(m phi) from
brdf_azimuth_np.mode_cos, divided by pi.  `rho_modes` here forms the same sums as ONE product of rho [..., nphi] with the table
w_q cos(m phi_q) / pi [nphi, modes] (65 modes of 16 129 pairs on 131 nodes in 0.1 s instead of 4 s mode by mode);
tests/test_brdf_builder_cases_host.py pins it to brdf_azimuth_np.rho_modes.

The measure.  The suite's builder tests divide the largest error by the largest entry of the whole array.  At N = 1024 with
mu_floor = 0 the Li-Sparse operator peaks at 5e5 on the grazing nodes (mu = 9.8e-4) and is of order 1 inside: 1e-12 'of the
maximum' lets an interior error of 1e-7 pass.  `rowwise` divides, for every exit direction (an upward node, a view cosine; for
the exact-azimuth entry a (column, lane)), the largest error of that direction's stored values by the largest stored value of
that direction in the reference, both over all second directions and all modes of the call, and returns the worst direction.

Does float64 NumPy hold 1e-12 in that measure?  `float64_gaps()` evaluates the same expressions a second time in np.longdouble
(x87 extended, 64-bit mantissa; pi, the nodes and the grid's cosines in long double too -- erfc, which NumPy has not in long
double, from its Taylor series and its continued fraction) and measures float64 against it row-wise, on the rows the device test
samples (every row at N = 4).  tests/test_brdf_builder_cases_host.py asserts every gap <= 1e-13, a tenth of the bound; the
figures are in profiles/brdf_builder_shapes_errors.txt."""
import functools

import numpy as np

import brdf_azimuth_np as BA
import brdf_np as G
import cox_munk_np as CM
import ross_li_np as RL
import sos_oracle as O
import stage_shape_cases as C

RPV = ("rpv", 0.2, 0.8, -0.1)
INDEX = 1.34
KINDS = {"lambertian": "lambertian", "rpv": RPV,
         "ross-thick": ("ross_thick", RL.MU_FLOOR), "ross-thick-floor0": ("ross_thick", 0.0),
         "li-sparse": ("li_sparse_r", RL.MU_FLOOR), "li-sparse-floor0": ("li_sparse_r", 0.0),
         "cox-munk-U2-shadow": ("cox_munk", CM.slope_variance(2), INDEX, 1.0),
         "cox-munk-U10-noshadow": ("cox_munk", CM.slope_variance(10), INDEX, 0.0)}
L = 24
SHAPES = {"floor": (4, 3), "headline": (128, 3), "shipped-N": (501, 3), "cap-N": (1024, 2), "many-columns": (130, 70)}     # (N, B)
# (shape, nphi, [(m_first, m_count) of every call])
PLANS = [("floor", 3, [(0, 2)]), ("floor", 256, [(0, 10)]), ("floor", 257, [(0, 10)]),
         ("floor", 65537, [(0, 1), (1, 1), (63, 1), (64, 1), (57, 8)]),
         ("headline", 65, [(0, 64)]), ("headline", 131, [(0, 65)]),
         ("shipped-N", 257, [(0, 9)]), ("cap-N", 65, [(0, 9)]), ("many-columns", 65, [(0, 10)])]
PLAN_IDS = ["%s-nphi%d" % (name, nphi) for name, nphi, _ in PLANS]
VIEWS = (1, 33, 64)
PHI_AT = np.array([0.0, 1e-9, 0.3, np.pi / 2, 2.0, np.pi - 1e-9, np.pi, 4.0, 2 * np.pi, -0.3])     # tests/test_gpu_cox_munk.py
PHI_MANY = np.linspace(0.0, 2 * np.pi, 361)                  # many-columns: 361 x 70 x 64 = 1 617 280 lanes of the azimuth kernel
KERNEL_BAR = 1e-12                                           # a builder against its model (tests/test_gpu_brdf_azimuth.py), row-wise here
GAP_BAR = 1e-13                                              # float64 against long double: a tenth of it


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def suns(name):
    return frozen(np.array([C.SUNS[b % 4] for b in range(SHAPES[name][1])]))


def view_mu(name, V):
    N = SHAPES[name][0]
    mv = C.view_cosines(max(V, 3), O.make_mu(N), N, C.SUNS[0])
    return mv if V >= 3 else frozen(np.array(mv[2:3]))


def sample_rows(name):
    """The upward nodes i whose rows of the operator are compared with the model: all at N <= 130; at N >= 501 the first three,
    the three around a wave's end, around a block's end, the last three, and six seeded ones"""
    N = SHAPES[name][0]
    M = N - 1
    if N <= 130:
        return np.arange(M)
    fixed = [i for i in (0, 1, 2, 63, 64, 65, 255, 256, 257, M - 3, M - 2, M - 1) if 0 <= i < M]
    extra = np.random.default_rng(N).choice(np.setdiff1d(np.arange(M), fixed), 6, replace=False)
    return np.sort(np.concatenate((fixed, extra))).astype(int)


def modes_of(calls):
    """the modes of a plan's calls, each once, ascending"""
    return sorted({m for m0, mc in calls for m in range(m0, m0 + mc)})


# ---- the measure --------------------------------------------------------------------------------------------------------------------
RESOLVED = 1e-2


def rowwise(got, ref, exit_axes, ref0=None):
    """The worst exit direction's largest error over its largest reference value; `exit_axes`: the axes that index the exit
    direction (the maxima run over all the others).  A direction whose reference is all zero must be all zero.

    ref0: for a call WITHOUT mode 0, the reference's mode 0 in the same layout.  float64 resolves the quadrature's sum to a few
    1e-16 of the integrand, whose size is the direction's mode 0; 1e-12 of a stored value below 1e-3 of that is finer than the
    format.  Such values occur: at cosine exactly 1 (the grid's last node, the last view cosine) the sine is 0, no kind depends
    on phi and every mode m >= 1 is an exact 0; the Lambertian modes m >= 1 are exact zeros; and away from a = b, where RPV and
    the Ross-Li kernels have a cusp in phi, the modes fall off exponentially -- at N = 4 the float64 MODEL's mode 63 of a beam
    row is rounding noise, 1e3 from its long double evaluation in the plain measure.  So a direction's divisor is never taken
    below RESOLVED = 1e-2 of its largest mode-0 value: there the bound is 1e-14 of the direction's mode 0.  (The float64 model
    itself is 3e-16 of mode 0 from long double in the Lambertian mode 1 on 65537 nodes; 1e-2 keeps that a third of GAP_BAR.)"""
    exit_axes = (exit_axes,) if isinstance(exit_axes, int) else tuple(exit_axes)
    other = tuple(a for a in range(np.ndim(ref)) if a not in exit_axes)
    e, d = np.max(np.abs(got - ref), axis=other), np.max(np.abs(ref), axis=other)
    if ref0 is not None:
        d = np.maximum(d, RESOLVED * np.max(np.abs(ref0), axis=other))
    if np.any((d == 0) & (e != 0)):
        return float("inf")
    return float(np.max(np.where(d == 0, 0.0, e / np.where(d == 0, 1.0, d))))


def globalwise(got, ref):
    """the suite's measure: the largest error over the largest entry of the whole array"""
    d = np.max(np.abs(ref))
    return float(np.max(np.abs(got - ref)) / (d if d > 0 else 1.0))


# ---- rho(a, b, phi) in a dtype ------------------------------------------------------------------------------------------------------------
def _pi(dtype):
    return np.pi if dtype is np.float64 else 4 * np.arctan(np.longdouble(1))


def _erfc_ld(x):
    """erfc on a long double array to a few units of 1e-19 ABSOLUTE (what 1 + Lambda needs): below 3 one minus the Taylor
    series of erf, from 3 on the continued fraction exp(-x^2) / sqrt(pi) / (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...))))"""
    ld = np.longdouble
    x = np.asarray(x, dtype=ld)
    pi = _pi(ld)
    small = np.minimum(x, ld(3))
    term, total = small.copy(), small.copy()
    for n in range(1, 120):
        term = -term * small * small / n
        total = total + term / (2 * n + 1)
    low = 1 - 2 / np.sqrt(pi) * total
    big = np.maximum(x, ld(3))
    f = big.copy()
    for k in range(120, 0, -1):
        f = big + (ld(k) / 2) / f
    high = np.exp(-big * big) / np.sqrt(pi) / f
    return np.where(x < 3, low, high)


def rho_ld(brdf):
    """rho(a, b, phi) of the named BRDF on long double arrays: the expressions of brdf_np.rho_rpv, ross_li_np.k_vol / k_geo and
    cox_munk_np.rho_glint, term for term"""
    ld = np.longdouble
    pi = _pi(ld)
    sin_of = lambda c: np.sqrt(np.maximum(ld(0), 1 - c * c))
    if brdf == "lambertian":
        return lambda a, b, phi: np.ones(np.broadcast(a, b, phi).shape, dtype=ld)
    if brdf[0] == "rpv":
        rho0, k, theta = (ld(x) for x in brdf[1:])

        def rpv(a, b, phi):
            sa, sb = sin_of(a), sin_of(b)
            ta, tb = sa / a, sb / b
            cosg = a * b + sa * sb * np.cos(phi)
            F = (1 - theta * theta) / (1 + 2 * theta * cosg + theta * theta) ** ld(1.5)
            Gg = np.sqrt(np.maximum(ld(0), (ta - tb) ** 2 + 4 * (ta * tb) * np.sin(phi / 2) ** 2))
            return rho0 * (a * b * (a + b)) ** (k - 1) * F * (1 + (1 - rho0) / (1 + Gg))
        return rpv
    if brdf[0] in ("ross_thick", "li_sparse_r"):
        floor = ld(brdf[1])

        def ross_li(a, b, phi):
            a, b = np.maximum(a, floor), np.maximum(b, floor)
            sa, sb = sin_of(a), sin_of(b)
            cx = np.clip(a * b + sa * sb * np.cos(phi), ld(-1), ld(1))
            if brdf[0] == "ross_thick":
                xi = np.arccos(cx)
                return ((pi / 2 - xi) * cx + np.sin(xi)) / (a + b) - pi / 4
            ta, tb = sa / a, sb / b
            sec = 1 / a + 1 / b
            hav = 2 * np.sin(phi / 2) ** 2
            D2 = np.maximum(ld(0), (ta - tb) ** 2 + 2 * (ta * tb) * hav)
            ct = np.clip(2 * np.sqrt(D2 + (ta * tb) ** 2 * (hav * (2 - hav))) / sec, ld(-1), ld(1))
            t = np.arccos(ct)
            return (t - np.sin(t) * ct) * sec / pi - sec + (1 + cx) / 2 / (a * b)
        return ross_li
    assert brdf[0] == "cox_munk"
    sigma2, n, shadow = ld(brdf[1]), ld(brdf[2]), bool(brdf[3])

    def smith(mu):
        s = sin_of(mu)
        with np.errstate(divide="ignore", invalid="ignore"):
            cot = mu / s
            lam = (np.sqrt(sigma2 / pi) * np.exp(-cot * cot / sigma2) / cot - _erfc_ld(np.where(s > 0, cot / np.sqrt(sigma2), ld(0)))) / 2
        return np.where(s > 0, lam, ld(0))

    def glint(a, b, phi):
        sa, sb = sin_of(a), sin_of(b)
        h2 = (sa - sb) ** 2 + 2 * sa * sb * (2 * np.cos(phi / 2) ** 2)
        t2 = h2 / (a + b) ** 2
        c = np.sqrt((h2 + (a + b) ** 2) / 4)
        g = np.sqrt(n * n - 1 + c * c)
        rs, rp = (c - g) / (c + g), (n * n * c - g) / (n * n * c + g)
        S = 1 / (1 + smith(a) + smith(b)) if shadow else ld(1)
        return (rs * rs + rp * rp) / 2 * np.exp(-t2 / sigma2) * (1 + t2) ** 2 / (4 * sigma2 * a * b) * S
    return glint


def rho_at(brdf, a, b, phi, dtype=np.float64):
    """rho(a, b, phi) for broadcastable arguments: the suite's model, or its expressions in long double"""
    if dtype is np.float64:
        return G._rho(brdf)(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    a, b, phi = (np.asarray(x, dtype=dtype) for x in (a, b, phi))
    return rho_ld(brdf)(a, b, phi)


def mode_table(ms, nphi, dtype=np.float64):
    """[nphi, len(ms)]: trapezoid weight of node q on [0, pi] times cos(m phi_q) / pi, the cosine of brdf_azimuth_np.mode_cos (the
    angle of the integer m q modulo 2 (nphi - 1), folded onto [0, pi]; exactly 0 at a quarter turn)"""
    half = nphi - 1
    pi = _pi(dtype)
    if dtype is np.float64:
        phi = np.linspace(0, np.pi, nphi)
        cos = np.stack([BA.mode_cos(m, nphi) for m in ms], axis=1)
    else:
        phi = pi * np.arange(nphi, dtype=dtype) / half
        r = (np.array(ms, dtype=np.int64)[None, :] * np.arange(nphi, dtype=np.int64)[:, None]) % (2 * half)
        r = np.where(r > half, 2 * half - r, r)
        cos = np.cos(pi * r.astype(dtype) / half)
        cos[2 * r == half] = 0
    return (G.trapezoid_weights(phi).astype(dtype) if dtype is np.float64 else _trapezoid_weights_ld(phi))[:, None] * cos / pi


def _trapezoid_weights_ld(x):
    w = np.zeros(len(x), dtype=np.longdouble)
    w[:-1] += np.diff(x) / 2
    w[1:] += np.diff(x) / 2
    return w


def nodes(nphi, dtype=np.float64):
    return np.linspace(0, np.pi, nphi) if dtype is np.float64 else _pi(dtype) * np.arange(nphi, dtype=dtype) / (nphi - 1)


def rho_modes(brdf, a, b, ms, nphi, dtype=np.float64):
    """rho^m(a, b) = (1 / pi) int_0^pi rho(a, b, phi) cos(m phi) dphi on the trapezoid nodes for the modes `ms` and broadcastable
    a, b: [len(ms), ...] (brdf_azimuth_np.rho_modes as one product).  The pairs go in slices of at most 2^22 (pair, node) values."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype))
    shape = a.shape
    a, b = a.reshape(-1), b.reshape(-1)
    phi, table = nodes(nphi, dtype), mode_table(ms, nphi, dtype)
    out = np.empty((a.size, len(ms)), dtype=dtype)
    step = max(1, (1 << 22) // nphi)
    for p in range(0, a.size, step):
        out[p:p + step] = rho_at(brdf, a[p:p + step, None], b[p:p + step, None], phi[None, :], dtype) @ table
    return np.moveaxis(out.reshape(shape + (len(ms),)), -1, 0)


# ---- the grid's directions and the flux quadrature ---------------------------------------------------------------------------------------
def grid(N, dtype=np.float64):
    """(up [N-1] = mu[N+1 ..], dn [N-1] = |mu[.. N-2]|, 2 w_j |mu_j| [N-1]) of oracle.make_mu(N).  In long double the SAME float64
    cosines (what the device is handed; k / (N - 1) in long double ends 5e-20 below 1, where sin is 3e-10 and not 0), the weights
    formed from them in long double"""
    mu = O.make_mu(N).astype(dtype)
    up, dn = mu[N + 1:], -mu[:N - 1]
    w = G.trapezoid_weights(mu[:N - 1]) if dtype is np.float64 else _trapezoid_weights_ld(mu[:N - 1])
    return up, dn, 2 * w * dn


# ---- the references of a case, in the layouts of the models ([m, i, j], [m, b, i], [m, v, j], [m, b, v], [q, b, v]) ------------------------------
# The exit directions the long double evaluation is made on (a subset of the rows of the same row-wise measure, to keep the host
# test's minute): the sampled rows' pattern at every N, and of the V = 64 view cosines the limb, the node, the cosine 4e-5 above
# the sun, three mid lanes and the last three -- at 65537 nodes the first three and the last.
def gap_rows(name):
    M = SHAPES[name][0] - 1
    if M <= 18:
        return np.arange(M)
    fixed = [i for i in (0, 1, 2, 63, 64, 65, 255, 256, 257, M - 3, M - 2, M - 1) if 0 <= i < M]
    return np.unique(np.concatenate((fixed, np.random.default_rng(M).choice(M, 6, replace=False)))).astype(int)


def gap_lanes(nphi):
    return (0, 1, 2, 63) if nphi > 1000 else (0, 1, 2, 31, 32, 33, 61, 62, 63)


def plan_modes(name, nphi):
    return modes_of(next(calls for n_, q, calls in PLANS if (n_, q) == (name, nphi)))


def pick(ref, ms_all, m_first, m_count):
    """the modes of one call out of a reference on the plan's modes"""
    return ref[[ms_all.index(m) for m in range(m_first, m_first + m_count)]]


def _views(name, V, lanes):
    mv = view_mu(name, V)
    return mv if lanes is None else mv[list(lanes)]


@functools.lru_cache(maxsize=None)
def operator_ref(name, nphi, kind, dtype=np.float64, rows=None):
    """(rows i [n], R^m[i, j] on those rows [modes, n, N-1]) for the modes of the plan's calls, ascending; rows: sample_rows"""
    up, dn, wj = grid(SHAPES[name][0], dtype)
    rows = sample_rows(name) if rows is None else np.array(rows)
    return rows, frozen(wj[None, None, :] * rho_modes(KINDS[kind], up[rows][:, None], dn[None, :], plan_modes(name, nphi), nphi, dtype))


@functools.lru_cache(maxsize=None)
def operator_columns_ref(name, nphi, kind):
    """R^m[i, j] for every i on the downward nodes j = N - 2 - i' whose cosine is that of the sampled upward nodes i': [modes, N-1, n]
    (the transposed partners of operator_ref's rows in the reciprocity check)"""
    N = SHAPES[name][0]
    up, dn, wj = grid(N)
    cols = N - 2 - sample_rows(name)
    return frozen(wj[cols][None, None, :] * rho_modes(KINDS[kind], up[:, None], dn[cols][None, :], plan_modes(name, nphi), nphi))


@functools.lru_cache(maxsize=None)
def beam_ref(name, nphi, kind, dtype=np.float64, rows=None):
    """r0^m[b, i]: [modes, B, N-1], in full at every N (rows: a subset of the nodes i)"""
    up = grid(SHAPES[name][0], dtype)[0]
    up = up if rows is None else up[list(rows)]
    return frozen(rho_modes(KINDS[kind], up[None, :], suns(name)[:, None], plan_modes(name, nphi), nphi, dtype))


@functools.lru_cache(maxsize=None)
def view_rows_ref(name, nphi, kind, V, dtype=np.float64, lanes=None):
    """Rv^m[v, j]: [modes, V, N-1]"""
    _, dn, wj = grid(SHAPES[name][0], dtype)
    return frozen(wj[None, None, :] * rho_modes(KINDS[kind], _views(name, V, lanes)[:, None], dn[None, :], plan_modes(name, nphi), nphi, dtype))


@functools.lru_cache(maxsize=None)
def view_beam_ref(name, nphi, kind, V, dtype=np.float64, lanes=None):
    """r0v^m[b, v]: [modes, B, V]"""
    return frozen(rho_modes(KINDS[kind], _views(name, V, lanes)[None, :], suns(name)[:, None], plan_modes(name, nphi), nphi, dtype))


@functools.lru_cache(maxsize=None)
def azimuth_ref(name, kind, V, many=False, dtype=np.float64, columns=None):
    """rho(mu_view_v, mu0_b, phi_q) at the azimuths themselves: [q, B, V] (columns: the first so many only)"""
    phi = PHI_MANY if many else PHI_AT
    return frozen(np.array(rho_at(KINDS[kind], view_mu(name, V)[None, None, :], suns(name)[None, :columns, None], phi[:, None, None], dtype)))


# Where float64 alone is more than GAP_BAR from its long double evaluation (float64_gaps; tests/test_brdf_builder_cases_host.py
# asserts that these are the only ones): the Ross-Thick kernel at an azimuth itself, 2.4e-13.  For the column mu0 = 1 the kernel
# does not depend on phi, and at the lane v = 0.3557 its two terms, ((pi/2 - xi) cos xi + sin xi) / (a + b) and pi/4 = 0.7854,
# leave -6.0e-4 at every azimuth: the (column, lane)'s largest value is 8e-4 of its terms, whose rounding, 1.4e-16, is 2.4e-13 of it.
# There the device is compared with the long double evaluation rounded to float64; the bound stays.
LONG_DOUBLE_REFERENCE = {("ross-thick", "exact azimuth"), ("ross-thick-floor0", "exact azimuth")}


@functools.lru_cache(maxsize=None)
def azimuth_reference(name, kind, V, many=False):
    if (kind, "exact azimuth") not in LONG_DOUBLE_REFERENCE:
        return azimuth_ref(name, kind, V, many)
    return frozen(np.asarray(azimuth_ref(name, kind, V, many, np.longdouble), dtype=np.float64))


# ---- the driver at the benchmark's direction count ----------------------------------------------------------------------------------------
# (L, N, B) = (64, 128, 2): the column of brdf_np.experiment_column (Rayleigh with an HG(0.6) slab, tau*_aer = 0.3) at two suns, over
# each ground the drivers name; the model's series in ground reflections on the oracle, 2 to 3 s per column.
DRIVER_L, DRIVER_N = 64, 128
DRIVER_SUNS = (0.6, 0.85)
ROSS_LI_WEIGHTS = np.array([[0.05, 0.30, 0.04], [0.10, 0.02, 0.15]])         # [b, (f_iso, f_vol, f_geo)]: two distinct triples
OCEAN_WEIGHTS = np.array([[0.02, 0.9], [0.05, 0.8]])                         # [b, (f_iso, f_glint)]
DRIVER_GROUNDS = {"rpv": RPV,
                  "ross_li": ("ross_li",) + tuple(list(ROSS_LI_WEIGHTS[:, k]) for k in range(3)),
                  "cox_munk": ("cox_munk", 5.0, INDEX, list(OCEAN_WEIGHTS[:, 0]), list(OCEAN_WEIGHTS[:, 1]))}


@functools.lru_cache(maxsize=None)
def driver_columns():
    return tuple(G.experiment_column(O, DRIVER_N, DRIVER_L, mu0, 0.0, 1.0, "specular") for mu0 in DRIVER_SUNS)


@functools.lru_cache(maxsize=None)
def driver_model(ground):
    """(I [B, L, 2N], bounces [B], ratio [B], status [B]) of the model's series: brdf_np.bounce_solve for RPV;
    ross_li_np.bounce_solve_columns with every column's composed operator for Ross-Li (Lambertian, Ross-Thick, Li-Sparse at the
    default floor) and for the ocean (Lambertian, the glint at U = 5 with shadowing), as tests/test_gpu_ross_li.py and
    tests/test_gpu_cox_munk.py compose them"""
    cols = driver_columns()
    mu, N = cols[0].mu, DRIVER_N
    terms, weights = {"rpv": ((RPV,), np.ones((2, 1))), "ross_li": (RL.terms(), ROSS_LI_WEIGHTS),
                      "cox_munk": (("lambertian", ("cox_munk", CM.slope_variance(5), INDEX, 1.0)), OCEAN_WEIGHTS)}[ground]
    Rs = np.stack([G.operator(mu, N, t) for t in terms])
    r0s = np.stack([np.stack([G.beam_row(mu, N, m0, t) for m0 in DRIVER_SUNS]) for t in terms])
    with np.errstate(all="ignore"):
        if ground == "rpv":
            out = G.bounce_solve(O, cols, Rs[0], r0s[0], (1.0, 1.0))[:4]
        else:
            out = RL.bounce_solve_columns(O, cols, np.tensordot(weights, Rs, axes=1), np.einsum("bk,kbi->bi", weights, r0s))
    out[0].setflags(write=False)
    return out


# ---- float64 against long double ---------------------------------------------------------------------------------------------------------
def float64_gaps(kinds=None, plans=None):
    """[(kind, shape, nphi, what, call, gap)]: the float64 references against their long double evaluation, row-wise, per call of
    the plan (a call's maxima run over the call's modes, `rowwise` with the mode 0 of a call that has none): the
    operator on gap_rows, the beam rows on them, the view rows and view beam rows on gap_lanes of V = 64, and per (kind, shape)
    the exact-azimuth values on all 64 lanes for the first four columns (the suns have a period of four; many-columns: at the
    361 azimuths too)"""
    ld = np.longdouble
    out = []
    for kind in kinds or KINDS:
        seen = set()
        for name, nphi, calls in plans or PLANS:
            N = SHAPES[name][0]
            ms = plan_modes(name, nphi)
            rows, lanes = tuple(int(i) for i in gap_rows(name)), gap_lanes(nphi)
            pairs = {"operator": (operator_ref(name, nphi, kind, np.float64, rows)[1], operator_ref(name, nphi, kind, ld, rows)[1], 1),
                     "beam rows": (beam_ref(name, nphi, kind, np.float64, rows), beam_ref(name, nphi, kind, ld, rows), 2),
                     "view rows V=64": (view_rows_ref(name, nphi, kind, 64, np.float64, lanes), view_rows_ref(name, nphi, kind, 64, ld, lanes), 1),
                     "view beam rows V=64": (view_beam_ref(name, nphi, kind, 64, np.float64, lanes), view_beam_ref(name, nphi, kind, 64, ld, lanes), 2)}
            for what, (a, l, axis) in pairs.items():
                for m0, mc in calls:
                    out.append((kind, name, nphi, what, (m0, mc), rowwise(pick(a, ms, m0, mc), pick(l, ms, m0, mc), axis, None if m0 == 0 else l[:1])))
            if name not in seen:
                seen.add(name)
                for many in (False, True) if name == "many-columns" else (False,):
                    out.append((kind, name, len(PHI_MANY if many else PHI_AT), "exact azimuth", (0, 0),
                                rowwise(azimuth_ref(name, kind, 64, many, np.float64, 4), azimuth_ref(name, kind, 64, many, ld, 4), (1, 2))))
    return out


def show(g):
    kind, name, nphi, what, call, gap = g
    at = "modes %2d..%-2d" % (call[0], call[0] + call[1] - 1) if call[1] else "%d azimuths" % nphi
    return "%-22s %-13s %-13s %-20s %s  float64 vs longdouble %.1e%s" % (kind, name, "nphi=%d" % nphi if call[1] else "", what, at, gap,
                                                                         "   <- above a tenth" if gap > GAP_BAR else "")


if __name__ == "__main__":
    import time
    t0 = time.time()
    for g in float64_gaps():
        print(show(g))
    print("%.1f s" % (time.time() - t0))
