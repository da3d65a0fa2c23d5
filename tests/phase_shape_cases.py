"""The cases of tests/test_gpu_phase_shapes.py: the phase builders of csrc/phase.hip (the matrix, P0, their Fourier modes, the
rows of all four at view cosines, the first-order point values) and the azimuth synthesis of csrc/epilogue.hip at the shapes the
product ships at and at the limits the header promises.  Per shape: the inputs handed to the device and to the NumPy models alike
and the models' tables, built once on the CPU, cached and never changed.

    name          (N, B)      reaches
    floor         (4, 3)      D = 8: 8 live lanes of 256
    headline      (128, 2)    D = 256: exactly one trip of the stride loops
    many-columns  (130, 70)   D = 260: four threads take a second element; 70 columns of P0
    shipped-N     (501, 3)    odd N; four trips, the last one partial
    cap-N         (1024, 2)   eight full trips; the normaliser's sum over 2048 exits

The models are those the suite has: every table is `azimuth_np.ring_modes` (the rings of all pairs of an exit and a second
direction) divided by the trapezoid sum over the grid's exits of its m = 0 ring, exactly as azimuth_np.phase_modes /
phase_p0_modes and view_azimuth_np.mode_rows / mode_p0_rows write it (tests/test_phase_shape_cases_host.py pins `tables` to
them bit for bit, and its mode 0 on 25 nodes to inputs.phase_function and view_np).  `tables` only adds what the shapes need:
a subset of second directions, and chunks of them, so that the ring array of N = 1024 never exists at once.

At D <= 260 the model covers every element.  At shipped-N and cap-N it covers all exits of `columns(name)`: 32 second directions
(the first, the last, both horizon nodes, the nodes next to them, seeded random ones); the rest of the table is covered by two
identities over the whole table, the sum rule (the trapezoid sum over the exits of mode 0 is 4 per column of the matrix, 2 per
row of P0) and reciprocity (P^m[a][b] Z_b = P^m[b][a] Z_a, Z the model's m = 0 normaliser on the same nphi from one threaded
ring pass over all columns, `normalisers`), each with ten times the residual the model itself leaves as its tolerance
(`identity_tolerances`).

Phase functions: Rayleigh, HG g = 0.9 (its mode 64 is a visible share of mode 0: `high_mode_share`), the fwc table, and the
isotropic one at floor.  mu0: 1.0 (s = 0: the odd modes of P0 vanish) and 0.05 in every batch.  View lanes: V2 = 1 and 128 (the
four edge cosines, both mu = 0 nodes and other grid nodes in front -- `node_lanes` -- then random cosines).

Build times on the CPU (8 threads), per shape and phase function, every mode set of the shape: the models of all nine entries,
then the normalisers of every column for the identities (one ring pass per nphi in use: 25, 31 and 131 at shipped-N, 25 and 131
at cap-N):

    floor 0.2 .. 0.3 s    headline 1.5 .. 2.6 s    many-columns 1.9 .. 3.4 s    shipped-N 0.5 .. 0.9 s + 1.1 .. 5.3 s
    cap-N 0.5 .. 1.4 s + 3.0 s (Rayleigh), 4.1 s (HG), 16.2 s (the table: 2048^2 x 156 x 2 binary searches in NumPy)

The table's normalisers at cap-N are over the ten seconds a shape should take; the subset of second directions has no part in
them (they are every column's, which is what the whole-table identity needs), and N is not cut.

Does float64 NumPy hold the bound of 1e-12 of the mode-0 maximum?  `float64_gaps()` evaluates every model a second time in
np.longdouble (x87 extended) at cap-N with the modes 1..64 on 131 nodes, and mode 0 on 25, and measures float64 against it in the
measure of the GPU test.  Measured (PYTHONPATH=oracle:tests:sos-radiative-transfer_amd python tests/phase_shape_cases.py; also in
profiles/phase_shapes_errors.txt):

    model                                  function   float64 vs longdouble   bound of the test
    matrix modes 1..64                     rayleigh   8.1e-16                 1e-12
    P0 modes 1..64                         rayleigh   8.1e-16                 1e-12
    rows V2=128 modes 1..64                rayleigh   8.1e-16                 1e-12
    P0 rows V2=128 modes 1..64             rayleigh   8.1e-16                 1e-12
    matrix mode 0                          rayleigh   1.6e-15                 1e-12
    P0 mode 0                              rayleigh   1.8e-15                 1e-12
    rows V2=128 mode 0                     rayleigh   1.5e-15                 1e-12
    P0 rows V2=128 mode 0                  rayleigh   1.3e-15                 1e-12
    P0 point values, 48 azimuths           rayleigh   1.9e-15                 1e-12
    matrix modes 1..64                     hg         1.2e-15                 1e-12
    P0 modes 1..64                         hg         2.1e-14                 1e-12
    rows V2=128 modes 1..64                hg         8.3e-16                 1e-12
    P0 rows V2=128 modes 1..64             hg         7.8e-16                 1e-12
    matrix mode 0                          hg         6.0e-15                 1e-12
    P0 mode 0                              hg         2.6e-14                 1e-12
    rows V2=128 mode 0                     hg         4.2e-15                 1e-12
    P0 rows V2=128 mode 0                  hg         4.2e-15                 1e-12
    P0 point values, 48 azimuths           hg         3.4e-14                 1e-12
    matrix modes 1..64                     table      1.7e-15                 1e-12
    P0 modes 1..64                         table      6.5e-14                 1e-12
    rows V2=128 modes 1..64                table      1.2e-15                 1e-12
    P0 rows V2=128 modes 1..64             table      1.1e-15                 1e-12
    matrix mode 0                          table      1.7e-15                 1e-12
    P0 mode 0                              table      6.3e-14                 1e-12
    rows V2=128 mode 0                     table      1.3e-15                 1e-12
    P0 rows V2=128 mode 0                  table      9.2e-16                 1e-12
    P0 point values, 48 azimuths           table      2.1e-13                 1e-12

Every gap but one is below a tenth of the bound: there the float64 models are the reference.  The point values of the table are
the exception: next to a node of the table the rounding of the scattering cosine moves the interpolant, and float64 is 2.1e-13
from long double.  For them the tests compare the device with the long double evaluation rounded to float64
(`p0_azimuth_reference`); the bound stays 1e-12.  The synthesis is compared with a long double
sum (`synthesis_reference`): its bar, (M + 4) 2^-53 of the sum of the terms' magnitudes, is a rounding bound that a float64
reference would spend itself."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import azimuth_np as A
import view_azimuth_np as VA
import view_np as VN
from phase_builder_cases import PHI
from sosrt import inputs

_trapz = A._trapz

# (N, B)
SHAPES = {"floor": (4, 3), "headline": (128, 2), "many-columns": (130, 70), "shipped-N": (501, 3), "cap-N": (1024, 2)}
LARGE = ("shipped-N", "cap-N")
KINDS = [("rayleigh", 0.0), ("hg", 0.9), ("table", 0.0)]
LOW, FULL = (1, 3, 25), (1, 64, 131)                       # (m_first, m_count, nphi): K = 9 and K = kMaxModes + 1 = 65
MATRIX_SETS = {"floor": [LOW, FULL], "headline": [LOW, FULL], "many-columns": [LOW, FULL],
               "shipped-N": [LOW, (1, 8, 31), (57, 8, 131)], "cap-N": [LOW, (63, 2, 131)]}
SMALL_SETS = [LOW, FULL]                                   # the tables of lanes and of P0, at every shape
NODE_K_SETS = [(1, 3, 25), (3, 14, 41), (2, 30, 71), FULL]  # 4, 15, 31 and 65 accumulators: K = 9, 17, 33, 65
V2S = (1, 128)
PHI48 = 2 * np.pi * np.arange(48) / 48                     # nphi_out * V2 = 6144: 24 trips of k_phase_p0_azimuth's stride loop
BOUND = 1e-12                                              # of the mode-0 maximum: the two small-shape tests' measure and bound
NSUB = 32
CHUNK = 3_000_000                                          # elements of a ring array in flight


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def fn_of(kind, g=0.0):
    return VN.phase_fn(kind, g, table=inputs.fwc_table() if kind == "table" else None)


@functools.lru_cache(maxsize=None)
def grid(name):
    return frozen(inputs.direction_grid(SHAPES[name][0]))


@functools.lru_cache(maxsize=None)
def suns(name):
    """mu0 [B]: 1.0 and 0.05 first; 70 columns are spread over (0.05, 1]"""
    B = SHAPES[name][1]
    return frozen(np.array([1.0, 0.05, 0.6][:B]) if B <= 3 else np.concatenate(([1.0], np.linspace(0.05, 1.0, B)[:-1])))


@functools.lru_cache(maxsize=None)
def node_lanes(name):
    """grid indices of the node lanes in front of lanes(name, 128): both ends, both mu = 0 nodes, the nodes next to them, others"""
    N = SHAPES[name][0]
    return frozen(np.unique(np.clip([0, 1, N - 2, N - 1, N, N + 1, 2 * N - 2, 2 * N - 1, N // 2, N + N // 3 + 1], 0, 2 * N - 1)))


@functools.lru_cache(maxsize=None)
def lanes(name, V2):
    """V2 signed exit cosines: one lane is -0.01; 128 are the nodes of node_lanes, +-0.01, then seeded random cosines"""
    if V2 == 1:
        return frozen(np.array([-0.01]))
    mu, k = grid(name), node_lanes(name)
    rng = np.random.default_rng(7)
    return frozen(np.concatenate((mu[k], [0.01, -0.01], rng.uniform(-1, 1, V2 - len(k) - 2))))


@functools.lru_cache(maxsize=None)
def columns(name):
    """indices of the second directions the model of a matrix covers: all of them at D <= 260, else NSUB"""
    N = SHAPES[name][0]
    if name not in LARGE:
        return frozen(np.arange(2 * N))
    fixed = [0, 2 * N - 1, N - 1, N, N - 2, N + 1]
    rest = np.setdiff1d(np.arange(2 * N), fixed)
    return frozen(np.sort(np.concatenate((fixed, np.random.default_rng(11).choice(rest, NSUB - len(fixed), replace=False)))))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _pool():
    return ThreadPoolExecutor(min(8, os.cpu_count() or 1))


def _ring(fn, ex, sec, ms, nphi, dtype):
    """azimuth_np.ring_modes in chunks of second directions, the chunks on threads: [len(ms), len(ex), len(sec)]"""
    step = max(1, min(CHUNK // (len(ex) * nphi), -(-len(sec) // 8)))
    with _pool() as pool:
        return np.concatenate(list(pool.map(lambda i: A.ring_modes(fn, ex, sec[i:i + step], ms, nphi, dtype), range(0, len(sec), step))), axis=2)


def tables(fn, mu, ex, sec, ms, nphi, second, dtype=np.float64):
    """(tables [len(ms), len(ex), len(sec)], Z [len(sec)]): the rings of the exits `ex` (None: the grid's) and the second
    directions `sec` -- grid nodes ('column': R / (2 pi) * 4 / Z) or suns ('mu0': R / (4 pi) / Z * 2) -- normalised by Z =
    trapz over the grid's exits of the m = 0 ring on the same nphi.  ms = [0]: mode 0 itself."""
    k = dtype(2 * np.pi if second == "column" else 4 * np.pi)
    ms = list(ms)
    sec = np.asarray(sec, dtype=np.float64)
    if ex is None:
        R = _ring(fn, mu, sec, [0] + ms, nphi, dtype) / k
        R0, R = R[0], R[1:]
    else:
        R0 = _ring(fn, mu, sec, [0], nphi, dtype)[0] / k
        R = _ring(fn, np.asarray(ex, dtype=np.float64), sec, ms, nphi, dtype) / k
    Z = _trapz(R0, mu.astype(dtype), axis=0)[None, :]
    return np.stack([4 * r / Z if second == "column" else r / Z * 2 for r in R]), Z[0]


def _ms(mset):
    return [0] if mset is None else list(range(mset[0], mset[0] + mset[1]))


def _nphi(mset):
    return 25 if mset is None else mset[2]


@functools.lru_cache(maxsize=None)
def matrix_model(name, kind, g, mset, dtype=np.float64):
    """[m, D exits, columns(name)]; mset None: mode 0 on the 25-node ring, [1, D, columns]"""
    mu = grid(name)
    return frozen(tables(fn_of(kind, g), mu, None, mu[columns(name)], _ms(mset), _nphi(mset), "column", dtype)[0])


@functools.lru_cache(maxsize=None)
def p0_model(name, kind, g, mset, dtype=np.float64):
    """[m, B, D]"""
    return frozen(np.ascontiguousarray(np.swapaxes(tables(fn_of(kind, g), grid(name), None, suns(name), _ms(mset), _nphi(mset), "mu0", dtype)[0], 1, 2)))


@functools.lru_cache(maxsize=None)
def rows_model(name, kind, g, mset, V2, dtype=np.float64):
    """[m, V2, columns(name)]"""
    mu = grid(name)
    return frozen(tables(fn_of(kind, g), mu, lanes(name, V2), mu[columns(name)], _ms(mset), _nphi(mset), "column", dtype)[0])


@functools.lru_cache(maxsize=None)
def p0_rows_model(name, kind, g, mset, V2, dtype=np.float64):
    """[m, B, V2]"""
    return frozen(np.ascontiguousarray(np.swapaxes(tables(fn_of(kind, g), grid(name), lanes(name, V2), suns(name), _ms(mset), _nphi(mset), "mu0", dtype)[0], 1, 2)))


@functools.lru_cache(maxsize=None)
def p0_azimuth_model(name, kind, g, V2, nphi_out, dtype=np.float64):
    """[nphi_out, B, V2]: p(c(s_j, mu0_b, phi_i)) / Z0_b (view_azimuth_np.p0_exact; in another dtype the same expression)"""
    phi = PHI if nphi_out == len(PHI) else PHI48
    if dtype is np.float64:
        return frozen(VA.p0_exact(fn_of(kind, g), grid(name), suns(name), lanes(name, V2), phi))
    s, mu0, ph = (np.asarray(x).astype(dtype) for x in (lanes(name, V2), suns(name), phi))
    Z = tables(fn_of(kind, g), grid(name), None, suns(name), [0], 25, "mu0", dtype)[1]
    c = -(s[None, None, :] * mu0[None, :, None] + np.sqrt(1 - s * s)[None, None, :] * np.sqrt(1 - mu0 * mu0)[None, :, None] * np.cos(ph)[:, None, None])
    return frozen(fn_of(kind, g)(c) / Z[None, :, None])


POINT_VALUES_IN_LONG_DOUBLE = ("table",)                  # float64_gaps: the table's point values are 2e-13 from long double


@functools.lru_cache(maxsize=None)
def p0_azimuth_reference(name, kind, g, V2, nphi_out):
    """What the device's point values are compared with: the float64 model; for the table its long double evaluation rounded to
    float64 (next to a node of the table the rounding of the scattering cosine moves the interpolant by more than a tenth of
    the bound)"""
    if kind not in POINT_VALUES_IN_LONG_DOUBLE:
        return p0_azimuth_model(name, kind, g, V2, nphi_out)
    return frozen(np.asarray(p0_azimuth_model(name, kind, g, V2, nphi_out, np.longdouble), dtype=np.float64))


def scales(name, kind, g):
    """The mode-0 maxima the differences are measured in: (matrix, P0 per column [B], rows {V2}, P0 rows {V2})"""
    return (float(np.max(np.abs(matrix_model(name, kind, g, None)))), np.max(np.abs(p0_model(name, kind, g, None)[0]), axis=1),
            {V2: float(np.max(np.abs(rows_model(name, kind, g, None, V2)))) for V2 in V2S},
            {V2: float(np.max(np.abs(p0_rows_model(name, kind, g, None, V2)))) for V2 in V2S})


def high_mode_share(name, kind, g):
    """max |P^64| / max |P^0| of the model's matrix columns, mode 64 on 131 nodes"""
    return float(np.max(np.abs(matrix_model(name, kind, g, (64, 1, 131)))) / scales(name, kind, g)[0])


# ---- the whole-table identities ---------------------------------------------------------------------------------------------------------
def trapz_weights(mu):
    w = np.zeros(len(mu))
    w[:-1] += np.diff(mu) / 2
    w[1:] += np.diff(mu) / 2
    return w


@functools.lru_cache(maxsize=None)
def normalisers(name, kind, g, nphi):
    """(Z, Zd) [D] of every column from one ring pass, chunks on threads: the m = 0 ring / (2 pi) on nphi nodes summed over the
    exits by np.trapz, as the model sums it (row after row), and as the grid's trapezoid weights times the ring, summed pairwise"""
    mu, fn = grid(name), fn_of(kind, g)
    D, w = len(mu), trapz_weights(mu)
    step = max(1, CHUNK // (D * nphi))

    def both(i):
        R0 = A.ring_modes(fn, mu, mu[i:i + step], [0], nphi)[0] / (2 * np.pi)
        return _trapz(R0, mu, axis=0), (R0.T * w[None, :]).sum(axis=1)
    with _pool() as pool:
        parts = list(pool.map(both, range(0, D, step)))
    return frozen(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


def reciprocity(Pab, Pba, Z_rows, Z_cols, scale, zmax):
    """max |P[m][a][b] Z_b - P[m][b][a] Z_a| / (scale zmax): Pab [m, rows, cols] holds P[m][a][b], Pba [m, cols, rows] P[m][b][a]
    (a whole table is both)"""
    r = 0.0
    for m in range(Pab.shape[0]):
        r = max(r, float(np.max(np.abs(Pab[m] * Z_cols[None, :] - Pba[m].T * Z_rows[:, None]))))
    return r / (scale * zmax)


def _ring0_reassociated(fn, mu, sec, nphi):
    """azimuth_np.ring_modes' m = 0 ring with s_a (s_b cos phi) in place of (s_a s_b) cos phi: the same scattering cosines to an
    ulp, as a fused multiply-add or any other order of the products gives them: [len(mu), len(sec)]"""
    phi = np.linspace(0, np.pi, nphi)
    cc = (mu[:, None] * sec[None, :])[..., None]
    x = np.sqrt(1 - mu * mu)[:, None, None] * (np.sqrt(1 - sec * sec)[None, :, None] * np.cos(0 - phi))
    return _trapz(fn(-(cc + x)) + fn(-(cc - x)), phi, axis=-1)


@functools.lru_cache(maxsize=None)
def identity_tolerances(name, kind, g, mset):
    """(sum rule, reciprocity): ten times the residual the model leaves.  The sum rule: |trapz_exits P^0 - 4| / 4 on the model's
    columns of mode 0, |trapz_exits P0 - 2| / 2 on its rows of P0.  Reciprocity, in `reciprocity`'s measure: with the normalisers
    the model divided by, the residual is two roundings of a product and says nothing about a second correct float64
    evaluation; the identity is between a table and normalisers that were formed on their own.  The model's ring is symmetric
    bit for bit (the host test asserts it), so on the pair (a, b) the residual of its table against other normalisers Z' is
    |P[a][b] Z_b| |d_b - d_a| with d = Z' / Z - 1, over the whole table at most the largest |P^m[a][b] Z_b| of the model's columns
    times the spread of d.  Two things move a correct float64 normaliser, and the spread taken is the sum of both: the order of
    the sum over 2N exits (np.trapz's row after row against a pairwise sum of weights times ring: `normalisers` has both for
    ALL columns), and the last bit of the scattering cosines, to which a steep p answers (the ring with its products in
    another order, `_ring0_reassociated`, on the model's columns)."""
    mu, c, fn = grid(name), columns(name), fn_of(kind, g)
    Z, Zd = normalisers(name, kind, g, _nphi(mset))
    d = Zd / Z - 1
    dc = _trapz(_ring0_reassociated(fn, mu, mu[c], _nphi(mset)) / (2 * np.pi), mu, axis=0) / Z[c] - 1
    spread = float(d.max() - d.min()) + float(dc.max() - dc.min())
    top = float(np.max(np.abs(matrix_model(name, kind, g, mset)) * Z[c][None, None, :]))
    rec = top * spread / (scales(name, kind, g)[0] * float(np.max(Z)))
    rule = float(np.max(np.abs(_trapz(matrix_model(name, kind, g, None)[0], mu, axis=0) - 4))) / 4
    rule0 = float(np.max(np.abs(_trapz(p0_model(name, kind, g, None)[0], mu, axis=1) - 2))) / 2
    return 10 * max(rule, rule0), 10 * rec


# ---- the synthesis ----------------------------------------------------------------------------------------------------------------------
def synthesis_fields(shape, M, seed):
    """[M + 1, *shape]: seeded normal fields whose modes decay like 0.9^m"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((M + 1,) + tuple(shape)) * (0.9 ** np.arange(M + 1)).reshape((-1,) + (1,) * len(shape))


def synthesis_reference(vals, phi):
    """(sum_m (2 - delta_m0) val^m cos(m phi) in long double, ascending m, [..., len(phi)]; sum_m |term_m|): the product m phi is
    formed in float64, as the device forms it, its cosine taken in long double"""
    ld = np.longdouble
    phi = np.asarray(phi, dtype=np.float64)
    out = np.repeat(vals[0][..., None].astype(ld), len(phi), axis=-1)
    mag = np.abs(out)
    for m in range(1, len(vals)):
        term = 2 * vals[m][..., None].astype(ld) * np.cos((m * phi).astype(ld))
        out, mag = out + term, mag + np.abs(term)
    return out, mag


def synthesis_bar(M):
    """An ascending float64 sum of M + 1 terms, each one rounded product with a cosine good to 2 ulp: (M + 4) 2^-53 of sum |term|"""
    return (M + 4) * 2.0 ** -53


# ---- float64 against long double ----------------------------------------------------------------------------------------------------------
def float64_gaps():
    """[(model, function, gap)] at cap-N: the float64 models against their evaluation in np.longdouble, max |difference| over the
    mode-0 maximum; the modes are 1..64 on 131 nodes (the matrix on 8 of its columns, which costs the long double pass 1/4)"""
    ld, name = np.longdouble, "cap-N"
    mu = grid(name)
    out = []
    for kind, g in KINDS:
        fn = fn_of(kind, g)
        sm, sp0, sr, spr = scales(name, kind, g)
        cols = mu[columns(name)[::4]]
        gap = lambda a, b, s: float(np.max(np.abs(a - b)) / s)
        for label, mset in (("modes 1..64", FULL), ("mode 0", None)):
            ms, nphi = _ms(mset), _nphi(mset)
            a, b = (tables(fn, mu, None, cols, ms, nphi, "column", t)[0] for t in (np.float64, ld))
            out.append(("matrix " + label, kind, gap(a, b, sm)))
            a, b = (tables(fn, mu, None, suns(name), ms, nphi, "mu0", t)[0] for t in (np.float64, ld))
            out.append(("P0 " + label, kind, max(gap(a[:, :, i], b[:, :, i], sp0[i]) for i in range(len(sp0)))))
            a, b = (tables(fn, mu, lanes(name, 128), cols, ms, nphi, "column", t)[0] for t in (np.float64, ld))
            out.append(("rows V2=128 " + label, kind, gap(a, b, sr[128])))
            a, b = (tables(fn, mu, lanes(name, 128), suns(name), ms, nphi, "mu0", t)[0] for t in (np.float64, ld))
            out.append(("P0 rows V2=128 " + label, kind, gap(a, b, spr[128])))
        a, b = p0_azimuth_model(name, kind, g, 128, 48), p0_azimuth_model(name, kind, g, 128, 48, ld)
        out.append(("P0 point values, 48 azimuths", kind, float(np.max(np.abs(a - b) / np.abs(b)))))
    return out


if __name__ == "__main__":
    import time
    for model, kind, gap in float64_gaps():
        print("    %-38s %-10s %.1e                 %.0e" % (model, kind, gap, BOUND))
    for name in SHAPES:
        for kind, g in KINDS:
            t0 = time.time()
            for mset in [None] + MATRIX_SETS[name]:
                matrix_model(name, kind, g, mset)
            for mset in [None] + SMALL_SETS:
                p0_model(name, kind, g, mset)
                for V2 in V2S:
                    rows_model(name, kind, g, mset, V2), p0_rows_model(name, kind, g, mset, V2)
            t1 = time.time()
            if name in LARGE:
                for mset in [None] + MATRIX_SETS[name]:
                    print("   ", name, kind, mset, "tolerances (sum rule, reciprocity): %.2e %.2e" % identity_tolerances(name, kind, g, mset))
            print("%-14s %-9s models %.1f s, normalisers and identities %.1f s; mode 64 is %.1e of mode 0" %
                  (name, kind, t1 - t0, time.time() - t1, high_mode_share(name, kind, g)))
