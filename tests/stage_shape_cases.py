"""The cases of tests/test_gpu_stage_shapes.py: the stage kernels beside the solve (the pseudo-spherical beam, thermal emission,
view radiance, the BRDF ground and its view term) at the shapes the product ships at and at the limits the header promises.
Per shape: the columns, the inputs handed to the device and to the NumPy model alike, and the model's results, built once on
the CPU, cached and never changed.

The kernels take P0 vectors, phase rows, operators and fields as arguments, so no phase MATRIX is built here (it costs seconds
at N = 501 and more at N = 1024, and no stage kernel reads it): columns are `oracle.make_column` with zero matrices, P0 vectors
and rows are `view_np.phase_p0_rows` of Rayleigh and HG(0.7), phase rows, operators, beam rows and fields are seeded positive
random arrays.

    name          (N, L, B)       reaches
    floor         (4, 24, 3)      N - 3 = 1 in the ground search; M = 3; D = 8 padded to 16; a 64-thread block with 4 live lanes
    headline      (128, 200, 2)   the benchmark's shape: two full blocks per column; 4 level blocks; L near the 256 stride
    shipped-N     (501, 24, 3)    odd N; 8 waves with a partial last one; the ground search in 8 trips; Dp = 1008
    cap-N         (1024, 24, 2)   1024-thread workgroups; the cross-wave sum of 16 waves; 16 blocks per column with B > 1
    cap-L         (32, 2048, 2)   64 KiB of dynamic LDS; 32 level blocks with B > 1; L >> 256 in the epilogues
    cap-L-2slabs  (32, 2048, 2)   cap-L on a two-slab zone table: zone boundaries beyond row 256 (beam and emission only)
    many-columns  (130, 24, 70)   3 blocks per column with B = 70: b = blockIdx.x / nblk with a remainder; 2 live lanes
    profile-cap-L (32, 1024, 2)   the profile stage's cap (kProfileMaxL): 48 KiB of dynamic LDS in k_first_order_profile
    profile-cap-L-2slabs          profile-cap-L on the two-slab zone table: zone boundaries deep in a long column, a P0 per zone

The profile stage (k_first_order_profile, k_emission_profile; `PROFILE`) runs at floor, shipped-N, cap-N,
many-columns and the two profile-cap-L shapes on the beam's and the thermal columns, with weights of profile_np.random_weights
per column.

Does float64 NumPy hold the tests' bounds at this depth?  At cap-L a recurrence runs over 2047 rows, at cap-N a dot product
over 1023 or 2048 terms.  `float64_gaps()` evaluates the models a second time in np.longdouble (x87 extended, 64-bit mantissa) --
the same functions with `dtype=np.longdouble` passed through, or the same expression on longdouble arrays -- and measures
float64 against it in the measure of the test that uses the model.  Measured (PYTHONPATH=oracle:tests python
tests/stage_shape_cases.py; also in profiles/stage_shapes_errors.txt):

    model                                         shape         float64 vs longdouble   bound of the test
    spherical_np.slant_path                       cap-L         3.8e-14                 1e-12
    spherical_np.first_order_beam                 cap-L         1.9e-14                 1e-12
    spherical_np.first_order_beam                 cap-L-2slabs  1.6e-14                 1e-12
    spherical_view_np.view_first_order_beam V=64  cap-L         1.3e-14                 1e-12
    thermal_np.emission specular                  cap-L         2.1e-13                 1e-12   <- above a tenth
    thermal_np.emission lambertian                cap-L         1.9e-13                 1e-12   <- above a tenth
    thermal_np.emission specular                  cap-L-2slabs  1.4e-13                 1e-12   <- above a tenth
    thermal_np.emission_view V=64                 cap-L         2.1e-13                 1e-12   <- above a tenth
    thermal_np.emission lambertian                cap-N         2.6e-15                 1e-12
    spherical_np.epilogue_beam (worst output)     cap-L         3.7e-13                 1e-10
    spherical_np.epilogue_beam (worst output)     cap-L-2slabs  7.2e-13                 1e-10
    thermal_np.epilogue_emission (worst output)   cap-L         1.4e-13                 1e-10
    thermal_np.epilogue_emission (worst output)   cap-L-2slabs  3.3e-13                 1e-10
    brdf_np.ground_source                         cap-N         6.5e-16                 1e-13
    ross_li_np.ground_source_terms                cap-N         6.8e-16                 1e-13
    brdf_np.ground_source at view lanes V=64      cap-N         7.8e-16                 1e-13
    view_np.source V=64                           cap-N         3.1e-16                 1e-10

    profile_np.first_order_profile (worst path)   profile-cap-L          3.2e-15         1e-12
    profile_np.first_order_profile (worst path)   profile-cap-L-2slabs   3.4e-15         1e-12
    profile_np.first_order_profile, P0 per zone   profile-cap-L-2slabs   5.3e-15         1e-12
    profile_np.emission_profile (worst surface)   profile-cap-L          6.6e-14         1e-12
    profile_np.emission_profile (worst surface)   profile-cap-L-2slabs   5.0e-14         1e-12
    (`profile_float64_gaps()`; every figure in profiles/brdf_builder_shapes_errors.txt)

Every gap but the emitted field's at cap-L is below a tenth of its bound: there the tests compare the device with the float64
models.  The emitted field at L = 2048 is the exception.  Its layers are equally thick, so a lane multiplies by the same
E = exp(-x) 2047 times, and the rounding of that one number (half an ulp of a value next to 1) adds up linearly instead of
averaging out: 2047 * 1.1e-16 = 2.3e-13.  For the emitted field and its view lanes at cap-L and cap-L-2slabs the tests therefore
compare the device with the long double evaluation (`thermal_reference`, `thermal_view_reference`), rounded to float64; the
bound stays 1e-12.  At the profile stage's cap of 1024 layers the weighted emitted field's gap is half of that and under a tenth of
the bound (`profile_float64_gaps()`; profile_np's two stage models take the dtype for it): the float64 model is the reference."""
import functools

import numpy as np

import brdf_np as G
import profile_np as P
import ross_li_np as RL
import sos_oracle as O
import spherical_np as S
import spherical_view_np as SV
import thermal_np as T
import view_np as VN

# (N, L, B)
SHAPES = {"floor": (4, 24, 3), "headline": (128, 200, 2), "shipped-N": (501, 24, 3), "cap-N": (1024, 24, 2), "cap-L": (32, 2048, 2),
          "cap-L-2slabs": (32, 2048, 2), "many-columns": (130, 24, 70), "profile-cap-L": (32, 1024, 2), "profile-cap-L-2slabs": (32, 1024, 2)}
SIX = ["floor", "headline", "shipped-N", "cap-N", "cap-L", "many-columns"]
WITH_SLABS = SIX + ["cap-L-2slabs"]                          # the stages that read a zone table: the beam, emission
VIEW_SHAPES = ["floor", "headline", "shipped-N", "cap-N"]
CAP_L = ("cap-L", "cap-L-2slabs")
# the profile stage (k_first_order_profile, k_emission_profile): kProfileMaxL = 1024 layers in place of 2048
PROFILE = ["floor", "shipped-N", "cap-N", "many-columns", "profile-cap-L", "profile-cap-L-2slabs"]
PROFILE_CAP_L = ("profile-cap-L", "profile-cap-L-2slabs")
FN_ATM, FN_AER = VN.phase_fn("rayleigh"), VN.phase_fn("hg", 0.7)
SUNS = (0.05, 1.0, 0.21, 0.6)                                # MU0S of tests/test_gpu_spherical.py; every shape has 0.05 and 1.0
RHOS = (0.3, 0.0, 0.5, 0.1, 0.2)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def no_matrix(N):
    """(P0 [2N], P [2N, 2N]) of zeros: what a column carries where no stage reads it"""
    return frozen(np.zeros(2 * N), np.zeros((2 * N, 2 * N)))


def levels_300(L):
    """300 levels, more than one launch takes (256), every row more than once where L < 300, out of order"""
    return [(7 * i) % L for i in range(300)]


def view_cosines(V, mu, N, sun):
    """V view cosines in [0.01, 1]: the two ends, a node of the grid and one cosine 4e-5 above the sun `sun` of a column (the limit
    branch |mu - mu0| < 1e-4 of the view stage's closed-form first order) among them"""
    mv = np.linspace(0.01, 1.0, V)
    mv[1], mv[2] = mu[N + max(N // 2, 1)], sun + 4e-5
    return frozen(mv)


# ---- the beam --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def beam_columns(name):
    """B three-zone columns (cap-L-2slabs: a five-zone table), Rayleigh + HG(0.7), suns and grounds cycling; P0 on the grid"""
    N, L, B = SHAPES[name]
    mu = O.make_mu(N)
    mu0 = np.array([SUNS[b % 4] for b in range(B)])
    P0a, P0r = (VN.phase_p0_rows(fn, mu, mu0, mu) for fn in (FN_ATM, FN_AER))
    Z2 = no_matrix(N)[1]
    if name.endswith("2slabs"):
        return tuple(O.make_column_slabs(mu0[b], S.Z0, S.TWO_SLABS, L, S.T_ATM, RHOS[b % 5], 1.0, N, P0a[b], Z2, P0r[b], Z2) for b in range(B))
    return tuple(O.make_column(mu0[b], S.Z0, 25, 17, L, S.T_ATM, S.T_AER, RHOS[b % 5], 1.0, 0.97, N, P0a[b], Z2, P0r[b], Z2) for b in range(B))


@functools.lru_cache(maxsize=None)
def beam_model(name, dtype=np.float64):
    """(sigma [B, L] on the sphere, I1 [B, L, 2N] of the model on it)"""
    cols = beam_columns(name)
    z = S.altitudes(len(cols[0].tau))
    sig = np.stack([S.slant_path(c.tau, z, c.mu0, dtype=dtype) for c in cols])
    I1 = np.stack([S.first_order_beam(c, sg, dtype=dtype) for c, sg in zip(cols, sig)])
    return frozen(sig, I1)


@functools.lru_cache(maxsize=None)
def beam_epilogue_model(name, norm):
    """{output: [B, L] or [B]} of spherical_np.epilogue_beam on the model's first order"""
    cols = beam_columns(name)
    sig, I = beam_model(name)
    z = S.altitudes(len(cols[0].tau))
    out = [S.epilogue_beam(I[b], c.mu, c.tau, sig[b], c.N, c.mu0, c.grd_alb, z_profile=z,
                           slabs=[(zn.r0, zn.r1) for zn in c.zones if zn.kind == "mix"], beam_norm=norm) for b, c in enumerate(cols)]
    return {k: frozen(np.stack([o[k] for o in out])) for k in out[0]}


@functools.lru_cache(maxsize=None)
def beam_view_case(name, V, dtype=np.float64):
    """(mu_view [V], p0a, p0r [B, 2V] at the signed lanes, model [B, L, 2V] on the sphere's path)"""
    cols = beam_columns(name)
    mv = view_cosines(V, cols[0].mu, cols[0].N, SUNS[0])
    mu0 = np.array([c.mu0 for c in cols])
    p0a, p0r = (VN.phase_p0_rows(fn, cols[0].mu, mu0, VN.signed(mv)) for fn in (FN_ATM, FN_AER))
    sig = beam_model(name)[0]
    ref = np.stack([SV.view_first_order_beam(c, sig[b], p0a[b], p0r[b], mv, dtype=dtype) for b, c in enumerate(cols)])
    return (mv,) + frozen(p0a, p0r, ref)


# ---- thermal emission -------------------------------------------------------------------------------------------
# (rho, tauStar_atm, alb_atm, tauStar_aer, alb_aer) of tests/test_gpu_thermal.py: a black ground in the second column, an atmosphere
# of 1e-6 in the third, whose layers take the small-x branch of the weights on every lane
THERMAL_BASE = [(0.3, 1.0, 0.2, 0.3, 0.6), (0.0, 0.5, 0.0, 0.3, 0.9), (0.5, 1e-6, 0.3, 2e-6, 0.7)]


@functools.lru_cache(maxsize=None)
def thermal_columns(name, surface):
    N, L, B = SHAPES[name]
    par = [THERMAL_BASE[b] if b < 3 else (0.1 * (b % 6), 0.05 + 0.03 * b, 0.01 * (b % 50), 0.02 * (b % 11), 0.1 * (b % 10)) for b in range(B)]
    if B == 2:
        par = [THERMAL_BASE[0], THERMAL_BASE[2]]
    Z1, Z2 = no_matrix(N)
    if name.endswith("2slabs"):
        return tuple(O.make_column_slabs(T.MU0, T.Z0, T.TWO_SLABS, L, ta, r, wa, N, Z1, Z2, Z1, Z2, surface=surface) for r, ta, wa, _, _ in par)
    return tuple(O.make_column(T.MU0, T.Z0, 25, 17, L, ta, tr, r, wa, wr, N, Z1, Z2, Z1, Z2, surface=surface) for r, ta, wa, tr, wr in par)


@functools.lru_cache(maxsize=None)
def thermal_sources(name):
    """(planck [B, L], planck_surface [B], an explicit emissivity [B])"""
    N, L, B = SHAPES[name]
    b = np.arange(B)
    return frozen(T.planck_profile(L)[None, :] * (1 + 0.1 * b[:, None]), 1 + 0.05 * b, 0.95 - 0.01 * (b % 40))


@functools.lru_cache(maxsize=None)
def thermal_model(name, surface, explicit, dtype=np.float64):
    cols = thermal_columns(name, surface)
    pl, bs, es = thermal_sources(name)
    return frozen(np.stack([T.emission(c, pl[b], bs[b], es[b] if explicit else None, dtype=dtype) for b, c in enumerate(cols)]))


@functools.lru_cache(maxsize=None)
def thermal_view_case(name, V, dtype=np.float64):
    """(mu_view [V], model [B, L, 2V] with the explicit emissivity, specular ground)"""
    cols = thermal_columns(name, "specular")
    pl, bs, es = thermal_sources(name)
    mv = view_cosines(V, cols[0].mu, cols[0].N, T.MU0)
    lev = np.arange(len(cols[0].tau))
    return mv, frozen(np.stack([T.emission_view(c, pl[b], bs[b], mv, lev, es[b], dtype=dtype) for b, c in enumerate(cols)]))


@functools.lru_cache(maxsize=None)
def thermal_reference(name, surface, explicit):
    """What the device's emitted field is compared with: the float64 model; at cap-L its long double evaluation rounded to
    float64 (the module's docstring: there float64 alone spends a fifth of the bound)"""
    if name not in CAP_L:
        return thermal_model(name, surface, explicit)
    return frozen(np.asarray(thermal_model(name, surface, explicit, np.longdouble), dtype=np.float64))


@functools.lru_cache(maxsize=None)
def thermal_view_reference(name, V):
    """(mu_view, reference [B, L, 2V]): thermal_view_case, at cap-L in long double as thermal_reference"""
    if name not in CAP_L:
        return thermal_view_case(name, V)
    mv, ref = thermal_view_case(name, V, np.longdouble)
    return mv, frozen(np.asarray(ref, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def thermal_epilogue_model(name):
    cols = thermal_columns(name, "specular")
    I = thermal_model(name, "specular", False)
    z = T.altitudes(len(cols[0].tau))
    out = [T.epilogue_emission(I[b], c.mu, c.N, z_profile=z, slabs=[(zn.r0, zn.r1) for zn in c.zones if zn.kind == "mix"])
           for b, c in enumerate(cols)]
    return {k: frozen(np.stack([o[k] for o in out])) for k in out[0]}


# ---- view radiance ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def view_columns(name):
    """the columns of test_off_grid_against_the_model (tests/test_gpu_view.py) at the shape, without matrices"""
    N, L, B = SHAPES[name]
    mu0 = np.linspace(0.25, 0.95, B)
    taer = 0.05 + 0.9 * ((np.arange(B) * 7) % 11) / 11
    rho = ((np.arange(B) * 3) % 5) / 5
    Z1, Z2 = no_matrix(N)
    return tuple(O.make_column(mu0[b], VN.Z0, 25, 17, L, 0.124 + 0.4 * (b % 3), taer[b], rho[b], 0.98, 0.9, N, Z1, Z2, Z1, Z2) for b in range(B))


@functools.lru_cache(maxsize=None)
def view_case(name, V):
    """dict: mv [V]; rows_atm, rows_aer [2V, 2N] and src [B, L, 2N] (seeded, positive, src decaying in tau); p0a, p0r [B, 2V]; the
    model on ALL levels: first [B, L, 2V], scat {'grid', 'linear'} [B, L, 2V]"""
    cols = view_columns(name)
    N, L, B = SHAPES[name]
    mu = cols[0].mu
    rng = np.random.default_rng(1000 * N + V)
    mv = view_cosines(V, mu, N, cols[B // 2].mu0)
    sgn = VN.signed(mv)
    mu0 = [c.mu0 for c in cols]
    rows_atm, rows_aer = rng.uniform(0.5, 2.0, (2 * V, 2 * N)), rng.uniform(0.1, 4.0, (2 * V, 2 * N))
    src = rng.uniform(0.1, 1.0, (B, L, 2 * N)) * np.exp(-np.linspace(0, 2, L))[None, :, None]
    p0a, p0r = (VN.phase_p0_rows(fn, mu, mu0, sgn) for fn in (FN_ATM, FN_AER))
    Sm = [VN.source(c, rows_atm, rows_aer, src[b]) for b, c in enumerate(cols)]
    scat = {q: np.stack([VN.transport(c, Sm[b], mv, qid) for b, c in enumerate(cols)]) for q, qid in (("grid", VN.QUAD_GRID), ("linear", VN.QUAD_LINEAR))}
    first = np.stack([VN.first_order(c, p0a[b], p0r[b], mv) for b, c in enumerate(cols)])
    frozen(rows_atm, rows_aer, src, p0a, p0r, first, scat["grid"], scat["linear"])
    return dict(mv=mv, rows_atm=rows_atm, rows_aer=rows_aer, src=src, p0a=p0a, p0r=p0r, first=first, scat=scat)


# ---- the BRDF ground and its view term (DESIGN sections 20, 22, 24) --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ground_case(name):
    """dict on the beam's columns: I [B, L, 2N] a positive field with structure in every index; R [i, j], r0 [B, i], scale [B] (a 0
    among them); Rs [3, i, j], r0s [3, B, i], weight [B, 3] (a column of zeros and a zero term among them): seeded, positive"""
    N, L, B = SHAPES[name]
    M = N - 1
    rng = np.random.default_rng(7000 + N + L)
    I = 0.05 + rng.random((B, L, 2 * N)) * (1 + np.arange(2 * N) / N)[None, None, :]
    R, r0 = rng.uniform(0.1, 1.0, (M, M)) / M, rng.uniform(0.05, 0.5, (B, M))
    scale = np.array([(0.3, 0.0, 0.8)[b % 3] for b in range(B)])
    Rs, r0s = rng.uniform(0.1, 1.0, (3, M, M)) / M, rng.uniform(0.05, 0.5, (3, B, M))
    weight = np.array([[(0.05, 0.0, 0.0), (0.0, 0.0, 0.0), (0.30, 0.15, 0.04), (0.10, 0.60, 0.02)][b % 4] for b in range(B)])
    frozen(I, R, r0, scale, Rs, r0s, weight)
    return dict(I=I, R=R, r0=r0, scale=scale, Rs=Rs, r0s=r0s, weight=weight)


@functools.lru_cache(maxsize=None)
def ground_view_case(name, V):
    """dict: mv [V]; Rv [v, j], r0v [B, v]; Rvs [3, v, j], r0vs [3, B, v]: seeded, positive"""
    cols = beam_columns(name)
    N, L, B = SHAPES[name]
    M = N - 1
    rng = np.random.default_rng(9000 + N + L + V)
    mv = view_cosines(V, cols[0].mu, N, SUNS[0])
    Rv, r0v = rng.uniform(0.1, 1.0, (V, M)) / M, rng.uniform(0.05, 0.5, (B, V))
    Rvs, r0vs = rng.uniform(0.1, 1.0, (3, V, M)) / M, rng.uniform(0.05, 0.5, (3, B, V))
    frozen(Rv, r0v, Rvs, r0vs)
    return dict(mv=mv, Rv=Rv, r0v=r0v, Rvs=Rvs, r0vs=r0vs)


def rough_then_smooth(S):
    """A ground source [B, N-1] whose first N - 11 lanes alternate by half of themselves: on the rows next to the ground the
    blend's search fails on them lane after lane and stops in its last trip of 64"""
    S = np.array(S)
    k = S.shape[1] - 10
    S[:, :k] *= 1 + 0.5 * (-1.0) ** np.arange(k)
    return S


# ---- per-level weights on the source function -------------------------------------------------------------------------
FN_AER_B = VN.phase_fn("hg", 0.3)                            # the second aerosol of the P0-per-zone case


@functools.lru_cache(maxsize=None)
def profile_weights(name, thermal=False):
    """(w_atm, w_aer) [B, L] of profile_np.random_weights per column (jumps at the first slab's first and last row, rows of
    exact 1 and exact 0), on the beam's columns or on the thermal ones"""
    cols = thermal_columns(name, "specular") if thermal else beam_columns(name)
    w = [P.random_weights(c, 500 + b) for b, c in enumerate(cols)]
    return frozen(np.stack([x[0] for x in w]), np.stack([x[1] for x in w]))


@functools.lru_cache(maxsize=None)
def profile_sigma(name, path):
    """the beam's path [B, L]: tau / mu0 on the plane, spherical_np.slant_path on the sphere"""
    if path == "plane":
        return frozen(np.stack([S.plane_path(c.tau, c.mu0) for c in beam_columns(name)]))
    return beam_model(name)[0]


@functools.lru_cache(maxsize=None)
def profile_p0_zones(name):
    """[B, 5, 2N]: a P0 of the aerosol per zone of the two-slab table, the first slab's HG(0.7), the second's HG(0.3)"""
    cols = beam_columns(name)
    mu0 = [c.mu0 for c in cols]
    P0b = VN.phase_p0_rows(FN_AER_B, cols[0].mu, mu0, cols[0].mu)
    P0z = np.zeros((len(cols), 5, 2 * cols[0].N))
    for b, c in enumerate(cols):
        P0z[b, 1], P0z[b, 3] = c.P0_aer, P0b[b]
    return frozen(P0z)


@functools.lru_cache(maxsize=None)
def profile_first_order_model(name, path, zp0=False, dtype=np.float64):
    """I1 [B, L, 2N] of profile_np.first_order_profile on the path; zp0: with profile_p0_zones"""
    cols, sig = beam_columns(name), profile_sigma(name, path)
    wa, wr = profile_weights(name)
    P0z = profile_p0_zones(name) if zp0 else [None] * len(cols)
    return frozen(np.stack([P.first_order_profile(c, sig[b], wa[b], wr[b], P0_aer_zone=P0z[b], dtype=dtype) for b, c in enumerate(cols)]))


@functools.lru_cache(maxsize=None)
def profile_emission_model(name, surface, explicit, dtype=np.float64):
    cols = thermal_columns(name, surface)
    pl, bs, es = thermal_sources(name)
    wa, wr = profile_weights(name, True)
    return frozen(np.stack([P.emission_profile(c, pl[b], bs[b], wa[b], wr[b], es[b] if explicit else None, dtype=dtype) for b, c in enumerate(cols)]))


def profile_float64_gaps():
    """[(model, shape, gap)] at the two profile-cap-L shapes, as float64_gaps"""
    ld = np.longdouble
    out = []
    worst = lambda a, l: max(_gap(a[b], l[b]) for b in range(len(a)))
    for name in PROFILE_CAP_L:
        for path in ("plane", "slant"):
            out.append(("profile_np.first_order_profile " + path, name, worst(profile_first_order_model(name, path), profile_first_order_model(name, path, False, ld))))
    name = "profile-cap-L-2slabs"
    out.append(("profile_np.first_order_profile, P0 per zone", name, worst(profile_first_order_model(name, "plane", True), profile_first_order_model(name, "plane", True, ld))))
    for name in PROFILE_CAP_L:
        for surface in ("specular", "lambertian", "lambertian_readme"):
            for explicit in (False, True):
                out.append(("profile_np.emission_profile %s%s" % (surface, " emissivity given" if explicit else ""), name,
                            worst(profile_emission_model(name, surface, explicit), profile_emission_model(name, surface, explicit, ld))))
    return out


# ---- float64 against long double ------------------------------------------------------------------------------------------------------
def _gap(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def float64_gaps():
    """[(model, shape, gap)]: the float64 models against their evaluation in np.longdouble, in the measure of the test that uses them"""
    ld = np.longdouble
    out = []
    for name in CAP_L:
        sig, I1 = beam_model(name)
        sig_l, I1_l = beam_model(name, ld)
        if name == "cap-L":
            out.append(("spherical_np.slant_path", name, max(_gap(sig[b], sig_l[b]) for b in range(len(sig)))))
        out.append(("spherical_np.first_order_beam", name, max(_gap(I1[b], I1_l[b]) for b in range(len(sig)))))
    ref, ref_l = beam_view_case("cap-L", 64)[3], beam_view_case("cap-L", 64, ld)[3]
    out.append(("spherical_view_np.view_first_order_beam V=64", "cap-L", max(_gap(ref[b], ref_l[b]) for b in range(len(ref)))))
    for name, surface in (("cap-L", "specular"), ("cap-L", "lambertian"), ("cap-L-2slabs", "specular"), ("cap-N", "lambertian")):
        a, b_ = thermal_model(name, surface, True), thermal_model(name, surface, True, ld)
        out.append(("thermal_np.emission " + surface, name, max(_gap(a[b], b_[b]) for b in range(len(a)))))
    a, b_ = thermal_view_case("cap-L", 64)[1], thermal_view_case("cap-L", 64, ld)[1]
    out.append(("thermal_np.emission_view V=64", "cap-L", max(_gap(a[b], b_[b]) for b in range(len(a)))))
    # the epilogues at cap-L: the flux sums and the heating rate's differences on a long double field, grid and altitudes
    for name in CAP_L:
        worst = [0.0, 0.0]
        for i, cols, I in ((0, beam_columns(name), beam_model(name)[1]), (1, thermal_columns(name, "specular"), thermal_model(name, "specular", False))):
            z = S.altitudes(len(cols[0].tau))
            for b, c in enumerate(cols):
                slabs = [(zn.r0, zn.r1) for zn in c.zones if zn.kind == "mix"]
                epi = ((lambda I_, mu_, z_: S.epilogue_beam(I_, mu_, c.tau, beam_model(name)[0][b], c.N, c.mu0, c.grd_alb, z_profile=z_, slabs=slabs))
                       if i == 0 else (lambda I_, mu_, z_: T.epilogue_emission(I_, mu_, c.N, z_profile=z_, slabs=slabs)))
                a, l = epi(I[b], c.mu, z), epi(I[b].astype(ld), c.mu.astype(ld), z.astype(ld))
                keys = [k for k in a if not (i == 1 and k == "heating_rate" and c.tauStar_tot < 1e-3)]     # (as the test)
                worst[i] = max(worst[i], max(_gap(np.atleast_1d(a[k]), np.atleast_1d(l[k])) for k in keys))
        out.append(("spherical_np.epilogue_beam (worst output)", name, worst[0]))
        out.append(("thermal_np.epilogue_emission (worst output)", name, worst[1]))
    # cap-N: the dot products, as the models write them, on long double arrays
    name = "cap-N"
    cols, g = beam_columns(name), ground_case(name)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    live = [b for b in range(len(cols)) if g["scale"][b] != 0]
    args = lambda b, f: (f(g["I"][b, -1]), f(g["r0"][b]), f(cols[b].tau[-1]), f(cols[b].mu0), f(g["scale"][b]))
    out.append(("brdf_np.ground_source", name, max(rel(G.ground_source(g["R"], *args(b, np.float64)),
                                                      G.ground_source(g["R"].astype(ld), *args(b, ld))) for b in live)))
    terms = lambda b, f: RL.ground_source_terms(g["Rs"].astype(f), f(g["I"][b, -1]), g["r0s"][:, b].astype(f), f(cols[b].tau[-1]),
                                                f(cols[b].mu0), g["weight"][b].astype(f))
    S64, Sld = np.stack([terms(b, np.float64) for b in range(len(cols))]), np.stack([terms(b, ld) for b in range(len(cols))])
    out.append(("ross_li_np.ground_source_terms", name, _gap(S64, Sld)))
    gv = ground_view_case(name, 64)
    vargs = lambda b, f: (f(g["I"][b, -1]), f(gv["r0v"][b]), f(cols[b].tau[-1]), f(cols[b].mu0), f(g["scale"][b]))
    out.append(("brdf_np.ground_source at view lanes V=64", name, max(rel(G.ground_source(gv["Rv"], *vargs(b, np.float64)),
                                                                         G.ground_source(gv["Rv"].astype(ld), *vargs(b, ld))) for b in live)))
    vc, vcols = view_case(name, 64), view_columns(name)
    gap = 0.0
    for b, c in enumerate(vcols):
        a = VN.source(c, vc["rows_atm"], vc["rows_aer"], vc["src"][b])
        # (view_np.source stores into a float64 array: its rows are evaluated here as it writes them, on long double arrays)
        Ra, Rr, src = vc["rows_atm"][:, ::-1].astype(ld), vc["rows_aer"][:, ::-1].astype(ld), vc["src"][b].astype(ld)
        for z in c.zones:
            for t in range(z.r0, z.r1 + 1):
                if z.kind == "mix":
                    fa, fr = c.zone_fractions(z)
                    row = (c.alb_atm / 4) * VN._trapz(Ra * src[t], c.mu, axis=1) * fa + (z.alb_aer / 4) * VN._trapz(Rr * src[t], c.mu, axis=1) * fr
                else:
                    row = (c.alb_atm / 4) * VN._trapz(Ra * src[t], c.mu, axis=1)
                gap = max(gap, float(np.max(np.abs(a[t] - row) / np.abs(row))))
    out.append(("view_np.source V=64", name, gap))
    return out


if __name__ == "__main__":
    for model, shape, gap in float64_gaps() + profile_float64_gaps():
        print("%-46s %-20s float64 vs longdouble %.1e" % (model, shape, gap))
