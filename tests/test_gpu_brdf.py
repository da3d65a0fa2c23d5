"""BRDF ground on the device (csrc/brdf.hip, csrc/api_brdf.hip) through the C ABI: the five stages against the
NumPy model of tests/brdf_np.py (which tests/test_brdf_host.py pins to the oracle's in-loop Lambertian ground), the whole
driver against the model's series on the oracle, the Lambertian operator against the device's own in-loop ground in the linear
regime, the blend that runs off a row, every refusal, and the default path's bytes."""
import ctypes
import functools

import numpy as np
import pytest

import brdf_np as M
import sos_oracle as O
from sosrt import _lib
from sosrt.solver import Solver

pytestmark = pytest.mark.gpu

RTOL = 1e-10
RPV = ("rpv", 0.2, 0.8, -0.1)
SHAPES = [(24, 37), (24, 66), (30, 64)]      # (L, N): N-1 = 36 a partial wave, 65 one lane into a second wave, 63
MU0S, SCALES = (0.35, 0.6, 0.85), (0.0, 0.3, 0.8)


def _torch():
    return pytest.importorskip("torch")


def dev(a, dtype=np.float64):
    torch = _torch()
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(torch.device("cuda", 0))


def dfull(shape, fill=np.nan, guard=0):
    """a float64 device tensor of `shape` filled with `fill`, with `guard` more elements behind it"""
    torch = _torch()
    n = int(np.prod(shape))
    return torch.full((n + guard,), fill, dtype=torch.float64, device=torch.device("cuda", 0))


def host(t, s, shape=None):
    s.synchronize()
    a = t.cpu().numpy()
    return a if shape is None else a[:int(np.prod(shape))].reshape(shape)


def sync():
    _torch().cuda.synchronize()


@functools.lru_cache(maxsize=None)
def columns(L, N, B=3, surface="specular", rho=0.0, p0_scale=1.0):
    return tuple(M.experiment_column(O, N, L, MU0S[b], rho, p0_scale, surface) for b in range(B))


def handle(cols, max_orders=64):
    c0 = cols[0]
    L, N, B = len(c0.tau), c0.N, len(cols)
    s = Solver(L, N, max_batch=B, max_orders=max_orders)
    s.set_grid(c0.mu)
    s.set_phase(c0.P_atm, c0.P_aer)
    col = lambda f: [f(c) for c in cols]
    s.set_columns(col(lambda c: c.idx_up), col(lambda c: c.idx_down), col(lambda c: c.mu0), col(lambda c: c.grd_alb),
                  col(lambda c: c.alb_atm), col(lambda c: c.alb_aer), col(lambda c: c.dtau_atm), col(lambda c: c.dtau_aer),
                  col(lambda c: c.tauStar_tot), surface=c0.surface)
    return s, np.stack([c.tau for c in cols])


def params_of(brdf):
    return ("lambertian", ()) if brdf == "lambertian" else (brdf[0], brdf[1:])


def run_operator(s, brdf, nphi=65):
    M1 = s.N - 1
    d_R = dfull((M1, M1))
    sync()
    kind, p = params_of(brdf)
    s.brdf_operator_device(kind, d_R.data_ptr(), p, nphi)
    return host(d_R, s).reshape(M1, M1).T            # [i, j], as the model writes it


def run_beam(s, brdf, mu0, nphi=65):
    B = len(mu0)
    d_mu0, d_r0 = dev(mu0), dfull((B, s.N - 1))
    sync()
    kind, p = params_of(brdf)
    s.brdf_beam_device(kind, d_mu0.data_ptr(), d_r0.data_ptr(), p, nphi, B=B)
    return host(d_r0, s).reshape(B, s.N - 1)


def run_source(s, I, tau, R, r0=None, scale=None):
    B = tau.shape[0]
    d = [dev(I), dev(tau), dev(R.T)]
    d_r0, d_sc = None if r0 is None else dev(r0), None if scale is None else dev(scale)
    d_S = dfull((B, s.N - 1))
    sync()
    s.ground_source_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_S.data_ptr(), 0 if d_r0 is None else d_r0.data_ptr(),
                           0 if d_sc is None else d_sc.data_ptr(), B=B)
    return host(d_S, s).reshape(B, s.N - 1)


def run_field(s, tau, S):
    torch = _torch()
    B = tau.shape[0]
    d_tau, d_S, d_G = dev(tau), dev(S), dfull((B, s.L, s.D))
    d_st = torch.full((B,), -1, dtype=torch.int32, device=d_tau.device)
    sync()
    s.ground_first_order_device(d_tau.data_ptr(), d_S.data_ptr(), d_G.data_ptr(), d_st.data_ptr(), B=B)
    return host(d_G, s).reshape(B, s.L, s.D), d_st.cpu().numpy()


@functools.lru_cache(maxsize=None)
def sample_field(L, N, B=3):
    """a positive field [B, L, 2N] with structure in every index, shared by the stage tests and never changed"""
    rng = np.random.default_rng(1000 * L + N)
    I = 0.05 + rng.random((B, L, 2 * N)) * (1 + np.arange(2 * N) / N)[None, None, :]
    I.setflags(write=False)
    return I


@functools.lru_cache(maxsize=None)
def model_operator(N, brdf):
    mu = O.make_mu(N)
    R, r0 = M.operator(mu, N, brdf), np.stack([M.beam_row(mu, N, m, brdf) for m in MU0S])
    R.setflags(write=False)
    r0.setflags(write=False)
    return R, r0


# ---- a. the kernels against the model --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brdf", ["lambertian", RPV], ids=["lambertian", "rpv"])
@pytest.mark.parametrize("L,N", SHAPES)
def test_operator_and_beam_rows_against_the_model(L, N, brdf):
    s, _ = handle(columns(L, N))
    R, r0 = model_operator(N, brdf)
    got_R, got_r0 = run_operator(s, brdf), run_beam(s, brdf, MU0S)
    eR, e0 = np.max(np.abs(got_R - R)) / np.max(R), np.max(np.abs(got_r0 - r0) / r0)
    print("L=%d N=%d %s: operator %.3e of its maximum, beam rows %.3e relative" % (L, N, brdf, eR, e0))
    assert np.all(np.isfinite(got_R)) and eR <= 1e-12 and e0 <= 1e-12
    assert np.array_equal(run_beam(s, brdf, MU0S[:1]), got_r0[:1])
    if brdf != "lambertian":                                 # another node count: the chunked cosine table (nphi > 256)
        mu = O.make_mu(N)
        assert np.max(np.abs(run_operator(s, brdf, 301) - M.operator(mu, N, brdf, 301))) / np.max(R) <= 1e-12
    s.close()


@pytest.mark.parametrize("L,N", SHAPES)
def test_ground_source_against_the_model(L, N):
    cols = columns(L, N)
    s, tau = handle(cols)
    I = sample_field(L, N)
    R, r0 = model_operator(N, RPV)
    scale = np.array([0.3, 0.0, 0.8])
    for use_r0, use_scale in ((True, True), (False, True), (True, False), (False, False)):
        ref = np.stack([M.ground_source(R, I[b, -1], r0[b] if use_r0 else None, tau[b, -1], MU0S[b], scale[b] if use_scale else 1.0)
                        for b in range(3)])
        got = run_source(s, I, tau, R, r0 if use_r0 else None, scale if use_scale else None)
        live = [b for b in range(3) if not (use_scale and scale[b] == 0)]
        err = max(np.max(np.abs(got[b] - ref[b]) / np.abs(ref[b])) for b in live)
        print("L=%d N=%d beam %s scale %s: ground source %.3e relative" % (L, N, use_r0, use_scale, err))
        assert err <= 1e-13
        if use_scale:
            assert not np.any(got[1]) and not np.any(np.signbit(got[1]))      # scale 0: exact zeros
        one = run_source(s, I[:1], tau[:1], R, r0[:1] if use_r0 else None, scale[:1] if use_scale else None)
        assert np.array_equal(one[0], got[0])                # a column's bits do not depend on B
    s.close()


def smooth_source(N, B=3):
    # (of the size of a real ground source: at N = 37 the second differences of a source of order 1 stay above the search's 1e-4)
    i = np.arange(N - 1) / (N - 1)
    return np.stack([(0.04 + 0.02 * b) * (1 + 0.3 * i) for b in range(B)])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L,N", SHAPES)
def test_ground_field_against_the_model(L, N, B):
    cols = columns(L, N)[:B]
    s, tau = handle(cols)
    S = smooth_source(N, B)
    got, st = run_field(s, tau, S)
    assert np.array_equal(st, np.zeros(B, dtype=np.int32))
    for b, c in enumerate(cols):
        ref, status, blended = M.ground_field(S[b], c.tau, c.mu, N)
        mx = np.max(ref)
        d = np.abs(got[b] - ref)
        e_plain, e_blend = np.max(d[~blended]) / mx, np.max(d[blended]) / mx
        print("L=%d N=%d B=%d column %d: ground field %.3e unblended, %.3e on %d blended lanes" % (L, N, B, b, e_plain, e_blend, blended.sum()))
        assert status == 0 and blended.any() and e_plain <= 1e-12 and e_blend <= 1e-10
        assert not np.any(got[b][:, :N + 1]) and not np.any(np.signbit(got[b][:, :N + 1]))    # lane N and the downward lanes: +0
    s.close()


@pytest.mark.parametrize("L,N", SHAPES)
def test_accumulate_is_the_exact_sum_and_the_ratio(L, N):
    s, _ = handle(columns(L, N))
    total0 = np.array(sample_field(L, N))
    Ik = 0.01 * np.array(sample_field(L, N))[:, ::-1, ::-1] * np.array([1.0, -1.0, 0.5])[:, None, None]
    Ik[1, 0, N:] = 0
    Ik[1, -1, :N] = 0
    total0[1, 0, N:] = 0                                     # the second column: both rows of the ratio are zero in the total
    total0[1, -1, :N] = 0
    d_Ik, d_tot, d_ratio = dev(Ik), dev(total0), dfull((3,))
    sync()
    s.bounce_accumulate_device(d_Ik.data_ptr(), d_tot.data_ptr(), d_ratio.data_ptr(), B=3)
    tot, ratio = host(d_tot, s), host(d_ratio, s)
    assert np.array_equal(tot, total0 + Ik)
    ref = np.array([M.bounce_ratio(Ik[b], (total0 + Ik)[b], N) for b in range(3)])
    print("L=%d N=%d ratios %s (model %s)" % (L, N, ratio, ref))
    assert ratio[1] == 0 and np.all(np.abs(ratio - ref) <= 1e-15 * np.maximum(ref, 1))
    s.close()


# ---- b. the whole driver against the model's series on the oracle ----------------------------------------------------------------------
def driver(L, N, brdf, grd_alb, **kw):
    from sosrt.main import SOS_Aer_batch
    cols = columns(L, N)
    c = cols[0]
    return SOS_Aer_batch(list(MU0S), 0.3, grd_alb, tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.9, nb_layers=L, nb_angles=N,
                         P_atm=c.P_atm, P_aer=c.P_aer, P0_atm=np.stack([x.P0_atm for x in cols]), P0_aer=np.stack([x.P0_aer for x in cols]),
                         max_orders=64, surface="brdf", brdf=brdf, **kw)


@functools.lru_cache(maxsize=None)
def model_series(L, N, brdf):
    R, r0 = model_operator(N, brdf)
    with np.errstate(all="ignore"):
        out = M.bounce_solve(O, columns(L, N), R, r0, SCALES if brdf == "lambertian" else (1.0, 1.0, 1.0))
    out[0].setflags(write=False)
    return out


@pytest.mark.parametrize("L,N,brdf", [(24, 37, "lambertian"), (30, 64, "lambertian"), (24, 66, "lambertian"), (24, 37, RPV)],
                         ids=["L24-N37-lambertian", "L30-N64-lambertian", "L24-N66-lambertian", "L24-N37-rpv"])
def test_driver_against_the_model_series(L, N, brdf):
    ref, bounces, ratio, status, terms = model_series(L, N, brdf)
    r = driver(L, N, brdf, list(SCALES) if brdf == "lambertian" else 1.0, raise_on_error=False)
    assert np.all(np.isfinite(r.I))
    err = [float(np.max(np.abs(r.I[b] - ref[b])) / np.max(np.abs(ref[b]))) for b in range(3)]
    print("L=%d N=%d %s: bounces %s (model %s), field vs the model's series %s of the maximum, ratios %s" %
          (L, N, brdf, r.bounces, bounces, ["%.2e" % e for e in err], r.bounce_ratio))
    # (at N = 37 the ground rows of the scale-0.8 column leave the grid in the blend's search, on the device as in the model: the
    # reference's IndexError, reported as the column's status; the rows stay unblended on both sides)
    assert np.array_equal(r.bounces, bounces) and np.array_equal(r.status, status)
    assert list(status) == ([0, 0, M.COL_INDEXERROR] if (N, brdf) == (37, "lambertian") else [0, 0, 0])
    assert max(err) <= RTOL
    assert np.all(np.abs(r.bounce_ratio - ratio) <= 1e-6 * np.maximum(ratio, 1e-12))
    if brdf == "lambertian":
        assert r.bounces[0] == 1 and r.bounce_ratio[0] == 0  # the black column: one bounce of zeros


def test_a_zero_scale_bounce_is_exact_zeros():
    """the stages on a column whose scale is 0: ground source, ground field and the solve started from it are +0 everywhere, no NaN"""
    torch = _torch()
    L, N = 24, 37
    cols = columns(L, N)
    s, tau = handle(cols)
    R, r0 = model_operator(N, "lambertian")
    S = run_source(s, sample_field(L, N), tau, R, r0, np.array(SCALES))
    G, st = run_field(s, tau, S)
    d_tau, d_G, d_Ik = dev(tau), dev(G), dfull((3, L, 2 * N))
    d_n, d_st = (torch.zeros(3, dtype=torch.int32, device=d_tau.device) for _ in range(2))
    sync()
    s.solve_device(d_tau.data_ptr(), 0, 0, d_Ik.data_ptr(), d_I1=d_G.data_ptr(), d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
    Ik = host(d_Ik, s).reshape(3, L, 2 * N)
    print("orders of the three bounce solves: %s, status %s" % (d_n.cpu().numpy(), d_st.cpu().numpy()))
    assert not np.any(S[0]) and not np.any(G[0]) and not np.any(Ik[0]) and not np.any(np.isnan(Ik))
    assert np.all(Ik[1:, 0, N + 1:] > 0) and not d_st.cpu().numpy().any()
    # the oracle makes the same decisions on an all-zero first order: 1 / 0 = inf goes on, 0 / 0 = NaN stops
    with np.errstate(all="ignore"):
        assert O.solve_column(cols[0], literal=False, I1=np.zeros((L, 2 * N))).n == int(d_n.cpu().numpy()[0])
    s.close()


def test_arrays_are_the_named_ground():
    L, N = 24, 66
    R, r0 = model_operator(N, "lambertian")
    a, b = driver(L, N, "lambertian", list(SCALES)), driver(L, N, (np.array(R), np.array(r0)), list(SCALES))
    assert np.array_equal(a.bounces, b.bounces)
    assert np.max(np.abs(a.I - b.I)) <= 1e-12 * np.max(a.I)


def test_the_cap_gives_a_status():
    r = driver(24, 66, "lambertian", list(SCALES), max_bounces=2)
    assert list(r.bounces) == [1, 2, 2] and list(r.status) == [0, _lib.COL_MAXORDERS, _lib.COL_MAXORDERS]


def test_flux_driver_over_a_brdf_ground():
    """toa_net_flux over the Lambertian BRDF ground: the flux of the model's field by the oracle's quadrature with grd_alb = 0"""
    from sosrt import forcing
    L, N = 24, 37
    c = columns(L, N)[1]
    got = forcing._net_flux_columns(c.tau[None], c.idx_up, c.idx_down, c.mu, c.mu0, 0.3, 1.0, 0.9, c.dtau_atm, c.dtau_aer,
                                    c.tauStar_tot, c.P_atm, c.P_aer, c.P0_atm, c.P0_aer, max_orders=64, surface="brdf", brdf="lambertian")
    R, r0 = model_operator(N, "lambertian")
    with np.errstate(all="ignore"):
        I = M.bounce_solve(O, [c], R, r0[1:2], [0.3])[0][0]
    ref = O.toa_net_flux(I, c.mu, c.tau, N, c.mu0, 0.0)
    print("net TOA flux over the BRDF ground %.12g (model %.12g)" % (got[0], ref))
    assert abs(got[0] - ref) <= 1e-9 * abs(ref)


# ---- c. the Lambertian operator against the device's own in-loop ground, linear regime ---------------------------------------------------
def test_lambertian_operator_is_the_in_loop_ground_in_the_linear_regime():
    """P0 and the beam term scaled by 1e-6: every blend search stops at its first test, the blend is a fixed linear map, and the
    series is the in-loop SOSRT_SURFACE_LAMBERTIAN_README solve from the same I1_in (the black first order + the ground field of
    its surface row and of the beam)."""
    from sosrt import main
    L, N, rho, k, tol = 30, 64, 0.3, 1e-6, 1e-12
    c = columns(L, N, 3, "specular", 0.0, k)[1]
    s, tau = handle([c], max_orders=128)
    R, r0 = model_operator(N, "lambertian")
    P0a, P0r = c.P0_atm[None], c.P0_aer[None]
    spec = main._brdf_args("brdf", (np.array(R), k * r0[1]), rho, N, 1)
    r, bx, _ = main.solve_brdf(s, tau, P0a, P0r, spec, [c.mu0], tol=tol, max_bounces=64)
    I1b = s.first_order(tau, P0a, P0r)
    S = run_source(s, I1b, tau, R, k * r0[1:2], np.array([rho]))
    G1, st = run_field(s, tau, S)
    lam = columns(L, N, 3, "lambertian_readme", rho, k)[1]
    s2, _ = handle([lam], max_orders=128)
    ref = s2.solve(tau, P0a, P0r, tol=tol, I1=I1b + G1)
    err = float(np.max(np.abs(r.I[0] - ref.I[0])) / np.max(np.abs(ref.I[0])))
    print("linear regime on the device: series (%d bounces) vs the in-loop ground (%d orders): %.3e of the maximum" %
          (bx["bounces"][0], ref.n[0], err))
    assert not r.status.any() and not ref.status.any() and st[0] == 0 and err <= 1e-10
    s.close()
    s2.close()


# ---- d. the blend running off the row --------------------------------------------------------------------------------------------------
def test_a_search_that_leaves_the_row_is_a_status():
    L, N = 24, 37
    cols = columns(L, N)
    s, tau = handle(cols)
    S = smooth_source(N)
    S[1] = (-1.0) ** np.arange(N - 1)
    got, st = run_field(s, tau, S)
    assert list(st) == [_lib.COL_OK, _lib.COL_INDEXERROR, _lib.COL_OK]
    for b in (0, 2):
        ref = M.ground_field(S[b], cols[b].tau, cols[b].mu, N)[0]
        assert np.max(np.abs(got[b] - ref)) <= 1e-10 * np.max(ref)
    ref, status, blended = M.ground_field(S[1], cols[1].tau, cols[1].mu, N)
    assert status == M.COL_INDEXERROR and not blended[-1].any()
    assert np.all(np.isfinite(got[1])) and np.array_equal(got[1][-1, N + 1:], S[1])       # the surface row: unblended, the source itself
    assert np.max(np.abs(got[1] - ref)) <= 1e-10
    s.close()


# ---- e. refusals: nothing is written -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    torch = _torch()
    L, N = 24, 37
    M1 = N - 1
    s, tau = handle(columns(L, N))
    lib = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    G = 7                                                     # guard elements behind every output
    d_R, d_r0, d_S, d_G, d_ratio = (dfull(sh, guard=G) for sh in ((M1, M1), (3, M1), (3, M1), (3, L, 2 * N), (3,)))
    d_I, d_tau, d_mu0 = dev(sample_field(L, N)), dev(tau), dev(MU0S)
    d_tot = dev(sample_field(L, N))
    d_st = torch.full((3 + G,), -7, dtype=torch.int32, device=d_tau.device)
    rpv = (ctypes.c_double * 3)(0.2, 0.8, -0.1)
    P = lambda *v: (ctypes.c_double * 3)(*v)
    op = lambda kind, p, n, nphi, out=d_R: lib.sosrt_brdf_operator_dev(s._h, kind, p, n, nphi, vp(out))
    beam = lambda B, kind, p, n, nphi, mu0=d_mu0, out=d_r0: lib.sosrt_brdf_beam_dev(s._h, B, kind, p, n, nphi, vp(mu0), vp(out))
    src = lambda B, I=d_I, t=d_tau, R=d_R, out=d_S: lib.sosrt_ground_source_dev(s._h, B, vp(I), vp(t), vp(R), None, None, vp(out))
    fld = lambda B, t=d_tau, S=d_S, out=d_G: lib.sosrt_ground_first_order_dev(s._h, B, vp(t), vp(S), vp(out), vp(d_st))
    acc = lambda B, Ik=d_I, tot=d_tot, out=d_ratio: lib.sosrt_bounce_accumulate_dev(s._h, B, vp(Ik), vp(tot), vp(out))
    calls = {
        "operator nphi": lambda: op(_lib.BRDF_RPV, rpv, 3, 2), "operator kind": lambda: op(7, None, 0, 65),
        "operator nparams": lambda: op(_lib.BRDF_RPV, rpv, 2, 65), "operator lambertian nparams": lambda: op(_lib.BRDF_LAMBERTIAN, rpv, 3, 65),
        "operator rho0": lambda: op(_lib.BRDF_RPV, P(0.0, 0.8, -0.1), 3, 65), "operator k": lambda: op(_lib.BRDF_RPV, P(0.2, -1.0, 0.0), 3, 65),
        "operator theta": lambda: op(_lib.BRDF_RPV, P(0.2, 0.8, 1.0), 3, 65), "operator nan": lambda: op(_lib.BRDF_RPV, P(0.2, 0.8, np.nan), 3, 65),
        "operator null params": lambda: op(_lib.BRDF_RPV, None, 3, 65), "operator null out": lambda: op(_lib.BRDF_LAMBERTIAN, None, 0, 65, None),
        "beam B=0": lambda: beam(0, _lib.BRDF_LAMBERTIAN, None, 0, 65), "beam B=4": lambda: beam(4, _lib.BRDF_LAMBERTIAN, None, 0, 65),
        "beam nphi": lambda: beam(3, _lib.BRDF_LAMBERTIAN, None, 0, 1), "beam kind": lambda: beam(3, -1, None, 0, 65),
        "beam null mu0": lambda: beam(3, _lib.BRDF_LAMBERTIAN, None, 0, 65, None), "beam null out": lambda: beam(3, _lib.BRDF_LAMBERTIAN, None, 0, 65, d_mu0, None),
        "source B=0": lambda: src(0), "source B=4": lambda: src(4), "source null I": lambda: src(3, None), "source null tau": lambda: src(3, d_I, None),
        "source null R": lambda: src(3, d_I, d_tau, None), "source null out": lambda: src(3, d_I, d_tau, d_R, None),
        "field B=0": lambda: fld(0), "field B=4": lambda: fld(4), "field null tau": lambda: fld(3, None), "field null S": lambda: fld(3, d_tau, None),
        "field null out": lambda: fld(3, d_tau, d_S, None),
        "accumulate B=0": lambda: acc(0), "accumulate B=4": lambda: acc(4), "accumulate null Ik": lambda: acc(3, None),
        "accumulate null total": lambda: acc(3, d_I, None), "accumulate null out": lambda: acc(3, d_I, d_tot, None),
    }

    def untouched():
        s.synchronize()
        sync()
        return (all(bool(torch.isnan(t).all()) for t in (d_R, d_r0, d_S, d_G, d_ratio)) and bool((d_st == -7).all())
                and np.array_equal(d_tot.cpu().numpy(), sample_field(L, N)))

    for name, call in calls.items():
        rc = call()
        assert rc == _lib.E_INVALID and lib.sosrt_last_error(), name
        assert untouched(), name
    # the single slab: every entry point
    s.set_columns_single_slab([0.5, 0.6, 0.7], 0.9, 0.3)
    for name, call in {"operator": lambda: op(_lib.BRDF_LAMBERTIAN, None, 0, 65), "beam": lambda: beam(3, _lib.BRDF_LAMBERTIAN, None, 0, 65),
                       "source": lambda: src(3), "field": lambda: fld(3), "accumulate": lambda: acc(3)}.items():
        assert call() == _lib.E_INVALID and b"single slab" in lib.sosrt_last_error(), name
        assert untouched(), name
    s.close()
    with pytest.raises(ValueError):
        Solver(L, 3)                                          # N < 4 never becomes a handle


# ---- f. the default path -----------------------------------------------------------------------------------------------------------------
def test_a_brdf_call_leaves_the_default_path_its_bytes():
    from sosrt.main import SOS_Aer_batch
    L, N = 24, 66
    kw = dict(tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.9, nb_layers=L, nb_angles=N, max_orders=64)
    plain = lambda: SOS_Aer_batch(list(MU0S), 0.3, [0.1, 0.3, 0.5], **kw)
    before = plain()
    r = SOS_Aer_batch(list(MU0S), 0.3, [0.1, 0.3, 0.5], surface="brdf", brdf="lambertian", **kw)
    after = plain()
    assert r.bounces is not None and before.bounces is None and not r.status.any()
    assert np.array_equal(before.I, after.I) and np.array_equal(before.n, after.n) and np.array_equal(before.status, after.status)
    assert np.max(np.abs(r.I - before.I)) > 1e-3 * np.max(before.I)      # another ground: another field


def test_the_other_drivers_reach_the_same_series():
    from sosrt.main import SOS_Aer, SOS_Aer_batch, SOS_Aer_layers, solve_batch_device
    kw = dict(tauStar_atm=0.124, alb_atm=1.0, nb_layers=24, nb_angles=66, max_orders=64, surface="brdf", brdf="lambertian")
    ref = SOS_Aer_batch([0.6], 0.3, [0.3], alb_aer=0.9, **kw)
    lay = SOS_Aer_layers([0.6], [0.3], [(25, 17, 0.3, 0.9)], **kw)
    one = SOS_Aer(mu0=0.6, tauStar_aer=0.3, grd_alb=0.3, alb_aer=0.9, aer_phase_fun="hg", g_aer=0.7, **kw)
    res, _ = solve_batch_device([0.6], 0.3, [0.3], alb_aer=0.9, **kw)
    assert not ref.status.any() and ref.bounces[0] >= 2
    for I, bounces, ratio in ((lay.I[0], lay.bounces[0], lay.bounce_ratio[0]), (one.I, one.bounces, one.bounce_ratio),
                              (res["I"][0].cpu().numpy(), int(res["bounces"][0]), float(res["bounce_ratio"][0]))):
        assert np.array_equal(I, ref.I[0]) and bounces == ref.bounces[0] and ratio == ref.bounce_ratio[0]
    assert one.I_saved is None and one.n == ref.n[0]
