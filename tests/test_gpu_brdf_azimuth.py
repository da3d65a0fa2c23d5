"""Azimuth-resolved radiance over a BRDF ground on the device (csrc/brdf.hip, csrc/api_brdf.hip) through the C
ABI: the Fourier modes of the operator and of the beam row against the NumPy model of tests/brdf_azimuth_np.py, their refusals,
the device chain (mode solves with the series in ground reflections inside) against a direct azimuth-resolved solve over a
phi-resolved BRDF ground in the linear regime, and SOS_Aer_batch(..., brdf_modes=True) at natural scale against the model's mode
series run with the device's own order and reflection counts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import azimuth_direct as D
import brdf_azimuth_np as BA
import sos_oracle as O
from sosrt import _lib, inputs
from sosrt.main import SOS_Aer_batch
from test_gpu_azimuth import _close, _kind, _solver
from test_gpu_azimuth_direct import _accumulate
from test_gpu_brdf import dev, dfull, host, params_of, run_beam, run_operator, sync
from util import RTOL

pytestmark = pytest.mark.gpu

RPV = ("rpv", 0.2, 0.8, -0.1)
MU0S = (0.35, 0.6, 0.85)
SCALE = 1e-6
RANGES = lambda nphi: [(0, 1), (1, 8), (1, 9), (3, 17), (min(nphi - 2, _lib.MAX_MODES), 1)]     # (m_first, m_count)


def in_range(m_first, m_count, nphi):
    return m_first + m_count - 1 <= min(_lib.MAX_MODES, nphi - 2)


def grid_handle(N, B=3):
    """a handle with the grid and B black three-zone columns at MU0S (the builders read the grid; the beam rows' B is checked
    against the columns)"""
    L = 8
    s = _solver(L, N, B=B)
    iu, idn = inputs.slab_indices(120, 25, 17, L)
    s.set_columns(np.full(B, iu), np.full(B, idn), np.array(MU0S[:B]), 0.0, 1.0, 0.95, 0.124 / L, 0.3 / (idn + 1 - iu), 0.424)
    return s


def run_operator_modes(s, brdf, m_first, m_count, nphi, sign_odd=False):
    M1 = s.N - 1
    d_R = dfull((m_count, M1, M1))
    sync()
    kind, p = params_of(brdf)
    s.brdf_operator_modes_device(kind, d_R.data_ptr(), m_first, m_count, p, nphi, sign_odd=sign_odd)
    return np.swapaxes(host(d_R, s).reshape(m_count, M1, M1), 1, 2)          # [m, i, j], as the model writes it


def run_beam_modes(s, brdf, mu0, m_first, m_count, nphi):
    B = len(mu0)
    d_mu0, d_r0 = dev(mu0), dfull((m_count, B, s.N - 1))
    sync()
    kind, p = params_of(brdf)
    s.brdf_beam_modes_device(kind, d_mu0.data_ptr(), d_r0.data_ptr(), m_first, m_count, p, nphi, B=B)
    return host(d_r0, s).reshape(m_count, B, s.N - 1)


@functools.lru_cache(maxsize=None)
def model_modes(N, nphi, brdf=RPV):
    """(R^m [m, i, j], r0^m [m, b, i]) of the model for every mode a call may ask for at this nphi; never changed"""
    mu = O.make_mu(N)
    ms = list(range(min(_lib.MAX_MODES, nphi - 2) + 1))
    R = BA.operator_modes(mu, N, brdf, ms, nphi)
    r0 = np.stack([BA.beam_modes(mu, N, m0, brdf, ms, nphi) for m0 in MU0S], axis=1)
    R.setflags(write=False)
    r0.setflags(write=False)
    return R, r0


# ---- a. the mode builders against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nphi", [9, 65, 300])
@pytest.mark.parametrize("N", [37, 66])
def test_operator_and_beam_modes_against_the_model(N, nphi):
    """N - 1 = 36 is a partial wave, 65 one lane into a second; nphi = 300 crosses the 256-node chunk of the cosine tables; the
    ranges straddle the 8 modes of one launch (8 = one full launch, 9 and 17 = one mode into the next).  A range past
    min(SOSRT_MAX_MODES, nphi - 2) is refused and writes nothing."""
    s = grid_handle(N)
    R, r0 = model_modes(N, nphi)
    mxR, mx0 = np.max(np.abs(R[0])), np.max(np.abs(r0[0]))
    lib = _lib.lib()
    for m_first, m_count in RANGES(nphi):
        if not in_range(m_first, m_count, nphi):
            M1 = N - 1
            d_R, d_r0, d_mu0 = dfull((m_count, M1, M1), guard=5), dfull((m_count, 3, M1), guard=5), dev(MU0S)
            p = (ctypes.c_double * 3)(*RPV[1:])
            sync()
            assert lib.sosrt_brdf_operator_modes_dev(s._h, _lib.BRDF_RPV, p, 3, nphi, m_first, m_count, 0,
                                                     ctypes.c_void_p(d_R.data_ptr())) == _lib.E_INVALID
            assert b"modes" in lib.sosrt_last_error()
            assert lib.sosrt_brdf_beam_modes_dev(s._h, 3, _lib.BRDF_RPV, p, 3, nphi, m_first, m_count, ctypes.c_void_p(d_mu0.data_ptr()),
                                                 ctypes.c_void_p(d_r0.data_ptr())) == _lib.E_INVALID
            s.synchronize()
            sync()
            assert bool(torch.isnan(d_R).all()) and bool(torch.isnan(d_r0).all())
            continue
        sl = slice(m_first, m_first + m_count)
        got_R, got_r0 = run_operator_modes(s, RPV, m_first, m_count, nphi), run_beam_modes(s, RPV, MU0S, m_first, m_count, nphi)
        eR, e0 = np.max(np.abs(got_R - R[sl])) / mxR, np.max(np.abs(got_r0 - r0[sl])) / mx0
        print("N=%d nphi=%d modes %d..%d: operator %.3e of max |R^0|, beam rows %.3e of max |r0^0|"
              % (N, nphi, m_first, m_first + m_count - 1, eR, e0))
        assert np.all(np.isfinite(got_R)) and np.all(np.isfinite(got_r0)) and eR <= 1e-12 and e0 <= 1e-12
        # the sign is exact negation of the odd modes; the beam rows of a column do not depend on B
        sgn = np.array([(-1.0) ** m for m in range(m_first, m_first + m_count)])
        assert np.array_equal(run_operator_modes(s, RPV, m_first, m_count, nphi, sign_odd=True), sgn[:, None, None] * got_R)
        assert np.array_equal(run_beam_modes(s, RPV, MU0S[:1], m_first, m_count, nphi), got_r0[:, :1])
        if m_first == 0:                                     # mode 0: the bits of the azimuth-mean entry points
            assert np.array_equal(got_R[0], run_operator(s, RPV, nphi)) and np.array_equal(got_r0[0], run_beam(s, RPV, MU0S, nphi))
    s.close()


def test_lambertian_modes_on_the_device():
    s = grid_handle(37)
    for nphi in (9, 300):
        m_last = min(_lib.MAX_MODES, nphi - 2)
        R, r0 = run_operator_modes(s, "lambertian", 0, m_last + 1, nphi), run_beam_modes(s, "lambertian", MU0S, 0, m_last + 1, nphi)
        assert np.array_equal(R[0], run_operator(s, "lambertian", nphi)) and np.array_equal(r0[0], run_beam(s, "lambertian", MU0S, nphi))
        print("nphi=%d: Lambertian modes m >= 1: operator %.2e, beam rows %.2e" % (nphi, np.max(np.abs(R[1:])), np.max(np.abs(r0[1:]))))
        assert np.max(np.abs(R[1:])) <= 1e-15 and np.max(np.abs(r0[1:])) <= 1e-15
    s.close()


# ---- b. refusals: nothing is written ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    N, M1, G = 37, 36, 7
    s = grid_handle(N)
    lib = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    d_R, d_r0 = dfull((4, M1, M1), guard=G), dfull((4, 3, M1), guard=G)
    d_mu0 = dev(MU0S)
    rpv = (ctypes.c_double * 3)(0.2, 0.8, -0.1)
    P = lambda *v: (ctypes.c_double * 3)(*v)
    op = lambda kind, p, n, nphi, m1=1, mc=4, out=d_R: lib.sosrt_brdf_operator_modes_dev(s._h, kind, p, n, nphi, m1, mc, 1, vp(out))
    beam = lambda B, kind, p, n, nphi, m1=1, mc=4, mu0=d_mu0, out=d_r0: lib.sosrt_brdf_beam_modes_dev(s._h, B, kind, p, n, nphi, m1, mc,
                                                                                               vp(mu0), vp(out))
    LAM, RP = _lib.BRDF_LAMBERTIAN, _lib.BRDF_RPV
    calls = {
        "operator nphi": lambda: op(RP, rpv, 3, 2), "operator nphi large": lambda: op(RP, rpv, 3, 65538), "operator kind": lambda: op(7, None, 0, 65),
        "operator nparams": lambda: op(RP, rpv, 2, 65), "operator lambertian nparams": lambda: op(LAM, rpv, 3, 65),
        "operator rho0": lambda: op(RP, P(0.0, 0.8, -0.1), 3, 65), "operator k": lambda: op(RP, P(0.2, -1.0, 0.0), 3, 65),
        "operator theta": lambda: op(RP, P(0.2, 0.8, 1.0), 3, 65), "operator nan": lambda: op(RP, P(0.2, 0.8, np.nan), 3, 65),
        "operator null params": lambda: op(RP, None, 3, 65), "operator null out": lambda: op(LAM, None, 0, 65, 1, 4, None),
        "operator m_first < 0": lambda: op(RP, rpv, 3, 65, -1, 4), "operator m_count = 0": lambda: op(RP, rpv, 3, 65, 1, 0),
        "operator m_count < 0": lambda: op(RP, rpv, 3, 65, 1, -3), "operator past nphi - 2": lambda: op(RP, rpv, 3, 5, 1, 4),
        "operator past MAX_MODES": lambda: op(RP, rpv, 3, 300, 62, 4), "operator m_first past": lambda: op(RP, rpv, 3, 300, 65, 1),
        "operator overflow": lambda: op(RP, rpv, 3, 300, 2, 2 ** 31 - 1),
        "beam B=0": lambda: beam(0, LAM, None, 0, 65), "beam B=4": lambda: beam(4, LAM, None, 0, 65), "beam nphi": lambda: beam(3, LAM, None, 0, 1),
        "beam kind": lambda: beam(3, -1, None, 0, 65), "beam nparams": lambda: beam(3, RP, rpv, 1, 65), "beam theta": lambda: beam(3, RP, P(0.2, 0.8, -1.0), 3, 65),
        "beam null mu0": lambda: beam(3, LAM, None, 0, 65, 1, 4, None), "beam null out": lambda: beam(3, LAM, None, 0, 65, 1, 4, d_mu0, None),
        "beam m_first < 0": lambda: beam(3, RP, rpv, 3, 65, -2, 4), "beam m_count = 0": lambda: beam(3, RP, rpv, 3, 65, 1, 0),
        "beam past nphi - 2": lambda: beam(3, RP, rpv, 3, 5, 0, 5), "beam past MAX_MODES": lambda: beam(3, RP, rpv, 3, 300, 64, 2),
    }

    def untouched():
        s.synchronize()
        sync()
        return bool(torch.isnan(d_R).all()) and bool(torch.isnan(d_r0).all())

    for name, call in calls.items():
        rc = call()
        assert rc == _lib.E_INVALID and lib.sosrt_last_error(), name
        assert untouched(), name
    s.set_columns_single_slab([0.5, 0.6, 0.7], 0.9, 0.3)
    for name, call in {"operator": lambda: op(LAM, None, 0, 65), "beam": lambda: beam(3, LAM, None, 0, 65)}.items():
        assert call() == _lib.E_INVALID and b"single slab" in lib.sosrt_last_error(), name
        assert untouched(), name
    s.close()
    # a valid call writes its modes and leaves the guard elements behind them alone
    s = grid_handle(N)
    assert op(RP, rpv, 3, 65) == 0 and beam(3, RP, rpv, 3, 65) == 0
    s.synchronize()
    sync()
    assert bool(torch.isfinite(d_R[:4 * M1 * M1]).all()) and bool(torch.isnan(d_R[4 * M1 * M1:]).all())
    assert bool(torch.isfinite(d_r0[:4 * 3 * M1]).all()) and bool(torch.isnan(d_r0[4 * 3 * M1:]).all())
    s.close()


# ---- c. the device chain against the direct solve, linear regime ------------------------------------------------------------------------
def reflections(s, d_tau, d_I, d_R, d_r0, tol=1e-4, targets=None, max_bounces=32):
    """The series in ground reflections on the resident field d_I [1, L, 2N] (in place), through the C ABI as `solve_brdf` runs
    it: without `targets` until the term is below tol (mode 0), with them one reflection per entry at that order count.
    Returns the order counts and the worst status."""
    dv = d_tau.device
    B, L = d_tau.shape
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dv)
    d_S, d_G, d_Ik, d_ratio = f64(B, s.N - 1), f64(B, L, s.D), f64(B, L, s.D), f64(B)
    d_n, d_st, d_gst = (torch.zeros(B, dtype=torch.int32, device=dv) for _ in range(3))
    orders, worst, src = [], 0, d_I
    try:
        for k in range(1, (len(targets) if targets is not None else max_bounces) + 1):
            s.ground_source_device(src.data_ptr(), d_tau.data_ptr(), d_R.data_ptr(), d_S.data_ptr(), d_r0.data_ptr() if k == 1 else 0, 0, B=B)
            s.ground_first_order_device(d_tau.data_ptr(), d_S.data_ptr(), d_G.data_ptr(), d_gst.data_ptr(), B=B)
            if targets is not None:
                d_t = torch.tensor([targets[k - 1]] * B, dtype=torch.int32, device=dv)
                torch.cuda.synchronize()
                s.set_order_targets(d_t.data_ptr())
            s.solve_device(d_tau.data_ptr(), 0, 0, d_Ik.data_ptr(), tol=tol, d_I1=d_G.data_ptr(), d_n_orders=d_n.data_ptr(),
                           d_status=d_st.data_ptr())
            s.bounce_accumulate_device(d_Ik.data_ptr(), d_I.data_ptr(), d_ratio.data_ptr(), B=B)
            s.synchronize()
            orders.append(int(d_n[0].item()))
            worst = worst or int(d_st.max().item()) or int(d_gst.max().item())
            src = d_Ik
            if targets is None and float(d_ratio.max().item()) < tol:
                break
    finally:
        s.set_order_targets(None)
    return orders, worst


@pytest.mark.parametrize("L,N,nq,M", [(16, 24, 48, 10), (24, 37, 48, 6)])
def test_device_chain_against_the_direct_solve(L, N, nq, M):
    """Rayleigh + HG g = 0.5 over RPV (0.2, 0.8, -0.1), mu0 = 0.6, P0 and the beam rows scaled by 1e-6.  The mode-0 solve and its
    reflections run to tol = 1e-4 and give n and n_k; mode m runs n orders with (-1)^m P^m, then the reflections of n_k orders with
    (-1)^m R^m and r0^m; sosrt_azimuth_accumulate_dev synthesises; the direct solve (nothing of it goes through a mode) runs the
    same counts, and its own modes 0..M are the comparison, at RTOL."""
    nphi = nq // 2 + 1
    mu0 = np.array([0.6])
    dv = torch.device("cuda", 0)
    s = _solver(L, N, B=1, max_orders=200)
    try:
        ka, fa = _kind(s, "rayleigh")
        kr, fr = _kind(s, "hg", 0.5)
        iu, idn = inputs.slab_indices(120, 25, 17, L)
        tau = inputs.tau_profile(0.124, 0.3, 120, 25, 17, L)[None]
        s.set_columns(np.full(1, iu), np.full(1, idn), mu0, 0.0, 1.0, 0.95, 0.124 / L, 0.3 / (idn + 1 - iu), 0.424)
        d_tau, d_mu0 = dev(tau), dev(mu0)
        M1 = N - 1
        d_R, d_r0 = dfull((M + 1, M1, M1)).reshape(M + 1, M1, M1), dfull((M + 1, 1, M1)).reshape(M + 1, 1, M1)
        sync()
        s.brdf_operator_modes_device("rpv", d_R.data_ptr(), 0, M + 1, RPV[1:], nphi, sign_odd=True)
        s.brdf_beam_modes_device("rpv", d_mu0.data_ptr(), d_r0.data_ptr(), 0, M + 1, RPV[1:], nphi, B=1)
        s.synchronize()
        d_r0 *= SCALE
        sync()
        s.set_phase(s.phase_matrix(ka), s.phase_matrix(kr, 0.5))
        r = s.solve(tau, SCALE * s.phase_p0(ka, mu0), SCALE * s.phase_p0(kr, mu0, 0.5), tol=1e-4)
        assert r.status[0] == 0
        n = int(r.n[0])
        d_I = dev(r.I)
        n_k, st = reflections(s, d_tau, d_I, d_R[0], d_r0[0])
        assert st == 0 and 2 <= len(n_k) < 32
        Im = [host(d_I, s)[0]]
        Pa, Pr = s.phase_modes(ka, 1, M, nphi), s.phase_modes(kr, 1, M, nphi, 0.5)
        P0a, P0r = SCALE * s.phase_p0_modes(ka, mu0, 1, M, nphi), SCALE * s.phase_p0_modes(kr, mu0, 1, M, nphi, 0.5)
        d_n, d_st = (torch.zeros(1, dtype=torch.int32, device=dv) for _ in range(2))
        d_t = torch.tensor([n], dtype=torch.int32, device=dv)
        for m in range(1, M + 1):
            s.synchronize()
            s.set_phase((-1) ** m * Pa[m - 1], (-1) ** m * Pr[m - 1])
            d_a, d_r = dev(P0a[m - 1]), dev(P0r[m - 1])
            sync()
            s.set_order_targets(d_t.data_ptr())
            try:
                s.solve_device(d_tau.data_ptr(), d_a.data_ptr(), d_r.data_ptr(), d_I.data_ptr(), d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())
                s.synchronize()
            finally:
                s.set_order_targets(None)
            assert int(d_n[0].item()) == n and int(d_st[0].item()) == 0
            got_k, st = reflections(s, d_tau, d_I, d_R[m], d_r0[m], targets=n_k)
            assert got_k == n_k and st == 0
            Im.append(host(d_I, s)[0])
        Im = np.stack(Im)
        phi = 2 * np.pi * np.arange(nq) / nq
        got = _accumulate(s, Im, phi)
    finally:
        s.close()
    gr = BA.black_three_zone(0.6, L, N)
    log = BA.BlendLog()
    with D.record_blend() as oracle_log:
        _, Iq = BA.direct_solve(gr, fa, fr, RPV, nq, n, n_k, SCALE, log=log)
    log.oracle = oracle_log
    assert log.first_test_everywhere()
    ref = D.synthesize(D.project(Iq, M), phi)
    print("L=%d N=%d: n = %d, reflections %s, device chain vs the direct solve's modes %.3e of the maximum"
          % (L, N, n, n_k, np.max(np.abs(got - ref)) / np.max(np.abs(ref))))
    _close(got, ref, RTOL, "L = %d, N = %d, M = %d, n = %d, reflections %s" % (L, N, M, n, n_k))


# ---- d. the whole driver at natural scale -----------------------------------------------------------------------------------------------
M_DRIVER = 6
PHI = 2 * np.pi * np.arange(2 * M_DRIVER + 2) / (2 * M_DRIVER + 2)          # phi = 0 is node 0, phi = pi node M + 1


@functools.lru_cache(maxsize=None)
def driver(L, N, brdf, brdf_modes=True, azimuths=True, grd_alb=1.0, surface="brdf"):
    kw = dict(alb_aer=0.95, nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.5, max_orders=64)
    if surface == "brdf":
        kw.update(surface="brdf", brdf=brdf)
    if azimuths:
        kw.update(azimuths=PHI, n_modes=M_DRIVER)
    if brdf_modes:
        kw.update(brdf_modes=True)
    return SOS_Aer_batch(list(MU0S), 0.3, grd_alb, **kw)


@pytest.mark.parametrize("L,N", [(30, 64), (24, 66)])
def test_driver_against_the_model_series(L, N):
    r, plain = driver(L, N, RPV), driver(L, N, RPV, brdf_modes=False, azimuths=False)
    assert r.mode_status.shape == (M_DRIVER + 1, 3) and not r.mode_status.any()
    assert r.bounce_orders.shape == (int(r.bounces.max()), 3) and plain.I_azimuth is None
    assert np.array_equal(r.I, plain.I) and np.array_equal(r.n, plain.n) and np.array_equal(r.bounces, plain.bounces)
    assert np.array_equal(r.status, plain.status) and np.array_equal(r.bounce_ratio, plain.bounce_ratio)
    assert np.array_equal(r.bounce_orders, plain.bounce_orders)
    # the mean over 2M + 2 uniform azimuths is mode 0
    mean = r.I_azimuth.mean(axis=-1)
    assert np.max(np.abs(mean - r.I[:, [0, L - 1]])) <= 1e-12 * np.max(np.abs(r.I))
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    for b, mu0 in enumerate(MU0S):
        gr = BA.black_three_zone(mu0, L, N)
        with np.errstate(all="ignore"):
            Im, status = BA.mode_series(gr, fa, fr, RPV, M_DRIVER, 25, int(r.n[b]), r.bounce_orders[:, b])
        ref = D.synthesize(Im[:, [0, L - 1]], PHI)
        err = np.max(np.abs(r.I_azimuth[b] - ref)) / np.max(np.abs(ref))
        print("L=%d N=%d mu0=%.2f: n = %d, reflections %s, I_azimuth vs the model's mode series %.3e of the maximum"
              % (L, N, mu0, r.n[b], r.bounce_orders[:, b], err))
        assert status == 0
        _close(r.I_azimuth[b], ref, RTOL, "mu0 = %g" % mu0)


def test_lambertian_ground_is_mode_zero_plus_the_atmosphere():
    """A Lambertian ground has no mode m >= 1: I_azimuth is the ground's mode 0 plus the atmosphere's modes over a black ground,
    which the specular machinery gives at grd_alb = 0."""
    L, N = 24, 66
    r = driver(L, N, "lambertian", grd_alb=(0.1, 0.3, 0.5))
    black = driver(L, N, None, brdf_modes=False, grd_alb=0.0, surface="specular")
    assert not r.mode_status.any() and np.array_equal(r.n, black.n)
    ref = black.I_azimuth + (r.I - black.I)[:, [0, L - 1], :, None]
    assert np.max(np.abs(r.I - black.I)) > 1e-3 * np.max(r.I)
    assert np.max(np.abs(r.I_azimuth - ref)) <= 1e-12 * np.max(np.abs(ref))


def test_the_hot_spot_reaches_the_result():
    """RPV at TOA, on the upward lane nearest mu0: back-scatter (phi = 0) minus forward (phi = pi) is larger over the BRDF's modes
    than the atmosphere alone gives -- the hot spot of the ground, which only the modes m >= 1 of the BRDF carry."""
    L, N = 30, 64
    r = driver(L, N, RPV)
    black = driver(L, N, None, brdf_modes=False, grd_alb=0.0, surface="specular")
    for b, mu0 in enumerate(MU0S):
        lane = N + int(np.argmin(np.abs(r.mu[N:] - mu0)))
        with_ground = r.I_azimuth[b, 0, lane, 0] - r.I_azimuth[b, 0, lane, M_DRIVER + 1]
        atmosphere = black.I_azimuth[b, 0, lane, 0] - black.I_azimuth[b, 0, lane, M_DRIVER + 1]
        print("mu0=%.2f lane mu=%.4f: I(0) - I(pi) at TOA %.6e over RPV, %.6e over a black ground" % (mu0, r.mu[lane], with_ground, atmosphere))
        assert with_ground > atmosphere


# ---- e. natural scale against the direct solve: recorded ------------------------------------------------------------------------------
# The model alone (tests/brdf_azimuth_np.py: mode series against direct solve, both at natural scale with the oracle's own counts
# n = 12 and 5 reflections of 13 orders, this column, modes 0..6 of both, TOA and surface rows) differs by 1.242e-1 of the rows'
# maximum on the CPU, with the direct solve on 24 nodes (48 nodes: 1.00e-1; at L = 24, N = 37: 3.4e-1): the blend's field-dependent
# stopping row per mode and per reflection (DESIGN sections 11, 20), which grows as the grid coarsens, and the 13-node quadrature
# of the hot spot in the direct solve.  The bound is twice that figure; the case is a record, not a rounding-level check.
MODEL_NATURAL = 1.242e-1


def test_natural_scale_against_the_direct_solve():
    L, N, b = 30, 64, 1
    r = driver(L, N, RPV)
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    with np.errstate(all="ignore"):
        _, Iq = BA.direct_solve(BA.black_three_zone(MU0S[b], L, N), fa, fr, RPV, 24, int(r.n[b]), r.bounce_orders[:, b])
    ref = D.synthesize(D.project(Iq, M_DRIVER)[:, [0, L - 1]], PHI)
    err = np.max(np.abs(r.I_azimuth[b] - ref)) / np.max(np.abs(ref))
    print("natural scale, mu0 = %.2f: I_azimuth vs the direct solve %.3e of the rows' maximum" % (MU0S[b], err))
    assert err <= 2 * MODEL_NATURAL
