"""Ross-Li ground on the device (csrc/brdf.hip, csrc/api_brdf.hip): the two kernels through every builder
against the NumPy model of tests/ross_li_np.py, the two terms kernels against the model and their bit rules, the driver against
the model's series with every column's own weights, Ross-Li (a, 0, 0) bit for bit against the Lambertian ground, the device
chain over the ground's modes against a direct azimuth-resolved solve in the linear regime, the view drivers against the model's
mode series, the albedos, every refusal, and the default path's bytes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import azimuth_direct as D
import brdf_azimuth_np as BA
import brdf_np as G
import brdf_view_np as BV
import ross_li_np as RL
import sos_oracle as O
import view_azimuth_np as VA
import view_np as VN
from sosrt import _lib, inputs
from sosrt.main import SOS_Aer_batch
from test_gpu_azimuth import _close, _kind, _solver
from test_gpu_azimuth_direct import _accumulate
from test_gpu_brdf import SHAPES, columns, dev, dfull, handle, host, run_beam, run_operator, run_source, sample_field, sync
from test_gpu_brdf_azimuth import run_beam_modes, run_operator_modes
from test_gpu_brdf_view import grid_handle, run_view_beam, run_view_ground, run_view_rows, view_cosines
from util import RTOL

pytestmark = pytest.mark.gpu

MU0S = (0.35, 0.6, 0.85)
WEIGHTS = np.array([[0.05, 0.0, 0.0], [0.30, 0.15, 0.04], [0.10, 0.60, 0.02]])      # [b, k]: f_iso, f_vol, f_geo of the columns
ROSS_LI = ("ross_li", 0.30, 0.15, 0.04)
KINDS = ("ross_thick", "li_sparse_r")
SCALE = 1e-6


def mx(a):
    return np.max(np.abs(a))


# ---- 1. the builders against the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu_floor", [RL.MU_FLOOR, 0.0], ids=["floor80", "floor0"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [n for _, n in SHAPES])
def test_builders_against_the_model(N, kind, mu_floor):
    """All four layouts, modes 0..9 (a launch of 8 and a remainder of 2) on 65 and 301 azimuth nodes (301: the chunked cosine
    table), to 1e-12 of the array's maximum magnitude -- the kernels cross zero.  Then the builders' bit guarantees."""
    brdf = (kind, mu_floor)
    s = grid_handle(N)
    mu = O.make_mu(N)
    mv, nodes = view_cosines(N, 17)
    off = len(mv) - len(nodes)
    ms = list(range(10))
    for nphi in (65, 301):
        R = BA.operator_modes(mu, N, brdf, ms, nphi)
        r0 = np.stack([BA.beam_modes(mu, N, m0, brdf, ms, nphi) for m0 in MU0S], axis=1)
        Rv = BV.view_rows_modes(mu, N, mv, brdf, ms, nphi)
        r0v = np.stack([BV.view_beam_modes(mv, m0, brdf, ms, nphi) for m0 in MU0S], axis=1)
        got = (run_operator_modes(s, brdf, 0, 10, nphi), run_beam_modes(s, brdf, MU0S, 0, 10, nphi),
               run_view_rows(s, brdf, mv, 0, 10, nphi), run_view_beam(s, brdf, MU0S, mv, 0, 10, nphi))
        err = [mx(g - r) / mx(r) for g, r in zip(got, (R, r0, Rv, r0v))]
        print("N=%d %s mu_floor=%.4f nphi=%d: operator %.2e, beam rows %.2e, view rows %.2e, view beam rows %.2e of their maxima"
              % ((N, kind, mu_floor, nphi) + tuple(err)))
        assert all(np.all(np.isfinite(g)) for g in got) and max(err) <= 1e-12
        # mode 0 through the modes entry: the bits of the azimuth-mean entry; the azimuth-mean entries against the model
        op, beam = run_operator(s, brdf, nphi), run_beam(s, brdf, MU0S, nphi)
        assert np.array_equal(got[0][0], op) and np.array_equal(got[1][0], beam)
        assert mx(op - G.operator(mu, N, brdf, nphi)) <= 1e-12 * mx(R[0]) and mx(beam - r0[0]) <= 1e-12 * mx(r0[0])
        # one mode alone, and a range that starts elsewhere: the same bits as inside the launch of many
        for m in (0, 3, 8, 9):
            assert np.array_equal(run_operator_modes(s, brdf, m, 1, nphi)[0], got[0][m])
            assert np.array_equal(run_beam_modes(s, brdf, MU0S, m, 1, nphi)[0], got[1][m])
            assert np.array_equal(run_view_rows(s, brdf, mv, m, 1, nphi)[0], got[2][m])
            assert np.array_equal(run_view_beam(s, brdf, MU0S, mv, m, 1, nphi)[0], got[3][m])
        assert np.array_equal(run_operator_modes(s, brdf, 2, 5, nphi), got[0][2:7])
        # a view cosine at a node: the node's bits; a beam row's bits do not depend on B; the sign is exact
        assert np.array_equal(got[2][:, off:], got[0][:, nodes]) and np.array_equal(got[3][:, :, off:], got[1][:, :, nodes])
        assert np.array_equal(run_beam_modes(s, brdf, MU0S[:1], 0, 10, nphi), got[1][:, :1])
        assert np.array_equal(run_view_beam(s, brdf, MU0S[:1], mv, 0, 10, nphi), got[3][:, :1])
        sgn = np.array([(-1.0) ** m for m in ms])[:, None, None]
        assert np.array_equal(run_operator_modes(s, brdf, 0, 10, nphi, sign_odd=True), sgn * got[0])
    # the value at an azimuth itself, the back-scatter pairs mu_view = mu0, phi = 0 among them
    phi = np.array([0.0, 1e-9, 0.3, np.pi / 2, 2.0, np.pi, 4.0, 2 * np.pi, -0.3])
    d_mu0, d_phi, d_out = dev(MU0S), dev(phi), dfull((len(phi), 3, len(mv)), guard=4)
    sync()
    s.brdf_view_beam_azimuth_device(kind, d_mu0.data_ptr(), mv, d_phi.data_ptr(), len(phi), d_out.data_ptr(), (mu_floor,), B=3)
    out = host(d_out, s)
    at = out[:-4].reshape(len(phi), 3, len(mv))
    ref = np.stack([BV.view_beam_azimuth(mv, m0, brdf, phi) for m0 in MU0S], axis=1)
    print("N=%d %s mu_floor=%.4f: values at azimuths %.2e of their maximum" % (N, kind, mu_floor, mx(at - ref) / mx(ref)))
    assert np.all(np.isnan(out[-4:])) and np.all(np.isfinite(at)) and mx(at - ref) <= 1e-12 * mx(ref)
    s.close()


# ---- 2. the terms kernels against the model, and their bit rules ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_terms(N, mu_floor=RL.MU_FLOOR):
    """(Rs [K, i, j], r0s [K, b, i]) of the model for the three terms of a Ross-Li ground; never changed"""
    mu = O.make_mu(N)
    Rs = np.stack([G.operator(mu, N, t) for t in RL.terms(mu_floor)])
    r0s = np.stack([np.stack([G.beam_row(mu, N, m0, t) for m0 in MU0S]) for t in RL.terms(mu_floor)])
    Rs.setflags(write=False)
    r0s.setflags(write=False)
    return Rs, r0s


def run_source_terms(s, I, tau, Rs, weight, r0s=None):
    """S [B, N-1] of sosrt_ground_source_terms_dev; Rs [K, i, j] as the model writes it, r0s [K, B, i], weight [B, K]"""
    B, K = tau.shape[0], len(Rs)
    d = [dev(I), dev(tau), dev(np.swapaxes(Rs, 1, 2)), dev(weight)]
    d_r0 = None if r0s is None else dev(r0s)
    d_S = dfull((B, s.N - 1), guard=3)
    sync()
    s.ground_source_terms_device(K, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_S.data_ptr(),
                                 0 if d_r0 is None else d_r0.data_ptr(), B=B)
    S = host(d_S, s)
    assert np.all(np.isnan(S[-3:])) and np.array_equal(host(d[0], s), I) and np.array_equal(host(d[3], s), weight)
    return S[:-3].reshape(B, s.N - 1)


def plus_zero(a):
    return not np.any(a) and not np.any(np.signbit(a))


@pytest.mark.parametrize("L,N", SHAPES)
def test_ground_source_terms_against_the_model(L, N):
    cols = columns(L, N)
    s, tau = handle(cols)
    I = np.array(sample_field(L, N))
    Rs, r0s = model_terms(N)
    for use_r0 in (True, False):
        beam = r0s if use_r0 else None
        got = run_source_terms(s, I, tau, Rs, WEIGHTS, beam)
        ref = np.stack([RL.ground_source_terms(Rs, I[b, -1], None if beam is None else beam[:, b], tau[b, -1], MU0S[b], WEIGHTS[b])
                        for b in range(3)])
        err = mx(got - ref) / mx(ref)
        print("L=%d N=%d beam %s: ground source over 3 terms %.3e of its maximum" % (L, N, use_r0, err))
        assert err <= 1e-13
        # K = 1: the bits of the single-term kernel with scale = weight
        for k in range(3):
            one = run_source_terms(s, I, tau, Rs[k:k + 1], WEIGHTS[:, k:k + 1].copy(), None if beam is None else beam[k:k + 1])
            assert np.array_equal(one, run_source(s, I, tau, Rs[k], None if beam is None else beam[k], WEIGHTS[:, k].copy())), k
        # a term of weight 0 leaves the bits alone: wherever it stands among the terms, and up to SOSRT_BRDF_MAX_TERMS terms
        two = run_source_terms(s, I, tau, Rs[[0, 2]], np.ascontiguousarray(WEIGHTS[:, [0, 2]]), None if beam is None else beam[[0, 2]])
        w0 = WEIGHTS.copy()
        w0[:, 1] = 0
        assert np.array_equal(run_source_terms(s, I, tau, Rs, w0, beam), two)
        four = np.concatenate((Rs[[1]], Rs)), np.concatenate((np.zeros((3, 1)), WEIGHTS), axis=1)
        assert np.array_equal(run_source_terms(s, I, tau, four[0], four[1], None if beam is None else np.concatenate((beam[[1]], beam))), got)
        assert np.array_equal(got[0], run_source(s, I, tau, Rs[0], None if beam is None else beam[0], WEIGHTS[:, 0].copy())[0])
        # all weights 0: exact +0; a column's bits do not depend on B
        wz = WEIGHTS.copy()
        wz[1] = 0
        z = run_source_terms(s, I, tau, Rs, wz, beam)
        assert plus_zero(z[1]) and np.array_equal(z[[0, 2]], got[[0, 2]])
        alone = run_source_terms(s, I[1:2], tau[1:2], Rs, WEIGHTS[1:2].copy(), None if beam is None else beam[:, 1:2].copy())
        # (the handle's column 0 carries another mu0 than the batch's column 1: without the beam term the source does not read it)
        if not use_r0:
            assert np.array_equal(alone[0], got[1])
        first = run_source_terms(s, I[:1], tau[:1], Rs, WEIGHTS[:1].copy(), None if beam is None else beam[:, :1].copy())
        assert np.array_equal(first[0], got[0])
    s.close()


def run_view_ground_terms(s, mv, tau, levels, weight, I=None, Rvs=None, r0vs=None, out0=None):
    """(out [B, nlev, 2V], S [B, V]) of sosrt_view_ground_terms_dev; Rvs [K, v, j] as the model writes it, r0vs [K, B, v]"""
    B, V, nlev = tau.shape[0], len(mv), len(levels)
    d_tau, d_w = dev(tau), dev(weight)
    d_I, d_Rv = (None, None) if I is None else (dev(I), dev(np.swapaxes(Rvs, 1, 2)))
    d_r0v = None if r0vs is None else dev(r0vs)
    d_out = dfull((B, nlev, 2 * V), guard=6) if out0 is None else torch.cat((dev(out0).reshape(-1), dfull((6,))))
    d_S = dfull((B, V), guard=2)
    sync()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    s.view_ground_terms_device(weight.shape[1], mv, d_tau.data_ptr(), levels, d_w.data_ptr(), d_out.data_ptr(), d_I=ptr(d_I),
                               d_Rv=ptr(d_Rv), d_r0v=ptr(d_r0v), accumulate=out0 is not None, d_S_out=d_S.data_ptr(), B=B)
    out, S = host(d_out, s), host(d_S, s)
    assert np.all(np.isnan(out[-6:])) and np.all(np.isnan(S[-2:]))
    return out[:-6].reshape(B, nlev, 2 * V), S[:-2].reshape(B, V)


@pytest.mark.parametrize("V", [1, 17])
@pytest.mark.parametrize("L,N", SHAPES)
def test_view_ground_terms_against_the_model(L, N, V):
    cols = columns(L, N)
    s, tau = handle(cols)
    mu = cols[0].mu
    I = np.array(sample_field(L, N))
    mv, nodes = view_cosines(N, V)
    off = V - len(nodes)
    Rvs = np.stack([BV.view_rows(mu, N, mv, t) for t in RL.terms()])
    r0vs = np.stack([np.stack([BV.view_beam_row(mv, m0, t) for m0 in MU0S]) for t in RL.terms()])
    levels = [0, L - 1, L // 2, 1, 0]
    for use_I, use_r0 in ((True, True), (True, False), (False, True)):
        kw = dict(I=I if use_I else None, Rvs=Rvs if use_I else None, r0vs=r0vs if use_r0 else None)
        got, S = run_view_ground_terms(s, mv, tau, levels, WEIGHTS, **kw)
        Sref = np.stack([RL.ground_source_terms(Rvs, I[b, -1] if use_I else np.zeros(2 * N), r0vs[:, b] if use_r0 else None, tau[b, -1],
                                                MU0S[b], WEIGHTS[b]) for b in range(3)])
        ref = np.stack([BV.view_ground(Sref[b], tau[b], mv)[levels] for b in range(3)])
        eS, eG = mx(S - Sref) / mx(Sref), mx(got - ref) / mx(ref)
        print("L=%d N=%d V=%d field %s beam %s: source %.3e, radiance %.3e of their maxima" % (L, N, V, use_I, use_r0, eS, eG))
        assert eS <= 1e-13 and eG <= 1e-13
        assert plus_zero(got[:, :, :V]) and np.array_equal(got[:, 1, V:], S)
        # K = 1: the bits of the single-term kernel with scale = weight
        for k in range(3):
            one, S1 = run_view_ground_terms(s, mv, tau, levels, WEIGHTS[:, k:k + 1].copy(), I=kw["I"], Rvs=Rvs[k:k + 1] if use_I else None,
                                            r0vs=r0vs[k:k + 1] if use_r0 else None)
            old, So = run_view_ground(s, mv, tau, levels, I=kw["I"], Rv=Rvs[k] if use_I else None, r0v=r0vs[k] if use_r0 else None,
                                      scale=WEIGHTS[:, k].copy())
            assert np.array_equal(one, old) and np.array_equal(S1, So), k
        # a term of weight 0 leaves the bits alone; all weights 0: exact +0; a column's bits do not depend on B
        w0 = WEIGHTS.copy()
        w0[:, 1] = 0
        two, S2 = run_view_ground_terms(s, mv, tau, levels, np.ascontiguousarray(WEIGHTS[:, [0, 2]]), I=kw["I"],
                                        Rvs=Rvs[[0, 2]] if use_I else None, r0vs=r0vs[[0, 2]] if use_r0 else None)
        z, Sz = run_view_ground_terms(s, mv, tau, levels, w0, **kw)
        assert np.array_equal(z, two) and np.array_equal(Sz, S2)
        wz = WEIGHTS.copy()
        wz[1] = 0
        z, Sz = run_view_ground_terms(s, mv, tau, levels, wz, **kw)
        assert plus_zero(z[1]) and plus_zero(Sz[1]) and np.array_equal(z[[0, 2]], got[[0, 2]])
        first, S1 = run_view_ground_terms(s, mv, tau[:1], levels, WEIGHTS[:1].copy(), I=None if not use_I else I[:1], Rvs=kw["Rvs"],
                                          r0vs=None if not use_r0 else r0vs[:, :1].copy())
        assert np.array_equal(first[0], got[0]) and np.array_equal(S1[0], S[0])
        if len(nodes) and use_I:                             # at a node: the bits of the grid's terms kernel
            Rs = np.stack([run_operator(s, t) for t in RL.terms()])
            r0s = np.stack([run_beam(s, t, MU0S) for t in RL.terms()])
            Rn = np.stack([run_view_rows(s, t, mv, 0, 1, 65)[0] for t in RL.terms()])
            r0n = np.stack([run_view_beam(s, t, MU0S, mv, 0, 1, 65)[0] for t in RL.terms()])
            _, Sn = run_view_ground_terms(s, mv, tau, levels, WEIGHTS, I=I, Rvs=Rn, r0vs=r0n if use_r0 else None)
            Sg = run_source_terms(s, I, tau, Rs, WEIGHTS, r0s if use_r0 else None)
            assert np.array_equal(Sn[:, off:], Sg[:, nodes])
    base = np.random.default_rng(7).random((3, len(levels), 2 * V))
    wrote, _ = run_view_ground_terms(s, mv, tau, levels, WEIGHTS, I=I, Rvs=Rvs)
    acc, _ = run_view_ground_terms(s, mv, tau, levels, WEIGHTS, I=I, Rvs=Rvs, out0=base)
    assert np.array_equal(acc[:, :, V:], base[:, :, V:] + wrote[:, :, V:]) and np.array_equal(acc[:, :, :V], base[:, :, :V])
    s.close()


# ---- 3. the driver against the model's series --------------------------------------------------------------------------------------------
def ross_li_of(weights, *floor):
    return ("ross_li",) + tuple(list(weights[:, k]) for k in range(3)) + floor


def driver(L, N, brdf, grd_alb=1.0, **kw):
    cols = columns(L, N)
    c = cols[0]
    return SOS_Aer_batch(list(MU0S), 0.3, grd_alb, tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.9, nb_layers=L, nb_angles=N,
                         P_atm=c.P_atm, P_aer=c.P_aer, P0_atm=np.stack([x.P0_atm for x in cols]), P0_aer=np.stack([x.P0_aer for x in cols]),
                         max_orders=64, surface="brdf", brdf=brdf, **kw)


@functools.lru_cache(maxsize=None)
def model_series(L, N):
    Rs, r0s = model_terms(N)
    R_b = np.tensordot(WEIGHTS, Rs, axes=1)                   # [b, i, j]
    r0_b = np.einsum("bk,kbi->bi", WEIGHTS, r0s)
    with np.errstate(all="ignore"):
        out = RL.bounce_solve_columns(O, columns(L, N), R_b, r0_b)
    out[0].setflags(write=False)
    return out


@pytest.mark.parametrize("L,N", [(30, 64), (24, 66)])
def test_driver_against_the_model_series(L, N):
    """mu0 = (0.35, 0.6, 0.85), every column its own weights (an isotropic ground among them), the default floor: equal bounce
    counts and status, the field within RTOL of its maximum.  The CPU model alone gives status 0 and 3 / 4 / 4 bounces."""
    ref, bounces, ratio, status = model_series(L, N)
    r = driver(L, N, ross_li_of(WEIGHTS), raise_on_error=False)
    err = [float(mx(r.I[b] - ref[b]) / mx(ref[b])) for b in range(3)]
    print("L=%d N=%d: bounces %s (model %s), status %s, field vs the model's series %s of the maximum, ratios %s"
          % (L, N, r.bounces, bounces, r.status, ["%.2e" % e for e in err], r.bounce_ratio))
    assert np.all(np.isfinite(r.I))
    assert np.array_equal(r.bounces, bounces) and np.array_equal(r.status, status) and not status.any()
    assert list(bounces) == [3, 4, 4]
    assert max(err) <= RTOL
    assert np.all(np.abs(r.bounce_ratio - ratio) <= 1e-6 * np.maximum(ratio, 1e-12))


# ---- 4. Ross-Li (a, 0, 0) is the Lambertian ground, bit for bit ------------------------------------------------------------------------------
ALB = [0.0, 0.3, 0.8]
PHI = 2 * np.pi * np.arange(14) / 14
KW = dict(alb_aer=0.95, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.5, max_orders=64)
SERIES = ("I", "n", "status", "bounces", "bounce_orders", "bounce_ratio")


def pair(L, N, **kw):
    a = SOS_Aer_batch(list(MU0S), 0.3, 1.0, nb_layers=L, nb_angles=N, surface="brdf", brdf=("ross_li", ALB, 0.0, 0.0), **KW, **kw)
    b = SOS_Aer_batch(list(MU0S), 0.3, ALB, nb_layers=L, nb_angles=N, surface="brdf", brdf="lambertian", **KW, **kw)
    return a, b


def same(a, b, names):
    for k in names:
        assert getattr(a, k) is not None and np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("L,N", [(30, 64), (24, 66)])
def test_isotropic_ross_li_is_the_lambertian_ground(L, N):
    a, b = pair(L, N)
    same(a, b, SERIES)
    assert b.bounces.max() >= 2 and b.black_sky_albedo is None and b.white_sky_albedo is None
    # (the grid's trapezoid starts at the first node above mu = 0: the albedo of a Lambertian ground a is a (1 - mu_1^2) on it)
    on_grid = np.array(ALB) * np.sum(RL.up_weights(O.make_mu(N), N))
    assert a.black_sky_albedo.shape == (3,) and np.max(np.abs(a.black_sky_albedo - on_grid)) <= 1e-13
    assert np.max(np.abs(a.white_sky_albedo - on_grid * np.sum(RL.up_weights(O.make_mu(N), N)))) <= 1e-13


def test_isotropic_ross_li_is_the_lambertian_ground_over_the_modes():
    a, b = pair(24, 66, azimuths=PHI, n_modes=6, brdf_modes=True)
    same(a, b, SERIES + ("I_azimuth", "mode_status"))


@pytest.mark.parametrize("first", [None, "exact", "modes"])
def test_isotropic_ross_li_is_the_lambertian_ground_at_the_view_lanes(first):
    L = 24
    kw = dict(view_mu=[0.123, 0.35, 0.6, 1.0], view_levels=(0, L // 3, -1), brdf_view=True)
    if first:
        kw.update(view_azimuths=PHI, n_modes=6, view_first_order=first)
    a, b = pair(L, 66, **kw)
    same(a, b, SERIES + ("I_view", "I_view_first", "I_view_scattered", "I_view_ground"))
    if first:
        same(a, b, ("I_view_azimuth", "I_view_azimuth_first", "I_view_azimuth_scattered", "I_view_azimuth_ground", "view_mode_status"))


# ---- 5. the linear regime against a direct azimuth-resolved solve; the view drivers against the model's mode series ----------------------------
def reflections_terms(s, d_tau, d_I, d_R, d_r0, d_w, tol=1e-4, targets=None, max_bounces=32):
    """test_gpu_brdf_azimuth.reflections with the terms kernel: d_R [K, N-1, N-1], d_r0 [K, 1, N-1], d_w [1, K]"""
    dv = d_tau.device
    B, L = d_tau.shape
    K = d_w.shape[1]
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dv)
    d_S, d_G, d_Ik, d_ratio = f64(B, s.N - 1), f64(B, L, s.D), f64(B, L, s.D), f64(B)
    d_n, d_st, d_gst = (torch.zeros(B, dtype=torch.int32, device=dv) for _ in range(3))
    orders, worst, src = [], 0, d_I
    try:
        for k in range(1, (len(targets) if targets is not None else max_bounces) + 1):
            s.ground_source_terms_device(K, src.data_ptr(), d_tau.data_ptr(), d_R.data_ptr(), d_w.data_ptr(), d_S.data_ptr(),
                                         d_r0.data_ptr() if k == 1 else 0, B=B)
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
    """test_gpu_brdf_azimuth's case with the Ross-Li ground of weights (0.30, 0.15, 0.04) in place of RPV, the ground source by the
    terms kernel: Rayleigh + HG g = 0.5, mu0 = 0.6, P0 and the beam rows scaled by 1e-6; the direct solve over rho(a, b, phi) itself
    runs the same counts and its modes 0..M are the comparison, at RTOL -- the bound of the RPV case."""
    nphi = nq // 2 + 1
    mu0 = np.array([0.6])
    dv = torch.device("cuda", 0)
    terms = RL.terms()
    s = _solver(L, N, B=1, max_orders=200)
    try:
        ka, fa = _kind(s, "rayleigh")
        kr, fr = _kind(s, "hg", 0.5)
        iu, idn = inputs.slab_indices(120, 25, 17, L)
        tau = inputs.tau_profile(0.124, 0.3, 120, 25, 17, L)[None]
        s.set_columns(np.full(1, iu), np.full(1, idn), mu0, 0.0, 1.0, 0.95, 0.124 / L, 0.3 / (idn + 1 - iu), 0.424)
        d_tau, d_mu0, d_w = dev(tau), dev(mu0), dev(np.array([ROSS_LI[1:]]))
        M1 = N - 1
        d_R = torch.empty((M + 1, 3, M1, M1), dtype=torch.float64, device=dv)
        d_r0 = torch.empty((M + 1, 3, 1, M1), dtype=torch.float64, device=dv)
        for k, t in enumerate(terms):
            kind, p = ("lambertian", ()) if t == "lambertian" else (t[0], t[1:])
            d_a, d_b = torch.empty((M + 1, M1, M1), dtype=torch.float64, device=dv), torch.empty((M + 1, 1, M1), dtype=torch.float64, device=dv)
            sync()
            s.brdf_operator_modes_device(kind, d_a.data_ptr(), 0, M + 1, p, nphi, sign_odd=True)
            s.brdf_beam_modes_device(kind, d_mu0.data_ptr(), d_b.data_ptr(), 0, M + 1, p, nphi, B=1)
            s.synchronize()
            d_R[:, k], d_r0[:, k] = d_a, d_b
        d_r0 *= SCALE
        sync()
        s.set_phase(s.phase_matrix(ka), s.phase_matrix(kr, 0.5))
        r = s.solve(tau, SCALE * s.phase_p0(ka, mu0), SCALE * s.phase_p0(kr, mu0, 0.5), tol=1e-4)
        assert r.status[0] == 0
        n = int(r.n[0])
        d_I = dev(r.I)
        n_k, st = reflections_terms(s, d_tau, d_I, d_R[0], d_r0[0], d_w)
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
            got_k, st = reflections_terms(s, d_tau, d_I, d_R[m], d_r0[m], d_w, targets=n_k)
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
        _, Iq = BA.direct_solve(gr, fa, fr, ROSS_LI, nq, n, n_k, SCALE, log=log)
    log.oracle = oracle_log
    assert log.first_test_everywhere()
    ref = D.synthesize(D.project(Iq, M), phi)
    print("L=%d N=%d: n = %d, reflections %s, device chain vs the direct solve's modes %.3e of the maximum"
          % (L, N, n, n_k, mx(got - ref) / mx(ref)))
    _close(got, ref, RTOL, "L = %d, N = %d, M = %d, n = %d, reflections %s" % (L, N, M, n, n_k))


M_DRIVER = 6
MU_VIEW = np.array([0.01, 0.123, 0.35, 0.6, 1.0])


def test_modes_driver_against_the_model_series():
    """SOS_Aer_batch(azimuths, brdf_modes) over Ross-Li at natural scale against the model's mode series over rho itself, run with
    the device's own order and reflection counts: RTOL, the bound of the RPV case"""
    L, N = 24, 66
    kw = dict(KW, nb_layers=L, nb_angles=N, surface="brdf", brdf=ROSS_LI)
    r = SOS_Aer_batch(list(MU0S), 0.3, 1.0, azimuths=PHI, n_modes=M_DRIVER, brdf_modes=True, **kw)
    plain = SOS_Aer_batch(list(MU0S), 0.3, 1.0, **kw)
    same(r, plain, SERIES)
    assert not r.mode_status.any()
    assert mx(r.I_azimuth.mean(axis=-1) - r.I[:, [0, L - 1]]) <= 1e-12 * mx(r.I)
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    for b, mu0 in enumerate(MU0S):
        with np.errstate(all="ignore"):
            Im, status = BA.mode_series(BA.black_three_zone(mu0, L, N), fa, fr, ROSS_LI, M_DRIVER, 25, int(r.n[b]), r.bounce_orders[:, b])
        ref = D.synthesize(Im[:, [0, L - 1]], PHI)
        print("mu0=%.2f: n = %d, reflections %s, I_azimuth vs the model's mode series %.3e of the maximum"
              % (mu0, r.n[b], r.bounce_orders[:, b], mx(r.I_azimuth[b] - ref) / mx(ref)))
        assert status == 0
        _close(r.I_azimuth[b], ref, RTOL, "mu0 = %g" % mu0)


@pytest.mark.parametrize("first", ["exact", "modes"])
def test_view_azimuth_driver_against_the_model_series(first):
    """test_gpu_brdf_view's case over Ross-Li: the scattered and the ground's term at (view lane, azimuth) against the model's mode
    series over rho itself with the device's counts, at RTOL; 'exact' takes the weighted sum of the kinds' values at the azimuth."""
    L, N = 30, 64
    lev = [0, L // 3, L - 1]
    V = len(MU_VIEW)
    kw = dict(KW, nb_layers=L, nb_angles=N, surface="brdf", brdf=ROSS_LI, view_mu=MU_VIEW, view_levels=(0, L // 3, -1), brdf_view=True)
    r = SOS_Aer_batch(list(MU0S), 0.3, 1.0, view_azimuths=PHI, n_modes=M_DRIVER, view_first_order=first, **kw)
    base = SOS_Aer_batch(list(MU0S), 0.3, 1.0, **kw)
    same(r, base, SERIES + ("I_view", "I_view_first", "I_view_scattered", "I_view_ground"))
    assert not r.view_mode_status.any() and not r.status.any()
    assert np.array_equal(r.I_view_azimuth, r.I_view_azimuth_first + r.I_view_azimuth_scattered + r.I_view_azimuth_ground)
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    for b in range(3):
        c, gr = BV.black_column(MU0S[b], L, N)
        with np.errstate(all="ignore"):
            out, status = BV.mode_series_view(c, gr, fa, fr, ROSS_LI, M_DRIVER, 25, int(r.n[b]), tuple(int(x) for x in r.bounce_orders[:, b]),
                                              MU_VIEW, VN.QUAD_GRID, ground_scale=1.0, beam_in_modes=first == "modes")
        assert status == 0
        ground = VA.synthesize(out["ground"][:, lev], PHI)
        if first == "exact":
            ground = ground + np.moveaxis(BV.beam_ground(gr, ROSS_LI, MU_VIEW, PHI)[:, lev], 0, -1)
        scat = VA.synthesize(out["scattered"][:, lev], PHI)
        m = mx(scat + ground)
        e_s, e_g = mx(r.I_view_azimuth_scattered[b] - scat) / m, mx(r.I_view_azimuth_ground[b] - ground) / m
        # (with 'exact' the model's mode 0 carries the diffuse part alone: the azimuth mean is compared where it carries the beam)
        e_0 = mx(r.I_view_ground[b] - out["ground"][0][lev]) / m if first == "modes" else 0.0
        print("%s mu0=%.2f: scattered %.3e, ground %.3e, azimuth-mean ground %.3e of their maximum" % (first, MU0S[b], e_s, e_g, e_0))
        assert e_s <= RTOL and e_g <= RTOL and e_0 <= RTOL


# ---- 6. the albedos ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,N", [(30, 64), (24, 66)])
def test_albedos_against_the_model(L, N):
    r = driver(L, N, ross_li_of(WEIGHTS))
    mu = O.make_mu(N)
    Rs, r0s = model_terms(N)
    bsa = np.array([RL.black_sky_albedo(mu, N, r0s[:, b], WEIGHTS[b]) for b in range(3)])
    wsa = np.array([RL.white_sky_albedo(mu, N, Rs, WEIGHTS[b]) for b in range(3)])
    print("L=%d N=%d: black-sky %s (model %s), white-sky %s (model %s)" % (L, N, r.black_sky_albedo, bsa, r.white_sky_albedo, wsa))
    assert np.max(np.abs(r.black_sky_albedo - bsa)) <= 1e-13 and np.max(np.abs(r.white_sky_albedo - wsa)) <= 1e-13
    # the kernels' own white-sky albedos at mu_floor = 0 against the published constants, within the grid's measured distance
    k = driver(L, N, ("ross_li", [0.0, 0.0, 0.5], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], 0.0), raise_on_error=False)
    for b, kind in ((0, "ross_thick"), (1, "li_sparse_r")):
        d = abs(k.white_sky_albedo[b] - RL.WHITE_SKY[kind])
        print("N=%d %s: white-sky albedo %.9f (published %.6f), distance %.3e" % (N, kind, k.white_sky_albedo[b], RL.WHITE_SKY[kind], d))
        assert d <= 2 * RL.WHITE_SKY_GRID_DISTANCE[kind, N]


# ---- 7. refusals: nothing is written --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    L, N = 24, 37
    M1, V, K, Gd = N - 1, 5, 3, 7
    s, tau = handle(columns(L, N))
    lib = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    d_R, d_r0, d_S, d_Sv, d_out = (dfull(sh, guard=Gd) for sh in ((4, M1, M1), (4, 3, M1), (3, M1), (3, V), (3, 2, 2 * V)))
    d_I, d_tau, d_mu0, d_w = dev(sample_field(L, N)), dev(tau), dev(MU0S), dev(WEIGHTS)
    d_Rs, d_r0s, d_Rv, d_r0v = dev(np.ones((K, M1, M1))), dev(np.ones((K, 3, M1))), dev(np.ones((K, M1, V))), dev(np.ones((K, 3, V)))
    P = lambda *v: (ctypes.c_double * 3)(*v)
    mv = (ctypes.c_double * V)(0.01, 0.123, 0.35, 0.6, 1.0)
    lev = (ctypes.c_int * 2)(0, L - 1)
    RT, LS = _lib.BRDF_ROSS_THICK, _lib.BRDF_LI_SPARSE_R
    op = lambda kind, p, n, nphi=65, out=d_R: lib.sosrt_brdf_operator_dev(s._h, kind, p, n, nphi, vp(out))
    opm = lambda kind, p, n: lib.sosrt_brdf_operator_modes_dev(s._h, kind, p, n, 65, 1, 4, 1, vp(d_R))
    beam = lambda kind, p, n: lib.sosrt_brdf_beam_modes_dev(s._h, 3, kind, p, n, 65, 1, 4, vp(d_mu0), vp(d_r0))
    vrow = lambda kind, p, n: lib.sosrt_brdf_view_rows_modes_dev(s._h, kind, p, n, 65, 1, 4, 0, V, mv, vp(d_R))
    vbeam = lambda kind, p, n: lib.sosrt_brdf_view_beam_modes_dev(s._h, 3, kind, p, n, 65, 1, 4, vp(d_mu0), V, mv, vp(d_r0))
    vaz = lambda kind, p, n: lib.sosrt_brdf_view_beam_azimuth_dev(s._h, 3, kind, p, n, vp(d_mu0), V, mv, 2, vp(d_mu0), vp(d_r0))
    src = lambda B=3, K=K, I=d_I, t=d_tau, R=d_Rs, r0=d_r0s, w=d_w, out=d_S: lib.sosrt_ground_source_terms_dev(
        s._h, B, K, vp(I), vp(t), vp(R), vp(r0), vp(w), vp(out))
    vg = lambda B=3, K=K, nv=V, t=d_tau, I=d_I, Rv=d_Rv, r0v=d_r0v, w=d_w, nlev=2, out=d_out: lib.sosrt_view_ground_terms_dev(
        s._h, B, K, nv, mv, vp(t), vp(I), vp(Rv), vp(r0v), vp(w), nlev, lev, 0, vp(d_Sv), vp(out))
    calls = {}
    for name, kind in (("ross-thick", RT), ("li-sparse", LS)):
        calls.update({
            name + " nparams 0": lambda kind=kind: op(kind, None, 0), name + " nparams 3": lambda kind=kind: op(kind, P(0.1, 0.2, 0.3), 3),
            name + " null params": lambda kind=kind: op(kind, None, 1), name + " floor 1": lambda kind=kind: op(kind, P(1.0), 1),
            name + " floor < 0": lambda kind=kind: op(kind, P(-0.1), 1), name + " floor nan": lambda kind=kind: op(kind, P(np.nan), 1),
            name + " floor inf": lambda kind=kind: op(kind, P(np.inf), 1), name + " nphi": lambda kind=kind: op(kind, P(0.1), 1, 2),
            name + " null out": lambda kind=kind: op(kind, P(0.1), 1, 65, None),
            name + " operator modes": lambda kind=kind: opm(kind, P(1.5), 1), name + " beam modes": lambda kind=kind: beam(kind, P(0.1), 2),
            name + " view rows": lambda kind=kind: vrow(kind, P(-1.0), 1), name + " view beam": lambda kind=kind: vbeam(kind, None, 1),
            name + " view azimuth": lambda kind=kind: vaz(kind, P(np.nan), 1),
        })
    calls.update({
        "kind 4": lambda: op(4, P(0.1), 1),
        "source K=0": lambda: src(K=0), "source K=5": lambda: src(K=_lib.BRDF_MAX_TERMS + 1), "source K<0": lambda: src(K=-1),
        "source B=0": lambda: src(B=0), "source B=4": lambda: src(B=4), "source null I": lambda: src(I=None), "source null tau": lambda: src(t=None),
        "source null R": lambda: src(R=None), "source null weight": lambda: src(w=None), "source null out": lambda: src(out=None),
        "view K=0": lambda: vg(K=0), "view K=5": lambda: vg(K=5), "view B=4": lambda: vg(B=4), "view V=0": lambda: vg(nv=0),
        "view V large": lambda: vg(nv=_lib.MAX_VIEWS + 1), "view null tau": lambda: vg(t=None), "view null weight": lambda: vg(w=None),
        "view null out": lambda: vg(out=None), "view I without rows": lambda: vg(Rv=None), "view rows without I": lambda: vg(I=None),
        "view no source": lambda: vg(I=None, Rv=None, r0v=None), "view no levels": lambda: vg(nlev=0),
    })

    def untouched():
        s.synchronize()
        sync()
        return all(bool(torch.isnan(t).all()) for t in (d_R, d_r0, d_S, d_Sv, d_out))

    for name, call in calls.items():
        rc = call()
        assert rc == _lib.E_INVALID and lib.sosrt_last_error(), name
        assert untouched(), name
    assert b"mu_floor" in (op(RT, P(1.0), 1), lib.sosrt_last_error())[1] and b"SOSRT_BRDF_MAX_TERMS" in (src(K=9), lib.sosrt_last_error())[1]
    s.set_columns_single_slab([0.5, 0.6, 0.7], 0.9, 0.3)
    for name, call in {"operator": lambda: op(RT, P(0.1), 1), "source": src, "view": vg}.items():
        assert call() == _lib.E_INVALID and b"single slab" in lib.sosrt_last_error(), name
        assert untouched(), name
    s.close()
    # valid calls write their outputs and leave the guard elements behind them alone
    s, _ = handle(columns(L, N))
    assert src() == 0 and vg() == 0 and opm(LS, P(0.0), 1) == 0
    s.synchronize()
    sync()
    for t, n in ((d_S, 3 * M1), (d_Sv, 3 * V), (d_out, 3 * 2 * 2 * V), (d_R, 4 * M1 * M1)):
        assert bool(torch.isfinite(t[:n]).all()) and bool(torch.isnan(t[n:]).all())
    s.close()


# ---- 8. the default path ---------------------------------------------------------------------------------------------------------------------
def test_a_ross_li_call_leaves_the_default_path_its_bytes():
    L, N = 24, 66
    kw = dict(tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.9, nb_layers=L, nb_angles=N, max_orders=64)
    plain = lambda: SOS_Aer_batch(list(MU0S), 0.3, [0.1, 0.3, 0.5], **kw)
    before = plain()
    r = SOS_Aer_batch(list(MU0S), 0.3, 1.0, surface="brdf", brdf=ross_li_of(WEIGHTS), **kw)
    after = plain()
    assert r.bounces is not None and r.white_sky_albedo is not None and before.bounces is None and before.white_sky_albedo is None
    assert not r.status.any()
    assert np.array_equal(before.I, after.I) and np.array_equal(before.n, after.n) and np.array_equal(before.status, after.status)
    assert np.max(np.abs(r.I - before.I)) > 1e-3 * np.max(before.I)


def test_the_other_drivers_reach_the_same_series():
    from sosrt import forcing
    from sosrt.main import SOS_Aer, SOS_Aer_layers, solve_batch_device
    kw = dict(tauStar_atm=0.124, alb_atm=1.0, nb_layers=24, nb_angles=66, max_orders=64, surface="brdf", brdf=ROSS_LI)
    ref = SOS_Aer_batch([0.6], 0.3, 1.0, alb_aer=0.9, **kw)
    lay = SOS_Aer_layers([0.6], 1.0, [(25, 17, 0.3, 0.9)], **kw)
    one = SOS_Aer(mu0=0.6, tauStar_aer=0.3, alb_aer=0.9, aer_phase_fun="hg", g_aer=0.7, **kw)
    res, _ = solve_batch_device([0.6], 0.3, 1.0, alb_aer=0.9, **kw)
    assert not ref.status.any() and ref.bounces[0] >= 2
    for I, bounces, ratio in ((lay.I[0], lay.bounces[0], lay.bounce_ratio[0]), (one.I, one.bounces, one.bounce_ratio),
                              (res["I"][0].cpu().numpy(), int(res["bounces"][0]), float(res["bounce_ratio"][0]))):
        assert np.array_equal(I, ref.I[0]) and bounces == ref.bounces[0] and ratio == ref.bounce_ratio[0]
    assert lay.white_sky_albedo[0] == ref.white_sky_albedo[0] and float(res["black_sky_albedo"][0]) == ref.black_sky_albedo[0]
    assert one.white_sky_albedo == ref.white_sky_albedo[0] and one.black_sky_albedo == ref.black_sky_albedo[0]
    flux = forcing.toa_net_flux(0.6, 0.124, [0.3], 1.0, 1.0, [0.9], nb_layers=24, nb_angles=66, max_orders=64, surface="brdf", brdf=ROSS_LI)
    black = forcing.toa_net_flux(0.6, 0.124, [0.3], 0.0, 1.0, [0.9], nb_layers=24, nb_angles=66, max_orders=64)
    print("net TOA flux over the Ross-Li ground %s, over a black ground %s" % (flux, black))
    assert np.all(np.isfinite(flux)) and np.all(np.abs(flux) < np.abs(black))     # a reflecting ground sends more back to space
