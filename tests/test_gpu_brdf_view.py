"""View radiance over a BRDF ground on the device (csrc/brdf.hip, csrc/api_brdf.hip) through the C ABI: the rows
of the operator's modes and the beam rows at view cosines against the NumPy model of tests/brdf_view_np.py and, at node cosines,
bit for bit against the builders of sections 20 and 21; the exact-azimuth beam rows; the view ground kernel; their refusals; and
SOS_Aer_batch(..., brdf_view=True) with view_mu and view_azimuths against the model's series run with the device's own order and
reflection counts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import brdf_azimuth_np as BA
import brdf_np as G
import brdf_view_np as BV
import sos_oracle as O
import view_azimuth_np as VA
import view_np as VN
from sosrt import _lib, inputs
from sosrt.main import SOS_Aer_batch
from sosrt.solver import Solver
from test_brdf_view_host import NODE_PIN
from test_gpu_azimuth import _close, _solver
from test_gpu_brdf import SHAPES, columns, dev, dfull, handle, host, params_of, run_beam, run_operator, run_source, sample_field, sync
from test_gpu_brdf_azimuth import RANGES, in_range, run_beam_modes, run_operator_modes
from util import RTOL

pytestmark = pytest.mark.gpu

RPV = ("rpv", 0.2, 0.8, -0.1)
MU0S = (0.35, 0.6, 0.85)
OFF_GRID = np.array([0.01, 0.123, 0.35, 0.6, 1.0])          # the limb, an ordinary cosine, two columns' mu0 (hot-spot lanes), the nadir


def grid_handle(N, B=3, L=8):
    """a handle with the grid and B black three-zone columns (the builders read the grid and check B against the columns)"""
    s = _solver(L, N, B=B)
    iu, idn = inputs.slab_indices(120, 25, 17, L)
    s.set_columns(np.full(B, iu), np.full(B, idn), column_mu0(B), 0.0, 1.0, 0.95, 0.124 / L, 0.3 / (idn + 1 - iu), 0.424)
    return s


def column_mu0(B):
    return np.array(MU0S[:B]) if B <= 3 else np.linspace(0.2, 0.95, B)


def view_cosines(N, V):
    """V view cosines: V = 1 off the grid; V = 5 OFF_GRID; V = 17 OFF_GRID and 12 nodes of the grid (first, last, across a wave)"""
    if V == 1:
        return np.array([0.4321]), np.zeros(0, dtype=int)
    if V == 5:
        return OFF_GRID.copy(), np.zeros(0, dtype=int)
    nodes = np.unique(np.linspace(0, N - 2, 12).round().astype(int))
    return np.concatenate((OFF_GRID, O.make_mu(N)[N + 1 + nodes])), nodes


def run_view_rows(s, brdf, mv, m_first, m_count, nphi, sign_odd=False):
    M1, V = s.N - 1, len(mv)
    d = dfull((m_count, M1, V))
    sync()
    kind, p = params_of(brdf)
    s.brdf_view_rows_modes_device(kind, mv, d.data_ptr(), m_first, m_count, p, nphi, sign_odd=sign_odd)
    return np.swapaxes(host(d, s).reshape(m_count, M1, V), 1, 2)               # [m, v, j], as the model writes it


def run_view_beam(s, brdf, mu0, mv, m_first, m_count, nphi):
    B, V = len(mu0), len(mv)
    d_mu0, d = dev(mu0), dfull((m_count, B, V))
    sync()
    kind, p = params_of(brdf)
    s.brdf_view_beam_modes_device(kind, d_mu0.data_ptr(), mv, d.data_ptr(), m_first, m_count, p, nphi, B=B)
    return host(d, s).reshape(m_count, B, V)


# ---- a. the builders against the model, and bit for bit against the grid's builders at nodes ------------------------------------------------
@pytest.mark.parametrize("nphi", [9, 65, 300])
@pytest.mark.parametrize("N,V", [(37, 17), (66, 17), (37, 1), (66, 5)])
def test_view_rows_and_beam_modes(N, V, nphi):
    """N - 1 = 36 is a partial wave, 65 one lane into a second; nphi = 300 crosses the 256-node chunk; the ranges straddle the 8 modes
    of a launch.  At a view cosine that is a node the rows are the bits of sosrt_brdf_operator_modes_dev's column and of
    sosrt_brdf_beam_modes_dev (mode 0: of the azimuth-mean entry points)."""
    s = grid_handle(N)
    mu = O.make_mu(N)
    mv, nodes = view_cosines(N, V)
    off = len(mv) - len(nodes)
    ms_all = list(range(min(_lib.MAX_MODES, nphi - 2) + 1))
    R = BV.view_rows_modes(mu, N, mv, RPV, ms_all, nphi)
    r0 = np.stack([BV.view_beam_modes(mv, m0, RPV, ms_all, nphi) for m0 in MU0S], axis=1)
    mxR, mx0 = np.max(np.abs(R[0])), np.max(np.abs(r0[0]))
    lib = _lib.lib()
    for m_first, m_count in RANGES(nphi):
        if not in_range(m_first, m_count, nphi):
            d_R, d_r0, d_mu0 = dfull((m_count, N - 1, V), guard=5), dfull((m_count, 3, V), guard=5), dev(MU0S)
            p = (ctypes.c_double * 3)(*RPV[1:])
            cmv = (ctypes.c_double * V)(*mv)
            sync()
            assert lib.sosrt_brdf_view_rows_modes_dev(s._h, _lib.BRDF_RPV, p, 3, nphi, m_first, m_count, 0, V, cmv,
                                                      ctypes.c_void_p(d_R.data_ptr())) == _lib.E_INVALID
            assert b"modes" in lib.sosrt_last_error()
            assert lib.sosrt_brdf_view_beam_modes_dev(s._h, 3, _lib.BRDF_RPV, p, 3, nphi, m_first, m_count, ctypes.c_void_p(d_mu0.data_ptr()),
                                                      V, cmv, ctypes.c_void_p(d_r0.data_ptr())) == _lib.E_INVALID
            s.synchronize()
            sync()
            assert bool(torch.isnan(d_R).all()) and bool(torch.isnan(d_r0).all())
            continue
        sl = slice(m_first, m_first + m_count)
        got_R, got_r0 = run_view_rows(s, RPV, mv, m_first, m_count, nphi), run_view_beam(s, RPV, MU0S, mv, m_first, m_count, nphi)
        eR, e0 = np.max(np.abs(got_R - R[sl])) / mxR, np.max(np.abs(got_r0 - r0[sl])) / mx0
        print("N=%d V=%d nphi=%d modes %d..%d: view rows %.3e of max |Rv^0|, beam rows %.3e of max |r0v^0|"
              % (N, V, nphi, m_first, m_first + m_count - 1, eR, e0))
        assert np.all(np.isfinite(got_R)) and np.all(np.isfinite(got_r0)) and eR <= 1e-12 and e0 <= 1e-12
        sgn = np.array([(-1.0) ** m for m in range(m_first, m_first + m_count)])
        assert np.array_equal(run_view_rows(s, RPV, mv, m_first, m_count, nphi, sign_odd=True), sgn[:, None, None] * got_R)
        assert np.array_equal(run_view_beam(s, RPV, MU0S[:1], mv, m_first, m_count, nphi), got_r0[:, :1])
        if len(nodes):
            grid_R, grid_r0 = run_operator_modes(s, RPV, m_first, m_count, nphi), run_beam_modes(s, RPV, MU0S, m_first, m_count, nphi)
            assert np.array_equal(got_R[:, off:], grid_R[:, nodes]) and np.array_equal(got_r0[:, :, off:], grid_r0[:, :, nodes])
            if m_first == 0:
                assert np.array_equal(got_R[0, off:], run_operator(s, RPV, nphi)[nodes])
                assert np.array_equal(got_r0[0][:, off:], run_beam(s, RPV, MU0S, nphi)[:, nodes])
    s.close()


def test_beam_rows_where_a_wave_straddles_columns():
    """B = 70, V = 1: one lane per column, a wave holds 64 of them"""
    B, N, nphi = 70, 37, 65
    s = grid_handle(N, B=B)
    mu0 = column_mu0(B)
    mv = np.array([0.6])
    got = run_view_beam(s, RPV, mu0, mv, 0, 9, nphi)
    ref = np.stack([BV.view_beam_modes(mv, m0, RPV, range(9), nphi) for m0 in mu0], axis=1)
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref[0]))
    for b in (0, 63, 64, 69):
        assert np.array_equal(run_view_beam(s, RPV, mu0[b:b + 1], mv, 0, 9, nphi)[:, 0], got[:, b])
    d_mu0, d_phi, d_out = dev(mu0), dev([0.0, 1.0, np.pi]), dfull((3, B, 1), guard=3)
    sync()
    s.brdf_view_beam_azimuth_device("rpv", d_mu0.data_ptr(), mv, d_phi.data_ptr(), 3, d_out.data_ptr(), RPV[1:], B=B)
    out = host(d_out, s)
    ref = np.stack([BV.view_beam_azimuth(mv, m0, RPV, [0.0, 1.0, np.pi]) for m0 in mu0], axis=1)
    assert np.all(np.isnan(out[3 * B:])) and np.max(np.abs(out[:3 * B].reshape(3, B, 1) - ref)) <= 1e-12 * np.max(ref)
    s.close()


def test_lambertian_view_modes():
    s = grid_handle(37)
    mv, _ = view_cosines(37, 17)
    for nphi in (9, 300):
        m_last = min(_lib.MAX_MODES, nphi - 2)
        R, r0 = run_view_rows(s, "lambertian", mv, 0, m_last + 1, nphi), run_view_beam(s, "lambertian", MU0S, mv, 0, m_last + 1, nphi)
        print("nphi=%d: Lambertian view modes m >= 1: rows %.2e, beam rows %.2e" % (nphi, np.max(np.abs(R[1:])), np.max(np.abs(r0[1:]))))
        assert np.max(np.abs(R[1:])) <= 1e-15 and np.max(np.abs(r0[1:])) <= 1e-15
        assert np.max(np.abs(R[0] - BV.view_rows(O.make_mu(37), 37, mv, "lambertian", nphi))) <= 1e-12 and np.max(np.abs(r0[0] - 1)) <= 1e-12
    s.close()


@pytest.mark.parametrize("V", [1, 5, 17])
def test_exact_azimuth_beam_rows(V):
    """rho at the azimuth itself against the model, the hot-spot pairs mu_view = mu0, phi = 0 among them (finite: G^2 does not cancel)"""
    N = 37
    s = grid_handle(N)
    mv, _ = view_cosines(N, V)
    phi = np.array([0.0, 1e-9, 0.3, np.pi / 2, 2.0, np.pi, 4.0, 2 * np.pi, -0.3])
    d_mu0, d_phi, d_out = dev(MU0S), dev(phi), dfull((len(phi), 3, V), guard=4)
    sync()
    for brdf in (RPV, "lambertian"):
        kind, p = params_of(brdf)
        s.brdf_view_beam_azimuth_device(kind, d_mu0.data_ptr(), mv, d_phi.data_ptr(), len(phi), d_out.data_ptr(), p, B=3)
        out = host(d_out, s)
        got = out[:len(phi) * 3 * V].reshape(len(phi), 3, V)
        ref = np.stack([BV.view_beam_azimuth(mv, m0, brdf, phi) for m0 in MU0S], axis=1)
        err = np.max(np.abs(got - ref)) / np.max(ref)
        print("V=%d %s: exact beam rows %.3e of the maximum" % (V, brdf if brdf == "lambertian" else "rpv", err))
        assert np.all(np.isnan(out[len(phi) * 3 * V:])) and np.all(np.isfinite(got)) and err <= 1e-12
    if V >= 5:                                               # the hot spot: the lane's maximum over the azimuths, and even in phi
        s.brdf_view_beam_azimuth_device("rpv", d_mu0.data_ptr(), mv, d_phi.data_ptr(), len(phi), d_out.data_ptr(), RPV[1:], B=3)
        got = host(d_out, s)[:len(phi) * 3 * V].reshape(len(phi), 3, V)
        assert got[0, 0, 2] == got[:, 0, 2].max() and got[0, 1, 3] == got[:, 1, 3].max()
        assert abs(got[2, 1, 3] - got[8, 1, 3]) <= 1e-15 * got[2, 1, 3]
    s.close()


# ---- b. the view ground kernel -----------------------------------------------------------------------------------------------------------
def run_view_ground(s, mv, tau, levels, I=None, Rv=None, r0v=None, scale=None, out0=None, want_S=True):
    """(out [B, nlev, 2V], S [B, V]); Rv [v, j] as the model writes it; out0: accumulate onto it"""
    B, V, nlev = tau.shape[0], len(mv), len(levels)
    d_tau = dev(tau)
    d_I, d_Rv = (None, None) if I is None else (dev(I), dev(Rv.T))
    d_r0v, d_sc = None if r0v is None else dev(r0v), None if scale is None else dev(scale)
    d_out = dfull((B, nlev, 2 * V), guard=6) if out0 is None else torch.cat((dev(out0).reshape(-1), dfull((6,))))
    d_S = dfull((B, V), guard=2)
    sync()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    s.view_ground_device(mv, d_tau.data_ptr(), levels, d_out.data_ptr(), d_I=ptr(d_I), d_Rv=ptr(d_Rv), d_r0v=ptr(d_r0v), d_scale=ptr(d_sc),
                         accumulate=out0 is not None, d_S_out=d_S.data_ptr() if want_S else 0, B=B)
    out, S = host(d_out, s), host(d_S, s)
    assert np.all(np.isnan(out[B * nlev * 2 * V:])) and np.all(np.isnan(S[B * V:]))
    if I is not None:                                        # the stage writes its outputs only
        assert np.array_equal(host(d_I, s), I) and np.array_equal(host(d_Rv, s), Rv.T) and np.array_equal(host(d_tau, s), tau)
    return out[:B * nlev * 2 * V].reshape(B, nlev, 2 * V), S[:B * V].reshape(B, V)


@pytest.mark.parametrize("V", [1, 5, 17])
@pytest.mark.parametrize("L,N", SHAPES)
def test_view_ground_against_the_model(L, N, V):
    cols = columns(L, N)
    s, tau = handle(cols)
    mu = cols[0].mu
    I = np.array(sample_field(L, N))
    mv, nodes = view_cosines(N, V)
    off = V - len(nodes)
    Rv = run_view_rows(s, RPV, mv, 0, 1, 65)[0]
    r0v = run_view_beam(s, RPV, MU0S, mv, 0, 1, 65)[0]
    scale = np.array([0.3, 0.0, 0.8])
    levels = [0, L - 1, L // 2, 1, 0]
    for use_I, use_r0, use_scale in ((True, True, True), (True, False, True), (False, True, True), (True, True, False), (True, False, False)):
        kw = dict(I=I if use_I else None, Rv=Rv if use_I else None, r0v=r0v if use_r0 else None, scale=scale if use_scale else None)
        got, S = run_view_ground(s, mv, tau, levels, **kw)
        for b in range(3):
            Sref = G.ground_source(Rv, I[b, -1] if use_I else np.zeros(2 * N), r0v[b] if use_r0 else None, tau[b, -1], MU0S[b],
                                   scale[b] if use_scale else 1.0)
            ref = BV.view_ground(Sref, tau[b], mv)[levels]
            if use_scale and scale[b] == 0:
                assert not np.any(got[b]) and not np.any(np.signbit(got[b])) and not np.any(S[b])
                continue
            eS, eG = np.max(np.abs(S[b] - Sref) / np.abs(Sref)), np.max(np.abs(got[b] - ref)) / np.max(ref)
            assert eS <= 1e-13 and eG <= 1e-12, (use_I, use_r0, use_scale, b, eS, eG)
            assert not np.any(got[b][:, :V]) and not np.any(np.signbit(got[b][:, :V]))        # downward lanes: exactly +0
            assert np.array_equal(got[b][1, V:], S[b])       # the surface row is the source itself
        one, S1 = run_view_ground(s, mv, tau[:1], levels, **{k: None if v is None else (v if k == "Rv" else v[:1]) for k, v in kw.items()})
        assert np.array_equal(one[0], got[0]) and np.array_equal(S1[0], S[0])               # a column's bits do not depend on B
        nos, _ = run_view_ground(s, mv, tau, levels, want_S=False, **kw)
        assert np.array_equal(nos, got)
        if len(nodes) and use_I:
            # at a node: the bits of sosrt_ground_source_dev with the grid's operator, and the model's unblended ground field
            R, r0 = run_operator(s, RPV), run_beam(s, RPV, MU0S)
            Sg = run_source(s, I, tau, R, r0 if use_r0 else None, scale if use_scale else None)
            assert np.array_equal(S[:, off:], Sg[:, nodes])
            for b in range(3):
                Gf, _, _ = G.ground_field(Sg[b], tau[b], mu, N, blend=False)
                ref = Gf[levels][:, N + 1 + nodes]
                assert np.max(np.abs(got[b][:, V + off:] - ref)) <= 1e-12 * max(np.max(ref), 1e-300)
    # accumulate: the upward lanes are added exactly, the downward ones left; more levels than one launch takes
    base = np.random.default_rng(7).random((3, len(levels), 2 * V))
    wrote, _ = run_view_ground(s, mv, tau, levels, I=I, Rv=Rv, scale=scale)
    acc, _ = run_view_ground(s, mv, tau, levels, I=I, Rv=Rv, scale=scale, out0=base)
    assert np.array_equal(acc[:, :, V:], base[:, :, V:] + wrote[:, :, V:]) and np.array_equal(acc[:, :, :V], base[:, :, :V])
    many = list(np.arange(260) % L)
    big, _ = run_view_ground(s, mv, tau, many, I=I, Rv=Rv, r0v=r0v)
    few, _ = run_view_ground(s, mv, tau, list(range(L)), I=I, Rv=Rv, r0v=r0v)
    assert np.array_equal(big, few[:, many])
    s.close()


def test_the_stages_leave_the_handle_alone():
    """A solve before and after the four stages has the same bits, and order targets set before them still hold after them"""
    L, N = 24, 37
    cols = columns(L, N)
    s, tau = handle(cols)
    P0a, P0r = np.stack([c.P0_atm for c in cols]), np.stack([c.P0_aer for c in cols])
    before = s.solve(tau, P0a, P0r)
    mv, _ = view_cosines(N, 17)
    d_t = torch.tensor([3, 4, 5], dtype=torch.int32, device=torch.device("cuda", 0))
    d_tau, d_a, d_r, d_I = dev(tau), dev(P0a), dev(P0r), dfull((3, L, 2 * N))
    d_n = torch.zeros(3, dtype=torch.int32, device=d_t.device)
    sync()
    s.set_order_targets(d_t.data_ptr())
    try:
        Rv, r0v = run_view_rows(s, RPV, mv, 0, 9, 65)[0], run_view_beam(s, RPV, MU0S, mv, 0, 9, 65)[0]
        d_mu0, d_phi, d_az = dev(MU0S), dev([0.0, 2.0]), dfull((2, 3, 17))
        sync()
        s.brdf_view_beam_azimuth_device("rpv", d_mu0.data_ptr(), mv, d_phi.data_ptr(), 2, d_az.data_ptr(), RPV[1:], B=3)
        run_view_ground(s, mv, tau, [0, L - 1], I=before.I, Rv=Rv, r0v=r0v)
        s.solve_device(d_tau.data_ptr(), d_a.data_ptr(), d_r.data_ptr(), d_I.data_ptr(), d_n_orders=d_n.data_ptr())
        s.synchronize()
    finally:
        s.set_order_targets(None)
    after = s.solve(tau, P0a, P0r)
    assert list(d_n.cpu().numpy()) == [3, 4, 5]
    assert np.array_equal(before.I, after.I) and np.array_equal(before.n, after.n) and np.array_equal(before.status, after.status)
    s.close()


# ---- c. refusals: nothing is written -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    L, N, V, Gd = 24, 37, 5, 7
    M1 = N - 1
    s, tau = handle(columns(L, N))
    lib = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    d_R, d_r0, d_az = dfull((4, M1, V), guard=Gd), dfull((4, 3, V), guard=Gd), dfull((2, 3, V), guard=Gd)
    d_out, d_S = dfull((3, 2, 2 * V), guard=Gd), dfull((3, V), guard=Gd)
    d_mu0, d_phi, d_tau, d_I, d_sc = dev(MU0S), dev([0.0, 1.0]), dev(tau), dev(sample_field(L, N)), dev([1.0, 1.0, 1.0])
    d_Rv, d_r0v = dev(np.ones((M1, V))), dev(np.ones((3, V)))
    rpv = (ctypes.c_double * 3)(0.2, 0.8, -0.1)
    P = lambda *v: (ctypes.c_double * 3)(*v)
    MV = lambda *v: (ctypes.c_double * len(v))(*v)
    mv = MV(*OFF_GRID)
    lev = (ctypes.c_int * 2)(0, L - 1)
    LAM, RP = _lib.BRDF_LAMBERTIAN, _lib.BRDF_RPV
    rows = lambda kind=RP, p=rpv, n=3, nphi=65, m1=1, mc=4, V=V, mv=mv, out=d_R: lib.sosrt_brdf_view_rows_modes_dev(
        s._h, kind, p, n, nphi, m1, mc, 1, V, mv, vp(out))
    beam = lambda B=3, kind=RP, p=rpv, n=3, nphi=65, m1=1, mc=4, mu0=d_mu0, V=V, mv=mv, out=d_r0: lib.sosrt_brdf_view_beam_modes_dev(
        s._h, B, kind, p, n, nphi, m1, mc, vp(mu0), V, mv, vp(out))
    az = lambda B=3, kind=RP, p=rpv, n=3, mu0=d_mu0, V=V, mv=mv, nout=2, phi=d_phi, out=d_az: lib.sosrt_brdf_view_beam_azimuth_dev(
        s._h, B, kind, p, n, vp(mu0), V, mv, nout, vp(phi), vp(out))
    gnd = lambda B=3, V=V, mv=mv, tau=d_tau, I=d_I, Rv=d_Rv, r0v=d_r0v, sc=d_sc, nlev=2, lev=lev, acc=0, S=d_S, out=d_out: lib.sosrt_view_ground_dev(
        s._h, B, V, mv, vp(tau), vp(I), vp(Rv), vp(r0v), vp(sc), nlev, lev, acc, vp(S), vp(out))
    calls = {
        "rows nphi": lambda: rows(nphi=2), "rows nphi large": lambda: rows(nphi=65538), "rows kind": lambda: rows(kind=7, p=None, n=0),
        "rows nparams": lambda: rows(n=2), "rows lambertian nparams": lambda: rows(kind=LAM), "rows rho0": lambda: rows(p=P(0.0, 0.8, -0.1)),
        "rows k": lambda: rows(p=P(0.2, -1.0, 0.0)), "rows theta": lambda: rows(p=P(0.2, 0.8, 1.0)), "rows nan": lambda: rows(p=P(0.2, 0.8, np.nan)),
        "rows null params": lambda: rows(p=None), "rows null out": lambda: rows(out=None), "rows m_first < 0": lambda: rows(m1=-1),
        "rows m_count = 0": lambda: rows(mc=0), "rows past nphi - 2": lambda: rows(nphi=5), "rows past MAX_MODES": lambda: rows(nphi=300, m1=62),
        "rows overflow": lambda: rows(nphi=300, m1=2, mc=2 ** 31 - 1), "rows V = 0": lambda: rows(V=0), "rows V = 65": lambda: rows(V=65, mv=MV(*([0.5] * 65))),
        "rows null mu_view": lambda: rows(mv=None), "rows mu_view small": lambda: rows(mv=MV(0.5, 0.5, 0.009, 0.5, 0.5)),
        "rows mu_view > 1": lambda: rows(mv=MV(0.5, 1.0000001, 0.5, 0.5, 0.5)), "rows mu_view nan": lambda: rows(mv=MV(0.5, 0.5, 0.5, 0.5, np.nan)),
        "rows mu_view negative": lambda: rows(mv=MV(-0.5, 0.5, 0.5, 0.5, 0.5)),
        "beam B=0": lambda: beam(B=0), "beam B=4": lambda: beam(B=4), "beam nphi": lambda: beam(nphi=1), "beam kind": lambda: beam(kind=-1, p=None, n=0),
        "beam theta": lambda: beam(p=P(0.2, 0.8, -1.0)), "beam null mu0": lambda: beam(mu0=None), "beam null out": lambda: beam(out=None),
        "beam m_count = 0": lambda: beam(mc=0), "beam past MAX_MODES": lambda: beam(nphi=300, m1=64, mc=2), "beam V": lambda: beam(V=-1),
        "beam mu_view inf": lambda: beam(mv=MV(0.5, np.inf, 0.5, 0.5, 0.5)),
        "azimuth B=0": lambda: az(B=0), "azimuth B=4": lambda: az(B=4), "azimuth kind": lambda: az(kind=9), "azimuth nparams": lambda: az(n=1),
        "azimuth k": lambda: az(p=P(0.2, 0.0, 0.0)), "azimuth nphi_out": lambda: az(nout=0), "azimuth null phi": lambda: az(phi=None),
        "azimuth null mu0": lambda: az(mu0=None), "azimuth null out": lambda: az(out=None), "azimuth V": lambda: az(V=0),
        "azimuth mu_view": lambda: az(mv=MV(0.5, 0.5, 0.5, 0.5, 0.0)),
        "ground B=0": lambda: gnd(B=0), "ground B=4": lambda: gnd(B=4), "ground V": lambda: gnd(V=0), "ground null mu_view": lambda: gnd(mv=None),
        "ground mu_view": lambda: gnd(mv=MV(0.5, 0.5, 0.5, 2.0, 0.5)), "ground nlev": lambda: gnd(nlev=0), "ground null levels": lambda: gnd(lev=None),
        "ground level = L": lambda: gnd(lev=(ctypes.c_int * 2)(0, L)), "ground level < 0": lambda: gnd(lev=(ctypes.c_int * 2)(-1, 0)),
        "ground I without Rv": lambda: gnd(Rv=None), "ground Rv without I": lambda: gnd(I=None), "ground no source": lambda: gnd(I=None, Rv=None, r0v=None),
        "ground null tau": lambda: gnd(tau=None), "ground null out": lambda: gnd(out=None), "ground accumulate, null out": lambda: gnd(acc=1, out=None),
    }

    def untouched():
        s.synchronize()
        sync()
        return all(bool(torch.isnan(t).all()) for t in (d_R, d_r0, d_az, d_out, d_S))

    for name, call in calls.items():
        rc = call()
        assert rc == _lib.E_INVALID and lib.sosrt_last_error(), name
        assert untouched(), name
    s.set_columns_single_slab([0.5, 0.6, 0.7], 0.9, 0.3)
    for name, call in {"rows": rows, "beam": beam, "azimuth": az, "ground": gnd}.items():
        assert call() == _lib.E_INVALID and b"single slab" in lib.sosrt_last_error(), name
        assert untouched(), name
    s.close()
    # valid calls write their outputs and leave the guard elements behind them alone
    s, _ = handle(columns(L, N))
    assert rows() == 0 and beam() == 0 and az() == 0 and gnd() == 0
    s.synchronize()
    sync()
    for t, n in ((d_R, 4 * M1 * V), (d_r0, 4 * 3 * V), (d_az, 2 * 3 * V), (d_out, 3 * 2 * 2 * V), (d_S, 3 * V)):
        assert bool(torch.isfinite(t[:n]).all()) and bool(torch.isnan(t[n:]).all())
    s.close()


# ---- d. the whole driver against the model's series run with the device's counts -------------------------------------------------------------
MU_VIEW = OFF_GRID
M_DRIVER = 6
PHI = 2 * np.pi * np.arange(2 * M_DRIVER + 2) / (2 * M_DRIVER + 2)          # 14 uniform azimuths: phi = 0 is node 0, phi = pi node 7
KW = dict(alb_aer=0.95, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.5, max_orders=64)


@functools.lru_cache(maxsize=None)
def driver(L, N, brdf, grd_alb=1.0, view=True, azimuths=False, first="exact", quad="grid"):
    kw = dict(KW, nb_layers=L, nb_angles=N, surface="brdf", brdf=brdf)
    if view:
        kw.update(view_mu=MU_VIEW, view_levels=(0, L // 3, -1), view_quadrature=quad, brdf_view=True)
    if azimuths:
        kw.update(view_azimuths=PHI, n_modes=M_DRIVER, view_first_order=first)
    return SOS_Aer_batch(list(MU0S), 0.3, grd_alb if np.isscalar(grd_alb) else list(grd_alb), **kw)


@functools.lru_cache(maxsize=None)
def model(L, N, brdf, b, n, orders, scale, quad, M=0, beam_in_modes=True):
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    c, gr = BV.black_column(MU0S[b], L, N)
    with np.errstate(all="ignore"):
        out, status = BV.mode_series_view(c, gr, fa, fr, brdf, M, 25, n, orders, MU_VIEW, VN.QUAD_GRID if quad == "grid" else VN.QUAD_LINEAR,
                                          ground_scale=scale, beam_in_modes=beam_in_modes)
    return out, status, gr


def same_series(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("I", "n", "status", "bounces", "bounce_ratio", "bounce_orders"))


@pytest.mark.parametrize("L,N,brdf,quad", [(30, 64, RPV, "grid"), (24, 66, RPV, "linear"), (24, 66, "lambertian", "grid")],
                         ids=["L30-N64-rpv-grid", "L24-N66-rpv-linear", "L24-N66-lambertian-grid"])
def test_view_mu_driver_against_the_model_series(L, N, brdf, quad):
    """mu0 = 0.35, 0.6, 0.85; RPV, and the Lambertian ground at scale 0, 0.3, 0.8.  I, n, status and the reflections' records are the
    bits of the call without view_mu; the three terms against the model's series run with the device's counts."""
    scales = (1.0, 1.0, 1.0) if brdf != "lambertian" else (0.0, 0.3, 0.8)
    r = driver(L, N, brdf, scales if brdf == "lambertian" else 1.0, quad=quad)
    plain = driver(L, N, brdf, scales if brdf == "lambertian" else 1.0, view=False)
    lev = [0, L // 3, L - 1]
    V = len(MU_VIEW)
    assert same_series(r, plain) and plain.I_view is None and not r.status.any()
    assert r.I_view_ground.shape == (3, 3, 2 * V) and r.I_view_azimuth is None
    assert np.array_equal(r.I_view, r.I_view_first + r.I_view_scattered + r.I_view_ground)
    assert not np.any(r.I_view_ground[:, :, :V]) and not np.any(np.signbit(r.I_view_ground[:, :, :V]))
    for b in range(3):
        out, status, _ = model(L, N, brdf, b, int(r.n[b]), tuple(int(x) for x in r.bounce_orders[:, b]), scales[b], quad)
        assert status == 0
        ref = {k: out[k][0][lev] for k in ("first", "scattered", "ground")}
        total = ref["first"] + ref["scattered"] + ref["ground"]
        mx = np.max(np.abs(total))
        err = {k: np.max(np.abs(getattr(r, "I_view_" + k)[b] - ref[k])) / mx for k in ref}
        e = np.max(np.abs(r.I_view[b] - total)) / mx
        print("L=%d N=%d %s mu0=%.2f scale %.1f: n = %d, reflections %s; I_view vs the model %.3e of its maximum (%s); ground's share %.2e"
              % (L, N, brdf if brdf == "lambertian" else "rpv", MU0S[b], scales[b], r.n[b], r.bounce_orders[:, b], e,
                 ", ".join("%s %.2e" % kv for kv in err.items()), np.max(ref["ground"]) / mx))
        assert np.all(np.isfinite(r.I_view[b])) and e <= RTOL and max(err.values()) <= RTOL
        if scales[b] == 0:
            assert not np.any(r.I_view_ground[b])
        else:
            assert np.max(ref["ground"]) > 1e-2 * mx         # the ground is a visible part of what the sensor sees


@pytest.mark.parametrize("first", ["exact", "modes"])
def test_view_azimuth_driver_against_the_model_series(first):
    """M = 6 at 14 uniform azimuths over RPV, (L, N) = (30, 64).  I_view* are the bits of the call without view_azimuths.  With
    'modes' the mean over the 14 azimuths is I_view to 1e-12 (the azimuths are the nodes of a rule exact for the modes <= 6); with
    'exact' the beam's reflection is rho at the azimuth itself, whose 14-node mean is not the 65-node rho_bar, so the mean is
    checked on the scattered part and on the ground's term minus the exact beam term."""
    L, N = 30, 64
    r, base = driver(L, N, RPV, azimuths=True, first=first), driver(L, N, RPV)
    lev = [0, L // 3, L - 1]
    V = len(MU_VIEW)
    assert same_series(r, base) and not r.view_mode_status.any() and r.view_mode_status.shape == (M_DRIVER + 1, 3)
    for k in ("I_view", "I_view_first", "I_view_scattered", "I_view_ground"):
        assert np.array_equal(getattr(r, k), getattr(base, k)), k
    assert r.I_view_azimuth_ground.shape == (3, 3, 2 * V, len(PHI))
    assert np.array_equal(r.I_view_azimuth, r.I_view_azimuth_first + r.I_view_azimuth_scattered + r.I_view_azimuth_ground)
    assert not np.any(r.I_view_azimuth_ground[:, :, :V])
    mxv = np.max(np.abs(r.I_view))
    assert np.max(np.abs(r.I_view_azimuth_scattered.mean(axis=-1) - r.I_view_scattered)) <= 1e-12 * mxv
    for b in range(3):
        out, status, gr = model(L, N, RPV, b, int(r.n[b]), tuple(int(x) for x in r.bounce_orders[:, b]), 1.0, "grid", M_DRIVER, first == "modes")
        assert status == 0
        ground = VA.synthesize(out["ground"][:, lev], PHI)
        beam = np.moveaxis(BV.beam_ground(gr, RPV, MU_VIEW, PHI)[:, lev], 0, -1)
        if first == "exact":
            ground = ground + beam
            assert np.max(np.abs((r.I_view_azimuth_ground[b] - beam).mean(axis=-1) - out["ground"][0][lev])) <= 1e-12 * mxv
        scat = VA.synthesize(out["scattered"][:, lev], PHI)
        total_scat_ground = scat + ground
        mx = np.max(np.abs(total_scat_ground))
        e_s, e_g = np.max(np.abs(r.I_view_azimuth_scattered[b] - scat)) / mx, np.max(np.abs(r.I_view_azimuth_ground[b] - ground)) / mx
        print("%s mu0=%.2f: scattered %.3e, ground %.3e of their maximum; the ground's term at TOA, lane mu_view = 0.6, phi = 0 / pi: %.4e / %.4e"
              % (first, MU0S[b], e_s, e_g, r.I_view_azimuth_ground[b, 0, V + 3, 0], r.I_view_azimuth_ground[b, 0, V + 3, M_DRIVER + 1]))
        assert e_s <= RTOL and e_g <= RTOL
    if first == "modes":
        assert np.max(np.abs(r.I_view_azimuth.mean(axis=-1) - r.I_view)) <= 1e-12 * mxv


def test_lambertian_ground_has_no_azimuth_of_its_own():
    """A Lambertian ground has no mode m >= 1: its reflections are skipped, and the ground's term is the same at every azimuth"""
    L, N = 24, 66
    r = driver(L, N, "lambertian", (0.1, 0.3, 0.5), azimuths=True)
    assert not r.view_mode_status.any()
    assert np.max(np.abs(r.I_view_azimuth_ground - r.I_view_ground[..., None])) <= 1e-13 * np.max(r.I_view_ground)
    assert np.max(r.I_view_ground) > 0


def test_the_hot_spot_is_seen_from_the_view_lane():
    """RPV at TOA on the view lane mu_view = mu0: back-scatter (phi = 0) minus forward (phi = pi), against the same over a Lambertian
    ground of equal albedo (RPV's directional-hemispherical albedo at mu0, by the flux quadrature).  Printed; asserted in sign only."""
    L, N = 30, 64
    mu = O.make_mu(N)
    up = mu[N + 1:]
    w = 2 * G.trapezoid_weights(up) * up
    alb = tuple(float(np.sum(w * G.rho_bar(RPV, up, m0))) for m0 in MU0S)
    r, lam = driver(L, N, RPV, azimuths=True), driver(L, N, "lambertian", alb, azimuths=True)
    V = len(MU_VIEW)
    for b, lane in enumerate((V + 2, V + 3)):                # MU_VIEW[2] = 0.35 = MU0S[0], MU_VIEW[3] = 0.6 = MU0S[1]
        d_rpv = r.I_view_azimuth[b, 0, lane, 0] - r.I_view_azimuth[b, 0, lane, M_DRIVER + 1]
        d_lam = lam.I_view_azimuth[b, 0, lane, 0] - lam.I_view_azimuth[b, 0, lane, M_DRIVER + 1]
        print("mu0 = mu_view = %.2f (albedo %.4f): I(0) - I(pi) at TOA %.6e over RPV, %.6e over the Lambertian ground; the ground's term alone %.6e / %.6e"
              % (MU0S[b], alb[b], d_rpv, d_lam, r.I_view_azimuth_ground[b, 0, lane, 0] - r.I_view_azimuth_ground[b, 0, lane, M_DRIVER + 1],
                 lam.I_view_azimuth_ground[b, 0, lane, 0] - lam.I_view_azimuth_ground[b, 0, lane, M_DRIVER + 1]))
        assert d_rpv > d_lam


# ---- e. the node pin at natural scale: recorded ---------------------------------------------------------------------------------------------
def test_node_pin_on_the_device():
    """The configuration of tests/test_brdf_view_host.py (N = 64, L = 30, mu0 = 0.85, Rayleigh + HG(0.6), omega = 0.9, RPV): view
    cosines on the grid's nodes, every row; I_view against the device's own summed field on the upward lanes the model found
    untouched by any blend.  The model's figure is NODE_PIN (the series' next term, of the order of tol); the bound is twice it."""
    L, N = 30, 64
    c = G.experiment_column(O, N, L, 0.85, 0.0)
    with np.errstate(all="ignore"):
        dist, lanes, ok, ref = BV.node_pin(c, RPV)
    mv, idx = VN.node_views(c.mu, N)
    V = len(mv)
    r = SOS_Aer_batch([0.85], 0.3, 1.0, alb_aer=0.9, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.6, max_orders=64, nb_layers=L,
                      nb_angles=N, surface="brdf", brdf=RPV, view_mu=mv, view_levels=list(range(L)), brdf_view=True)
    assert V <= _lib.MAX_VIEWS and lanes >= 30 and not r.status.any()
    assert [int(r.n[0])] + [int(x) for x in r.bounce_orders[:, 0]] == ref["orders"]
    mx = np.max(np.abs(r.I))
    got = np.max(np.abs(r.I_view[0][:, V:] - r.I[0][:, idx[V:]])[:, ok]) / mx
    print("node pin on the device: %.3e of the field maximum on %d untouched upward lanes (model %.3e)" % (got, lanes, dist))
    assert got <= 2 * NODE_PIN


# ---- f. the cached handle afterwards ------------------------------------------------------------------------------------------------------
def test_the_cached_handle_solves_a_plain_batch_with_its_old_bits(monkeypatch):
    L, N = 24, 66
    kw = dict(KW, nb_layers=L, nb_angles=N)
    plain = lambda: SOS_Aer_batch(list(MU0S), 0.3, [0.1, 0.3, 0.5], view_mu=MU_VIEW, **kw)
    call = lambda: SOS_Aer_batch(list(MU0S), 0.3, 1.0, surface="brdf", brdf=RPV, view_mu=MU_VIEW, view_azimuths=PHI[:3], n_modes=3,
                                 brdf_view=True, **kw)
    same = lambda a, b: all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("I", "n", "status", "I_view"))
    before = plain()
    r = call()
    assert r.I_view_azimuth_ground is not None and same(before, plain())
    # an error raised inside the loop over the modes: the handle's matrices and targets are put back
    # (mode 0 calls the stage once for the beam and once per reflection; the call after the next is reflection 2 of mode 1)
    real, count, K = Solver.view_ground_device, [0], r.bounce_orders.shape[0]

    def failing(self, *a, **k):
        count[0] += 1
        if count[0] == K + 3:
            raise RuntimeError("injected")
        return real(self, *a, **k)
    inside = []
    real_modes = Solver.set_order_targets
    monkeypatch.setattr(Solver, "set_order_targets", lambda self, t: (inside.append(t), real_modes(self, t))[1])
    monkeypatch.setattr(Solver, "view_ground_device", failing)
    with pytest.raises(RuntimeError, match="injected"):
        call()
    monkeypatch.undo()
    assert count[0] == K + 3 and K >= 2 and inside[-1] is None       # (the last word on the targets was to clear them)
    assert same(before, plain())
    again = call()
    assert np.array_equal(again.I_view_azimuth, r.I_view_azimuth) and np.array_equal(again.I, r.I)
