"""Cox-Munk ocean ground on the device (csrc/brdf.hip, csrc/api_brdf.hip): the kind through all seven builder
entry points against the NumPy model of tests/cox_munk_np.py, the builders' bit guarantees, every refusal of the C ABI, the driver
against the model's series with the composed operators, mixed winds and the Lambertian limit bit for bit, the device chain over
the ground's modes against a direct azimuth-resolved solve in the linear regime, the mode and view drivers against the model's
mode series, and the glint seen from the specular view lane."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import azimuth_direct as D
import brdf_azimuth_np as BA
import brdf_np as G
import brdf_view_np as BV
import cox_munk_np as CM
import ross_li_np as RL
import sos_oracle as O
import view_azimuth_np as VA
import view_np as VN
from sosrt import _lib, inputs
from sosrt.main import SOS_Aer_batch
from test_gpu_azimuth import _close, _kind, _solver
from test_gpu_azimuth_direct import _accumulate
from test_gpu_brdf import columns, dev, dfull, host, run_beam, run_operator, sync
from test_gpu_brdf_azimuth import reflections, run_beam_modes, run_operator_modes
from test_gpu_brdf_view import grid_handle, run_view_beam, run_view_rows, view_cosines
from util import RTOL

pytestmark = pytest.mark.gpu

MU0S = (0.35, 0.6, 0.85)
INDEX = 1.34
F_ISO, F_GLINT = [0.0, 0.02, 0.05], [1.0, 0.9, 0.8]          # the columns' water-leaving / whitecap reflectance and glint weight
SCALE = 1e-6
SERIES = ("I", "n", "status", "bounces", "bounce_orders", "bounce_ratio")


def mx(a):
    return np.max(np.abs(a))


def glint(U, shadow=True):
    """the kind as the builders and the model name it"""
    return ("cox_munk", CM.slope_variance(U), INDEX, 1.0 if shadow else 0.0)


def ocean(b, U, shadow=True):
    """column b's composed ground as the model names it"""
    return ("ocean", F_ISO[b], F_GLINT[b], CM.slope_variance(U), INDEX, shadow)


def run_view_azimuth(s, brdf, mu0, mv, phi):
    d_mu0, d_phi, d_out = dev(mu0), dev(phi), dfull((len(phi), len(mu0), len(mv)), guard=4)
    sync()
    s.brdf_view_beam_azimuth_device(brdf[0], d_mu0.data_ptr(), mv, d_phi.data_ptr(), len(phi), d_out.data_ptr(), brdf[1:], B=len(mu0))
    out = host(d_out, s)
    assert np.all(np.isnan(out[-4:]))
    return out[:-4].reshape(len(phi), len(mu0), len(mv))


# ---- 1. the seven builders against the model; their bit guarantees ------------------------------------------------------------------------------
PHI_AT = np.array([0.0, 1e-9, 0.3, np.pi / 2, 2.0, np.pi - 1e-9, np.pi, 4.0, 2 * np.pi, -0.3])


@pytest.mark.parametrize("shadow", [True, False], ids=["shadow", "noshadow"])
@pytest.mark.parametrize("U", [2, 10])
@pytest.mark.parametrize("N", [32, 33])
def test_builders_against_the_model(N, U, shadow):
    """L = 24, B = 3, 65 azimuth nodes, modes 0..9 (a launch of eight modes and one of two, so both instantiations of the pair kernel
    run and a launch boundary falls inside the range), view cosines 0.01, 0.123, 0.35, 0.6, 1.0 and 12 nodes: every array within
    the GPU parity bound, 1e-10 of its maximum."""
    brdf = glint(U, shadow)
    s = grid_handle(N, L=24)
    mu = O.make_mu(N)
    mv, _ = view_cosines(N, 17)
    ms, nphi = list(range(10)), 65
    ref = {"operator": G.operator(mu, N, brdf, nphi),
           "beam": np.stack([G.beam_row(mu, N, m0, brdf, nphi) for m0 in MU0S]),
           "operator modes": BA.operator_modes(mu, N, brdf, ms, nphi),
           "beam modes": np.stack([BA.beam_modes(mu, N, m0, brdf, ms, nphi) for m0 in MU0S], axis=1),
           "view rows modes": BV.view_rows_modes(mu, N, mv, brdf, ms, nphi),
           "view beam modes": np.stack([BV.view_beam_modes(mv, m0, brdf, ms, nphi) for m0 in MU0S], axis=1),
           "view beam azimuth": np.stack([BV.view_beam_azimuth(mv, m0, brdf, PHI_AT) for m0 in MU0S], axis=1)}
    got = {"operator": run_operator(s, brdf, nphi), "beam": run_beam(s, brdf, MU0S, nphi),
           "operator modes": run_operator_modes(s, brdf, 0, 10, nphi), "beam modes": run_beam_modes(s, brdf, MU0S, 0, 10, nphi),
           "view rows modes": run_view_rows(s, brdf, mv, 0, 10, nphi), "view beam modes": run_view_beam(s, brdf, MU0S, mv, 0, 10, nphi),
           "view beam azimuth": run_view_azimuth(s, brdf, MU0S, mv, PHI_AT)}
    s.close()
    err = {k: mx(got[k] - ref[k]) / mx(ref[k]) for k in ref}
    print("N=%d U=%d shadow=%s: %s of their maxima" % (N, U, shadow, ", ".join("%s %.2e" % kv for kv in err.items())))
    for k in ref:
        assert got[k].shape == ref[k].shape and np.all(np.isfinite(got[k])), k
        assert err[k] <= RTOL, k
    assert np.all(got["view beam azimuth"] >= 0) and np.all(got["beam"] > 0)
    # the specular direction is phi = pi: on the lane mu_view = mu0 = 0.6 the value there is F(mu0) / (4 sigma2 mu0^2) S
    peak = CM.fresnel(0.6) / (4 * brdf[1] * 0.36) * CM.shadowing(0.6, 0.6, brdf[1], shadow)
    assert abs(got["view beam azimuth"][6, 1, 3] - peak) <= 1e-12 * peak and got["view beam azimuth"][0, 1, 3] < 1e-3 * peak


@pytest.mark.parametrize("N", [32, 33])
def test_builders_bit_guarantees(N):
    """Mode 0 of the mode builders has the bits of the azimuth-mean builders; a mode's bits do not depend on how many modes a launch
    takes or where it starts; a view cosine equal to a node has the node's bits; a beam row's bits do not depend on B; sign_odd is
    an exact negation of the odd modes."""
    brdf = glint(2)
    s = grid_handle(N, L=24)
    mv, nodes = view_cosines(N, 17)
    off = len(mv) - len(nodes)
    nphi = 65
    R, r0 = run_operator_modes(s, brdf, 0, 10, nphi), run_beam_modes(s, brdf, MU0S, 0, 10, nphi)
    Rv, r0v = run_view_rows(s, brdf, mv, 0, 10, nphi), run_view_beam(s, brdf, MU0S, mv, 0, 10, nphi)
    assert np.array_equal(R[0], run_operator(s, brdf, nphi)) and np.array_equal(r0[0], run_beam(s, brdf, MU0S, nphi))
    for m in (0, 3, 7, 8, 9):
        assert np.array_equal(run_operator_modes(s, brdf, m, 1, nphi)[0], R[m]), m
        assert np.array_equal(run_beam_modes(s, brdf, MU0S, m, 1, nphi)[0], r0[m]), m
        assert np.array_equal(run_view_rows(s, brdf, mv, m, 1, nphi)[0], Rv[m]), m
        assert np.array_equal(run_view_beam(s, brdf, MU0S, mv, m, 1, nphi)[0], r0v[m]), m
    assert np.array_equal(run_operator_modes(s, brdf, 2, 5, nphi), R[2:7]) and np.array_equal(run_beam_modes(s, brdf, MU0S, 5, 5, nphi), r0[5:])
    assert np.array_equal(run_view_rows(s, brdf, mv, 1, 9, nphi), Rv[1:]) and np.array_equal(run_view_beam(s, brdf, MU0S, mv, 7, 2, nphi), r0v[7:9])
    assert np.array_equal(Rv[:, off:], R[:, nodes]) and np.array_equal(r0v[:, :, off:], r0[:, :, nodes])
    assert np.array_equal(run_beam_modes(s, brdf, MU0S[:1], 0, 10, nphi), r0[:, :1])
    assert np.array_equal(run_view_beam(s, brdf, MU0S[:1], mv, 0, 10, nphi), r0v[:, :1])
    sgn = np.array([(-1.0) ** m for m in range(10)])[:, None, None]
    assert np.array_equal(run_operator_modes(s, brdf, 0, 10, nphi, sign_odd=True), sgn * R)
    assert np.array_equal(run_view_rows(s, brdf, mv, 0, 10, nphi, sign_odd=True), sgn * Rv)
    assert np.any(R[1::2] != 0)
    # the value at an azimuth itself on a lane that is a node of the grid: the same whether the cosine comes as a view cosine alone
    at = run_view_azimuth(s, brdf, MU0S, mv, PHI_AT)
    assert np.array_equal(run_view_azimuth(s, brdf, MU0S, mv[off:], PHI_AT), at[:, :, off:])
    s.close()


# ---- 2. refusals at the C ABI: nothing is written ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    L, N = 24, 33
    M1, V, Gd = N - 1, 5, 7
    s = grid_handle(N, L=L)
    lib = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    d_R, d_r0 = dfull((4, M1, M1), guard=Gd), dfull((4, 3, M1), guard=Gd)
    d_mu0 = dev(MU0S)
    P = lambda *v: (ctypes.c_double * len(v))(*v)
    mv = (ctypes.c_double * V)(0.01, 0.123, 0.35, 0.6, 1.0)
    CMK = _lib.BRDF_COX_MUNK
    assert CMK == 4
    entry = {
        "operator": lambda kind, p, n: lib.sosrt_brdf_operator_dev(s._h, kind, p, n, 65, vp(d_R)),
        "beam": lambda kind, p, n: lib.sosrt_brdf_beam_dev(s._h, 3, kind, p, n, 65, vp(d_mu0), vp(d_r0)),
        "operator modes": lambda kind, p, n: lib.sosrt_brdf_operator_modes_dev(s._h, kind, p, n, 65, 1, 4, 1, vp(d_R)),
        "beam modes": lambda kind, p, n: lib.sosrt_brdf_beam_modes_dev(s._h, 3, kind, p, n, 65, 1, 4, vp(d_mu0), vp(d_r0)),
        "view rows": lambda kind, p, n: lib.sosrt_brdf_view_rows_modes_dev(s._h, kind, p, n, 65, 1, 4, 0, V, mv, vp(d_R)),
        "view beam": lambda kind, p, n: lib.sosrt_brdf_view_beam_modes_dev(s._h, 3, kind, p, n, 65, 1, 4, vp(d_mu0), V, mv, vp(d_r0)),
        "view azimuth": lambda kind, p, n: lib.sosrt_brdf_view_beam_azimuth_dev(s._h, 3, kind, p, n, vp(d_mu0), V, mv, 2, vp(d_mu0), vp(d_r0)),
    }
    nan, inf = float("nan"), float("inf")
    bad = {"nparams 0": (None, 0, b"nparams"), "nparams 1": (P(0.02), 1, b"nparams"), "nparams 2": (P(0.02, 1.34), 2, b"nparams"),
           "nparams 4": (P(0.02, 1.34, 1.0, 0.0), 4, b"nparams"), "null params": (None, 3, b"null params"),
           "sigma2 0": (P(0.0, 1.34, 1.0), 3, b"sigma2"), "sigma2 < 0": (P(-0.02, 1.34, 1.0), 3, b"sigma2"),
           "sigma2 nan": (P(nan, 1.34, 1.0), 3, b"sigma2"), "sigma2 inf": (P(inf, 1.34, 1.0), 3, b"sigma2"),
           "index 1": (P(0.02, 1.0, 1.0), 3, b"refractive_index"), "index < 1": (P(0.02, 0.75, 1.0), 3, b"refractive_index"),
           "index nan": (P(0.02, nan, 1.0), 3, b"refractive_index"), "index inf": (P(0.02, inf, 1.0), 3, b"refractive_index"),
           "shadow 0.5": (P(0.02, 1.34, 0.5), 3, b"shadow"), "shadow 2": (P(0.02, 1.34, 2.0), 3, b"shadow"),
           "shadow -1": (P(0.02, 1.34, -1.0), 3, b"shadow"), "shadow nan": (P(0.02, 1.34, nan), 3, b"shadow")}

    def untouched():
        s.synchronize()
        sync()
        return bool(torch.isnan(d_R).all()) and bool(torch.isnan(d_r0).all())

    for name, call in entry.items():
        for what, (p, n, word) in bad.items():
            assert call(CMK, p, n) == _lib.E_INVALID, (name, what)
            assert word in lib.sosrt_last_error(), (name, what, lib.sosrt_last_error())
            assert untouched(), (name, what)
        for kind in (-1, 5, 7, 9):
            assert call(kind, P(0.02, 1.34, 1.0), 3) == _lib.E_INVALID and b"unknown BRDF kind" in lib.sosrt_last_error(), (name, kind)
            assert untouched(), (name, kind)
    ok = P(0.02, 1.34, 1.0)
    assert lib.sosrt_brdf_operator_dev(s._h, CMK, ok, 3, 2, vp(d_R)) == _lib.E_INVALID and b"nphi" in lib.sosrt_last_error()
    assert lib.sosrt_brdf_operator_dev(s._h, CMK, ok, 3, 65, None) == _lib.E_INVALID and untouched()
    assert lib.sosrt_brdf_beam_dev(s._h, 4, CMK, ok, 3, 65, vp(d_mu0), vp(d_r0)) == _lib.E_INVALID and untouched()
    s.set_columns_single_slab([0.5, 0.6, 0.7], 0.9, 0.3)
    assert entry["operator"](CMK, ok, 3) == _lib.E_INVALID and b"single slab" in lib.sosrt_last_error() and untouched()
    s.close()
    # valid calls through every entry point write their outputs and leave the guard elements behind them alone
    s = grid_handle(N, L=L)
    sizes = {"operator": (d_R, M1 * M1), "beam": (d_r0, 3 * M1), "operator modes": (d_R, 4 * M1 * M1), "beam modes": (d_r0, 4 * 3 * M1),
             "view rows": (d_R, 4 * M1 * V), "view beam": (d_r0, 4 * 3 * V), "view azimuth": (d_r0, 2 * 3 * V)}
    for name, (t, n) in sizes.items():
        t.fill_(float("nan"))
        sync()
        for shadow in (0.0, 1.0):
            assert entry[name](CMK, P(0.02, 1.34, shadow), 3) == 0, name
        s.synchronize()
        sync()
        assert bool(torch.isfinite(t[:n]).all()) and bool(torch.isnan(t[n:]).all()), name
    s.close()


# ---- 3. the driver against the model's series ----------------------------------------------------------------------------------------------------
def driver(L, N, brdf, grd_alb=1.0, **kw):
    cols = columns(L, N)
    c = cols[0]
    return SOS_Aer_batch(list(MU0S), 0.3, grd_alb, tauStar_atm=0.124, alb_atm=1.0, alb_aer=0.9, nb_layers=L, nb_angles=N,
                         P_atm=c.P_atm, P_aer=c.P_aer, P0_atm=np.stack([x.P0_atm for x in cols]), P0_aer=np.stack([x.P0_aer for x in cols]),
                         max_orders=64, surface="brdf", brdf=brdf, **kw)


@functools.lru_cache(maxsize=None)
def model_operators(N, U, shadow=True):
    """(Rs [K, i, j], r0s [K, b, i]) of the model for the two terms of the ocean ground; never changed"""
    mu = O.make_mu(N)
    terms = ("lambertian", glint(U, shadow))
    Rs = np.stack([G.operator(mu, N, t) for t in terms])
    r0s = np.stack([np.stack([G.beam_row(mu, N, m0, t) for m0 in MU0S]) for t in terms])
    Rs.setflags(write=False)
    r0s.setflags(write=False)
    return Rs, r0s


WEIGHTS = np.stack([F_ISO, F_GLINT], axis=1)                 # [b, k]


@functools.lru_cache(maxsize=None)
def model_series(L, N, U):
    Rs, r0s = model_operators(N, U)
    with np.errstate(all="ignore"):
        out = RL.bounce_solve_columns(O, columns(L, N), np.tensordot(WEIGHTS, Rs, axes=1), np.einsum("bk,kbi->bi", WEIGHTS, r0s))
    out[0].setflags(write=False)
    return out


@pytest.mark.parametrize("U", [2, 10])
@pytest.mark.parametrize("L,N", [(24, 33), (24, 66)])
def test_driver_against_the_model_series(L, N, U):
    """mu0 = (0.35, 0.6, 0.85), every column its own f_iso and f_glint, against ross_li_np.bounce_solve_columns with the composed
    operators on the oracle: equal bounce counts and status, the field within RTOL of its maximum, the ratios as section 24's driver
    test bounds them.  At N = 33 the glint's peak among so few lanes runs the mu -> 0 search of some columns off the ground row
    (COL_INDEXERROR, the reference's IndexError) in the model and on the device alike; at N = 66 every status is 0."""
    ref, bounces, ratio, status = model_series(L, N, U)
    r = driver(L, N, ("cox_munk", float(U), INDEX, F_ISO, F_GLINT), raise_on_error=False)
    err = [float(mx(r.I[b] - ref[b]) / mx(ref[b])) for b in range(3)]
    print("L=%d N=%d U=%d: bounces %s (model %s), status %s (model %s), field vs the model's series %s of the maximum"
          % (L, N, U, r.bounces, bounces, r.status, status, ["%.2e" % e for e in err]))
    assert np.all(np.isfinite(r.I))
    assert np.array_equal(r.bounces, bounces) and np.array_equal(r.status, status)
    assert N < 64 or not status.any()
    assert max(err) <= RTOL
    assert np.all(np.abs(r.bounce_ratio - ratio) <= 1e-6 * np.maximum(ratio, 1e-12))
    # the albedos on the grid's quadrature, from the model's rows
    mu = O.make_mu(N)
    Rs, r0s = model_operators(N, U)
    bsa = np.array([RL.black_sky_albedo(mu, N, r0s[:, b], WEIGHTS[b]) for b in range(3)])
    wsa = np.array([RL.white_sky_albedo(mu, N, Rs, WEIGHTS[b]) for b in range(3)])
    print("black-sky %s (model %s), white-sky %s (model %s)" % (r.black_sky_albedo, bsa, r.white_sky_albedo, wsa))
    assert np.max(np.abs(r.black_sky_albedo - bsa)) <= RTOL and np.max(np.abs(r.white_sky_albedo - wsa)) <= RTOL
    assert abs(bsa[0] - CM.black_sky_grid(mu, N, MU0S[0], glint(U))) <= 1e-15


# ---- 4. mixed winds; the Lambertian limit; the other drivers ------------------------------------------------------------------------------------
KW = dict(alb_aer=0.95, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.5, max_orders=64)
PHI = 2 * np.pi * np.arange(14) / 14                         # phi = 0 is node 0, phi = pi node 7


def same(a, b, names, cols=slice(None)):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert x is not None and y is not None, k
        if k in ("bounce_orders", "mode_status", "view_mode_status"):
            assert np.array_equal(x[:, cols], y[:, cols]), k
        else:
            assert np.array_equal(x[cols], y[cols]), k


@pytest.mark.parametrize("L,N", [(24, 33), (24, 66)])
def test_a_column_of_a_mixed_wind_batch_has_the_bits_of_its_own_wind(L, N):
    """Winds (2, 10, 2): two glint terms, every column's weight 0 on the other's; against the two batches at one wind (one glint term
    each), column by column, in the field, the counts, the albedos and the azimuth-resolved radiance"""
    call = lambda wind: SOS_Aer_batch(list(MU0S), 0.3, 1.0, nb_layers=L, nb_angles=N, surface="brdf", brdf=("cox_munk", wind, INDEX, F_ISO, F_GLINT),
                                      azimuths=PHI, n_modes=6, brdf_modes=True, raise_on_error=False, **KW)
    mixed, calm, rough = call([2.0, 10.0, 2.0]), call(2.0), call([10.0] * 3)
    assert mixed.bounce_orders.shape == calm.bounce_orders.shape == rough.bounce_orders.shape      # (every column runs the batch's bounces)
    names = SERIES + ("black_sky_albedo", "white_sky_albedo", "I_azimuth", "mode_status")
    same(mixed, calm, names, [0, 2])
    same(mixed, rough, names, [1])
    assert mx(calm.I[1] - rough.I[1]) > 1e-6 * mx(calm.I[1]) and mx(calm.I_azimuth[1] - rough.I_azimuth[1]) > 1e-4 * mx(calm.I_azimuth[1])


ALB = [0.0, 0.3, 0.8]


def lambertian_pair(L, N, **kw):
    """(at N = 33 the mu -> 0 search leaves the ground row of two columns over either ground: the statuses are compared, not raised)"""
    kw = dict(kw, raise_on_error=False)
    a =SOS_Aer_batch(list(MU0S), 0.3, 1.0, nb_layers=L, nb_angles=N, surface="brdf", brdf=("cox_munk", 5.0, INDEX, ALB, 0.0), **KW, **kw)
    b = SOS_Aer_batch(list(MU0S), 0.3, ALB, nb_layers=L, nb_angles=N, surface="brdf", brdf="lambertian", **KW, **kw)
    return a, b


@pytest.mark.parametrize("L,N", [(24, 33), (24, 66)])
def test_without_glint_the_ocean_is_the_lambertian_ground(L, N):
    """('cox_munk', U, n, a, 0) is brdf='lambertian', grd_alb=a bit for bit, as Ross-Li (a, 0, 0) is"""
    a, b = lambertian_pair(L, N)
    same(a, b, SERIES)
    assert b.bounces.max() >= 2 and b.black_sky_albedo is None
    on_grid = np.array(ALB) * np.sum(RL.up_weights(O.make_mu(N), N))
    assert a.black_sky_albedo.shape == (3,) and np.max(np.abs(a.black_sky_albedo - on_grid)) <= 1e-13


def test_without_glint_the_ocean_is_the_lambertian_ground_over_the_modes():
    a, b = lambertian_pair(24, 33, azimuths=PHI, n_modes=6, brdf_modes=True)
    same(a, b, SERIES + ("I_azimuth", "mode_status"))


@pytest.mark.parametrize("first", [None, "exact", "modes"])
def test_without_glint_the_ocean_is_the_lambertian_ground_at_the_view_lanes(first):
    L = 24
    kw = dict(view_mu=[0.123, 0.35, 0.6, 1.0], view_levels=(0, L // 3, -1), brdf_view=True)
    if first:
        kw.update(view_azimuths=PHI, n_modes=6, view_first_order=first)
    a, b = lambertian_pair(L, 33, **kw)
    same(a, b, SERIES + ("I_view", "I_view_first", "I_view_scattered", "I_view_ground"))
    if first:
        same(a, b, ("I_view_azimuth", "I_view_azimuth_first", "I_view_azimuth_scattered", "I_view_azimuth_ground", "view_mode_status"))


def test_the_other_drivers_reach_the_same_series():
    from sosrt import forcing, ocean
    from sosrt.main import SOS_Aer, SOS_Aer_layers, solve_batch_device
    W = float(ocean.whitecap_fraction(8.0))
    brdf = ("cox_munk", 8.0, INDEX, W * 0.22 + 0.01, 1 - W)
    kw = dict(tauStar_atm=0.124, alb_atm=1.0, nb_layers=24, nb_angles=66, max_orders=64, surface="brdf", brdf=brdf)
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
    flux = forcing.toa_net_flux(0.6, 0.124, [0.3], 1.0, 1.0, [0.9], nb_layers=24, nb_angles=66, max_orders=64, surface="brdf", brdf=brdf)
    black = forcing.toa_net_flux(0.6, 0.124, [0.3], 0.0, 1.0, [0.9], nb_layers=24, nb_angles=66, max_orders=64)
    print("net TOA flux over the ocean %s, over a black ground %s" % (flux, black))
    assert np.all(np.isfinite(flux)) and np.all(np.abs(flux) < np.abs(black))     # a reflecting ground sends more back to space
    # the default path keeps its bytes around a call over the ocean
    plain = lambda: SOS_Aer_batch(list(MU0S), 0.3, [0.1, 0.3, 0.5], tauStar_atm=0.124, nb_layers=24, nb_angles=66, max_orders=64)
    before = plain()
    SOS_Aer_batch(list(MU0S), 0.3, 1.0, **kw)
    after = plain()
    assert np.array_equal(before.I, after.I) and np.array_equal(before.n, after.n) and before.black_sky_albedo is None


# ---- 5. the modes: the device chain against a direct azimuth-resolved solve in the linear regime --------------------------------------------------
def test_device_chain_against_the_direct_solve():
    """test_gpu_brdf_azimuth's case with the glint at U = 10 in place of RPV and the modes 0..32: Rayleigh + HG g = 0.5, mu0 = 0.6,
    L = 16, N = 24, P0 and the beam rows scaled by 1e-6; the direct solve over rho(a, b, phi) itself on 72 uniform azimuths runs the
    same counts and its modes 0..32 are the comparison, at RTOL -- the bound of the RPV and Ross-Li chains.  The modes of rho(0.6,
    0.6, .) fall from 5e-2 at m = 0 to 2e-5 at m = 16 and 2e-14 at m = 32: the 37 nodes of the half circle carry all of them."""
    L, N, nq, M, U = 16, 24, 72, 32, 10
    brdf = glint(U)
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
        s.brdf_operator_modes_device("cox_munk", d_R.data_ptr(), 0, M + 1, brdf[1:], nphi, sign_odd=True)
        s.brdf_beam_modes_device("cox_munk", d_mu0.data_ptr(), d_r0.data_ptr(), 0, M + 1, brdf[1:], nphi, B=1)
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
        _, Iq = BA.direct_solve(gr, fa, fr, brdf, nq, n, n_k, SCALE, log=log)
    log.oracle = oracle_log
    assert log.first_test_everywhere()
    ref = D.synthesize(D.project(Iq, M), phi)
    print("L=%d N=%d U=%d: n = %d, reflections %s, device chain over modes 0..%d vs the direct solve's %.3e of the maximum"
          % (L, N, U, n, n_k, M, mx(got - ref) / mx(ref)))
    _close(got, ref, RTOL, "L = %d, N = %d, M = %d, n = %d, reflections %s" % (L, N, M, n, n_k))
    # the glint reaches the result: at the surface, on the upward lane nearest mu0, forward (phi = pi) outshines back-scatter
    lane = N + int(np.argmin(np.abs(gr.geo.mu[N:] - 0.6)))
    assert got[L - 1, lane, nq // 2] > 2 * got[L - 1, lane, 0]


# ---- 6. the mode and view drivers at natural scale against the model's mode series ------------------------------------------------------------------
M_DRIVER = 6
L_D, N_D, U_D = 24, 66, 10
OCEAN_CALL = ("cox_munk", float(U_D), INDEX, F_ISO, F_GLINT)
FNS = lambda: (inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0])


def test_modes_driver_against_the_model_series():
    """SOS_Aer_batch(azimuths, brdf_modes) over the ocean against the model's mode series over rho = f_iso + f_glint rho_glint itself,
    run with the device's own order and reflection counts: RTOL, the bound of the RPV and Ross-Li cases"""
    kw = dict(KW, nb_layers=L_D, nb_angles=N_D, surface="brdf", brdf=OCEAN_CALL)
    r = SOS_Aer_batch(list(MU0S), 0.3, 1.0, azimuths=PHI, n_modes=M_DRIVER, brdf_modes=True, **kw)
    plain = SOS_Aer_batch(list(MU0S), 0.3, 1.0, **kw)
    same(r, plain, SERIES)
    assert not r.mode_status.any()
    assert mx(r.I_azimuth.mean(axis=-1) - r.I[:, [0, L_D - 1]]) <= 1e-12 * mx(r.I)
    fa, fr = FNS()
    for b, mu0 in enumerate(MU0S):
        with np.errstate(all="ignore"):
            Im, status = BA.mode_series(BA.black_three_zone(mu0, L_D, N_D), fa, fr, ocean(b, U_D), M_DRIVER, 25, int(r.n[b]), r.bounce_orders[:, b])
        ref = D.synthesize(Im[:, [0, L_D - 1]], PHI)
        print("mu0=%.2f: n = %d, reflections %s, I_azimuth vs the model's mode series %.3e of the maximum"
              % (mu0, r.n[b], r.bounce_orders[:, b], mx(r.I_azimuth[b] - ref) / mx(ref)))
        assert status == 0
        _close(r.I_azimuth[b], ref, RTOL, "mu0 = %g" % mu0)


MU_VIEW = np.array([0.01, 0.35, 0.6, 0.85, 1.0])             # the limb, the columns' mu0 (their specular lanes), the nadir


@pytest.mark.parametrize("first", ["exact", "modes"])
def test_view_azimuth_driver_and_the_glint_at_the_specular_lane(first):
    """view_mu + brdf_view + view_azimuths over the ocean.  The scattered and the ground's term at (view lane, azimuth) against the
    model's mode series with the device's counts, at RTOL; I_view* are the bits of the call without view_azimuths.  With 'exact' the
    beam's single reflection is rho at the azimuth itself: on the lane mu_view = mu0 at phi = pi, the specular point, the ground's
    term minus the model's diffuse part is f_glint rho_glint(mu0, mu0, pi) exp(-tau* / mu0) exp(-(tau* - tau) / mu0) (+ f_iso's
    share), the model's beam normalisation being 1; the peak sits at phi = pi and not at 0."""
    L, N = L_D, N_D
    lev = [0, L // 3, L - 1]
    V = len(MU_VIEW)
    kw = dict(KW, nb_layers=L, nb_angles=N, surface="brdf", brdf=OCEAN_CALL, view_mu=MU_VIEW, view_levels=(0, L // 3, -1), brdf_view=True)
    r = SOS_Aer_batch(list(MU0S), 0.3, 1.0, view_azimuths=PHI, n_modes=M_DRIVER, view_first_order=first, **kw)
    base = SOS_Aer_batch(list(MU0S), 0.3, 1.0, **kw)
    same(r, base, SERIES + ("I_view", "I_view_first", "I_view_scattered", "I_view_ground"))
    assert not r.view_mode_status.any() and not r.status.any()
    assert np.array_equal(r.I_view_azimuth, r.I_view_azimuth_first + r.I_view_azimuth_scattered + r.I_view_azimuth_ground)
    fa, fr = FNS()
    for b in range(3):
        brdf = ocean(b, U_D)
        c, gr = BV.black_column(MU0S[b], L, N)
        with np.errstate(all="ignore"):
            out, status = BV.mode_series_view(c, gr, fa, fr, brdf, M_DRIVER, 25, int(r.n[b]), tuple(int(x) for x in r.bounce_orders[:, b]),
                                              MU_VIEW, VN.QUAD_GRID, ground_scale=1.0, beam_in_modes=first == "modes")
        assert status == 0
        diffuse = ground = VA.synthesize(out["ground"][:, lev], PHI)
        if first == "exact":
            ground = diffuse + np.moveaxis(BV.beam_ground(gr, brdf, MU_VIEW, PHI)[:, lev], 0, -1)
        scat = VA.synthesize(out["scattered"][:, lev], PHI)
        m = mx(scat + ground)
        e_s, e_g = mx(r.I_view_azimuth_scattered[b] - scat) / m, mx(r.I_view_azimuth_ground[b] - ground) / m
        e_0 = mx(r.I_view_ground[b] - out["ground"][0][lev]) / m if first == "modes" else 0.0
        lane, mu0 = V + 1 + b, MU0S[b]                        # MU_VIEW[1 + b] = MU0S[b]
        g = r.I_view_azimuth_ground[b, :, lane]
        print("%s mu0=%.2f: scattered %.3e, ground %.3e, azimuth-mean ground %.3e of their maximum; the ground's term at TOA on the "
              "specular lane, phi = 0 / pi: %.4e / %.4e" % (first, mu0, e_s, e_g, e_0, g[0, 0], g[0, 7]))
        assert e_s <= RTOL and e_g <= RTOL and e_0 <= RTOL
        if first == "exact":
            tau = gr.tau
            beam = (F_ISO[b] + F_GLINT[b] * CM.rho_glint(mu0, mu0, np.pi, CM.slope_variance(U_D), INDEX, True)) \
                * np.exp(-tau[-1] / mu0) * np.exp(-(tau[-1] - tau[lev]) / mu0)
            assert mx(g[:, 7] - diffuse[:, lane, 7] - beam) <= RTOL * m
            assert np.all(np.argmax(g, axis=-1) == 7) and np.all(g[:, 7] > g[:, 0])
