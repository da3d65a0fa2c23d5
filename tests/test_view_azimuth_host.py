"""Azimuth-resolved view radiance (SOS_Aer_batch(..., view_mu=, view_azimuths=)), CPU tier: the four symbols of
the C ABI, the NumPy model of the stage (tests/view_azimuth_np.py) pinned to the mode builders at the nodes and to a direct
view radiance that never goes through a Fourier mode, the exact first order against the modes', and the checks the Python layer
makes before any handle exists.  No GPU."""
import os
import re

import numpy as np
import pytest

import azimuth_direct as AD
import azimuth_np as A
import sos_oracle as O
import view_azimuth_np as VA
import view_np as VN
from sosrt import inputs
from util import RTOL, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sosrt_phase_rows_modes_dev": 10, "sosrt_phase_p0_rows_modes_dev": 11, "sosrt_phase_p0_rows_azimuth_dev": 10,
           "sosrt_view_azimuth_accumulate_dev": 9}


def _err(a, b):
    """max |a - b| / max |b| (tests/test_gpu_azimuth.py `_close`): modes and azimuth-resolved fields cross zero."""
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


def test_symbols_and_version():
    from sosrt import _lib
    header = open(os.path.join(ROOT, "include", "sosrt.h")).read()
    L = _lib.lib()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in sosrt.h" % name
        assert name in _lib.SIGNATURES, "%s is not bound in sosrt._lib" % name
        assert getattr(L, name) is not None
        declared = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
        assert len(_lib.SIGNATURES[name][1]) == declared == nargs, name
    assert L.sosrt_version() == 105
    from sosrt.solver import Solver
    for meth in ("phase_rows_modes_device", "phase_p0_rows_modes_device", "phase_p0_rows_azimuth_device", "view_azimuth_accumulate_device"):
        assert callable(getattr(Solver, meth))


@pytest.mark.parametrize("N", [32, 33])
def test_model_mode_rows_at_nodes_are_the_mode_matrices(N):
    mu = O.make_mu(N)
    mu0 = np.array([0.3, 0.6])
    ms, nphi = [1, 2, 3, 4, 7], 25
    for name, g in (("rayleigh", 0.0), ("hg", 0.7), ("fwc", 0.0)):
        fn = inputs._scalar_phase(name, g)[0]
        ref = A.phase_modes(fn, mu, ms, nphi)
        got = VA.mode_rows(fn, mu, mu, ms, nphi)
        assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(A.phase_modes(fn, mu, [0], nphi)))
        assert np.max(np.abs(VA.solve_rows(fn, mu, mu, ms, nphi) - A.solve_modes(fn, mu, ms, nphi))) <= 1e-12 * np.max(np.abs(ref))
        p0 = VA.mode_p0_rows(fn, mu, mu0, mu, ms, nphi)
        for b in range(2):
            r0 = A.phase_p0_modes(fn, mu, mu0[b], ms, nphi)
            assert np.max(np.abs(p0[:, b] - r0)) <= 1e-12 * np.max(np.abs(A.phase_p0_modes(fn, mu, mu0[b], [0], nphi)))
    assert not np.any(VA.mode_rows(None, mu, mu, ms, nphi)) and not np.any(VA.mode_p0_rows(None, mu, mu0, mu, ms, nphi))


# ---- the per-mode view stage against a direct view radiance, in the linear regime of DESIGN section 11 -------------------------------
SCALE = 1e-6
MU_VIEW = np.array([0.01, 0.37, 0.83])                          # none is a node of N = 32
PHI_VIEW = np.array([0.0, 0.7, np.pi / 2, 2.4, np.pi])
K_ORDERS = 4                                                    # orders 1..3 feed the source: the stage returns orders 2..4


@pytest.fixture(scope="module", params=["three_zone", "single_slab"])
def linear_case(request):
    """Rayleigh, M = 2 (all its modes), L = 24, N = 32: the direct field on nq = 8 nodes and the mode fields on 5 ring nodes
    (the same quadrature), orders 1..K_ORDERS - 1, with P0 scaled so that every blend search stops at its first test."""
    L, N, nq, M = 24, 32, 8, 2
    fn = inputs._scalar_phase("rayleigh")[0]
    c, geo = VA.three_zone(0.6, L, N) if request.param == "three_zone" else VA.single_slab(0.55, L, N)
    with AD.record_blend() as log:
        _, Iq = AD.direct_solve(geo, fn, None, nq, K_ORDERS - 1, SCALE)
        Im = AD.mode_fields(geo, fn, None, M, nq // 2 + 1, K_ORDERS - 1, SCALE)
    assert log and all(log)
    return request.param, c, geo, fn, Iq, Im, nq // 2 + 1


@pytest.mark.parametrize("quad", [VN.QUAD_GRID, VN.QUAD_LINEAR], ids=["grid", "linear"])
def test_mode_synthesis_is_the_direct_view_radiance(linear_case, quad):
    name, c, geo, fn, Iq, Im, nphi = linear_case
    surface = "specular" if name == "three_zone" else None
    first_d, scat_d = VA.direct_view(c, geo, fn, None, Iq, MU_VIEW, PHI_VIEW, quad, SCALE, surface=surface)
    scat_m = [VA.mode_scattered(c, fn, fn, Im[m], m, MU_VIEW, quad, nphi, surface=surface) for m in range(len(Im))]
    p0 = [SCALE * VA.mode_p0(fn, c.mu, c.mu0, MU_VIEW, m, nphi) for m in range(len(Im))]
    if name == "three_zone":
        first_m = [VN.first_order(c, p, p, MU_VIEW) for p in p0]
    else:
        first_m = [VN.first_order_single_slab(c.tau, c.tauStar_tot, c.mu0, c.alb_atm, p, MU_VIEW) for p in p0]
    scat = np.moveaxis(VA.synthesize(np.stack(scat_m), PHI_VIEW), -1, 0)
    first = np.moveaxis(VA.synthesize(np.stack(first_m), PHI_VIEW), -1, 0)
    e_s, e_f, e_t = _err(scat, scat_d), _err(first, first_d), _err(first + scat, first_d + scat_d)
    print("%s: scattered %.2e, first order %.2e, total %.2e of the maximum; scattered / first %.2e"
          % (name, e_s, e_f, e_t, np.max(np.abs(scat_d)) / np.max(np.abs(first_d))))
    assert np.max(np.abs(scat_d)) > 1e-3 * np.max(np.abs(first_d))        # (the orders n >= 2 are a visible part of the total)
    assert e_s <= RTOL and e_f <= RTOL and e_t <= RTOL
    # the fold's sign matters: with rows^m itself the odd mode has the wrong sign off the grid too
    bad = VN.transport(c, VN.source(c, VA.mode_rows(fn, c.mu, VN.signed(MU_VIEW), [1], nphi)[0],
                                    VA.mode_rows(fn, c.mu, VN.signed(MU_VIEW), [1], nphi)[0] if name == "three_zone" else None, Im[1]),
                       MU_VIEW, quad, surface=surface)
    wrong = np.moveaxis(VA.synthesize(np.stack([scat_m[0], bad, scat_m[2]]), PHI_VIEW), -1, 0)
    assert _err(wrong, scat_d) > 1e-4


# ---- the exact first order ---------------------------------------------------------------------------------------------------------
def _first_case():
    N, L = 32, 24
    c = O.make_column(0.6, 120, 25, 17, L, 0.124, 0.3, 0.15, 1.0, 0.95, N, np.zeros(2 * N), np.zeros((2 * N, 2 * N)), np.zeros(2 * N),
                      np.zeros((2 * N, 2 * N)))
    return c, VN.signed(MU_VIEW)


def _first_modes(c, fa, fr, M, nphi, phi):
    vals = [VN.first_order(c, VA.mode_p0(fa, c.mu, c.mu0, MU_VIEW, m, nphi), VA.mode_p0(fr, c.mu, c.mu0, MU_VIEW, m, nphi), MU_VIEW)
            for m in range(M + 1)]
    return np.moveaxis(VA.synthesize(np.stack(vals), phi), -1, 0)


def _first_exact(c, fa, fr, sgn, phi):
    pa, pr = VA.p0_exact(fa, c.mu, [c.mu0], sgn, phi)[:, 0], VA.p0_exact(fr, c.mu, [c.mu0], sgn, phi)[:, 0]
    return np.stack([VN.first_order(c, pa[i], pr[i], MU_VIEW) for i in range(len(phi))])


def test_exact_first_order_is_the_modes_for_rayleigh():
    c, sgn = _first_case()
    fn = inputs._scalar_phase("rayleigh")[0]
    exact = _first_exact(c, fn, fn, sgn, PHI_VIEW)
    modes = _first_modes(c, fn, fn, 2, 25, PHI_VIEW)
    assert np.max(np.abs(exact - modes)) <= 1e-12 * np.max(np.abs(exact))


def test_ring_is_the_mean_over_48_uniform_azimuths():
    """The 25-node trapezoid of p(c(phi)) + p(c(phi + pi)) on [0, pi] is (pi / 24) times the sum over phi = 2 pi k / 48: the end
    nodes carry half weight and each is shared by the two halves of the circle."""
    phi = np.linspace(0, np.pi, 25)
    w = np.zeros(25)
    w[:-1] += np.diff(phi) / 2
    w[1:] += np.diff(phi) / 2
    full = np.zeros(48)
    for q in range(25):                                           # node q of the ring serves azimuths q and q + 24 (mod 48)
        full[q % 48] += w[q]
        full[(q + 24) % 48] += w[q]
    assert np.max(np.abs(full - np.pi / 24)) < 1e-15


@pytest.mark.parametrize("name,g", [("rayleigh", 0.0), ("hg", 0.5), ("fwc", 0.0)])
def test_exact_first_order_mean_over_48_azimuths_is_the_plain_first_order(name, g):
    c, sgn = _first_case()
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase(name, g)[0]
    phi48 = 2 * np.pi * np.arange(48) / 48
    mean = _first_exact(c, fa, fr, sgn, phi48).mean(axis=0)
    plain = VN.first_order(c, VN.phase_p0_rows(fa, c.mu, [c.mu0], sgn)[0], VN.phase_p0_rows(fr, c.mu, [c.mu0], sgn)[0], MU_VIEW)
    assert_close(mean, plain, 1e-12, "mean of the exact first order")
    assert_close(VA.p0_exact(fr, c.mu, [0.3, c.mu0], sgn, phi48).mean(axis=0), VN.phase_p0_rows(fr, c.mu, [0.3, c.mu0], sgn), 1e-12,
                 "mean of the exact p0 rows")


def test_modes_first_order_converges_to_the_exact_one():
    """HG g = 0.5: the distance of the 'modes' first order from the exact one as M grows -- a measurement of the truncation
    (measured 3.4e-2, 1.4e-3, 2.1e-6 of the maximum at M = 4, 8, 16), asserted only to fall."""
    c, sgn = _first_case()
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    exact = _first_exact(c, fa, fr, sgn, PHI_VIEW)
    d = [_err(_first_modes(c, fa, fr, M, 41, PHI_VIEW), exact) for M in (4, 8, 16)]
    print("modes against exact first order, M = 4, 8, 16: %.2e %.2e %.2e" % tuple(d))
    assert d[0] > d[1] > d[2]


# ---- refusals of the Python layer -----------------------------------------------------------------------------------------------------
OK = dict(view_mu=[0.3, 0.7], view_azimuths=[0.0, 1.0], nb_layers=24, nb_angles=16)
P = np.ones((32, 32))


@pytest.mark.parametrize("bad", [
    dict(view_mu=None), dict(azimuths=[0.0]), dict(mode_batch=True), dict(mode_chunk=2), dict(mode_batch=True, mode_chunk=2),
    dict(view_first_order="legendre"), dict(view_first_order=None), dict(n_modes=24, nphi_modes=25), dict(n_modes=0), dict(n_modes=65),
    dict(view_azimuths=[]), dict(view_azimuths=[0.0, np.nan]), dict(view_azimuths=[np.inf]), dict(view_azimuths=np.zeros((2, 2))),
    # everything view_mu already refuses
    dict(aer_set=[0]), dict(devices=[0, 1]), dict(P_atm=P), dict(P_aer=P), dict(P0_atm=np.ones(32)), dict(P0_aer=np.ones(32)),
    dict(surface="lambertian"), dict(surface="lambertian_readme"), dict(first_order="readme"), dict(view_quadrature="simpson"),
    dict(view_mu=[]), dict(view_mu=np.linspace(0.1, 1, 65)), dict(view_mu=[0.005]), dict(view_mu=[1.5]), dict(view_mu=[np.nan]),
    dict(view_levels=[24]), dict(view_levels=[-25]), dict(view_levels=[]),
], ids=lambda kw: ",".join(sorted(kw)) + "=" + str(list(kw.values())[0])[:12])
def test_python_refusals_before_any_handle(bad, monkeypatch):
    from sosrt import main
    monkeypatch.setattr(main, "get_solver", lambda *a, **k: pytest.fail("a handle was requested"))
    with pytest.raises(ValueError):
        main.SOS_Aer_batch(0.5, 0.1, 0.1, **dict(OK, **bad))


def test_view_mu_with_azimuths_points_at_view_azimuths():
    from sosrt.main import SOS_Aer_batch
    with pytest.raises(ValueError, match="view_azimuths"):
        SOS_Aer_batch(0.5, 0.1, 0.1, view_mu=[0.3], azimuths=[0.0], nb_layers=24, nb_angles=16)
