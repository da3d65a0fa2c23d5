"""The NumPy model of the view-radiance stage (tests/view_np.py) pinned to the oracle, so that the device tests
(tests/test_gpu_view.py) have a pinned yardstick: evaluated at the nodes of the direction grid the model must give the oracle's
phase matrices, its first order and -- with the source of all orders but the last -- its scattered field on every lane the
mu -> 0 treatments left alone.  The LINEAR quadrature is pinned by a known answer.  No GPU."""
import os
import re

import numpy as np
import pytest

import sos_oracle as O
import view_np as VN
from util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sosrt_phase_rows_dev", "sosrt_phase_p0_rows_dev", "sosrt_view_radiance_dev")


def test_symbols_and_version():
    from sosrt import _lib
    header = open(os.path.join(ROOT, "include", "sosrt.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), "%s is not declared in sosrt.h" % name
        assert name in _lib.SIGNATURES, "%s is not bound in sosrt._lib" % name
        assert getattr(L, name) is not None
    for name, value in (("SOSRT_MAX_VIEWS", 64), ("SOSRT_VIEW_QUAD_GRID", 0), ("SOSRT_VIEW_QUAD_LINEAR", 1)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, header)
        assert m and int(m.group(1)) == value, name
    assert (_lib.MAX_VIEWS, _lib.VIEW_QUAD_GRID, _lib.VIEW_QUAD_LINEAR) == (64, 0, 1)
    assert L.sosrt_version() == 105
    assert len(_lib.SIGNATURES["sosrt_view_radiance_dev"][1]) == 15


@pytest.mark.parametrize("N", [32, 33])
def test_phase_rows_at_nodes_are_the_matrix(N):
    mu = O.make_mu(N)
    mu0 = 0.6
    tab_mu = np.linspace(-1, 1, 181)
    tab_p = np.exp(2.5 * tab_mu) + 0.3 * (1 + tab_mu ** 2)          # a forward-peaked table, un-normalised like fwc:3,173
    cases = [("rayleigh", {}, O.phase_rayleigh(N, mu, mu0)),
             ("hg", dict(g=0.7), O.phase_hg(N, mu, mu0, 0.7)),
             ("table", dict(table=(tab_mu, tab_p)), O.phase_table(N, mu, mu0, tab_mu, tab_p))]
    for kind, kw, (P0, P) in cases:
        fn = VN.phase_fn(kind, **kw)
        assert_close(VN.phase_rows(fn, mu, mu), P, 1e-12, "%s rows at the nodes" % kind)
        assert_close(VN.phase_p0_rows(fn, mu, [mu0], mu)[0], P0, 1e-12, "%s P0 rows at the nodes" % kind)
    P0, P = O.phase_isotropic(N, mu)
    assert np.array_equal(VN.phase_rows(None, mu, mu), P) and np.array_equal(VN.phase_p0_rows(None, mu, [mu0], mu)[0], P0)


@pytest.mark.parametrize("case", [VN.case_A, VN.case_B], ids=["A", "B"])
def test_first_order_at_nodes(case):
    c = case()
    mv, lanes = VN.node_views(c.mu, c.N)
    got = VN.first_order(c, c.P0_atm[lanes], c.P0_aer[lanes], mv)
    assert_close(got, O.first_order(c)[:, lanes], 1e-12, "first order at the nodes")


def test_first_order_at_nodes_single_slab():
    N, L, mu0, alb, tauStar = 32, 30, 0.45, 0.9, 1.5
    mu = O.make_mu(N)
    tau = np.linspace(0, tauStar, L)
    P0, P = O.phase_hg(N, mu, mu0, 0.6)
    mv, lanes = VN.node_views(mu, N)
    got = VN.first_order_single_slab(tau, tauStar, mu0, alb, P0[lanes], mv)
    assert_close(got, O.I1_NumInt(tau, mu, tauStar, mu0, P0, alb, N)[:, lanes], 1e-12, "I1_NumInt at the nodes")


@pytest.mark.parametrize("case", [VN.case_A, VN.case_B], ids=["A", "B"])
def test_grid_quadrature_reproduces_the_grid_at_nodes(case):
    c, sol = VN.solved(case)
    assert sol.n >= 3
    err, rewritten = VN.node_errors(c, sol)
    V = err.shape[1] // 2
    down = np.where(rewritten, 0.0, err[:, :V])
    print("down max %.3e, rewritten lanes per row up to %d" % (down.max(), rewritten.sum(axis=1).max()))
    assert down.max() < 1e-12
    assert (~rewritten).all(axis=0).sum() >= V - int(0.06 * c.N)      # (the exclusion is the a4b block and nothing else)
    ok = VN.untouched_up(err)
    print("untouched upward lanes: %d of %d, max error on them %.3e" % (ok.sum(), V, err[:, V:][:, ok].max()))
    assert ok.sum() >= 30


KNOWN_MU = np.array([0.011, 0.05, 0.33, 1.0])


def known_answer_column(three_zone, L=24, N=16):
    """Isotropic, conservative, I_src = 1: S = 1 and the exact answer is 1 - exp(-tauStar / mu)."""
    mu = O.make_mu(N)
    P0, P = O.phase_isotropic(N, mu)
    if three_zone:
        return O.make_column(0.5, VN.Z0, 25, 17, L, 0.5, 0.5, 0.0, 1.0, 1.0, N, P0, P, P0, P)
    return VN.single_slab_column(np.linspace(0, 1.0, L), mu, N, 0.5, 1.0, 1.0)


@pytest.mark.parametrize("three_zone", [True, False], ids=["three_zone", "single_slab"])
def test_linear_quadrature_known_answer(three_zone):
    c = known_answer_column(three_zone)
    L, V = len(c.tau), len(KNOWN_MU)
    rows = VN.phase_rows(None, c.mu, VN.signed(KNOWN_MU))
    S = VN.source(c, rows, rows, np.ones((L, 2 * c.N)))
    assert np.max(np.abs(S - 1)) < 1e-14
    exact = 1 - np.exp(-c.tau[-1] / KNOWN_MU)
    lin = VN.transport(c, S, KNOWN_MU, VN.QUAD_LINEAR, surface=None)
    print("LINEAR: TOA-up %.2e, surface-down %.2e" % (np.max(np.abs(lin[0, V:] - exact)), np.max(np.abs(lin[-1, :V] - exact))))
    assert np.max(np.abs(lin[0, V:] - exact)) < 1e-13 and np.max(np.abs(lin[-1, :V] - exact)) < 1e-13
    assert np.all(lin[0, :V] == 0) and np.all(lin[-1, V:] == 0)
    if three_zone:
        # the two modes are not the same thing: the trapezoid rule with the H4 gaps misses the answer visibly
        grid = VN.transport(c, S, KNOWN_MU, VN.QUAD_GRID, surface=None)
        print("GRID at mu = 0.33: off by %.3f" % abs(grid[0, V + 2] - exact[2]))
        assert abs(grid[0, V + 2] - exact[2]) > 1e-2


def test_python_refusals_before_any_handle():
    """`view_mu` with what the stage does not serve raises ValueError before a handle is made (no GPU is touched)."""
    from sosrt.main import SOS_Aer_batch
    ok = dict(view_mu=[0.3, 0.7], nb_layers=24, nb_angles=16)
    P = np.ones((32, 32))
    for bad in (dict(azimuths=[0.0]), dict(aer_set=[0]), dict(devices=[0, 1]), dict(P_atm=P), dict(P_aer=P), dict(P0_atm=np.ones(32)),
                dict(P0_aer=np.ones(32)), dict(surface="lambertian"), dict(surface="lambertian_readme"), dict(first_order="readme"),
                dict(view_quadrature="simpson"), dict(view_mu=[]), dict(view_mu=np.linspace(0.1, 1, 65)), dict(view_mu=[0.005]),
                dict(view_mu=[1.5]), dict(view_mu=[np.nan]), dict(view_levels=[24]), dict(view_levels=[-25]), dict(view_levels=[])):
        with pytest.raises(ValueError):
            SOS_Aer_batch(0.5, 0.1, 0.1, **dict(ok, **bad))
