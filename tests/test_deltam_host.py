"""Delta-M without a GPU: the identities of the NumPy model of tests/deltam_np.py and of sosrt.deltam, the
library's symbols, the drivers' refusals, and what the method is for on the oracle -- the raw cloud table 'fwc' stops solving as
the layer thickens, its delta-M columns converge, agree with each other and take a fifth of the orders."""
import numpy as np
import pytest

import deltam_np as DM
from sosrt import _lib, deltam, inputs
from sosrt.solver import Solver

L, N, MU0 = 40, 64, 0.6
ORDERS = (8, 12, 16)


@pytest.fixture(scope="module")
def fwc():
    return inputs.fwc_table()


@pytest.fixture(scope="module")
def thin(fwc):
    """tauStar_aer = 0.2: the raw table and its delta-M columns, solved once."""
    return {o: DM.solve(MU0, L, N, 0.2, *fwc, order=o) for o in (None,) + ORDERS}


def test_symbols_and_methods():
    lib = _lib.lib()
    for name, nargs in (("sosrt_phase_moments", 8), ("sosrt_phase_moments_dev", 8), ("sosrt_phase_delta_m", 9),
                        ("sosrt_phase_delta_m_dev", 9), ("sosrt_phase_p0_normaliser_dev", 6)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name) is not None
    for meth in ("phase_moments", "phase_moments_device", "delta_m_table", "delta_m_table_device", "p0_normaliser",
                 "p0_normaliser_device"):
        assert callable(getattr(Solver, meth))
    assert lib.sosrt_version() == 105                         # new symbols, the same ABI


def test_host_only_handle_refuses():
    s = Solver(4, 4, device=-1)
    try:
        for call in (lambda: s.phase_moments(np.ones(5), 4), lambda: s.phase_moments_device(8, 1, 5, 4, 8),
                     lambda: s.delta_m_table(np.ones(5), 2, ntab=9), lambda: s.delta_m_table_device(8, 1, 4, 2, 9, 8),
                     lambda: s.p0_normaliser_device("hg", 8, 8, 1, 0.5)):
            with pytest.raises(_lib.SosrtError, match="host-only"):
                call()
    finally:
        s.close()


def test_chi0_is_one(fwc):
    chi, norm = DM.moments(*fwc, 16)
    assert chi[0] == 1.0
    x, p = fwc
    assert norm == pytest.approx(0.25 * np.sum((p[1:] + p[:-1]) * np.diff(x)), rel=1e-13)   # the interpolant's integral is the trapezoid's


def test_linear_table_moments():
    a = 0.37
    x = np.linspace(-1, 1, 33)
    for tab_mu in (None, x, np.sort(np.concatenate(([-1.0, 1.0], np.random.default_rng(3).uniform(-1, 1, 31))))):
        xx = DM.abscissa(33, tab_mu)
        chi, norm = DM.moments(tab_mu, 1 + a * xx, 6)
        assert abs(chi[1] - a / 3) < 1e-14
        assert np.max(np.abs(chi[2:])) < 1e-14
        assert abs(norm - 1) < 1e-14


def test_rule_is_exact_to_degree_six():
    # a linear table times P_6 is a polynomial of degree 7 = 2 * 4 - 1 on every interval
    x = np.linspace(-1, 1, 9)
    p = 2 - x
    c4, c8 = DM.moments(x, p, 6)[0], DM.moments(x, p, 6, nodes=8)[0]
    assert np.max(np.abs(c4 - c8)) < 1e-14


def test_hg_moments_and_series():
    g, lmax = 0.7, 128
    chi = deltam.hg_moments(g, lmax)
    assert chi[0] == 1.0 and chi[3] == pytest.approx(g ** 3, rel=1e-15)
    # the moments of the 6001-point table of HG are g^l to the table's resolution
    x = np.linspace(-1, 1, 6001)
    assert np.max(np.abs(DM.moments(None, DM.hg(g)(x), 16)[0] - chi[:17])) < 1e-5
    # Lambda = lmax = 128 reproduces HG 0.7: f = 0.7^128 = 1.5e-20, the tail is below 1e-16
    t, f = DM.delta_m_table(chi, 128, x)
    assert DM.table_bound(chi, 128) == pytest.approx(18.9, abs=0.05)
    assert np.max(np.abs(t - DM.hg(g)(x))) < 1e-11 * 18.9


def test_truncated_table_has_unit_mean(fwc):
    x, t, f = DM.truncated(*fwc, 16)
    chi, norm = DM.moments(x, t, 4)
    # c_0 = 1, so the series has mean 1; the moments are of its interpolant on 1001 points, the trapezoid rule of a polynomial
    # of degree 15: h^2 / 12 * (p'(1) - p'(-1)) / 2 with h = 0.002 and p'(1) <= sum (2l + 1) l (l + 1) / 2 = 1.6e4 is <= 3e-3
    assert abs(norm - 1) < 3e-3 and 0 < f < 1


def test_scale_optics_keeps_absorption():
    rng = np.random.default_rng(5)
    t, w, f = rng.uniform(0.01, 2, 200), rng.uniform(0.05, 1, 200), rng.uniform(0, 0.9, 200)
    t2, w2 = deltam.scale_optics(t, w, f)
    ulp = lambda ref: 4 * np.spacing(np.abs(ref))
    assert np.all(np.abs(w2 * t2 - (1 - f) * w * t) <= ulp((1 - f) * w * t))
    # (1 - w') tau' = (1 - w) tau: a difference of rounded numbers, so 4 ulp of the numbers it is the difference of
    assert np.all(np.abs((1 - w2) * t2 - (1 - w) * t) <= ulp(t))
    assert deltam.scale_optics(0.3, 0.9, 0.5)[0] == pytest.approx(0.3 * 0.55)
    # arrays broadcast
    assert deltam.scale_optics(t[:3, None], w[None, :4], 0.2)[0].shape == (3, 4)
    m = DM.scale_optics(t, w, f)
    assert np.array_equal(m[0], t2) and np.array_equal(m[1], w2)


def test_scale_optics_identity_at_zero():
    rng = np.random.default_rng(6)
    t, w = rng.uniform(0, 2, 50), rng.uniform(0, 1, 50)
    t2, w2 = deltam.scale_optics(t, w, 0.0)
    assert np.array_equal(t2, t) and np.array_equal(w2, w)


def test_order_check():
    for bad in (1, 129, 0, -3, 2.0, "16", True):
        with pytest.raises(ValueError):
            deltam.check_order(bad)
    assert deltam.check_order(np.int64(16)) == 16 and deltam.check_order(2) == 2 and deltam.check_order(128) == 128


def test_driver_refusals():
    """Every combination without a delta-M form raises ValueError before a handle exists."""
    from sosrt import forcing
    from sosrt.main import SOS_Aer, SOS_Aer_batch, SOS_Aer_layers, SOS_Aer_spectrum, solve_batch_device
    base = dict(nb_layers=L, nb_angles=32, aer_phase_fun="fwc", delta_m=8)
    D = 64
    refused = [dict(azimuths=[0.0]), dict(aer_set=[0]), dict(aer_phase_fun=["fwc", "hg"], aer_set=[0]), dict(P_aer=np.ones((D, D))),
               dict(P0_aer=np.ones((1, D))), dict(azimuths=[0.0], mode_batch=True), dict(azimuths=[0.0], mode_chunk=2),
               dict(surface="brdf", brdf="lambertian"), dict(beam="spherical"),
               dict(source="thermal", planck=np.ones(L), planck_surface=1.0), dict(first_order="readme", surface="lambertian"),
               dict(devices=[0, 1]), dict(aer_phase_fun="iso"), dict(aer_phase_fun="rayleigh"), dict(delta_m=1), dict(delta_m=129),
               dict(delta_m=16.0)]
    for kw in refused:
        with pytest.raises(ValueError):
            SOS_Aer_batch([0.6], [0.2], [0.1], **dict(base, **kw))
    for kw in (dict(aer_set=[0]), dict(P_aer=np.ones((D, D))), dict(surface="brdf", brdf="lambertian"), dict(beam="spherical"),
               dict(source="thermal", planck=np.ones(L), planck_surface=1.0), dict(delta_m=1)):
        with pytest.raises(ValueError):
            solve_batch_device([0.6], [0.2], [0.1], **dict(base, **kw))
    with pytest.raises(ValueError):
        SOS_Aer(delta_m=8, beam="spherical", nb_layers=L, nb_angles=32)
    with pytest.raises(ValueError):
        SOS_Aer(delta_m=8, P_aer=np.ones((D, D)), nb_layers=L, nb_angles=32)
    with pytest.raises(ValueError):
        SOS_Aer_layers([0.6], [0.1], [(25, 17, 0.2, 0.99)], nb_layers=L, nb_angles=32, delta_m=8)
    with pytest.raises(ValueError):
        SOS_Aer_spectrum([0.55], [0.6], 0.2, [0.1], dict(m=1.44 + 0j, r_m=0.5, sig=1.2), nb_layers=L, nb_angles=32, delta_m=8)
    for kw in (dict(beam="spherical"), dict(surface="brdf", brdf="lambertian"), dict(delta_m=1),
               dict(phases=(np.ones(D), np.ones((D, D)), np.ones(D), np.ones((D, D))))):
        with pytest.raises(ValueError):
            forcing.toa_net_flux(0.6, 0.124, [0.2], 0.1, 1.0, [0.99], nb_layers=L, nb_angles=32, aer_phase_fun="fwc",
                                 **dict(dict(delta_m=8), **kw))


# ---- the oracle: what delta-M is for -----------------------------------------------------------------------------------------
def test_oracle_raw_fwc_stops_solving_and_delta_m_converges(fwc):
    with pytest.raises(IndexError):
        DM.solve(MU0, L, N, 0.5, *fwc, order=None)
    for o in ORDERS:
        sol, f, c = DM.solve(MU0, L, N, 0.5, *fwc, order=o)
        print("tauStar_aer 0.5, Lambda %d: n = %d, f = %.4f, TOA-up %.5f" % (o, sol.n, f, DM.toa_up(sol, c)))
        assert sol.n < 256 and sol.ratios[-1] < 1e-4 and np.all(np.isfinite(sol.I))        # measured 13, 14, 15 orders


def test_oracle_orders_agree(thin):
    up = [DM.toa_up(*thin[o][::2]) for o in ORDERS]
    print("tauStar_aer 0.2: TOA-up", up, "raw", DM.toa_up(*thin[None][::2]))
    assert (max(up) - min(up)) / min(up) < 0.02                                             # measured 1.1 %


def test_oracle_order_counts(thin):
    ns = [thin[o][0].n for o in ORDERS]
    print("tauStar_aer 0.2: orders", ns, "raw", thin[None][0].n)
    assert max(ns) <= 12                                                                    # measured 9, 10, 10
    assert thin[None][0].n >= 40                                                            # measured 49
