"""The references of tests/test_gpu_brdf_builder_shapes.py on the CPU (tests/brdf_builder_cases.py): its one-product quadrature
against brdf_azimuth_np.rho_modes, its long double expressions against the suite's float64 models, its erfc, its measure, and
the rule of the device test: float64 NumPy within a tenth of the bound of its long double evaluation, row-wise, for every kind,
shape and call -- except where the cases module says that the device is compared with the long double evaluation."""
import math

import numpy as np
import pytest

import brdf_azimuth_np as BA
import brdf_builder_cases as K
import brdf_np as G
import brdf_view_np as BV
import sos_oracle as O


@pytest.mark.parametrize("kind", list(K.KINDS))
def test_float64_is_within_a_tenth_of_the_bound(kind):
    gaps = K.float64_gaps([kind])
    shapes = {(g[1], g[2]) for g in gaps if g[4][1]}
    assert shapes == {(name, nphi) for name, nphi, _ in K.PLANS}
    worst = max(gaps, key=lambda g: g[5])
    print(K.show(worst))
    for g in gaps:
        if (kind, g[3]) in K.LONG_DOUBLE_REFERENCE:
            assert K.GAP_BAR < g[5] <= K.KERNEL_BAR, K.show(g)     # (the exception is one: float64 alone would spend a quarter of the bound)
        else:
            assert g[5] <= K.GAP_BAR, K.show(g)


@pytest.mark.parametrize("kind", list(K.KINDS))
def test_one_product_quadrature_is_the_models(kind):
    """rho_modes here against brdf_azimuth_np.rho_modes mode by mode, and through it the operator, beam-row and view-row references
    against brdf_azimuth_np.operator_modes, beam_modes and brdf_view_np.view_rows_modes, at N = 4 and 37 on 3, 65, 257 and 300 nodes"""
    brdf = K.KINDS[kind]
    for N, nphi in ((4, 3), (4, 257), (37, 65), (37, 300)):
        mu = O.make_mu(N)
        ms = list(range(min(nphi - 2, 12) + 1))
        up, dn, wj = K.grid(N)
        R = wj[None, None, :] * K.rho_modes(brdf, up[:, None], dn[None, :], ms, nphi)
        ref = BA.operator_modes(mu, N, brdf, ms, nphi)
        assert np.max(np.abs(R - ref)) <= 1e-14 * np.max(np.abs(ref)), (N, nphi)
        r0 = K.rho_modes(brdf, up, 0.21, ms, nphi)
        ref = BA.beam_modes(mu, N, 0.21, brdf, ms, nphi)
        assert np.max(np.abs(r0 - ref)) <= 1e-14 * np.max(np.abs(ref)), (N, nphi)
        mv = np.array([0.01, 0.05004, 0.5, 1.0])
        Rv = wj[None, None, :] * K.rho_modes(brdf, mv[:, None], dn[None, :], ms, nphi)
        ref = BV.view_rows_modes(mu, N, mv, brdf, ms, nphi)
        assert np.max(np.abs(Rv - ref)) <= 1e-14 * np.max(np.abs(ref)), (N, nphi)


@pytest.mark.parametrize("kind", list(K.KINDS))
def test_long_double_expressions_are_the_models(kind):
    """rho_ld restates the models' expressions: on random directions and azimuths it agrees with the float64 model to float64's
    own resolution of the value, 1e-13 of the largest value of the direction pair (the Ross-Thick kernel's two terms cancel to
    4e-2 of themselves and the glint loses arg * 1e-16 in its exponential, so not 1e-16)"""
    rng = np.random.default_rng(5)
    a, b = rng.uniform(0.01, 1.0, (200, 1)), rng.uniform(0.01, 1.0, (200, 1))
    phi = np.concatenate((rng.uniform(0, np.pi, 30), K.PHI_AT))[None, :]
    f64, ld = K.rho_at(K.KINDS[kind], a, b, phi), K.rho_at(K.KINDS[kind], a, b, phi, np.longdouble)
    assert ld.dtype == np.longdouble
    assert K.rowwise(f64, ld, 0) <= 1e-13


def test_erfc_in_long_double():
    x = np.array([0.0, 1e-3, 0.087, 0.5, 1.0, 2.0, 2.999, 3.0, 3.5, 5.0, 8.0, 12.0, 30.0])
    got = K._erfc_ld(x)
    ref = np.array([math.erfc(v) for v in x])
    assert got.dtype == np.longdouble and np.max(np.abs(got - ref)) <= 2e-16          # (math.erfc: a float64 value, half an ulp of at most 1)
    assert np.all(np.abs(got[7:12] - ref[7:12]) <= 1e-14 * ref[7:12])                  # the continued fraction: relative


def test_the_measures():
    ref = np.array([[[1e5, 2e5], [1.0, 2.0]], [[1e3, 0.0], [0.5, 0.0]]])               # [m, i, j]: row 0 grazing, row 1 interior
    got = ref.copy()
    got[0, 1, 0] += 1e-7
    assert K.globalwise(got, ref) == pytest.approx(5e-13) and K.rowwise(got, ref, 1) == pytest.approx(5e-8)
    # a call without mode 0: a direction whose stored values are below RESOLVED of its mode 0 is measured against that
    high, noise = np.array([[[1e-9, 0.0], [3e-3, 4e-3]]]), np.array([[[1e-9 + 1e-15, 1e-16], [3e-3, 4e-3 + 1e-15]]])
    assert K.rowwise(noise, high, 1, ref[:1]) == pytest.approx(max(1e-15 / (1e-2 * 2e5), 1e-15 / 2e-2))
    assert K.rowwise(noise, high, 1) == pytest.approx(1e-15 / 1e-9, rel=1e-6)
    assert K.rowwise(np.ones((2, 2)), np.zeros((2, 2)), 0) == float("inf") and K.rowwise(np.zeros((2, 2)), np.zeros((2, 2)), 0) == 0.0


def test_the_cases():
    assert len(K.KINDS) == 8 and len(K.PLANS) == 9
    for name, (N, B) in K.SHAPES.items():
        rows = K.sample_rows(name)
        assert len(np.unique(rows)) == len(rows) == (N - 1 if N <= 130 else 18) and rows[0] == 0 and rows[-1] == N - 2
        assert list(K.suns(name)[:2]) == [0.05, 1.0]
        for V in K.VIEWS:
            mv = K.view_mu(name, V)
            assert len(mv) == V and np.all((mv >= 0.01) & (mv <= 1.0))
    for name, nphi, calls in K.PLANS:
        assert all(m0 + mc - 1 <= min(nphi - 2, 64) for m0, mc in calls) and 0 in K.plan_modes(name, nphi)


def test_the_driver_cases_are_served_by_the_model():
    """at least one column per ground is COL_OK in the model's series at (L, N, B) = (64, 128, 2): here all are"""
    for ground in K.DRIVER_GROUNDS:
        I, bounces, ratio, status = K.driver_model(ground)
        assert np.all(np.isfinite(I)) and (status == G.COL_OK).all() and np.all(bounces >= 2) and np.all(ratio < 1e-4), ground
