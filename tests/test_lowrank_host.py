"""The low-rank form of the plain rows (sosrt.h, sosrt_phase_rank; csrc/jn_gemm_tile.hpp, lowrank_rows) without a GPU: the rank
the library finds for each phase function on a host-only handle, and a NumPy model of the factored contraction against the
reference's goldens."""
import numpy as np
import pytest

import gpu_model as M
import sos_oracle as O
from sosrt import inputs
from sosrt.solver import Solver
from legendre_phase import factor as _factor
from util import assert_close, column_case, g1_case, golden

ALG = 5e-13


def _rank(N, P_atm, P_aer=None):
    s = Solver(10, N, device=-1)
    s.set_grid(inputs.direction_grid(N))
    s.set_phase(P_atm, P_aer)
    try:
        return s.phase_rank()
    finally:
        s.close()


@pytest.mark.parametrize("N", [32, 128, 256, 501])
def test_rayleigh_is_rank_two_and_iso_rank_one(N):
    mu = inputs.direction_grid(N)
    r, res, uses = _rank(N, inputs.phase_function("rayleigh", N, mu, 0.5)[1])
    assert (r, uses) == (2, True) and res <= 1e-14, (r, res)
    r, res, uses = _rank(N, inputs.phase_function("iso", N, mu, 0.5)[1])
    assert (r, uses) == (1, True) and res <= 1e-14, (r, res)


@pytest.mark.parametrize("name,g", [("hg", 0.7), ("eva", 0.0)])
def test_forward_peaked_matrices_are_not_low_rank(name, g):
    N = 64
    mu = inputs.direction_grid(N)
    r, res, uses = _rank(N, inputs.phase_function(name, N, mu, 0.5, g)[1])
    assert r == -1 and not uses and res > 1e-3


def test_random_flip_symmetric_nan_and_asymmetric_matrices_are_refused():
    N = 32
    D = 2 * N
    rng = np.random.default_rng(3)
    G = rng.uniform(0.5, 2.0, (D, D))
    assert _rank(N, 0.5 * (G + G[::-1, ::-1]))[0] == -1      # flip-symmetric, full rank
    assert _rank(N, G)[0] == -1                               # no structure at all
    P = inputs.phase_function("rayleigh", N, inputs.direction_grid(N), 0.5)[1].copy()
    P[3, 7] = np.nan
    r, res, uses = _rank(N, P)
    assert r == -1 and not uses and np.isnan(res)


def test_zero_matrix_is_rank_zero_and_a_positive_rank_one_matrix_is_accepted():
    N = 32
    D = 2 * N
    r, res, uses = _rank(N, np.zeros((D, D)))
    assert (r, res, uses) == (0, 0.0, True)
    rng = np.random.default_rng(7)
    P = np.outer(rng.uniform(0.5, 2.0, D), rng.uniform(0.5, 2.0, D))   # no flip symmetry
    r, res, uses = _rank(N, P)
    assert (r, uses) == (1, True) and res <= 1e-14


def _source_factored(In_1, U, V, Wa, Wr, ca, cr, slab):
    """Plain rows ca (In_1 U) V, slab rows the product with both matrices (gpu_model.source_model)."""
    Jn = ca[:, None] * ((In_1 @ U) @ V)
    if slab.any():
        Jn[slab] = M.source_model(In_1[slab], Wa, Wr, ca[slab], cr[slab])
    return Jn


@pytest.mark.parametrize("path", golden("g1_*_iso.npz"), ids=lambda p: p.split("/")[-1][3:-4])
def test_factored_model_single_slab(path):
    d, N, P = g1_case(path)
    tau, mu, alb = d["tau"], d["mu"], float(d["alb"])
    L = len(tau)
    W = M.fold_weights(P, mu)
    U, V = _factor(W)
    assert U.shape[1] == 1
    In_1, n = d["I1"], 2
    while "In_%d" % n in d:
        Jn = _source_factored(In_1, U, V, W, W, np.full(L, alb / 4), np.zeros(L), np.zeros(L, bool))
        assert_close(Jn, d["Jn_%d" % n], ALG, "Jn (low-rank form)")
        In_1 = d["In_%d" % n]
        n += 1


@pytest.mark.parametrize("path", golden("g3_*.npz") + golden("g6_*.npz"), ids=lambda p: p.split("/")[-1][:-4])
def test_factored_model_three_zone(path):
    d, c = column_case(path)
    N, L, mu, tau = c["N"], c["L"], c["mu"], c["tau"]
    iu, idn = c["idx_up"], c["idx_down"]
    fa = c["dtau_atm"] / (c["dtau_atm"] + c["dtau_aer"])
    fr = c["dtau_aer"] / (c["dtau_atm"] + c["dtau_aer"])
    ca = np.full(L, c["alb_atm"] / 4)
    cr = np.zeros(L)
    ca[iu:idn + 1] *= fa
    cr[iu:idn + 1] = c["alb_aer"] / 4 * fr
    slab = np.zeros(L, bool)
    slab[iu:idn + 1] = True
    Wa, Wr = M.fold_weights(c["P_atm"], mu), M.fold_weights(c["P_aer"], mu)
    U, V = _factor(Wa)
    zones = [(0, iu - 1), (iu, idn), (idn + 1, L - 1)]
    nfix = [M.a4b_count(tau[iu - 1], N), M.a4b_count(tau[idn], N), M.a4b_count(tau[idn], N)]
    Isv = d["I_saved"]
    In_1, I, In, n = Isv[0], Isv[0].copy(), np.ones_like(Isv[0]), 1
    tol = 5e-11 if c["surface"] == "lambertian" else ALG   # (the bar test_gpu_model.py sets for these columns)
    while O.convergence_ratio(In, I, N) >= 1e-4:
        n += 1
        Jn = _source_factored(In_1, U, V, Wa, Wr, ca, cr, slab)
        assert_close(Jn, M.source_model(In_1, Wa, Wr, ca, cr), ALG, "Jn, order %d" % n)
        In, st = M.transport_model(Jn, tau, mu, N, zones, nfix, c["surface"], c["grd_alb"])
        assert st == 0
        assert_close(In, Isv[n - 1], tol, "order %d" % n)
        In_1 = In
        I = I + In
    assert n == c["n"]
    assert_close(I, d["I"], tol, "I")
