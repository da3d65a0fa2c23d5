"""The rank the library finds (sosrt.h, sosrt_phase_rank) for Legendre-series phase matrices of every rank the low-rank form of
the plain rows has code for -- 0 .. 4 terms accepted, five refused, with and without the flip symmetry -- on a host-only handle;
and the error bounds that tests/test_gpu_contraction_edges.py asserts on the device, checked here against NumPy models of the
same summations."""
import numpy as np
import pytest

import gpu_model as M
import legendre_phase as LP
from sosrt import inputs
from sosrt.solver import Solver

SIZES = [4, 6, 37, 128, 501]


def _handle_answers(N, P_atm, P_aer=None):
    s = Solver(10, N, device=-1)
    s.set_grid(inputs.direction_grid(N))
    s.set_phase(P_atm, P_aer)
    try:
        return s.phase_rank(), s.phase_asymmetry(), s.plan_fold(0)
    finally:
        s.close()


@pytest.mark.parametrize("N", SIZES)
def test_the_helper_builds_what_it_says(N):
    """Column normalisation 4, P0 normalisation 2, positive entries, exactly r terms of rank in the NumPy elimination, a fifth
    pivot far above the bar for five terms, flip symmetry to rounding -- and none with no_flip."""
    mu = inputs.direction_grid(N)
    trapz = LP._trapz
    for r in range(1, 6):
        P, P0 = LP.legendre_phase(N, mu, LP.terms(r), mu0=0.6)
        assert np.allclose(trapz(P, mu, axis=0), 4.0, rtol=1e-13, atol=0)
        assert abs(trapz(P0, mu) - 2.0) <= 1e-13
        assert P.min() >= 0.2 - 1e-12
        W = M.fold_weights(P, mu)
        assert M.asymmetry(W) <= 1e-13
        rank, piv = LP.rank_of(W)
        if r <= 4:
            assert rank == r and piv <= 1e-14
            U, V = LP.factor(W)
            assert U.shape == (2 * N, r) and V.shape == (r, 2 * N)
            assert np.max(np.abs(W - U @ V)) <= 1e-14 * np.max(np.abs(W))
        else:
            assert rank == -1 and piv > 1e-4
    P, P0 = LP.legendre_phase(N, mu, [], mu0=0.6)
    assert not P.any() and not P0.any()
    P, P0 = LP.legendre_phase(N, mu, LP.terms(3), mu0=0.6, no_flip=True)
    assert np.allclose(trapz(P, mu, axis=0), 4.0, rtol=1e-13, atol=0) and abs(trapz(P0, mu) - 2.0) <= 1e-13
    W = M.fold_weights(P, mu)
    assert M.asymmetry(W) > 1e-2 and LP.rank_of(W)[0] == 3


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_r_terms_are_rank_r(N, r):
    P, _ = LP.legendre_phase(N, inputs.direction_grid(N), LP.terms(r))
    (rank, res, uses), (asym, sym), W = _handle_answers(N, P)
    assert (rank, uses) == (r, True) and res <= 1e-13, (rank, res, uses)
    assert sym and asym <= 1e-13
    # the NumPy restatement factors the library's own folded matrix to the same rank
    assert LP.factor(W)[0].shape[1] == r


@pytest.mark.parametrize("N", SIZES)
def test_five_terms_are_refused(N):
    P, _ = LP.legendre_phase(N, inputs.direction_grid(N), LP.terms(5))
    (rank, res, uses), (asym, sym), _ = _handle_answers(N, P)
    assert rank == -1 and not uses and res > 1e-4, (rank, res, uses)
    assert sym                                                  # (the symmetric MFMA form is what then runs)


@pytest.mark.parametrize("N", SIZES)
def test_the_zero_matrix_is_rank_zero(N):
    (rank, res, uses), (asym, sym), _ = _handle_answers(N, np.zeros((2 * N, 2 * N)))
    assert (rank, res, uses) == (0, 0.0, True)
    assert (asym, sym) == (0.0, True)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("r", [1, 3, 4])
def test_without_flip_symmetry_the_rank_is_accepted_and_the_symmetric_form_is_off(N, r):
    mu = inputs.direction_grid(N)
    P, _ = LP.legendre_phase(N, mu, LP.terms(r), no_flip=True)
    Pr = inputs.phase_function("hg", N, mu, 0.5, 0.7)[1]
    (rank, res, uses), (asym, sym), _ = _handle_answers(N, P, Pr)
    assert rank == r and uses and res <= 1e-13, (rank, res, uses)
    assert not sym and asym > 1e-2


# ---- the bounds of tests/test_gpu_contraction_edges.py against NumPy models of the device's summations ----------------------------
def _edge_input(rng, L, D):
    X = rng.choice([-1.0, 1.0], (L, D)) * 10.0 ** rng.uniform(-6, 0, (L, D))
    X[1] = 0.0
    X[2] = 0.0; X[2, D - 1] = 1.0
    X[3] = 0.0; X[3, 0] = 1.0
    return X


@pytest.mark.parametrize("N", [4, 6, 37, 100])
@pytest.mark.parametrize("case", ["r1", "r4", "r3_no_flip"])
def test_numpy_models_of_the_four_forms_obey_the_derived_bounds(N, case):
    """float64 / float32 NumPy evaluations of the full product, the flip-symmetric form (gpu_model.source_symmetric), the
    factored plain rows and the float product against the long-double sum: each within the bound the device test asserts for the
    kernel of that form (legendre_phase.bounds).  A derivation that a plain evaluation of the same sum breaks would be
    a wrong derivation."""
    D, L = 2 * N, 9
    mu = inputs.direction_grid(N)
    Pa, _ = LP.legendre_phase(N, mu, LP.terms(int(case[1])), no_flip=case.endswith("no_flip"))
    Pr = inputs.phase_function("hg", N, mu, 0.5, 0.7)[1]
    rng = np.random.default_rng(N)
    X = _edge_input(rng, L, D)
    ca = np.full(L, 0.25); cr = np.zeros(L)
    ca[4:7] = 0.25 * 0.3; cr[4:7] = 0.95 / 4 * 0.7
    slab = cr != 0
    Wa, Wr = M.fold_weights(Pa, mu), M.fold_weights(Pr, mu)
    sym = max(M.asymmetry(Wa), M.asymmetry(Wr)) <= 1e-12
    U, V = LP.factor(Wa)
    J_ld, bound = LP.bounds(X, mu, Pa, Pr, ca, cr, Wa, sym, (U, V))
    full = M.source_model(X, Wa, Wr, ca, cr)
    dense = M.source_model(X, Wa, Wr, ca, cr, symmetric=True) if sym else full
    lr = dense.copy()
    lr[~slab] = ca[~slab, None] * ((X[~slab] @ U) @ V)
    f32 = ((ca[:, None] * X).astype(np.float32) @ Wa.astype(np.float32)).astype(np.float64)
    Wm = (ca[slab][0] * Wa + cr[slab][0] * Wr).astype(np.float32)
    f32[slab] = (X[slab].astype(np.float32) @ Wm).astype(np.float64)
    for mode, J in (("f64_full", full), ("f64_dense", dense), ("f64", lr), ("f32", f32)):
        ratio = LP.worst_ratio(J, J_ld, bound[mode])
        assert ratio <= 1.0, (mode, ratio)
