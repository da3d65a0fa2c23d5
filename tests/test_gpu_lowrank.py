"""The low-rank form of the plain rows on the device (csrc/jn_gemm_tile.hpp, lowrank_rows): the source function against the
reference's trapezoid sum and against the MFMA forms, whole columns against the dense contraction, and the bits of a column
across the tilings of one solve."""
import numpy as np
import pytest

import sos_oracle as O
from sosrt import inputs
from sosrt.main import SOS_Aer_batch
from sosrt.solver import Solver
from util import assert_close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L,N", [(200, 128), (400, 256), (800, 501)])
def test_source_low_rank_against_the_reference_and_the_mfma_forms(L, N):
    """Rayleigh plain rows, EVA slab rows (rows 40 % .. 47 % of the column): f64 (low-rank plain rows), f64_dense and f64_full
    against Jn_NumInt, and within 1e-13 of each other."""
    rng = np.random.default_rng(L + N)
    B = 2
    mu = inputs.direction_grid(N)
    Pa = inputs.phase_function("rayleigh", N, mu, 0.5)[1]
    Pr = inputs.phase_function("eva", N, mu, 0.5)[1]
    X = rng.uniform(0.0, 1.0, (B, L, 2 * N)) * np.linspace(0.5, 2.0, 2 * N)
    iu, idn = int(0.4 * L), int(0.47 * L)
    s = Solver(L, N, max_batch=B)
    s.set_grid(mu)
    s.set_phase(Pa, Pr)
    r, res, uses = s.phase_rank()
    assert (r, uses) == (2, True) and res <= 1e-14
    d_atm, d_aer, a_atm, a_aer = 0.1, 0.3, 1.0, 0.95
    s.set_columns(np.full(B, iu), np.full(B, idn), np.full(B, 0.5), np.zeros(B), np.full(B, a_atm), np.full(B, a_aer),
                  np.full(B, d_atm), np.full(B, d_aer), np.full(B, 0.5))
    J = {}
    for mode in ("f64", "f64_dense", "f64_full"):
        s.set_contraction(mode)
        assert s.phase_rank()[2] == (mode == "f64")
        J[mode] = s.source(X)
    s.set_contraction("f64")
    assert np.array_equal(s.source(X), J["f64"])
    fa, fr = d_atm / (d_atm + d_aer), d_aer / (d_atm + d_aer)
    for b in range(B):
        ref = O.Jn_NumInt(2, X[b], np.zeros(L), mu, 0.5, 0.5, Pa, a_atm, N)
        ref[iu:idn + 1] = (fa * O.Jn_NumInt(2, X[b][iu:idn + 1], np.zeros(idn + 1 - iu), mu, 0.5, 0.5, Pa, a_atm, N) +
                           fr * O.Jn_NumInt(2, X[b][iu:idn + 1], np.zeros(idn + 1 - iu), mu, 0.5, 0.5, Pr, a_aer, N))
        for mode, Jm in J.items():
            assert_close(Jm[b], ref, 1e-13, "Jn column %d (%s)" % (b, mode))
        assert_close(J["f64"][b], J["f64_dense"][b], 1e-13, "f64 vs f64_dense")
        assert_close(J["f64"][b], J["f64_full"][b], 1e-13, "f64 vs f64_full")
    s.close()


def _fresh(M):
    for s_ in list(M._solvers.values()):
        s_.close()
    M._solvers.clear()


def test_whole_columns_low_rank_against_dense():
    """Rayleigh + EVA columns: the same order counts and results within 1e-12 with and without the low-rank form."""
    from sosrt import main as M
    rng = np.random.default_rng(31)
    B = 64
    mu0 = rng.uniform(0.2, 1.0, B)
    taer = rng.choice([0.02, 0.12, 0.6, 1.0], B)
    rho = rng.uniform(0.0, 0.8, B)
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, aer_phase_fun="eva", max_orders=200)
    _fresh(M)
    lr = SOS_Aer_batch(mu0, taer, rho, **kw)
    (s,) = M._solvers.values()
    assert s.phase_rank()[2]
    s.set_contraction("f64_dense")
    assert not s.phase_rank()[2]
    dense = SOS_Aer_batch(mu0, taer, rho, **kw)
    assert len(M._solvers) == 1
    _fresh(M)
    assert (lr.status == 0).all() and np.array_equal(lr.n, dense.n)
    assert_close(lr.I, dense.I, 1e-12, "I")


def test_a_column_keeps_its_bits_alone_in_a_sub_batch_and_in_the_headline_batch():
    """A 512-column Rayleigh + EVA batch at L = 200, N = 128 runs the dense tiling while every column is live, the live-column
    tilings as columns converge and the register tile for the last few: a column solved alone, in a sub-batch or in the whole
    batch has the same bits and order count."""
    from sosrt import main as M
    rng = np.random.default_rng(512)
    B = 512
    mu0 = rng.uniform(0.2, 1.0, B)
    # (a few aerosol depths: the slab rows of every batch get their combined matrices -- more distinct coefficient pairs than the
    # library caches would give a large batch two passes and a lone column one, a different summation of its slab rows)
    taer = rng.choice([0.02, 0.12, 0.6, 1.0], B)
    rho = rng.uniform(0.0, 0.6, B)
    kw = dict(tauStar_atm=0.124, alb_aer=0.95, aer_phase_fun="eva", max_orders=200)
    _fresh(M)
    whole = SOS_Aer_batch(mu0, taer, rho, **kw)
    assert (whole.status == 0).all() and whole.n.max() > whole.n.min()
    sub = SOS_Aer_batch(mu0[100:140], taer[100:140], rho[100:140], **kw)
    assert np.array_equal(sub.n, whole.n[100:140])
    assert np.array_equal(sub.I, whole.I[100:140])
    for c in (int(np.argmax(whole.n)), int(np.argmin(whole.n)), 333):
        one = SOS_Aer_batch(mu0[c:c + 1], taer[c:c + 1], rho[c:c + 1], **kw)
        assert one.n[0] == whole.n[c]
        assert np.array_equal(one.I[0], whole.I[c]), c
    _fresh(M)
