"""Several aerosol phase matrices on one handle, the part that needs no GPU: the C ABI (version 105), the folds of the sets on
a host-only handle, argument errors, and the superposition helper the device tests compare per-zone sets against."""
import ctypes
import os

import numpy as np
import pytest

import sos_oracle as O
from phase_sets_helper import solve_column_zone_sets
from sosrt import _lib, inputs
from sosrt.solver import Solver


def _matrices(N, mu):
    return (inputs.phase_function("rayleigh", N, mu, 0.5)[1],
            np.stack([inputs.phase_function("hg", N, mu, 0.5, g=0.7)[1], inputs.phase_function("hg", N, mu, 0.5, g=0.3)[1],
                      inputs.phase_function("fwc", N, mu, 0.5)[1]]))


def test_symbols_and_version():
    L = _lib.lib()
    assert L.sosrt_version() >= 105
    for name in ("sosrt_set_phase_sets", "sosrt_set_aerosol_sets", "sosrt_phase_sets_info"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sosrt.h")).read()
    assert "#define SOSRT_VERSION 105" in header and "#define SOSRT_MAX_PHASE_SETS 64" in header
    assert _lib.MAX_PHASE_SETS == 64


@pytest.mark.parametrize("N", [32, 128])
def test_folds_of_the_sets_are_the_folds_of_set_phase(N):
    """set_phase_sets then plan_fold(1 + s) is the fold of set_phase(P_atm, P_aer[s]) for every s, bit for bit; W_atm too."""
    mu = inputs.direction_grid(N)
    Pa, Ps = _matrices(N, mu)
    h = Solver(20, N, device=-1)
    h.set_grid(mu)
    h.set_phase_sets(Pa, Ps)
    assert h.phase_sets_info()["sets"] == 3
    one = Solver(20, N, device=-1)
    one.set_grid(mu)
    for k in range(3):
        one.set_phase(Pa, Ps[k])
        assert np.array_equal(h.plan_fold(1 + k), one.plan_fold(1)), k
        assert np.array_equal(h.plan_fold(0), one.plan_fold(0))
    # S = 1 through the new entry point is set_phase
    h.set_phase_sets(Pa, Ps[2:3])
    assert h.phase_sets_info()["sets"] == 1
    assert np.array_equal(h.plan_fold(1), one.plan_fold(1))
    assert h.phase_asymmetry() == one.phase_asymmetry() and h.phase_rank() == one.phase_rank()
    with pytest.raises(ValueError):
        h.plan_fold(2)
    h.close(); one.close()


def test_the_asymmetry_is_the_maximum_over_the_sets():
    N = 32
    mu = inputs.direction_grid(N)
    Pa, Ps = _matrices(N, mu)
    h = Solver(20, N, device=-1)
    h.set_grid(mu)
    h.set_phase_sets(Pa, Ps)
    a, uses = h.phase_asymmetry()
    assert a <= 1e-12 and uses
    bad = Ps.copy()
    bad[1, 3, 5] *= 1.5                     # one set without the flip symmetry switches the symmetric form off for all
    h.set_phase_sets(Pa, bad)
    a, uses = h.phase_asymmetry()
    assert a > 1e-6 and not uses
    h.close()


def test_argument_errors():
    N = 32
    mu = inputs.direction_grid(N)
    Pa, Ps = _matrices(N, mu)
    h = Solver(20, N, device=-1)
    h.set_grid(mu)
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.sosrt_set_phase_sets(h._h, p(Pa), 0, p(Ps)) == _lib.E_INVALID                  # S = 0
    big = np.ascontiguousarray(np.broadcast_to(Ps[0], (65, 2 * N, 2 * N)))
    assert L.sosrt_set_phase_sets(h._h, p(Pa), 65, p(big)) == _lib.E_INVALID                # S above the maximum
    assert b"SOSRT_MAX_PHASE_SETS" in L.sosrt_last_error()
    assert L.sosrt_set_phase_sets(h._h, p(Pa), 2, None) == _lib.E_INVALID
    with pytest.raises(ValueError):
        h.set_phase_sets(Pa, Ps[0])                                                          # not a stack
    h.set_phase_sets(Pa, Ps)
    z = np.array([0, 3], dtype=np.int32)
    assert L.sosrt_set_aerosol_sets(h._h, 2, 1, p(z)) != 0                                   # (a host-only handle has no columns)
    assert L.sosrt_set_aerosol_sets(h._h, 2, 0, p(z)) == _lib.E_INVALID                      # nzmax
    assert L.sosrt_set_aerosol_sets(h._h, 2, 9, p(z)) == _lib.E_INVALID
    assert L.sosrt_set_aerosol_sets(h._h, 0, 1, p(z)) == _lib.E_INVALID
    assert L.sosrt_set_aerosol_sets(h._h, 2, 1, None) == _lib.E_INVALID
    h.close()


def _two_slab_column(N, L, mu0, phase_hi, phase_lo):
    mu = O.make_mu(N)
    P0a, Pa = O.phase_rayleigh(N, mu, mu0)
    slabs = [(25, 17, 0.12, 0.97), (12, 8, 0.2, 0.9)]
    c = O.make_column_slabs(mu0, 120, slabs, L, 0.124, 0.15, 1.0, N, P0a, Pa, phase_hi[0], phase_hi[1])
    return c, [phase_hi, phase_lo]


def test_the_superposition_helper_reproduces_the_oracle_when_all_zones_share_a_set():
    """Rayleigh + HG g = 0.7 in both slabs (L = 60, N = 32, mu0 = 0.6): the superposed loop gives the n of solve_column and a
    field within 1e-13 of its maximum (the sums re-associate: not to the bit); with HG g = 0.3 in the lower slab, or the two
    swapped, the field moves by far more than that -- the device tests' guards have signal."""
    N, L, mu0 = 32, 60, 0.6
    mu = O.make_mu(N)
    hi, lo = O.phase_hg(N, mu, mu0, 0.7), O.phase_hg(N, mu, mu0, 0.3)
    c, _ = _two_slab_column(N, L, mu0, hi, hi)
    ref = O.solve_column(c, literal=False)
    got = solve_column_zone_sets(c, [hi, hi])
    scale = np.max(np.abs(ref.I))
    assert got.n == ref.n
    assert np.max(np.abs(got.I - ref.I)) <= 1e-13 * scale
    mixed = solve_column_zone_sets(c, [hi, lo])
    swapped = solve_column_zone_sets(c, [lo, hi])
    assert np.max(np.abs(mixed.I - ref.I)) > 1e-3 * scale
    assert np.max(np.abs(mixed.I - swapped.I)) > 1e-3 * scale


def test_the_reallocation_walk_shape_plans_the_live_tiling():
    """The shape of test_gpu_phase_sets.test_buffers_regrown_on_one_handle_leave_no_stale_state (L = 24, N = 16, B = 4, three
    zones, specular) takes the contraction over the live columns from the first order on and can hold several phase sets'
    mix groups: that test walks the buffers of the path the sweeps run.  (The group count itself needs columns, which a
    host-only handle cannot take; the device test asserts it.)"""
    s = Solver(24, 16, max_batch=4, device=-1)
    s.set_grid(inputs.direction_grid(16))
    p = s.plan_launch(4, 4)
    assert p["groups"] == 1 and p["gemm"] != _lib.PLAN_GEMM_DENSE and p["tail_cols"] == 4
    info = s.phase_sets_info()
    assert info["sets"] == 1 and info["group_cap"] >= 4
    s.close()
