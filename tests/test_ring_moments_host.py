"""When an order runs in the ring kernel's moment mode (csrc/solve.hip: plan_order, LaunchPlan::moments), asked of host-only
handles through sosrt_plan_ring_moments: the contraction then writes a 64-byte moment record per plain row instead of the row of
Jn and the ring kernel expands it, so both launches of the order must agree -- one decision, tested here without a GPU."""
import functools

from sosrt import _lib, inputs
from sosrt.solver import Solver

L, N = 200, 128


@functools.lru_cache(maxsize=None)
def _matrices(aerosol):
    mu = inputs.direction_grid(N)
    Pa = inputs.phase_function("rayleigh", N, mu, 0.5)[1]
    Pr = inputs.phase_function(aerosol, N, mu, 0.5, 0.7)[1]
    return Pa, Pr


def _handle(monkeypatch, atmosphere="rayleigh", aerosol="eva", **env):
    monkeypatch.delenv("SOSRT_RING_MOMENTS", raising=False)
    monkeypatch.setenv("SOSRT_GROUPS", "1")                # one column group, as the benchmark's sweep runs
    for k, v in env.items():
        monkeypatch.setenv(k, v)                            # (knobs are read when the handle is created)
    s = Solver(L, N, max_batch=512, device=-1)
    s.set_grid(inputs.direction_grid(N))
    Pa, Pr = _matrices(aerosol)
    s.set_phase(_matrices("hg")[1] if atmosphere == "hg" else Pa, Pr)
    return s


def test_on_for_rayleigh_over_eva_while_the_ring_kernel_runs(monkeypatch):
    s = _handle(monkeypatch)
    try:
        assert s.phase_rank()[0] == 2 and s.phase_rank()[2] and s.phase_asymmetry()[1]
        for live in (512, 400, 201):
            assert s.plan_launch(512, live)["transport"] == _lib.PLAN_TRANSPORT_RING
            assert s.plan_ring_moments(512, live), live
        # at 200 live columns and below the chunk-parallel kernel transports: rows of Jn
        for live in (200, 64, 1):
            assert s.plan_launch(512, live)["transport"] == _lib.PLAN_TRANSPORT_SCAN
            assert not s.plan_ring_moments(512, live), live
        for surface in ("specular", "lambertian", "none"):
            assert s.plan_ring_moments(512, 512, surface=surface, zones=3 if surface != "none" else 1)
    finally:
        s.close()


def test_off_without_the_low_rank_form(monkeypatch):
    s = _handle(monkeypatch, atmosphere="hg")              # Henyey-Greenstein molecules: no factorisation within the tolerance
    try:
        assert s.phase_rank()[0] < 0 and not s.phase_rank()[2]
        assert s.plan_launch(512, 512)["transport"] == _lib.PLAN_TRANSPORT_RING
        assert not s.plan_ring_moments(512, 512)
    finally:
        s.close()
    s = _handle(monkeypatch, SOSRT_CONTRACT="full")        # the full D x D product: the factors exist and are not used
    try:
        assert s.phase_rank()[0] == 2 and not s.phase_rank()[2] and not s.plan_ring_moments(512, 512)
    finally:
        s.close()


def test_off_with_the_knob(monkeypatch):
    s = _handle(monkeypatch, SOSRT_RING_MOMENTS="0")
    try:
        assert s.phase_rank()[2] and s.plan_launch(512, 512)["transport"] == _lib.PLAN_TRANSPORT_RING
        assert not s.plan_ring_moments(512, 512)
    finally:
        s.close()
    s = _handle(monkeypatch, SOSRT_RING_MOMENTS="1")
    try:
        assert s.plan_ring_moments(512, 512)
    finally:
        s.close()


def test_off_with_atmosphere_sets_saved_orders_and_kept_smallmu_lanes(monkeypatch):
    s = _handle(monkeypatch)
    try:
        assert s.plan_ring_moments(512, 512)
        assert not s.plan_ring_moments(512, 512, atm_sets=True)
        assert not s.plan_ring_moments(512, 512, saved_orders=True)
        # (k_smallmu reads rows of Jn; it runs while some |mu| < 0.01 lane keeps its value: mu = -1/127 on this grid)
        assert not s.plan_ring_moments(512, 512, need_smallmu=True)
    finally:
        s.close()


def test_off_with_a_column_of_more_than_three_zones(monkeypatch):
    s = _handle(monkeypatch)
    try:
        for zones in (5, 7):
            assert s.plan_launch(512, 512, zones=zones)["transport"] == _lib.PLAN_TRANSPORT_RING
            assert not s.plan_ring_moments(512, 512, zones=zones), zones
        assert s.plan_ring_moments(512, 512, zones=3)
    finally:
        s.close()


def test_off_where_another_kernel_transports(monkeypatch):
    for mode in ("scan", "general", "fast"):
        s = _handle(monkeypatch, SOSRT_TRANSPORT=mode)
        try:
            assert s.plan_launch(512, 512)["transport"] != _lib.PLAN_TRANSPORT_RING
            assert not s.plan_ring_moments(512, 512), mode
        finally:
            s.close()
    monkeypatch.delenv("SOSRT_TRANSPORT")


def test_the_count_of_moment_orders_is_zero_before_any_solve(monkeypatch):
    s = _handle(monkeypatch)
    try:
        assert s.ring_moments_stats() == (0, 0)
    finally:
        s.close()
