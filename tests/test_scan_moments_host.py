"""When an order runs in the chunk-parallel kernel's moment mode (csrc/solve.hip: plan_order, LaunchPlan::scan_moments), asked of
host-only handles through sosrt_plan_scan_moments: a second decision beside the ring kernel's (LaunchPlan::moments,
tests/test_ring_moments_host.py), whose answers must not move -- every point below also asks sosrt_plan_ring_moments."""
import functools

import pytest

from sosrt import _lib, inputs
from sosrt.solver import Solver

L, N = 200, 128
KNOBS = ("SOSRT_RING_MOMENTS", "SOSRT_SCAN_MOMENTS", "SOSRT_SCAN_MOMENTS_MIN", "SOSRT_TRANSPORT", "SOSRT_CONTRACT", "SOSRT_SCAN_SPLIT")


@functools.lru_cache(maxsize=None)
def _matrices(aerosol, n=N):
    mu = inputs.direction_grid(n)
    Pa = inputs.phase_function("rayleigh", n, mu, 0.5)[1]
    Pr = inputs.phase_function(aerosol, n, mu, 0.5, 0.7)[1]
    return Pa, Pr


def _handle(monkeypatch, atmosphere="rayleigh", aerosol="eva", shape=(L, N), **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SOSRT_GROUPS", "1")                # one column group, as the benchmark's sweep runs
    for k, v in env.items():
        monkeypatch.setenv(k, v)                            # (knobs are read when the handle is created)
    s = Solver(shape[0], shape[1], max_batch=512, device=-1)
    s.set_grid(inputs.direction_grid(shape[1]))
    Pa, Pr = _matrices(aerosol, shape[1])
    s.set_phase(_matrices("hg", shape[1])[1] if atmosphere == "hg" else Pa, Pr)
    return s


def _ring_unchanged(s, live, on=None, **kw):
    """sosrt_plan_ring_moments answers what it did before the second mode existed: on exactly where the ring kernel transports
    (and `on` says the handle allows it)"""
    ring = s.plan_launch(512, live, **{k: v for k, v in kw.items() if k in ("surface", "zones")})["transport"] == _lib.PLAN_TRANSPORT_RING
    assert s.plan_ring_moments(512, live, **kw) == (ring if on is None else on), (live, kw)


def test_on_for_rayleigh_over_eva_where_the_chunk_parallel_kernel_runs(monkeypatch):
    s = _handle(monkeypatch)
    try:
        assert s.phase_rank()[0] == 2 and s.phase_rank()[2] and s.phase_asymmetry()[1]
        for live in (200, 128):
            assert s.plan_launch(512, live)["transport"] == _lib.PLAN_TRANSPORT_SCAN
            assert s.plan_scan_moments(512, live), live
            assert not s.plan_ring_moments(512, live), live
        for surface in ("specular", "lambertian", "none"):
            assert s.plan_scan_moments(512, 200, surface=surface, zones=3 if surface != "none" else 1)
    finally:
        s.close()


@pytest.mark.parametrize("threshold", [1, 64, 96, 200])
def test_on_from_the_threshold_up_and_off_below_it(monkeypatch, threshold):
    s = _handle(monkeypatch, SOSRT_SCAN_MOMENTS_MIN=str(threshold))
    try:
        for live in (200, 128, 96, 64, 8, 1):
            assert s.plan_launch(512, live)["transport"] == _lib.PLAN_TRANSPORT_SCAN
            assert s.plan_scan_moments(512, live) == (live >= threshold), (threshold, live)
            _ring_unchanged(s, live)
        assert s.plan_scan_moments(512, threshold)
        assert threshold == 1 or not s.plan_scan_moments(512, threshold - 1)
    finally:
        s.close()


def test_off_where_the_ring_kernel_transports(monkeypatch):
    s = _handle(monkeypatch)
    try:
        for live in (512, 400, 201):
            assert s.plan_launch(512, live)["transport"] == _lib.PLAN_TRANSPORT_RING
            assert not s.plan_scan_moments(512, live), live
            assert s.plan_ring_moments(512, live), live
    finally:
        s.close()
    s = _handle(monkeypatch, SOSRT_TRANSPORT="ring")
    try:
        for live in (512, 200, 64, 1):
            assert not s.plan_scan_moments(512, live) and s.plan_ring_moments(512, live), live
    finally:
        s.close()


def test_the_two_modes_never_answer_together(monkeypatch):
    for env in ({}, {"SOSRT_TRANSPORT": "scan"}, {"SOSRT_TRANSPORT": "ring"}, {"SOSRT_SCAN_MOMENTS_MIN": "1"}):
        s = _handle(monkeypatch, **env)
        try:
            for live in (512, 201, 200, 128, 64, 1):
                assert not (s.plan_scan_moments(512, live) and s.plan_ring_moments(512, live)), (env, live)
        finally:
            s.close()


def test_on_for_every_live_count_with_the_kernel_forced(monkeypatch):
    s = _handle(monkeypatch, SOSRT_TRANSPORT="scan", SOSRT_SCAN_MOMENTS_MIN="1")
    try:
        for live in (512, 200, 64, 1):
            assert s.plan_launch(512, live)["transport"] == _lib.PLAN_TRANSPORT_SCAN
            assert s.plan_scan_moments(512, live) and not s.plan_ring_moments(512, live), live
    finally:
        s.close()


def test_off_without_the_low_rank_form(monkeypatch):
    s = _handle(monkeypatch, atmosphere="hg")              # Henyey-Greenstein molecules: no factorisation within the tolerance
    try:
        assert s.phase_rank()[0] < 0 and not s.phase_rank()[2]
        for live in (200, 128):
            assert s.plan_launch(512, live)["transport"] == _lib.PLAN_TRANSPORT_SCAN
            assert not s.plan_scan_moments(512, live)
        for live in (512, 200, 128):
            _ring_unchanged(s, live, on=False)
    finally:
        s.close()
    s = _handle(monkeypatch, SOSRT_CONTRACT="full")        # the full D x D product: the factors exist and are not used
    try:
        assert s.phase_rank()[0] == 2 and not s.phase_rank()[2] and not s.plan_scan_moments(512, 200)
        _ring_unchanged(s, 512, on=False)
    finally:
        s.close()


def test_off_with_the_knob(monkeypatch):
    s = _handle(monkeypatch, SOSRT_SCAN_MOMENTS="0")
    try:
        assert s.phase_rank()[2]
        for live in (200, 128, 1):
            assert s.plan_launch(512, live)["transport"] == _lib.PLAN_TRANSPORT_SCAN and not s.plan_scan_moments(512, live)
        for live in (512, 201, 200, 128):                   # (the ring kernel's mode has its own knob)
            _ring_unchanged(s, live)
    finally:
        s.close()
    s = _handle(monkeypatch, SOSRT_SCAN_MOMENTS="1", SOSRT_RING_MOMENTS="0")
    try:
        assert s.plan_scan_moments(512, 200) and not s.plan_ring_moments(512, 512)
    finally:
        s.close()


def test_off_with_atmosphere_sets_saved_orders_and_kept_smallmu_lanes(monkeypatch):
    s = _handle(monkeypatch)
    try:
        assert s.plan_scan_moments(512, 200)
        assert not s.plan_scan_moments(512, 200, atm_sets=True)
        assert not s.plan_scan_moments(512, 200, saved_orders=True)
        # (k_smallmu reads rows of Jn; it runs while some |mu| < 0.01 lane keeps its value: mu = -1/127 on this grid)
        assert not s.plan_scan_moments(512, 200, need_smallmu=True)
        for live in (512, 200):
            for kw in ({"atm_sets": True}, {"saved_orders": True}, {"need_smallmu": True}):
                _ring_unchanged(s, live, on=False, **kw)
            _ring_unchanged(s, live)
    finally:
        s.close()


def test_off_with_a_column_of_more_than_three_zones(monkeypatch):
    s = _handle(monkeypatch)
    try:
        for zones in (5, 7):
            assert s.plan_launch(512, 200, zones=zones)["transport"] == _lib.PLAN_TRANSPORT_SCAN
            assert not s.plan_scan_moments(512, 200, zones=zones), zones
            _ring_unchanged(s, 200, on=False, zones=zones)
            _ring_unchanged(s, 512, on=False, zones=zones)
        assert s.plan_scan_moments(512, 200, zones=3)
    finally:
        s.close()


def test_off_for_the_wide_instantiation(monkeypatch):
    """N = 501, L = 800 (the reference's shipped size): the split form's WIDE instantiation transports, which has no moment mode."""
    s = _handle(monkeypatch, shape=(800, 501), SOSRT_SCAN_MOMENTS_MIN="1")
    try:
        assert s.phase_rank()[0] == 2 and s.phase_rank()[2]
        for live in (64, 8, 1):
            plan = s.plan_launch(512, live)
            assert plan["transport"] == _lib.PLAN_TRANSPORT_SCAN and plan["parts"] == 8, plan
            assert not s.plan_scan_moments(512, live), live
            assert not s.plan_ring_moments(512, live), live
    finally:
        s.close()


def test_the_count_of_moment_orders_is_zero_before_any_solve(monkeypatch):
    s = _handle(monkeypatch)
    try:
        assert s.scan_moments_stats() == (0, 0) and s.ring_moments_stats() == (0, 0)
    finally:
        s.close()
