"""The plain rows' stream (csrc/jn_gemm_tile.hpp: lowrank_stream) against the bits of the commit before it: SHA-256 digests of
Solver.source and of whole solves, recorded with that commit's library by tools/record_lowrank_bits.py
(tests/golden/lowrank_stream_bits.json; cases and seeds in tests/lowrank_stream_cases.py).  The stream changes how a wave gets to
its rows and what is in flight, not a row's arithmetic: every digest must be the parent's."""
import json
import os

import numpy as np
import pytest

import lowrank_stream_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lowrank_stream_bits.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_converging_batch_spreads_its_order_counts():
    """(no GPU) The oracle's order counts of the converging batch: three columns stop several orders before the rest, and the rest
    are more than 60 % of the batch -- so the dense tiling runs on with converged columns in its row lists."""
    n = C.conv_oracle_orders()
    early = list(C.CONV_EARLY)
    late = [b for b in range(len(n)) if b not in early]
    print("oracle order counts", n)
    assert 2 <= len(early) <= 3 and len(late) > 0.6 * len(n)
    assert n[early].max() + 5 <= n[late].min(), n


def test_the_recorded_bits_are_the_parents_and_complete():
    """(no GPU) The golden file names a library other than the in-tree one and holds every case."""
    g = _golden()
    assert g["library"] != "libsosrt.so"
    assert set(g["source"]) == set(C.SOURCE_SHAPES) and all(set(v) == set(C.ATMOSPHERES) for v in g["source"].values())
    assert set(g["conv"]) == {"moments", "moments_0"} and set(g["tilings"]) == set(C.ATMOSPHERES)


@pytest.mark.gpu
@pytest.mark.parametrize("atm", C.ATMOSPHERES)
@pytest.mark.parametrize("shape", list(C.SOURCE_SHAPES))
def test_source_has_the_parents_bits(shape, atm):
    """Solver.source (the dense launch, rows of Jn written) at every rank, batch count per wave and width."""
    assert C.source_case(shape, atm) == _golden()["source"][shape][atm]


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["default", "dense", "dense_moments_0", "moments_0"])
def test_columns_that_converge_under_the_dense_tiling(env, monkeypatch):
    """B = 8 with three columns that stop at order 5 while five go on to 45 .. 49: the whole batch has the parent's bits, and every
    column the field and the order count, bit for bit, of the same column solved alone.  `dense`: SOSRT_GEMM_SMALL=0, without which
    a batch this small is tiled over its live columns from the start -- the plan must then say `dense` for 8 and for 5 live columns;
    `moments_0`: SOSRT_RING_MOMENTS=0, the rows of Jn written instead of moment records."""
    from sosrt import _lib
    from sosrt import main as M
    envs = {"default": {}, "dense": {"SOSRT_GEMM_SMALL": "0"}, "dense_moments_0": {"SOSRT_GEMM_SMALL": "0", "SOSRT_RING_MOMENTS": "0"},
            "moments_0": {"SOSRT_RING_MOMENTS": "0"}}[env]
    want = _golden()["conv"]["moments_0" if "moments_0" in env else "moments"]
    B = len(C.CONV["mu0"])
    C.fresh(monkeypatch, **envs)
    try:
        r = C.conv_solve()
        (s,) = M._solvers.values()
        assert s.phase_rank()[0] == 2 and s.phase_rank()[2]
        if "dense" in env:
            for live in (B, B - len(C.CONV_EARLY)):
                assert s.plan_launch(B, live)["gemm"] == _lib.PLAN_GEMM_DENSE, (live, s.plan_launch(B, live))
        C.fresh()
        print("order counts", r.n)
        assert (r.status == 0).all()
        assert [int(x) for x in r.n] == want["orders"]
        assert C.solve_digests(r) == {"I": want["I"], "n": want["n"]}
        for b in range(B):
            one = C.conv_solve(slice(b, b + 1))
            assert one.n[0] == r.n[b], b
            assert np.array_equal(one.I[0], r.I[b]), b
    finally:
        C.fresh()


@pytest.mark.gpu
@pytest.mark.parametrize("tiling", list(C.TILING_ENV))
@pytest.mark.parametrize("atm", C.ATMOSPHERES)
def test_every_tiling_has_the_parents_bits(atm, tiling, monkeypatch):
    """40 columns that stop at different orders, through the default plan and with the live-column tilings forced the way
    tests/test_gpu_contraction_edges.py forces them (the staged small tilings instead of the register tile, the dense tiling
    until the live-column ones -- the register tile or, with both knobs, the 64-row tiling --, the transport over all columns): the parent's bits of its default plan."""
    from sosrt import _lib
    from sosrt import main as M
    want = _golden()["tilings"][atm]
    B = C.TILINGS["B"]
    C.fresh(monkeypatch, **C.TILING_ENV[tiling])
    try:
        r = C.tilings_solve(atm)
        (s,) = M._solvers.values()
        plans = {live: s.plan_launch(B, live)["gemm"] for live in (B, B // 2, 2)}
    finally:
        C.fresh()
    # Which kernels the knobs gave the batch's orders, at 40, 20 and 2 live columns (csrc/solve.hip: plan_order -- at L = 72, N = 64
    # the register tile takes up to 64 columns, so without a knob every order is k_jn_gemm_lone):
    D, L64, L32, DEEP, REGS = (_lib.PLAN_GEMM_DENSE, _lib.PLAN_GEMM_LIVE64, _lib.PLAN_GEMM_LIVE32, _lib.PLAN_GEMM_LIVE32_DEEP,
                               _lib.PLAN_GEMM_LIVE16_REGS)
    expect = {"default": (REGS, REGS, REGS), "dense_live_list_0": (REGS, REGS, REGS),
              "gemm_regs_0": (L32, DEEP, DEEP),              # k_jn_gemm_tail, then k_jn_gemm_tail_deep
              "gemm_small_0": (D, REGS, REGS),               # k_jn_gemm while more than 60 % are live
              "gemm_small_0_regs_0": (D, L64, L64)}[tiling]  # ... then k_jn_gemm_cols
    print("plans", plans)
    assert (plans[B], plans[B // 2], plans[2]) == expect, plans
    assert (r.status == 0).all() and (atm == "zero" or r.n.max() > r.n.min())     # (a zero atmosphere: every column stops at order 2)
    assert [int(r.n.min()), int(r.n.max())] == want["orders"]
    assert C.solve_digests(r) == {"I": want["I"], "n": want["n"]}
