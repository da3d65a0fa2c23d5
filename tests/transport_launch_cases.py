"""The cases of tests/test_gpu_transport_launch.py, shared with tools/record_transport_launch_bits.py (which records their bits with
the parent commit's library): every distinct way the host feeds a transport launch (csrc/solve.hip: transport_args), on the
smallest shapes that reach it.  A case is (env, plan, run):

  env   the knobs its handles are created under (they are read by sosrt_create);
  plan  what a host-only handle's plan query must say under those knobs -- which kernel the case takes (no GPU);
  run   the library calls; returns (arrays by name, statistics by name).  The arrays are compared as SHA-256 digests with those
        the parent commit's library gave (tests/golden/transport_launch_bits.json), never with the code under test."""
import contextlib
import os

import numpy as np

import driver_cases as DC
import lowrank_stream_cases as LS
import sos_oracle as O
from sosrt import _lib, inputs

KNOBS = ("SOSRT_TRANSPORT", "SOSRT_GROUPS", "SOSRT_SPLIT_MIN", "SOSRT_RING_MOMENTS", "SOSRT_ORDER_LOOP", "SOSRT_SCAN_COLS",
         "SOSRT_SCAN_SPLIT", "SOSRT_RING_SLOTS", "SOSRT_GROUP_RING_SLOTS", "SOSRT_ETAB") + LS.KNOBS
GENERAL, FAST, RING, SCAN = _lib.PLAN_TRANSPORT_GENERAL, _lib.PLAN_TRANSPORT_FAST, _lib.PLAN_TRANSPORT_RING, _lib.PLAN_TRANSPORT_SCAN
ALL_KNOBS = ("general", "fast", "ring", "scan", "auto")
TWO_GROUPS = {"SOSRT_GROUPS": "2", "SOSRT_SPLIT_MIN": "2"}

digest = LS.digest


@contextlib.contextmanager
def knobs(env):
    """The process environment with every knob cleared and `env` set; cached handles are closed on the way in and out."""
    keep = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    LS.fresh()
    try:
        yield
    finally:
        LS.fresh()
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def probe(L, N):
    """A host-only handle with the grid set: answers plan queries under the knobs it was created with."""
    from sosrt.solver import Solver
    s = Solver(L, N, device=-1)
    s.set_grid(inputs.direction_grid(N))
    return s


def planned(L, N, batch, live, **kw):
    s = probe(L, N)
    try:
        return s.plan_launch(batch, live, **kw)
    finally:
        s.close()


# ---- 1. the step entry Solver.transport (not accumulating) --------------------------------------------------------------------------
# A step has no live count: under `auto` it takes what `ring` takes, never the chunk-parallel kernel (csrc/solve.hip:
# plan_step_transport).  So its kernel is the plan's under the same knob, and under `auto` the plan's under `ring`.
STEP_L = 24
STEP_KERNEL = {(32, "general"): GENERAL, (32, "fast"): FAST, (32, "ring"): RING, (32, "scan"): SCAN, (32, "auto"): RING,
               (128, "general"): GENERAL, (128, "fast"): FAST, (128, "ring"): RING, (128, "scan"): SCAN, (128, "auto"): RING,
               (101, "fast"): FAST,                         # odd N: the register-streaming kernel, and the repair launch behind it
               (70, "fast"): GENERAL, (70, "auto"): GENERAL}    # no wave-independent kernel at all


def step_plan(N, knob):
    def check(env):
        with knobs({"SOSRT_TRANSPORT": "ring" if knob == "auto" else knob}):
            p = planned(STEP_L, N, 2, 2)
        assert p["transport"] == STEP_KERNEL[(N, knob)], p
        assert p["repair"] == (1 if (STEP_KERNEL[(N, knob)] == FAST and N - 3 > 61) else 0), p
    return check


def step_inputs(N):
    """Two columns of different depth; at N = 128 the Jn of test_search_beyond_wave0_is_repaired (second differences above 1e-4 over
    the first ~70 upward angles: the upward search leaves wave 0, which sets cv.redo under the register-streaming kernel)."""
    L = STEP_L
    mu = inputs.direction_grid(N)
    tau = np.linspace(0, 0.4, L) ** 1.3
    j = np.arange(N)
    Jn = np.zeros((L, 2 * N))
    Jn[:, :N] = 0.03 + 0.01 * np.linspace(0, 1, N)
    Jn[:, N:] = 0.1 * (1.0 + 0.3 * mu[N:])[None, :] * (1 + 0.2 * np.linspace(0, 1, L))[:, None]
    if N == 128:
        Jn[:, N:] += np.where(j < 70, 0.02 * (-1.0) ** j, 0.0)[None, :]
    return np.stack([tau, 0.5 * tau]), np.stack([Jn, 0.7 * Jn])


def step_run(N):
    def run():
        from sosrt.solver import Solver
        tau, Jn = step_inputs(N)
        s = Solver(STEP_L, N, max_batch=2)
        try:
            s.set_grid(inputs.direction_grid(N))
            s.set_columns_single_slab(np.full(2, 0.5), np.full(2, 1.0), tau[:, -1])
            In, st = s.transport(tau, Jn)
        finally:
            s.close()
        return {"I": In, "status": st}, {}
    return run


# ---- 2. the three columns of tests/driver_cases.py, with and without saved orders ---------------------------------------------------
SOLVE_KERNEL = {"general": GENERAL, "fast": FAST, "ring": RING, "scan": SCAN, "auto": SCAN}      # (auto: 3 columns <= SOSRT_SCAN_COLS)


def batch_arrays(r, saved=False):
    out = {"I": r.I, "n": np.asarray(r.n, dtype=np.int64), "status": np.asarray(r.status, dtype=np.int64)}
    if saved:
        out["I_saved"] = r.I_saved
    return out


def solve_run(save):
    def run():
        from sosrt.main import SOS_Aer_batch
        r = SOS_Aer_batch(DC.MU0, DC.T_AER, DC.RHO, raise_on_error=False, save_orders=save, **DC.SHAPE, **DC.PHASE)
        assert (r.status == 0).all(), r.status
        return batch_arrays(r, save), {}
    return run


def kernel_plan(L, N, batch, live, kernel, groups=1, parts=None, **kw):
    def check(env):
        with knobs(env):
            p = planned(L, N, batch, live, **kw)
        assert p["transport"] == kernel and p["groups"] == groups, p
        if parts is not None:
            assert p["parts"] == parts, p
    return check


# ---- 3. columns that stop at different orders: the transport over the live list, 0 < live < B ----------------------------------------
def conv_run():
    r = LS.conv_solve()
    assert r.n.max() > r.n.min()
    return batch_arrays(r), {}


# ---- 4. two column groups ----------------------------------------------------------------------------------------------------------
# B = 6 at N = 32, groups of three: columns 2 | 3 and 0 | 4 share an optical-depth profile across the group boundary, so the second
# group's columns read attenuation tables built for columns of the first (erep holds whole-batch ids; the table base is not offset)
G6_MU0 = np.array([0.3, 0.5, 0.8, 0.6, 0.4, 0.9])
G6_T_AER = np.array([0.05, 0.15, 0.1, 0.1, 0.05, 0.15])
G6_RHO = np.array([0.1, 0.3, 0.0, 0.2, 0.3, 0.1])
# B = 4 at N = 128 under `scan`: two workgroups per column; the second group's exchange rows and sync words start at column 2
G4_MU0 = np.array([0.3, 0.5, 0.8, 0.6])
G4_T_AER = np.array([0.05, 0.15, 0.1, 0.2])
G4_RHO = np.array([0.1, 0.3, 0.0, 0.2])


def groups_run(N, mu0, t_aer, rho):
    def run():
        from sosrt.main import SOS_Aer_batch
        r = SOS_Aer_batch(mu0, t_aer, rho, raise_on_error=False, nb_layers=24, nb_angles=N, **DC.PHASE)
        return batch_arrays(r), {}
    return run


# ---- 5. a batch holding a five-zone column (tests/test_gpu_shapes.py: test_three_zone_columns_keep_their_bits_...) -----------------
Z_L, Z_N = 48, 64


def zones_run():
    from sosrt.solver import Solver
    L, N = Z_L, Z_N
    mu = inputs.direction_grid(N)
    P0a, Pa = inputs.phase_function("rayleigh", N, mu, 0.6)
    P0r, Pr = inputs.phase_function("hg", N, mu, 0.6, 0.7)
    tau1, r1, mix1, dta1 = inputs.tau_profile_slabs(0.124, [(25, 17, 0.3)], 120, L)
    c2 = O.make_column_slabs(0.6, 120, [(60, 50, 0.2, 0.90), (25, 17, 0.4, 0.97)], L, 0.124, 0.3, 1.0, N, P0a, Pa, P0r, Pr)
    nzmax = len(c2.zones)
    assert nzmax == 5 and len(r1) == 3

    def pad(x, fill=0):
        return list(x) + [fill] * (nzmax - len(x))

    wr1 = pad([0.95 if m else 0.0 for m in mix1])
    zr0 = np.array([pad(r1), [z.r0 for z in c2.zones], pad(r1)], dtype=np.int32)
    zmix = np.array([pad(mix1), [z.kind == "mix" for z in c2.zones], pad(mix1)], dtype=np.int32)
    zwr = np.array([wr1, [z.alb_aer for z in c2.zones], wr1])
    zdt = np.array([pad(dta1), [z.dtau_aer for z in c2.zones], pad(dta1)])
    s = Solver(L, N, max_batch=3, max_orders=100)
    try:
        s.set_grid(mu); s.set_phase(Pa, Pr)
        s.set_columns_zones(zr0, zmix, 0.6, [0.1, c2.grd_alb, 0.5], 1.0, 0.124 / L, zwr, zdt, [0.424, c2.tauStar_tot, 0.424], nz=[3, 5, 3])
        r = s.solve(np.stack([tau1, c2.tau, tau1]), np.tile(P0a, (3, 1)), np.tile(P0r, (3, 1)))
    finally:
        s.close()
    assert (r.status == 0).all(), r.status
    return batch_arrays(r), {}


# ---- 6. the ring kernel's moment mode ----------------------------------------------------------------------------------------------
# (tests/test_gpu_ring_moments.py: the columns start at depth 0.07, so that no |mu| < 0.01 lane keeps its k_smallmu value and the mode runs)
M_L, M_N, M_SLAB, M_TOP, M_TATM = 16, 64, (6, 9), 0.07, 0.124
M_MU0 = np.array([0.35, 0.9, 0.6, 0.5, 0.8, 0.45])
M_TAER = np.array([0.6, 0.02, 0.6, 0.3, 0.02, 0.6])
M_RHO = np.array([0.5, 0.05, 0.7, 0.2, 0.1, 0.6])


def moments_run(B):
    def run():
        from sosrt.solver import Solver
        L, N, (iu, idn) = M_L, M_N, M_SLAB
        mu = inputs.direction_grid(N)
        mu0, taer, rho = M_MU0[:B], M_TAER[:B], M_RHO[:B]
        k = np.arange(L)
        tau = np.stack([M_TOP + k * M_TATM / (L - 1) + np.where(k < iu, 0.0, np.where(k <= idn, (k + 1 - iu) * t / (idn + 1 - iu), t))
                        for t in taer])
        Pa = inputs.phase_function("rayleigh", N, mu, 0.5, 0.0)[1]
        Pr = inputs.phase_function("hg", N, mu, 0.5, 0.7)[1]
        P0a = np.stack([O.phase_p0("rayleigh", N, mu, m, 0.0) for m in mu0])
        P0r = np.stack([O.phase_p0("hg", N, mu, m, 0.7) for m in mu0])
        s = Solver(L, N, max_batch=B, max_orders=200)
        try:
            s.set_grid(mu); s.set_phase(Pa, Pr)
            s.set_columns(np.full(B, iu), np.full(B, idn), mu0, rho, 1.0, 0.95, M_TATM / L, taer / (idn + 1 - iu), M_TOP + M_TATM + taer)
            r = s.solve(tau, P0a, P0r)
            moment_orders, orders = s.ring_moments_stats()
        finally:
            s.close()
        assert (r.status == 0).all(), r.status
        return batch_arrays(r), {"moment_orders": moment_orders, "orders": orders}
    return run


# ---- 7. the order-loop launch: the smallest entry of tests/test_gpu_shapes.py's _OL_SHAPES -------------------------------------------
OL_L, OL_N, OL_B = 50, 32, 7


def order_loop_run():
    from sosrt import main as M
    from sosrt.main import SOS_Aer_batch
    L, N, B = OL_L, OL_N, OL_B
    rng = np.random.default_rng(1000 * L + 7 * N + B)
    mu0 = rng.uniform(0.2, 1.0, B)
    taer = rng.choice([0.02, 0.12, 0.6, 1.0], B)
    rho = rng.uniform(0.0, 0.8, B)
    r = SOS_Aer_batch(mu0, taer, rho, tauStar_atm=0.124, alb_aer=0.95, nb_layers=L, nb_angles=N, max_orders=200, surface="specular",
                      raise_on_error=False)
    (s,) = M._solvers.values()
    launches, refused = s.order_loop_stats()
    return batch_arrays(r), {"launches": launches, "refused": refused}


def order_loop_plan(env):
    with knobs(env):
        p = planned(OL_L, OL_N, OL_B, 1)
    assert p["order_loop"] == 1 and p["ol_grid"] > 0, p


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _cases():
    c = {}
    for N in (32, 128):
        for k in ALL_KNOBS:
            c["step_N%d_%s" % (N, k)] = ({"SOSRT_TRANSPORT": k}, step_plan(N, k), step_run(N))
    for N, k in ((101, "fast"), (70, "fast"), (70, "auto")):
        c["step_N%d_%s" % (N, k)] = ({"SOSRT_TRANSPORT": k}, step_plan(N, k), step_run(N))
    for k in ALL_KNOBS:
        for save in (False, True):
            c["solve3_%s%s" % (k, "_saved" if save else "")] = ({"SOSRT_TRANSPORT": k}, kernel_plan(DC.L, DC.N, 3, 3, SOLVE_KERNEL[k]),
                                                                solve_run(save))
    for k, kern in (("ring", RING), ("scan", SCAN), ("auto", SCAN)):
        c["live_list_%s" % k] = ({"SOSRT_TRANSPORT": k}, kernel_plan(LS.CONV["L"], LS.CONV["N"], 8, 5, kern), conv_run)
    c["groups_B6_erep"] = (dict(TWO_GROUPS), kernel_plan(24, 32, 6, 3, SCAN, groups=2), groups_run(32, G6_MU0, G6_T_AER, G6_RHO))
    c["groups_B4_N128_scan"] = (dict(TWO_GROUPS, SOSRT_TRANSPORT="scan"), kernel_plan(24, 128, 4, 2, SCAN, groups=2, parts=2),
                                groups_run(128, G4_MU0, G4_T_AER, G4_RHO))
    for k, kern in (("general", GENERAL), ("ring", RING), ("scan", SCAN)):
        c["zones5_%s" % k] = ({"SOSRT_TRANSPORT": k}, kernel_plan(Z_L, Z_N, 3, 3, kern, zones=5), zones_run)
    for B, grp in ((3, {}), (6, TWO_GROUPS)):
        for off in (False, True):
            env = dict(grp, SOSRT_TRANSPORT="ring", **({"SOSRT_RING_MOMENTS": "0"} if off else {}))
            c["moments_B%d%s" % (B, "_off" if off else "")] = (env, kernel_plan(M_L, M_N, B, 3, RING, groups=2 if grp else 1), moments_run(B))
    c["order_loop"] = ({"SOSRT_ORDER_LOOP": "1"}, order_loop_plan, order_loop_run)
    return c


CASES = _cases()


def check_plan(name):
    env, plan, _ = CASES[name]
    plan(env)


def run(name):
    """(digests of the case's arrays, its statistics), from handles created under the case's knobs"""
    env, _, fn = CASES[name]
    with knobs(env):
        arrays, stats = fn()
    for k, a in arrays.items():
        assert not np.isnan(np.asarray(a, dtype=np.float64)).any(), (name, k)
    return {k: digest(a) for k, a in arrays.items()}, stats


def check_stats(name, stats):
    """What a case must have done besides giving its bits."""
    if name.startswith("moments_"):
        if name.endswith("_off"):
            assert stats["moment_orders"] == 0 < stats["orders"], stats
        else:
            assert stats["moment_orders"] > 0, stats
    if name == "order_loop":
        assert stats["launches"] >= 1, stats
