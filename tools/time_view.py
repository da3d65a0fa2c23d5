#!/usr/bin/env python3
"""Cost of the view-radiance stage on the C4 batch: 512 columns = 8 mu0 x 8 tau*_aer x 8 grd_alb, L = 200,
N = 128, Rayleigh + EVA, TOA and surface rows, V = 16 and V = 64 view cosines, both quadratures.  Median of `reps` after one
warm-up, milliseconds: the two row builders (both phase functions), the source contraction, the sweeps and the first order
(HIP events of the library, `Solver.view_timing`), the whole `view_radiance_device` call (host clock around the call and a
wait), and beside them the plain solve of the same visit.  Writes profiles/view_timing.txt.

    python3 tools/time_view.py [reps] [--out FILE]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sosrt import inputs  # noqa: E402
from sosrt.solver import Solver  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(args[0]) if args else 10
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "view_timing.txt")
L, N, side = 200, 128, 8
B, D = side ** 3, 2 * N
g = np.meshgrid(np.linspace(0.2, 1.0, side), np.geomspace(0.01, 1.0, side), np.linspace(0.0, 0.8, side), indexing="ij")
mu0, taer, rho = (x.reshape(-1).copy() for x in g)
iu, idn = inputs.slab_indices(120, 25, 17, L)
tau = np.stack([inputs.tau_profile(0.124, t, 120, 25, 17, L) for t in taer])
dev = torch.device("cuda", 0)
s = Solver(L, N, max_batch=B, max_orders=256)
s.set_grid(inputs.direction_grid(N))
tab = inputs._scalar_phase("eva")[1][1]
s.set_phase_table(*tab)
P0a, P0r = s.phase_p0("rayleigh", mu0), s.phase_p0("table", mu0)
s.set_phase(s.phase_matrix("rayleigh"), s.phase_matrix("table"))
s.set_columns(np.full(B, iu), np.full(B, idn), mu0, rho, 1.0, 0.97, 0.124 / L, taer / (idn + 1 - iu), 0.124 + taer)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_tau, d_mu0, d_P0a, d_P0r = t(tau), t(mu0), t(P0a), t(P0r)
d_I = torch.empty((B, L, D), dtype=torch.float64, device=dev)
d_n = torch.zeros(B, dtype=torch.int32, device=dev)
lines = []


def say(x):
    print(x, flush=True)
    lines.append(x)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    s.synchronize()
    return (time.perf_counter() - t0) * 1e3


med = lambda v: float(np.median(v))
solve = lambda: s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I.data_ptr(), d_n_orders=d_n.data_ptr())
wall(solve)
t_solve = [wall(solve) for _ in range(REPS)]
n = d_n.cpu().numpy()
field_bytes = B * L * D * 8
say("C4 batch: B=%d L=%d N=%d Rayleigh + EVA, levels (0, L-1), median of %d after warm-up; field %.1f MB" % (B, L, N, REPS, field_bytes / 1e6))
say("plain solve: %.3f ms (min %.3f, max %.3f; orders: max %d, sum %d)" % (med(t_solve), min(t_solve), max(t_solve), n.max(), n.sum()))
for V in (16, 64):
    mv = np.linspace(0.02, 1.0, V)
    sgn = np.concatenate((-mv, mv))
    rows = [torch.empty((2 * V, D), dtype=torch.float64, device=dev) for _ in range(2)]
    p0 = [torch.empty((B, 2 * V), dtype=torch.float64, device=dev) for _ in range(2)]
    d_scat = torch.empty((B, 2, 2 * V), dtype=torch.float64, device=dev)
    d_first = torch.empty_like(d_scat)

    def build_rows():
        s.phase_rows_device("rayleigh", sgn, rows[0].data_ptr())
        s.phase_rows_device("table", sgn, rows[1].data_ptr())

    def build_p0():
        s.phase_p0_rows_device("rayleigh", d_mu0.data_ptr(), sgn, p0[0].data_ptr(), B)
        s.phase_p0_rows_device("table", d_mu0.data_ptr(), sgn, p0[1].data_ptr(), B)

    wall(build_rows), wall(build_p0)
    t_rows, t_p0 = [wall(build_rows) for _ in range(REPS)], [wall(build_p0) for _ in range(REPS)]
    say("V=%d builders (both phase functions, wall): k_phase_rows %.3f ms, k_phase_p0_rows %.3f ms" % (V, med(t_rows), med(t_p0)))
    for quad in ("grid", "linear"):
        call = lambda: s.view_radiance_device(mv, d_tau.data_ptr(), d_I.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), [0, L - 1],
                                              d_scat_out=d_scat.data_ptr(), d_first_out=d_first.data_ptr(),
                                              d_p0rows_atm=p0[0].data_ptr(), d_p0rows_aer=p0[1].data_ptr(), quadrature=quad)
        wall(call)
        tw, tk = [], []
        for _ in range(REPS):
            tw.append(wall(call))
            tk.append(s.view_timing())
        src, swp, fst = (med([k[i] for k in tk]) for i in range(3))
        say("V=%d %s: k_view_source %.3f ms (%.2f TB/s of the field read once; %.1f%% of 8 TB/s, %.1f%% of 5.7 TB/s; %.2f TFLOP/s fp64), "
            "k_view_transport %.3f ms (%.3f us per dependent step of its 2 L = %d), k_view_first_order %.3f ms, whole call %.3f ms "
            "(min %.3f, max %.3f) = %.1f%% of the plain solve"
            % (V, quad, src, field_bytes / src / 1e9, 100 * field_bytes / src / 1e9 / 8, 100 * field_bytes / src / 1e9 / 5.7,
               2.0 * B * L * D * 4 * V / src / 1e9, swp, 1e3 * swp / (2 * L), 2 * L, fst, med(tw), min(tw), max(tw),
               100 * med(tw) / med(t_solve)))
assert np.all(np.isfinite(d_scat.cpu().numpy())) and np.all(np.isfinite(d_first.cpu().numpy()))
s.close()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
