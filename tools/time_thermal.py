#!/usr/bin/env python3
"""Cost of the thermal source, Rayleigh + EVA on grey columns (tau*_atm = 0.5, omega_atm = 0.5, omega_aer =
0.8), at three sizes: the C4 batch (512 columns = 8 mu0 x 8 tau*_aer x 8 grd_alb, L = 200, N = 128), one column of that shape,
and one column of the shipped shape (L = 800, N = 501).

    python3 tools/time_thermal.py [reps] [--out FILE]
        call times, milliseconds, median of `reps` after a warm-up (host clock around work that ends in a synchronise): the
        solar call (sosrt_solve_dev) and the thermal call on the same columns (the emitted field, sosrt_solve_dev fed that
        field), and the emission epilogue beside the plain one.  Writes profiles/thermal_timing.txt.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/time_thermal.py [reps] --trace SIZE
        (SIZE: c4 | one | shipped) the same work of one size under the profiler, and the beam first order on the plane path beside
        it; nothing written;
    python3 tools/time_thermal.py --kernels DIR SIZE [--out FILE]
        then reads DIR's kernel trace and appends the median time of the new kernels and, beside them, of k_first_order_beam,
        k_first_order, k_init_from_I1 and k_epilogue to FILE.
"""
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))
import numpy as np  # noqa: E402

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "thermal_timing.txt")
SIZES = {"c4": (200, 128, 8), "one": (200, 128, 1), "shipped": (800, 501, 1)}
NAMES = {"c4": "C4 batch", "one": "one column", "shipped": "shipped shape, one column"}
KERNELS = ["k_emission_view", "k_emission", "k_epilogue_emission", "k_first_order_beam", "k_first_order", "k_init_from_I1", "k_epilogue"]


def kernel_of(name):
    """The kernel of KERNELS a (demangled or mangled) trace name belongs to, the longest match first."""
    for k in sorted(KERNELS, key=len, reverse=True):
        if k in name:
            return k
    return None


def parse(directory, size):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                k = kernel_of(r["Kernel_Name"])
                if k:
                    rows.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not rows:
        sys.exit("no kernel trace under %s" % directory)
    L, N, side = SIZES[size]
    lines = ["%s (B=%d L=%d N=%d): kernel times from the kernel trace, microseconds, median over the launches (first one dropped)"
             % (NAMES[size], side ** 3, L, N)]
    med = {}
    for k in KERNELS:
        if k in rows:
            v = rows[k][1:] or rows[k]
            med[k] = float(np.median(v))
            lines.append("  %-20s %10.2f us  (min %.2f, max %.2f, %d launches)" % (k, med[k], min(v), max(v), len(v)))
    for a, b in (("k_emission", "k_first_order_beam"), ("k_emission", "k_first_order"), ("k_epilogue_emission", "k_epilogue")):
        if a in med and b in med:
            lines.append("  %s / %s = %.2f" % (a, b, med[a] / med[b]))
    print("\n".join(lines))
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


if "--kernels" in sys.argv:
    i = sys.argv.index("--kernels")
    parse(sys.argv[i + 1], sys.argv[i + 2])
    sys.exit(0)

import torch  # noqa: E402

from sosrt import inputs  # noqa: E402
from sosrt.solver import Solver  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(args[0]) if args and args[0].isdigit() else 10
TRACE = sys.argv[sys.argv.index("--trace") + 1] if "--trace" in sys.argv else None
dev = torch.device("cuda", 0)
lines = []


def say(x):
    print(x, flush=True)
    lines.append(x)


def run(size):
    L, N, side = SIZES[size]
    B, D = side ** 3, 2 * N
    g = np.meshgrid(np.linspace(0.2, 1.0, side) if side > 1 else np.array([0.3]), np.geomspace(0.01, 1.0, side) if side > 1 else np.array([0.3]),
                    np.linspace(0.0, 0.8, side) if side > 1 else np.array([0.3]), indexing="ij")
    mu0, taer, rho = (x.reshape(-1).copy() for x in g)
    iu, idn = inputs.slab_indices(120, 25, 17, L)
    tau = np.stack([inputs.tau_profile(0.124, t, 120, 25, 17, L) for t in taer])
    s = Solver(L, N, max_batch=B, max_orders=256)
    s.set_grid(inputs.direction_grid(N))
    s.set_phase_table(*inputs._scalar_phase("eva")[1][1])
    P0a, P0r = s.phase_p0("rayleigh", mu0), s.phase_p0("table", mu0)
    s.set_phase(s.phase_matrix("rayleigh"), s.phase_matrix("table"))
    s.set_columns(np.full(B, iu), np.full(B, idn), mu0, rho, 0.5, 0.8, 0.5 / L, taer / (idn + 1 - iu), 0.5 + taer)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = np.linspace(120, 0, L)
    planck = np.tile((np.maximum(288.0 - 6.5 * z, 216.5) / 288.0) ** 4, (B, 1))
    d_tau, d_z, d_P0a, d_P0r, d_pl, d_bs = t(tau), t(z), t(P0a), t(P0r), t(planck), t(np.ones(B))
    d_sig = t(tau / mu0[:, None])
    d_I0 = torch.empty((B, L, D), dtype=torch.float64, device=dev)
    d_I1 = torch.empty((B, L, D), dtype=torch.float64, device=dev)
    d_I = torch.empty((B, L, D), dtype=torch.float64, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    d_f = torch.empty((4, B, L), dtype=torch.float64, device=dev)
    d_net = torch.empty(B, dtype=torch.float64, device=dev)
    d_view = torch.empty((B, 2, 16), dtype=torch.float64, device=dev)
    vmu = np.linspace(0.05, 1.0, 8)

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        s.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def solar():
        s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I.data_ptr(), d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())

    def stage():
        s.emission_device(d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), d_I0.data_ptr())

    def thermal():
        stage()
        s.solve_device(d_tau.data_ptr(), 0, 0, d_I.data_ptr(), d_I1=d_I0.data_ptr(), d_n_orders=d_n.data_ptr(), d_status=d_st.data_ptr())

    def beam_first():     # the yardstick kernel of the same visit: the layer-by-layer first order on the plane path
        s.first_order_beam_device(d_tau.data_ptr(), d_sig.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I1.data_ptr())

    def view():
        s.emission_view_device(vmu, d_tau.data_ptr(), d_pl.data_ptr(), d_bs.data_ptr(), [0, L - 1], d_view.data_ptr())

    outs = [d_f[i].data_ptr() for i in range(4)] + [d_net.data_ptr()]
    epi = lambda: s.epilogue_device(d_tau.data_ptr(), d_I.data_ptr(), d_z.data_ptr(), "crit", *outs)
    epi_em = lambda: s.epilogue_emission_device(d_tau.data_ptr(), d_I.data_ptr(), d_z.data_ptr(), *outs)
    res, orders = {}, {}
    for name, f in (("solar", solar), ("thermal", thermal), ("stage", stage), ("beam_first", beam_first), ("view", view),
                    ("epilogue", epi), ("epilogue_emission", epi_em)):
        wall(f)
        res[name] = [wall(f) for _ in range(REPS)]
        if name in ("solar", "thermal"):
            orders[name] = (d_n.cpu().numpy().copy(), int((d_st.cpu().numpy() != 0).sum()))
    assert np.all(np.isfinite(d_I0.cpu().numpy())) and np.all(np.isfinite(d_view.cpu().numpy()))
    s.close()
    m = lambda k: (float(np.median(res[k])), min(res[k]), max(res[k]))
    say("%s: B=%d L=%d N=%d Rayleigh + EVA, grey columns, median of %d after warm-up, milliseconds (min, max)" % (NAMES[size], B, L, N, REPS))
    for k in ("solar", "thermal"):
        n, bad = orders[k]
        say("  %-7s call %.3f (%.3f, %.3f)   orders: max %d, sum %d; columns with a non-zero status: %d%s" %
            ((k,) + m(k) + (n.max(), n.sum(), bad, "" if k == "solar" else "   = %.3f x the solar call" % (m("thermal")[0] / m("solar")[0]))))
    say("  of which the emitted field (one launch) %.3f (%.3f, %.3f); the beam first order on the plane path %.3f (%.3f, %.3f)"
        % (m("stage") + m("beam_first")))
    say("  emission at 8 view cosines, 2 levels %.3f (%.3f, %.3f)" % m("view"))
    say("  epilogue %.3f (%.3f, %.3f), emission epilogue %.3f (%.3f, %.3f)" % (m("epilogue") + m("epilogue_emission")))


for size in ([TRACE] if TRACE else list(SIZES)):
    run(size)
if not TRACE:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
