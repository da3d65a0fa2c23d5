#!/usr/bin/env python3
"""Cost of the pseudo-spherical direct beam, Rayleigh + EVA, at three sizes: the C4 batch (512 columns = 8 mu0
x 8 tau*_aer x 8 grd_alb, L = 200, N = 128), one column of that shape, and one column of the shipped shape (L = 800, N = 501).

    python3 tools/time_spherical.py [reps] [--out FILE]
        call times, milliseconds, median of `reps` after a warm-up (host clock around work that ends in a synchronise): the
        plane call (sosrt_solve_dev) and the spherical call (slant path, first order on it, sosrt_solve_dev fed that first
        order), and the beam epilogue beside the plain one.  Writes profiles/spherical_timing.txt.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/time_spherical.py [reps] --trace SIZE
        (SIZE: c4 | one | shipped) the same work of one size under the profiler, nothing written;
    python3 tools/time_spherical.py --kernels DIR SIZE [--out FILE]
        then reads DIR's kernel trace and appends the median time of the three new kernels and, beside them, of
        k_first_order and k_init_from_I1 to FILE.
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

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "spherical_timing.txt")
SIZES = {"c4": (200, 128, 8), "one": (200, 128, 1), "shipped": (800, 501, 1)}
NAMES = {"c4": "C4 batch", "one": "one column", "shipped": "shipped shape, one column"}
KERNELS = ["k_beam_slant", "k_first_order_beam", "k_epilogue_beam", "k_first_order", "k_init_from_I1", "k_epilogue"]


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
    if "k_first_order_beam" in med and "k_first_order" in med:
        lines.append("  k_first_order_beam / k_first_order = %.2f" % (med["k_first_order_beam"] / med["k_first_order"]))
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
    s.set_columns(np.full(B, iu), np.full(B, idn), mu0, rho, 1.0, 0.97, 0.124 / L, taer / (idn + 1 - iu), 0.124 + taer)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_tau, d_z, d_P0a, d_P0r = t(tau), t(np.linspace(120, 0, L)), t(P0a), t(P0r)
    d_sig = torch.empty((B, L), dtype=torch.float64, device=dev)
    d_I1 = torch.empty((B, L, D), dtype=torch.float64, device=dev)
    d_I = torch.empty((B, L, D), dtype=torch.float64, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    d_f = torch.empty((4, B, L), dtype=torch.float64, device=dev)
    d_net = torch.empty(B, dtype=torch.float64, device=dev)

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        s.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def plane():
        s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I.data_ptr(), d_n_orders=d_n.data_ptr())

    def stage():
        s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), d_sig.data_ptr())
        s.first_order_beam_device(d_tau.data_ptr(), d_sig.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I1.data_ptr())

    def spherical():
        stage()
        s.solve_device(d_tau.data_ptr(), d_P0a.data_ptr(), d_P0r.data_ptr(), d_I.data_ptr(), d_I1=d_I1.data_ptr(), d_n_orders=d_n.data_ptr())

    outs = [d_f[i].data_ptr() for i in range(4)] + [d_net.data_ptr()]
    epi = lambda: s.epilogue_device(d_tau.data_ptr(), d_I.data_ptr(), d_z.data_ptr(), "crit", *outs)
    epi_beam = lambda: s.epilogue_beam_device(d_tau.data_ptr(), d_I.data_ptr(), d_sig.data_ptr(), d_z.data_ptr(), "crit", *outs)
    res = {}
    for name, f in (("plane", plane), ("spherical", spherical), ("stage", stage), ("epilogue", epi), ("epilogue_beam", epi_beam)):
        wall(f)
        res[name] = [wall(f) for _ in range(REPS)]
        if name == "plane":
            n_plane = d_n.cpu().numpy().copy()
    n_sph = d_n.cpu().numpy()
    assert np.all(np.isfinite(d_sig.cpu().numpy())) and np.all(np.isfinite(d_I1.cpu().numpy()))
    s.close()
    m = lambda k: (float(np.median(res[k])), min(res[k]), max(res[k]))
    say("%s: B=%d L=%d N=%d Rayleigh + EVA, median of %d after warm-up, milliseconds (min, max)" % (NAMES[size], B, L, N, REPS))
    say("  plane call     %.3f (%.3f, %.3f)   orders: max %d, sum %d" % (m("plane") + (n_plane.max(), n_plane.sum())))
    say("  spherical call %.3f (%.3f, %.3f)   orders: max %d, sum %d   = %.3f x the plane call" %
        (m("spherical") + (n_sph.max(), n_sph.sum(), m("spherical")[0] / m("plane")[0])))
    say("  of which slant path + first order (two launches, one read-back of z) %.3f (%.3f, %.3f)" % m("stage"))
    say("  epilogue %.3f (%.3f, %.3f), beam epilogue %.3f (%.3f, %.3f)" % (m("epilogue") + m("epilogue_beam")))


for size in ([TRACE] if TRACE else list(SIZES)):
    run(size)
if not TRACE:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
