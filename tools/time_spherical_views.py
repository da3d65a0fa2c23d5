#!/usr/bin/env python3
"""Cost of the pseudo-spherical beam in the azimuth and view stages, Rayleigh + EVA, at two sizes: the C4
batch (512 columns = 8 mu0 x 8 tau*_aer x 8 grd_alb, L = 200, N = 128) and one column of that shape.

    python3 tools/time_spherical_views.py [reps] [--out FILE]
        call times, milliseconds, median of `reps` after a warm-up (host clock around work that ends in a synchronise):
        SOS_Aer_batch with beam='spherical', beam_stages=True against the plane call of the same stage, for view_mu (V = 16),
        azimuths (M = 16, 36 azimuths) and view_mu + view_azimuths (both view_first_order settings); then the new entry
        sosrt_view_first_order_beam_dev at nset = 1 and nset = 36 against its yardstick, 1 and 36 calls of
        sosrt_view_radiance_dev for the closed-form first order on the same lanes.  Writes profiles/spherical_views_timing.txt.
    python3 tools/time_spherical_views.py [reps] --plane-only
        the plane driver calls alone (no keyword of this stage is used: runs on a tree without it), printed.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/time_spherical_views.py [reps] --trace SIZE
        (SIZE: c4 | one) the entry-level work of one size under the profiler, nothing written;
    python3 tools/time_spherical_views.py --kernels DIR SIZE [--out FILE]
        then reads DIR's kernel trace and appends the kernels' median times to FILE.
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

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "spherical_views_timing.txt")
SIZES = {"c4": (200, 128, 8), "one": (200, 128, 1)}
NAMES = {"c4": "C4 batch", "one": "one column"}
KERNELS = ["k_view_first_order_beam", "k_view_first_order", "k_prepare"]
V, NSET, M = 16, 36, 16
VIEW_MU = np.linspace(0.05, 1.0, V)
PHI = np.linspace(0.0, np.pi, NSET)


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
    lines = ["%s (B=%d L=%d N=%d V=%d): kernel times from the kernel trace, microseconds" % (NAMES[size], side ** 3, L, N, V)]
    if "k_view_first_order_beam" in rows:
        # the trace run alternates launches at nset = 1 and nset = 36 (the first pair is the warm-up)
        v = rows["k_view_first_order_beam"][2:]
        one, many = v[0::2], v[1::2]
        lines.append("  k_view_first_order_beam nset = 1   %10.2f us  (min %.2f, max %.2f, %d launches)" % (np.median(one), min(one), max(one), len(one)))
        lines.append("  k_view_first_order_beam nset = %d  %10.2f us  (min %.2f, max %.2f, %d launches)" % (NSET, np.median(many), min(many), max(many), len(many)))
        lines.append("  nset = %d over nset = 1: %.2f" % (NSET, np.median(many) / np.median(one)))
    for k in ("k_view_first_order", "k_prepare"):
        if k in rows:
            v = rows[k][1:] or rows[k]
            lines.append("  %-24s %10.2f us  (min %.2f, max %.2f, %d launches); %d launches: %.2f us"
                         % (k, np.median(v), min(v), max(v), len(v), NSET, NSET * np.median(v)))
    print("\n".join(lines))
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


if "--kernels" in sys.argv:
    i = sys.argv.index("--kernels")
    parse(sys.argv[i + 1], sys.argv[i + 2])
    sys.exit(0)

import torch  # noqa: E402

from sosrt import inputs  # noqa: E402
from sosrt.main import SOS_Aer_batch  # noqa: E402
from sosrt.solver import Solver  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(args[0]) if args and args[0].isdigit() else 10
TRACE = sys.argv[sys.argv.index("--trace") + 1] if "--trace" in sys.argv else None
PLANE_ONLY = "--plane-only" in sys.argv
dev = torch.device("cuda", 0)
lines = []


def say(x):
    print(x, flush=True)
    lines.append(x)


def columns(side):
    g = np.meshgrid(np.linspace(0.2, 1.0, side) if side > 1 else np.array([0.3]), np.geomspace(0.01, 1.0, side) if side > 1 else np.array([0.3]),
                    np.linspace(0.0, 0.8, side) if side > 1 else np.array([0.3]), indexing="ij")
    return tuple(x.reshape(-1).copy() for x in g)


def med(v):
    return float(np.median(v)), min(v), max(v)


STAGES = {"view_mu (V = %d)" % V: dict(view_mu=VIEW_MU),
          "azimuths (M = %d, %d azimuths)" % (M, NSET): dict(azimuths=PHI, n_modes=M),
          "view_azimuths, exact (V = %d, M = %d, %d azimuths)" % (V, M, NSET): dict(view_mu=VIEW_MU, view_azimuths=PHI, n_modes=M),
          "view_azimuths, modes (V = %d, M = %d, %d azimuths)" % (V, M, NSET): dict(view_mu=VIEW_MU, view_azimuths=PHI, n_modes=M,
                                                                                   view_first_order="modes")}


def drivers(size):
    L, N, side = SIZES[size]
    mu0, taer, rho = columns(side)
    kw = dict(alb_aer=0.97, nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="eva", raise_on_error=False)

    def wall(**more):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        SOS_Aer_batch(mu0, taer, rho, **dict(kw, **more))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    say("%s: B=%d L=%d N=%d Rayleigh + EVA, SOS_Aer_batch, median of %d after warm-up, milliseconds (min, max)" % (NAMES[size], side ** 3, L, N, REPS))
    for name, stage in STAGES.items():
        wall(**stage)
        plane = [wall(**stage) for _ in range(REPS)]
        say("  %-55s plane     %9.3f (%.3f, %.3f)" % ((name,) + med(plane)))
        if PLANE_ONLY:
            continue
        sph = dict(stage, beam="spherical", beam_stages=True)
        wall(**sph)
        sphere = [wall(**sph) for _ in range(REPS)]
        say("  %-55s spherical %9.3f (%.3f, %.3f)   = %.3f x the plane call" % ((name,) + med(sphere) + (med(sphere)[0] / med(plane)[0],)))


def entry(size):
    L, N, side = SIZES[size]
    B = side ** 3
    mu0, taer, rho = columns(side)
    iu, idn = inputs.slab_indices(120, 25, 17, L)
    tau = np.stack([inputs.tau_profile(0.124, t, 120, 25, 17, L) for t in taer])
    s = Solver(L, N, max_batch=B, max_orders=256)
    s.set_grid(inputs.direction_grid(N))
    s.set_columns(np.full(B, iu), np.full(B, idn), mu0, rho, 1.0, 0.97, 0.124 / L, taer / (idn + 1 - iu), 0.124 + taer)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    d_tau, d_z = t(tau), t(np.linspace(120, 0, L))
    d_p0a, d_p0r = t(0.5 + rng.random((NSET, B, 2 * V))), t(0.5 + rng.random((NSET, B, 2 * V)))     # (timing only: any phase values)
    d_sig = torch.empty((B, L), dtype=torch.float64, device=dev)
    d_out = torch.empty((NSET, B, 2, 2 * V), dtype=torch.float64, device=dev)
    levels = [0, L - 1]
    torch.cuda.synchronize()
    s.beam_slant_device(d_tau.data_ptr(), d_z.data_ptr(), d_sig.data_ptr())
    s.synchronize()

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        s.synchronize()
        return (time.perf_counter() - t0) * 1e3

    beam = lambda nset: s.view_first_order_beam_device(VIEW_MU, d_tau.data_ptr(), d_sig.data_ptr(), d_p0a.data_ptr(), d_p0r.data_ptr(),
                                                       levels, d_out.data_ptr(), nset=nset)

    def closed(n):
        for i in range(n):
            s.view_radiance_device(VIEW_MU, d_tau.data_ptr(), 0, 0, 0, levels, d_first_out=d_out[i].data_ptr(),
                                   d_p0rows_atm=d_p0a[i].data_ptr(), d_p0rows_aer=d_p0r[i].data_ptr(), quadrature="grid")
    res = {}
    if TRACE:
        for _ in range(REPS + 1):                              # launches alternate nset = 1 and nset = 36: `parse` relies on it
            wall(lambda: beam(1))
            wall(lambda: beam(NSET))
        for _ in range(REPS + 1):
            wall(lambda: closed(1))
    else:
        for name, f in (("beam1", lambda: beam(1)), ("beamN", lambda: beam(NSET)), ("closed1", lambda: closed(1)), ("closedN", lambda: closed(NSET))):
            wall(f)
            res[name] = [wall(f) for _ in range(REPS)]
    assert np.all(np.isfinite(d_out.cpu().numpy()))
    s.close()
    if TRACE:
        return
    say("%s: B=%d L=%d N=%d V=%d, levels (0, L - 1), the first order at the view lanes, call times, median of %d, milliseconds (min, max)"
        % (NAMES[size], B, L, N, V, REPS))
    say("  sosrt_view_first_order_beam_dev nset = 1    %.3f (%.3f, %.3f)" % med(res["beam1"]))
    say("  sosrt_view_first_order_beam_dev nset = %d   %.3f (%.3f, %.3f)   = %.2f x nset = 1" % ((NSET,) + med(res["beamN"]) + (med(res["beamN"])[0] / med(res["beam1"])[0],)))
    say("  sosrt_view_radiance_dev (first order only), 1 call    %.3f (%.3f, %.3f)" % med(res["closed1"]))
    say("  sosrt_view_radiance_dev (first order only), %d calls  %.3f (%.3f, %.3f)" % ((NSET,) + med(res["closedN"])))
    say("  new / closed form: %.2f at nset = 1, %.2f at nset = %d" % (med(res["beam1"])[0] / med(res["closed1"])[0],
                                                                     med(res["beamN"])[0] / med(res["closedN"])[0], NSET))


for size in ([TRACE] if TRACE else list(SIZES)):
    if not TRACE:
        drivers(size)
    if not PLANE_ONLY:
        entry(size)
if not TRACE and not PLANE_ONLY:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
