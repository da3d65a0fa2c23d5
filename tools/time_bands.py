#!/usr/bin/env python3
"""Cost of band integration: `bands.band_thermal` and `bands.band_solar` at K = 16 spectral points x C = 1, 8
and 32 columns, L = 200, N = 128, Rayleigh + Henyey-Greenstein, beside what a caller does without them: K calls of
`thermal.thermal_toa_flux` (resp. `forcing.toa_net_flux`), one per point, on the same columns, and a weighted sum on the host.
The loop is given its inputs ready-made (the normalised Planck sources of the thermal loop and the phase functions of the solar
loop are built before the clock starts), so it is the loop at its best.

    python3 tools/time_bands.py [reps] [--out FILE]
        call times, milliseconds, median of `reps` after a warm-up (host clock around calls that end in a synchronise and a
        copy to the host).  Writes profiles/bands_timing.txt.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/time_bands.py [reps] --trace C
        the band calls of one C under the profiler; nothing written;
    python3 tools/time_bands.py --kernels DIR C [--out FILE]
        then reads DIR's kernel trace and appends the median times of k_planck_bands and k_band_reduce and, beside them, of
        k_emission, k_epilogue_emission, k_epilogue and k_init_from_I1 to FILE.
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

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "bands_timing.txt")
K, L, N = 16, 200, 128
WIDTHS = (1, 8, 32)
KERNELS = ["k_planck_bands", "k_band_reduce", "k_emission", "k_epilogue_emission", "k_epilogue", "k_init_from_I1"]


def kernel_of(name):
    for k in sorted(KERNELS, key=len, reverse=True):
        if k in name:
            return k
    return None


def parse(directory, C):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                k = kernel_of(r["Kernel_Name"])
                if k:
                    rows.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not rows:
        sys.exit("no kernel trace under %s" % directory)
    lines = ["K=%d points x C=%s columns (L=%d N=%d): kernel times from the kernel trace, microseconds, median over the launches "
             "(first one dropped)" % (K, C, L, N)]
    for k in KERNELS:
        if k in rows:
            v = rows[k][1:] or rows[k]
            lines.append("  %-20s %10.2f us  (min %.2f, max %.2f, %d launches)" % (k, float(np.median(v)), min(v), max(v), len(v)))
    print("\n".join(lines))
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


if "--kernels" in sys.argv:
    i = sys.argv.index("--kernels")
    parse(sys.argv[i + 1], sys.argv[i + 2])
    sys.exit(0)

import torch  # noqa: E402

from sosrt import bands, forcing, inputs, thermal  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(args[0]) if args and args[0].isdigit() else 10
TRACE = int(sys.argv[sys.argv.index("--trace") + 1]) if "--trace" in sys.argv else None
lines = []
GEOM = dict(z0=120, nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.7)
# sixteen longwave bands between 10 and 3250 cm^-1; grey points of the family profiles/thermal_timing.txt solved
EDGES = np.array([10, 100, 350, 500, 630, 700, 820, 980, 1080, 1180, 1390, 1480, 1800, 2080, 2250, 2600, 3250], dtype=np.float64)
Z = np.linspace(120, 0, L)
TEMPERATURE = np.maximum(288.0 - 6.5 * Z, 216.5)


def say(x):
    print(x, flush=True)
    lines.append(x)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def timed(f):
    wall(f)
    out = [wall(f) for _ in range(REPS)]
    t = [o[0] for o in out]
    return (float(np.median(t)), min(t), max(t)), out[-1][1]


def run(C):
    t_aer = np.geomspace(0.01, 1.0, C) if C > 1 else np.array([0.3])
    rho = np.linspace(0.0, 0.8, C) if C > 1 else np.array([0.3])
    lo, hi = EDGES[:-1], EDGES[1:]
    # ---- thermal
    th = dict(tauStar_atm=np.linspace(0.3, 0.8, K), alb_atm=0.5, alb_aer=0.8)
    w = np.linspace(0.5, 1.5, K)
    b = bands.planck_band(TEMPERATURE[None, :], lo[:, None], hi[:, None])
    bs = bands.planck_band(288.0, lo, hi)
    scale = np.maximum(b.max(axis=1), bs)
    b, bs = b / scale[:, None], bs / scale

    def band_th(want=("flux_up",)):
        return bands.band_thermal((lo, hi), TEMPERATURE, 288.0, t_aer[None, :], rho, weights=w, want=want, **th, **GEOM)

    def loop_th():
        olr = np.zeros(C)
        for k in range(K):
            olr += w[k] * scale[k] * thermal.thermal_toa_flux(t_aer, rho, b[k], bs[k], tauStar_atm=th["tauStar_atm"][k], alb_atm=0.5,
                                                              alb_aer=0.8, **GEOM)
        return olr

    if TRACE is not None:
        for _ in range(REPS):
            band_th(bands.WANT)
    else:
        (tb, r), (tl, ref) = timed(band_th), timed(loop_th)
        tf, _ = timed(lambda: band_th(bands.WANT))
        say("thermal, K=%d x C=%d, L=%d N=%d, median of %d after warm-up, milliseconds (min, max); orders: sum %d, max %d"
            % (K, C, L, N, REPS, r.n.sum(), r.n.max()))
        say("  band_thermal (flux_up)        %8.3f (%.3f, %.3f)" % tb)
        say("  %2d x thermal_toa_flux + sum   %8.3f (%.3f, %.3f)   band / loop = %.3f" % ((K,) + tl + (tb[0] / tl[0],)))
        say("  band_thermal (all of `want`)  %8.3f (%.3f, %.3f)" % tf)
        say("  outgoing flux, band call vs loop: %.2e relative" % np.max(np.abs(r.flux_up[:, 0] / ref - 1)))
    # ---- solar: one sun, the columns differ in the layer (forcing.toa_net_flux takes one mu0 and one ground)
    mu0, rho_s = 0.5, 0.1
    t_atm, w_aer = np.geomspace(0.5, 0.02, K), np.linspace(0.99, 0.85, C) if C > 1 else np.array([0.95])
    flux = np.linspace(1.5, 0.5, K)
    mu = inputs.direction_grid(N)
    phases = inputs.phase_function("rayleigh", N, mu, mu0) + inputs.phase_function("hg", N, mu, mu0, 0.7)
    phases = (phases[0], phases[1], phases[2], phases[3])

    def band_so(want=("net_toa",)):
        return bands.band_solar(flux, mu0, t_aer[None, :], rho_s, tauStar_atm=t_atm, alb_atm=1.0, alb_aer=w_aer[None, :], want=want, **GEOM)

    def loop_so():
        net = np.zeros(C)
        for k in range(K):
            net += flux[k] * forcing.toa_net_flux(mu0, t_atm[k], t_aer, rho_s, 1.0, w_aer, z0=120, nb_layers=L, nb_angles=N, phases=phases)
        return net

    if TRACE is not None:
        for _ in range(REPS):
            band_so(bands.WANT)
        return
    (tb, r), (tl, ref) = timed(band_so), timed(loop_so)
    tf, _ = timed(lambda: band_so(bands.WANT))
    say("solar, K=%d x C=%d, L=%d N=%d, median of %d after warm-up, milliseconds (min, max); orders: sum %d, max %d"
        % (K, C, L, N, REPS, r.n.sum(), r.n.max()))
    say("  band_solar (net_toa)          %8.3f (%.3f, %.3f)" % tb)
    say("  %2d x toa_net_flux + sum       %8.3f (%.3f, %.3f)   band / loop = %.3f" % ((K,) + tl + (tb[0] / tl[0],)))
    say("  band_solar (all of `want`)    %8.3f (%.3f, %.3f)" % tf)
    say("  net flux, band call vs loop: %.2e relative" % np.max(np.abs(r.net_toa / ref - 1)))


for C in ([TRACE] if TRACE is not None else WIDTHS):          # (any error ends the tool there, with nothing written)
    run(C)
if TRACE is None:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
