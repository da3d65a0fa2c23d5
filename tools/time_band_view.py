#!/usr/bin/env python3
"""Cost of a channel's view radiances and brightness temperatures in the band drivers: the median of 10 calls
after 2 warm-up calls, wall time of a call and the wait for it.  Every line is a fresh process (a child under a time limit; a child
that fails ends the run).

  brightness  sosrt_brightness_temperature_dev alone at C M = 512 x 2 x 32 elements (512 columns, two levels, 16 view cosines),
              K = 1, 16 and 64 bands of 40 cm^-1 from 400 cm^-1 on, temperatures 200 .. 300 K
  thermal     band_thermal at K = 16, C = 8, L = 200, N = 128 (the sixteen longwave bands and columns of tools/time_gas_profile.py)
              with view_mu (V = 16, the top and the ground) and without, with gas_tau and without
  per_point   the same channel from sixteen SOS_Aer_batch(source='thermal', view_mu=...) calls, one per band, each field brought
              back to the host, summed in NumPy (the host's Planck inversion not counted)

    python3 tools/time_band_view.py            (prints; > profiles/band_view_timing.txt keeps it)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sos-radiative-transfer_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

from time_gas_profile import CHILD_TIMEOUT_S, L, N, REPS, WARM, Z, gas_profile, median_ms  # noqa: E402

K, C, V = 16, 8, 16
EDGES = np.array([10, 100, 350, 500, 630, 700, 820, 980, 1080, 1180, 1390, 1480, 1800, 2080, 2250, 2600, 3250], dtype=np.float64)
TEMPERATURE = np.maximum(288.0 - 6.5 * Z, 216.5)
VIEW = dict(view_mu=np.linspace(0.05, 1.0, V), view_levels=[0, L - 1])
GEOM = dict(z0=120, nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.7)
POINTS = dict(tauStar_atm=np.linspace(0.3, 0.8, K), alb_atm=0.5, alb_aer=0.8)
WEIGHTS = np.linspace(0.5, 1.5, K)
T_AER, RHO = np.geomspace(0.01, 1.0, C), np.linspace(0.0, 0.8, C)


def gas_points():
    return gas_profile()[None, :] * np.geomspace(0.05, 3.0, K)[:, None]


def child_brightness(k):
    import torch
    from sosrt import bands
    from sosrt.main import get_solver
    k, Cb, Mb = int(k), 512, 2 * 32
    lo = 400.0 + 40.0 * np.arange(k)
    hi = lo + 40.0
    rng = np.random.default_rng(k)
    w = rng.uniform(0.5, 1.5, (k, Cb))
    T = rng.uniform(200.0, 300.0, (Cb, Mb))
    R = np.einsum("kc,kcm->cm", w, bands.planck_band(T[None], lo[:, None, None], hi[:, None, None]))
    s = get_solver(24, 32, 1, 64, 0)
    dev = torch.device("cuda", 0)
    d_R, d_w = torch.from_numpy(R).to(dev), torch.from_numpy(w).to(dev)
    d_T = torch.empty((Cb, Mb), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def call():
        s.brightness_temperature_device(d_R.data_ptr(), d_T.data_ptr(), lo, hi, Cb, Mb, d_w.data_ptr())
        s.synchronize()
    ms = median_ms(call)
    err = float(np.max(np.abs(d_T.cpu().numpy() / T - 1)))
    return dict(K=k, ms=ms, round_trip=err)


def child_thermal(mode):
    from sosrt import bands
    kw = dict(POINTS, weights=WEIGHTS, **GEOM)
    if "gas" in mode:
        kw["gas_tau"] = gas_points()
    if "view" in mode:
        kw.update(VIEW)
    out = {}

    def call():
        out["r"] = bands.band_thermal((EDGES[:-1], EDGES[1:]), TEMPERATURE, 288.0, T_AER[None, :], RHO, **kw)
    ms = median_ms(call)
    r = out["r"]
    tb = None if r.brightness_temperature is None else [float(r.brightness_temperature[C // 2, 0, V]), float(r.brightness_temperature[C // 2, 0, -1])]
    return dict(mode=mode, ms=ms, n_sum=int(r.n.sum()), olr=float(r.flux_up[C // 2, 0]), tb=tb,
                toa_nadir=None if r.I_view is None else float(r.I_view[C // 2, 0, -1]))


def child_per_point(mode):
    from sosrt import bands
    from sosrt.main import SOS_Aer_batch
    lo, hi = EDGES[:-1], EDGES[1:]
    b = bands.planck_band(TEMPERATURE[None, :], lo[:, None], hi[:, None])
    bs = bands.planck_band(288.0, lo, hi)
    scale = np.maximum(b.max(axis=1), bs)
    b, bs = b / scale[:, None], bs / scale
    gas = gas_points() if mode == "gas" else None
    out = {}

    def call():
        total = 0.0
        for k in range(K):
            kw = {} if gas is None else dict(gas_tau=gas[k], gas_view=True)
            r = SOS_Aer_batch(0.5, T_AER, RHO, tauStar_atm=POINTS["tauStar_atm"][k], alb_atm=POINTS["alb_atm"], alb_aer=POINTS["alb_aer"],
                              source="thermal", planck=b[k], planck_surface=float(bs[k]), **VIEW, **GEOM, **kw)
            total = total + (WEIGHTS[k] * scale[k]) * r.I_view
        out["I_view"] = total
    ms = median_ms(call)
    return dict(mode=mode, ms=ms, toa_nadir=float(out["I_view"][C // 2, 0, -1]))


def fresh(*args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], check=True,
                         stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT_S).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child = {"brightness": child_brightness, "thermal": child_thermal, "per_point": child_per_point}[sys.argv[2]]
        print(json.dumps(child(*sys.argv[3:])))
        sys.exit(0)
    print("# python3 tools/time_band_view.py on one MI355X: the median of %d calls after %d warm-up calls; every line is a fresh process."
          % (REPS, WARM))
    summary = []
    print("# (a) sosrt_brightness_temperature_dev alone, C M = 512 x 2 x 32 = 32768 elements, bands of 40 cm^-1 from 400 cm^-1, 200 .. 300 K "
          "(ms: median (min, max)):")
    for k in (1, 16, 64):
        d = fresh("brightness", k)
        print("K = %2d: %.3f ms (%.3f, %.3f); round trip %.2e" % (k, d["ms"][0], d["ms"][1], d["ms"][2], d["round_trip"]))
        summary.append("brightness_K%d_ms=%.3f" % (k, d["ms"][0]))
    print("# (b) band_thermal, K = %d, C = %d, L = %d, N = %d, V = %d, levels 0 and %d, results on the host (ms: median (min, max)):"
          % (K, C, L, N, V, L - 1))
    got = {}
    for mode, name in (("view", "view_mu           "), ("plain", "no view_mu        "), ("gas_view", "gas_tau, view_mu  "),
                       ("gas", "gas_tau, no view_mu")):
        d = got[mode] = fresh("thermal", mode)
        print("%s: %.2f ms (%.2f, %.2f); orders: sum %d; flux_up at the top, column %d: %.4f%s"
              % (name, d["ms"][0], d["ms"][1], d["ms"][2], d["n_sum"], C // 2, d["olr"],
                 "" if d["tb"] is None else "; TOA I_view at mu = 1: %.6f; T_b at mu = 0.05 / 1: %.3f / %.3f K" % (d["toa_nadir"], d["tb"][0], d["tb"][1])))
        summary.append("thermal_%s_ms=%.2f" % (mode, d["ms"][0]))
    print("view_mu costs %.2f ms without gas_tau and %.2f ms with it"
          % (got["view"]["ms"][0] - got["plain"]["ms"][0], got["gas_view"]["ms"][0] - got["gas"]["ms"][0]))
    print("# (c) the same channel from %d per-point SOS_Aer_batch(source='thermal', view_mu=...) calls, summed on the host (ms: median (min, max)):" % K)
    for mode, name, band in (("plain", "no gas ", "view"), ("gas", "gas_tau", "gas_view")):
        d = fresh("per_point", mode)
        print("%s: %.2f ms (%.2f, %.2f); TOA I_view at mu = 1, column %d: %.6f; band_thermal(view_mu) takes %.2f of it"
              % (name, d["ms"][0], d["ms"][1], d["ms"][2], C // 2, d["toa_nadir"], got[band]["ms"][0] / d["ms"][0]))
        summary.append("per_point_%s_ms=%.2f" % (mode, d["ms"][0]))
    print("SUMMARY " + " ".join(summary))
