#!/usr/bin/env python3
"""Cost of a gas absorption profile: the median of 10 calls after 2 warm-up calls, wall time of a call and the
wait for it.  Every `batch` and `bands` line is a fresh process; the `stages` figures come from ONE process, in the order printed:

  batch     solve_batch_device of 512 columns (L = 200, N = 128, the EVA aerosol, tauStar_aer = 0.05 .. 0.5, mu0 = 0.3 .. 1), the
            field left on the device: with gas_tau, without, and without under SOSRT_MIX_GROUPS=0 -- the ordinary call with its
            slab rows in the two-pass form, the like-for-like yardstick for the contraction under weights; order counts
  stages    sosrt_first_order_profile_dev and sosrt_emission_profile_dev of those columns beside sosrt_first_order_beam_dev and
            sosrt_emission_dev, and sosrt_set_row_weights_dev
  bands     bands.band_thermal at K = 16 points x C = 8 columns with a profile per point ([K, L]) and without

    python3 tools/time_gas_profile.py            (prints; > profiles/gas_profile_timing.txt keeps it)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sos-radiative-transfer_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

REPS, WARM = 10, 2
CHILD_TIMEOUT_S = 300                 # a child that hangs ends the run
L, N, B = 200, 128, 512
Z = np.linspace(120, 0, L)


def gas_profile(total=0.3):
    """A stratospheric layer around 25 km over a scale-height profile near the ground, `total` in all: cumulative from the top."""
    k = 0.6 * np.exp(-0.5 * ((Z - 25.0) / 5.0) ** 2) / 12.5 + 0.4 * np.exp(-Z / 2.0) / 2.0       # per km
    layer = 0.5 * (k[1:] + k[:-1]) * -np.diff(Z)
    g = np.concatenate(([0.0], np.cumsum(layer)))
    return g * (total / g[-1])


def median_ms(fn):
    t = []
    for _ in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[WARM:])), float(min(t[WARM:])), float(max(t[WARM:]))


def columns():
    return np.linspace(0.3, 1.0, B), np.geomspace(0.05, 0.5, B), np.full(B, 0.1)


def child_batch(mode):
    import torch
    from sosrt.main import solve_batch_device
    mu0, t_aer, rho = columns()
    kw = dict(tauStar_atm=0.124, alb_aer=0.97, nb_layers=L, nb_angles=N, aer_phase_fun="eva")
    if mode == "gas":
        kw["gas_tau"] = gas_profile()
    out = {}

    def call():
        out["d"] = solve_batch_device(mu0, t_aer, rho, **kw)[0]
        torch.cuda.synchronize()
    ms = median_ms(call)
    n, st = out["d"]["n"].cpu().numpy(), out["d"]["status"].cpu().numpy()
    return dict(mode=mode, ms=ms, n_sum=int(n.sum()), n_max=int(n.max()), statuses=sorted(set(int(v) for v in st)))


def child_stages(_):
    import torch
    from sosrt.main import _gas_args, _prepare_batch
    mu0, t_aer, rho = columns()
    gas = _gas_args(gas_profile(), B, L)
    s, tau, P0a, P0r, _, _, _, _ = _prepare_batch(mu0, t_aer, rho, 0.124, 1.0, 0.97, 120, 25, 17, L, N, "rayleigh", 0.0, "eva", 0.5, None,
                                                  None, None, None, None, None, "specular", 64, 0, gas=gas)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    d_tau, d_sig, d_P0a, d_P0r, d_w = up(tau), up(tau / mu0[:, None]), up(P0a), up(P0r), up(gas.w)
    d_pl, d_bs = up(np.tile(np.linspace(0.4, 1.0, L), (B, 1))), up(np.ones(B))
    d_out = torch.empty((B, L, 2 * N), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()

    def timed(f):
        def call():
            f()
            s.synchronize()
        return median_ms(call)[0]
    r = {}
    r["beam"] = timed(lambda: s.first_order_beam_device(p(d_tau), p(d_sig), p(d_P0a), p(d_P0r), p(d_out)))
    r["emission"] = timed(lambda: s.emission_device(p(d_tau), p(d_pl), p(d_bs), p(d_out)))
    s.set_row_weights_device(p(d_w), p(d_w))
    r["set"] = timed(lambda: s.set_row_weights_device(p(d_w), p(d_w)))
    r["first_order_profile"] = timed(lambda: s.first_order_profile_device(p(d_tau), p(d_sig), p(d_P0a), p(d_P0r), p(d_out)))
    r["emission_profile"] = timed(lambda: s.emission_profile_device(p(d_tau), p(d_pl), p(d_bs), p(d_out)))
    s.set_row_weights_device(0, 0)
    return r


def child_bands(mode):
    from sosrt import bands
    K, C = 16, 8
    edges = np.array([10, 100, 350, 500, 630, 700, 820, 980, 1080, 1180, 1390, 1480, 1800, 2080, 2250, 2600, 3250], dtype=np.float64)
    T = np.maximum(288.0 - 6.5 * Z, 216.5)
    kw = dict(tauStar_atm=np.linspace(0.3, 0.8, K), alb_atm=0.5, alb_aer=0.8, weights=np.linspace(0.5, 1.5, K), z0=120, nb_layers=L,
              nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.7)
    if mode == "gas":
        kw["gas_tau"] = gas_profile()[None, :] * np.geomspace(0.05, 3.0, K)[:, None]
    out = {}

    def call():
        out["r"] = bands.band_thermal((edges[:-1], edges[1:]), T, 288.0, np.geomspace(0.01, 1.0, C)[None, :], np.linspace(0.0, 0.8, C), **kw)
    ms = median_ms(call)
    r = out["r"]
    return dict(mode=mode, ms=ms, n_sum=int(r.n.sum()), olr=float(r.flux_up[0, 0]), hr_min=float(r.heating_rate[0].min()),
                hr_argmin_km=float(Z[int(np.argmin(r.heating_rate[0]))]))


def fresh(*args, env=None):
    e = dict(os.environ, **(env or {}))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], check=True,
                         stdout=subprocess.PIPE, text=True, env=e, timeout=CHILD_TIMEOUT_S).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child = {"batch": child_batch, "stages": child_stages, "bands": child_bands}[sys.argv[2]]
        print(json.dumps(child(sys.argv[3])))
        sys.exit(0)
    print("# python3 tools/time_gas_profile.py on one MI355X: the median (min, max) of %d calls after %d warm-up calls; every batch and "
          "bands line is a fresh process, the stages figures come from one process in the order printed." % (REPS, WARM))
    print("# batch: solve_batch_device, %d columns, L = %d, N = %d, EVA, tauStar_aer = 0.05 .. 0.5, mu0 = 0.3 .. 1, alb_aer = 0.97, "
          "grd_alb = 0.1; gas_tau: 0.3 in all, a layer at 25 km over a 2 km scale height." % (B, L, N))
    res = {}
    for name, mode, env in (("gas_tau          ", "gas", None), ("no gas           ", "plain", None),
                            ("no gas, two-pass ", "plain", {"SOSRT_MIX_GROUPS": "0"})):
        d = res[name.strip()] = fresh("batch", mode, env=env)
        print("%s: %.2f ms (%.2f, %.2f); orders: sum %d, max %d; statuses %s"
              % (name, d["ms"][0], d["ms"][1], d["ms"][2], d["n_sum"], d["n_max"], d["statuses"]))
    st = fresh("stages", 0)
    print("# stages, the same %d columns resident on the device, one process (ms):" % B)
    print("sosrt_first_order_profile_dev %.3f beside sosrt_first_order_beam_dev %.3f; sosrt_emission_profile_dev %.3f beside "
          "sosrt_emission_dev %.3f" % (st["first_order_profile"], st["beam"], st["emission_profile"], st["emission"]))
    print("sosrt_set_row_weights_dev %.3f" % st["set"])
    print("# bands: bands.band_thermal, K = 16 points x C = 8 columns, L = %d, N = %d, all four outputs." % (L, N))
    bd = {m: fresh("bands", m) for m in ("gas", "plain")}
    for m, name in (("gas", "gas_tau [K, L]"), ("plain", "no gas        ")):
        d = bd[m]
        print("%s: %.2f ms (%.2f, %.2f); orders: sum %d; column 0: outgoing flux %.4f W m-2, strongest cooling %.4g at %.1f km"
              % (name, d["ms"][0], d["ms"][1], d["ms"][2], d["n_sum"], d["olr"], d["hr_min"], d["hr_argmin_km"]))
    print("SUMMARY batch_ms_gas=%.2f batch_ms_plain=%.2f batch_ms_two_pass=%.2f first_order_profile_ms=%.3f first_order_beam_ms=%.3f "
          "band_thermal_ms_gas=%.2f band_thermal_ms_plain=%.2f"
          % (res["gas_tau"]["ms"][0], res["no gas"]["ms"][0], res["no gas, two-pass"]["ms"][0], st["first_order_profile"], st["beam"],
             bd["gas"]["ms"][0], bd["plain"]["ms"][0]))
