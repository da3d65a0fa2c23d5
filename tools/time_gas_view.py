#!/usr/bin/env python3
"""Cost of a gas absorption profile at view angles: the median of 10 calls after 2 warm-up calls, wall time of
a call and the wait for it.  Every line is a fresh process (a child under a time limit; a child that fails ends the run).  The
configuration: 512 columns (L = 200, N = 128, the EVA aerosol, tauStar_aer = 0.05 .. 0.5, mu0 = 0.3 .. 1), V = 16 and V = 64 view
cosines in [0.05, 1], two levels (the top and the ground).

  stages    each new entry beside its unweighted counterpart on a handle without weights: sosrt_view_radiance_profile_dev beside
            sosrt_view_radiance_dev (scattered term only), sosrt_view_first_order_profile_dev beside
            sosrt_view_first_order_beam_dev, sosrt_emission_view_profile_dev beside sosrt_emission_view_dev
  batch     SOS_Aer_batch(gas_tau, view_mu, gas_view=True) beside the same call without view_mu and beside the gas-free view_mu call

    python3 tools/time_gas_view.py            (prints; > profiles/gas_view_timing.txt keeps it)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sos-radiative-transfer_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

from time_gas_profile import columns, gas_profile  # noqa: E402

REPS, WARM = 10, 2
CHILD_TIMEOUT_S = 300                 # a child that hangs ends the run
L, N, B = 200, 128, 512
LEVELS = [0, L - 1]


def view_mu(V):
    return np.linspace(0.05, 1.0, V)


def median_ms(fn):
    t = []
    for _ in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[WARM:])), float(min(t[WARM:])), float(max(t[WARM:]))


def child_stages(V):
    import torch
    from sosrt.main import _gas_args, _phase_kind, _prepare_batch
    V = int(V)
    mv = view_mu(V)
    sgn = np.concatenate((-mv, mv))
    mu0, t_aer, rho = columns()
    gas = _gas_args(gas_profile(), B, L)
    s, tau, P0a, P0r, _, _, _, _ = _prepare_batch(mu0, t_aer, rho, 0.124, 1.0, 0.97, 120, 25, 17, L, N, "rayleigh", 0.0, "eva", 0.5, None,
                                                  None, None, None, None, None, "specular", 64, 0, gas=gas)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    d_tau, d_sig, d_w, d_mu0 = up(tau), up(tau / mu0[:, None]), up(gas.w), up(mu0)
    d_pl, d_bs = up(np.tile(np.linspace(0.4, 1.0, L), (B, 1))), up(np.ones(B))
    rng = np.random.default_rng(1)
    d_I = up(0.05 + rng.random((B, L, 2 * N)))
    rows, p0rows = [], []
    for phase in (("rayleigh", 0.0, None), ("eva", 0.5, None)):
        kind, g = _phase_kind(s, *phase)
        rw, p0 = new(2 * V, 2 * N), new(B, 2 * V)
        torch.cuda.synchronize()
        s.phase_rows_device(kind, sgn, rw.data_ptr(), g)
        s.phase_p0_rows_device(kind, d_mu0.data_ptr(), sgn, p0.data_ptr(), B, g)
        rows.append(rw)
        p0rows.append(p0)
    d_out = new(B, len(LEVELS), 2 * V)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()

    def timed(f):
        def call():
            f()
            s.synchronize()
        return median_ms(call)[0]
    r = {"V": V}
    r["view_radiance"] = timed(lambda: s.view_radiance_device(mv, p(d_tau), p(d_I), p(rows[0]), p(rows[1]), LEVELS, d_scat_out=p(d_out)))
    r["view_first_order_beam"] = timed(lambda: s.view_first_order_beam_device(mv, p(d_tau), p(d_sig), p(p0rows[0]), p(p0rows[1]), LEVELS,
                                                                              p(d_out)))
    r["emission_view"] = timed(lambda: s.emission_view_device(mv, p(d_tau), p(d_pl), p(d_bs), LEVELS, p(d_out)))
    s.set_row_weights_device(p(d_w), p(d_w))
    r["view_radiance_profile"] = timed(lambda: s.view_radiance_profile_device(mv, p(d_tau), p(d_I), p(rows[0]), p(rows[1]), LEVELS, p(d_out)))
    r["view_first_order_profile"] = timed(lambda: s.view_first_order_profile_device(mv, p(d_tau), p(d_sig), p(p0rows[0]), p(p0rows[1]),
                                                                                    LEVELS, p(d_out)))
    r["emission_view_profile"] = timed(lambda: s.emission_view_profile_device(mv, p(d_tau), p(d_pl), p(d_bs), LEVELS, p(d_out)))
    s.set_row_weights_device(0, 0)
    return r


def child_batch(mode, V):
    from sosrt.main import SOS_Aer_batch
    mu0, t_aer, rho = columns()
    kw = dict(tauStar_atm=0.124, alb_aer=0.97, nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="eva", raise_on_error=False)
    view = dict(view_mu=view_mu(int(V)), view_levels=LEVELS)
    kw.update({"gas_view": dict(gas_tau=gas_profile(), gas_view=True, **view), "gas": dict(gas_tau=gas_profile()), "view": view}[mode])
    out = {}

    def call():
        out["r"] = SOS_Aer_batch(mu0, t_aer, rho, **kw)
    ms = median_ms(call)
    r = out["r"]
    toa = None if r.I_view is None else float(r.I_view[B // 2, 0, -1])
    return dict(mode=mode, V=int(V), ms=ms, n_sum=int(r.n.sum()), statuses=sorted(set(int(v) for v in r.status)), toa_nadir=toa)


def fresh(*args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], check=True,
                         stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT_S).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child = {"stages": child_stages, "batch": child_batch}[sys.argv[2]]
        print(json.dumps(child(*sys.argv[3:])))
        sys.exit(0)
    print("# python3 tools/time_gas_view.py on one MI355X: the median of %d calls after %d warm-up calls; every line is a fresh process."
          % (REPS, WARM))
    print("# %d columns, L = %d, N = %d, EVA, tauStar_aer = 0.05 .. 0.5, mu0 = 0.3 .. 1, alb_aer = 0.97, grd_alb = 0.1; gas_tau: 0.3 in "
          "all, a layer at 25 km over a 2 km scale height; view cosines 0.05 .. 1, levels 0 and %d." % (B, L, N, L - 1))
    print("# stages, the columns resident on the device (ms; the new entry, its unweighted counterpart on a handle without weights, the ratio):")
    pairs = (("view_radiance_profile", "view_radiance"), ("view_first_order_profile", "view_first_order_beam"),
             ("emission_view_profile", "emission_view"))
    summary = []
    for V in (16, 64):
        st = fresh("stages", V)
        for new, old in pairs:
            print("V = %2d: sosrt_%s_dev %.3f beside sosrt_%s_dev %.3f: %.2fx" % (V, new, st[new], old, st[old], st[new] / st[old]))
            summary.append("%s_V%d_ms=%.3f %s_V%d_ms=%.3f" % (new, V, st[new], old, V, st[old]))
    print("# batch: the whole SOS_Aer_batch call, results on the host (ms: median (min, max)):")
    for V in (16, 64):
        for mode, name in (("gas_view", "gas_tau, view_mu, gas_view=True"), ("gas", "gas_tau, no view_mu            "),
                           ("view", "no gas, view_mu                ")):
            d = fresh("batch", mode, V)
            print("V = %2d: %s: %.2f ms (%.2f, %.2f); orders: sum %d; statuses %s%s"
                  % (V, name, d["ms"][0], d["ms"][1], d["ms"][2], d["n_sum"], d["statuses"],
                     "" if d["toa_nadir"] is None else "; TOA I_view at mu = 1, column %d: %.6f" % (B // 2, d["toa_nadir"])))
            summary.append("batch_%s_V%d_ms=%.2f" % (mode, V, d["ms"][0]))
    print("SUMMARY " + " ".join(summary))
