"""Timing of a spectrum solved wavelength by wavelength against the same spectrum in one batch.

EVA-like log-normal ensemble, L = 200, N = 128, W wavelengths x 8 columns.  Wall-clock (time.perf_counter) around synchronous
calls, two warm-up runs, median of --repeat runs (default 10):
  (a) SOS_Aer_spectrum, the per-wavelength loop            (b) SOS_Aer_spectrum(one_batch=True)
and the parts of (b): the Mie kernels (HIP events, Solver.mie_timing), matrices + fold (table -> P0 rows and matrix per
wavelength on the device, set_phase_sets_device; and, for comparison, the same through the host: phase_matrix,
set_phase_sets), the solve of the W x 8 columns with W aerosol sets, and -- the price of the sets themselves -- the
solve of the same 8 W columns with ONE aerosol (set 0 for all).

    python tools/time_phase_sets.py [--out profiles/phase_sets_timing.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))


def median_ms(fn, repeat, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_sets_timing.txt"))
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--wavelengths", type=int, nargs="*", default=[16, 64])
    a = ap.parse_args()
    import torch
    from sosrt import main as M
    from sosrt.main import SOS_Aer_spectrum

    L, N, C = 200, 128, 8
    mu0 = np.linspace(0.25, 0.95, C)
    rho = np.linspace(0.0, 0.35, C)
    aer = dict(m=1.44 + 0.0j, r_m=0.506, sig=1.2)
    kw = dict(angstrom=1.3, nb_layers=L, nb_angles=N, max_orders=200)
    lines = ["phase sets timing: L = %d, N = %d, %d columns per wavelength, median [min, max] of %d runs, ms" % (L, N, C, a.repeat),
             "device: %s, %d CUs (an MI355X; this is the name torch reports for it)" % (torch.cuda.get_device_name(0),
                                                                                     torch.cuda.get_device_properties(0).multi_processor_count)]
    for W in a.wavelengths:
        wl = np.linspace(0.35, 1.0, W)
        ta = median_ms(lambda: SOS_Aer_spectrum(wl, mu0, 0.12, rho, aer, **kw), a.repeat)
        tb = median_ms(lambda: SOS_Aer_spectrum(wl, mu0, 0.12, rho, aer, one_batch=True, **kw), a.repeat)
        # the parts of (b), on the handle the one-batch call left in the cache
        (s,) = M._solvers.values()
        r, bulk = SOS_Aer_spectrum(wl, mu0, 0.12, rho, aer, one_batch=True, **kw)
        mie = sum(s.mie_timing())
        B = W * C
        sets = np.repeat(np.arange(W, dtype=np.int32), C)
        t_aer = 0.12 * (wl / 0.550) ** -1.3
        t_atm = 0.124 * (0.550 / wl) ** 4
        d_p = torch.empty((W, 6001), dtype=torch.float64, device="cuda")
        s.mie_ensembles_device(d_p.data_ptr(), 0, wl, np.full(W, aer["m"]), np.full(W, aer["r_m"]), np.full(W, aer["sig"]))
        s.synchronize()
        P0r, Ps = np.empty((W, C, 2 * N)), np.empty((W, 2 * N, 2 * N))
        Pa = s.phase_matrix("rayleigh")

        def matrices():
            for w in range(W):
                s.set_phase_table_dev(d_p[w].data_ptr(), 6001)
                P0r[w], Ps[w] = s.phase_p0("table", mu0), s.phase_matrix("table")
            s.set_phase_sets(Pa, Ps)
        tmh = median_ms(matrices, a.repeat)
        d_P = torch.empty((W, 2 * N, 2 * N), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def matrices_dev():
            for w in range(W):
                s.set_phase_table_dev(d_p[w].data_ptr(), 6001)
                s.phase_matrix_device("table", d_P[w].data_ptr())
                P0r[w] = s.phase_p0("table", mu0)
            s.set_phase_sets_device(Pa, d_P.data_ptr(), W)
        tm = median_ms(matrices_dev, a.repeat)
        prep = lambda aer_set: M._prepare_batch(np.tile(mu0, W), np.repeat(t_aer, C), np.tile(rho, W), np.repeat(t_atm, C), 1.0,
                                                np.repeat(bulk[:, 0], C), 120, 25, 17, L, N, "rayleigh", 0.0, "hg", 0.7, None,
                                                None, None, Ps, None, P0r.reshape(B, 2 * N), "specular", 200, 0, aer_set=aer_set)
        out = {}
        for name, aset in (("sets", sets), ("one aerosol", np.zeros(B, dtype=np.int32))):
            s2, tau, P0a, P0x = prep(aset)[:4]
            info = s2.phase_sets_info()
            out[name] = (median_ms(lambda: s2.solve(tau, P0a, P0x, fetch_field=False), a.repeat), info)
        s2.set_aerosol_sets(np.zeros(B, dtype=np.int32))
        f = lambda t: "%9.3f [%8.3f, %8.3f]" % t
        lines += ["", "W = %d wavelengths (%d columns)" % (W, B),
                  "  (a) per-wavelength loop, whole call          %s" % f(ta),
                  "  (b) one_batch=True, whole call               %s   (a)/(b) = %.2f" % (f(tb), ta[0] / tb[0]),
                  "      Mie kernels (HIP events)                 %9.3f" % mie,
                  "      matrices + fold on the device            %s" % f(tm),
                  "      (the same through the host fold          %s)" % f(tmh)]
        for name, (t, info) in out.items():
            lines.append("      solve, %-11s (groups %3d, %s)  %s" % (name, info["groups"], "single pass" if info["single_pass"] else "two passes", f(t)))
        lines.append("      sets / one aerosol = %.3f" % (out["sets"][0][0] / out["one aerosol"][0][0]))
        for s_ in list(M._solvers.values()):
            s_.close()
        M._solvers.clear()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
