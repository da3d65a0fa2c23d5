#!/usr/bin/env python3
"""Device time of the Mie table builder beside the host series: one EVA ensemble (100 radii, 6001
abscissae) and a batch of 64 wavelengths of it in one call.  Per call: HIP events around the three kernels (warm: the
median of `reps` calls after two warm-up calls), the wall time of the host-output call, and the useful vector-FP64 rate of
the angle kernel (21 flops per (abscissa, radius, term): eight FMA of the amplitude sums, two of the recurrence, three
plain operations) over the FMA rate the library's microbenchmark measures on the same device.  The output of the timed call is compared
with `mie.log_normal_bulk_phase` in the same run.

    python3 tools/time_mie.py [reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sos-radiative-transfer_amd"))
import numpy as np  # noqa: E402

from sosrt import mie  # noqa: E402
from sosrt.solver import Solver  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
R, NTAB = 100, 6001
sc = mie.SCENARIOS["eva"]
s = Solver(2, 4, max_batch=1, max_orders=1)
peak = s.microbench(2)                                       # v_fma_f64, TFLOP/s, measured


def terms(wl):
    x = 2 * np.pi * np.linspace(0.01, 10.0, R)[None, :] / np.atleast_1d(wl)[:, None]
    return np.round(x + 4.0 * x ** (1.0 / 3.0) + 2.0)


def run(what, wl):
    wl = np.atleast_1d(np.asarray(wl, dtype=np.float64))
    ms, wall = [], []
    for rep in range(REPS + 2):
        s.synchronize()
        t0 = time.perf_counter()
        p, bulk = s.mie_ensembles(wl, sc["m"], sc["r_m"], sc["sig"], R, 0.01, 10.0, NTAB)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(s.mie_timing())
    ms, wall = np.median(np.array(ms[2:]), axis=0), float(np.median(wall[2:]))
    nt = terms(wl)
    flops = 21.0 * NTAB * nt.sum()
    print("%s: coefficients %.4f ms, angles %.4f ms, integration %.4f ms, three kernels %.4f ms (%.4f ms per ensemble); call with "
          "host output %.3f ms wall" % (what, ms[0], ms[1], ms[2], ms.sum(), ms.sum() / wl.size, wall))
    print("%s: %d series terms over the radii (longest sphere %d), angle kernel %.3f GFLOP -> %.2f TFLOP/s = %.3f of the measured "
          "v_fma_f64 rate %.1f TFLOP/s" % (what, nt.sum(), nt.max(), flops / 1e9, flops / ms[1] / 1e9, flops / ms[1] / 1e9 / peak, peak))
    return p, bulk, ms


p1, b1, _ = run("one ensemble (eva, 0.55 um)", sc["wl"])
t0 = time.perf_counter()
_, ph = mie.log_normal_bulk_phase(**sc)
host = time.perf_counter() - t0
err = float(np.max(np.abs(p1[0] - ph) / ph))
print("host mie.log_normal_bulk_phase, same arguments, this machine's CPU: %.3f s; device table vs host, max relative %.3e" % (host, err))
assert err <= 1e-12
wl64 = np.linspace(0.35, 1.05, 64)
p64, b64, ms64 = run("64 wavelengths 0.35 .. 1.05 um in one call", wl64)
k = int(np.argmin(np.abs(wl64 - 0.55)))
assert np.all(np.isfinite(p64)) and np.all(p64 > 0)
t0 = time.perf_counter()
_, phk = mie.log_normal_bulk_phase(**dict(sc, wl=float(wl64[k])))
hostk = time.perf_counter() - t0
print("batch row %d (%.4f um) vs host (%.3f s): max relative %.3e; omega %.15g g %.6f" % (k, wl64[k], hostk, float(np.max(np.abs(p64[k] - phk) / phk)), b64[k, 0], b64[k, 1]))
print("SUMMARY one_ensemble_host_s=%.3f batch64_device_ms=%.3f host_over_device_per_ensemble=%.0f" % (host, ms64.sum(), host * 1e3 / (ms64.sum() / 64)))
s.close()
