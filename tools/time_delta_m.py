#!/usr/bin/env python3
"""Times of delta-M, every measurement in a fresh process, the median of 10 calls after 2 warm-up calls:

  kernels   sosrt_phase_moments_dev and sosrt_phase_delta_m_dev at ntab = 6001, lmax = order = 128, S = 1 and 64 tables resident
            on the device (wall time of the call and the wait for it; the delta-M entry includes its copy of the moments to the
            host), beside the NumPy model of tests/deltam_np.py on the same machine
  driver    SOS_Aer_batch of 512 columns of the cloud table 'fwc' (L = 200, N = 128, tauStar_aer = 0.2, mu0 = 0.3 .. 1) with
            delta_m=16 and without: whole-call wall time, order counts, statuses; the same columns through solve_batch_device
            (the field stays on the device); and the delta-M step of a call alone

    python3 tools/time_delta_m.py            (prints; > profiles/delta_m_timing.txt keeps it)"""
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
NTAB, LMAX = 6001, 128


def median_ms(fn):
    t = []
    for _ in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[WARM:]))


def child_kernels(S):
    import torch
    import deltam_np as DM
    from sosrt.solver import Solver
    dev = torch.device("cuda", 0)
    s = Solver(2, 4, max_batch=1, max_orders=1)
    x = np.linspace(-1, 1, NTAB)
    P = np.stack([DM.hg(0.85 - 0.005 * k)(x) for k in range(S)])
    d_P = torch.from_numpy(P).to(dev)
    d_chi = torch.empty((S, LMAX + 1), dtype=torch.float64, device=dev)
    d_out = torch.empty((S, NTAB), dtype=torch.float64, device=dev)
    d_f = torch.empty(S, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def moments():
        s.phase_moments_device(d_P.data_ptr(), S, NTAB, LMAX, d_chi.data_ptr())
        s.synchronize()

    def table():
        s.delta_m_table_device(d_chi.data_ptr(), S, LMAX, LMAX, NTAB, d_out.data_ptr(), d_f.data_ptr())
        s.synchronize()
    r = dict(S=S, moments_ms=median_ms(moments), table_ms=median_ms(table))
    chi = d_chi.cpu().numpy()
    t0 = time.perf_counter()
    want = np.stack([DM.moments(None, P[k], LMAX)[0] for k in range(S)])
    r["model_moments_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    wt = np.stack([DM.delta_m_table(chi[k], LMAX, x)[0] for k in range(S)])
    r["model_table_ms"] = (time.perf_counter() - t0) * 1e3
    r["moments_err"] = float(np.max(np.abs(chi - want)))
    r["table_err"] = float(np.max(np.abs(d_out.cpu().numpy() - wt)))
    s.close()
    return r


def child_driver(order):
    from sosrt.main import SOS_Aer_batch
    B = 512
    mu0 = np.linspace(0.3, 1.0, B)
    kw = dict(tauStar_atm=0.124, alb_aer=0.99, nb_layers=200, nb_angles=128, aer_phase_fun="fwc", raise_on_error=False)
    if order:
        kw["delta_m"] = order
    out = {}

    def call():
        out["r"] = SOS_Aer_batch(mu0, np.full(B, 0.2), np.full(B, 0.1), **kw)
    ms = median_ms(call)
    r = out["r"]
    ok = r.status == 0
    return dict(order=order, call_ms=ms, converged=int(ok.sum()), statuses=sorted(set(int(v) for v in r.status)),
                n_min=int(r.n[ok].min()) if ok.any() else 0, n_median=float(np.median(r.n[ok])) if ok.any() else 0,
                n_max=int(r.n[ok].max()) if ok.any() else 0, n_sum=int(r.n.sum()),
                f=None if r.delta_m_f is None else float(r.delta_m_f))


def child_resident(order):
    """The same columns through solve_batch_device: the field stays on the device, so the call is the inputs and the solve."""
    import torch
    from sosrt.main import solve_batch_device
    B = 512
    mu0 = np.linspace(0.3, 1.0, B)
    kw = dict(tauStar_atm=0.124, alb_aer=0.99, nb_layers=200, nb_angles=128, aer_phase_fun="fwc")
    if order:
        kw["delta_m"] = order

    def call():
        solve_batch_device(mu0, np.full(B, 0.2), np.full(B, 0.1), **kw)
        torch.cuda.synchronize()
    return dict(order=order, call_ms=median_ms(call))


def child_chain(order):
    """The delta-M step of a driver call alone: the table up, moments, truncated table, the handle's table, f back."""
    from sosrt import deltam
    from sosrt.solver import Solver
    s = Solver(2, 4, max_batch=1, max_orders=1)

    def call():
        f, _, keep = deltam.delta_m(s, "fwc", order)
        keep["truncated"].cpu()
    ms = median_ms(call)
    s.close()
    return dict(order=order, call_ms=ms)


def fresh(*args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child = {"kernels": child_kernels, "driver": child_driver, "resident": child_resident, "chain": child_chain}[sys.argv[2]]
        print(json.dumps(child(int(sys.argv[3]))))
        sys.exit(0)
    print("# python3 tools/time_delta_m.py on one MI355X: every line a fresh process, the median of %d calls after %d warm-up calls." % (REPS, WARM))
    print("# kernels: wall time of the call and the wait for it, tables resident on the device; ntab = %d, lmax = order = %d." % (NTAB, LMAX))
    for S in (1, 64):
        k = fresh("kernels", S)
        print("S = %2d: sosrt_phase_moments_dev %.4f ms (NumPy model on this machine's CPU %.1f ms, |chi - model| <= %.2e); "
              "sosrt_phase_delta_m_dev %.4f ms with its copy of the moments to the host (model %.1f ms, |table - model| <= %.2e)"
              % (k["S"], k["moments_ms"], k["model_moments_ms"], k["moments_err"], k["table_ms"], k["model_table_ms"], k["table_err"]))
    print("# driver: SOS_Aer_batch, 512 columns of 'fwc', L = 200, N = 128, tauStar_aer = 0.2, mu0 = 0.3 .. 1, alb_aer = 0.99, grd_alb = 0.1.")
    res = {}
    for order in (0, 16):
        d = res[order] = fresh("driver", order)
        print("%s: whole call %.2f ms; %d of 512 columns converged (statuses %s); orders of the converged columns min %d, median %g, "
              "max %d; sum over all columns %d%s"
              % ("delta_m=16" if order else "no delta_m ", d["call_ms"], d["converged"], d["statuses"], d["n_min"], d["n_median"],
                 d["n_max"], d["n_sum"], "; f = %.6f" % d["f"] if d["f"] is not None else ""))
    dev = {order: fresh("resident", order)["call_ms"] for order in (0, 16)}
    print("solve_batch_device, the same columns, the field left on the device: no delta_m %.2f ms, delta_m=16 %.2f ms"
          % (dev[0], dev[16]))
    print("the delta-M step of a call alone (deltam.delta_m of 'fwc' at 16 and the truncated table's copy to the host): %.3f ms"
          % fresh("chain", 16)["call_ms"])
    print("SUMMARY call_ms_plain=%.2f call_ms_delta_m=%.2f resident_ms_plain=%.2f resident_ms_delta_m=%.2f orders_sum_plain=%d "
          "orders_sum_delta_m=%d" % (res[0]["call_ms"], res[16]["call_ms"], dev[0], dev[16], res[0]["n_sum"], res[16]["n_sum"]))
