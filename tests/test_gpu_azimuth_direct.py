"""Azimuth-resolved radiance on the device against a direct azimuth-resolved solve (tests/azimuth_direct.py),
which never goes through a Fourier mode.

Exact cases: P0 and P0^m scaled by 1e-6, so that every search of the mu -> 0+ upward blend stops at its first test (asserted on
the reference side) and the solve is linear in P0; the mode-0 solve at tol 1e-4 gives n, modes 1..M run n orders
(sosrt_set_order_targets) with (-1)^m P^m, sosrt_azimuth_accumulate_dev synthesises them, and the result is compared with
the direct solve's own modes 0..M at RTOL.  The direct solve on nq = 2 (nphi - 1) nodes uses the builders' nphi-node quadrature, so its modes
are the mode solves' to rounding whatever M leaves out.  One natural-scale SOS_Aer_batch case bounds what the blend, applied
per mode, costs against the direct solve."""
import numpy as np
import pytest
import torch

import azimuth_direct as D
from sosrt import inputs
from sosrt.main import SOS_Aer_batch
from test_gpu_azimuth import _close, _kind, _solve_targets, _solver, _three_zone
from util import RTOL

pytestmark = pytest.mark.gpu

SCALE = 1e-6
# Natural scale, Rayleigh + HG g = 0.5 three-zone column, mu0 = 0.6, TOA and surface rows: the synthesis misses the direct
# solve by 2.7e-2 of those rows' maximum (mu0 = 0.35 / 0.85: 3.7e-2 / 2.8e-2; Rayleigh alone 1.2-2.1e-3), all of it from the
# blend's field-dependent stopping row; the largest errors sit at upward mu < 0.1 of the surface row.
BLEND_BOUND = 5e-2


def _accumulate(s, Im, phi):
    """sosrt_azimuth_accumulate_dev over modes 0..M of one column, every row: [L, 2N, len(phi)]."""
    dev = torch.device("cuda", 0)
    L, Dd = Im.shape[1:]
    d_Im = [torch.from_numpy(np.ascontiguousarray(I[None])).to(dev) for I in Im]
    d_lev = torch.arange(L, dtype=torch.int32, device=dev)
    d_phi = torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float64)).to(dev)
    out = torch.empty((1, L, Dd, len(phi)), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for m, d in enumerate(d_Im):
        s.azimuth_accumulate_device(m, d.data_ptr(), d_lev.data_ptr(), L, d_phi.data_ptr(), len(phi), out.data_ptr(), B=1)
    s.synchronize()
    return out.cpu().numpy()[0]


@pytest.mark.parametrize("case", ["rayleigh", "rayleigh_hg", "eva"])
def test_device_modes_against_the_direct_solve(case):
    """Three-zone columns: Rayleigh at L = 60, N = 64 (M = 2, nq = 8: all of it), Rayleigh + HG g = 0.5 (M = 24, nq = 96),
    Rayleigh + EVA at L = 200, N = 128 (M = 8, nq = 48 on the reference's 25 nodes)."""
    L, N, aer, g, M, nq, tau_aer = {"rayleigh": (60, 64, "rayleigh", 0.0, 2, 8, 0.3),
                                    "rayleigh_hg": (60, 64, "hg", 0.5, 24, 96, 0.3),
                                    "eva": (200, 128, "eva", 0.0, 8, 48, 0.5)}[case]
    nphi = max(25, nq // 2 + 1)
    mu0 = np.array([0.6])
    s = _solver(L, N, B=1, max_orders=200)
    try:
        ka, fa = _kind(s, "rayleigh")
        kr, fr = _kind(s, aer, g)
        tau, iu, idn = _three_zone(s, 1, mu0, L=L, N=N, tau_aer=tau_aer)
        s.set_phase(s.phase_matrix(ka), s.phase_matrix(kr, g))
        r0 = s.solve(tau, SCALE * s.phase_p0(ka, mu0), SCALE * s.phase_p0(kr, mu0, g), tol=1e-4)
        assert r0.status[0] == 0
        n = int(r0.n[0])
        Pa, Pr = s.phase_modes(ka, 1, M, nphi), s.phase_modes(kr, 1, M, nphi, g)
        P0a, P0r = SCALE * s.phase_p0_modes(ka, mu0, 1, M, nphi), SCALE * s.phase_p0_modes(kr, mu0, 1, M, nphi, g)
        Im = [r0.I[0]]
        for m in range(1, M + 1):
            s.set_phase((-1) ** m * Pa[m - 1], (-1) ** m * Pr[m - 1])   # (the fold's sign, as SOS_Aer_batch applies it)
            I, nn, st = _solve_targets(s, tau, P0a[m - 1], P0r[m - 1], [n])
            assert int(nn[0]) == n and st[0] == 0
            Im.append(I[0])
        Im = np.stack(Im)
        phi = 2 * np.pi * np.arange(nq) / nq
        got = _accumulate(s, Im, phi)
    finally:
        s.close()
    geo = D.three_zone(0.6, L, N, tau_aer=tau_aer)
    with D.record_blend() as log:
        _, Iq = D.direct_solve(geo, fa, fr, nq, n, SCALE)
    assert log and all(log)
    ref = D.synthesize(D.project(Iq, M), phi)
    if case == "rayleigh":                                      # modes 0..2 are all of it
        assert np.max(np.abs(ref - np.moveaxis(Iq, 0, -1))) <= 1e-13 * np.max(np.abs(Iq))
    _close(got, ref, RTOL, "%s, M = %d, n = %d" % (case, M, n))


def test_natural_scale_driver_against_the_direct_solve():
    """SOS_Aer_batch(..., azimuths=) unscaled at TOA and surface (Rayleigh + HG g = 0.5, M = 32, on the direct solve's 96
    nodes): the blend's search stops where each mode field lets it, so the synthesis is within BLEND_BOUND, not RTOL."""
    L, N, M, nq = 60, 64, 32, 96
    phi = 2 * np.pi * np.arange(nq) / nq
    r = SOS_Aer_batch(0.6, 0.3, 0.15, alb_aer=0.95, nb_layers=L, nb_angles=N, atm_phase_fun="rayleigh", aer_phase_fun="hg",
                      g_aer=0.5, max_orders=64, azimuths=phi, n_modes=M, nphi_modes=nq // 2 + 1)
    assert not r.mode_status.any()
    fa, fr = inputs._scalar_phase("rayleigh")[0], inputs._scalar_phase("hg", 0.5)[0]
    with D.record_blend() as log:
        _, Iq = D.direct_solve(D.three_zone(0.6, L, N), fa, fr, nq, int(r.n[0]))
    assert not all(log)                                         # (the case does reach the field-dependent blend)
    ref = np.moveaxis(Iq[:, [0, L - 1]], 0, -1)
    _close(r.I_azimuth[0], ref, BLEND_BOUND, "natural scale, n = %d" % r.n[0])
