"""Handle-level Python API over the C ABI (host NumPy arrays in, NumPy arrays out;
`solve_device` works on resident device buffers, e.g. torch tensors)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, lib


def _f64(a, shape=None, name="array"):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, a.shape, tuple(shape)))
    return a


def _i32(a, n, name):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.shape != (n,):
        raise ValueError("%s has shape %s, expected (%d,)" % (name, a.shape, n))
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _vp(address):
    """A device address (an integer, e.g. torch's `tensor.data_ptr()`) as the C ABI takes it; 0 is the null pointer."""
    return ctypes.c_void_p(address) if address else None


def _vec(x, B, name):
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (B,)))
    return a


def _surface_code(surface):
    # 'lambertian' is the reference's file as coded (lam:399/401: negative reflected radiance);
    # 'lambertian_readme' the same term with the sign of the reference's README.md:215
    sf = {"specular": _lib.SURFACE_SPECULAR, "lambertian": _lib.SURFACE_LAMBERTIAN,
          "lambertian_readme": _lib.SURFACE_LAMBERTIAN_README}.get(surface)
    if sf is None:
        raise ValueError("surface must be 'specular', 'lambertian' or 'lambertian_readme', got %r" % (surface,))
    return sf


@dataclass
class DevicePhaseSets:
    """S aerosol phase matrices resident on the device ([S, 2N, 2N] float64 at `address`), for `SOS_Aer_batch(P_aer=...)`
    with `aer_set`: they are handed to `Solver.set_phase_sets_device`.  `keep` holds whatever owns the memory."""
    address: int
    S: int
    keep: object = None


@dataclass
class SolveResult:
    I: np.ndarray                  # [B, L, 2N]
    n: np.ndarray                  # [B] final order count (spec:307-310)
    status: np.ndarray             # [B] SOSRT_COL_*
    I_saved: Optional[np.ndarray]  # [B, max(n), L, 2N] (slots >= n[b] are zero) or None


class Solver:
    """One sosrt handle: fixed (nb_layers, nb_angles), a direction grid, a pair of phase
    matrices and a batch of columns."""

    def __init__(self, nb_layers: int, nb_angles: int, max_batch: int = 1, max_orders: int = 64, device: int = 0):
        self.L, self.N, self.D = int(nb_layers), int(nb_angles), 2 * int(nb_angles)
        self.max_batch, self.max_orders, self.device = int(max_batch), int(max_orders), int(device)
        self._h = ctypes.c_void_p()
        check(lib().sosrt_create(self.device, self.L, self.N, self.max_batch, self.max_orders, ctypes.byref(self._h)))
        self.B = 0
        self.order_budget = self.max_orders
        self.mu = None
        self._P = (None, None)
        self._p0_zones = 0          # > 0: P0_aer is [B, _p0_zones, 2N] (set_aerosol_sets with a zone table)
        self.single_slab = False    # the current columns are set_columns_single_slab's

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().sosrt_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup -------------------------------------------------------------
    def set_stream(self, stream_handle: Optional[int]):
        """Run on a caller's HIP stream (its integer handle, e.g. `torch.cuda.current_stream().cuda_stream`).  0 is the
        legacy default stream -- torch's default stream -- exactly as in HIP; None goes back to the handle's own stream (a
        blocking stream: it too orders against the default stream)."""
        if stream_handle is None:
            check(lib().sosrt_use_own_stream(self._h))
        else:
            check(lib().sosrt_set_stream(self._h, ctypes.c_void_p(stream_handle) if stream_handle else None))

    def synchronize(self):
        check(lib().sosrt_synchronize(self._h))

    def set_contraction(self, mode="f64"):
        """'f64' (default, the parity path: fp64; the plain rows in the low-rank form of W_atm when it has one, the MFMA product
        elsewhere, using the flip symmetry of the folded matrices when they have it) | 'f64_dense' ('f64' without the low-rank
        form: the MFMA product on every row) | 'f64_full' (fp64 MFMA, always the full 2N x 2N product) | 'f32' (float operands
        and accumulator in the dense Jn contraction: opt-in, about 3e-7 away from the fp64 result; BASELINE configs[4])."""
        m = {"f64": _lib.CONTRACT_F64, "f32": _lib.CONTRACT_F32, "f64_full": _lib.CONTRACT_F64_FULL,
             "f64_dense": _lib.CONTRACT_F64_DENSE}.get(mode)
        if m is None:
            raise ValueError("contraction must be 'f64', 'f64_dense', 'f64_full' or 'f32'")
        check(lib().sosrt_set_contraction(self._h, m))

    def set_order_budget(self, max_orders: int):
        """The solves that follow run at most `max_orders` orders (<= the handle's max_orders); a column still iterating then
        has status COL_MAXORDERS."""
        check(lib().sosrt_set_order_budget(self._h, int(max_orders)))
        self.order_budget = int(max_orders)

    def set_order_loop(self, on=True):
        """Whether the last orders of the last few live columns run in ONE launch (csrc/order_loop.hip).  0 / False (the
        library's default: the launch has the same bits and was measured slower) every order stays two launches; 1 / True
        one launch where the launch plan says so; 2 a test mode whose launch is always refused, so that the hand-back to
        the two-launch orders runs (include/sosrt.h, sosrt_set_order_loop)."""
        check(lib().sosrt_set_order_loop(self._h, int(on) if on in (0, 1, 2) else (1 if on else 0)))

    def order_loop_stats(self, column_orders=False):
        """(order-loop launches of the last solve, launches that found their grid not resident and handed back[, the (column,
        order) pairs that ran inside them -- synchronises])"""
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        check(lib().sosrt_order_loop_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c) if column_orders else None))
        return (a.value, b.value, c.value) if column_orders else (a.value, b.value)

    def phase_asymmetry(self):
        """(max |W[k][m] - W[2N-1-k][2N-1-m]| / max |W| of the folded matrices, whether the next solve uses the symmetry)"""
        a, u = ctypes.c_double(), ctypes.c_int()
        check(lib().sosrt_phase_asymmetry(self._h, ctypes.byref(a), ctypes.byref(u)))
        return a.value, bool(u.value)

    def phase_rank(self):
        """(rank r of the low-rank form of the folded W_atm, or -1; max |W_atm - U V| / max |W_atm|; whether the next solve
        computes its plain rows in that form)"""
        r, a, u = ctypes.c_int(), ctypes.c_double(), ctypes.c_int()
        check(lib().sosrt_phase_rank(self._h, ctypes.byref(r), ctypes.byref(a), ctypes.byref(u)))
        return r.value, a.value, bool(u.value)

    def set_first_order(self, mode="coded"):
        """'coded' (default): spec:104-292, what both mains of the reference compute (specularly reflected beam).
        'readme': the Lambertian first order of the reference's README.md:126-171 (direct beam + the beam reflected
        isotropically by the ground + isotropic reflection of the downward first order) -- PARITY UNPINNED, the
        reference has no runnable code for it; meant for surface='lambertian_readme', after set_columns."""
        m = {"coded": _lib.FIRST_ORDER_CODED, "readme": _lib.FIRST_ORDER_README}.get(mode)
        if m is None:
            raise ValueError("first_order must be 'coded' or 'readme'")
        check(lib().sosrt_set_first_order(self._h, m))

    def set_grid(self, mu):
        mu = _f64(mu, (self.D,), "mu")
        check(lib().sosrt_set_grid(self._h, _ptr(mu)))
        self.mu = mu.copy()
        self._P = (None, None)

    def set_phase(self, P_atm, P_aer=None):
        Pa = _f64(P_atm, (self.D, self.D), "P_atm")
        Pr = None if P_aer is None else _f64(P_aer, (self.D, self.D), "P_aer")
        check(lib().sosrt_set_phase(self._h, _ptr(Pa), _ptr(Pr)))
        self._P = (Pa.copy(), None if Pr is None else Pr.copy())

    def set_phase_sets(self, P_atm, P_aer_sets):
        """Several aerosol phase matrices `P_aer_sets` [S, 2N, 2N] beside one P_atm; `set_aerosol_sets` says which one the
        aerosol of a column (or of an aerosol zone) reads -- set 0 until then.  S = 1 is `set_phase`, bit for bit."""
        Pa = _f64(P_atm, (self.D, self.D), "P_atm")
        Pr = np.ascontiguousarray(P_aer_sets, dtype=np.float64)
        if Pr.ndim != 3 or Pr.shape[1:] != (self.D, self.D):
            raise ValueError("P_aer_sets has shape %s, expected (S, %d, %d)" % (Pr.shape, self.D, self.D))
        check(lib().sosrt_set_phase_sets(self._h, _ptr(Pa), int(Pr.shape[0]), _ptr(Pr)))
        self._P = (Pa.copy(), Pr.copy())

    def set_phase_sets_device(self, P_atm, d_P_aer: int, S: int):
        """`set_phase_sets` with the S aerosol matrices in device memory (address of [S, 2N, 2N] float64, e.g. filled by
        `phase_matrix_device`): folded and measured by kernels in the handle's stream order, no trip through the host."""
        Pa = _f64(P_atm, (self.D, self.D), "P_atm")
        check(lib().sosrt_set_phase_sets_dev(self._h, _ptr(Pa), int(S), ctypes.c_void_p(d_P_aer) if d_P_aer else None))
        self._P = (None, None)          # (what the device buffer held is not known here: the next same_phase says no)

    def set_aerosol_sets(self, sets):
        """Aerosol set per column (`sets` [B], after `set_columns`) or per zone of the zone table (`sets` [B, nzmax] with the
        nzmax of `set_columns_zones`; entries of clear zones are ignored).  With a [B, nzmax] table, P0_aer of `first_order`
        and `solve` is [B, nzmax, 2N]: aerosol zone z of column b reads row (b, z).  `set_columns*` puts every column back
        on set 0."""
        z = np.ascontiguousarray(sets, dtype=np.int32)
        if z.ndim == 1:
            z = z.reshape(-1, 1)
        if z.ndim != 2 or z.shape[0] != self.B:
            raise ValueError("sets has shape %s, expected (%d,) or (%d, nzmax)" % (np.shape(sets), self.B, self.B))
        check(lib().sosrt_set_aerosol_sets(self._h, int(z.shape[0]), int(z.shape[1]), _ptr(z)))
        self._p0_zones = int(z.shape[1]) if z.shape[1] > 1 else 0

    def phase_sets_info(self):
        """{'sets': phase sets on the handle, 'groups': combined-matrix groups of the current columns (0: none, or two
        passes), 'single_pass': whether their slab rows take the single pass, 'group_cap': groups the cache holds with sets
        in use}"""
        out = (ctypes.c_int * 4)()
        check(lib().sosrt_phase_sets_info(self._h, out))
        return {"sets": out[0], "groups": out[1], "single_pass": bool(out[2]), "group_cap": out[3]}

    def set_atm_phase_sets(self, P_atm_sets):
        """Several ATMOSPHERE phase matrices `P_atm_sets` [S_atm, 2N, 2N], after `set_phase*` (set 0 replaces its P_atm);
        `set_atmosphere_sets` says which one a column reads -- set 0 until then.  Every set must be low-rank (rank <= 4) and
        flip-symmetric like the P_atm of `set_phase`; otherwise ValueError and the handle is unchanged (sosrt.h)."""
        Pa = np.ascontiguousarray(P_atm_sets, dtype=np.float64)
        if Pa.ndim != 3 or Pa.shape[1:] != (self.D, self.D):
            raise ValueError("P_atm_sets has shape %s, expected (S_atm, %d, %d)" % (Pa.shape, self.D, self.D))
        check(lib().sosrt_set_atm_phase_sets(self._h, int(Pa.shape[0]), _ptr(Pa)))
        self._P = (None, None)          # (set 0 replaced P_atm: the next same_phase says no)

    def set_atmosphere_sets(self, sets):
        """Atmosphere set per column (`sets` [B], after `set_columns*`, which puts every column back on set 0)."""
        z = np.ascontiguousarray(sets, dtype=np.int32)
        if z.shape != (self.B,):
            raise ValueError("sets has shape %s, expected (%d,)" % (np.shape(sets), self.B))
        check(lib().sosrt_set_atmosphere_sets(self._h, int(self.B), _ptr(z)))

    def atm_sets_info(self):
        """{'sets': atmosphere sets on the handle, 'in_use': whether a current column is off atmosphere set 0}"""
        out = (ctypes.c_int * 2)()
        check(lib().sosrt_atm_sets_info(self._h, out))
        return {"sets": out[0], "in_use": bool(out[1])}

    def same_grid(self, mu):
        return self.mu is not None and np.array_equal(self.mu, np.asarray(mu, dtype=np.float64))

    def same_phase(self, P_atm, P_aer=None):
        a, r = self._P
        if a is None or not np.array_equal(a, P_atm):
            return False
        if (r is None) != (P_aer is None):
            return False
        # (a stack of sets [S, 2N, 2N] is a different state from one matrix [2N, 2N], also for S = 1: shapes must agree)
        return r is None or (np.shape(r) == np.shape(P_aer) and np.array_equal(r, P_aer))

    def set_columns(self, idx_up, idx_down, mu0, grd_alb, alb_atm, alb_aer, dtau_atm, dtau_aer, tauStar_tot,
                    surface="specular"):
        """Three-zone columns (spec:23-53).  Scalars broadcast over the batch."""
        B = int(np.size(idx_up))
        sf = _surface_code(surface)
        iu = _i32(np.reshape(idx_up, (B,)), B, "idx_up")
        idn = _i32(np.reshape(idx_down, (B,)), B, "idx_down")
        v = [_vec(x, B, n) for x, n in ((mu0, "mu0"), (grd_alb, "grd_alb"), (alb_atm, "alb_atm"), (alb_aer, "alb_aer"),
                                        (dtau_atm, "dtau_atm"), (dtau_aer, "dtau_aer"), (tauStar_tot, "tauStar_tot"))]
        check(lib().sosrt_set_columns(self._h, B, _lib.GEOM_THREE_ZONE, sf, _ptr(iu), _ptr(idn), *[_ptr(x) for x in v]))
        self.B = B
        self._p0_zones = 0
        self.single_slab = False

    def set_columns_zones(self, zone_r0, zone_mix, mu0, grd_alb, alb_atm, dtau_atm, zone_alb_aer, zone_dtau_aer, tauStar_tot,
                          nz=None, surface="specular"):
        """Columns described by a zone table: `zone_r0`, `zone_mix` [B, nzmax] (first row of each zone, 1 for an
        aerosol zone), `zone_alb_aer`, `zone_dtau_aer` [B, nzmax] (per aerosol zone), `nz` [B] zones per column (default:
        all nzmax).  (clear, slab, clear) is `set_columns`."""
        zr0 = np.ascontiguousarray(np.atleast_2d(zone_r0), dtype=np.int32)
        B, nzmax = zr0.shape
        zmix = np.ascontiguousarray(np.broadcast_to(np.asarray(zone_mix, dtype=np.int32), (B, nzmax)))
        zwr = np.ascontiguousarray(np.broadcast_to(np.asarray(zone_alb_aer, dtype=np.float64), (B, nzmax)))
        zdt = np.ascontiguousarray(np.broadcast_to(np.asarray(zone_dtau_aer, dtype=np.float64), (B, nzmax)))
        nzv = np.full(B, nzmax, dtype=np.int32) if nz is None else _i32(np.reshape(nz, (B,)), B, "nz")
        sf = _surface_code(surface)
        v = [_vec(x, B, n) for x, n in ((mu0, "mu0"), (grd_alb, "grd_alb"), (alb_atm, "alb_atm"), (dtau_atm, "dtau_atm"),
                                        (tauStar_tot, "tauStar_tot"))]
        check(lib().sosrt_set_columns_zones(self._h, B, sf, nzmax, _ptr(nzv), _ptr(zr0), _ptr(zmix), _ptr(v[0]), _ptr(v[1]),
                                            _ptr(v[2]), _ptr(v[3]), _ptr(zwr), _ptr(zdt), _ptr(v[4])))
        self.B = B
        self._p0_zones = 0
        self.single_slab = False

    def set_columns_single_slab(self, mu0, alb, tauStar):
        """Single homogeneous slab over a black surface (I1_In:13-130)."""
        B = int(np.size(mu0))
        m, a, t = _vec(mu0, B, "mu0"), _vec(alb, B, "alb"), _vec(tauStar, B, "tauStar")
        check(lib().sosrt_set_columns(self._h, B, _lib.GEOM_SINGLE_SLAB, _lib.SURFACE_NONE, None, None, _ptr(m), None,
                                      _ptr(a), None, None, None, _ptr(t)))
        self.B = B
        self._p0_zones = 0
        self.single_slab = True

    def _p0_shape(self):
        return (self.B, self._p0_zones, self.D) if self._p0_zones else (self.B, self.D)

    # ---- step level ----------------------------------------------------------
    def first_order(self, tau, P0_atm, P0_aer=None):
        B = self.B
        tau = _f64(tau, (B, self.L), "tau")
        Pa = _f64(P0_atm, (B, self.D), "P0_atm")
        Pr = None if P0_aer is None else _f64(P0_aer, self._p0_shape(), "P0_aer")
        out = np.empty((B, self.L, self.D))
        check(lib().sosrt_first_order(self._h, B, _ptr(tau), _ptr(Pa), _ptr(Pr), _ptr(out)))
        return out

    def source(self, In_1):
        B = self.B
        x = _f64(In_1, (B, self.L, self.D), "In_1")
        out = np.empty_like(x)
        check(lib().sosrt_source(self._h, B, _ptr(x), _ptr(out)))
        return out

    def transport(self, tau, Jn):
        B = self.B
        tau = _f64(tau, (B, self.L), "tau")
        J = _f64(Jn, (B, self.L, self.D), "Jn")
        out = np.empty_like(J)
        st = np.zeros(B, dtype=np.int32)
        check(lib().sosrt_transport(self._h, B, _ptr(tau), _ptr(J), _ptr(out), _ptr(st)))
        return out, st

    # ---- column level --------------------------------------------------------
    def solve(self, tau, P0_atm=None, P0_aer=None, tol=1e-4, I1=None, save_orders=False, fetch_field=True) -> SolveResult:
        """fetch_field=False leaves the radiance field on the device (SolveResult.I is None) for `epilogue`."""
        B = self.B
        tau = _f64(tau, (B, self.L), "tau")
        Pa = None if P0_atm is None else _f64(P0_atm, (B, self.D), "P0_atm")
        Pr = None if P0_aer is None else _f64(P0_aer, self._p0_shape(), "P0_aer")
        I1a = None if I1 is None else _f64(I1, (B, self.L, self.D), "I1")
        I = np.empty((B, self.L, self.D)) if fetch_field else None
        n = np.zeros(B, dtype=np.int32)
        st = np.zeros(B, dtype=np.int32)
        sv = None
        if save_orders:
            # The per-order history has n entries (spec:304-305,458), n known only afterwards: a first pass without
            # it (the field stays on the device) gives n, the second stores exactly max(n) orders per column --
            # not max_orders of them (1.6 GB per column at the reference's shipped size with a 256-order budget).
            check(lib().sosrt_solve(self._h, B, _ptr(tau), _ptr(Pa), _ptr(Pr), float(tol), _ptr(I1a), None, None, _ptr(n), _ptr(st)))
            slots = int(max(1, n.max()))
            check(lib().sosrt_set_saved_orders(self._h, slots))
            sv = np.zeros((B, slots, self.L, self.D))
        try:
            check(lib().sosrt_solve(self._h, B, _ptr(tau), _ptr(Pa), _ptr(Pr), float(tol), _ptr(I1a), _ptr(I), _ptr(sv),
                                    _ptr(n), _ptr(st)))
        finally:
            if save_orders:
                check(lib().sosrt_set_saved_orders(self._h, self.max_orders))
        return SolveResult(I=I, n=n, status=st, I_saved=sv)

    def solve_device(self, d_tau: int, d_P0_atm: int, d_P0_aer: int, d_I_out: int, tol=1e-4, d_I1: int = 0,
                     d_I_saved: int = 0, d_n_orders: int = 0, d_status: int = 0):
        """All arguments are device addresses (e.g. torch `tensor.data_ptr()`); work is enqueued on
        the handle's stream (set_stream) and is complete after synchronize()."""
        check(lib().sosrt_solve_dev(self._h, self.B, _vp(d_tau), _vp(d_P0_atm), _vp(d_P0_aer), float(tol), _vp(d_I1),
                                    _vp(d_I_out), _vp(d_I_saved), _vp(d_n_orders), _vp(d_status)))

    def last_solve_stats(self):
        mo = ctypes.c_int()
        so = ctypes.c_longlong()
        check(lib().sosrt_last_solve_stats(self._h, ctypes.byref(mo), ctypes.byref(so)))
        return mo.value, so.value

    def fluxes(self, tau, I, beam_norm="crit"):
        B = self.B
        tau = _f64(tau, (B, self.L), "tau")
        I = _f64(I, (B, self.L, self.D), "I")
        fd = np.empty((B, self.L))
        fu = np.empty((B, self.L))
        check(lib().sosrt_fluxes(self._h, B, _ptr(tau), _ptr(I), 0 if beam_norm == "crit" else 1, _ptr(fd), _ptr(fu)))
        return fd, fu

    def epilogue(self, z_profile=None, beam_norm="crit", want=("flux_down", "flux_up", "diffusivity", "heating_rate", "net_toa")):
        """Fluxes, diffusivity, heating rate and TOA net flux of the field the last `solve` left on the device
        (graphe:10,74-91,157-158, crit:377-382); only these [B, L] / [B] arrays cross PCIe."""
        B = self.B
        want = set(want)
        if z_profile is None:
            want.discard("heating_rate")
        z = None if z_profile is None else _f64(z_profile, (self.L,), "z_profile")
        arr = {k: (np.empty(B) if k == "net_toa" else np.empty((B, self.L))) if k in want else None
               for k in ("flux_down", "flux_up", "diffusivity", "heating_rate", "net_toa")}
        check(lib().sosrt_epilogue(self._h, B, 0 if beam_norm == "crit" else 1, _ptr(z), _ptr(arr["flux_down"]),
                                   _ptr(arr["flux_up"]), _ptr(arr["diffusivity"]), _ptr(arr["heating_rate"]),
                                   _ptr(arr["net_toa"])))
        return {k: v for k, v in arr.items() if v is not None}

    def epilogue_device(self, d_tau: int, d_I: int, d_z: int = 0, beam_norm="crit", d_flux_down: int = 0, d_flux_up: int = 0,
                        d_diffusivity: int = 0, d_heating_rate: int = 0, d_net_toa: int = 0):
        """Same on caller-owned device buffers (addresses), enqueued on the handle's stream."""
        check(lib().sosrt_epilogue_dev(self._h, self.B, _vp(d_tau), _vp(d_I), 0 if beam_norm == "crit" else 1, _vp(d_z),
                                       _vp(d_flux_down), _vp(d_flux_up), _vp(d_diffusivity), _vp(d_heating_rate), _vp(d_net_toa)))

    # ---- pseudo-spherical direct beam (sosrt.h) --------------------------------
    def set_saved_orders(self, slots: Optional[int] = None):
        """Orders per column that the solves that follow store in their per-order output (None: the handle's max_orders)."""
        check(lib().sosrt_set_saved_orders(self._h, int(self.max_orders if slots is None else slots)))

    def beam_slant_device(self, d_tau: int, d_z: int, d_sigma_out: int, earth_radius=6371.0, d_mu0: int = 0, B: Optional[int] = None):
        """Slant optical depth of the direct beam through spherical shells: d_tau [B, L], d_z [L] (km, strictly descending),
        d_sigma_out [B, L] (device addresses); d_mu0 [B] or 0 for the columns' own mu0.  Enqueued on the handle's stream (the
        call reads d_z back to check it)."""
        check(lib().sosrt_beam_slant_dev(self._h, int(self.B if B is None else B), _vp(d_tau), _vp(d_z), float(earth_radius),
                                         _vp(d_mu0), _vp(d_sigma_out)))

    def first_order_beam_device(self, d_tau: int, d_sigma: int, d_P0_atm: int, d_P0_aer: int, d_I1_out: int, B: Optional[int] = None):
        """The first order layer by layer on the beam path d_sigma [B, L] (sigma = tau / mu0: the coded first order, to
        rounding): d_I1_out [B, L, 2N] is the `d_I1` of `solve_device`.  P0 layouts as `solve_device` takes them."""
        check(lib().sosrt_first_order_beam_dev(self._h, int(self.B if B is None else B), _vp(d_tau), _vp(d_sigma), _vp(d_P0_atm),
                                               _vp(d_P0_aer), _vp(d_I1_out)))

    def epilogue_beam_device(self, d_tau: int, d_I: int, d_sigma: int, d_z: int = 0, beam_norm="crit", d_flux_down: int = 0,
                             d_flux_up: int = 0, d_diffusivity: int = 0, d_heating_rate: int = 0, d_net_toa: int = 0,
                             B: Optional[int] = None):
        """`epilogue_device` with the beam terms of the fluxes on the path d_sigma [B, L]."""
        check(lib().sosrt_epilogue_beam_dev(self._h, int(self.B if B is None else B), _vp(d_tau), _vp(d_I),
                                            0 if beam_norm == "crit" else 1, _vp(d_z), _vp(d_flux_down), _vp(d_flux_up),
                                            _vp(d_diffusivity), _vp(d_heating_rate), _vp(d_net_toa), _vp(d_sigma)))

    def view_first_order_beam_device(self, mu_view, d_tau: int, d_sigma: int, d_p0rows_atm: int, d_p0rows_aer: int, levels,
                                     d_first_out: int, nset: int = 1, B: Optional[int] = None):
        """`first_order_beam_device` at the view cosines `mu_view` [V] (host, each in [0.01, 1], V <= 64) and the rows `levels`
        (DESIGN section 27): d_first_out [nset, B, nlev, 2V] on the signed lanes (-mu_view, +mu_view) from the p0 rows
        d_p0rows_atm, d_p0rows_aer [nset, B, 2V] (the azimuths of an exact first order, or one set); the geometry of a lane is
        evaluated once for all sets.  Specular or no surface."""
        m = np.ascontiguousarray(np.atleast_1d(mu_view), dtype=np.float64)
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.int32)
        check(lib().sosrt_view_first_order_beam_dev(self._h, int(self.B if B is None else B), int(m.size),
                                                    _ptr(m) if m.size else None, _vp(d_tau), _vp(d_sigma), int(nset),
                                                    _vp(d_p0rows_atm), _vp(d_p0rows_aer), int(lev.size),
                                                    _ptr(lev) if lev.size else None, _vp(d_first_out)))

    # ---- thermal emission (sosrt.h) ----------------------------------------------
    def emission_device(self, d_tau: int, d_planck: int, d_planck_surface: int, d_I0_out: int, d_emissivity: int = 0,
                        B: Optional[int] = None):
        """The field the layers and the ground emit: d_tau, d_planck [B, L] (the Planck radiance at every level),
        d_planck_surface [B], d_emissivity [B] or 0 for 1 - grd_alb; d_I0_out [B, L, 2N] is the `d_I1` of `solve_device`.
        Device addresses; enqueued on the handle's stream; nothing but the output is written."""
        check(lib().sosrt_emission_dev(self._h, int(self.B if B is None else B), _vp(d_tau), _vp(d_planck), _vp(d_planck_surface),
                                       _vp(d_emissivity), _vp(d_I0_out)))

    def emission_view_device(self, mu_view, d_tau: int, d_planck: int, d_planck_surface: int, levels, d_out: int,
                             d_emissivity: int = 0, B: Optional[int] = None):
        """`emission_device` at the view cosines `mu_view` [V] (host, each in [0.01, 1], V <= 64) and the rows `levels`:
        d_out [B, nlev, 2V] on the signed lanes (-mu_view, +mu_view).  Specular or no surface."""
        m = np.ascontiguousarray(np.atleast_1d(mu_view), dtype=np.float64)
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.int32)
        check(lib().sosrt_emission_view_dev(self._h, int(self.B if B is None else B), int(m.size), _ptr(m) if m.size else None,
                                            _vp(d_tau), _vp(d_planck), _vp(d_planck_surface), _vp(d_emissivity), int(lev.size),
                                            _ptr(lev) if lev.size else None, _vp(d_out)))

    def epilogue_emission_device(self, d_tau: int, d_I: int, d_z: int = 0, d_flux_down: int = 0, d_flux_up: int = 0,
                                 d_diffusivity: int = 0, d_heating_rate: int = 0, d_net_toa: int = 0, B: Optional[int] = None):
        """`epilogue_device` without the two beam terms: the fluxes, diffusivity, heating rate and TOA net flux of a thermal field."""
        check(lib().sosrt_epilogue_emission_dev(self._h, int(self.B if B is None else B), _vp(d_tau), _vp(d_I), _vp(d_z),
                                                _vp(d_flux_down), _vp(d_flux_up), _vp(d_diffusivity), _vp(d_heating_rate),
                                                _vp(d_net_toa)))

    # ---- gas absorption profiles: per-level weights (sosrt.h) ------------------------
    def set_row_weights_device(self, d_w_atm: int = 0, d_w_aer: int = 0, B: Optional[int] = None):
        """Per-level weights on the two row coefficients of the source function: d_w_atm, d_w_aer [B, L] (device addresses,
        copied in stream order; finite and >= 0).  One 0 stands for ones, both 0 clear the weights; `set_columns*` clears them
        too.  While set, the first order is `first_order_profile_device`, the emission `emission_profile_device`, and the
        entries that evaluate one constant per zone raise SosrtError."""
        check(lib().sosrt_set_row_weights_dev(self._h, int(self.B if B is None else B), _vp(d_w_atm), _vp(d_w_aer)))

    def first_order_profile_device(self, d_tau: int, d_sigma: int, d_P0_atm: int, d_P0_aer: int, d_I1_out: int,
                                   B: Optional[int] = None):
        """`first_order_beam_device` with the handle's weights in the scattering coefficient of every row."""
        check(lib().sosrt_first_order_profile_dev(self._h, int(self.B if B is None else B), _vp(d_tau), _vp(d_sigma),
                                                  _vp(d_P0_atm), _vp(d_P0_aer), _vp(d_I1_out)))

    def emission_profile_device(self, d_tau: int, d_planck: int, d_planck_surface: int, d_I0_out: int, d_emissivity: int = 0,
                                B: Optional[int] = None):
        """`emission_device` with the handle's weights in the emission coefficient of every row."""
        check(lib().sosrt_emission_profile_dev(self._h, int(self.B if B is None else B), _vp(d_tau), _vp(d_planck),
                                               _vp(d_planck_surface), _vp(d_emissivity), _vp(d_I0_out)))

    # ---- gas absorption at view angles: the weights in the view stage (sosrt.h) --------
    def view_radiance_profile_device(self, mu_view, d_tau: int, d_I_src: int, d_rows_atm: int, d_rows_aer: int, levels,
                                     d_scat_out: int, quadrature="grid", B: Optional[int] = None):
        """The scattered term of `view_radiance_device` with the handle's weights on the stage's row coefficients:
        d_scat_out [B, nlev, 2V].  It has no first-order arguments: under weights the first term is
        `view_first_order_profile_device` or `emission_view_profile_device`.  Needs weights to be set."""
        m = np.ascontiguousarray(np.atleast_1d(mu_view), dtype=np.float64)
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.int32)
        q = self._QUADS.get(quadrature, quadrature)
        if isinstance(q, str) or isinstance(q, bool) or not isinstance(q, (int, np.integer)):
            raise ValueError("quadrature must be 'grid' or 'linear' (got %r)" % (quadrature,))
        check(lib().sosrt_view_radiance_profile_dev(self._h, int(self.B if B is None else B), int(m.size),
                                                    _ptr(m) if m.size else None, _vp(d_tau), _vp(d_I_src), _vp(d_rows_atm),
                                                    _vp(d_rows_aer), int(q), int(lev.size), _ptr(lev) if lev.size else None,
                                                    _vp(d_scat_out)))

    def view_first_order_profile_device(self, mu_view, d_tau: int, d_sigma: int, d_p0rows_atm: int, d_p0rows_aer: int, levels,
                                        d_first_out: int, nset: int = 1, B: Optional[int] = None):
        """`view_first_order_beam_device` with the handle's weights in the scattering coefficient of every row (d_sigma =
        tau / mu0 is the plane beam, `beam_slant_device` on the total tau the sphere): d_first_out [nset, B, nlev, 2V]."""
        m = np.ascontiguousarray(np.atleast_1d(mu_view), dtype=np.float64)
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.int32)
        check(lib().sosrt_view_first_order_profile_dev(self._h, int(self.B if B is None else B), int(m.size),
                                                       _ptr(m) if m.size else None, _vp(d_tau), _vp(d_sigma), int(nset),
                                                       _vp(d_p0rows_atm), _vp(d_p0rows_aer), int(lev.size),
                                                       _ptr(lev) if lev.size else None, _vp(d_first_out)))

    def emission_view_profile_device(self, mu_view, d_tau: int, d_planck: int, d_planck_surface: int, levels, d_out: int,
                                     d_emissivity: int = 0, B: Optional[int] = None):
        """`emission_view_device` with the handle's weights in the emission coefficient of every row: d_out [B, nlev, 2V]."""
        m = np.ascontiguousarray(np.atleast_1d(mu_view), dtype=np.float64)
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.int32)
        check(lib().sosrt_emission_view_profile_dev(self._h, int(self.B if B is None else B), int(m.size),
                                                    _ptr(m) if m.size else None, _vp(d_tau), _vp(d_planck), _vp(d_planck_surface),
                                                    _vp(d_emissivity), int(lev.size), _ptr(lev) if lev.size else None, _vp(d_out)))

    # ---- band integration (sosrt.h) --------------------------------------------------
    def planck_bands_device(self, d_T: int, d_T_surface: int, nu_lo, nu_hi, d_planck_out: int, d_planck_surface_out: int,
                            d_scale_out: int = 0, C: int = 1, normalise=True):
        """Planck band radiances (W m-2 sr-1) of the K bands [nu_lo, nu_hi] (host, cm^-1) at the levels and the ground of C
        columns: d_T [C, L] and d_T_surface [C] in kelvin; d_planck_out [K, C, L], d_planck_surface_out [K, C], d_scale_out
        [K, C].  normalise: every (k, c) divided by its maximum, which goes to d_scale_out (0 is allowed without it).  Device
        addresses; enqueued on the handle's stream; nothing but the outputs is written."""
        lo = np.ascontiguousarray(np.atleast_1d(nu_lo), dtype=np.float64)
        hi = np.ascontiguousarray(np.atleast_1d(nu_hi), dtype=np.float64)
        if lo.ndim != 1 or lo.shape != hi.shape:
            raise ValueError("nu_lo and nu_hi must be two arrays [K] of one length")
        check(lib().sosrt_planck_bands_dev(self._h, int(C), int(lo.size), _vp(d_T), _vp(d_T_surface), _ptr(lo) if lo.size else None,
                                           _ptr(hi) if hi.size else None, int(bool(normalise)), _vp(d_planck_out),
                                           _vp(d_planck_surface_out), _vp(d_scale_out)))

    def band_reduce_device(self, d_x: int, d_out: int, C: int, K: int, M: int, d_weight: int = 0, d_scale: int = 0,
                           accumulate=False):
        """d_out [C, M] = (accumulate ? d_out : 0) + sum over k ascending of (weight[k, c] scale[k, c]) d_x[k, c, m], one fused
        multiply-add per k; d_weight, d_scale [K, C] or 0 for ones.  The same bits however K is split over accumulating calls."""
        check(lib().sosrt_band_reduce_dev(self._h, int(C), int(K), int(M), _vp(d_weight), _vp(d_scale), _vp(d_x), _vp(d_out),
                                          int(bool(accumulate))))

    def brightness_temperature_device(self, d_radiance: int, d_T_out: int, nu_lo, nu_hi, C: int, M: int, d_weight: int = 0):
        """The brightness temperature of a band-summed radiance: d_T_out [C, M] (kelvin) is the temperature
        at which sum_k weight[k, c] B_k(T) equals d_radiance [C, M] (W m-2 sr-1), B_k the band radiance of `planck_bands_device`
        over [nu_lo[k], nu_hi[k]] (host, cm^-1, K <= 64); d_weight [K, C] or 0 for ones.  NaN where there is no such
        temperature in (1 K, 1e5 K): a radiance that is not finite or <= 0, weights of a column that are all zero or hold a
        negative one.  Device addresses; enqueued on the handle's stream; nothing but the output is written."""
        lo = np.ascontiguousarray(np.atleast_1d(nu_lo), dtype=np.float64)
        hi = np.ascontiguousarray(np.atleast_1d(nu_hi), dtype=np.float64)
        if lo.ndim != 1 or lo.shape != hi.shape:
            raise ValueError("nu_lo and nu_hi must be two arrays [K] of one length")
        check(lib().sosrt_brightness_temperature_dev(self._h, int(C), int(lo.size), int(M), _ptr(lo) if lo.size else None,
                                                     _ptr(hi) if hi.size else None, _vp(d_weight), _vp(d_radiance), _vp(d_T_out)))

    # ---- BRDF ground (sosrt.h) --------------------------------------------------------
    _BRDF_KINDS = {"lambertian": _lib.BRDF_LAMBERTIAN, "rpv": _lib.BRDF_RPV, "ross_thick": _lib.BRDF_ROSS_THICK,
                   "li_sparse_r": _lib.BRDF_LI_SPARSE_R, "cox_munk": _lib.BRDF_COX_MUNK}

    def _brdf_pack(self, kind, params):
        """(kind, params, nparams) as the C entry points take a named BRDF"""
        k = self._BRDF_KINDS.get(kind)
        if k is None:
            raise ValueError("BRDF kind must be 'lambertian', 'rpv', 'ross_thick', 'li_sparse_r' or 'cox_munk' (got %r)" % (kind,))
        p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64))) if np.size(params) else np.zeros(0)
        return k, _ptr(p) if p.size else None, int(p.size)

    @staticmethod
    def _view_pack(mu_view):
        """(V, mu_view) as the C entry points take view cosines"""
        m = np.ascontiguousarray(np.atleast_1d(mu_view), dtype=np.float64)
        return int(m.size), _ptr(m)

    def brdf_operator_device(self, kind, d_R_out: int, params=(), nphi=65):
        """The reflection operator of a named BRDF ('lambertian', or 'rpv' with params (rho0, k, Theta)), its azimuth mean on
        `nphi` trapezoid nodes and the flux quadrature folded in: d_R_out [N-1, N-1] with element (j, i) = 2 w_j |mu_j|
        rho_bar(mu[N+1+i], |mu_j|), the upward lanes i of one downward lane j contiguous.  Enqueued on the handle's stream."""
        check(lib().sosrt_brdf_operator_dev(self._h, *self._brdf_pack(kind, params), int(nphi), _vp(d_R_out)))

    def brdf_beam_device(self, kind, d_mu0: int, d_r0_out: int, params=(), nphi=65, B: Optional[int] = None):
        """The reflection of the direct beam: d_r0_out [B, N-1] = rho_bar(mu[N+1+i], d_mu0[b])."""
        check(lib().sosrt_brdf_beam_dev(self._h, int(self.B if B is None else B), *self._brdf_pack(kind, params), int(nphi),
                                        _vp(d_mu0), _vp(d_r0_out)))

    def brdf_operator_modes_device(self, kind, d_R_out: int, m_first, m_count, params=(), nphi=65, sign_odd=False):
        """The Fourier modes m_first .. m_first + m_count - 1 in azimuth of `brdf_operator_device`: d_R_out
        [m_count, N-1, N-1] with rho^m = (1 / pi) int rho cos(m phi) dphi in place of the azimuth mean; sign_odd: mode m as
        (-1)^m R^m, what `ground_source_device` takes for mode m.  Mode 0 has the bits of `brdf_operator_device`."""
        check(lib().sosrt_brdf_operator_modes_dev(self._h, *self._brdf_pack(kind, params), int(nphi), int(m_first), int(m_count),
                                                  int(bool(sign_odd)), _vp(d_R_out)))

    def brdf_beam_modes_device(self, kind, d_mu0: int, d_r0_out: int, m_first, m_count, params=(), nphi=65, B: Optional[int] = None):
        """The same modes of `brdf_beam_device`: d_r0_out [m_count, B, N-1] = rho^m(mu[N+1+i], d_mu0[b]) (no sign)."""
        check(lib().sosrt_brdf_beam_modes_dev(self._h, int(self.B if B is None else B), *self._brdf_pack(kind, params), int(nphi),
                                              int(m_first), int(m_count), _vp(d_mu0), _vp(d_r0_out)))

    def ground_source_device(self, d_I: int, d_tau: int, d_R: int, d_S_out: int, d_r0: int = 0, d_scale: int = 0,
                             B: Optional[int] = None):
        """d_S_out [B, N-1] = scale[b] (R I[b, L-1, 0 .. N-2] + r0[b] exp(-tau[b, L-1] / mu0[b])) with the columns' mu0; d_r0 0:
        no beam term; d_scale 0: 1.  d_R as `brdf_operator_device` writes it."""
        check(lib().sosrt_ground_source_dev(self._h, int(self.B if B is None else B), _vp(d_I), _vp(d_tau), _vp(d_R), _vp(d_r0),
                                            _vp(d_scale), _vp(d_S_out)))

    def ground_source_terms_device(self, K: int, d_I: int, d_tau: int, d_R: int, d_weight: int, d_S_out: int, d_r0: int = 0,
                                   B: Optional[int] = None):
        """`ground_source_device` over K operator terms with per-column weights (the Ross-Li ground): d_S_out
        [B, N-1] = sum_k weight[b, k] (R[k] I[b, L-1, 0 .. N-2] + r0[k, b] exp(-tau[b, L-1] / mu0[b])), k ascending in fused
        multiply-adds from +0.  d_R [K, N-1, N-1], d_r0 [K, B, N-1] (0: no beam term), d_weight [B, K].  With K = 1 the bits of
        `ground_source_device` with scale = weight; a term of weight 0 leaves the bits alone."""
        check(lib().sosrt_ground_source_terms_dev(self._h, int(self.B if B is None else B), int(K), _vp(d_I), _vp(d_tau), _vp(d_R),
                                                  _vp(d_r0), _vp(d_weight), _vp(d_S_out)))

    def ground_first_order_device(self, d_tau: int, d_S: int, d_G_out: int, d_status: int = 0, B: Optional[int] = None):
        """The unscattered upward field of the ground source d_S [B, N-1], with the mu -> 0+ blend of the order loop on every
        row: d_G_out [B, L, 2N] is the `d_I1` of `solve_device` over a black ground; d_status [B] int32 (COL_INDEXERROR where
        the blend's search leaves the row)."""
        check(lib().sosrt_ground_first_order_dev(self._h, int(self.B if B is None else B), _vp(d_tau), _vp(d_S), _vp(d_G_out),
                                                 _vp(d_status)))

    def bounce_accumulate_device(self, d_Ik: int, d_I_total: int, d_ratio_out: int, B: Optional[int] = None):
        """d_I_total += d_Ik ([B, L, 2N]); d_ratio_out [B]: the larger of max |Ik| / max |total| on the upward lanes of row 0 and
        on the downward lanes of row L-1."""
        check(lib().sosrt_bounce_accumulate_dev(self._h, int(self.B if B is None else B), _vp(d_Ik), _vp(d_I_total), _vp(d_ratio_out)))

    # ---- the BRDF ground's term at view lanes off the grid (sosrt.h) -------------------
    def brdf_view_rows_modes_device(self, kind, mu_view, d_out: int, m_first, m_count, params=(), nphi=65, sign_odd=False):
        """Rows of `brdf_operator_modes_device` at the view cosines `mu_view` [V] (host) in place of the upward nodes: d_out
        [m_count, N-1, V] with element (j, v) = 2 w_j |mu_j| rho^m(mu_view[v], |mu_j|) ((-1)^m with sign_odd).  At a node the
        bits of that builder's column."""
        check(lib().sosrt_brdf_view_rows_modes_dev(self._h, *self._brdf_pack(kind, params), int(nphi), int(m_first), int(m_count),
                                                   int(bool(sign_odd)), *self._view_pack(mu_view), _vp(d_out)))

    def brdf_view_beam_modes_device(self, kind, d_mu0: int, mu_view, d_out: int, m_first, m_count, params=(), nphi=65,
                                    B: Optional[int] = None):
        """The same of `brdf_beam_modes_device`: d_out [m_count, B, V] = rho^m(mu_view[v], d_mu0[b])."""
        check(lib().sosrt_brdf_view_beam_modes_dev(self._h, int(self.B if B is None else B), *self._brdf_pack(kind, params),
                                                   int(nphi), int(m_first), int(m_count), _vp(d_mu0), *self._view_pack(mu_view),
                                                   _vp(d_out)))

    def brdf_view_beam_azimuth_device(self, kind, d_mu0: int, mu_view, d_phi: int, nphi_out: int, d_out: int, params=(),
                                      B: Optional[int] = None):
        """rho(mu_view[v], d_mu0[b], d_phi[q]) at the azimuth itself (phi = 0: the hot spot), no quadrature: d_out [nphi_out, B, V]."""
        check(lib().sosrt_brdf_view_beam_azimuth_dev(self._h, int(self.B if B is None else B), *self._brdf_pack(kind, params),
                                                     _vp(d_mu0), *self._view_pack(mu_view), int(nphi_out), _vp(d_phi), _vp(d_out)))

    def view_ground_device(self, mu_view, d_tau: int, levels, d_out: int, d_I: int = 0, d_Rv: int = 0, d_r0v: int = 0,
                           d_scale: int = 0, accumulate=False, d_S_out: int = 0, B: Optional[int] = None):
        """The ground's unscattered radiance at the view lanes: d_out [B, nlev, 2V], upward lanes (+)= S[b, v] exp(-(tau[b, L-1] -
        tau[b, t]) / mu_view[v]) with S = scale[b] (Rv I[b, L-1, 0 .. N-2] + r0v[b] exp(-tau[b, L-1] / mu0[b])) (d_S_out [B, V],
        optional); downward lanes +0 unless accumulating.  d_I, d_Rv 0: the beam-only call; d_r0v 0: the diffuse-only one."""
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.int32)
        check(lib().sosrt_view_ground_dev(self._h, int(self.B if B is None else B), *self._view_pack(mu_view), _vp(d_tau), _vp(d_I),
                                          _vp(d_Rv), _vp(d_r0v), _vp(d_scale), int(lev.size), _ptr(lev), int(bool(accumulate)),
                                          _vp(d_S_out), _vp(d_out)))

    def view_ground_terms_device(self, K: int, mu_view, d_tau: int, levels, d_weight: int, d_out: int, d_I: int = 0, d_Rv: int = 0,
                                 d_r0v: int = 0, accumulate=False, d_S_out: int = 0, B: Optional[int] = None):
        """`view_ground_device` over K operator terms with per-column weights, as `ground_source_terms_device`: d_Rv [K, N-1, V],
        d_r0v [K, B, V], d_weight [B, K]."""
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.int32)
        check(lib().sosrt_view_ground_terms_dev(self._h, int(self.B if B is None else B), int(K), *self._view_pack(mu_view),
                                                _vp(d_tau), _vp(d_I), _vp(d_Rv), _vp(d_r0v), _vp(d_weight), int(lev.size), _ptr(lev),
                                                int(bool(accumulate)), _vp(d_S_out), _vp(d_out)))

    # ---- phase functions on the device (phase:68-292) ----------------------------
    _KINDS ={"iso": _lib.PHASE_ISO, "rayleigh": _lib.PHASE_RAYLEIGH, "hg": _lib.PHASE_HG, "table": _lib.PHASE_TABLE}

    def set_phase_table(self, tab_mu, tab_p):
        tm = np.ascontiguousarray(tab_mu, dtype=np.float64)
        tp = _f64(tab_p, tm.shape, "tab_p")
        check(lib().sosrt_phase_table(self._h, _ptr(tm), _ptr(tp), int(tm.size)))

    def set_phase_table_dev(self, d_tab_p: int, ntab: int, d_tab_mu: int = 0):
        """The table from DEVICE arrays (addresses), in stream order: `d_tab_p` [ntab] on the uniform abscissa
        linspace(-1, 1, ntab) -- a row of `mie_ensembles_device`'s output -- or on `d_tab_mu` [ntab]."""
        check(lib().sosrt_phase_table_dev(self._h, ctypes.c_void_p(d_tab_mu) if d_tab_mu else None, ctypes.c_void_p(d_tab_p),
                                          int(ntab)))

    # ---- Lorenz-Mie tables on the device (sosrt.h) ----------------
    @staticmethod
    def _mie_args(wl, m, r_m, sig):
        wl, mm, rm, sg = np.broadcast_arrays(*[np.atleast_1d(np.asarray(a)) for a in (wl, m, 1.0 if r_m is None else r_m,
                                                                                     2.0 if sig is None else sig)])
        mm = mm.astype(np.complex128)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        return f(wl), f(mm.real), f(mm.imag), f(rm), f(sg)

    def mie_ensembles(self, wl, m, r_m=None, sig=None, nb_radius=100, r_min=0.01, r_max=10.0, ntab=6001):
        """Phase tables of S log-normal Mie ensembles (arrays broadcast to [S]; `m` = n + ik with k > 0 absorbing, see
        `mie.refractive_index`) -> (p [S, ntab] on linspace(-1, 1, ntab), bulk [S, 3] = single-scattering albedo, asymmetry
        parameter, mean extinction cross-section).  nb_radius = 1: one sphere of radius r_min."""
        a = self._mie_args(wl, m, r_m, sig)
        S = a[0].size
        p, bulk = np.empty((S, max(int(ntab), 0))), np.empty((S, 3))
        check(lib().sosrt_mie_ensembles(self._h, S, *[_ptr(v) for v in a], int(nb_radius), float(r_min), float(r_max), int(ntab),
                                        _ptr(p), _ptr(bulk)))
        return p, bulk

    def mie_ensembles_device(self, d_p_out: int, d_bulk_out: int, wl, m, r_m=None, sig=None, nb_radius=100, r_min=0.01,
                             r_max=10.0, ntab=6001):
        """The same into device buffers (addresses; [S, ntab] and [S, 3] or 0), enqueued on the handle's stream."""
        a = self._mie_args(wl, m, r_m, sig)
        check(lib().sosrt_mie_ensembles_dev(self._h, a[0].size, *[_ptr(v) for v in a], int(nb_radius), float(r_min), float(r_max),
                                            int(ntab), ctypes.c_void_p(d_p_out), ctypes.c_void_p(d_bulk_out) if d_bulk_out else None))

    def mie_efficiencies(self, m, x):
        """(Q_ext, Q_sca, Q_back, g) of K spheres -> [K, 4] (`m`, `x` broadcast; m = n + ik, k > 0 absorbing)."""
        mm, xx = np.broadcast_arrays(np.atleast_1d(np.asarray(m, dtype=np.complex128)), np.atleast_1d(np.asarray(x, dtype=np.float64)))
        mr, mi, xx = (np.ascontiguousarray(v, dtype=np.float64) for v in (mm.real, mm.imag, xx))
        out = np.empty((xx.size, 4))
        check(lib().sosrt_mie_efficiencies(self._h, int(xx.size), _ptr(mr), _ptr(mi), _ptr(xx), _ptr(out)))
        return out

    def mie_timing(self):
        """Milliseconds of the three kernels of the last `mie_ensembles` (coefficients, angles, integration)."""
        ms = (ctypes.c_double * 3)()
        check(lib().sosrt_mie_timing(self._h, ms))
        return tuple(ms)

    def phase_p0(self, kind, mu0, g=0.0):
        """P0(mu, mu0[b]) for an array of mu0 -> [len(mu0), 2N]."""
        m = np.ascontiguousarray(np.atleast_1d(mu0), dtype=np.float64)
        out = np.empty((m.size, self.D))
        step = max(1, self.max_batch)
        for i in range(0, m.size, step):
            mm = np.ascontiguousarray(m[i:i + step])
            oo = np.empty((mm.size, self.D))
            check(lib().sosrt_phase_p0(self._h, int(mm.size), self._KINDS[kind], float(g), _ptr(mm), _ptr(oo)))
            out[i:i + step] = oo
        return out

    def phase_p0_device(self, kind, d_mu0: int, d_P0_out: int, B: int, g=0.0):
        check(lib().sosrt_phase_p0_dev(self._h, int(B), self._KINDS[kind], float(g), ctypes.c_void_p(d_mu0), ctypes.c_void_p(d_P0_out)))

    def phase_matrix(self, kind, g=0.0):
        out = np.empty((self.D, self.D))
        check(lib().sosrt_phase_matrix(self._h, self._KINDS[kind], float(g), _ptr(out)))
        return out

    def phase_matrix_device(self, kind, d_P_out: int, g=0.0):
        """`phase_matrix` left on the device: d_P_out is the address of [2N, 2N] float64; enqueued on the handle's stream."""
        check(lib().sosrt_phase_matrix_dev(self._h, self._KINDS[kind], float(g), ctypes.c_void_p(d_P_out) if d_P_out else None))

    # ---- delta-M scaling (sosrt.h) ----
    def phase_moments(self, tab_p, lmax, tab_mu=None):
        """Legendre moments of the piecewise-linear interpolant of S tables `tab_p` [S, ntab] (or [ntab]) on `tab_mu` [ntab]
        (None: linspace(-1, 1, ntab)) -> (chi [S, lmax + 1] with chi[:, 0] = 1, norm [S] = half the integral of the table); a
        single table gives (chi [lmax + 1], norm)."""
        p = np.ascontiguousarray(tab_p, dtype=np.float64)
        one = p.ndim == 1
        p = np.atleast_2d(p)
        tm = None if tab_mu is None else _f64(tab_mu, (p.shape[1],), "tab_mu")
        chi, norm = np.empty((p.shape[0], max(int(lmax), 0) + 1)), np.empty(p.shape[0])
        check(lib().sosrt_phase_moments(self._h, int(p.shape[0]), _ptr(tm), _ptr(p), int(p.shape[1]), int(lmax), _ptr(chi), _ptr(norm)))
        return (chi[0], float(norm[0])) if one else (chi, norm)

    def phase_moments_device(self, d_tab_p: int, S: int, ntab: int, lmax: int, d_chi_out: int, d_norm_out: int = 0, d_tab_mu: int = 0):
        """The same on device addresses, enqueued on the handle's stream: d_tab_p [S, ntab], d_chi_out [S, lmax + 1], d_norm_out
        [S] or 0, d_tab_mu [ntab] or 0 for the uniform abscissa."""
        check(lib().sosrt_phase_moments_dev(self._h, int(S), _vp(d_tab_mu), _vp(d_tab_p), int(ntab), int(lmax), _vp(d_chi_out),
                                            _vp(d_norm_out)))

    def delta_m_table(self, chi, order, ntab=None, tab_mu=None):
        """The delta-M table of the moments `chi` [S, lmax + 1] (or [lmax + 1]) truncated at `order`: (table [S, ntab] = sum over
        l < order of (2l + 1) (chi_l - f) / (1 - f) P_l on `tab_mu` (None: linspace(-1, 1, ntab)), f [S] = chi[:, order]); a
        single set of moments gives (table [ntab], f)."""
        c = np.ascontiguousarray(chi, dtype=np.float64)
        one = c.ndim == 1
        c = np.atleast_2d(c)
        tm = None if tab_mu is None else np.ascontiguousarray(tab_mu, dtype=np.float64)
        n = int(ntab) if tm is None else int(tm.size)
        out, f = np.empty((c.shape[0], max(n, 0))), np.empty(c.shape[0])
        check(lib().sosrt_phase_delta_m(self._h, int(c.shape[0]), _ptr(c), int(c.shape[1]) - 1, int(order), _ptr(tm), n, _ptr(out),
                                        _ptr(f)))
        return (out[0], float(f[0])) if one else (out, f)

    def delta_m_table_device(self, d_chi: int, S: int, lmax: int, order: int, ntab: int, d_tab_out: int, d_f_out: int = 0,
                             d_tab_mu: int = 0):
        """The same on device addresses: d_chi [S, lmax + 1], d_tab_out [S, ntab], d_f_out [S] or 0.  Waits for the moments (the
        refusals are made on the host), then enqueues on the handle's stream."""
        check(lib().sosrt_phase_delta_m_dev(self._h, int(S), _vp(d_chi), int(lmax), int(order), _vp(d_tab_mu), int(ntab),
                                            _vp(d_tab_out), _vp(d_f_out)))

    def p0_normaliser_device(self, kind, d_mu0: int, d_Z_out: int, B: int, g=0.0):
        """d_Z_out [B] = the normaliser `phase_p0_rows_azimuth_device` divides the point values of column b by."""
        check(lib().sosrt_phase_p0_normaliser_dev(self._h, int(B), self._KINDS[kind], float(g), _vp(d_mu0), _vp(d_Z_out)))

    def p0_normaliser(self, kind, mu0, g=0.0):
        """The same for a host array of mu0 -> [len(mu0)]."""
        import torch
        dev = torch.device("cuda", self.device)
        d_mu0 = torch.from_numpy(np.array(np.atleast_1d(mu0), dtype=np.float64)).to(dev)
        d_Z = torch.empty(d_mu0.shape[0], dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self.p0_normaliser_device(kind, d_mu0.data_ptr(), d_Z.data_ptr(), d_mu0.shape[0], g)
        self.synchronize()
        return d_Z.cpu().numpy()

    # ---- Fourier modes in azimuth (sosrt.h: azimuth-resolved radiance) ----
    def phase_modes(self, kind, m_first, m_count, nphi=25, g=0.0):
        """Modes m_first .. m_first + m_count - 1 of P -> [m_count, 2N, 2N].  Mode 0 is `phase_matrix` bit for bit; modes
        m >= 1 use the nphi-point ring (1 <= m <= min(64, nphi - 2))."""
        out = np.empty((int(m_count), self.D, self.D))
        check(lib().sosrt_phase_modes(self._h, self._KINDS[kind], float(g), int(m_first), int(m_count), int(nphi), _ptr(out)))
        return out

    def phase_modes_device(self, kind, d_P_out: int, m_first, m_count, nphi=25, g=0.0, sign_odd=False):
        """`phase_modes` left on the device: d_P_out is the address of [m_count, 2N, 2N] float64; enqueued on the handle's
        stream.  sign_odd: mode m is written as (-1)^m P^m, what the solve of mode m takes (`set_phase_sets_device`)."""
        check(lib().sosrt_phase_modes_dev(self._h, self._KINDS[kind], float(g), int(m_first), int(m_count), int(nphi),
                                          1 if sign_odd else 0, ctypes.c_void_p(d_P_out) if d_P_out else None))

    def phase_p0_modes(self, kind, mu0, m_first, m_count, nphi=25, g=0.0):
        """The same modes of P0 for an array of mu0 -> [m_count, len(mu0), 2N]."""
        m = np.ascontiguousarray(np.atleast_1d(mu0), dtype=np.float64)
        out = np.empty((int(m_count), m.size, self.D))
        step = max(1, self.max_batch)
        for i in range(0, m.size, step):
            mm = np.ascontiguousarray(m[i:i + step])
            oo = np.empty((int(m_count), mm.size, self.D))
            check(lib().sosrt_phase_p0_modes(self._h, int(mm.size), self._KINDS[kind], float(g), int(m_first), int(m_count),
                                             int(nphi), _ptr(mm), _ptr(oo)))
            out[:, i:i + step] = oo
        return out

    def phase_p0_modes_device(self, kind, d_mu0: int, d_P0_out: int, B: int, m_first, m_count, nphi=25, g=0.0):
        """Device twin: d_mu0 [B], d_P0_out [m_count][B][2N] (addresses), enqueued on the handle's stream."""
        check(lib().sosrt_phase_p0_modes_dev(self._h, int(B), self._KINDS[kind], float(g), int(m_first), int(m_count), int(nphi),
                                             ctypes.c_void_p(d_mu0), ctypes.c_void_p(d_P0_out)))

    # ---- view radiance: the solved field's source integrated off the grid (sosrt.h) ----
    _QUADS = {"grid": _lib.VIEW_QUAD_GRID, "linear": _lib.VIEW_QUAD_LINEAR}

    def phase_rows_device(self, kind, mu_signed, d_rows_out: int, g=0.0):
        """Rows of the stored phase matrix at the exit cosines `mu_signed` [V2] (host, off the grid or on it) with the stored
        matrix's own normalisers: d_rows_out is the address of [V2, 2N] float64; enqueued on the handle's stream."""
        m = np.ascontiguousarray(np.atleast_1d(mu_signed), dtype=np.float64)
        check(lib().sosrt_phase_rows_dev(self._h, self._KINDS[kind], float(g), int(m.size), _ptr(m),
                                         ctypes.c_void_p(d_rows_out) if d_rows_out else None))

    def phase_p0_rows_device(self, kind, d_mu0: int, mu_signed, d_out: int, B: int, g=0.0):
        """The same of P0 for B columns: d_mu0 [B], d_out [B, V2] (addresses)."""
        m = np.ascontiguousarray(np.atleast_1d(mu_signed), dtype=np.float64)
        check(lib().sosrt_phase_p0_rows_dev(self._h, int(B), self._KINDS[kind], float(g), _vp(d_mu0), int(m.size), _ptr(m), _vp(d_out)))

    def view_radiance_device(self, mu_view, d_tau: int, d_I_src: int, d_rows_atm: int, d_rows_aer: int, levels,
                             d_scat_out: int = 0, d_first_out: int = 0, d_p0rows_atm: int = 0, d_p0rows_aer: int = 0,
                             quadrature="grid", B: Optional[int] = None):
        """Radiance at the view cosines `mu_view` [V] (host, each in [0.01, 1], V <= 64) at the rows `levels`, from the field
        d_I_src [B, L, 2N] and the current columns: d_scat_out [B, nlev, 2V] the transport of the field's source at the signed
        lanes (-mu_view, +mu_view), d_first_out [B, nlev, 2V] the closed-form first order (needs the p0rows).  quadrature:
        'grid' (the grid's trapezoid arithmetic: at a node, with I_src = I - I_last, the grid's own I - I1) or 'linear' (exact
        attenuation of a piecewise-linear source: the one for limb-ward views, where dtau / mu >~ 1).  All d_* are device
        addresses; enqueued on the handle's stream; nothing but the outputs is written."""
        m = np.ascontiguousarray(np.atleast_1d(mu_view), dtype=np.float64)
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.int32)
        q = self._QUADS.get(quadrature, quadrature)
        if isinstance(q, str) or isinstance(q, bool) or not isinstance(q, (int, np.integer)):
            raise ValueError("quadrature must be 'grid' or 'linear' (got %r)" % (quadrature,))
        check(lib().sosrt_view_radiance_dev(self._h, int(self.B if B is None else B), int(m.size), _ptr(m), _vp(d_tau), _vp(d_I_src),
                                            _vp(d_rows_atm), _vp(d_rows_aer), _vp(d_p0rows_atm), _vp(d_p0rows_aer), int(q),
                                            int(lev.size), _ptr(lev), _vp(d_scat_out), _vp(d_first_out)))

    def view_timing(self):
        """Milliseconds of the last `view_radiance_device`: (source contraction, sweeps, first order); waits for them."""
        ms = (ctypes.c_double * 3)()
        check(lib().sosrt_view_timing(self._h, ms))
        return tuple(ms)

    # ---- azimuth-resolved view radiance: the view stage per Fourier mode (sosrt.h) ----
    def phase_rows_modes_device(self, kind, mu_signed, d_rows_out: int, m_first, m_count, nphi=25, g=0.0, sign_odd=False):
        """Rows of the modes m_first .. m_first + m_count - 1 (m_first >= 1) of the phase function at the exit cosines
        `mu_signed` [V2] (host), normalised as `phase_modes` normalises: d_rows_out is the address of [m_count, V2, 2N] float64.
        sign_odd: mode m is written as (-1)^m rows^m, what `view_radiance_device` takes for the field of mode m."""
        m = np.ascontiguousarray(np.atleast_1d(mu_signed), dtype=np.float64)
        check(lib().sosrt_phase_rows_modes_dev(self._h, self._KINDS[kind], float(g), int(m_first), int(m_count), int(nphi),
                                               int(bool(sign_odd)), int(m.size), _ptr(m),
                                               ctypes.c_void_p(d_rows_out) if d_rows_out else None))

    def phase_p0_rows_modes_device(self, kind, d_mu0: int, mu_signed, d_out: int, B: int, m_first, m_count, nphi=25, g=0.0):
        """The same of P0 for B columns: d_mu0 [B], d_out [m_count, B, V2] (addresses)."""
        m = np.ascontiguousarray(np.atleast_1d(mu_signed), dtype=np.float64)
        check(lib().sosrt_phase_p0_rows_modes_dev(self._h, int(B), self._KINDS[kind], float(g), int(m_first), int(m_count),
                                                  int(nphi), _vp(d_mu0), int(m.size), _ptr(m), _vp(d_out)))

    def phase_p0_rows_azimuth_device(self, kind, d_mu0: int, mu_signed, d_phi: int, nphi_out: int, d_out: int, B: int, g=0.0):
        """p(c(s_j, mu0_b, phi_i)) / Z0_b, the first-order phase value at a view lane and an azimuth with the normaliser of
        `phase_p0_rows_device`: d_mu0 [B], d_phi [nphi_out] (radians), d_out [nphi_out, B, V2] (addresses).  The [B, V2] block of
        one azimuth is a `d_p0rows_*` of `view_radiance_device`."""
        m = np.ascontiguousarray(np.atleast_1d(mu_signed), dtype=np.float64)
        check(lib().sosrt_phase_p0_rows_azimuth_dev(self._h, int(B), self._KINDS[kind], float(g), _vp(d_mu0), int(m.size), _ptr(m),
                                                    int(nphi_out), _vp(d_phi), _vp(d_out)))

    def view_azimuth_accumulate_device(self, m: int, d_val: int, nlev: int, V2: int, d_phi: int, nphi_out: int, d_out: int,
                                       B: Optional[int] = None):
        """out[b][lev][j][i] (+)= (2 - delta_m0) val[b][lev][j] cos(m phi[i]) on device addresses (m = 0 writes): the synthesis
        of `azimuth_accumulate_device` over view lanes, d_val [B, nlev, V2] being mode m of the view radiance."""
        check(lib().sosrt_view_azimuth_accumulate_dev(self._h, int(self.B if B is None else B), int(m), int(nlev), int(V2), _vp(d_val),
                                                      int(nphi_out), _vp(d_phi), _vp(d_out)))

    def set_order_targets(self, d_targets: Optional[int]):
        """Fixed order counts for the solves that follow: `d_targets` is the device address of an int32 [B] array (kept by the
        caller while set), None / 0 switches back to the convergence test."""
        check(lib().sosrt_set_order_targets(self._h, ctypes.c_void_p(d_targets) if d_targets else None))

    def azimuth_accumulate_device(self, m: int, d_Im: int, d_levels: int, nlev: int, d_phi: int, nphi_out: int, d_out: int,
                                  B: Optional[int] = None):
        """out[b][lev][dir][j] (+)= (2 - delta_m0) I^m[b][levels[lev]][dir] cos(m phi[j]) on device addresses (m = 0 writes)."""
        check(lib().sosrt_azimuth_accumulate_dev(self._h, int(self.B if B is None else B), int(m), ctypes.c_void_p(d_Im), int(nlev),
                                                 ctypes.c_void_p(d_levels), int(nphi_out), ctypes.c_void_p(d_phi),
                                                 ctypes.c_void_p(d_out)))

    def azimuth_synthesize_device(self, M: int, d_I0: int, d_Im: int, d_levels: int, nlev: int, d_phi: int, nphi_out: int,
                                  d_out: int, B: Optional[int] = None):
        """The whole synthesis in one launch: out[b][lev][dir][j] = I0[b][levels[lev]][dir] + sum_{m=1..M} 2 Im[m-1][b][levels[lev]]
        [dir] cos(m phi[j]) on device addresses (d_I0 [B, L, 2N], d_Im [M, B, L, 2N]); the bits of `azimuth_accumulate_device`
        called for m = 0..M."""
        check(lib().sosrt_azimuth_synthesize_dev(self._h, int(self.B if B is None else B), int(M), _vp(d_I0), _vp(d_Im), int(nlev),
                                                 _vp(d_levels), int(nphi_out), _vp(d_phi), _vp(d_out)))

    # ---- multi-GPU gather over RCCL (one process per GPU) -------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """128-byte RCCL id, made by one rank and handed to the others by any means."""
        buf = ctypes.create_string_buffer(128)
        check(lib().sosrt_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        check(lib().sosrt_comm_init(self._h, int(rank), int(world), ctypes.c_char_p(unique_id)))

    def gather_device(self, root: int, counts, d_send: int, d_recv: int):
        """counts[world] doubles per rank; d_send / d_recv device addresses; enqueued on the handle's stream."""
        c = np.ascontiguousarray(counts, dtype=np.int64)
        check(lib().sosrt_gather(self._h, int(root), _ptr(c), ctypes.c_void_p(d_send) if d_send else None,
                                 ctypes.c_void_p(d_recv) if d_recv else None))

    def comm_destroy(self):
        check(lib().sosrt_comm_destroy(self._h))

    # ---- helper level ----------------------------------------------------------
    def limit_mu_down(self, rows, idx):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != self.N:
            raise ValueError("rows must be [R, nb_angles]")
        out = np.empty((rows.shape[0], idx))
        if idx:
            check(lib().sosrt_limit_mu_down(self._h, rows.shape[0], int(idx), _ptr(rows), _ptr(out)))
        return out

    def asymptotic_down(self, J, tau, lens, tau_t, mu):
        J = np.ascontiguousarray(J, dtype=np.float64)
        tau = _f64(tau, J.shape, "tau")
        R, stride = J.shape
        lens = _i32(lens, R, "len")
        tt = _f64(tau_t, (R,), "tau_t")
        m = _f64(mu, (R,), "mu")
        out = np.empty(R)
        check(lib().sosrt_asymptotic_down(self._h, R, stride, _ptr(lens), _ptr(J), _ptr(tau), _ptr(tt), _ptr(m), _ptr(out)))
        return out

    # ---- plan introspection (host only) ----------------------------------------
    def plan_weights(self):
        w = np.empty(self.D)
        check(lib().sosrt_plan_weights(self._h, _ptr(w)))
        return w

    def plan_fold(self, which=0):
        W = np.empty((self.D, self.D))
        check(lib().sosrt_plan_fold(self._h, which, _ptr(W)))
        return W

    def plan_fix_table(self, idx):
        s0, ns = ctypes.c_int(), ctypes.c_int()
        C = np.zeros((max(idx, 1), 5))
        check(lib().sosrt_plan_fix_table(self._h, int(idx), ctypes.byref(s0), ctypes.byref(ns), _ptr(C)))
        return s0.value, ns.value, C.reshape(-1)[: idx * ns.value].reshape(idx, ns.value).copy()

    def plan_launch(self, batch, live, surface="specular", zones=3, cus=0):
        """The kernels an order of the order loop launches for a batch of `batch` columns (up to `zones` zones each) of whose
        first column group `live` are live -- sosrt_plan_launch, the one function the order loop decides with; host only."""
        sf = {"none": _lib.SURFACE_NONE, "specular": _lib.SURFACE_SPECULAR, "lambertian": _lib.SURFACE_LAMBERTIAN,
              "lambertian_readme": _lib.SURFACE_LAMBERTIAN_README}[surface]
        out = (ctypes.c_int * 9)()
        check(lib().sosrt_plan_launch(self._h, int(batch), int(live), sf, int(zones), int(cus), out))
        keys = ("groups", "gemm", "tail_cols", "transport", "parts", "repair", "order_loop", "ol_parts", "ol_grid")
        return dict(zip(keys, list(out)))

    def plan_ring_moments(self, batch, live, surface="specular", zones=3, cus=0, saved_orders=False, atm_sets=False,
                          need_smallmu=False):
        """Whether an order of `batch` columns with `live` of its first group live runs in the ring kernel's moment mode
        (sosrt_plan_ring_moments: the same plan as plan_launch, with the handle's own phase matrices); host only."""
        sf = {"none": _lib.SURFACE_NONE, "specular": _lib.SURFACE_SPECULAR, "lambertian": _lib.SURFACE_LAMBERTIAN,
              "lambertian_readme": _lib.SURFACE_LAMBERTIAN_README}[surface]
        on = ctypes.c_int(0)
        flags = (1 if saved_orders else 0) | (2 if atm_sets else 0) | (4 if need_smallmu else 0)
        check(lib().sosrt_plan_ring_moments(self._h, int(batch), int(live), sf, int(zones), int(cus), flags, ctypes.byref(on)))
        return bool(on.value)

    def ring_moments_stats(self):
        """(the (column group, order) pairs of the last solve that ran in the ring kernel's moment mode, all the pairs that its
        two-launch loop ran): what the solve did, where plan_ring_moments says what a plan would allow"""
        a, b = ctypes.c_int(), ctypes.c_int()
        check(lib().sosrt_ring_moments_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def plan_scan_moments(self, batch, live, surface="specular", zones=3, cus=0, saved_orders=False, atm_sets=False,
                          need_smallmu=False):
        """Whether an order of `batch` columns with `live` of its first group live runs in the chunk-parallel kernel's moment mode
        (sosrt_plan_scan_moments: a second decision of the plan plan_ring_moments asks); host only."""
        sf = {"none": _lib.SURFACE_NONE, "specular": _lib.SURFACE_SPECULAR, "lambertian": _lib.SURFACE_LAMBERTIAN,
              "lambertian_readme": _lib.SURFACE_LAMBERTIAN_README}[surface]
        on = ctypes.c_int(0)
        flags = (1 if saved_orders else 0) | (2 if atm_sets else 0) | (4 if need_smallmu else 0)
        check(lib().sosrt_plan_scan_moments(self._h, int(batch), int(live), sf, int(zones), int(cus), flags, ctypes.byref(on)))
        return bool(on.value)

    def scan_moments_stats(self):
        """(the (column group, order) pairs of the last solve that ran in the chunk-parallel kernel's moment mode, all the pairs
        that its two-launch loop ran)"""
        a, b = ctypes.c_int(), ctypes.c_int()
        check(lib().sosrt_scan_moments_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def microbench(self, which):
        """0: FP64 MFMA TFLOP/s, 1: streaming copy GB/s, 2: FP64 FMA TFLOP/s, measured on this device."""
        r = ctypes.c_double()
        check(lib().sosrt_microbench(self._h, int(which), ctypes.byref(r)))
        return r.value

    # ---- profiling ---------------------------------------------------------------
    def profile_enable(self, on=True):
        check(lib().sosrt_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        check(lib().sosrt_profile_reset(self._h))

    def profile_get(self, kernel):
        ms, cnt, w = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        check(lib().sosrt_profile_get(self._h, kernel, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(w)))
        return ms.value, cnt.value


def fix_count(tau_ref: float, nb_angles: int) -> int:
    """Number of downward angles next to mu=0 the reference rewrites (I1_In:124-127)."""
    return lib().sosrt_plan_fix_count(float(tau_ref), int(nb_angles))
