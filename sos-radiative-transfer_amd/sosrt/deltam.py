"""Delta-M scaling of a forward-peaked aerosol (Wiscombe 1977) with the TMS first order (Nakajima & Tanaka 1988): DESIGN
section 28.

The phase function is replaced by its Legendre series truncated at order Lambda, with the fraction f = chi_Lambda of the
scattering counted as unscattered: the solve sees a smooth table, a thinner and more absorbing aerosol (`scale_optics`) and a
Fourier series in azimuth that ends at Lambda - 1.  The moments and the truncated table are built on the device
(`Solver.phase_moments_device`, `Solver.delta_m_table_device`), where the Mie tables are."""
from __future__ import annotations

import numpy as np

MIN_ORDER, MAX_ORDER = 2, 128      # the drivers' `delta_m=` (the C entry takes order 1 too: the isotropic remainder)
HG_NTAB = 6001                     # the uniform abscissa an analytic function is tabulated on (that of the Mie tables)


def scale_optics(tauStar_aer, alb_aer, f):
    """(tauStar_aer (1 - w f), (1 - f) w / (1 - w f)) with w = alb_aer: the optical depth and single-scattering albedo of the
    aerosol once the fraction f of its scattering is counted as unscattered.  Arrays broadcast.  Absorption is kept,
    (1 - w') tau' = (1 - w) tau, and the scattering is (1 - f) w tau; f = 0 returns the inputs bit for bit."""
    t, w, f = np.broadcast_arrays(np.asarray(tauStar_aer, dtype=np.float64), np.asarray(alb_aer, dtype=np.float64),
                                  np.asarray(f, dtype=np.float64))
    k = 1 - w * f
    return t * k, (1 - f) * w / k


def hg_moments(g, lmax):
    """The Legendre moments of Henyey-Greenstein: chi_l = g^l, l = 0 .. lmax."""
    return float(g) ** np.arange(int(lmax) + 1)


def check_order(order):
    """`delta_m=` of the drivers as an int in MIN_ORDER .. MAX_ORDER."""
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or not MIN_ORDER <= int(order) <= MAX_ORDER:
        raise ValueError("delta_m must be None or an integer order in %d..%d (got %r)" % (MIN_ORDER, MAX_ORDER, order))
    return int(order)


def delta_m(solver, name, order, g=0.0, mie=None):
    """Delta-M of the named phase function on `solver` at `order` = Lambda.  'fwc' / 'table' / 'mie' / 'eva' / 'wildfire': the
    table the drivers would hand to the builders (`mie` = the dict of `mie_aer`; `device=True` in it builds it with the Mie
    kernels of this handle) goes to the device and its moments 0 .. Lambda are taken there; 'hg': the analytic moments g^l, on
    the uniform abscissa of HG_NTAB points.  The truncated table is left as the handle's table (`Solver.set_phase_table_dev`, in
    stream order), so the builders of kind 'table' read it.  Returns (f, the device address of the exact table DIVIDED BY ITS
    NORM half its integral, so that its mean over [-1, 1] is 1 as the truncated table's is: what the TMS first order evaluates
    -- for 'hg' 0: the exact function is the kind 'hg' itself --, a dict that keeps the device arrays alive: 'tab_mu' [ntab]
    float64, 'exact' (that table) and 'truncated' [ntab], 'chi' [Lambda + 1], 'f' [1] as torch tensors, and 'ntab').  'iso' and
    'rayleigh' have no forward peak to move: ValueError."""
    import torch
    from .inputs import _scalar_phase
    order = int(order)
    if name in ("iso", "rayleigh"):
        raise ValueError("delta_m is for a forward-peaked aerosol: %r has no peak to truncate" % (name,))
    dev = torch.device("cuda", solver.device)
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dev)
    keep = {}
    d_mu = lambda: keep["tab_mu"].data_ptr()
    if name == "hg":
        ntab = HG_NTAB
        keep["tab_mu"] = up(np.linspace(-1, 1, ntab))
        d_mu = lambda: 0                                   # (the entries' own uniform abscissa: the same numbers)
        keep["chi"] = up(hg_moments(g, order))
        keep["exact"] = None
    else:
        kw = dict(mie or {})
        if kw.get("device") is True:
            kw["device"] = solver
        kind, tab = _scalar_phase(name, g, **kw)[1]
        if tab is None:
            raise ValueError("delta_m needs 'hg' or a tabulated phase function (got %r)" % (name,))
        ntab = int(len(tab[0]))
        keep["tab_mu"], keep["exact"] = up(tab[0]), up(tab[1])
        keep["chi"] = torch.empty(order + 1, dtype=torch.float64, device=dev)
        keep["norm"] = torch.empty(1, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        solver.phase_moments_device(keep["exact"].data_ptr(), 1, ntab, order, keep["chi"].data_ptr(), keep["norm"].data_ptr(),
                                    d_tab_mu=d_mu())
        solver.synchronize()
        keep["exact"] = keep["exact"] / keep["norm"]       # the mean over [-1, 1] is 1, as the truncated table's is
    keep["truncated"] = torch.empty(ntab, dtype=torch.float64, device=dev)
    keep["f"] = torch.empty(1, dtype=torch.float64, device=dev)
    keep["ntab"] = ntab
    torch.cuda.current_stream(dev).synchronize()
    solver.delta_m_table_device(keep["chi"].data_ptr(), 1, order, order, ntab, keep["truncated"].data_ptr(), keep["f"].data_ptr(),
                                d_tab_mu=d_mu())
    solver.set_phase_table_dev(keep["truncated"].data_ptr(), ntab, d_mu())
    solver.synchronize()
    f = float(keep["f"].cpu().numpy()[0])
    return f, 0 if keep["exact"] is None else keep["exact"].data_ptr(), keep
