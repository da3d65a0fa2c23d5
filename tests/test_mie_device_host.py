"""The device Mie builder's host-side surface (no GPU): ABI version, the "no device" error of a host-only handle, the
untouched default of `inputs.scenario_table`, and the argument checks of `SOS_Aer_spectrum`."""
import numpy as np
import pytest

from sosrt import _lib, inputs, mie
from sosrt.main import SOS_Aer_spectrum, _spectrum_args
from sosrt.solver import Solver


def test_version_and_symbols():
    assert _lib.lib().sosrt_version() >= 103
    for name in ("sosrt_mie_ensembles", "sosrt_mie_ensembles_dev", "sosrt_mie_efficiencies", "sosrt_mie_timing", "sosrt_phase_table_dev"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)


def test_host_only_handle_refuses_the_device_builders():
    s = Solver(4, 4, device=-1)
    try:
        for call in (lambda: s.mie_ensembles(0.55, 1.44 + 0j, 0.506, 1.2),
                     lambda: s.mie_ensembles_device(8, 0, 0.55, 1.44 + 0j, 0.506, 1.2),
                     lambda: s.mie_efficiencies(1.5 + 0j, 10.0),
                     lambda: s.mie_timing(),
                     lambda: s.set_phase_table_dev(8, 6001),
                     lambda: mie.log_normal_bulk_phase_device(s, 0.55, 1.44 + 0j, 0.506, 1.2)):
            with pytest.raises(_lib.SosrtError, match="host-only"):
                call()
    finally:
        s.close()


def test_scenario_table_default_is_the_host_series(monkeypatch):
    """Without `device` the table is the host's, under the cache key it always had; the device tag is a key of its own."""
    calls = []
    real = mie.log_normal_bulk_phase

    def spy(**kw):
        calls.append(kw)
        return real(**dict(kw, nb_radius=3, nb_mu=11))      # (a small stand-in: the series itself is test_host.py's)

    monkeypatch.setattr(inputs, "_bulk_cache", {})
    monkeypatch.setattr(inputs._mie, "log_normal_bulk_phase", spy)
    t = inputs.scenario_table("eva")
    assert inputs.scenario_table("eva") is t and inputs.scenario_table("eva", device=None) is t and len(calls) == 1
    tab = inputs._scalar_phase("eva")[1][1]
    assert tab[0] is t[0] and tab[1] is t[1] and len(calls) == 1
    key = ("eva", ("convention", "n+ik"), ("m", 1.44 + 0j), ("r_m", 0.506), ("sig", 1.2), ("wl", 0.55))
    assert list(inputs._bulk_cache) == [key]
    # the device path asks the device (here: a host-only handle, which refuses) and never the host series
    s = Solver(4, 4, device=-1)
    try:
        with pytest.raises(_lib.SosrtError, match="host-only"):
            inputs.scenario_table("eva", device=s)
        with pytest.raises(_lib.SosrtError, match="host-only"):
            inputs._scalar_phase("mie", r=0.4, lambda0=0.55, indx=1.44, device=s)
    finally:
        s.close()
    assert len(calls) == 1 and list(inputs._bulk_cache) == [key]


def test_spectrum_argument_checks():
    aer = dict(m=1.44 + 0j, r_m=0.506, sig=1.2)
    wl = [0.4, 0.55, 0.8]
    for bad in (dict(wavelengths=[]), dict(wavelengths=[0.5, -1.0]), dict(wavelengths=[[0.5]]), dict(aer=dict(m=1.4)),
                dict(aer=dict(aer, extra=1)), dict(tauStar_aer=[0.1, 0.2]), dict(tauStar_aer=[0.1] * 3, angstrom=1.0),
                dict(tauStar_aer=lambda w: 0.1, angstrom=1.0), dict(tauStar_aer=-0.1), dict(alb_aer=[0.9, 0.9]),
                dict(lambda_ref=0.0), dict(aer=dict(aer, sig=[1.2, 1.3]))):
        kw = dict(dict(wavelengths=wl, mu0=0.5, tauStar_aer=0.12, grd_alb=0.15, aer=aer), **bad)
        with pytest.raises(ValueError):
            SOS_Aer_spectrum(**kw)
    for k in ("P_aer", "aer_phase_fun", "mie_aer", "tauStar_atm", "devices"):
        with pytest.raises(ValueError, match="sets %s itself" % k):
            SOS_Aer_spectrum(wl, 0.5, 0.12, 0.15, aer, **{k: None})
    w, t_aer, t_atm, m, r_m, sig = _spectrum_args(wl, 0.12, 1.5, 0.55, aer, "mie", 0.124)
    assert np.allclose(t_atm, 0.124 * (0.55 / np.array(wl)) ** 4, rtol=1e-15) and t_atm[1] == 0.124
    assert np.allclose(t_aer, 0.12 * (np.array(wl) / 0.55) ** -1.5, rtol=1e-15) and t_aer[1] == 0.12
    assert m.shape == r_m.shape == sig.shape == (3,) and m.dtype == complex
    assert np.array_equal(_spectrum_args(wl, lambda x: 2 * x, None, 0.55, aer, 0.9, 0.124)[1], 2 * np.array(wl))
