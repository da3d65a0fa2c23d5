"""Atmosphere phase sets and the batched azimuth modes without a GPU: the new entry points are declared and exported, the header's
version line stands, and the argument checks of the driver are made before any handle exists."""
import os
import re
import subprocess

import numpy as np
import pytest

from sosrt import _lib
from sosrt import main as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sosrt_set_atm_phase_sets", "sosrt_set_atmosphere_sets", "sosrt_atm_sets_info", "sosrt_phase_modes_dev",
       "sosrt_azimuth_synthesize_dev")


def _header():
    with open(os.path.join(ROOT, "include", "sosrt.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", NEW)
def test_new_symbols_are_declared_bound_and_exported(name):
    assert re.search(r"^int %s\(sosrt_t\* h, " % name, _header(), re.M), name
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.lib(), name)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % name, out, re.M), name


def test_the_version_line_is_unchanged():
    assert "#define SOSRT_VERSION 105\n" in _header()
    assert _lib.lib().sosrt_version() == 105


def test_argument_checks_come_before_any_handle(monkeypatch):
    def no_handle(*a, **k):
        raise AssertionError("a handle was asked for")
    monkeypatch.setattr(M, "get_solver", no_handle)
    az = dict(azimuths=np.array([0.0, 1.0]), n_modes=2)
    for bad in (dict(mode_batch=1), dict(mode_batch="yes"), dict(mode_chunk=2), dict(mode_batch=True, mode_chunk=0),
                dict(mode_batch=True, mode_chunk=65), dict(mode_batch=True, mode_chunk=2.0), dict(mode_batch=True, mode_chunk=True)):
        with pytest.raises(ValueError, match="mode_"):
            M.SOS_Aer_batch(0.5, 0.1, 0.1, nb_layers=20, nb_angles=8, **az, **bad)
    for kw in (dict(mode_batch=True), dict(mode_chunk=2)):                         # without azimuths
        with pytest.raises(ValueError, match="azimuths"):
            M.SOS_Aer_batch(0.5, 0.1, 0.1, nb_layers=20, nb_angles=8, **kw)
    # the checks themselves
    args = (np.array([0.0]), 4, None, (0, -1), 20, None, None, None, None, "specular", None, "coded")
    assert M._azimuth_args(*args) == M._azimuth_args(*args, mode_batch=True, mode_chunk=3) == (4, 25, [0, 19])
    assert M._mode_chunk_cap(3, 60, 64, 4, None) == 4 and M._mode_chunk_cap(3, 60, 64, 4, 3) == 3
    assert M._mode_chunk_cap(1, 200, 128, 64, None) == 64 and M._mode_chunk_cap(512, 200, 128, 16, None) == 5
    # a field that MODE_BATCH_FIELD_BYTES does not hold even for one mode
    monkeypatch.setattr(M, "MODE_BATCH_FIELD_BYTES", 1000)
    with pytest.raises(ValueError, match="mode_batch=False works"):
        M.SOS_Aer_batch(0.5, 0.1, 0.1, nb_layers=20, nb_angles=8, mode_batch=True, **az)
    # the fields of all modes, which wait for the one synthesis launch whatever the chunk: refused beyond MODE_BATCH_MODES_BYTES
    monkeypatch.setattr(M, "MODE_BATCH_FIELD_BYTES", 1 << 30)
    assert M.MODE_BATCH_MODES_BYTES == 16 << 30 and M._mode_chunk_cap(512, 200, 128, 64, None) == 5      # (13.4 GB: taken)
    with pytest.raises(ValueError, match="MODE_BATCH_MODES_BYTES.*mode_batch=False works"):
        M._mode_chunk_cap(1024, 200, 128, 64, 1)                                                         # (26.8 GB)
    monkeypatch.setattr(M, "MODE_BATCH_MODES_BYTES", 2 * 20 * 16 * 8)                                    # (one column, two modes)
    M._mode_chunk_cap(1, 20, 8, 2, None)
    with pytest.raises(ValueError, match="MODE_BATCH_MODES_BYTES"):
        M.SOS_Aer_batch([0.5, 0.6], 0.1, 0.1, nb_layers=20, nb_angles=8, mode_batch=True, mode_chunk=1, **az)
