"""The modes of an azimuth-resolved call solved as one batch (SOS_Aer_batch(..., mode_batch=True)) against
the loop over the modes, bit for bit; the one-launch synthesis against the per-mode launches; the signed device modes."""
import numpy as np
import pytest
import torch

from sosrt import inputs
from sosrt.main import SOS_Aer_batch
from sosrt.solver import Solver

pytestmark = pytest.mark.gpu


def _same(a, b):
    assert np.array_equal(a.I_azimuth, b.I_azimuth, equal_nan=True) and np.array_equal(a.mode_status, b.mode_status)
    assert np.array_equal(a.I, b.I) and np.array_equal(a.n, b.n) and np.array_equal(a.status, b.status)


# ---- 6: driver -------------------------------------------------------------------------------
def test_mode_batch_is_the_loop_bit_for_bit():
    mu0 = np.array([0.3, 0.6, 0.9])
    kw = dict(alb_aer=0.95, nb_layers=60, nb_angles=64, atm_phase_fun="rayleigh", aer_phase_fun="hg", g_aer=0.7,
              azimuths=np.linspace(0, np.pi, 7), n_modes=4, levels=(0, 10, -1))
    plain = SOS_Aer_batch(mu0, 0.3, 0.15, **{k: v for k, v in kw.items() if k not in ("azimuths", "n_modes", "levels")})
    loop = SOS_Aer_batch(mu0, 0.3, 0.15, mode_batch=False, **kw)
    assert (loop.mode_status == 0).all() and loop.I_azimuth.shape == (3, 3, 128, 7)
    _same(SOS_Aer_batch(mu0, 0.3, 0.15, mode_batch=True, **kw), loop)
    _same(SOS_Aer_batch(mu0, 0.3, 0.15, mode_batch=True, mode_chunk=3, **kw), loop)       # two chunks: 3 + 1 modes
    # the cached handle is left as it was: the plain call again gives the same bits
    again = SOS_Aer_batch(mu0, 0.3, 0.15, **{k: v for k, v in kw.items() if k not in ("azimuths", "n_modes", "levels")})
    assert np.array_equal(again.I, plain.I) and np.array_equal(again.n, plain.n) and np.array_equal(loop.I, plain.I)


def test_mode_batch_eva_at_the_flagship_shape():
    mu0 = np.array([0.4, 0.8])
    kw = dict(nb_layers=200, nb_angles=128, atm_phase_fun="rayleigh", aer_phase_fun="eva", azimuths=np.linspace(0, np.pi, 5),
              n_modes=6, levels=(0, -1))
    _same(SOS_Aer_batch(mu0, 0.12, 0.1, mode_batch=True, **kw), SOS_Aer_batch(mu0, 0.12, 0.1, **kw))


# ---- 7: driver refusals ----------------------------------------------------------------------
def test_an_atmosphere_that_is_not_low_rank_is_refused():
    mu0 = np.array([0.3, 0.6])
    kw = dict(nb_layers=60, nb_angles=64, atm_phase_fun="hg", g_atm=0.5, aer_phase_fun="hg", g_aer=0.7,
              azimuths=np.linspace(0, np.pi, 3), n_modes=2)
    before = SOS_Aer_batch(mu0, 0.3, 0.15, mode_batch=False, **kw)
    with pytest.raises(ValueError, match="mode_batch=False works"):
        SOS_Aer_batch(mu0, 0.3, 0.15, mode_batch=True, **kw)
    after = SOS_Aer_batch(mu0, 0.3, 0.15, mode_batch=False, **kw)                 # (the handle was put back)
    _same(after, before)
    assert (after.mode_status == 0).all()


# ---- 8: synthesis ----------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 1, 64])
def test_one_launch_synthesis_is_the_sequence_of_accumulate_launches(M):
    """Random fields, two levels and one outside [0, L), 7 azimuths.  (N = 4, not the 3 the issue names: sosrt_create takes
    nb_angles >= 4, so no handle -- and no launch -- exists at N = 3; 4 is the smallest, and 2N x 7 = 56 elements is still no
    multiple of anything in the kernel.)"""
    B, L, N = 2, 5, 4
    D = 2 * N
    s = Solver(L, N, max_batch=B)
    s.set_grid(inputs.direction_grid(N))
    rng = np.random.default_rng(M)
    dev = torch.device("cuda", 0)
    d_I = torch.from_numpy(rng.standard_normal((M + 1, B, L, D))).to(dev)
    d_lev = torch.tensor([0, 4, 7], dtype=torch.int32, device=dev)                # (7: outside [0, L) -- NaN rows)
    d_phi = torch.from_numpy(np.linspace(0, 2 * np.pi, 7)).to(dev)
    seq = torch.full((B, 3, D, 7), 5.0, dtype=torch.float64, device=dev)
    one = torch.full((B, 3, D, 7), 6.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for m in range(M + 1):
        s.azimuth_accumulate_device(m, d_I[m].data_ptr(), d_lev.data_ptr(), 3, d_phi.data_ptr(), 7, seq.data_ptr(), B=B)
    s.azimuth_synthesize_device(M, d_I[0].data_ptr(), d_I[1:].data_ptr() if M else 0, d_lev.data_ptr(), 3, d_phi.data_ptr(), 7,
                                one.data_ptr(), B=B)
    s.synchronize()
    a, b = seq.cpu().numpy(), one.cpu().numpy()
    try:
        with pytest.raises(ValueError, match="SOSRT_MAX_MODES"):           # (one mode more than the kernel's table holds)
            s.azimuth_synthesize_device(65, d_I[0].data_ptr(), d_I[0].data_ptr(), d_lev.data_ptr(), 3, d_phi.data_ptr(), 7,
                                        one.data_ptr(), B=B)
        s.synchronize()
        assert np.array_equal(one.cpu().numpy(), b, equal_nan=True)         # (refused before any launch)
    finally:
        s.close()
    assert np.isnan(a[:, 2]).all() and not np.isnan(a[:, :2]).any()
    assert np.array_equal(a, b, equal_nan=True)
    if M == 0:
        assert np.array_equal(b[:, 0], np.broadcast_to(d_I[0, :, 0].cpu().numpy()[..., None], (B, D, 7)))


# ---- 9: signed device modes ------------------------------------------------------------------
@pytest.mark.parametrize("name,g,N", [("hg", 0.7, 37), ("fwc", 0.0, 32)])
def test_signed_modes_on_the_device_are_the_host_modes(name, g, N):
    s = Solver(20, N, max_batch=1)
    s.set_grid(inputs.direction_grid(N))
    kind, tab = inputs._scalar_phase(name, g)[1]
    if tab is not None:
        s.set_phase_table(*tab)
    host = s.phase_modes(kind, 1, 4, 25, g)
    sgn = np.where(np.arange(1, 5) & 1, -1.0, 1.0)[:, None, None]
    d = torch.zeros((4, 2 * N, 2 * N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for signed in (True, False):
        s.phase_modes_device(kind, d.data_ptr(), 1, 4, 25, g, sign_odd=signed)
        s.synchronize()
        assert np.array_equal(d.cpu().numpy(), sgn * host if signed else host)
    # mode 0 in front, as sosrt_phase_modes lays it out
    d0 = torch.zeros((3, 2 * N, 2 * N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.phase_modes_device(kind, d0.data_ptr(), 0, 3, 25, g, sign_odd=True)
    s.synchronize()
    assert np.array_equal(d0.cpu().numpy(), np.array([1.0, -1.0, 1.0])[:, None, None] * s.phase_modes(kind, 0, 3, 25, g))
    assert np.any(host[3])
    s.close()
