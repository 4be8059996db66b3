"""Hogbom and Clark CLEAN on the GPU against the numpy yardstick (tests/_clean_ref.py).  Images are non-square (96 x 80) so
an x / y swap shows."""

import numpy as np
import pytest

from tests import _clean_ref as ref

pytestmark = pytest.mark.gpu

NX, NY = 96, 80


def _gauss(nxp, nyp, sx, sy, peak=1.0, cx=0.0, cy=0.0):
    x = np.arange(nxp)[:, None] - nxp // 2 - cx
    y = np.arange(nyp)[None, :] - nyp // 2 - cy
    return peak * np.exp(-0.5 * (x / sx) ** 2 - 0.5 * (y / sy) ** 2)


def _psfhat(psf):
    return np.fft.rfft2(np.fft.ifftshift(psf, axes=(1, 2)), axes=(1, 2))


def _sky(nband, npts, rng, nx=NX, ny=NY):
    sky = np.zeros((nband, nx, ny))
    pos = set()
    while len(pos) < npts:
        pos.add((int(rng.integers(8, nx - 8)), int(rng.integers(8, ny - 8))))
    for n, (i, j) in enumerate(sorted(pos)):
        sky[:, i, j] = (1.0 + 0.37 * n) * (1 + 0.2 * rng.standard_normal(nband))
    return sky, sorted(pos)


def _plan(psf, psfhat=None):
    from pfb_imaging_amd.clean import CleanPlan

    return CleanPlan(psf, psfhat, NX, NY)


def test_hogbom_bit_identical_to_yardstick():
    rng = np.random.default_rng(11)
    nband = 3
    psf = np.stack([_gauss(2 * NX, 2 * NY, s, 0.8 * s, peak=pk) for s, pk in ((1.8, 1.0), (2.5, 0.8), (3.1, 1.3))])
    sky, _ = _sky(nband, 12, rng)
    dirty = ref.psf_convolve_cube(sky, _psfhat(psf), 2 * NY) + 0.01 * rng.standard_normal((nband, NX, NY))
    m_ref, r_ref, k_ref, s_ref = ref.hogbom(dirty, psf, gamma=0.1, pf=0.01, maxit=2000)
    plan = _plan(psf)
    model, status, resid = plan.hogbom(dirty, gamma=0.1, pf=0.01, maxit=2000, residual=True)
    assert plan.info["iters"] == k_ref and status == s_ref and k_ref > 100
    assert np.array_equal(model, m_ref)
    assert np.array_equal(resid, r_ref)


def test_hogbom_analytic_tie_and_zero_cases():
    from pfb_imaging_amd import deconv

    F, gamma, pf = 3.0, 0.1, 0.1
    psf = _gauss(2 * NX, 2 * NY, 2.0, 2.0)[None]
    dirty = F * psf[:, NX - 7:2 * NX - 7, NY - 5:2 * NY - 5]
    model, status = deconv.hogbom(dirty, psf, gamma=gamma, pf=pf, maxit=1000, verbosity=0)
    k = int(np.ceil(np.log(pf) / np.log(1 - gamma)))
    assert status == 0 and np.flatnonzero(model[0]).tolist() == [7 * NY + 5]
    assert model[0, 7, 5] == pytest.approx(F * (1 - (1 - gamma) ** k), rel=1e-12)
    # two exactly equal peaks: maxit = 1 takes the first in row-major order
    d2 = np.zeros((1, NX, NY))
    d2[0, 60, 3] = d2[0, 20, 70] = 1.0
    model, status = deconv.hogbom(d2, psf, gamma=0.5, maxit=1, verbosity=0)
    assert status == 1 and np.flatnonzero(model[0]).tolist() == [20 * NY + 70]
    model, status = deconv.hogbom(np.zeros((1, NX, NY)), psf, verbosity=0)
    assert status == 0 and not model.any()
    # float32 in, float32 out
    model, status = deconv.hogbom(dirty.astype(np.float32), psf.astype(np.float32), gamma=gamma, pf=pf, verbosity=0)
    assert model.dtype == np.float32 and np.flatnonzero(model[0]).tolist() == [7 * NY + 5]


def _clark_case(seed, nband=4, zero_band=1, extended=False):
    rng = np.random.default_rng(seed)
    psf = np.stack([_gauss(2 * NX, 2 * NY, 1.6 + 0.3 * b, 1.3 + 0.2 * b) for b in range(nband)])
    psfhat = _psfhat(psf)
    if extended:
        x = np.arange(NX)[:, None] - 50.0
        y = np.arange(NY)[None, :] - 37.0
        sky = np.exp(-0.5 * (x / 30) ** 2 - 0.5 * (y / 25) ** 2)[None].repeat(nband, 0) * 0.05
    else:
        sky, _ = _sky(nband, 10, rng)
    dirty = ref.psf_convolve_cube(sky, psfhat, 2 * NY) + 0.005 * rng.standard_normal((nband, NX, NY))
    wsums = np.linspace(1.0, 2.0, nband)
    if zero_band is not None:
        wsums[zero_band] = 0.0
        dirty[zero_band] = 0.0
    wsums /= wsums.sum()
    mask = np.ones((NX, NY))
    mask[70:90, 5:30] = 0.0
    return dirty, psf, psfhat, wsums, mask


def _assert_model_close(model, m_ref, rtol):
    assert np.array_equal(model != 0, m_ref != 0)
    assert np.abs(model - m_ref).max() <= rtol * np.abs(m_ref).max()


def test_clark_matches_yardstick():
    dirty, psf, psfhat, wsums, mask = _clark_case(5)
    kw = dict(gamma=0.1, pf=0.05, maxit=50, subpf=0.5, submaxit=1000)
    m_ref, r_ref, k_ref, s_ref, n_ref = ref.clark(dirty, psf, psfhat, wsums, mask, **kw)
    plan = _plan(psf, psfhat)
    model, status, resid = plan.clark(dirty, wsums, mask, residual=True, **kw)
    info = plan.info
    assert (info["iters"], info["minor_iters"], status) == (k_ref, n_ref, s_ref)
    assert k_ref > 2 and not model[1].any()
    _assert_model_close(model, m_ref, 1e-10)
    assert np.abs(resid - r_ref).max() <= 1e-10 * np.abs(r_ref).max()


def test_clark_conventions_pinned():
    """An asymmetric PSF (Gaussian plus an off-centre lobe), one major iteration, a few sub-minor steps: the device follows the
    reflected sub-minor PSF and the aliased xhat; a copied xhat would not pass."""
    nband = 2
    psf = np.stack([_gauss(2 * NX, 2 * NY, 2.0, 1.5) + 0.4 * _gauss(2 * NX, 2 * NY, 1.5, 1.5, cx=3, cy=-2) for _ in range(nband)])
    psfhat = _psfhat(psf)
    x = np.arange(NX)[:, None] - 40.0
    y = np.arange(NY)[None, :] - 33.0
    dirty = np.exp(-0.5 * (x / 6) ** 2 - 0.5 * (y / 5) ** 2)[None].repeat(nband, 0) * np.array([1.0, 0.8])[:, None, None]
    wsums = np.array([0.5, 0.5])
    mask = np.ones((NX, NY))
    kw = dict(gamma=0.3, pf=0.01, maxit=1, subpf=0.3, submaxit=6)
    m_ref, _, _, _, n_ref = ref.clark(dirty, psf, psfhat, wsums, mask, **kw)
    m_copy, _, _, _, _ = ref.clark(dirty, psf, psfhat, wsums, mask, copy_xhat=True, **kw)
    model, status = _plan(psf, psfhat).clark(dirty, wsums, mask, **kw)
    assert n_ref == 6 and status == 1
    _assert_model_close(model, m_ref, 1e-12)
    assert np.abs(m_copy - m_ref).max() > 1e-6 * np.abs(m_ref).max()


@pytest.mark.parametrize("extended", [False, True])
def test_clark_subminor_paths(extended):
    dirty, psf, psfhat, wsums, mask = _clark_case(8, nband=3, zero_band=None, extended=extended)
    kw = dict(gamma=0.1, pf=0.1, maxit=4 if extended else 20, subpf=0.5 if extended else 0.3, submaxit=300)
    m_ref, _, k_ref, s_ref, n_ref = ref.clark(dirty, psf, psfhat, wsums, mask, **kw)
    plan = _plan(psf, psfhat)
    model, status = plan.clark(dirty, wsums, mask, **kw)
    info = plan.info
    assert (info["iters"], info["minor_iters"], status) == (k_ref, n_ref, s_ref)
    _assert_model_close(model, m_ref, 1e-10)
    if extended:
        assert info["nsub_grid"] > 0
    else:
        assert info["nsub_lds"] > 0


def test_clark_end_to_end_with_products():
    """Point sources through this package's imaging chain: image_data_products_arrays -> clark -> compute_residual_arrays."""
    from pfb_imaging_amd import deconv
    from pfb_imaging_amd.operators.gridder import compute_residual_arrays, image_data_products_arrays, wgridder_conventions
    from pfb_imaging_amd.utils import synth
    from pfb_imaging_amd.wgridder import Gridder

    n = 256
    c = synth.make_case(nrow=6000, nchan=2, npix=n, seed=4)
    sources = [(70, 90, 1.0), (150, 200, 0.6), (200, 60, 0.8)]
    sky = np.zeros((n, n))
    for i, j, f in sources:
        sky[i, j] = f
    flip_u, flip_v, flip_w, _, _ = wgridder_conventions(0.0, 0.0)
    g = Gridder(c["uvw"], c["freq"], np.ones_like(c["mask"]), npix_x=n, npix_y=n, pixsize_x=c["cell"], pixsize_y=c["cell"],
                center_x=0.0, center_y=0.0, epsilon=1e-8, flip_u=flip_u, flip_v=flip_v, flip_w=flip_w, do_wgridding=True,
                divide_by_n=False)
    vis = g.dirty2vis(sky)
    g.close()
    nband = 1
    prod, _ = image_data_products_arrays(c["uvw"], c["freq"], vis[None], c["wgt"][None], c["mask"], n, n, 2 * n, 2 * n,
                                         c["cell"], c["cell"], do_residual=False)
    wsum = prod["WSUM"].sum()
    dirty, psf, psfhat = prod["DIRTY"] / wsum, prod["PSF"] / wsum, prod["PSFHAT"] / wsum
    pf = 0.05
    model, status = deconv.clark(dirty, psf, psfhat, prod["WSUM"] / wsum, np.ones((n, n)), gamma=0.1, pf=pf, maxit=50,
                                 verbosity=0)
    assert status == 0
    comps = set(zip(*np.nonzero(model[0])))
    assert {(i, j) for i, j, _ in sources} <= comps
    flux = {(i, j): model[0, i, j] for i, j, _ in sources}
    assert sum(flux.values()) >= 0.8 * model.sum()
    resid = compute_residual_arrays(prod["DIRTY"], model, c["uvw"], c["freq"], prod["WEIGHT"], c["mask"],
                                    np.ones((nband, n, n)), c["cell"]) / wsum
    # the minor cycle subtracts with the PSF (an approximation of the exact residual): allow for its error
    approx = np.abs(ref.psf_convolve_cube(model, psfhat, 2 * n)[0] - (dirty[0] - resid[0])).max()
    assert np.abs(resid).max() <= pf * np.abs(dirty).max() + approx + 1e-9
