"""The l1 reweighting kernels (csrc/reweight.hip): pfbhip_l21_reweight / pfbhip_l21_rms against the numpy formulas of
L21.update_weights / init_reweighting (prox/l21.py:52-88, utils/misc.py:742-755), and the device-resident ``L21.l1weight``."""

import numpy as np
import pytest

from oracle import psi as opsi
from tests._pd_ref import band_sum

pytestmark = pytest.mark.gpu

rel = lambda a, b: np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)  # noqa: E731
EPS = np.finfo(np.float64).eps


def _band(nx, ny, bases, nlevel=2):
    from pfb_imaging_amd.operators.psi import PsiBand

    return PsiBand(nx, ny, bases, nlevel)


# padded frames: (34, 26) -> 38 x 30, even (two coefficients per thread, 16-byte accesses, up to 16 bands in registers);
# (32, 48) -> 37 x 53, odd (one coefficient per thread, also the form for more than 16 bands)
@pytest.mark.parametrize("alpha", [2.0, 4.0, 3.5])
@pytest.mark.parametrize("nband,nx,ny", [(n, 34, 26) for n in range(1, 18)] + [(2, 32, 48), (5, 32, 48), (17, 32, 48)])
def test_reweight_matches_numpy(nband, nx, ny, alpha):
    from pfb_imaging_amd import prox

    bases = ("self", "db2", "db1")
    rng = np.random.default_rng(nband)
    band = _band(nx, ny, bases)
    o = opsi.Psi(nband, nx, ny, bases, 2)
    assert (o.nxmax, o.nymax) == (band.nxmax, band.nymax)
    x = rng.standard_normal((nband, nx, ny))
    if nband > 1:
        x[-1, :, : ny // 2] = -x[:-1, :, : ny // 2].sum(axis=0)  # (band sums that cancel, exactly or to rounding)
    rms = np.array([0.7, 1.3, 2.1])
    w, s = prox.l21_reweight(band, x, rms, 0.7, alpha, return_bandsum=True)
    # the coefficients themselves are the device's (pfbhip_psi_dot, tested against the oracle elsewhere): the band sum
    # and the formula are what is new here
    a = np.zeros((nband, len(bases), band.nxmax, band.nymax))
    for b in range(nband):
        band.dot(x[b], a[b])
    sref = np.sum(a, axis=0)
    # (the sum returned is the one the rms pass forms, k_l21_rms_sum; the fused kernel adds the same bands in the same
    # order in registers, and its sum is seen only through the weight below)
    assert np.array_equal(s, sref)
    ref = 1.7 / (1 + np.abs(sref) ** alpha / rms[:, None, None] ** alpha)
    assert w.shape == ref.shape
    assert np.abs(w - ref).max() <= 1e-12 * np.abs(ref).max() and rel(w, ref) < 1e-12
    assert rel(s, band_sum(o, x)) < 1e-13
    pad = sref == 0  # cells of the padded frame hold no coefficient
    assert pad.any() and np.all(w[pad] == 1.7)


def test_reweight_all_zero_basis_and_bad_rms():
    from pfb_imaging_amd import prox

    bases = ("self", "db1")
    band = _band(32, 32, bases)
    x = np.zeros((3, 32, 32))
    w = prox.l21_reweight(band, x, np.ones(2), 0.25, 2.0)
    assert np.all(w == 1.25)
    with pytest.raises(ValueError):
        prox.l21_reweight(band, x, np.array([1.0, 0.0]), 0.25, 2.0)


@pytest.mark.parametrize("nband,nx,ny", [(1, 32, 48), (3, 34, 26), (17, 64, 64)])
def test_rms_matches_numpy(nband, nx, ny):
    """Both sides sum ``count`` non-negative terms (s - mean)^2, numpy pairwise, the device per thread, per workgroup and
    then over 512 workgroups on the host.  Each order's relative error is a random walk of at most ``count`` roundings of
    eps / 2, rms <= eps sqrt(count) / 2; the two are independent (x sqrt 2), the square root halves the relative error, and
    the per-term roundings and the error of the mean (second order: the deviations sum to zero) are below that.  So the
    difference has rms <= eps sqrt(count) sqrt(2) / 4 ~ 0.35 eps sqrt(count); the bound is 4 eps sqrt(count), > 10 sigma."""
    from pfb_imaging_amd import prox

    bases = ("self", "db2", "db3")
    rng = np.random.default_rng(7 + nband)
    band = _band(nx, ny, bases)
    upd = rng.standard_normal((nband, nx, ny)) + 0.3  # (a non-zero mean: the second pass matters)
    upd[:, :4] = 0.0  # rows of exact zeros: not counted
    rms, count = prox.l21_rms(band, upd)
    a = np.zeros((nband, len(bases), band.nxmax, band.nymax))
    for b in range(nband):
        band.dot(upd[b], a[b])
    s = np.sum(a, axis=0)
    for i in range(len(bases)):
        nz = s[i][s[i] != 0]
        assert count[i] == nz.size and nz.size > 0
        err = abs(rms[i] - np.std(nz)) / np.std(nz)
        print(i, nz.size, err / (EPS * np.sqrt(nz.size)))
        assert err <= 4 * EPS * np.sqrt(nz.size)


def test_empty_basis_keeps_rms_one():
    from pfb_imaging_amd import prox
    from pfb_imaging_amd.operators.psi import PsiNocopyt
    from pfb_imaging_amd.opt import L21

    bases = ("self", "db1")
    psi = PsiNocopyt(2, 32, 32, bases, 2, 1)
    rms, count = prox.l21_rms(psi._band, np.zeros((2, 32, 32)))
    assert list(count) == [0, 0] and list(rms) == [0.0, 0.0]
    reg = L21(psi, bases)
    reg.init_reweighting(np.zeros((2, 32, 32)))
    assert reg.reweight_active and np.array_equal(reg._rms_comps, np.ones(2))


@pytest.mark.parametrize("layout", ["psi", "nocopyt"])
def test_l1weight_property(layout):
    from pfb_imaging_amd.operators.psi import Psi, PsiNocopyt
    from pfb_imaging_amd.opt import L21

    nband, nx, ny, bases = 2, 32, 48, ("self", "db2")
    rng = np.random.default_rng(4)
    psi = (Psi if layout == "psi" else PsiNocopyt)(nband, nx, ny, bases, 2, 1)
    reg = L21(psi, bases, rmsfactor=0.7, alpha=4.0)
    assert reg._wdev is None and np.array_equal(reg.l1weight, np.ones(reg.coeff_shape()[1:]))
    upd, x = rng.standard_normal((nband, nx, ny)), rng.standard_normal((nband, nx, ny))
    reg.init_reweighting(upd)
    reg.update_weights(x)
    assert reg._wdev is not None and reg._l1weight is None  # in HBM, not downloaded yet
    o = opsi.Psi(nband, nx, ny, bases, 2, transposed=layout == "psi")
    a = np.zeros((nband, 2) + reg.coeff_shape()[2:])
    o.dot(upd, a)
    s = a.sum(axis=0)
    rms = np.array([np.std(s[i][s[i] != 0]) for i in range(2)])
    o.dot(x, a)
    ref = 1.7 / (1 + np.abs(a.sum(axis=0)) ** 4 / rms[:, None, None] ** 4)
    w = reg.l1weight
    assert w is reg.l1weight  # downloaded once, cached
    assert w.shape == reg.coeff_shape()[1:] == ref.shape and w.dtype == np.float64 and w.flags.c_contiguous
    assert rel(w, ref) < 1e-12
    # a second update replaces the cached array; assignment drops the device copy
    reg.update_weights(upd)
    assert reg._l1weight is None and rel(reg.l1weight, ref) > 1e-3
    mine = 0.5 + rng.random(ref.shape)
    reg.l1weight = mine
    assert reg._wdev is None and reg.l1weight is mine
    # any array other than a lending solver's iterate is uploaded: same result from a non-contiguous view
    reg.update_weights(np.asfortranarray(x))
    assert rel(reg.l1weight, ref) < 1e-12


def test_single_process_ray_dictionary_takes_the_device_path():
    """L21 over a single-process PsiNocopytRay (what ForwardBackward's device loop accepts) reweights on the device too:
    same rms, same weights as over PsiNocopyt."""
    from pfb_imaging_amd.operators.band_worker import BandWorkerPool
    from pfb_imaging_amd.operators.psi import PsiNocopyt, PsiNocopytRay
    from pfb_imaging_amd.opt import L21

    nband, nx, ny, bases = 2, 48, 64, ("self", "db1", "db3")
    rng = np.random.default_rng(8)
    upd, x = rng.standard_normal((nband, nx, ny)), rng.standard_normal((nband, nx, ny))
    pool = BandWorkerPool(nband)
    res = []
    for psi in (PsiNocopytRay(nband, nx, ny, bases, 2, 1, workers=pool), PsiNocopyt(nband, nx, ny, bases, 2, 1)):
        reg = L21(psi, bases, rmsfactor=0.5)
        assert reg._psi_dev() is not None
        reg.init_reweighting(upd)
        reg.update_weights(x)
        assert reg._wdev is not None
        res.append((reg._rms_comps.copy(), reg.l1weight.copy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert res[0][1].shape == (len(bases), psi.nxmax, psi.nymax)
    pool.close()
