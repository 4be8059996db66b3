"""The fused Hessian apply of one-plane coloured plans (k_hess_wd, csrc/gridder_kernels_wd.hpp) against the gather / scatter
pair it replaces (PFBHIP_WD_FUSED=0).  Both compute the same sums in a different order, so they agree to rounding: the
image-side correction amplifies the reordering to a few 1e-12 relative (2.7e-12 seen at W = 15), hence 2e-11."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pfb_imaging_amd.utils import synth  # noqa: E402


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def plan(c, npix, cell, eps, force=None):
    from pfb_imaging_amd.wgridder import Gridder

    g = Gridder(c["uvw"], c["freq"], c["mask"], npix_x=npix, npix_y=npix, pixsize_x=cell, pixsize_y=cell, center_x=0.0,
                center_y=0.0, epsilon=eps, flip_u=False, flip_v=True, flip_w=False, do_wgridding=True, divide_by_n=False,
                force_wmode=2, force=force)
    assert g.info["wmode"] == 2 and g.info["nplanes"] == 1, g.info
    g.set_weights(c["wgt"])
    return g


def applies(g, c, x):
    """hessian with and without beam / eta / wsum, residual_dev, then a plain dirty2vis, vis2dirty and hessian on the same plan
    (nothing of a Hessian apply may carry over into the next call); and the number of gather launches the first one made"""
    from pfb_imaging_amd._lib import DeviceArray

    beam = 0.5 + np.random.default_rng(3).random(x.shape)
    g.profile(True)
    g.profile_get(reset=True)
    h0 = g.hessian(x)
    gathers = g.profile_get(reset=True)["degrid"][1]
    g.profile(False)
    h1 = g.hessian(x, beam=beam, eta=0.3, wsum=7.0)
    h2 = g.hessian(x, wsum=2.5)
    acc = np.random.default_rng(4).standard_normal(x.shape)
    m_d, a_d, b_d = DeviceArray.from_host(x), DeviceArray.from_host(acc), DeviceArray.from_host(beam)
    o_d = DeviceArray(x.shape, np.float64)
    g.residual_dev(m_d, a_d, o_d, beam_dev=b_d)
    r = o_d.download()
    for d in (m_d, a_d, b_d, o_d):
        d.free()
    v = g.dirty2vis(x)
    d = g.vis2dirty(v, c["wgt"])
    h3 = g.hessian(x)
    return (h0, h1, h2, r, v, d, h3), gathers


def fused_vs_pair(c, npix, cell, eps, monkeypatch, force=None, tol=2e-11):
    x = np.ascontiguousarray(c["x"][:npix, :npix])
    monkeypatch.setenv("PFBHIP_WD_COLOURS", "1")
    g = plan(c, npix, cell, eps, force)
    info = dict(g.info)
    got, gathers = applies(g, c, x)
    g.close()
    monkeypatch.setenv("PFBHIP_WD_FUSED", "0")
    g = plan(c, npix, cell, eps, force)
    ref, gathers0 = applies(g, c, x)
    g.close()
    assert gathers0 > 0
    # fused on coloured plans (four launches; a grid of whole tile pairs) where the frame fits a 16-lane row
    # (W + block edge - 1 <= 16), the pair elsewhere
    fits = info["scatter_launches"] == 4 and info["W"] + info["scatter_block"] - 1 <= 16
    assert (gathers == 0) == fits, (info, gathers)
    for a, b in zip(got, ref):
        assert rel(a, b) < tol, rel(a, b)
    return info


@pytest.mark.parametrize("W, sigma", [(13, 1.5), (14, 1.5), (15, 1.25), (16, 1.25)])  # (grids of 768 / 640: whole tile pairs)
@pytest.mark.parametrize("block", ["auto", "4"])
def test_fused_hessian_supports_and_anchorings(W, sigma, block, monkeypatch):
    c = synth.make_case(60000, 2, 512, zscale=1e-3, seed=11)
    if block == "4":
        monkeypatch.setenv("PFBHIP_WD_BLOCK", "4")
    info = fused_vs_pair(c, 512, c["cell"] * 16.0, 1e-7, monkeypatch, force=(sigma, W))
    assert info["W"] == W and info["scatter_launches"] == 4, info


@pytest.mark.parametrize("K, widen, eps", [(2, 10.0, 1e-4), (3, 16.0, 1e-7), (4, 30.0, 1e-7)])
def test_fused_hessian_term_counts(K, widen, eps, monkeypatch):
    c = synth.make_case(60000, 2, 512, zscale=1e-3, seed=5)
    info = fused_vs_pair(c, 512, c["cell"] * widen, eps, monkeypatch, force=(1.5, 13))  # (a 768 grid: coloured)
    assert info["nderiv"] == K and info["scatter_launches"] == 4, info


def test_fused_hessian_dense_tiles(monkeypatch):
    """few, crowded tiles: a tile's visibilities span several work items of one colour launch (shared, atomic flush)"""
    c = synth.make_case(200000, 2, 256, zscale=1e-3, seed=9)
    cell = c["cell"] * 2.0
    monkeypatch.setenv("PFBHIP_WD_COLOURS", "1")
    g = plan(c, 256, cell, 1e-7)
    bm, nu, nv = g.binmap(), g.info["nu"], g.info["nv"]
    g.close()
    # visibilities per 32 x 32-cell tile (of the first-tap cell); the scatter's colour lists cut a tile's run into items of at
    # most 2048 visibilities and flag every part shared (pad = 1), so a tile of more than 2048 has shared items
    on = c["mask"].ravel() != 0
    tiles = (np.mod(bm["iu0"][on], nu) // 32) * (nv // 32 + 1) + np.mod(bm["iv0"][on], nv) // 32
    assert np.bincount(tiles).max() > 2 * 2048
    info = fused_vs_pair(c, 256, cell, 1e-7, monkeypatch)
    assert info["scatter_launches"] == 4, info


def test_small_plan_keeps_the_pair(monkeypatch):
    """a plan of few work items (one scatter launch, atomic flush) runs the gather / scatter pair whatever the switch says"""
    c = synth.make_case(2500, 2, 64, zscale=1e-3, seed=5)
    x = np.ascontiguousarray(c["x"][:, :64])
    g = plan(c, 64, c["cell"] * 130.0, 1e-7)
    assert g.info["scatter_launches"] == 1
    got, gathers = applies(g, c, x)
    g.close()
    monkeypatch.setenv("PFBHIP_WD_FUSED", "0")
    g = plan(c, 64, c["cell"] * 130.0, 1e-7)
    ref, _ = applies(g, c, x)
    g.close()
    assert gathers > 0
    for a, b in zip(got, ref):  # (same kernels; the atomic flushes add in no fixed order)
        assert rel(a, b) < 1e-12
