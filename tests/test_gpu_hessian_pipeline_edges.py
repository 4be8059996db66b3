"""What a deeper read pipeline in the fused Hessian kernel (k_hess_wd, csrc/gridder_kernels_wd.hpp) can get wrong and the cases of
test_gpu_hessian_fused.py do not pin.  The kernel requests the first tile rows of a row stream's NEXT record while it still
works on the current one, so these plans have

* work items with fewer visibilities than the 16 row streams of a workgroup (streams that are empty or hold one record: the
  look-ahead then reads a clamped record of a neighbouring stream, and its weight must stay out of the sums),
* a last work item that ends on the last record of the plan (the look-ahead past the end), and
* footprints in the last rows and columns of a tile's 48 x 48 LDS image (first tap on local cell 31: rows / columns 31 .. 31 + W - 1),

for the widest supports of both block edges (W = 13: 4 cells; W = 14, 15: 2 cells) and K = 2 .. 4 terms.  As in
test_gpu_hessian_fused.py the plans are forced onto the coloured path (PFBHIP_WD_COLOURS=1) and compared with the gather /
scatter pair (PFBHIP_WD_FUSED=0), which computes the same sums in another order, at that file's 2e-11."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pfb_imaging_amd.utils import synth  # noqa: E402

TOL = 2e-11
SUPPORTS = [(13, 1.5), (14, 1.5), (15, 1.25)]  # (oversampled grids of 768 / 640 cells: whole tile pairs)
TERMS = [(2, 10.0, 1e-4), (3, 16.0, 1e-7), (4, 30.0, 1e-7)]  # K, field widening, epsilon (as test_fused_hessian_term_counts)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def plan(c, npix, cell, eps, force):
    from pfb_imaging_amd.wgridder import Gridder

    g = Gridder(c["uvw"], c["freq"], c["mask"], npix_x=npix, npix_y=npix, pixsize_x=cell, pixsize_y=cell, center_x=0.0,
                center_y=0.0, epsilon=eps, flip_u=False, flip_v=True, flip_w=False, do_wgridding=True, divide_by_n=False,
                force_wmode=2, force=force)
    assert g.info["wmode"] == 2 and g.info["nplanes"] == 1, g.info
    g.set_weights(c["wgt"])
    return g


def applies(g, x):
    """two Hessian applies (the second with a beam, eta and wsum) and the number of gather launches of the first"""
    beam = 0.5 + np.random.default_rng(3).random(x.shape)
    g.profile(True)
    g.profile_get(reset=True)
    h0 = g.hessian(x)
    gathers = g.profile_get(reset=True)["degrid"][1]
    g.profile(False)
    h1 = g.hessian(x, beam=beam, eta=0.3, wsum=7.0)
    return (h0, h1), gathers


def first_taps(g, c):
    """local first-tap cell (row, column) inside its 32 x 32 tile and the tile index, per unmasked visibility"""
    bm, nu, nv = g.binmap(), g.info["nu"], g.info["nv"]
    on = c["mask"].ravel() != 0
    iu, iv = np.mod(bm["iu0"][on], nu), np.mod(bm["iv0"][on], nv)
    return iu % 32, iv % 32, (iu // 32) * (nv // 32 + 1) + iv // 32


def fused_vs_pair(c, npix, cell, eps, force, monkeypatch, check):
    x = np.ascontiguousarray(c["x"][:npix, :npix])
    monkeypatch.setenv("PFBHIP_WD_COLOURS", "1")
    g = plan(c, npix, cell, eps, force)
    info = dict(g.info)
    check(g)
    got, gathers = applies(g, x)
    g.close()
    monkeypatch.setenv("PFBHIP_WD_FUSED", "0")
    g = plan(c, npix, cell, eps, force)
    ref, gathers0 = applies(g, x)
    g.close()
    assert info["scatter_launches"] == 4 and info["W"] + info["scatter_block"] - 1 <= 16, info
    assert gathers == 0 and gathers0 > 0, (gathers, gathers0)  # the fused kernel ran, and the reference is the pair
    for a, b in zip(got, ref):
        print("fused against pair, relative l2:", rel(a, b))
        assert rel(a, b) < TOL, rel(a, b)
    return info


@pytest.mark.parametrize("K, widen, eps", TERMS)
@pytest.mark.parametrize("W, sigma", SUPPORTS)
def test_sparse_items_short_and_empty_row_streams(W, sigma, K, widen, eps, monkeypatch):
    """a few thousand visibilities over some hundred tiles: most work items hold fewer records than a workgroup has row
    streams, some hold exactly one"""
    c = synth.make_case(1500, 2, 512, zscale=1e-3, seed=21)

    def check(g):
        _, _, tiles = first_taps(g, c)
        n = np.bincount(tiles)
        n = n[n > 0]
        assert n.min() == 1, n
        assert np.count_nonzero(n < 16) > n.size // 2, n  # (16 row streams per workgroup)

    info = fused_vs_pair(c, 512, c["cell"] * widen, eps, (sigma, W), monkeypatch, check)
    assert info["W"] == W and info["nderiv"] == K, info


@pytest.mark.parametrize("K, widen, eps", TERMS)
@pytest.mark.parametrize("W, sigma", SUPPORTS)
def test_footprints_on_the_last_rows_and_columns_of_the_tile_image(W, sigma, K, widen, eps, monkeypatch):
    """crowded tiles (items of up to 2048 records, row streams of many records) with first taps on the tile's last row, last
    column and last cell: the rows requested ahead for them end at row / column 31 + W - 1 <= 45 of the 48 x 48 image"""
    c = synth.make_case(60000, 2, 512, zscale=1e-3, seed=23)

    def check(g):
        lu, lv, _ = first_taps(g, c)
        assert np.count_nonzero(lu == 31) > 100 and np.count_nonzero(lv == 31) > 100
        assert np.count_nonzero((lu == 31) & (lv == 31)) > 0

    info = fused_vs_pair(c, 512, c["cell"] * widen, eps, (sigma, W), monkeypatch, check)
    assert info["W"] == W and info["nderiv"] == K, info
