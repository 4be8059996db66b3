"""The device-resident visibility chunk (pfb_imaging_amd.vischunk, csrc/vischunk.hip, the ``*_rows_dev`` entries of
csrc/gridder.hip) against the uploading path it stands beside: ``Gridder.vis2dirty`` / ``dirty2vis`` / ``set_weights``,
``utils.weighting.imaging_weights`` and ``image_data_products_arrays``, which this package's parent commit already had.

Shape.  Unless a test says otherwise: ``synth.make_case(3000, 2, 40, zscale=0.2, seed=11)`` with ``cell *= 30``, the ``case()`` of
tests/test_gpu_callables.py: 6000 samples (no multiple of 256, 24 blocks), 5 % flagged, both Hermitian halves, several
w-planes.  ``ncorr = 2`` with ``vis = [v, conj v]`` and ``wgt = [w, 1]``.

Tolerances (``rel`` is the relative l2 difference; u = 2^-53):
  * 1e-11 between two runs of the same arithmetic on the device: the scatter's LDS atomics reorder sums from run to run at
    about 1e-13 (tests/test_gpu_gridder.py uses the same bound for the same reason);
  * 1e-10 where another rounding enters in front of the same arithmetic (weights that differ in their last bits);
  * 1e-7 against the direct DFT: the plans' ``epsilon``;
  * sums of n positive terms, in any order, differ from the exact sum by at most n u relatively (every partial sum is an
    exact sum rounded once, errors (1 + u)^(n - 1) - 1 at worst), so two such sums differ by at most 2 n u; the tests hold the
    device to n u against numpy, half of that;
  * l2-reweighted weights: ovar carries n u on either side, (dof + 2) / (dof + q) has sensitivity q / (dof + q) < 1 to it, plus a
    handful of roundings: 4 n u element-wise.
"""

import numpy as np
import pytest

from oracle import dft
from pfb_imaging_amd.utils import synth
from tests import _vischunk_ref as ref
from tests._vischunk_ref import rel

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CONV = dict(flip_u=False, flip_v=True, flip_w=False)


@pytest.fixture(scope="module")
def c():
    """The shared case; nothing writes to it."""
    c = synth.make_case(3000, 2, 40, zscale=0.2, seed=11)
    c["cell"] *= 30.0
    c["vis2"] = np.stack([c["vis"], c["vis"].conj()])
    c["wgt2"] = np.stack([c["wgt"], np.ones_like(c["wgt"])])
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def plan(c, nx, ny, l0=0.0, m0=0.0, mask="case"):
    from pfb_imaging_amd.wgridder import Gridder

    return Gridder(c["uvw"], c["freq"], c["mask"] if isinstance(mask, str) else mask, npix_x=nx, npix_y=ny, pixsize_x=c["cell"],
                   pixsize_y=c["cell"], center_x=-l0, center_y=-m0, epsilon=1e-7, do_wgridding=True, divide_by_n=False, sigma_min=1.1,
                   sigma_max=3.0, **CONV)


def chunk_of(c, vis=None, wgt=None, mask=None):
    from pfb_imaging_amd.vischunk import VisChunk

    return VisChunk(c["uvw"], c["freq"], c["vis2"] if vis is None else vis, c["wgt2"] if wgt is None else wgt,
                    c["mask"] if mask is None else mask)


def dev_image(nx, ny):
    from pfb_imaging_amd._lib import DeviceArray

    return DeviceArray((nx, ny), np.float64)


# ---- 1. row entries against the uploading entries ------------------------------------------------------------------------

def test_vis2dirty_rows_dev_equals_the_uploading_entry_and_the_dft(c):
    nx = ny = 40
    with chunk_of(c) as ch:
        g, img = plan(c, nx, ny), dev_image(nx, ny)
        try:
            for k in range(2):
                off = ch.corr_offset(k)
                for weighted in (True, False):
                    g.vis2dirty_rows_dev(ch.vis, ch.wgt if weighted else None, img, vis_offset=off, wgt_offset=off)
                    got = img.download()
                    want = g.vis2dirty(c["vis2"][k], c["wgt2"][k] if weighted else None)
                    r = rel(got, want)
                    print(f"corr {k} weighted={weighted}: rows vs upload {r:.3e}")
                    assert r < 1e-11
                    if weighted:
                        d = dft.dft_vis2dirty(c["uvw"], c["freq"], c["vis2"][k], c["wgt2"][k], c["mask"], nx, ny, c["cell"], c["cell"],
                                              0.0, 0.0, False, True, False, True, False)
                        print(f"corr {k}: rows vs DFT {rel(got, d):.3e}")
                        assert rel(got, d) < 1e-7
        finally:
            g.close()
            img.free()


def test_set_weights_dev_then_hessian_equals_set_weights_then_hessian(c):
    nx = ny = 40
    x = c["x"][:nx, :ny]
    with chunk_of(c) as ch:
        g = plan(c, nx, ny)
        try:
            for k in range(2):
                g.set_weights(c["wgt2"][k])
                want = g.hessian(x)
                g.set_weights_dev(ch.wgt, wgt_offset=ch.corr_offset(k))
                got = g.hessian(x)
                print(f"corr {k}: hessian after set_weights_dev vs set_weights {rel(got, want):.3e}")
                assert rel(got, want) < 1e-11
            g.set_weights(None)
            want = g.hessian(x)
            g.set_weights_dev(None)
            assert rel(g.hessian(x), want) < 1e-11
        finally:
            g.close()


def test_a_fully_flagged_chunk_gives_a_zero_image_and_zero_wsum(c):
    nx = ny = 40
    none = np.zeros_like(c["mask"])
    with chunk_of(c, mask=none) as ch:
        g, img = plan(c, nx, ny, mask=none), dev_image(nx, ny)
        try:
            img.upload(np.ones((nx, ny)))
            g.vis2dirty_rows_dev(ch.vis, ch.wgt, img)
            assert not img.download().any()
            assert np.array_equal(ch.wsum(), np.zeros(2))
        finally:
            g.close()
            img.free()


# ---- 2. PSF ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l0,m0", [(0.0, 0.0), (0.002, -0.001)])
def test_psf_rows_dev_equals_gridding_psf_visibilities(c, l0, m0):
    """The PSF whose visibilities are formed in the sort kernel == vis2dirty(psf_visibilities(...), wgt) on the same plan.

    At the phase centre the PSF peaks at [nx, ny] with the value wsum (the identity test_image_data_products_arrays checks).
    Away from it the identity does not hold for EITHER path: psf_visibilities' ramp and the plan's own centre shift have the
    same sign, so they add and the response moves off the centre pixel (the direct DFT of the same visibilities puts 26.6 at
    [nx, ny] of this case for wsum = 9240.0).  There the test holds the new path to the uploading path's centre value."""
    from pfb_imaging_amd.operators.gridder import psf_visibilities, wgridder_conventions

    nx = ny = 40
    fu, fv, fw, x0, y0 = wgridder_conventions(l0, m0)
    with chunk_of(c) as ch:
        g, img = plan(c, 2 * nx, 2 * ny, l0, m0), dev_image(2 * nx, 2 * ny)
        try:
            pv = psf_visibilities(c["uvw"], c["freq"], x0, y0, fu, fv)
            wsum = ch.wsum()
            for k in range(2):
                g.psf_rows_dev(ch.wgt, img, wgt_offset=ch.corr_offset(k))
                got = img.download()
                want = g.vis2dirty(pv, c["wgt2"][k])
                print(f"l0={l0} m0={m0} corr {k}: psf rows vs upload {rel(got, want):.3e}; centre {got[nx, ny]:.6f}, upload "
                      f"{want[nx, ny]:.6f}, wsum {wsum[k]:.6f}")
                assert rel(got, want) < 1e-11
                if l0 == 0.0 and m0 == 0.0:
                    assert abs(got[nx, ny] - wsum[k]) < 1e-6 * wsum[k]
                else:
                    assert abs(got[nx, ny] - want[nx, ny]) < 1e-6 * wsum[k]
            g.psf_rows_dev(None, img)  # unit weights
            assert rel(img.download(), g.vis2dirty(pv, None)) < 1e-11
        finally:
            g.close()
            img.free()


# ---- 3. dirty2vis_rows_dev -----------------------------------------------------------------------------------------------

def test_dirty2vis_rows_dev_plain_subtracting_and_in_place(c):
    from pfb_imaging_amd._lib import DeviceArray

    nx = ny = 40
    x = np.ascontiguousarray(c["x"][:nx, :ny])
    live = c["mask"] != 0
    with chunk_of(c) as ch:
        g, img = plan(c, nx, ny), DeviceArray.from_host(x)
        out = DeviceArray(ch.vis.shape, np.complex128)
        try:
            want = g.dirty2vis(x)
            out.upload(np.full(ch.vis.shape, 7.0 + 7.0j))  # (no sample may keep what was there)
            for k in range(2):
                g.dirty2vis_rows_dev(img, out, vis_offset=ch.corr_offset(k))
            got = out.download()
            for k in range(2):
                print(f"corr {k}: dirty2vis rows vs upload {rel(got[k], want):.3e}")
                assert rel(got[k], want) < 1e-11
                assert not got[k][~live].any()
            # vis - R dirty into a second array, then in place over the chunk's own visibilities
            for k in range(2):
                off = ch.corr_offset(k)
                g.dirty2vis_rows_dev(img, out, minuend_dev=ch.vis, vis_offset=off, minuend_offset=off)
            sub = out.download()
            for k in range(2):
                off = ch.corr_offset(k)
                g.dirty2vis_rows_dev(img, ch.vis, minuend_dev=ch.vis, vis_offset=off, minuend_offset=off)
            inplace = ch.vis.download()
            for name, got in (("separate", sub), ("in place", inplace)):
                for k in range(2):
                    r = rel(got[k][live], (c["vis2"][k] - want)[live])
                    print(f"corr {k} {name}: vis - dirty2vis {r:.3e}")
                    assert r < 1e-11
                    assert np.array_equal(got[k][~live], c["vis2"][k][~live])
        finally:
            g.close()
            img.free()
            out.free()


# ---- 4. wsum -------------------------------------------------------------------------------------------------------------------

# 262 145 = 1024 blocks x 256 threads + 1: the first size at which a first-stage thread takes a second grid-stride step
@pytest.mark.parametrize("nvis", [1, 255, 256, 257, 6000, 262145])
def test_wsum_sizes_bound_and_reproducibility(nvis):
    from pfb_imaging_amd.vischunk import VisChunk

    rng = np.random.default_rng(nvis)
    wgt = np.exp(rng.standard_normal((2, nvis, 1)))
    mask = (rng.random((nvis, 1)) > 0.05).astype(np.uint8)
    mask[nvis // 2] = 1
    with VisChunk(np.zeros((nvis, 3)), np.ones(1), np.zeros((2, nvis, 1), dtype=np.complex128), wgt, mask) as ch:
        got, again = ch.wsum(), ch.wsum()
    want = wgt[:, mask != 0].sum(-1)
    n = int((mask != 0).sum())
    err = np.abs(got - want) / want
    print(f"nvis={nvis}: wsum relative error {err.max():.3e}, bound {n * U:.3e}")
    assert (err <= n * U).all()
    assert got.tobytes() == again.tobytes()


# ---- 5. l2 reweighting -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def l2_inputs(c):
    rng = np.random.default_rng(5)
    res = np.array(c["vis2"])
    res[1] *= 100.0  # a variance taken jointly over the correlations fails by orders of magnitude
    wgtp = rng.uniform(0.5, 2.0, res.shape)
    res.setflags(write=False)
    wgtp.setflags(write=False)
    return res, wgtp


@pytest.mark.parametrize("wgtp_kind", ["scalar", "array"])
def test_l2_reweight_equals_the_restated_reference(c, l2_inputs, wgtp_kind):
    from pfb_imaging_amd._lib import DeviceArray

    res, wgtp_arr = l2_inputs
    wgtp = 1.0 if wgtp_kind == "scalar" else wgtp_arr
    live = c["mask"] != 0
    n = int(live.sum())
    want, want_ovar = ref.l2_reweight(res, c["wgt2"], c["mask"], 5, wgtp)
    with chunk_of(c) as ch:
        res_dev = DeviceArray.from_host(res)
        try:
            ovar = ch.l2_reweight(res_dev, 5, wgtp)
            got = ch.weights()
        finally:
            res_dev.free()
    eo = np.abs(ovar - want_ovar) / want_ovar
    ew = (np.abs(got - want) / want)[:, live]
    print(f"{wgtp_kind}: ovar {ovar} error {eo.max():.3e} (bound {n * U:.3e}); weights error {ew.max():.3e} (bound {4 * n * U:.3e})")
    assert (eo <= n * U).all()
    assert (ew <= 4 * n * U).all()
    assert want_ovar[1] > 1e3 * want_ovar[0]


def test_l2_reweight_of_a_zero_residual_raises_and_leaves_the_weights(c):
    from pfb_imaging_amd._lib import DeviceArray

    with chunk_of(c) as ch:
        res_dev = DeviceArray(ch.vis.shape, np.complex128)
        try:
            res_dev.zero()
            with pytest.raises(ValueError, match="zero residual variance"):
                ch.l2_reweight(res_dev, 5)
            assert ch.weights().tobytes() == c["wgt2"].tobytes()
        finally:
            res_dev.free()


# ---- 6. imaging weights ----------------------------------------------------------------------------------------------------

def test_imaging_weights_on_the_chunk_equal_the_uploading_pipeline():
    from pfb_imaging_amd.utils.weighting import imaging_weights
    from pfb_imaging_amd.vischunk import VisChunk

    w = synth.make_case(6000, 3, 96, seed=4)
    rng = np.random.default_rng(0)
    wgt0 = np.exp(rng.standard_normal((2,) + w["mask"].shape))
    vis0 = np.zeros(wgt0.shape, dtype=np.complex128)
    nxp = nyp = 164
    for robust, level, sup in ((0.0, 5.0, 0), (-1.0, 10.0, 2), (-3.0, 0.0, 1)):
        want, wcounts = imaging_weights(w["uvw"], w["freq"], w["mask"], wgt0.copy(), nxp, nyp, w["cell"], w["cell"], robust,
                                        filter_level=level, npix_super=sup, usign=-1.0, vsign=1.0, return_counts=True)
        with VisChunk(w["uvw"], w["freq"], vis0, wgt0, w["mask"]) as ch:
            counts = ch.imaging_weights(nxp, nyp, w["cell"], w["cell"], robust, filter_level=level, npix_super=sup, usign=-1.0,
                                        vsign=1.0, return_counts=True)
            got = ch.weights()
        np.testing.assert_allclose(got, want, rtol=1e-11)
        np.testing.assert_allclose(counts, wcounts, rtol=1e-11)
    with VisChunk(w["uvw"], w["freq"], vis0, wgt0, np.zeros_like(w["mask"])) as ch:
        assert ch.imaging_weights(nxp, nyp, w["cell"], w["cell"], 0.0, usign=-1.0, vsign=1.0) is None
        assert ch.weights().tobytes() == wgt0.tobytes()


# ---- 7. the chain ----------------------------------------------------------------------------------------------------------

def chain_args(c):
    nx = ny = 40
    return (nx, ny, 2 * nx, 2 * ny, c["cell"], c["cell"])


def test_chain_natural_weights_no_model(c):
    from pfb_imaging_amd.operators.gridder import image_data_products_arrays, image_data_products_chunk

    args = chain_args(c)
    n = int((c["mask"] != 0).sum())
    want, wout = image_data_products_arrays(c["uvw"], c["freq"], c["vis2"], c["wgt2"], c["mask"], *args, do_beam=True, do_psfpars=True)
    with chunk_of(c) as ch:
        got, gout = image_data_products_chunk(ch, *args, do_beam=True, do_psfpars=True)
    assert set(got) == set(want) and set(gout) == set(wout)
    for key in ("DIRTY", "PSF", "PSFHAT"):
        print(f"{key}: chunk vs arrays {rel(got[key], want[key]):.3e}")
        assert got[key].shape == want[key].shape and rel(got[key], want[key]) < 1e-11
    assert (np.abs(got["WSUM"] - want["WSUM"]) <= n * U * want["WSUM"]).all()
    assert np.array_equal(got["WEIGHT"], c["wgt2"]) and np.array_equal(got["MASK"], c["mask"]) and np.array_equal(got["UVW"], c["uvw"])
    assert (got["BEAM"] == 1).all() and got["BEAM"].shape == want["BEAM"].shape
    assert gout["residual"] is got["DIRTY"] and gout["psf"] is got["PSF"] and gout["wsum"] is got["WSUM"]
    np.testing.assert_allclose(got["PSFPARSN"], want["PSFPARSN"], rtol=1e-6)  # (the same fit of PSFs that agree to 1e-11)
    with chunk_of(c) as ch:
        with pytest.raises(ValueError, match="no model"):
            image_data_products_chunk(ch, *args, l2_reweight_dof=5)


def test_chain_with_model_briggs_and_l2_reweighting(c):
    from pfb_imaging_amd.operators.gridder import image_data_products_arrays, image_data_products_chunk

    args = chain_args(c)
    nx, ny = args[:2]
    model = np.random.default_rng(9).standard_normal((2, nx, ny))
    kw = dict(model=model, robustness=0.0, l2_reweight_dof=5)
    live = c["mask"] != 0
    want, wout = image_data_products_arrays(c["uvw"], c["freq"], c["vis2"], c["wgt2"], c["mask"], *args, **kw)
    with chunk_of(c) as ch:
        got, gout = image_data_products_chunk(ch, *args, **kw)
    assert set(got) == set(want) and set(gout) == set(wout)
    assert gout["residual"] is got["RESIDUAL"] and got["MODEL"] is model
    np.testing.assert_allclose(got["WEIGHT"][:, live], want["WEIGHT"][:, live], rtol=1e-11)
    for key in ("DIRTY", "RESIDUAL", "PSF"):
        print(f"{key}: chunk vs arrays {rel(got[key], want[key]):.3e}")
        assert rel(got[key], want[key]) < 1e-10
    for k in range(2):
        mv = dft.dft_dirty2vis(c["uvw"], c["freq"], model[k], c["cell"], c["cell"], 0.0, 0.0, False, True, False, True, False)
        d = dft.dft_vis2dirty(c["uvw"], c["freq"], mv, got["WEIGHT"][k], c["mask"], nx, ny, c["cell"], c["cell"], 0.0, 0.0, False, True,
                              False, True, False)
        r = rel(got["DIRTY"][k] - got["RESIDUAL"][k], d)
        print(f"corr {k}: DIRTY - RESIDUAL vs DFT {r:.3e}")
        assert r < 1e-7


# ---- 8. from raw correlations --------------------------------------------------------------------------------------------

def test_chain_from_raw_correlations():
    """4 correlations, linear feeds, diagonal Jones, product IQ at (38, 5): the shape tests/test_gpu_stokes.py runs that
    combination at (test_every_admitted_combination)."""
    from pfb_imaging_amd.operators.gridder import image_data_products_arrays, image_data_products_chunk
    from pfb_imaging_amd.utils.weighting import weight_data
    from pfb_imaging_amd.vischunk import VisChunk
    from tests.test_gpu_stokes import case as stokes_case

    nrow, nchan, npix = 38, 5, 32
    s = synth.make_case(nrow, nchan, npix, zscale=0.2, seed=3, with_vis=False)
    cell = s["cell"] * 4.0
    raw = stokes_case(nrow, nchan, 4, False, "random")
    flag = raw[2]
    vis, wgt = weight_data(*raw, "linear", "IQ", "4", "l2")
    mask = (~flag.any(-1)).astype(np.uint8)
    args = (npix, npix, 2 * npix, 2 * npix, cell, cell)
    want, _ = image_data_products_arrays(s["uvw"], s["freq"], np.ascontiguousarray(vis.transpose(2, 0, 1)),
                                         np.ascontiguousarray(wgt.transpose(2, 0, 1)), mask, *args)
    with VisChunk.from_weight_data(s["uvw"], s["freq"], *raw, "linear", "IQ", "4", "l2") as ch:
        assert ch.ncorr == 2 and np.array_equal(ch.mask_host, mask)
        got, _ = image_data_products_chunk(ch, *args)
    for key in ("DIRTY", "PSF"):
        print(f"{key}: chunk from raw correlations vs arrays {rel(got[key], want[key]):.3e}")
        assert rel(got[key], want[key]) < 1e-10
