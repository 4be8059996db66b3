"""The snapshot imager on the device (pfb_imaging_amd/utils/stokes2im.py, csrc/snapshot.hip, the signed PSF entry of
csrc/gridder.hip) against the numpy restatement of the reference's ``stokes_image`` (tests/_snapshot_ref.py) over the direct DFT.

Tolerances (``rel`` is the relative l2 difference; u = 2^-53):
  * rephasing: the phase in cycles, ``w_diff * (f / c)``, carries one rounding of the quotient and one of the product on the
    device against the long-double reference: 2 P u cycles for a phase of P cycles, 4 pi P u radians; the complex products and
    the subtraction add a few ulp of |vis| + |model|: ``(4 pi P u + 8 u) (|vis| + |model|)`` element-wise, P the largest phase of
    the case (at most 500 cycles: |w_diff| <= 100 m, f <= 1.5 GHz);
  * joint reweighting: a sum of n positive terms in any order is within n u of the exact sum (tests/test_gpu_vischunk.py): ovar
    within n u of numpy's, weights within 4 n u, n = ncorr * (unmasked samples);
  * 1e-11 between two runs of the same arithmetic on the device (the scatter's LDS atomics reorder sums);
  * 1e-7 against the direct DFT: the plans' epsilon; a float32 cube adds half a float32 ulp, 2^-24; ``weight``, one pixel of such
    an image, 1e-7 |psf|_2 / peak, and ``rms`` both of these;
  * rms: the mean carries n u |mean| and enters the deviations absolutely, every deviation carries u |mean| from the subtraction
    as well, the sum of squares n u: ``4 n u (1 + |mean| / std)`` relative;
  * with a beam the compiler may fuse ``pbeam^2 + eta``, and the float32 cast sits on a rounding boundary: one float32 ulp;
  * the clean-beam parameters: 1e-12 against the fit of the same PSF planes (tests/test_gpu_cleanbeam.py's tolerance for one
    input fitted twice); the major and minor axes to 1e-5 relative against the fit of the restatement's PSF, which differs
    from the device's by the plans' epsilon 1e-7 on a smooth, well-conditioned fit (a margin of 100); the position angle to
    1e-5 rad on the same argument: the fixture's beam has an axis ratio of 0.56, so the angle is as well determined as the axes.
"""

import ctypes as ct

import numpy as np
import pytest

from tests import _dft_ref, _snapshot_ref as ref
from tests import _stokes_ref
from tests._snapshot_ref import rel

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def chunk(vis, wgt, mask, uvw=None, freq=None):
    from pfb_imaging_amd.vischunk import VisChunk

    ncorr, nrow, nchan = vis.shape
    return VisChunk(np.zeros((nrow, 3)) if uvw is None else uvw, np.ones(nchan) if freq is None else freq, vis, wgt, mask)


def random_chunk_arrays(shape, seed):
    rng = np.random.default_rng(seed)
    ncorr, nrow, nchan = shape
    vis = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    model = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    mask = (rng.random((nrow, nchan)) > 0.2).astype(np.uint8)
    mask[0, 0] = 1 if nrow * nchan == 1 else 0
    mask[-1, -1] = 1
    freq = np.sort(rng.uniform(0.9e9, 1.5e9, nchan))
    w_diff = rng.uniform(-100.0, 100.0, nrow)
    return vis, model, mask, freq, w_diff


SHAPES = [(2, 1, 1), (2, 255, 1), (2, 256, 1), (2, 257, 1), (2, 37, 5)]


# ---- 1. rephase / subtract ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("with_w,with_model", [(False, False), (True, False), (False, True), (True, True)])
def test_rephase_residual(shape, with_w, with_model):
    from pfb_imaging_amd._lib import DeviceArray

    vis, model, mask, freq, w_diff = random_chunk_arrays(shape, 17 + shape[1])
    want = ref.rephase_residual(vis, mask, freq, w_diff if with_w else None, model if with_model else None)
    P = float(np.abs(w_diff).max() * freq.max() / ref.C0) if with_w else 0.0
    assert P <= 500.4
    size = np.abs(vis) + (np.abs(model) if with_model else 0.0)
    bound = (4 * np.pi * P * U + 8 * U) * size
    with chunk(vis, np.ones(shape), mask, freq=freq) as ch:
        ch.rephase_residual(w_diff if with_w else None, model if with_model else None)
        got = ch.vis.download()
        if with_model:  # the resident form of the model gives the same bits
            ch.vis.upload(vis)
            md = DeviceArray.from_host(model)
            try:
                ch.rephase_residual(w_diff[:, None] if with_w else None, md)
            finally:
                md.free()
            assert ch.vis.download().tobytes() == got.tobytes()
    err = np.abs(got - want)
    print(f"{shape} w_diff={with_w} model={with_model}: P = {P:.1f} cycles, max |err| / bound = {(err / bound).max():.3f}, "
          f"max |err| / size = {(err / size).max():.3e}")
    assert (err <= bound).all()
    dead = mask == 0
    if with_model:
        assert not got[:, dead].any() and not np.signbit(got[:, dead].real).any() and not np.signbit(got[:, dead].imag).any()
    elif not with_w:
        assert got.tobytes() == vis.tobytes()


# ---- 2. joint reweighting ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 1, 1), (2, 257, 1), (2, 37, 5)])
def test_l2_reweight_joint(shape):
    vis, _, mask, _, _ = random_chunk_arrays(shape, 29 + shape[1])
    if shape[1] * shape[2] == 1:
        vis = np.array([[[3.0 + 4.0j]], [[1.0 - 2.0j]]])  # (squares that are exact whichever way they are formed)
    vis[1] = 100.0 * vis[0]
    live = mask != 0
    n = shape[0] * int(live.sum())
    want, want_ovar = ref.l2_reweight_joint(vis, mask, 5)
    per_corr = (np.abs(vis) ** 2 * mask[None]).sum(axis=(1, 2)) / mask.sum()
    assert per_corr[1] > 1e3 * per_corr[0] and want_ovar > 1e3 * per_corr[0]  # a per-correlation variance fails by orders of magnitude
    wgt0 = np.random.default_rng(3).uniform(0.5, 2.0, shape)
    with chunk(vis, wgt0, mask) as ch:
        ovar = ch.l2_reweight_joint(5)
        got = ch.weights()
        ch.wgt.upload(wgt0)
        again = ch.l2_reweight_joint(5)
        assert again == ovar and ch.weights().tobytes() == got.tobytes()
    eo = abs(ovar - want_ovar) / want_ovar
    ew = (np.abs(got - want) / want).max()
    print(f"{shape}: ovar {ovar} error {eo:.3e} (bound {n * U:.3e}); weights error {ew:.3e} (bound {4 * n * U:.3e})")
    assert eo <= n * U
    assert ew <= 4 * n * U
    np.testing.assert_array_equal(want[:, ~live], (5 + 1) / 5 / want_ovar)


def test_l2_reweight_joint_refusals_leave_the_weights():
    shape = (2, 37, 5)
    vis, _, mask, _, _ = random_chunk_arrays(shape, 31)
    wgt0 = np.random.default_rng(4).uniform(0.5, 2.0, shape)
    with chunk(np.zeros(shape, dtype=complex), wgt0, mask) as ch:
        with pytest.raises(ValueError, match="exactly zero"):
            ch.l2_reweight_joint(5)
        assert ch.weights().tobytes() == wgt0.tobytes()
    with chunk(vis, wgt0, np.zeros_like(mask)) as ch:
        with pytest.raises(ValueError, match="mask is empty"):
            ch.l2_reweight_joint(5)
        assert ch.weights().tobytes() == wgt0.tobytes()
    from pfb_imaging_amd._lib import check, f64, i64, lib

    with chunk(vis, wgt0, mask) as ch:  # the entry itself refuses a dof that is not positive
        for dof in (0.0, -2.0, float("nan")):
            with pytest.raises(ValueError, match="dof"):
                check(lib().pfbhip_chunk_l2_reweight_joint_dev(ch.vis.ptr, ch.mask.ptr, ch.wgt.ptr, i64(2), i64(ch.nvis), f64(dof), None))
        assert ch.weights().tobytes() == wgt0.tobytes()


# ---- 3. the signed PSF ramp --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def psf_case():
    from pfb_imaging_amd.utils import synth

    c = synth.make_case(300, 4, 128, zscale=0.2, seed=21, with_vis=False)
    c["cell"] *= 4.0
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def psf_plan(c, x0, y0, mask=None):
    from pfb_imaging_amd.wgridder import Gridder

    return Gridder(c["uvw"], c["freq"], c["mask"] if mask is None else mask, npix_x=128, npix_y=128, pixsize_x=c["cell"], pixsize_y=c["cell"], center_x=x0,
                   center_y=y0, epsilon=1e-7, flip_u=False, flip_v=True, flip_w=False, do_wgridding=True, divide_by_n=True, sigma_min=1.7)


def test_signed_psf_ramp(psf_case):
    from pfb_imaging_amd._lib import DeviceArray, check, lib
    from pfb_imaging_amd.operators.gridder import psf_visibilities

    c = psf_case
    x0, y0 = 0.002, -0.001
    wgt = DeviceArray.from_host(c["wgt"])
    img = DeviceArray((128, 128), np.float64)
    g, g0 = psf_plan(c, x0, y0), psf_plan(c, 0.0, 0.0)
    try:
        pv = psf_visibilities(c["uvw"], c["freq"], x0, y0, False, True)
        g.psf_rows_dev(wgt, img, ramp_sign=-1.0)
        minus = img.download()
        want = g.vis2dirty(pv.conj(), c["wgt"])
        print(f"ramp_sign=-1 vs vis2dirty of the conjugated ramp: {rel(minus, want):.3e}; peak at "
              f"{np.unravel_index(minus.argmax(), minus.shape)}, {minus.max():.6f} of wsum {c['wgt'][c['mask'] != 0].sum():.6f}")
        assert rel(minus, want) < 1e-11
        assert np.unravel_index(minus.argmax(), minus.shape) == (64, 64)  # the conjugate ramp cancels the plan's shift
        # ramp_sign = +1 is the existing entry: the same kernel with the same arguments (x0 * 1.0 is x0).  Two runs of the
        # existing entry already differ in their last bits on this case (the scatter's LDS atomics add in the order the waves
        # arrive: 6e-16 measured between two calls of pfbhip_gridder_psf_rows_dev), so bit-identity of the images can be asked
        # only where no two visibilities meet in a cell -- the one-sample plans below -- and here the bound is that of two runs
        # of the same arithmetic.
        g.psf_rows_dev(wgt, img, ramp_sign=1.0)
        plus = img.download()
        check(lib().pfbhip_gridder_psf_rows_dev(g._h, wgt.ptr, img.ptr))
        old = img.download()
        check(lib().pfbhip_gridder_psf_rows_dev(g._h, wgt.ptr, img.ptr))
        old2 = img.download()
        print(f"ramp_sign=+1 vs the existing entry: {rel(plus, old):.3e} (the existing entry against itself: {rel(old2, old):.3e}, "
              f"bit-identical: {old2.tobytes() == old.tobytes()})")
        assert rel(plus, old) < 1e-11 and rel(old2, old) < 1e-11
        assert rel(plus, g.vis2dirty(pv, c["wgt"])) < 1e-11
        g0.psf_rows_dev(wgt, img, ramp_sign=-1.0)
        a = img.download()
        g0.psf_rows_dev(wgt, img, ramp_sign=1.0)
        print(f"at the phase centre, -1 vs +1: {rel(a, img.download()):.3e}")
        assert rel(a, img.download()) < 1e-11
        one = np.zeros_like(c["mask"])
        one[7, 2] = 1
        # ... and a plan of several samples of which no two meet in a cell: footprints (W x W cells from the anchor the plan
        # reports) that are disjoint on the periodic grid, chosen greedily in row order
        bm, W, nu, nv = g.binmap(), g.info["W"], g.info["nu"], g.info["nv"]
        apart, kept = np.zeros_like(c["mask"]), []
        for i in np.flatnonzero(c["mask"].ravel()):
            du = np.array([abs(int(bm["iu0"][i]) - int(bm["iu0"][k])) for k in kept])
            dv = np.array([abs(int(bm["iv0"][i]) - int(bm["iv0"][k])) for k in kept])
            if not kept or (np.maximum(np.minimum(du, nu - du), np.minimum(dv, nv - dv)) > W).all():
                kept.append(i)
        apart.ravel()[kept] = 1
        print(f"{len(kept)} samples with disjoint footprints (W = {W}, grid {nu} x {nv})")
        assert len(kept) >= 8
        for cx, cy, mk in ((x0, y0, one), (0.0, 0.0, one), (x0, y0, apart)):
            g1 = psf_plan(c, cx, cy, mk)
            try:
                g1.psf_rows_dev(wgt, img, ramp_sign=1.0)
                plus = img.download()
                check(lib().pfbhip_gridder_psf_rows_dev(g1._h, wgt.ptr, img.ptr))
                assert plus.any() and plus.tobytes() == img.download().tobytes()
                if cx == 0.0:
                    g1.psf_rows_dev(wgt, img, ramp_sign=-1.0)
                    assert plus.tobytes() == img.download().tobytes()
            finally:
                g1.close()
        with pytest.raises(ValueError, match="ramp_sign"):
            check(lib().pfbhip_gridder_psf_rows_signed_dev(g._h, wgt.ptr, ct.c_double(0.5), img.ptr))
    finally:
        g.close()
        g0.close()
        wgt.free()
        img.free()


# ---- 4. the finish -------------------------------------------------------------------------------------------------------------

FINISH_SHAPES = [((1, 2, 2), (128, 128)), ((2, 33, 65), (33, 65)), ((1, 64, 64), (128, 128)), ((4, 130, 128), (33, 65))]


def finish(residual, psf, wsum, pbeam=None, eta=1e-5, out_dtype=np.float32):
    """``(outputs, residual after, psf after)`` of one call"""
    from pfb_imaging_amd._lib import DeviceArray
    from pfb_imaging_amd.utils.stokes2im import snapshot_finish

    r, p = DeviceArray.from_host(residual), DeviceArray.from_host(psf)
    b = None if pbeam is None else DeviceArray.from_host(pbeam)
    try:
        out = snapshot_finish(r, p, wsum, b, eta, psf_out=True, out_dtype=out_dtype)
        return out, r.download(), p.download()
    finally:
        for d in (r, p, b):
            if d is not None:
                d.free()


def finish_inputs(shape, pshape, seed):
    rng = np.random.default_rng(seed)
    ns = shape[0]
    residual = rng.standard_normal(shape)
    psf = rng.uniform(-0.2, 0.9, (ns,) + pshape) * rng.uniform(1.0, 50.0, (ns, 1, 1))
    for c in range(ns):  # the peak: first element, last element, somewhere inside
        psf[c].flat[(0, psf[c].size - 1, psf[c].size // 3, 7)[c % 4] % psf[c].size] = 60.0 + c
    return residual, psf


@pytest.mark.parametrize("shape,pshape", FINISH_SHAPES)
def test_finish_without_a_beam_is_exact(shape, pshape):
    residual, psf = finish_inputs(shape, pshape, sum(shape))
    ns = shape[0]
    pm = psf.max(axis=(1, 2))
    for dtype in (np.float64, np.float32):
        out, r_after, p_after = finish(residual, psf, np.ones(ns), out_dtype=dtype)
        assert out["psf_max"].tobytes() == pm.tobytes()
        want_r, want_p = residual / pm[:, None, None], psf / pm[:, None, None]
        assert r_after.tobytes() == want_r.tobytes() and p_after.tobytes() == want_p.tobytes()
        assert out["cube"].dtype == dtype and out["cube"].shape == (ns, shape[2], shape[1])
        assert out["cube"].tobytes() == np.ascontiguousarray(np.transpose(want_r.astype(dtype), (0, 2, 1))).tobytes()
        assert out["psf"].tobytes() == np.ascontiguousarray(np.transpose(want_p.astype(dtype), (0, 2, 1))).tobytes()
        assert "beam_weight" not in out
        again, _, _ = finish(residual, psf, np.ones(ns), out_dtype=dtype)
        assert again["rms"].tobytes() == out["rms"].tobytes()


@pytest.mark.parametrize("shape,pshape", FINISH_SHAPES)
def test_finish_transposes_a_plane_that_encodes_its_own_index(shape, pshape):
    ns, nx, ny = shape
    index = np.arange(ns * nx * ny, dtype=np.float64).reshape(shape) + 1.0
    pindex = np.arange(ns * pshape[0] * pshape[1], dtype=np.float64).reshape((ns,) + pshape)
    psf = -pindex
    psf[:, -1, 0] = 2.0  # the peak: division by it is exact
    out, _, _ = finish(index, psf, np.ones(ns), out_dtype=np.float64)
    c, j, i = np.meshgrid(np.arange(ns), np.arange(ny), np.arange(nx), indexing="ij")
    assert np.array_equal(out["cube"] * 2.0, (c * nx + i) * ny + j + 1.0)
    c, j, i = np.meshgrid(np.arange(ns), np.arange(pshape[1]), np.arange(pshape[0]), indexing="ij")
    want = -((c * pshape[0] + i) * pshape[1] + j) / 2.0
    want[:, 0, -1] = 1.0
    assert np.array_equal(out["psf"], want)


@pytest.mark.parametrize("shape,pshape", FINISH_SHAPES)
def test_finish_with_a_beam(shape, pshape):
    residual, psf = finish_inputs(shape, pshape, 5 + sum(shape))
    ns = shape[0]
    pbeam = np.random.default_rng(8).uniform(0.05, 1.0, shape)
    eta = 1e-3
    out, r_after, _ = finish(residual, psf, np.ones(ns), pbeam, eta)
    pm = psf.max(axis=(1, 2))[:, None, None]
    want = (residual / pm) * (pbeam / (pbeam**2 + eta))
    wcube, wbw = np.transpose(want, (0, 2, 1)), np.transpose(pbeam**2 + eta, (0, 2, 1))
    e1 = (np.abs(out["cube"] - wcube) / np.abs(wcube)).max()
    e2 = (np.abs(out["beam_weight"] - wbw) / wbw).max()
    e3 = (np.abs(r_after - want) / np.abs(want)).max()
    print(f"{shape}: cube {e1:.3e}, beam_weight {e2:.3e} (one float32 ulp {2.0 ** -23:.3e}); float64 residual {e3:.3e}")
    assert out["cube"].dtype == np.float32 and out["beam_weight"].dtype == np.float32
    assert e1 <= 2.0 ** -23 and e2 <= 2.0 ** -23 and e3 <= 4 * U
    # the rms is that of the normalised residual BEFORE the beam (:692 precedes :708)
    for c in range(ns):
        assert abs(out["rms"][c] - ref.std(residual[c] / pm[c])) <= 4 * residual[c].size * U * 2 * out["rms"][c]


@pytest.mark.parametrize("nx,ny", [(64, 64), (33, 65)])
@pytest.mark.parametrize("ratio", [0.0, 1.0, 1.0e6])
def test_finish_rms_is_two_pass(nx, ny, ratio):
    rng = np.random.default_rng(int(nx + ratio))
    residual = rng.standard_normal((1, nx, ny)) * 3.0
    residual += ratio * residual.std() - residual.mean()
    psf = np.full((1, 128, 128), 0.5)
    psf[0, 64, 64] = 4.0
    x = residual[0] / 4.0
    want = ref.std(x)
    r = abs(float(x.astype(np.longdouble).mean())) / want
    n = nx * ny
    bound = 4 * n * U * (1 + r)
    out, _, _ = finish(residual, psf, np.ones(1))
    err = abs(out["rms"][0] - want) / want
    one_pass = float(np.sqrt(abs(np.float64((x * x).mean()) - np.float64(x.mean()) ** 2)))
    print(f"{nx} x {ny}, |mean| / std = {r:.3e}: rms error {err:.3e}, bound {bound:.3e}; a one-pass formula in float64: "
          f"{abs(one_pass - want) / want:.3e}; numpy's std {abs(float(np.std(x)) - want) / want:.3e}")
    assert err <= bound


def test_finish_leaves_a_stokes_without_weight_at_zero():
    shape, pshape = (3, 33, 65), (33, 65)
    residual, psf = finish_inputs(shape, pshape, 77)
    residual[1], psf[1] = np.nan, np.nan  # (what was never gridded may hold anything)
    out, r_after, p_after = finish(residual, psf, np.array([2.0, 0.0, 1.0]))
    keep = [0, 2]
    alone, r2, p2 = finish(residual[keep], psf[keep], np.ones(2))
    assert not out["cube"][1].any() and not out["psf"][1].any() and not r_after[1].any() and not p_after[1].any()
    assert out["psf_max"][1] == 0.0 and out["rms"][1] == 0.0
    assert out["cube"][keep].tobytes() == alone["cube"].tobytes() and out["psf"][keep].tobytes() == alone["psf"].tobytes()
    assert out["rms"][keep].tobytes() == alone["rms"].tobytes() and out["psf_max"][keep].tobytes() == alone["psf_max"].tobytes()
    # with a beam: the idle Stokes stays zero whatever its beam holds, and its beam_weight is pbeam^2 + eta all the same (:751)
    pbeam = np.random.default_rng(2).uniform(0.1, 1.0, shape)
    pbeam[1, ::2] = np.nan
    out, r_after, _ = finish(residual, psf, np.array([2.0, 0.0, 1.0]), pbeam, 1e-3)
    assert not out["cube"][1].any() and not r_after[1].any()
    want_bw = np.transpose((pbeam**2 + 1e-3).astype(np.float32), (0, 2, 1))
    assert np.array_equal(out["beam_weight"], want_bw, equal_nan=True) and np.isnan(out["beam_weight"][1]).any()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------

NANT, NTIME, NCHAN, NPIX = 12, 3, 4, 64


@pytest.fixture(scope="module")
def snap():
    """12 antennas x 3 times = 198 rows x 4 channels, linear feeds, 4 correlations, diagonal Jones -> IQ.  Nothing writes to it."""
    from pfb_imaging_amd.utils import synth
    from pfb_imaging_amd.utils.weighting import weight_data

    rng = np.random.default_rng(2024)
    p, q = np.triu_indices(NANT, 1)
    nbl = p.size
    nrow = nbl * NTIME
    s = synth.make_case(nrow, NCHAN, NPIX, zscale=0.2, seed=12, with_vis=False)
    uvw = s["uvw"] * np.array([1.0, 0.6, 1.0])  # an elliptical beam: its position angle is well conditioned
    shape = (nrow, NCHAN, 4)
    data = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    weight = rng.uniform(0.1, 2.0, shape)
    flag = rng.random(shape) < 0.03
    jones = _stokes_ref.random_jones(rng, (NTIME, NANT, NCHAN, 1), False)
    raw = (data, weight, flag, jones, np.arange(NTIME) * nbl, np.full(NTIME, nbl), np.tile(p, NTIME), np.tile(q, NTIME))
    vis, wgt = weight_data(*raw, "linear", "IQ", "4", "l2")
    out = dict(raw=raw, uvw=uvw, freq=s["freq"], cell=s["cell"] * 2.0, mask=(~flag.any(-1)).astype(np.uint8),
               vis=np.ascontiguousarray(vis.transpose(2, 0, 1)), wgt=np.ascontiguousarray(wgt.transpose(2, 0, 1)),
               time=np.repeat(np.arange(NTIME) * 8.0, nbl),
               model=rng.standard_normal((2, nrow, NCHAN)) + 1j * rng.standard_normal((2, nrow, NCHAN)),
               w_diff=rng.uniform(-30.0, 30.0, nrow))
    for a in list(out.values()) + list(raw):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def restated(s, x0=0.0, y0=0.0, robustness=None, model=None, w_diff=None, dof=None, transients=None, pbeam=None, eta=1e-5):
    """tests/_snapshot_ref.py in the reference's order; the imaging weights are the array entry's (utils.weighting.imaging_weights,
    pinned to the reference by tests/test_gpu_weighting_pins.py)."""
    from pfb_imaging_amd.utils.weighting import imaging_weights

    data, weight = np.array(s["vis"]), np.array(s["wgt"])
    if w_diff is not None or model is not None:
        data = ref.rephase_residual(data, s["mask"], s["freq"], w_diff, model)
    if dof:
        weight, _ = ref.l2_reweight_joint(data, s["mask"], dof)
    if transients is not None:
        d3 = np.ascontiguousarray(data.transpose(1, 2, 0))
        d3, _ = _dft_ref.inject(d3, transients["uvw"], s["freq"], transients["time"], transients["sources"], transients["all_times"],
                                transients["all_freqs"], w_diff=w_diff)
        data = np.ascontiguousarray(d3.transpose(2, 0, 1))
    if robustness is not None:
        weight = imaging_weights(s["uvw"], s["freq"], s["mask"], np.ascontiguousarray(weight), ref.pad_size(NPIX, 1.7), ref.pad_size(NPIX, 1.7),
                                 s["cell"], s["cell"], robustness, filter_level=5.0, npix_super=0, usign=-1.0, vsign=1.0)
    return ref.image(s["uvw"], s["freq"], data, weight, s["mask"], NPIX, NPIX, s["cell"], x0, y0, pbeam=pbeam, eta=eta)


def compare(got64, got32, want, s, label):
    """the issue's end-to-end bounds"""
    from pfb_imaging_amd.utils.misc import fitcleanbeam

    cube64 = np.transpose(got64["cube"], (0, 2, 1))
    r64, r32 = rel(cube64, want["residual64"]), rel(got32["cube"], want["cube"])
    # one pixel of an image whose l2 error is 1e-7 of its norm: the PSF peak (1 after normalisation) is off by 1e-7 |psf|_2 at
    # most; the rms is a norm of the cube divided by that peak, about its mean
    bw = 1e-7 * np.sqrt((want["psf64"] ** 2).sum(axis=(1, 2)))
    ew = np.abs(got64["weight"] - want["weight"]) / want["weight"]
    ratio = np.abs(want["residual64"].mean(axis=(1, 2))) / want["rms"]
    br = (1e-7 + bw) * np.sqrt(1 + ratio**2)
    er = np.abs(got64["rms"] - want["rms"]) / want["rms"]
    own = fitcleanbeam(np.ascontiguousarray(np.transpose(got64["psf"], (0, 2, 1))), level=0.5, pixsize=np.rad2deg(s["cell"]))
    dft_fit = fitcleanbeam(want["psf64"], level=0.5, pixsize=np.rad2deg(s["cell"]))
    gp = np.stack([got64["psf_maj"], got64["psf_min"], got64["psf_pa"] * np.pi / 180], axis=1)
    e_own = np.abs(gp - own).max()
    e_axes = (np.abs(gp[:, :2] - dft_fit[:, :2]) / dft_fit[:, :2]).max()
    dpa = np.abs(gp[:, 2] - dft_fit[:, 2]) % np.pi  # (an ellipse's angle is defined modulo pi)
    e_pa = np.minimum(dpa, np.pi - dpa).max()
    print(f"{label}: cube f64 {r64:.3e}, f32 {r32:.3e}, psf {rel(np.transpose(got64['psf'], (0, 2, 1)), want['psf64']):.3e}, weight {ew.max():.3e} "
          f"(bound {bw.min():.3e}), rms {er.max():.3e} (bound {br.min():.3e}); beam {gp[0]} vs the fit of its own PSF {e_own:.3e}, axes vs the restatement's {e_axes:.3e} "
          f"(pa {e_pa:.3e} rad)")
    assert got32["cube"].dtype == np.float32 and got32["rms"].dtype == np.float32 and got32["psf_maj"].dtype == np.float32
    assert r64 < 1e-7 and r32 < 1e-7 + 2.0 ** -24
    assert (ew <= bw).all() and (er <= br).all()
    assert e_own <= 1e-12 and e_axes < 1e-5 and e_pa < 1e-5
    assert got64["nonzero"].all() and got32["nonzero"].all()
    np.testing.assert_allclose(got32["rms"], want["rms"].astype(np.float32), rtol=2.0 ** -23 + br.max())


def run_chunk(s, **kw):
    with chunk(s["vis"], s["wgt"], s["mask"], s["uvw"], s["freq"]) as ch:
        from pfb_imaging_amd.utils.stokes2im import snapshot_image_chunk

        return snapshot_image_chunk(ch, NPIX, NPIX, s["cell"], **kw)


@pytest.mark.parametrize("robustness", [None, 0.0])
@pytest.mark.parametrize("x0,y0", [(0.0, 0.0), (0.002, -0.001)])
def test_snapshot_against_the_restatement_over_the_dft(snap, robustness, x0, y0):
    want = restated(snap, x0, y0, robustness)
    kw = dict(x0=x0, y0=y0, robustness=robustness, psf_out=True)
    got64, got32 = run_chunk(snap, out_dtype=np.float64, **kw), run_chunk(snap, **kw)
    assert set(got32) == {"cube", "psf", "weight", "rms", "nonzero", "psf_maj", "psf_min", "psf_pa", "x0", "y0"}
    assert got32["cube"].shape == (2, NPIX, NPIX) and got32["psf"].shape == (2, 128, 128) and (got32["x0"], got32["y0"]) == (x0, y0)
    compare(got64, got32, want, snap, f"robustness={robustness} centre=({x0}, {y0})")
    assert rel(got32["psf"], want["psf"]) < 1e-7 + 2.0 ** -24


def test_snapshot_with_model_rephasing_and_joint_reweighting(snap):
    kw = dict(model_vis=snap["model"], w_diff=snap["w_diff"], l2_reweight_dof=5, psf_out=True)
    want = restated(snap, model=snap["model"], w_diff=snap["w_diff"], dof=5)
    compare(run_chunk(snap, out_dtype=np.float64, **kw), run_chunk(snap, **kw), want, snap, "model, w_diff, dof=5")


def test_snapshot_with_a_transient_at_a_pixel_centre(snap):
    ix, iy = 40, 23
    src = dict(l=(ix - NPIX // 2) * snap["cell"], m=-(iy - NPIX // 2) * snap["cell"],  # (flip_v: the image's m axis is the sky's -m)
               time_profile=np.array([1.0, 1.0]), freq_profile=np.array([50.0, 50.0]))
    tr = dict(uvw=snap["uvw"], time=snap["time"], sources=[src], all_times=np.array([-1.0, 100.0]), all_freqs=np.array([1e8, 1e10]))
    want = restated(snap, transients=tr)
    kw = dict(transients=tr, psf_out=True)
    got64, got32 = run_chunk(snap, out_dtype=np.float64, **kw), run_chunk(snap, **kw)
    compare(got64, got32, want, snap, "transient")
    peak = np.unravel_index(np.abs(got32["cube"][0]).argmax(), (NPIX, NPIX))
    print(f"peak {got32['cube'][0][peak]:.4f} at (y, x) = {peak}; the restatement has {want['cube'][0][iy, ix]:.4f} there")
    assert peak == (iy, ix)  # (the cube is transposed)
    assert abs(got32["cube"][0, iy, ix] - want["cube"][0, iy, ix]) < 1e-6 * abs(want["cube"][0, iy, ix])
    assert np.abs(got32["cube"][1]).max() < 0.2 * got32["cube"][0, iy, ix]  # Stokes I only (:558)


def test_snapshot_with_a_beam_and_the_weight_grid(snap):
    pbeam = np.random.default_rng(6).uniform(0.2, 1.0, (2, NPIX, NPIX))
    want = restated(snap, robustness=0.0, pbeam=pbeam, eta=1e-3)
    got = run_chunk(snap, robustness=0.0, pbeam=pbeam, eta=1e-3, weight_grid_out=True)
    npad = ref.pad_size(NPIX, 1.7)
    print(f"beam: cube {rel(got['cube'], want['cube']):.3e}, beam_weight {rel(got['beam_weight'], want['beam_weight']):.3e}")
    assert rel(got["cube"], want["cube"]) < 1e-7 + 2.0 ** -24
    assert (np.abs(got["beam_weight"] - want["beam_weight"]) <= 2.0 ** -23 * want["beam_weight"]).all()
    assert got["wgtgrid"].shape == (2, npad, npad) and got["wgtgrid"].dtype == np.float32
    assert (got["wgtgrid"] >= 0).all() and got["wgtgrid"].any() and "psf" not in got


def test_chunk_and_array_faces_agree(snap):
    from pfb_imaging_amd.utils.stokes2im import stokes_image_arrays

    kw = dict(x0=0.002, y0=-0.001, robustness=0.0, model_vis=snap["model"], l2_reweight_dof=5, psf_out=True, out_dtype=np.float64)
    a = run_chunk(snap, **kw)
    b = stokes_image_arrays(*snap["raw"], snap["uvw"], snap["freq"], "linear", "IQ", "4", "l2", NPIX, NPIX, snap["cell"], **kw)
    assert set(a) == set(b)
    for key in ("cube", "psf", "weight", "rms"):
        print(f"{key}: chunk vs arrays {rel(a[key], b[key]):.3e}")
        assert rel(a[key], b[key]) < 1e-11
    assert np.array_equal(a["nonzero"], b["nonzero"]) and (a["x0"], a["y0"]) == (b["x0"], b["y0"])
    # The beam parameters are where a descent stops, not a sum, so the images' 1e-11 does not carry over to them.  The fit
    #  accepts a step when the objective, a float64 sum of squares, does not rise, and stops when its damped
    # step falls below 1e-12 (1 + |p|).  A minimum located by comparing rounded objective values is determined to sqrt(u) of
    # the parameter's scale at best -- a change dp moves a quadratic minimum's value by f'' dp^2 / 2, invisible below u f -- and
    # two descents on PSFs that differ in their last bits may stop anywhere in that basin.  Bound: sqrt(u) (1 + |p|) in the
    # fit's own units (pixels, pixels, radians).  Measured over four runs: 1.2e-13 to 5.5e-11 of psf_min, up to 1.8e-11 of
    # psf_maj, 4.7e-11 of psf_pa -- while the PSF planes themselves agree to 1.5e-15.
    cell_deg = np.rad2deg(snap["cell"])
    for key, unit in (("psf_maj", cell_deg), ("psf_min", cell_deg), ("psf_pa", 180 / np.pi)):
        pa, pb = a[key] / unit, b[key] / unit
        err = np.abs(pa - pb) / (1 + np.abs(pb))
        print(f"{key}: chunk vs arrays {err.max():.3e} of (1 + |p|) in the fit's units; relative {rel(a[key], b[key]):.3e}")
        assert (err <= np.sqrt(U)).all()


def test_a_stokes_without_weight_is_reported_and_leaves_the_other_alone(snap):
    wgt = np.array(snap["wgt"])
    wgt[1] = 0.0
    from pfb_imaging_amd.utils.stokes2im import snapshot_image_chunk

    with chunk(snap["vis"], wgt, snap["mask"], snap["uvw"], snap["freq"]) as ch:
        got = snapshot_image_chunk(ch, NPIX, NPIX, snap["cell"], psf_out=True, out_dtype=np.float64)
    with chunk(snap["vis"][:1], wgt[:1], snap["mask"], snap["uvw"], snap["freq"]) as ch:
        alone = snapshot_image_chunk(ch, NPIX, NPIX, snap["cell"], psf_out=True, out_dtype=np.float64)
    assert list(got["nonzero"]) == [True, False] and got["weight"][1] == 0.0 and got["rms"][1] == 0.0
    assert not got["cube"][1].any() and not got["psf"][1].any()
    assert np.isnan([got["psf_maj"][1], got["psf_min"][1], got["psf_pa"][1]]).all()
    assert rel(got["cube"][0], alone["cube"][0]) < 1e-11 and rel(got["psf"][0], alone["psf"][0]) < 1e-11
    assert abs(got["psf_maj"][0] - alone["psf_maj"][0]) < 1e-6 * alone["psf_maj"][0]


def test_a_stokes_without_weight_gets_a_zero_weight_grid(snap):
    """With imaging weights (robustness 0) the dead plane's counts are the reference's 0 / 0 (weighting.py:172-174), so its
    ``wgtgrid`` plane is zero (stokes2im.py:740-742), not ones; the live plane's is that of the one-plane chunk to 1e-6: the
    float32 cast of both sides, and the joint-median filter sees the same positives."""
    wgt = np.array(snap["wgt"])
    wgt[1] = 0.0
    from pfb_imaging_amd.utils.stokes2im import snapshot_image_chunk

    kw = dict(robustness=0.0, weight_grid_out=True, psf_out=True, out_dtype=np.float64)
    with chunk(snap["vis"], wgt, snap["mask"], snap["uvw"], snap["freq"]) as ch:
        got = snapshot_image_chunk(ch, NPIX, NPIX, snap["cell"], **kw)
    with chunk(snap["vis"][:1], wgt[:1], snap["mask"], snap["uvw"], snap["freq"]) as ch:
        alone = snapshot_image_chunk(ch, NPIX, NPIX, snap["cell"], **kw)
    npad = ref.pad_size(NPIX, 1.7)
    err = np.abs(got["wgtgrid"][0] - alone["wgtgrid"][0])
    print(f"wgtgrid: dead plane max {np.abs(got['wgtgrid'][1]).max()}, live plane vs the one-plane chunk "
          f"{(err / np.maximum(alone['wgtgrid'][0], 1e-300)).max():.3e}, {int((got['wgtgrid'][0] > 0).sum())} cells")
    assert got["wgtgrid"].shape == (2, npad, npad) and got["wgtgrid"].dtype == np.float32
    assert not got["wgtgrid"][1].any()
    assert got["wgtgrid"][0].any() and np.array_equal(got["wgtgrid"][0] > 0, alone["wgtgrid"][0] > 0)
    assert (err <= 1e-6 * alone["wgtgrid"][0]).all()
    assert list(got["nonzero"]) == [True, False] and got["weight"][1] == 0.0 and got["rms"][1] == 0.0
    assert not got["cube"][1].any() and not got["psf"][1].any()
    assert np.isnan([got["psf_maj"][1], got["psf_min"][1], got["psf_pa"][1]]).all()
    assert rel(got["cube"][0], alone["cube"][0]) < 1e-11 and rel(got["psf"][0], alone["psf"][0]) < 1e-11
    assert abs(got["psf_maj"][0] - alone["psf_maj"][0]) < 1e-6 * alone["psf_maj"][0]
