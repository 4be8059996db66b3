"""GPU tests of the component model (csrc/comps.hip, comps.py, utils/modelspec.py, operators/gridder.py comps2vis) against the
host restatement (tests/_modelspec_ref.py) with its elementwise bounds, and against the reference-run pins
(tests/golden/modelspec_pins.npz) with the bounds of tests/test_modelspec_cpu.py."""

import os
import subprocess
import sys

import numpy as np
import pytest

from . import _modelspec_ref as ref
from ._modelspec_pins import FIT_CASES, basis_of, c2v_fixture, fit_inputs, fit_outputs, pins

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_TAGS = [t for t, c in FIT_CASES.items() if c[0] is not None]


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def _lambdified(tag):
    from pfb_imaging_amd.utils.modelspec import _parse

    _, _, _, expr, params, texpr, fexpr, _ = fit_outputs(tag)
    return _parse(expr, params, texpr, fexpr)


@pytest.mark.parametrize("tag", FIT_TAGS)
def test_device_fit_against_restatement_and_reference(tag):
    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.comps import Comps
    from pfb_imaging_amd.utils.modelspec import fit_image_cube

    time, freq, image, wgt, nbt, nbf, method, sigmasq = fit_inputs(tag)
    coeffs, xi, yi, expr, params, texpr, fexpr, cond = fit_outputs(tag)
    cube = np.ascontiguousarray(image.reshape(-1, *image.shape[2:]))
    # the kernels against the restatement, same A: mask + ordered compaction exact, fit within the sum's bound
    xfit, w, hess, _ = ref.design(time, freq, wgt, nbt, nbf, method, sigmasq)
    A = ref.fit_matrix(xfit, w, hess)
    wx, wy = np.where(np.any(image, axis=(0, 1)))
    want, bound = ref.fit(cube, A, wx, wy)
    for src in (cube, _lib.DeviceArray.from_host(cube)):       # uploaded, and already in HBM
        comps = Comps.fit(src, A)
        assert comps.x_index.dtype == comps.y_index.dtype == np.int64
        assert np.array_equal(comps.x_index, wx) and np.array_equal(comps.y_index, wy)
        err = np.abs(comps.coeffs - want)
        print(f"{tag}: ncomps {comps.ncomps} fit max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound)
        comps.close()
    # the public function against the reference
    assert cond < 1e8
    got = fit_image_cube(time, freq, image, wgt=wgt, nbasist=nbt, nbasisf=nbf, method=method, sigmasq=sigmasq)
    assert np.array_equal(got[1], xi) and np.array_equal(got[2], yi)
    assert (got[3], got[4], got[5], got[6]) == (expr, params, texpr, fexpr)
    err, tol = np.abs(got[0] - coeffs).max(), 64 * cond * ref.EPS * np.abs(coeffs).max()
    print(f"{tag}: vs reference max|diff| {err:.3e} bound {tol:.3e}")
    assert err <= tol
    # the same call with the (ntime, nband, nx, ny) cube already in HBM: the same kernels on the same bytes
    dev = _lib.DeviceArray.from_host(np.ascontiguousarray(image))
    again = fit_image_cube(time, freq, dev, wgt=wgt, nbasist=nbt, nbasisf=nbf, method=method, sigmasq=sigmasq)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], xi) and np.array_equal(again[2], yi)
    assert tuple(again[3:]) == tuple(got[3:])
    dev.free()


def test_single_plane_fit_and_the_reference_quirk():
    """ntime == nband == 1: the device gives coeffs = beta (A = [[1]]); fit_image_cube raises like the reference."""
    from pfb_imaging_amd.comps import Comps
    from pfb_imaging_amd.utils.modelspec import fit_image_cube

    p = pins()
    plane = np.ascontiguousarray(p["fit_cube"][1, 2])
    comps = Comps.fit(plane[None], np.ones((1, 1)))
    wx, wy = np.where(plane)
    assert np.array_equal(comps.x_index, wx) and np.array_equal(comps.y_index, wy)
    assert np.array_equal(comps.coeffs[0], plane[wx, wy])
    assert np.array_equal(comps.render(np.ones(1)), plane)
    comps.close()
    with pytest.raises(ValueError, match="unbound"):
        fit_image_cube(p["time"][:1], p["freq"][:1], p["fit_cube"][:1, :1])
    empty = Comps.fit(np.zeros((2, 33, 17)), np.ones((3, 2)))     # no support at all
    assert empty.ncomps == 0 and empty.coeffs.shape == (3, 0) and not empty.render(np.ones(3)).any()
    empty.close()


@pytest.mark.parametrize("method", ["poly", "Legendre"])
def test_device_render_against_restatement_and_reference(method):
    from pfb_imaging_amd.comps import Comps
    from pfb_imaging_amd.utils.modelspec import eval_coeffs_to_cube

    p = pins()
    tag = f"small_{method}"
    coeffs, xi, yi, expr, params, texpr, fexpr, _ = fit_outputs(tag)
    basis = basis_of(tag)
    region = np.ones((40, 28), dtype=bool)
    region[::3] = False
    comps = Comps(40, 28, xi, yi, coeffs)
    comps.set_region(region)
    bounds = {}
    for i, t in enumerate(p["eval_time"]):
        for j, f in enumerate(p["eval_freq"]):
            b = basis(t, f)
            want, bound = ref.render(40, 28, xi, yi, coeffs, b)
            assert np.all(np.abs(comps.render(b) - want) <= bound)
            want_r, bound_r = ref.render(40, 28, xi, yi, coeffs, b, region)
            got_r = comps.render(b, region=True)
            assert np.all(np.abs(got_r - want_r) <= bound_r) and not got_r[~region].any()
            bounds[i, j] = bound
    comps.close()
    cube = eval_coeffs_to_cube(p["eval_time"], p["eval_freq"], 40, 28, coeffs, xi, yi, expr, params, texpr, fexpr)
    want = p[f"cube_{method}"]
    assert cube.shape == want.shape
    for (i, j), bound in bounds.items():
        assert np.all(np.abs(cube[i, j] - want[i, j]) <= bound)


@pytest.mark.parametrize("method", ["poly", "Legendre"])
@pytest.mark.parametrize("k", range(4))
def test_device_regrid_against_restatement_and_reference(method, k):
    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.comps import regrid, regrid_dev
    from pfb_imaging_amd.utils.modelspec import eval_coeffs_to_slice

    p = pins()
    tag = f"small_{method}"
    coeffs, xi, yi, expr, params, texpr, fexpr, _ = fit_outputs(tag)
    nxi, nyi, cxi, cyi, x0i, y0i = p["slice_in"]
    nxo, nyo, cxo, cyo, x0o, y0o = p["slice_grids"][k]
    nxi, nyi, nxo, nyo = int(nxi), int(nyi), int(nxo), int(nyo)
    image, rbound = ref.render(nxi, nyi, xi, yi, coeffs, basis_of(tag)(p["eval_time"][1], p["eval_freq"][0]))
    want, bound, interpolated = ref.regrid(image, cxi, cyi, x0i, y0i, nxo, nyo, cxo, cyo, x0o, y0o)
    got = regrid(image, cxi, cyi, x0i, y0i, nxo, nyo, cxo, cyo, x0o, y0o)
    assert got.shape == (nxo, nyo) and np.all(np.abs(got - want) <= bound)
    src, dst = _lib.DeviceArray.from_host(image), _lib.DeviceArray.from_host(np.full((nxo, nyo), np.nan))
    assert regrid_dev(src, cxi, cyi, x0i, y0i, dst, cxo, cyo, x0o, y0o) == interpolated == (k != 3)
    assert np.array_equal(dst.download(), got)
    if k == 3:
        assert np.array_equal(got, image)                       # as it is: no area ratio
    # the public function (device render, then regrid) against the reference
    ref_out = p[f"slice_{method}_{k}"]
    out = eval_coeffs_to_slice(p["eval_time"][1], p["eval_freq"][0], coeffs, xi, yi, expr, params, texpr, fexpr, nxi, nyi, cxi, cyi,
                               x0i, y0i, nxo, nyo, cxo, cyo, x0o, y0o)
    carried = ref.regrid(rbound, cxi, cyi, x0i, y0i, nxo, nyo, cxo, cyo, x0o, y0o)[0]
    assert out.shape == ref_out.shape and np.all(np.abs(out - ref_out) <= bound + carried)


def test_locations_outside_the_image_are_refused():
    from pfb_imaging_amd.comps import Comps

    with pytest.raises(ValueError, match="outside"):
        Comps(8, 8, np.array([8]), np.array([0]), np.ones((1, 1)))
    with pytest.raises(ValueError, match="outside"):
        Comps(8, 8, np.array([0]), np.array([-1]), np.ones((1, 1)))
    with pytest.raises(ValueError, match="distinct"):      # the scatter would race where numpy lets the last one win
        Comps(8, 8, np.array([1, 3, 1]), np.array([2, 2, 2]), np.ones((1, 3)))


def test_render_into_poisoned_targets():
    env = dict(os.environ, PFBHIP_DEVCACHE_POISON="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_modelspec_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "poison ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def _c2v_gridder_kw(mds, epsilon=1e-7):
    a = mds["attrs"]
    return dict(pixsize_x=a["cell_rad_x"], pixsize_y=a["cell_rad_x"], center_x=a["center_x"], center_y=a["center_y"], epsilon=epsilon,
                flip_u=a["flip_u"], flip_v=a["flip_v"], flip_w=a["flip_w"], do_wgridding=True, divide_by_n=False)


def test_dirty2vis_dev_adds_no_arithmetic():
    """dirty2vis of the device render is bit-identical to dirty2vis of its download on the same plan."""
    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.comps import Comps
    from pfb_imaging_amd.wgridder import Gridder

    args, region, mds, _ = c2v_fixture()
    uvw, freq = args[0], args[2]
    nx, ny = mds["attrs"]["npix_x"], mds["attrs"]["npix_y"]
    comps = Comps(nx, ny, mds["location_x"], mds["location_y"], mds["coefficients"])
    render_dev = _lib.DeviceArray((nx, ny), np.float64)
    comps.render_dev(basis_of("c2v_fit")(1100.0, 1.1e9), render_dev)
    render_host = render_dev.download()
    assert render_host.any()
    wgt = np.random.default_rng(5).random((uvw.shape[0], freq.size))
    g = Gridder(uvw, freq, None, npix_x=nx, npix_y=ny, **_c2v_gridder_kw(mds))
    for w in (None, wgt):
        a, b = g.dirty2vis_dev(render_dev, w), g.dirty2vis(render_host, w)
        assert a.shape == (uvw.shape[0], freq.size) and a.any() and np.array_equal(a, b)
    g.close()
    comps.close()


def test_comps2vis_on_the_device():
    from pfb_imaging_amd import wgridder
    from pfb_imaging_amd.operators.gridder import comps2vis

    p = pins()
    args, region, mds, frange = c2v_fixture()
    coeffs, xi, yi = mds["coefficients"], mds["location_x"], mds["location_y"]
    nx, ny = mds["attrs"]["npix_x"], mds["attrs"]["npix_y"]
    modelf, tfunc, ffunc = _lambdified("c2v_fit")
    basis = basis_of("c2v_fit")
    kw = _c2v_gridder_kw(mds)
    info = {}
    got = comps2vis(*args, region, mds, modelf, tfunc, ffunc, epsilon=1e-7, product="IQ", info=info, **frange)
    assert got.shape == (400, 6, 2) and got.dtype == np.complex128
    assert info["device_renders"] == 4 and info["host_renders"] == 0 and info["plans"] >= 1
    assert np.array_equal(got[..., 0], got[..., 1]) and not got[:, 4:].any() and got[:, :4].all()

    def degrid(uvw, freq, image):
        return wgridder.dirty2vis(uvw=uvw, freq=freq, dirty=image, **kw)

    # the host composition of the parent commit: restatement render, then the stateless dirty2vis.  Render sums of 4 terms
    # reach the visibilities linearly, so the two agree to a small multiple of 2^-53.
    want = ref.comps2vis(*args, region, coeffs, xi, yi, nx, ny, lambda t, f: ref.render(nx, ny, xi, yi, coeffs, basis(t, f))[0],
                         degrid, nproduct=2, **frange)
    print(f"comps2vis vs host composition: rel l2 {rel(got, want):.3e}; vs DFT pins {rel(got, p['c2v_vis']):.3e}")
    assert rel(got, want) < 1e-12
    assert rel(got, p["c2v_vis"]) < 1e-7                        # the direct DFT of the reference-run pins, at the plan's epsilon

    # a modelf with a squared parameter is rendered on the host, never linearised
    info = {}
    got_n = comps2vis(*args, region, mds, ref.nonlinear_modelf, tfunc, ffunc, epsilon=1e-7, product="IQ", info=info, **frange)
    assert info["device_renders"] == 0 and info["host_renders"] == 4

    def render_nl(t, f):
        image = np.zeros((nx, ny))
        image[xi, yi] = ref.nonlinear_modelf(tfunc(t), ffunc(f), *coeffs)
        return image

    want_n = ref.comps2vis(*args, region, coeffs, xi, yi, nx, ny, render_nl, degrid, nproduct=2, **frange)
    assert rel(got_n, want_n) < 1e-12 and rel(got_n, p["c2v_vis_nonlinear"]) < 1e-7
    assert rel(got_n, got) > 1e-3                               # (and it is a different model)


def test_comps2vis_empty_region_makes_no_plan():
    from pfb_imaging_amd import wgridder
    from pfb_imaging_amd.operators.gridder import comps2vis

    args, region, mds, frange = c2v_fixture()
    modelf, tfunc, ffunc = _lambdified("c2v_fit")
    wgridder.clear_cache()
    info = {}
    got = comps2vis(*args, np.zeros_like(region), mds, modelf, tfunc, ffunc, epsilon=1e-7, product="IQ", info=info, **frange)
    assert got.shape == (400, 6, 2) and not got.any()
    assert info == dict(device_renders=0, host_renders=0, plans=0) and len(wgridder._cache) == 0
