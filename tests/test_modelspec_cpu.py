"""CPU tests of the component model: the host restatement (tests/_modelspec_ref.py) and the host side of the product
(strings, linearity check, comps2vis bookkeeping) against the reference-run pins of tests/golden/modelspec_pins.npz.

Bounds.  Render and regrid: elementwise ``8 n 2^-53 sum|terms|`` as computed by the restatement (n = nparam or 4).  Fit:
``64 cond(hess_coeffs) 2^-53 |coeffs|_inf`` per case -- the restatement applies an explicit ``A = solve(hess, xfit^T w)`` where
the reference solves per right-hand side, and the two differ by the conditioning (largest ratio observed against
``cond 2^-53 |coeffs|_inf``: 1.2)."""

import numpy as np
import pytest

from . import _modelspec_ref as ref
from ._modelspec_pins import FIT_CASES, basis_of, c2v_fixture, fit_inputs, fit_outputs, pins

FIT_TAGS = [t for t, c in FIT_CASES.items() if c[0] is not None]


def _lambdified(expr, params, texpr, fexpr):
    from pfb_imaging_amd.utils.modelspec import _parse

    return _parse(expr, params, texpr, fexpr)


@pytest.mark.parametrize("tag", FIT_TAGS)
def test_fit_restatement_matches_reference(tag):
    time, freq, image, wgt, nbt, nbf, method, sigmasq = fit_inputs(tag)
    coeffs, xi, yi, expr, params, texpr, fexpr, cond = fit_outputs(tag)
    cube = image.reshape(-1, *image.shape[2:])
    rx, ry = ref.support(cube)
    assert np.array_equal(rx, xi) and np.array_equal(ry, yi)
    xfit, w, hess, basis = ref.design(time, freq, wgt, nbt, nbf, method, sigmasq)
    assert np.linalg.cond(hess) < 1e8 and cond < 1e8                       # the condition the fit bound rests on
    assert abs(np.linalg.cond(hess) - cond) <= 1e-6 * cond
    got, _ = ref.fit(cube, ref.fit_matrix(xfit, w, hess), rx, ry)
    assert got.shape == coeffs.shape == (basis.nparam, xi.size)
    err = np.abs(got - coeffs).max()
    bound = 64 * cond * ref.EPS * np.abs(coeffs).max()
    print(f"{tag}: ncomps {xi.size} max|diff| {err:.3e} bound {bound:.3e} cond {cond:.3e}")
    assert err <= bound


def test_fit_fixture_has_the_hard_pixels():
    """The shapes the compaction can go wrong at are really in the fixture."""
    cube = pins()["fit_cube"].reshape(12, 300, 260)
    xi, yi = ref.support(cube)
    flat = xi * 260 + yi
    assert 2500 < xi.size < 3500
    assert flat[0] == 0 and flat[-1] == 300 * 260 - 1                       # first and last pixel
    assert (xi == 50).sum() == 260                                          # one full row
    assert np.diff(flat).max() > 2 * 1024                                   # a zero run longer than two workgroups' pixels
    assert (cube[:, 10, 7] != 0).sum() == 1                                 # nonzero in exactly one plane
    assert cube[:, 11, 200].sum() == 0.0 and (cube[:, 11, 200] != 0).sum() == 3 and (11 * 260 + 200) in flat
    assert (cube < 0).any()


@pytest.mark.parametrize("tag", FIT_TAGS)
def test_product_strings_are_the_references(tag):
    """expr / params / tfunc / ffunc are formed on the host by the product exactly as the reference forms them."""
    from pfb_imaging_amd.utils.modelspec import _design

    time, freq, image, wgt, nbt, nbf, method, sigmasq = fit_inputs(tag)
    _, _, _, expr, params, texpr, fexpr, cond = fit_outputs(tag)
    xfit, w, hess, e, p, tf, ff = _design(time, freq, wgt, nbt, nbf, method, sigmasq)
    assert (e, p, tf, ff) == (expr, params, texpr, fexpr)
    rxfit, rw, rhess, _ = ref.design(time, freq, wgt, nbt, nbf, method, sigmasq)
    np.testing.assert_allclose(xfit, rxfit, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(hess, rhess, rtol=1e-12)
    assert np.array_equal(w[:, 0], rw)


def test_single_band_raises_as_the_reference_does():
    from pfb_imaging_amd.utils.modelspec import fit_image_cube

    assert str(pins()["fit_11_raises"]) == "UnboundLocalError"             # what the reference did with ntime == nband == 1
    p = pins()
    with pytest.raises(ValueError, match="unbound"):
        fit_image_cube(p["time"][:1], p["freq"][:1], p["fit_cube"][:1, :1])
    with pytest.raises(ValueError, match="unbound"):
        fit_image_cube(p["time"], p["freq"][:1], p["fit_cube"][:, :1])


@pytest.mark.parametrize("method", ["poly", "Legendre"])
def test_render_restatement_matches_reference(method):
    p = pins()
    tag = f"small_{method}"
    coeffs, xi, yi, expr, params, texpr, fexpr, _ = fit_outputs(tag)
    basis = basis_of(tag)
    modelf, tfunc, ffunc = _lambdified(expr, params, texpr, fexpr)
    want = p[f"cube_{method}"]
    for i, t in enumerate(p["eval_time"]):
        for j, f in enumerate(p["eval_freq"]):
            b = basis(t, f)
            # the restatement's basis vector is the lambdified expression's, to rounding of each entry's own few terms
            np.testing.assert_allclose(b, modelf(tfunc(t), ffunc(f), *np.eye(basis.nparam)), rtol=0, atol=32 * ref.EPS * np.abs(b).max())
            image, bound = ref.render(40, 28, xi, yi, coeffs, b)
            assert bound.max() > 0 and np.all(np.abs(image - want[i, j]) <= bound)
            assert not image[want[i, j] == 0].any()


@pytest.mark.parametrize("method", ["poly", "Legendre"])
@pytest.mark.parametrize("k", range(4))
def test_regrid_restatement_matches_reference(method, k):
    p = pins()
    tag = f"small_{method}"
    coeffs, xi, yi = fit_outputs(tag)[:3]
    nxi, nyi, cxi, cyi, x0i, y0i = p["slice_in"]
    nxo, nyo, cxo, cyo, x0o, y0o = p["slice_grids"][k]
    image, rbound = ref.render(int(nxi), int(nyi), xi, yi, coeffs, basis_of(tag)(p["eval_time"][1], p["eval_freq"][0]))
    out, bound, interpolated = ref.regrid(image, cxi, cyi, x0i, y0i, int(nxo), int(nyo), cxo, cyo, x0o, y0o)
    want = p[f"slice_{method}_{k}"]
    assert out.shape == want.shape == (int(nxo), int(nyo))
    assert interpolated == (k != 3)
    # the render's own bound reaches the output through the same non-negative corner weights
    carried = ref.regrid(rbound, cxi, cyi, x0i, y0i, int(nxo), int(nyo), cxo, cyo, x0o, y0o)[0]
    assert np.all(np.abs(out - want) <= bound + carried)
    if k == 0:    # zero padding on all four sides: the output grid reaches beyond the input everywhere
        assert not want[0].any() and not want[-1].any() and not want[:, 0].any() and not want[:, -1].any() and want.any()
    if k == 3:    # pass-through: the image as rendered, no area ratio
        assert np.all(np.abs(want - image) <= rbound)


def test_basis_vector_accepts_linear_and_refuses_nonlinear():
    from pfb_imaging_amd.comps import basis_vector

    for tag in ("small_poly", "small_Legendre", "c2v_fit"):
        coeffs, _, _, expr, params, texpr, fexpr, _ = fit_outputs(tag)
        modelf, tfunc, ffunc = _lambdified(expr, params, texpr, fexpr)
        tt, ff = tfunc(1234.5), ffunc(1.17e9)
        b = basis_vector(modelf, tt, ff, len(params))
        assert b is not None and b.shape == (len(params),)
        direct = modelf(tt, ff, *coeffs)
        assert np.all(np.abs(b @ coeffs - direct) <= 8 * b.size * ref.EPS * (np.abs(b) @ np.abs(coeffs)))
    assert basis_vector(ref.nonlinear_modelf, 0.3, -0.2, 4) is None
    assert basis_vector(lambda t, f, a, b: 1.0 + a * t + b * f, 0.3, -0.2, 2) is None      # affine: modelf(0) != 0
    assert basis_vector(lambda t, f, a, b: a * b, 0.3, -0.2, 2) is None                     # bilinear: zero at 0 and on the axes


def _dft(uvw, freq, dirty, pixsize_x, pixsize_y, center_x, center_y, flip_u, flip_v, flip_w, epsilon, do_wgridding, divide_by_n,
         nthreads):
    from oracle.dft import dft_dirty2vis

    return dft_dirty2vis(uvw, freq, dirty, pixsize_x, pixsize_y, center_x, center_y, flip_u, flip_v, flip_w, do_wgridding, divide_by_n)


@pytest.mark.parametrize("case", ["linear", "nonlinear", "zero_region"])
def test_comps2vis_bookkeeping_matches_reference(case):
    """Rows, time chunks, channels, region mask, frequency range and product replication of comps2vis, with the gridder
    replaced by the direct DFT the pins were made with."""
    from pfb_imaging_amd.operators.gridder import comps2vis

    p = pins()
    args, region, mds, frange = c2v_fixture()
    coeffs, xi, yi, expr, params, texpr, fexpr, _ = fit_outputs("c2v_fit")
    modelf, tfunc, ffunc = _lambdified(expr, params, texpr, fexpr)
    want = p["c2v_vis" + {"linear": "", "nonlinear": "_nonlinear", "zero_region": "_zero_region"}[case]]
    if case == "nonlinear":
        modelf = ref.nonlinear_modelf
    if case == "zero_region":
        region = np.zeros_like(region)
    info = {}
    got = comps2vis(*args, region, mds, modelf, tfunc, ffunc, epsilon=1e-7, product="IQ", info=info, _dirty2vis=_dft, **frange)
    assert got.shape == want.shape == (400, 6, 2) and got.dtype == want.dtype == np.complex128
    # the same images through the same DFT: only the order of a few additions inside modelf could differ
    assert np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1.0)
    assert np.array_equal(got[..., 0], got[..., 1])
    assert not got[:, 4:].any()                                             # the band outside [freq_min, freq_max]
    if case == "zero_region":
        assert not got.any() and info["host_renders"] == 0
    else:
        assert got[:, :4].all() and info["host_renders"] == 4               # 2 time chunks x 2 bands in range
    if case != "linear":
        return
    # the restatement of the bookkeeping, rendering with its own basis vectors
    nx, ny, attrs = mds["attrs"]["npix_x"], mds["attrs"]["npix_y"], mds["attrs"]
    basis = basis_of("c2v_fit")
    slack = []

    def render_at(t, f):
        image, bound = ref.render(nx, ny, xi, yi, coeffs, basis(t, f))
        # |vis| sums |pixel| over the nonzero pixels (unit-modulus phases): the render's bound and the DFT's own sum
        slack.append(bound.sum() + 8 * xi.size * ref.EPS * np.abs(image).sum())
        return image

    def degrid(uvw, freq, image):
        return _dft(uvw, freq, image, attrs["cell_rad_x"], attrs["cell_rad_x"], attrs["center_x"], attrs["center_y"], attrs["flip_u"],
                    attrs["flip_v"], attrs["flip_w"], 1e-7, True, False, 1)

    mine = ref.comps2vis(*args, region, coeffs, xi, yi, nx, ny, render_at, degrid, nproduct=2, **frange)
    assert np.abs(mine - want).max() <= max(slack)


def test_comps2vis_dtype_and_out_of_range():
    """Nothing is touched when no channel lies in the range; the dtype follows the coefficients."""
    from pfb_imaging_amd.operators.gridder import comps2vis

    args, region, mds, _ = c2v_fixture()
    mds = dict(mds, coefficients=mds["coefficients"].astype(np.float32))

    def never(**kw):
        raise AssertionError("degridded")

    got = comps2vis(*args, region, mds, None, None, None, product="I", freq_min=2e9, freq_max=3e9, _dirty2vis=never)
    assert got.shape == (400, 6, 1) and got.dtype == np.complex64 and not got.any()
