"""GPU tests of ``pfbhip_gaussconv_*`` (csrc/restore.hip) through ``utils.misc.convolve2gaussres`` and
``utils.restoration.restore_arrays``, against the reference-run fixture tests/golden/restore_pins.npz.

The bound of every comparison is the larger of 10 x the stored disagreement of the two reference runs (numpy-FFT against
scipy-FFT stand-ins, relative to the output's max norm) and 1e-11 (tests/_restore_ref.py ``bound``).  Each test prints its
figures before it asserts.
"""

import numpy as np
import pytest

from tests import _restore_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pins(golden_dir):
    return np.load(f"{golden_dir}/restore_pins.npz")


def check(tag, got, pins, key):
    err, dis = ref.rel_max(got, pins[f"{key}_np"]), float(pins[f"{key}_disagreement"])
    print(f"{tag}: device vs numpy-FFT reference run {err:.3e}; reference runs disagree by {dis:.3e}; bound {ref.bound(dis):.1e}")
    assert np.isfinite(got).all() and err <= ref.bound(dis)


def conv(c, **kw):
    from pfb_imaging_amd.utils.misc import convolve2gaussres

    return convolve2gaussres(c["image"], c["xx"], c["yy"], c["gaussparf"], gausspari=c["gausspari"], pfrac=c["pfrac"], **kw)


def test_plan_shape_follows_get_padding_info(pins):
    from pfb_imaging_amd.gaussconv import cached_plan

    p = cached_plan(3, 36, 50, 0.2)
    assert (p.nfft_x, p.nfft_y, p.padl_x, p.padl_y) == (45, 60, 4, 5)  # one odd, one even, left pad < right pad on x
    assert cached_plan(3, 36, 50, 0.2) is p
    q = cached_plan(2, 40, 40, 0.5)
    assert (q.nfft_x, q.nfft_y, q.padl_x, q.padl_y) == (60, 60, 10, 10)


@pytest.mark.parametrize("norm", [False, True])
def test_case_a_point_sources_in_the_corners(pins, norm):
    got = conv(ref.case("A"), norm_kernel=norm)
    check(f"A norm_kernel={norm}", got, pins, f"A_norm{int(norm)}")


def test_case_b_per_band_resolution_even_sizes(pins):
    check("B", conv(ref.case("B")), pins, "B")


def test_case_c_ratio_of_gaussians(pins):
    check("C", conv(ref.case("C")), pins, "C")


def test_scaled_grids_and_host_rendered_kernels(pins):
    """A grid in radians with the resolution in radians is case A again (the axis scale goes down to the render kernel);
    grids that are no scaled pixel offsets take kernels rendered on the host, here one that happens to be case A's."""
    from pfb_imaging_amd.gaussconv import cached_plan
    from pfb_imaging_amd.utils.misc import gaussian2d

    a = ref.case("A")
    cell = 2.0 ** -15  # a power of two: the scaled problem is case A exactly
    xx, yy = ref.offsets(36, 50, cell, cell)
    par = a["gaussparf"] * np.array([cell, cell, 1.0])
    from pfb_imaging_amd.utils.misc import convolve2gaussres

    check("A scaled grid", convolve2gaussres(a["image"], xx, yy, par, pfrac=0.2), pins, "A_norm0")
    plan = cached_plan(3, 36, 50, 0.2)
    kern = gaussian2d(a["xx"], a["yy"], a["gaussparf"], normalise=True)[None]
    check("A host-rendered kernel", plan.apply(a["image"], a["gaussparf"], kernf=kern), pins, "A_norm1")
    # the dispatch itself: grids shifted by an amount far below the comparison's bound are no pixel offsets any more
    got = convolve2gaussres(a["image"], a["xx"] + 1e-13, a["yy"], a["gaussparf"], pfrac=0.2, norm_kernel=True)
    check("A perturbed grid (host render)", got, pins, "A_norm1")


def test_case_d_restore(pins):
    from pfb_imaging_amd.utils.restoration import restore_arrays

    d = ref.case("D")
    image, parf = restore_arrays(d["model"], d["residual"], d["wsum"], d["gausspari"], d["gaussparf"])
    assert np.array_equal(parf, d["gaussparf"])
    check("D", image, pins, "D")
    mine = ref.rel_max(image, ref.restore(**d))
    print(f"D: device vs tests/_restore_ref.py {mine:.3e}")
    assert mine <= ref.bound(pins["D_disagreement"])
    # a 1-D gaussparf is tiled over the bands (restoration.py:56-60)
    image1, parf1 = restore_arrays(d["model"], d["residual"], d["wsum"], d["gausspari"], (6.0, 5.0, 0.3))
    assert parf1.shape == (3, 3) and np.array_equal(image1[0], image[0]) and np.array_equal(image1[2], image[2])
    assert ref.rel_max(image1, ref.restore(d["model"], d["residual"], d["wsum"], d["gausspari"], (6.0, 5.0, 0.3))) <= ref.BOUND_FLOOR


def test_plan_reuse_dev_and_host_poisoned_between(pins):
    """Host and device entry points agree bit for bit; two applies on one plan with different parameters carry nothing
    over (every buffer of the plan is NaN in between); a repeated call is bit-identical, normalisation included."""
    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.gaussconv import GaussConvPlan

    a, c, d = ref.case("A"), ref.case("C"), ref.case("D")
    plan = GaussConvPlan(3, 36, 50, 0.2)
    first = plan.apply(a["image"], a["gaussparf"], norm_kernel=True).copy()
    plan.debug_fill(0xFF)
    ratio = plan.apply(c["image"], c["gaussparf"], c["gausspari"]).copy()
    check("C on a poisoned plan", ratio, pins, "C")
    plan.debug_fill(0xFF)
    second = plan.apply(a["image"], a["gaussparf"], norm_kernel=True).copy()
    assert np.array_equal(first, second)
    check("A after C on a poisoned plan", second, pins, "A_norm1")
    assert np.array_equal(plan.apply(a["image"], a["gaussparf"], norm_kernel=True), first)  # no poison in between either

    x_dev, out_dev = _lib.DeviceArray.from_host(c["image"]), _lib.DeviceArray((3, 36, 50))
    plan.debug_fill(0xFF)
    plan.apply_dev(x_dev, out_dev, c["gaussparf"], c["gausspari"])
    assert np.array_equal(out_dev.download(), ratio)
    m_dev, r_dev = _lib.DeviceArray.from_host(d["model"]), _lib.DeviceArray.from_host(d["residual"])
    plan.restore_dev(m_dev, r_dev, out_dev, d["wsum"], d["gausspari"], d["gaussparf"])
    dev_image = out_dev.download().copy()
    plan.debug_fill(0xFF)
    assert np.array_equal(plan.restore(d["model"], d["residual"], d["wsum"], d["gausspari"], d["gaussparf"]), dev_image)
    check("D through restore_dev", dev_image, pins, "D")
    for arr in (x_dev, out_dev, m_dev, r_dev):
        arr.free()
    plan.close()


def test_bad_parameters_are_refused_not_faulted():
    from pfb_imaging_amd.gaussconv import GaussConvPlan

    plan = GaussConvPlan(2, 12, 10, 0.5)
    img = np.ones((2, 12, 10))
    ok = np.array([[3.0, 2.0, 0.1], [3.0, 2.5, 0.2]])
    for parf, pari, word in (((np.nan, 2.0, 0.0), None, "finite"), ((2.0, 3.0, 0.0), None, "emin"), ((0.0, 0.0, 0.0), None, "positive"),
                             ((3.0, 2.0, 0.0), ok[:1], "length nband"), (np.ones((3, 3)), None, "expected 1 or nband"),
                             (ok, np.array([[3.0, 2.0, 0.1], [3.0, np.inf, 0.2]]), "finite")):
        with pytest.raises(ValueError, match=word):
            plan.apply(img, parf, pari)
    with pytest.raises(ValueError, match="wsum"):
        plan.restore(img, img, [1.0, 0.0], ok, ok)
    with pytest.raises(ValueError, match="scales"):
        plan.apply(img, ok, scale=(0.0, 1.0))
    assert np.isfinite(plan.apply(img, ok, ok)).all()  # the plan is still good
    plan.close()
