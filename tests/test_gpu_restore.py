"""GPU tests of ``pfbhip_gaussconv_*`` (csrc/restore.hip) through ``utils.misc.convolve2gaussres`` and
``utils.restoration.restore_arrays``, against the reference-run fixtures tests/golden/restore_pins.npz (cases A-D) and
restore_edge_pins.npz (cases E-L: every launch form of the kernels, ``_restore_ref.kernel_forms``).

The bound of every comparison is the larger of 10 x the stored disagreement of the two reference runs (numpy-FFT against
scipy-FFT stand-ins, relative to the output's max norm) and 1e-11 (tests/_restore_ref.py ``bound``).  Each test prints its
figures before it asserts.
"""

import ctypes as ct

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


# ---- the edge cases E-L of tests/_restore_ref.py: every launch form of csrc/restore.hip (``kernel_forms`` there) -----------------
@pytest.fixture(scope="module")
def edge_pins(golden_dir):
    return np.load(f"{golden_dir}/restore_edge_pins.npz")


@pytest.fixture(scope="module")
def plans():
    """``plans(nband, nx, ny, pfrac)``: one plan per geometry, made on first use and shared by the tests below"""
    from pfb_imaging_amd.gaussconv import GaussConvPlan

    made = {}

    def get(*key):
        if key not in made:
            made[key] = GaussConvPlan(*key)
        return made[key]

    yield get
    for plan in made.values():
        plan.close()


def statement_spread(c, norm=False, **kw):
    """the numpy statement over scipy.fft against itself over numpy.fft: how far transform rounding moves this case"""
    args = (c["image"], c["xx"], c["yy"], c["gaussparf"], c["gausspari"], c["pfrac"], norm)
    import scipy.fft

    return ref.rel_max(ref.convolve(*args, fft=scipy.fft, **kw), ref.convolve(*args, **kw))


@pytest.mark.parametrize("tag", list(ref.EDGE_RUNS))
def test_edge_case_against_its_reference_run(edge_pins, plans, tag):
    """E, F: one element per lane in pad and render, two and three trips of the row loop; G: two per lane, two trips, the ratio
    with both sums read from device memory; H: the smallest geometry; I: a padded row of exactly 512, half of the division
    in its second branch; J: the same on a grid with a negative step (through ``convolve2gaussres``, whose ``_axis_scales``
    hands the step down); L: an odd padded row of one trip, per-band resolutions on both sides of the ratio."""
    from pfb_imaging_amd.utils.misc import convolve2gaussres

    name, norm = ref.EDGE_RUNS[tag]
    c = ref.case(name)
    print(f"{tag}: {ref.kernel_forms(*ref.geometry(name))}")
    if c["gausspari"] is not None:
        print(f"{tag}: statement over scipy.fft vs over numpy.fft {statement_spread(c, norm):.3e}")
    if name == "J_scaled":
        from pfb_imaging_amd.utils.misc import _axis_scales

        assert c["yy"][0, -1] < 0 and _axis_scales(c["xx"], c["yy"], 7, 301) == ref.J_SCALE  # rendered on the device
        got = conv(c, norm_kernel=norm)
    else:
        got = plans(*ref.geometry(name)).apply(c["image"], c["gaussparf"], c["gausspari"], norm_kernel=norm)
    check(tag, got, edge_pins, tag)
    if name == "J":  # the public entry point on the unit grid is the same call
        assert np.array_equal(convolve2gaussres(c["image"], c["xx"], c["yy"], c["gaussparf"], gausspari=c["gausspari"], pfrac=0.2), got)


def test_case_k_restore_at_an_odd_row_of_two_trips(edge_pins):
    """Band 0 takes the ratio and the accumulating crop, band 1 the pass-through add, both one element per lane, two trips."""
    from pfb_imaging_amd.utils.restoration import restore_arrays

    k = ref.case("K")
    image, parf = restore_arrays(k["model"], k["residual"], k["wsum"], k["gausspari"], k["gaussparf"])
    assert np.array_equal(parf, k["gaussparf"])
    check("K", image, edge_pins, "K")
    mine = ref.rel_max(image, ref.restore(**k))
    print(f"K: device vs tests/_restore_ref.py {mine:.3e}")
    assert mine <= ref.bound(edge_pins["K_disagreement"])


class Shifted:
    """a cube of ``shape`` one double past the start of a device allocation one double longer: 8-byte aligned, not 16"""

    def __init__(self, shape, host=None):
        from pfb_imaging_amd import _lib

        self.n = int(np.prod(shape))
        self.shape, self.buf = tuple(shape), _lib.DeviceArray((self.n + 1,))
        self.ptr = ct.c_void_p(self.buf.ptr.value + 8)
        assert self.buf.ptr.value % 16 == 0 and self.ptr.value % 16 == 8
        if host is not None:
            host = np.ascontiguousarray(host, dtype=np.float64)
            assert host.shape == self.shape
            _lib.check(_lib.lib().pfbhip_memcpy_h2d(self.ptr, _lib.ptr(host), ct.c_size_t(8 * self.n)))

    def download(self):
        from pfb_imaging_amd import _lib

        out = np.empty(self.shape)
        _lib.check(_lib.lib().pfbhip_memcpy_d2h(_lib.ptr(out), self.ptr, ct.c_size_t(8 * self.n)))
        return out

    def free(self):
        self.buf.free()
        self.ptr = None


def test_store_widths_agree_bit_for_bit(plans):
    """The crop pass stores pairs where the row is even and both cubes are 16-byte aligned, single elements otherwise: same
    arithmetic, so the same bits.  Case G's even rows (540: two trips at pairs, three at single elements) through
    ``pfbhip_gaussconv_apply_dev`` with the output, then the input, misaligned; the restore of case D with the residual
    misaligned, which is the ``add`` operand of its pass-through band."""
    from pfb_imaging_amd import _lib
    from pfb_imaging_amd._lib import cint, f64

    g = ref.case("G")
    plan = plans(*ref.geometry("G"))
    *_, pargs = plan._par_args(g["gaussparf"], g["gausspari"])

    def apply_raw(image_ptr, out_ptr):
        _lib.check(_lib.lib().pfbhip_gaussconv_apply_dev(plan._h, image_ptr, *pargs, cint(1), f64(1.0), f64(1.0), None, None, out_ptr))

    x_dev, out_dev = _lib.DeviceArray.from_host(g["image"]), _lib.DeviceArray(g["image"].shape)
    apply_raw(x_dev.ptr, out_dev.ptr)
    aligned = out_dev.download().copy()
    assert np.array_equal(aligned, plan.apply(g["image"], g["gaussparf"], g["gausspari"], norm_kernel=True))
    out_off = Shifted(g["image"].shape, np.full(g["image"].shape, np.nan))
    apply_raw(x_dev.ptr, out_off.ptr)
    assert np.array_equal(out_off.download(), aligned)
    out_dev.upload(np.full(g["image"].shape, np.nan))
    x_off = Shifted(g["image"].shape, g["image"])  # named: the allocation must outlive the call
    assert np.array_equal(x_off.download(), g["image"])
    apply_raw(x_off.ptr, out_dev.ptr)
    assert np.array_equal(out_dev.download(), aligned)

    d = ref.case("D")
    plan = plans(3, 36, 50, 0.2)
    *_, rargs = plan._restore_args(d["wsum"], d["gausspari"], d["gaussparf"])
    want = plan.restore(d["model"], d["residual"], d["wsum"], d["gausspari"], d["gaussparf"]).copy()
    m_dev, image_dev = _lib.DeviceArray.from_host(d["model"]), _lib.DeviceArray(d["model"].shape)
    r_off = Shifted(d["residual"].shape, d["residual"])
    _lib.check(_lib.lib().pfbhip_gaussconv_restore_dev(plan._h, m_dev.ptr, r_off.ptr, *rargs, image_dev.ptr))
    assert np.array_equal(image_dev.download(), want)
    for arr in (x_dev, out_dev, m_dev, image_dev, out_off, x_off, r_off):
        arr.free()


def test_mask_branch_and_a_pure_phase_denominator(plans):
    """``kerni = 0`` makes thishat exactly zero: the output is exactly zero, not NaN.  ``kerni`` a single 1 at the centre pixel
    of case I's geometry lands on padded index -1 of both axes (5 -> 6, 427 -> 512): thishat is a pure phase of modulus 1
    and the division takes both of its branches; the statement is fed the same kernel images."""
    c = ref.case("I")
    plan = plans(*ref.geometry("I"))
    kernf = ref.gaussian(c["xx"], c["yy"], c["gaussparf"])[None]
    kerni = np.zeros_like(c["image"])
    got = plan.apply(c["image"], c["gaussparf"], c["gausspari"], kernf=kernf, kerni=kerni)
    assert np.isfinite(got).all() and np.array_equal(got, np.zeros_like(got))
    kerni[0, 5 // 2, 427 // 2] = 1.0
    got = plan.apply(c["image"], c["gaussparf"], c["gausspari"], kernf=kernf, kerni=kerni)
    want = ref.convolve(c["image"], c["xx"], c["yy"], c["gaussparf"], c["gausspari"], c["pfrac"], kernf=kernf, kerni=kerni)
    spread = statement_spread(c, kernf=kernf, kerni=kerni)
    err = ref.rel_max(got, want)
    print(f"pure-phase thishat: device vs statement {err:.3e}; statement over scipy.fft vs over numpy.fft {spread:.3e}; "
          f"bound {ref.bound(spread):.1e}")
    assert np.isfinite(got).all() and err <= ref.bound(spread)
    # dividing by a unit impulse one pixel off the origin is a shift by one pixel on both axes
    shifted = ref.convolve(c["image"], c["xx"], c["yy"], c["gaussparf"], None, c["pfrac"], kernf=kernf)
    assert ref.rel_max(want[0, 1:, 1:], shifted[0, :-1, :-1]) <= ref.BOUND_FLOOR


def test_poison_and_reuse_at_the_odd_forms(edge_pins, plans):
    """E, then J, then E again on one (1, 7, 301) plan, every buffer NaN in between: the two-stage sum at one element per lane
    with a row of two trips carries nothing over and repeats bit for bit."""
    e, j = ref.case("E"), ref.case("J")
    plan = plans(*ref.geometry("E"))
    first = plan.apply(e["image"], e["gaussparf"], norm_kernel=True).copy()
    plan.debug_fill(0xFF)
    check("J on a poisoned plan", plan.apply(j["image"], j["gaussparf"], j["gausspari"]), edge_pins, "J")
    plan.debug_fill(0xFF)
    second = plan.apply(e["image"], e["gaussparf"], norm_kernel=True).copy()
    assert np.array_equal(first, second)
    check("E after J on a poisoned plan", second, edge_pins, "E_norm1")


def test_plan_cache_closes_the_oldest_and_a_stale_plan_is_refused():
    from pfb_imaging_amd.gaussconv import cached_plan, clear_cache

    clear_cache()
    keys = ((1, 4, 6, 0.5), (1, 6, 4, 0.5), (2, 4, 6, 0.5))
    img = np.random.default_rng(46).standard_normal((1, 4, 6))
    par = (3.0, 2.0, 0.4)
    first = cached_plan(*keys[0])
    before = first.apply(img, par).copy()
    assert cached_plan(*keys[1]) is not first and cached_plan(*keys[0]) is first  # two fit
    cached_plan(*keys[1])  # the first is now the older of the two
    cached_plan(*keys[2])
    assert not first._h.value
    with pytest.raises(ValueError, match="NULL"):
        first.apply(img, par)
    with pytest.raises(ValueError, match="NULL"):
        first.debug_fill()
    again = cached_plan(*keys[0])
    assert again is not first and np.array_equal(again.apply(img, par), before)
    xx, yy = ref.offsets(4, 6)
    c = dict(image=img, xx=xx, yy=yy, gaussparf=np.array(par), gausspari=None, pfrac=0.5)
    err, spread = ref.rel_max(before, ref.convolve(img, xx, yy, par)), statement_spread(c)
    print(f"plan cache: device vs statement {err:.3e}; bound {ref.bound(spread):.1e}")
    assert err <= ref.bound(spread)
    clear_cache()


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
