"""The clean-beam fit on the device (csrc/cleanbeam.hip, utils/misc.fitcleanbeam) against the pins of
tests/golden/cleanbeam_pins.npz: the reference's steps restated with scipy on the cases of tests/_cleanbeam_ref.py.

The reference's own function needs jax and cannot run here.  The fit is therefore held to the objective the reference
minimises: the device's point must be at least as good as the restated reference's by that objective (to the reference's
own stopping threshold factr * eps = 2.2e-9) and no further from the minimiser than the reference's point is.  Every test
prints its figures before it asserts."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cleanbeam_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FACTR_EPS = 2.2e-9   # factr = 1e7 times the machine epsilon: L-BFGS-B's relative-decrease threshold in the reference


@pytest.fixture(scope="module")
def pins():
    return ref.load_pins()


@pytest.fixture(scope="module")
def fits():
    """name -> (pars, info) of one device call per case, shared by the tests below."""
    from pfb_imaging_amd.utils.misc import _cleanbeam_raw

    out = {}

    def get(name):
        if name not in out:
            out[name] = _cleanbeam_raw(ref.case(name), ref.LEVEL, ref.NSIGMA)
        return out[name]

    return get


@pytest.mark.parametrize("name", ref.FITTED)
def test_lobe_region_and_start_match_the_pins(name, pins, fits):
    _, info = fits(name)
    r = info[0]
    tol = np.maximum(10 * pins[f"{name}_p0_disagreement"], 1e-12)
    print(f"{name}: status {r['status']} window {r['window']} nlobe {r['nlobe']} (pin {pins[f'{name}_nlobe']}) nfit {r['nfit']} "
          f"(pin {pins[f'{name}_nfit']}) |p0 - pin| {np.abs(r['p0'] - pins[f'{name}_p0'])} tol {tol}")
    assert r["nlobe"] == pins[f"{name}_nlobe"]
    assert r["nfit"] == pins[f"{name}_nfit"]
    assert np.all(np.abs(r["p0"] - pins[f"{name}_p0"]) <= tol)
    # the final window is the smallest of 64, 128, 256 that holds the lobe clear of its edges
    assert r["window"] == pins[f"{name}_window"]


@pytest.mark.parametrize("name", ref.FITTED)
def test_fit_is_as_good_as_the_reference_and_as_near_the_minimiser(name, pins, fits):
    pars, info = fits(name)
    p, r = pars[0], info[0]
    f_dev, f_ref = ref.f(p, name), float(pins[f"{name}_f_ref"])
    dist = np.abs(p - pins[f"{name}_p_exact"])
    bound = np.maximum(np.abs(pins[f"{name}_p_ref"] - pins[f"{name}_p_exact"]), 10 * pins[f"{name}_exact_spread"])
    print(f"{name}: status {r['status']} nit {r['nit']} p {p} f_dev {f_dev:.17g} f_ref {f_ref:.17g} (f_dev - f_ref) / f_ref "
          f"{(f_dev - f_ref) / f_ref:.3e} device's own f {r['f']:.17g} |p - p_exact| {dist} bound {bound}")
    assert r["status"] == "converged"
    assert f_dev <= f_ref * (1 + FACTR_EPS)
    # the record's objective is the reference's at the returned point, up to the order of a sum of nfit positive terms and
    # an ulp or two of exp in every model value (d(r^2) = 2 |r| dr, summed by Cauchy-Schwarz)
    n = float(pins[f"{name}_nfit"])
    assert abs(r["f"] - f_dev) <= n * 2.3e-16 * f_dev + 1e-15 * np.sqrt(n * f_dev)
    assert np.all(dist <= bound)


def test_window_doubles_for_a_lobe_wider_than_64(pins, fits):
    """Case E as stated (FWHM 40 x 25: the lobe above half the peak is 20 pixels from the centre at most) fits the first
    window; E2, twice as wide, cannot, and must end at 128."""
    we, we2 = fits("E")[1][0]["window"], fits("E2")[1][0]["window"]
    print("window E", we, "E2", we2)
    assert (we, we2) == (64, 128) and pins["E2_window"] == 128


def test_scaled_peak_gives_the_same_answer(fits):
    pa, pg = fits("A")[0], fits("G")[0]
    print("A", pa, "G", pg, "diff", np.abs(pa - pg))
    assert np.all(np.abs(pa - pg) <= 1e-12)


def test_islands_and_diagonal_neighbours_stay_out(pins, fits):
    """Case C carries a 4 x 4 island above the level far from the centre and one pixel above the level that touches the lobe
    through a corner only; the plain beam of the same shape has the same lobe."""
    above = int((ref.normalised(ref.case("C")[0]) > ref.LEVEL).sum())
    nlobe = fits("C")[1][0]["nlobe"]
    print("C: above level", above, "in lobe", nlobe)
    assert nlobe == pins["C_nlobe"] == above - 17


def test_spiral_needs_many_rounds(pins, fits):
    _, info = fits("H")
    print("H:", {k: info[0][k] for k in ("status", "window", "nlobe", "nit")})
    assert info[0]["nlobe"] == pins["H_nlobe"] == int((ref.case("H")[0] > 0.5).sum())
    assert info[0]["window"] == pins["H_window"]


def test_three_bands_in_one_call(pins, fits):
    from pfb_imaging_amd.utils.misc import fitcleanbeam

    pars, info = fits("I")
    print("I:", pars, [r["status"] for r in info])
    assert [r["status"] for r in info] == ["converged", "all_zero", "converged"]
    assert np.isnan(pars[1]).all()
    assert np.array_equal(pars[0], fits("A")[0][0]) and np.array_equal(pars[2], fits("I2")[0][0])
    out = fitcleanbeam(ref.case("I"), pixsize=2.5)
    assert out.shape == (3, 3) and np.isnan(out[1]).all()
    assert np.array_equal(out[[0, 2], :2], pars[[0, 2], :2] * 2.5) and np.array_equal(out[[0, 2], 2], pars[[0, 2], 2])


def test_host_and_device_entry_points_agree_bit_for_bit():
    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.utils.misc import fitcleanbeam, fitcleanbeam_dev

    cube = ref.case("I")
    d = _lib.DeviceArray.from_host(cube)
    try:
        a, b = fitcleanbeam(cube), fitcleanbeam_dev(d)
    finally:
        d.free()
    print(a, b)
    assert np.array_equal(a, b, equal_nan=True)
    with pytest.raises(TypeError):
        fitcleanbeam_dev(cube)


def test_sizes_around_the_peak_kernels_block():
    """k_cb_peak on cubes smaller than one block, of an odd size and of several blocks with a tail: the peak is found where
    it is (last element included) and the fit of a planted beam does not move."""
    from pfb_imaging_amd.utils.misc import _cleanbeam_raw

    for shape in ((9, 11), (63, 65), (127, 129)):
        psf = ref.beam(shape, (3.0, 2.0, 0.5), 0.0)
        want, _ = _cleanbeam_raw(psf[None])
        spiked = psf.copy()
        spiked[-1, -1] = 4.0   # the cube's last element becomes the peak: everything else is now below level / 4
        with pytest.raises(ValueError, match="centre pixel"):
            _cleanbeam_raw(spiked[None])
        got, _ = _cleanbeam_raw((psf * 0.25)[None])
        print(shape, want, got)
        assert np.all(np.abs(got - want) <= 1e-12)


def test_refusals():
    import time

    from pfb_imaging_amd.utils.misc import fitcleanbeam

    a = ref.case("A")[0]
    low = a.copy()
    low[64, 64] = 0.4
    low[10, 10] = 1.0
    with pytest.raises(ValueError, match="centre pixel"):
        fitcleanbeam(low[None])
    with pytest.raises(ValueError, match="positive"):
        fitcleanbeam(-(a + 1.0)[None])
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match="256"):
        fitcleanbeam(np.ones((1, 600, 600)))
    dt = time.perf_counter() - t0
    print(f"600 x 600 plateau refused after {dt:.3f} s")
    assert dt < 2.0
    with pytest.raises(ValueError):
        fitcleanbeam(np.ones((4, 4)))


def test_psfparsn_is_opt_in():
    from pfb_imaging_amd.operators.gridder import image_data_products_arrays
    from pfb_imaging_amd.utils import synth
    from pfb_imaging_amd.utils.misc import fitcleanbeam

    c = synth.make_case(3000, 2, 40, zscale=0.2, seed=11)
    cell = c["cell"] * 30.0
    nx, ny = c["nx"], c["ny"]
    args = (c["uvw"], c["freq"], c["vis"][None], c["wgt"][None], c["mask"], nx, ny, 2 * nx, 2 * ny, cell, cell)
    off, _ = image_data_products_arrays(*args, do_residual=False)
    on, _ = image_data_products_arrays(*args, do_residual=False, do_psfpars=True)
    print("PSFPARSN", on["PSFPARSN"])
    assert sorted(off) == ["DIRTY", "MASK", "PSF", "PSFHAT", "UVW", "WEIGHT", "WSUM"]
    assert sorted(on) == sorted(list(off) + ["PSFPARSN"])
    assert on["PSF"].shape == off["PSF"].shape == (1, 2 * nx, 2 * ny)
    assert on["PSFPARSN"].shape == (1, 3) and np.isfinite(on["PSFPARSN"]).all()
    assert np.array_equal(on["PSFPARSN"], fitcleanbeam(on["PSF"], pixsize=1.0))
    with pytest.raises(ValueError, match="do_psf"):
        image_data_products_arrays(*args, do_psf=False, do_psfpars=True)


def test_grid_partition_psfparsn_is_opt_in(golden_dir):
    from pfb_imaging_amd.operators.gridder import grid_partition
    from pfb_imaging_amd.utils.misc import fitcleanbeam

    gold = np.load(f"{golden_dir}/synth_partition.npz")
    part = {"UVW": gold["uvw"], "FREQ": gold["freq"], "VIS": gold["vis"], "WEIGHT": gold["wgt"], "MASK": gold["mask"],
            "BEAM": np.ones((1, 16, 16))}
    kw = dict(nx=16, ny=16, nx_psf=32, ny_psf=32, cell_rad=float(gold["cell"]), robustness=None)
    off, on = grid_partition(part, None, **kw), grid_partition(part, None, do_psfpars=True, **kw)
    print("PSFPARSN", on["PSFPARSN"])
    assert sorted(off) == ["BEAM", "DIRTY", "PSF", "PSFHAT", "WEIGHT", "WSUM"]
    assert sorted(on) == sorted(list(off) + ["PSFPARSN"])
    assert on["PSFPARSN"].shape == (1, 3) and np.isfinite(on["PSFPARSN"]).all()
    assert np.array_equal(on["PSFPARSN"], fitcleanbeam(on["PSF"], pixsize=1.0))
