"""CPU tests of the Gaussian-resolution convolution and the restore step: the reference-run fixture
(tests/golden/restore_pins.npz), the host helpers of utils/misc.py, the numpy statement of tests/_restore_ref.py and the
error returns of ``pfbhip_gaussconv_*`` that need no device."""

import ctypes as ct
import importlib.util
import os

import numpy as np
import pytest

from tests import _restore_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pins(golden_dir):
    return np.load(f"{golden_dir}/restore_pins.npz")


def test_fixture_regenerates_bit_for_bit(pins):
    """Where the reference checkout is at hand, the generator reproduces every stored array exactly."""
    spec = importlib.util.spec_from_file_location("make_restore_pins", os.path.join(HERE, "golden", "make_restore_pins.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    if not os.path.isdir(gen.REF):
        pytest.skip("the reference checkout is not on this machine: the committed fixture travels instead")
    again = gen.compute()
    assert sorted(again) == sorted(pins.files)
    for k in pins.files:
        assert np.array_equal(np.asarray(again[k]), pins[k]), k


def test_fixture_holds_no_source_and_records_the_standins(pins):
    cites = [str(c) for c in pins["cites"]]
    assert any("convolve2gaussres" in c for c in cites) and any("gaussian2d" in c for c in cites)
    assert any("numpy.fft" in c and "scipy.fft" in c for c in cites) and any("good_size" in c for c in cites)
    assert all(pins[k].dtype.kind in "fi" for k in pins.files if k != "cites")
    assert min(pins["C_min_over_max_thishat"]) >= 1e-6 and float(pins["C_disagreement"]) <= 1e-8


def test_padding_info_equals_the_reference_run(pins):
    from pfb_imaging_amd.utils.misc import get_padding_info

    for (nx, ny, pfrac), want in zip(pins["pad_cases"], pins["pad_out"]):
        padding, ux, uy = get_padding_info(int(nx), int(ny), float(pfrac))
        got = [padding[0][0], padding[0][1], padding[1][0], padding[1][1], ux.start, ux.stop, uy.start, uy.stop]
        assert got == [int(v) for v in want], (nx, ny, pfrac)
        assert [ref.pads(int(nx), pfrac)[1:], ref.pads(int(ny), pfrac)[1:]] == [tuple(want[0:2]), tuple(want[2:4])]


def test_gaussian2d_equals_the_reference_run(pins):
    from pfb_imaging_amd.utils.misc import gaussian2d

    for k, row in enumerate(pins["gauss_cases"]):
        par, normalise, (sx, sy) = tuple(row[:3]), bool(row[3]), row[4:6]
        xx, yy = ref.offsets(17, 22, sx, sy)
        want = pins[f"gauss_{k}"]
        got = gaussian2d(xx, yy, par, normalise=normalise)
        assert got.shape == want.shape and np.array_equal(got == 0, want == 0)  # the support is the reference's, exactly
        assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max(), k
        assert ref.rel_max(ref.gaussian(xx, yy, par, normalise), want) < 1e-13


def test_axis_scales_tell_scaled_offsets_from_other_grids():
    from pfb_imaging_amd.utils.misc import _axis_scales

    assert _axis_scales(*ref.offsets(36, 50), 36, 50) == (1.0, 1.0)
    assert _axis_scales(*ref.offsets(36, 50, 2.5e-5, -2.0e-5), 36, 50) == (2.5e-5, -2.0e-5)
    xx, yy = ref.offsets(9, 7)
    assert _axis_scales(xx + 0.5, yy, 9, 7) is None            # shifted
    assert _axis_scales(xx, yy + 1e-3 * xx, 9, 7) is None      # not separable
    assert _axis_scales(yy, xx, 9, 7) is None                  # axes swapped
    assert _axis_scales(xx[:, :5], yy[:, :5], 9, 7) is None


@pytest.mark.parametrize("case", ["A_norm0", "A_norm1", "B", "C"])
def test_numpy_statement_agrees_with_the_reference_runs(pins, case):
    c = ref.case(case[0])
    got = ref.convolve(c["image"], c["xx"], c["yy"], c["gaussparf"], c["gausspari"], c["pfrac"], case.endswith("1"))
    err = ref.rel_max(got, pins[f"{case}_np"])
    print(f"{case}: statement vs numpy-FFT run {err:.3e}, stored disagreement {float(pins[f'{case}_disagreement']):.3e}")
    assert err <= ref.bound(pins[f"{case}_disagreement"])


def test_numpy_restore_agrees_with_the_composed_reference_runs(pins):
    d = ref.case("D")
    assert np.allclose(d["gaussparf"][1], d["gausspari"][1]) and not np.allclose(d["gaussparf"][0], d["gausspari"][0])
    err = ref.rel_max(ref.restore(**d), pins["D_np"])
    print(f"D: statement vs composed numpy-FFT runs {err:.3e}, stored disagreement {float(pins['D_disagreement']):.3e}")
    assert err <= ref.bound(pins["D_disagreement"])


def test_cabi_refuses_bad_geometry_without_a_device():
    """Argument errors come back as status 1 with a message before any device work."""
    from pfb_imaging_amd import _lib
    from pfb_imaging_amd._lib import f64, i64

    L = _lib.lib()
    h = ct.c_void_p()
    for nband, nx, ny, pfrac, word in ((0, 8, 8, 0.5, "shape"), (1, 0, 8, 0.5, "shape"), (1, 8, -3, 0.5, "shape"),
                                       (1, 8, 8, float("nan"), "padding fraction"), (1, 8, 8, -0.1, "padding fraction"),
                                       (1, 100, 7, 0.0, "right pad"), (2, 16, 16, 0.01, "right pad")):
        st = L.pfbhip_gaussconv_create(i64(nband), i64(nx), i64(ny), f64(pfrac), ct.byref(h))
        assert st == 1 and not h.value and word in _lib.last_error(), (nband, nx, ny, pfrac, _lib.last_error())
    assert L.pfbhip_gaussconv_create(i64(1), i64(8), i64(8), f64(0.5), None) == 1 and "NULL" in _lib.last_error()
    v = i64(0)
    assert L.pfbhip_gaussconv_shape(None, ct.byref(v), ct.byref(v), ct.byref(v), ct.byref(v)) == 1
    assert L.pfbhip_gaussconv_apply(None, None, None, i64(1), None, i64(0), 0, f64(1), f64(1), None, None, None) == 1
    assert L.pfbhip_gaussconv_restore_dev(None, None, None, None, None, i64(0), None, i64(1), None) == 1
    assert L.pfbhip_gaussconv_debug_fill(None, 255) == 1 and "NULL" in _lib.last_error()
    assert L.pfbhip_gaussconv_destroy(None) == 0


def test_python_shells_refuse_bad_arguments_without_a_device():
    from pfb_imaging_amd.utils.misc import convolve2gaussres
    from pfb_imaging_amd.utils.restoration import restore_arrays

    xx, yy = ref.offsets(8, 8)
    img = np.zeros((2, 8, 8))
    with pytest.raises(ValueError, match="length nband"):
        convolve2gaussres(img, xx, yy, (3.0, 2.0, 0.0), gausspari=np.ones((3, 3)))
    with pytest.raises(ValueError, match="gaussparf"):
        convolve2gaussres(img, xx, yy, np.ones((5, 3)))
    with pytest.raises(ValueError, match="right pad"):
        convolve2gaussres(img, xx, yy, (3.0, 2.0, 0.0), pfrac=0.0)
    with pytest.raises(ValueError, match="gaussparf should have shape"):
        restore_arrays(img, img, np.ones(2), np.ones((2, 3)), np.ones((3, 3)))
    with pytest.raises(ValueError, match="gausspari should have shape"):
        restore_arrays(img, img, np.ones(2), np.ones((3, 3)), (3.0, 2.0, 0.0))
