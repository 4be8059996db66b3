"""CPU tests of the Gaussian-resolution convolution and the restore step: the reference-run fixtures
(tests/golden/restore_pins.npz, restore_edge_pins.npz), the guard that the cases of tests/_restore_ref.py reach every launch
form of csrc/restore.hip, the host helpers of utils/misc.py, the numpy statement of tests/_restore_ref.py and the error
returns of ``pfbhip_gaussconv_*`` that need no device."""

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


@pytest.fixture(scope="module")
def edge_pins(golden_dir):
    return np.load(f"{golden_dir}/restore_edge_pins.npz")


def test_fixture_regenerates_bit_for_bit(pins, edge_pins):
    """Where the reference checkout is at hand, the generator reproduces every stored array of both fixtures exactly."""
    spec = importlib.util.spec_from_file_location("make_restore_pins", os.path.join(HERE, "golden", "make_restore_pins.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    if not os.path.isdir(gen.REF):
        pytest.skip("the reference checkout is not on this machine: the committed fixture travels instead")
    for again, stored in ((gen.compute(), pins), (gen.compute_edge(), edge_pins)):
        assert sorted(again) == sorted(stored.files)
        for k in stored.files:
            assert np.array_equal(np.asarray(again[k]), stored[k]), k


def test_edge_fixture_holds_outputs_scalars_and_conditions_only(edge_pins):
    want = {"cites", "K_np", "K_disagreement", "K_min_over_max_thishat"}
    for tag, (name, _) in ref.EDGE_RUNS.items():
        want |= {f"{tag}_np", f"{tag}_disagreement"}
        if ref.case(name)["gausspari"] is not None:
            want.add(f"{tag}_min_over_max_thishat")
    assert set(edge_pins.files) == want
    assert all(edge_pins[k].dtype.kind == "f" for k in edge_pins.files if k != "cites")
    assert all(edge_pins[k].shape == () and float(edge_pins[k]) <= 1e-8 for k in edge_pins.files if k.endswith("_disagreement"))
    assert sum(edge_pins[k].size for k in edge_pins.files if k != "cites") < 40_000


# ---- the guard of the case table: cases A-L together reach every launch form of csrc/restore.hip ------------------------------
CASES = ["A", "B", "C", "D", "E", "F", "G", "H", "H_ratio", "I", "J", "J_scaled", "K", "L"]


def test_cases_reach_every_kernel_form():
    """A later edit of tests/_restore_ref.py cannot lose a form silently: this fails if one of E-L goes, or if an odd length
    of theirs is made even."""
    assert {c for c, _ in ref.RUNS.values()} | set(ref.RESTORES) == set(CASES)
    forms = {name: ref.kernel_forms(*ref.geometry(name)) for name in CASES}
    for name in ("E", "F", "G", "H", "I", "J", "K"):  # the table as the issue gives it, to the pad
        assert name in forms
    assert (forms["E"]["nfft"], forms["E"]["pads"]) == ((8, 375), ((0, 1), (37, 37)))
    assert (forms["F"]["nfft"], forms["F"]["pads"]) == ((6, 625), ((0, 1), (52, 53)))
    assert (forms["G"]["nfft"], forms["G"]["pads"]) == ((9, 810), ((1, 2), (135, 135)))
    assert (forms["H"]["nfft"], forms["H"]["pads"]) == ((3, 4), ((0, 1), (0, 1)))
    assert (forms["I"]["nfft"], forms["I"]["pads"]) == ((6, 512), ((0, 1), (42, 43)))
    assert forms["J"] == forms["E"] and forms["J_scaled"] == forms["E"] and forms["K"] == dict(forms["E"], nband=2)
    assert (forms["F"]["pad_trips"], forms["I"]["pad_v"], forms["I"]["pad_trips"]) == (3, 2, 1)  # 512: one trip, filled to its last pair

    def reached(what):
        return {(f[f"{what}_v"], min(f[f"{what}_trips"], 2)) for f in forms.values()}

    assert reached("pad") == {(1, 1), (1, 2), (2, 1), (2, 2)}, reached("pad")
    assert reached("crop") == {(1, 1), (1, 2), (2, 1), (2, 2)}, reached("crop")
    for axis in (0, 1):
        kinds = {("zero" if left == 0 else "less" if left < right else "equal" if left == right else "more")
                 for left, right in (f["pads"][axis] for f in forms.values())}
        assert kinds == {"zero", "less", "equal"}, (axis, kinds)
        assert {f["left_pad_zero"][axis] for f in forms.values()} == {False, True}
        assert {f["odd"][axis] for f in forms.values()} == {False, True}
    assert any(f["nband"] == 1 for f in forms.values())
    assert any(ref.geometry(n)[1] % 2 == 1 for n in CASES)  # an odd nx
    # a per-band gaussparf together with gausspari, and a negative axis scale
    assert any(c["gaussparf"].ndim == 2 and c["gausspari"] is not None for c in (ref.case(n) for n, _ in ref.RUNS.values()))
    assert ref.case("J_scaled")["yy"][0, -1] < 0 < ref.case("J_scaled")["xx"][-1, 0] and ref.case("J_scaled")["gaussparf"][2] != 0
    from pfb_imaging_amd.utils.misc import _axis_scales

    js = ref.case("J_scaled")  # its grids are scaled pixel offsets: convolve2gaussres renders them on the device, step and sign
    assert _axis_scales(js["xx"], js["yy"], 7, 301) == ref.J_SCALE and ref.J_SCALE[1] < 0
    k = ref.case("K")
    assert not np.allclose(k["gaussparf"][0], k["gausspari"][0]) and np.allclose(k["gaussparf"][1], k["gausspari"][1])
    assert np.array_equal(np.log2(k["wsum"]) % 1, [0, 0]) and set(k["wsum"]) != {1.0}


def _ratio_runs():
    """(tag, dict with image, grids, gausspari and pfrac, norm_kernel) of every convolution with a ratio, K's band 0 included"""
    runs = [(tag, ref.case(name), norm) for tag, (name, norm) in ref.RUNS.items() if ref.case(name)["gausspari"] is not None]
    k = ref.case("K")
    xx, yy = ref.offsets(*k["model"].shape[1:])
    return runs + [("K", dict(image=k["residual"][:1], xx=xx, yy=yy, gausspari=k["gausspari"][:1], pfrac=0.2), False)]


def test_ratio_cases_divide_safely_and_take_both_branches_of_the_division(pins, edge_pins):
    """Conditions on the INPUTS, counted from the statement's own spectra.  The device divides as numpy does (Smith): by the
    real part where |Re| >= |Im|, else by the imaginary part.  Where the kernel's centre lands on index 0 of both padded axes
    (case C) thishat is almost real and the second branch is never taken; where it lands on index -1 (n odd, nfft even) thishat
    carries a phase ramp and about half of the elements take it."""
    share = {}
    for tag, c, norm in _ratio_runs():
        hat = ref.thishat(c, norm)
        mag = np.abs(hat)
        ratio = mag.min(axis=(1, 2)) / mag.max(axis=(1, 2))
        share[tag] = float(np.mean(np.abs(hat.real) < np.abs(hat.imag)))
        print(f"{tag}: min / max |thishat| {ratio.min():.2e}; |Re| < |Im| on {np.sum(np.abs(hat.real) < np.abs(hat.imag))} of {hat.size}")
        assert ratio.min() >= 1e-6, tag
        stored = pins["C_min_over_max_thishat"] if tag == "C" else edge_pins[f"{tag}_min_over_max_thishat"]
        assert np.allclose(ratio, stored, rtol=1e-9, atol=0)
    assert share["C"] == 0.0  # what the cases before E left unreached
    assert sum(s >= 0.25 for s in share.values()) >= 2 and share["I"] >= 0.25 and share["J"] >= 0.25, share
    hat_i = ref.thishat(ref.case("I"))
    assert int(np.sum(np.abs(hat_i.real) < np.abs(hat_i.imag))) * 2 == hat_i.size == 1542


@pytest.mark.parametrize("name", CASES)
def test_odd_padded_lengths_see_the_two_shifts_exchanged(name):
    """ifftshift and fftshift differ by one pixel on an axis of odd length and not at all on an even one.  A case with an odd
    padded length must tell them apart: the statement with the shift on load replaced by the other one, and with the shift on
    store replaced, is far from the statement.  With BOTH exchanged the image moves one pixel, the kernel one, the output one
    back: a product moves by one pixel, which is asserted too, but in a ratio the two kernels' displacements cancel and the
    statement is unchanged to rounding (2.8e-15 for case C), so that exchange is no condition on a ratio case."""
    forms = ref.kernel_forms(*ref.geometry(name))
    c = ref.case(name)
    load, store = ref.SHIFTS

    def run(shifts):
        if name in ref.RESTORES:
            return ref.restore(**c, shifts=shifts)
        return ref.convolve(c["image"], c["xx"], c["yy"], c["gaussparf"], c["gausspari"], c["pfrac"], shifts=shifts)

    right = run(ref.SHIFTS)
    diffs = {"load": ref.rel_max(run((store, store)), right), "store": ref.rel_max(run((load, load)), right)}
    if name not in ref.RESTORES and c["gausspari"] is None:
        diffs["both"] = ref.rel_max(run((store, load)), right)
    print(f"{name}: padded {forms['nfft']}, a wrong shift moves the statement by "
          + ", ".join(f"{v:.3e} ({k})" for k, v in diffs.items()) + " of its max norm")
    if any(forms["odd"]):
        assert min(diffs.values()) > 1e-2
    else:
        assert max(diffs.values()) == 0.0


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


@pytest.mark.parametrize("tag", list(ref.EDGE_RUNS) + ["K"])
def test_numpy_statement_agrees_with_the_edge_reference_runs(edge_pins, tag):
    if tag == "K":
        got = ref.restore(**ref.case("K"))
    else:
        name, norm = ref.EDGE_RUNS[tag]
        c = ref.case(name)
        got = ref.convolve(c["image"], c["xx"], c["yy"], c["gaussparf"], c["gausspari"], c["pfrac"], norm)
    err = ref.rel_max(got, edge_pins[f"{tag}_np"])
    print(f"{tag}: statement vs numpy-FFT run {err:.3e}, stored disagreement {float(edge_pins[f'{tag}_disagreement']):.3e}")
    assert got.shape == edge_pins[f"{tag}_np"].shape and err <= ref.bound(edge_pins[f"{tag}_disagreement"])


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
