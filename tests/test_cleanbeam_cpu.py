"""The parts of the clean-beam fit that need no GPU: the exported symbols and the record's layout, the finishing step
(swap rule, pixel size, NaN rows), the opt-in switches, and -- with scipy -- that the committed pins are what
tests/golden/make_cleanbeam_pins.py writes and that the device's iteration, restated in numpy, meets the bounds the GPU
test sets."""

import ctypes as ct
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cleanbeam_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_cleanbeam_symbols():
    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.utils.misc import fitcleanbeam, fitcleanbeam_dev  # noqa: F401

    L = _lib.lib()
    for name in ("pfbhip_cleanbeam_fit", "pfbhip_cleanbeam_fit_dev"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    # invalid arguments come back through the status channel before any device work
    assert L.pfbhip_cleanbeam_fit(None, _lib.i64(1), _lib.i64(8), _lib.i64(8), _lib.f64(0.5), _lib.f64(10.0), None, None) == 1
    assert "NULL" in _lib.last_error()
    buf = np.zeros(3)
    assert L.pfbhip_cleanbeam_fit(_lib.ptr(buf), _lib.i64(0), _lib.i64(8), _lib.i64(8), _lib.f64(0.5), _lib.f64(10.0),
                                  _lib.ptr(buf), None) == 1
    assert "shape" in _lib.last_error()


def test_info_record_matches_the_header(tmp_path):
    from pfb_imaging_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pfbhip.h"\nint main(void){\n'
                   'printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(pfbhip_cleanbeam_info), offsetof(pfbhip_cleanbeam_info, nlobe),'
                   " offsetof(pfbhip_cleanbeam_info, nfit), offsetof(pfbhip_cleanbeam_info, f), offsetof(pfbhip_cleanbeam_info, p0),"
                   " PFBHIP_CB_CONVERGED, PFBHIP_CB_ALL_ZERO, PFBHIP_CB_LOBE_TOO_WIDE);\nreturn 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    C = _lib.CleanbeamInfo
    names = _lib.CB_STATUS_NAMES
    assert out == [ct.sizeof(C), C.nlobe.offset, C.nfit.offset, C.f.offset, C.p0.offset, names.index("converged"),
                   names.index("all_zero"), names.index("lobe_too_wide")]
    assert len(names) == 8


def test_finishing_step():
    from pfb_imaging_amd.utils.misc import _finish_cleanbeam

    raw = np.array([[6.0, 3.5, 0.7], [np.nan, np.nan, np.nan], [3.0, 5.0, 0.25], [4.0, 4.0, 1.0]])
    before = raw.copy()
    out = _finish_cleanbeam(raw, pixsize=2.0)
    assert np.array_equal(raw, before, equal_nan=True)             # the input is left alone
    assert np.array_equal(out[0], [12.0, 7.0, 0.7])                # axes in order: scaled only
    assert np.isnan(out[1]).all()                                  # an all-zero band
    assert np.array_equal(out[2], [10.0, 6.0, 0.25 + np.pi / 2])   # p[0] < p[1]: swapped, pa + pi / 2 (misc.py:619-622)
    assert np.array_equal(out[3], [8.0, 8.0, 1.0])                 # p[0] == p[1] counts as in order (misc.py:615)
    assert _finish_cleanbeam([3.0, 5.0, 0.0]).shape == (1, 3)


def test_switches_default_off():
    from pfb_imaging_amd.operators import gridder
    from pfb_imaging_amd.utils import misc

    for fn in (gridder.image_data_products_arrays, gridder.grid_partition):
        assert inspect.signature(fn).parameters["do_psfpars"].default is False
    sig = inspect.signature(misc.fitcleanbeam)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("level", 0.5), ("pixsize", 1.0), ("nsigma", 10.0)]
    assert list(inspect.signature(misc.fitcleanbeam_dev).parameters)[1:] == ["level", "pixsize", "nsigma"]


def test_cases_are_what_they_claim():
    """The cases' own properties, without scipy: no diagonal leak and no island in C's lobe, a one-pixel-wide spiral with
    at least six turns in H, a three-pixel lobe with a floored minor axis and a start on the bound in D."""
    c = ref.problem("C")
    plain = ref.main_lobe(ref.normalised(ref.beam(*ref.BEAMS["C"])))
    assert np.array_equal(c["lobe"], plain) and (c["psfv"] > ref.LEVEL).sum() == plain.sum() + 17
    h = ref.case("H")[0] > 0.5
    assert ref.main_lobe(ref.normalised(ref.case("H")[0])).sum() == h.sum() > 800
    assert not (h[:-1, :-1] & h[1:, :-1] & h[:-1, 1:] & h[1:, 1:]).any()       # no 2 x 2 block: one pixel wide
    assert (np.diff(h[64, 64:].astype(int)) == 1).sum() >= 6                    # a ray from the centre crosses >= 6 arms
    d = ref.problem("D")
    assert d["lobe"].sum() == 3 and d["p0"][1] == 1.0 and d["p0"][2] == np.pi
    assert ref.window_for(ref.problem("E")["lobe"]) == 64 and ref.window_for(ref.problem("E2")["lobe"]) == 128
    assert np.array_equal(ref.case("I")[0], ref.case("A")[0]) and not ref.case("I")[1].any()


def test_pins_reproduce_and_the_restated_iteration_meets_the_bounds():
    pytest.importorskip("scipy")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_cleanbeam_pins as gen

    pins = ref.load_pins()
    for name in ref.FITTED:
        got = gen.pin_case(name)
        for k in ("nlobe", "nfit", "window"):
            assert got[k] == pins[f"{name}_{k}"], (name, k)
        np.testing.assert_allclose(got["p0"], pins[f"{name}_p0"], rtol=0, atol=1e-13)
        # (L-BFGS-B's stopping point and the minimiser may move in their last digits between scipy builds)
        np.testing.assert_allclose(got["p_ref"], pins[f"{name}_p_ref"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(got["p_exact"], pins[f"{name}_p_exact"], rtol=0, atol=1e-6)
        # the condition on the cases
        assert np.abs(pins[f"{name}_p_ref"] - pins[f"{name}_p_exact"]).max() <= 1e-4
        assert pins[f"{name}_p_exact"][0] / pins[f"{name}_p_exact"][1] >= 1.05
        # the device's iteration, in numpy, against the bounds of tests/test_gpu_cleanbeam.py
        p, f, nit, ok = ref.lm_fit(*ref.problem(name)["data"], pins[f"{name}_p0"])
        bound = np.maximum(np.abs(pins[f"{name}_p_ref"] - pins[f"{name}_p_exact"]), 10 * pins[f"{name}_exact_spread"])
        print(name, nit, ok, np.abs(p - pins[f"{name}_p_exact"]), bound)
        assert ok and nit < 50
        assert f <= pins[f"{name}_f_ref"] * (1 + 2.2e-9)
        assert np.all(np.abs(p - pins[f"{name}_p_exact"]) <= bound)
