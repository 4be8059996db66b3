"""The shape tables of tests/test_gpu_rowfft_shapes.py are exactly the instantiation lists of csrc/rowfft.hpp: a shape added to
RF_FOR_SHAPES / RF_FOR_SHAPES2 without a test case fails here, on a machine without a GPU."""

import math
import os
import re

from tests import test_gpu_rowfft_shapes as sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pfb-imaging_amd", "csrc", "rowfft.hpp")


def _macro_shapes(name):
    src = open(HEADER).read()
    m = re.search(r"#define " + name + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", src)
    assert m, name
    return [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", m.group(1))]


def _params(fn, arg):
    """values of the parametrize mark of `fn` that names `arg`"""
    for mark in fn.pytestmark:
        if mark.name == "parametrize" and mark.args[0] == arg:
            return list(mark.args[1])
    raise AssertionError((fn.__name__, arg))


def test_shape_tables_are_the_headers_lists():
    plain, doubled = _macro_shapes("RF_FOR_SHAPES"), _macro_shapes("RF_FOR_SHAPES2")
    assert len(plain) == len(set(plain)) and len(doubled) == len(set(doubled))
    assert sorted(sweep.RF_SHAPES) == sorted(plain)
    assert sorted(sweep.RF_DOUBLED) == sorted(doubled)
    ns = sorted(lead << k for lead, k in plain)
    ns2 = sorted(2 * (lead << k) for lead, k in doubled)
    assert sweep.PLAIN_NS == ns and sweep.DOUBLED_NS == ns2
    # every test of the sweep that runs per shape runs every shape
    assert sorted(_params(sweep.test_plain_kernel_both_families_vs_numpy, "n")) == sorted(ns + ns2)
    assert _params(sweep.test_plain_kernel_both_families_vs_numpy, "family") == [0, 1]
    for fn in (sweep.test_second_axis_composite_planes, sweep.test_second_axis_es_planes_separable,
               sweep.test_second_axis_single_plane_launches, sweep.test_first_axis_transposing):
        assert sorted(_params(fn, "n")) == ns, fn.__name__
    assert sorted(sweep.FUSED_NX) == ns
    # the smallest shape of every leading factor
    leads = sorted({lead for lead, _ in plain})
    assert sweep.SMALLEST_NS == sorted(min(l << k for l, k in plain if l == lead) for lead in leads)


def test_image_sizes_land_on_their_shape():
    """Both grid candidates of the plan (csrc/gridder.hip: choose_kernel; csrc/eskernel.cpp: grid_size) at the length's sigma
    are the shape under test, for the image sizes the sweep uses; the sizes are even and no multiple of 64."""
    lengths = sweep.PLAIN_NS + sweep.DOUBLED_NS

    def candidates(npix, sigma):
        return sweep.grid_size(npix, sigma), min(n for n in lengths if n >= sigma * npix - 1e-9)

    cases = [(n, nx, sweep.sigma_of(n)) for n, nx in sweep.FUSED_NX.items()] + [(20480, sweep.NX_20480, sweep.SIGMA)]
    cases += [(1024, nx, sigma) for sigma, nx in sweep.NY_1024.items()]
    for n, nx, sigma in cases:
        assert nx % 2 == 0 and nx % 64 != 0 and nx <= n / sigma, (n, nx)
        assert candidates(nx, sigma) == (n, n), (n, nx, candidates(nx, sigma))
    assert set(sweep.NY_1024) == {sweep.sigma_of(n) for n in sweep.PLAIN_NS}
    assert 48 <= sweep.NY_THIN <= 64 and sweep.grid_size(sweep.NY_THIN, sweep.SIGMA) == 72


def test_lds_row_reach():
    """The LDS image row of the fused kernels (lds_row_fits restates fused_row_fits with the header's RF_XPAD) fits at every
    length but those named unreachable, and those are out of reach of every oversampling the kernel table holds."""
    import json

    assert re.search(r"#define RF_XPAD 2\b", open(HEADER).read())
    table = json.load(open(os.path.join(ROOT, "oracle", "es_kernel_table.json")))["rows"]
    sigma_max = max(r["sigma"] for r in table)
    assert {sweep.sigma_of(n) for n in sweep.PLAIN_NS} <= {r["sigma"] for r in table if r["W"] == 13}
    for n in sweep.PLAIN_NS:
        assert sweep.lds_row_fits(n, sweep.FUSED_NX[n]) == (n not in sweep.NO_LDS_ROW), n
    for n in sweep.NO_LDS_ROW:  # (an image of fewer than n / sigma_max pixels lands on a shorter length)
        assert not sweep.lds_row_fits(n, math.floor(n / sigma_max) - 2), n
