"""The numpy restatement of the primary-beam operations (tests/_beam_ref.py) against scipy's answers
(tests/golden/beam_pins.npz, written by tests/golden/make_beam_pins.py from the reference's eval_beam and from
ndimage.rotate).  The device tests (test_gpu_beam.py) lean on both.

Tolerances:
  regrid         64 eps max|beam|: each value is a convex combination of four values formed in about six roundings in
                 either evaluation order.
  rotation mean  1e-12 max|beam0| on pixels all of whose samples lie inside the padded array (the coefficients agree with
                 scipy's to 7e-15).  On the other pixels -- they exist at (64, 64) and (96, 80) only -- the restatement was
                 measured at 9.5e-17 and 1.4e-16 max|beam0| from scipy with the rule its docstring states; ten times the
                 larger figure is asserted (OUTSIDE_TOL), far below the cap of 1e-8.
"""

import functools
import os

import numpy as np
import pytest

from tests import _beam_ref as ref

EPS = 2.0**-52
REGRID_TOL = 64 * EPS
INSIDE_TOL = 1e-12
OUTSIDE_TOL = 1.4e-15  # 10 x the measured 1.36e-16
ROT_SHAPES = ((33, 33), (40, 40), (48, 37), (64, 64), (96, 80))
ROT_SETS = ("lin25", "zero", "q90_180")
REGRID_CASES = [(g, form) for g in ("g5x4", "g33x29") for form in ("sep", "2d")]


@functools.lru_cache(maxsize=None)
def pins():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_pins.npz")
    with np.load(path) as d:
        return {k: d[k] for k in d.files}


def regrid_case(grid, form):
    """(beam, l_in, m_in, l_out, m_out, expected) of one fixture case, inputs as float64."""
    d = pins()
    lo, mo = (d[f"rg_{grid}_l_out"], d[f"rg_{grid}_m_out"]) if form == "sep" else (d[f"rg_{grid}_ll"], d[f"rg_{grid}_mm"])
    return d[f"rg_{grid}_beam"].astype(np.float64), d[f"rg_{grid}_l_in"], d[f"rg_{grid}_m_in"], lo, mo, d[f"rg_{grid}_{form}"]


def rot_case(shape, key):
    d = pins()
    tag = f"rot_{shape[0]}x{shape[1]}"
    return d[f"{tag}_beam0"].astype(np.float64), d[f"rot_angles_{key}"], d[f"{tag}_{key}"]


def check_rotation(got, expected, beam0, angles):
    """The two bounds of the module docstring; returns the two measured figures relative to max|beam0|."""
    scale = np.abs(beam0).max()
    inside = ref.inside_mask(beam0.shape, angles)
    err = np.abs(got - expected) / scale
    e_in = err[inside].max()
    e_out = err[~inside].max() if (~inside).any() else 0.0
    print(f"rotation {beam0.shape} x {angles.size} angles: inside {e_in:.2e}, outside {e_out:.2e} ({(~inside).sum()} pixels)")
    assert e_in <= INSIDE_TOL
    assert e_out <= OUTSIDE_TOL
    return e_in, e_out


def test_fixture_cases_are_what_they_claim():
    d = pins()
    for grid, form in REGRID_CASES:
        beam, l_in, m_in, lo, mo, exp = regrid_case(grid, form)
        assert beam.shape[0] == 2 and exp.shape == (2, 64, 48)
        ll, mm = (lo[:, None] + 0 * mo[None, :], 0 * lo[:, None] + mo[None, :]) if form == "sep" else (lo, mo)
        for nodes, x in ((l_in, ll), (m_in, mm)):  # all four edges straddled; points exactly on first, last, interior nodes
            assert (x < nodes[0]).any() and (x > nodes[-1]).any()
            assert (x == nodes[0]).any() and (x == nodes[-1]).any() and np.isin(x, nodes[1:-1]).any()
    assert (np.diff(np.diff(d["rg_g5x4_l_in"])) != 0).any()  # non-uniform
    assert (d["gp_beam"][1] == 1.0).all() and d["gp_out"].shape == (2, 64, 48)
    # pixels with samples outside the padded array exist exactly at the two large shapes
    for shape in ROT_SHAPES:
        outside = (~ref.inside_mask(shape, d["rot_angles_lin25"])).sum()
        assert (outside > 0) == (shape in ((64, 64), (96, 80)))
    assert "eval_beam" in " ".join(d["cites"])


@pytest.mark.parametrize("grid,form", REGRID_CASES)
def test_regrid_restatement_matches_scipy(grid, form):
    beam, l_in, m_in, lo, mo, exp = regrid_case(grid, form)
    got = ref.regrid(beam, l_in, m_in, lo, mo)
    err = np.abs(got - exp).max() / np.abs(beam).max()
    print(f"regrid {grid} {form}: {err / EPS:.2f} eps")
    assert err <= REGRID_TOL
    assert ((got == 1.0) == (exp == 1.0)).all()  # the fill value lands on the same points, the last node is inside


def test_regrid_restatement_grid_partition_case_and_ones():
    d = pins()
    nx, ny, cell = int(d["gp_nx"]), int(d["gp_ny"]), float(d["gp_cell_rad"])
    x, y = np.rad2deg((-nx / 2 + np.arange(nx)) * cell), np.rad2deg((-ny / 2 + np.arange(ny)) * cell)
    beam = d["gp_beam"].astype(np.float64)
    got = ref.regrid(beam, d["gp_l_beam"], d["gp_m_beam"], x, y)
    assert np.abs(got - d["gp_out"]).max() <= REGRID_TOL * np.abs(beam).max()
    assert (got[1] == 1.0).all()
    with pytest.raises(ValueError, match="Only 1 or 2D coordinates"):
        ref.regrid(beam[0], d["gp_l_beam"], d["gp_m_beam"], np.zeros((2, 2, 2)), np.zeros((2, 2, 2)))


@pytest.mark.parametrize("key", ROT_SETS)
@pytest.mark.parametrize("shape", ROT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rotation_restatement_matches_scipy(shape, key):
    beam0, angles, exp = rot_case(shape, key)
    check_rotation(ref.rotate_mean(beam0, angles), exp, beam0, angles)
