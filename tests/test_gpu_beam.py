"""Device primary beams (pfb_imaging_amd.utils.beam, csrc/beam.hip) against scipy's answers (tests/golden/beam_pins.npz)
at the tolerances of test_beam_cpu.py, and against the numpy restatement (tests/_beam_ref.py) everywhere at 1e-12 max.

Shapes beyond the fixtures are the smallest that take the kernels' other paths: an odd ``ny`` (rows of the regrid that
start on an odd element and leave their first value in an 8-byte store), ``ny = 1``, a row longer than one workgroup's
512 outputs, more rows than one step of the launch's row walk; for the prefilter a line of one segment (57 samples), of two without and with a far end beyond the first
tile (88, 120) and of three (174: a segment warmed up on both sides), more lines than one tile of 32; more angles than
one staging of 64.
"""

import ctypes as ct
import functools

import numpy as np
import pytest

from tests import _beam_ref as ref
from tests.test_beam_cpu import EPS, REGRID_CASES, REGRID_TOL, ROT_SETS, ROT_SHAPES, check_rotation, pins, regrid_case, rot_case

pytestmark = pytest.mark.gpu

RESTATEMENT_TOL = 1e-12


@functools.lru_cache(maxsize=None)
def restated_rotation(shape, key):
    beam0, angles, _ = rot_case(shape, key)
    out = ref.rotate_mean(beam0, angles)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("grid,form", REGRID_CASES)
def test_regrid_matches_scipy_and_restatement(grid, form):
    from pfb_imaging_amd.utils.beam import eval_beam

    beam, l_in, m_in, lo, mo, exp = regrid_case(grid, form)
    got = eval_beam(beam, l_in, m_in, lo, mo)
    assert got.shape == exp.shape and got.dtype == np.float64
    scale = np.abs(beam).max()
    err = np.abs(got - exp).max() / scale
    err_r = np.abs(got - ref.regrid(beam, l_in, m_in, lo, mo)).max() / scale
    print(f"regrid {grid} {form}: {err / EPS:.2f} eps from scipy, {err_r / EPS:.2f} eps from the restatement")
    assert err <= REGRID_TOL
    assert err_r <= RESTATEMENT_TOL
    assert ((got == 1.0) == (exp == 1.0)).all()
    # one correlation, reference signature: a 2-D beam in, a 2-D image out
    one = eval_beam(beam[1], l_in, m_in, lo, mo)
    assert one.shape == exp.shape[1:] and (one == got[1]).all()


@pytest.mark.parametrize("nx,ny", [(7, 45), (5, 1), (3, 1031), (2, 2), (300, 5001), (70000, 1)])
def test_regrid_row_starts_and_tails(nx, ny):
    """Odd rows (every other row of every correlation begins on an odd element), one column, more than one workgroup per row,
    more rows than a launch takes in one step (900 rows of 10 workgroups against 8192 workgroups in the separable form;
    210000 rows against a grid of 65534 in the 2-D form)."""
    from pfb_imaging_amd.utils.beam import eval_beam

    rng = np.random.default_rng(nx * 1000 + ny)
    l_in, m_in = np.sort(rng.uniform(-1, 1, 9)), np.sort(rng.uniform(-1, 1, 6))
    beam = rng.standard_normal((3, 9, 6))
    l_out, m_out = rng.uniform(-1.2, 1.2, nx), rng.uniform(-1.2, 1.2, ny)
    m_out[0], l_out[-1] = m_in[-1], l_in[0]
    want = ref.regrid(beam, l_in, m_in, l_out, m_out)
    got = eval_beam(beam, l_in, m_in, l_out, m_out)
    assert np.abs(got - want).max() <= RESTATEMENT_TOL * np.abs(beam).max()
    ll, mm = np.meshgrid(l_out, m_out, indexing="ij")
    assert (eval_beam(beam, l_in, m_in, ll, mm) == got).all()


def test_regrid_forms_agree_exactly_and_ones_are_exact():
    from pfb_imaging_amd.utils.beam import eval_beam

    beam, l_in, m_in, l_out, m_out, _ = regrid_case("g33x29", "sep")
    ll, mm = np.meshgrid(l_out, m_out, indexing="ij")
    sep, gen = eval_beam(beam, l_in, m_in, l_out, m_out), eval_beam(beam, l_in, m_in, ll, mm)
    assert (sep == gen).all()
    stack = np.array([beam[0], np.ones_like(beam[0]), beam[1]])
    for lo, mo in ((l_out, m_out), (ll, mm)):
        out = eval_beam(stack, l_in, m_in, lo, mo)
        assert (out[1] == 1.0).all() and (out[0] == sep[0]).all() and (out[2] == sep[1]).all()
        assert (eval_beam(np.ones((33, 29)), l_in, m_in, lo, mo) == 1.0).all()
    almost = np.ones((33, 29))
    almost[-1, -1] = 1.0 + 2.0**-52  # one value in the last place: not the short-circuit
    assert eval_beam(almost, l_in, m_in, l_in, m_in)[-1, -1] == almost[-1, -1]


def test_regrid_refusals():
    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.utils.beam import eval_beam

    beam, l_in, m_in, l_out, m_out, _ = regrid_case("g5x4", "sep")
    with pytest.raises(ValueError, match="Only 1 or 2D coordinates supported for beam evaluation"):
        eval_beam(beam[0], l_in, m_in, np.zeros((2, 2, 2)), np.zeros((2, 2, 2)))
    for bad in (l_in[::-1], np.array([-1.0, -0.6, -0.6, 0.45, 1.3])):
        with pytest.raises(ValueError, match="strictly ascending"):
            eval_beam(beam[0], bad, m_in, l_out, m_out)
    with pytest.raises(ValueError, match="strictly ascending"):
        eval_beam(beam[0], l_in, m_in[::-1], l_out, m_out)
    # the library itself refuses them too, and NULL
    L, out, bad = _lib.lib(), np.empty((64, 48)), np.ascontiguousarray(l_in[::-1])
    b0 = np.ascontiguousarray(beam[0])
    args = (_lib.i32(1), _lib.i64(5), _lib.i64(4))
    tail = (ct.c_int(0), _lib.i64(64), _lib.i64(48), _lib.ptr(out), None)
    assert L.pfbhip_beam_regrid(_lib.ptr(b0), *args, _lib.ptr(bad), _lib.ptr(m_in), _lib.ptr(l_out), _lib.ptr(m_out), *tail) == 1
    assert "strictly ascending" in _lib.last_error()
    assert L.pfbhip_beam_regrid(None, *args, _lib.ptr(l_in), _lib.ptr(m_in), _lib.ptr(l_out), _lib.ptr(m_out), *tail) == 1
    assert "NULL" in _lib.last_error()
    assert L.pfbhip_beam_rotate_mean(_lib.ptr(b0), _lib.i32(1), _lib.i64(5), _lib.i64(4), None, _lib.i32(1), _lib.ptr(out), None) == 1


@pytest.mark.parametrize("key", ROT_SETS)
@pytest.mark.parametrize("shape", ROT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rotation_matches_scipy_and_restatement(shape, key):
    from pfb_imaging_amd.utils.beam import rotate_mean

    beam0, angles, exp = rot_case(shape, key)
    got = rotate_mean(beam0, angles)
    assert got.shape == beam0.shape and got.dtype == np.float64
    check_rotation(got, exp, beam0, angles)
    err_r = np.abs(got - restated_rotation(shape, key)).max() / np.abs(beam0).max()
    print(f"from the restatement: {err_r:.2e}")
    assert err_r <= RESTATEMENT_TOL
    if key == "zero":
        assert np.abs(got - beam0).max() <= 1e-12 * np.abs(beam0).max()


def test_rotation_default_angles_stack_long_lines_and_many_angles():
    from pfb_imaging_amd.utils.beam import rotate_mean

    rng = np.random.default_rng(5)
    u, v = np.meshgrid(np.linspace(-1, 1, 150), np.linspace(-1, 1, 70), indexing="ij")
    stack = np.array([np.exp(-(u**2 / 0.3 + v**2 / 0.5)), 0.7 * np.exp(-(u**2 / 0.6 + v**2 / 0.2))])
    stack += 0.01 * rng.standard_normal(stack.shape)
    got = rotate_mean(stack)  # linspace(0, 359, 25)
    want = ref.rotate_mean(stack)
    assert got.shape == stack.shape
    assert np.abs(got - want).max() <= RESTATEMENT_TOL * np.abs(stack).max()
    assert (rotate_mean(stack[1]) == got[1]).all()
    small, angles = rot_case((33, 33), "zero")[0], np.linspace(-400.0, 725.0, 70)
    assert np.abs(rotate_mean(small, angles) - ref.rotate_mean(small, angles)).max() <= RESTATEMENT_TOL * np.abs(small).max()


def test_grid_partition_regrids_the_beam_on_the_device(golden_dir):
    from pfb_imaging_amd.operators.gridder import grid_partition

    d = pins()
    gold = np.load(f"{golden_dir}/synth_partition.npz")
    two = lambda a: np.concatenate([a, a], axis=0)  # noqa: E731  (the synthetic partition has one correlation)
    part = {"UVW": gold["uvw"], "FREQ": gold["freq"], "VIS": two(gold["vis"]), "WEIGHT": two(gold["wgt"]), "MASK": gold["mask"],
            "BEAM": d["gp_beam"].astype(np.float64), "l_beam": d["gp_l_beam"], "m_beam": d["gp_m_beam"]}
    nx, ny = int(d["gp_nx"]), int(d["gp_ny"])
    out = grid_partition(part, None, nx=nx, ny=ny, nx_psf=96, ny_psf=72, cell_rad=float(d["gp_cell_rad"]), robustness=None)
    assert out["BEAM"].shape == (2, nx, ny) and out["DIRTY"].shape == (2, nx, ny)
    assert np.abs(out["BEAM"] - d["gp_out"]).max() <= REGRID_TOL * np.abs(d["gp_beam"]).max()
    assert (out["BEAM"][1] == 1.0).all()
