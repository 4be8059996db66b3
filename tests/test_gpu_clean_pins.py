"""Hogbom and Clark CLEAN on the GPU against RUNS OF THE REFERENCE (tests/golden/clean_pins.npz, made by
tests/golden/make_clean_pins.py from the inputs of tests/_clean_cases.py), at the sizes where csrc/clean.hip changes path:
grid-stride second trips, a ragged last workgroup, the LDS / grid switch of the sub-minor loop, nband 1 and 64, ties, PSFs that
are odd, larger or smaller than twice the image.  DESIGN.md section 8 lists which kernel path each case reaches.

Class E (Hogbom; Clark with one major cycle): the reference's model bit for bit, its k and status.  Class T (Clark, several major
cycles, rocFFT inside the loop): same support, k and status, and max|model - pin| / max|pin| within ten times the reference's own
numpy.fft / scipy.fft disagreement, not below 64 eps = 1.42e-14.  Measured on an MI355X: T1 1.8e-16, T2 3.8e-16, T3 2.9e-16, each
against the bound 1.42e-14.  Class F (H6, float32 inputs): same support, k and status, the model within ten times the
reference's own float32-run / float64-run disagreement (7.9e-7; measured 8.7e-8).  What the reference does not return -- the
sub-minor count and the residual -- is compared
with the yardstick, which tests/test_clean_cpu.py holds to the same pins.
"""

import os

import numpy as np
import pytest

from tests import _clean_cases as cc
from tests import _clean_ref as ref

pytestmark = pytest.mark.gpu

PINS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clean_pins.npz"))


def _pin(name, c, key="val"):
    return cc.dense(PINS[f"{name}_idx"], PINS[f"{name}_{key}"], c["dirty"].shape), int(PINS[f"{name}_k"]), int(PINS[f"{name}_status"])


def _device(c):
    """(model, status, residual, info) through a CleanPlan of the case's own"""
    from pfb_imaging_amd.clean import CleanPlan

    clark = c["kind"] == "clark"
    plan = CleanPlan(c["psf"], cc.psfhat(c["psf"]) if clark else None, *c["dirty"].shape[1:])
    try:
        if clark:
            model, status, resid = plan.clark(c["dirty"], c["wsums"], c["mask"], residual=True, **c["kw"])
        else:
            model, status, resid = plan.hogbom(c["dirty"], residual=True, **c["kw"])
        return model, status, resid, plan.info
    finally:
        plan.close()


def _check_against_yardstick(c, resid, info):
    """the sub-minor count and the residual, which the reference does not return"""
    if c["kind"] == "hogbom":
        _, r_ref, k_ref, _ = ref.hogbom(c["dirty"], c["psf"], **c["kw"])
        assert info["minor_iters"] == k_ref
        assert np.array_equal(resid, r_ref)
        return
    _, r_ref, _, _, n_ref = ref.clark(c["dirty"], c["psf"], cc.psfhat(c["psf"]), c["wsums"], c["mask"], **c["kw"])
    assert info["minor_iters"] == n_ref
    assert np.abs(resid - r_ref).max() <= 1e-10 * np.abs(r_ref).max()
    path = c.get("path")
    if path == "lds":
        assert info["nsub_lds"] > 0 and info["nsub_grid"] == 0
    elif path == "grid":
        assert info["nsub_grid"] > 0 and info["nsub_lds"] == 0


@pytest.mark.parametrize("name", cc.E_CASES)
def test_class_e_bit_equal_to_the_reference(name):
    c = cc.case(name)
    m_pin, k_pin, s_pin = _pin(name, c)
    model, status, resid, info = _device(c)
    assert (info["iters"], status) == (k_pin, s_pin)
    assert np.array_equal(model != 0, m_pin != 0)
    assert np.array_equal(model, m_pin)
    _check_against_yardstick(c, resid, info)


@pytest.mark.parametrize("name", cc.CLARK_T_CASES)
def test_class_t_within_the_reference_fft_disagreement(name):
    c = cc.case(name)
    m_pin, k_pin, s_pin = _pin(name, c)
    model, status, resid, info = _device(c)
    err, bound = cc.rel_max(model, m_pin), cc.t_bound(PINS[f"{name}_disagreement"])
    print(f"{name}: max|model - pin| / max|pin| = {err:.3e}, bound {bound:.3e}; nsub_lds {info['nsub_lds']} nsub_grid {info['nsub_grid']}")
    assert (info["iters"], status) == (k_pin, s_pin)
    assert np.array_equal(model != 0, m_pin != 0)
    assert err <= bound
    _check_against_yardstick(c, resid, info)
    if name == "T3":  # the run crosses from the grid sub-minor loop to the one-workgroup one
        assert info["nsub_grid"] > 0 and info["nsub_lds"] > 0


@pytest.mark.parametrize("name", ["H1", "C4_6"])
def test_reference_signature_entry_points(name):
    from pfb_imaging_amd import deconv

    c = cc.case(name)
    m_pin, _, s_pin = _pin(name, c)
    if c["kind"] == "hogbom":
        model, status = deconv.hogbom(c["dirty"], c["psf"], verbosity=0, **c["kw"])
    else:
        model, status = deconv.clark(c["dirty"], c["psf"], cc.psfhat(c["psf"]), c["wsums"], c["mask"], verbosity=0, **c["kw"])
    assert status == s_pin and model.dtype == np.float64
    assert np.array_equal(model, m_pin)


def test_float32_inputs_within_ten_times_the_float32_pin_disagreement():
    """H6: the reference computes in float32, the device widens; the pin stores the reference's own float32 / float64 difference."""
    from pfb_imaging_amd import clean, deconv

    c = cc.case("H6")
    m_pin, k_pin, s_pin = _pin("H6", c)
    model, status = deconv.hogbom(c["dirty"], c["psf"], verbosity=0, **c["kw"])
    info = clean.cached_plan(c["psf"], None, cc.NX, cc.NY).info
    err, bound = cc.rel_max(model, m_pin), cc.f_bound(PINS["H6_disagreement"])
    print(f"H6: max|model - pin| / max|pin| = {err:.3e}, bound {bound:.3e}")
    assert model.dtype == np.float32 and (info["iters"], status) == (k_pin, s_pin)
    assert np.array_equal(model != 0, m_pin != 0)
    assert err <= bound


def test_more_than_64_bands_are_refused():
    from pfb_imaging_amd.clean import CleanPlan

    with pytest.raises(ValueError, match="nband"):
        CleanPlan(np.ones((65, 8, 8)), None, 4, 4)
