"""CPU tests of the snapshot imager (pfb_imaging_amd/utils/stokes2im.py, csrc/snapshot.hip): the numpy restatement the GPU
tests compare against (tests/_snapshot_ref.py) reproduces values worked by hand, both public functions refuse bad
arguments before they touch the device, and the library exports the four new entries the header declares."""

import ctypes as ct
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import _snapshot_ref as ref

NEW_SYMBOLS = ("pfbhip_chunk_rephase_residual_dev", "pfbhip_chunk_l2_reweight_joint_dev", "pfbhip_gridder_psf_rows_signed_dev",
               "pfbhip_snapshot_finish_dev")


def test_library_exports_and_header_declares_the_four_new_symbols():
    from pfb_imaging_amd import _lib

    L = _lib.lib()
    assert [s for s in NEW_SYMBOLS if not hasattr(L, s)] == []
    assert set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfbhip.h")).read()
    assert [s for s in NEW_SYMBOLS if f"int {s}(" not in header] == []


# ---- the restatement against hand-worked values ------------------------------------------------------------------------------

def test_joint_reweighting_on_a_2_by_3_example_in_exact_fractions():
    """nrow = 2, nchan = 3, two correlations, dof = 2.  |r0|^2 = [[1, 1, 4], [0, 2, 9]], r1 = 2 r0, mask = [[1, 1, 0], [1, 0, 1]]:
    sum ressq = (1 + 1 + 0 + 9) (1 + 4) = 55, mask.sum() = 4, ovar = 55 / 4 -- ONE variance; per correlation they would be 11 / 4
    and 11.  wgt = 3 / (2 + 4 ressq / 55) * 4 / 55 = 6 / (55 + 2 ressq) with ressq zero on the masked samples: 6 / 55 there."""
    r0 = np.array([[1.0, 1.0j, 2.0], [0.0, 1.0 + 1.0j, 3.0]])
    data = np.stack([r0, 2.0 * r0])
    mask = np.array([[1, 1, 0], [1, 0, 1]], dtype=np.uint8)
    wgt, ovar = ref.l2_reweight_joint(data, mask, 2)
    want = np.array([[[Fraction(6, 57), Fraction(6, 57), Fraction(6, 55)], [Fraction(6, 55), Fraction(6, 55), Fraction(6, 73)]],
                     [[Fraction(6, 63), Fraction(6, 63), Fraction(6, 55)], [Fraction(6, 55), Fraction(6, 55), Fraction(6, 127)]]],
                    dtype=object).astype(np.float64)
    assert ovar == 13.75
    np.testing.assert_allclose(wgt, want, rtol=4e-16)
    with pytest.raises(ValueError, match="exactly zero"):
        ref.l2_reweight_joint(np.zeros_like(data), mask, 2)
    with pytest.raises(ValueError, match="empty mask"):
        ref.l2_reweight_joint(data, np.zeros_like(mask), 2)


def test_one_rephased_sample():
    """f = c and 2 c, so f / c = 1 and 2 cycles per metre; w_diff = 1 / 4 m: p = exp(-2 pi i / 4) = -i and exp(-2 pi i / 2) = -1.
    (1 + 2i)(-i) = 2 - i; minus the model 1 * (-i): 2.  Second channel: -(1 + 2i) + 1 = -2i.  The masked row is zero only
    with a model."""
    freq = np.array([ref.C0, 2 * ref.C0])
    data = np.full((1, 2, 2), 1.0 + 2.0j)
    model = np.ones((1, 2, 2), dtype=complex)
    mask = np.array([[1, 1], [0, 0]], dtype=np.uint8)
    w_diff = np.array([0.25, 0.25])
    got = ref.rephase_residual(data, mask, freq, w_diff, model)
    np.testing.assert_allclose(got[0], [[2.0, -2.0j], [0.0, 0.0]], atol=1e-15)
    got = ref.rephase_residual(data, mask, freq, w_diff, None)
    np.testing.assert_allclose(got[0], [[2.0 - 1.0j, -1.0 - 2.0j]] * 2, atol=1e-15)
    assert np.array_equal(ref.rephase_residual(data, mask, freq), data)
    # the PSF ramp of :483-486 at (x0, y0) = (0.6, 0), n - 1 = -0.2: u = 1 m gives 0.6 cycles, w = 1 m gives +0.2 cycles
    pv = ref.psf_vis(np.array([[1.0, 5.0, 0.0], [0.0, 0.0, 1.0]]), freq[:1], 0.6, 0.0)
    np.testing.assert_allclose(pv[:, 0], np.exp(-2j * np.pi * np.array([0.6, 0.2])), atol=1e-15)


@pytest.mark.parametrize("n,min_padding,want", [(64, 1.7, 108), (100, 1.7, 176), (2048, 1.7, 3500), (10, 1.0, 10), (13, 1.0, 14)])
def test_pad_size_rule(n, min_padding, want):
    """int(1.7 * 100) = 170 = 2 * 5 * 17 is not smooth; 175 = 5^2 * 7 is, but odd; 176 = 2^4 * 11.  3481 = 59^2 -> 3500 = 2^2 5^3 7."""
    from pfb_imaging_amd.utils import stokes2im

    assert ref.pad_size(n, min_padding) == want
    assert stokes2im.pad_size(n, min_padding) == want


@pytest.mark.parametrize("nx,ny,rel_size,want", [(64, 64, None, (128, 128)), (64, 64, 1.5, (128, 128)), (200, 100, 1.0, (128, 128)),
                                                 (200, 150, 1.0, (200, 150)), (129, 173, 1.0, (132, 176)), (2048, 2048, 0.25, (512, 512))])
def test_psf_size_rule(nx, ny, rel_size, want):
    """Either side below 128 sets both to 128 (:617-619); 129 -> 132 = 2^2 * 3 * 11, 173 -> 175 is odd -> 176."""
    from pfb_imaging_amd.utils import stokes2im

    assert ref.psf_size(nx, ny, rel_size) == want
    assert stokes2im.psf_size(nx, ny, rel_size) == want


def test_std_is_two_pass():
    """[1, 2, 3, 4]: mean 5 / 2, squared deviations 9/4, 1/4, 1/4, 9/4, variance 5 / 4 -- also on top of 10^6, where the one-pass
    E[x^2] - mean^2 loses it: x^2 ~ 10^12 carries 53 - 40 = 13 bits of the variance."""
    x = np.array([[1.0, 2.0], [3.0, 4.0]])
    assert abs(ref.std(x) - np.sqrt(1.25)) < 1e-15
    assert abs(ref.std(x + 1.0e6) - np.sqrt(1.25)) < 1e-15


# ---- refusals before the device ----------------------------------------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the refusals below must come first."""
    from pfb_imaging_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "require_gpu", touched)
    monkeypatch.setattr(_lib.DeviceArray, "__init__", touched)


def fake_device_array(shape, dtype):
    from pfb_imaging_amd._lib import DeviceArray

    d = DeviceArray.__new__(DeviceArray)
    d.shape, d.dtype = tuple(shape), np.dtype(dtype)
    d.nbytes = int(np.prod(shape)) * d.dtype.itemsize
    d.ptr = ct.c_void_p(0)
    return d


def test_snapshot_image_chunk_refuses_bad_arguments_before_the_device(no_device):
    from pfb_imaging_amd.utils.stokes2im import snapshot_image_chunk
    from pfb_imaging_amd.vischunk import VisChunk

    ch = VisChunk.__new__(VisChunk)  # (a chunk that never saw a device: the refusals need only its sizes)
    ch.ncorr, ch.nrow, ch.nchan, ch.nvis = 2, 4, 3, 12
    ch.vis = ch.wgt = ch.mask = None
    args = (8, 8, 1e-5)
    with pytest.raises(TypeError, match="VisChunk"):
        snapshot_image_chunk(dict(vis=None), *args)
    bad = [
        (ValueError, "positive integers", dict(), (0, 8, 1e-5)),
        (ValueError, "positive integers", dict(), (8.5, 8, 1e-5)),
        (ValueError, "cell_rad", dict(), (8, 8, 0.0)),
        (ValueError, "sphere", dict(x0=0.8, y0=0.7), args),
        (ValueError, "min_padding", dict(min_padding=0.5), args),
        (ValueError, "psf_relative_size", dict(psf_relative_size=0.0), args),
        (TypeError, "out_dtype", dict(out_dtype=np.float16), args),
        (ValueError, "model_vis shape", dict(model_vis=np.zeros((2, 4, 2), dtype=complex)), args),
        (TypeError, "complex128", dict(model_vis=fake_device_array((2, 4, 3), np.complex64)), args),
        (ValueError, "w_diff shape", dict(w_diff=np.zeros(5)), args),
        (ValueError, "l2_reweight_dof", dict(l2_reweight_dof=-1), args),
        (ValueError, "transients lacks", dict(transients=dict(uvw=np.zeros((4, 3)))), args),
        (ValueError, "weight_grid_out", dict(weight_grid_out=True), args),
        (ValueError, "pbeam shape", dict(pbeam=np.ones((1, 8, 8))), args),
        (TypeError, "pbeam must be real", dict(pbeam=np.ones((2, 8, 8), dtype=complex)), args),
        (ValueError, "eta", dict(pbeam=np.ones((2, 8, 8)), eta=-1.0), args),
        (TypeError, "w_diff must be real", dict(w_diff=np.zeros(4, dtype=complex)), args),
        (TypeError, "model_vis must be complex", dict(model_vis=np.zeros((2, 4, 3))), args),
        (ValueError, "l2_reweight_dof", dict(l2_reweight_dof=float("nan")), args),
        (ValueError, "epsilon", dict(epsilon=0.0), args),
        (ValueError, "npix_super", dict(robustness=0.0, npix_super=-1), args),
        (ValueError, "npix_super", dict(robustness=0.0, npix_super=1.5), args),
        (ValueError, "filter_counts_level", dict(robustness=0.0, filter_counts_level=-1.0), args),
        (ValueError, "robustness", dict(robustness=float("nan")), args),
        (ValueError, "closed", dict(), args),
    ]
    for exc, match, kw, a in bad:
        with pytest.raises(exc, match=match):
            snapshot_image_chunk(ch, *a, **kw)
    for dof in (0, -1.0, float("nan"), float("inf")):  # (a masked sample gets (dof + 1) / dof / ovar)
        with pytest.raises(ValueError, match="dof"):
            ch.l2_reweight_joint(dof)


def test_stokes_image_arrays_refuses_bad_arguments_before_the_device(no_device):
    from pfb_imaging_amd.utils.stokes2im import stokes_image_arrays

    nrow, nchan, nant = 6, 3, 4
    good = dict(data=np.zeros((nrow, nchan, 4), dtype=complex), weight=np.ones((nrow, nchan, 4)), flag=np.zeros((nrow, nchan, 4), dtype=bool),
                jones=np.ones((1, nant, nchan, 1, 2), dtype=complex), tbin_idx=np.array([0]), tbin_counts=np.array([nrow]),
                ant1=np.array([0, 0, 0, 1, 1, 2]), ant2=np.array([1, 2, 3, 2, 3, 3]), uvw=np.zeros((nrow, 3)), freq=np.ones(nchan),
                pol="linear", product="IQ", nc="4", wgt_mode="l2", nx=8, ny=8, cell_rad=1e-5)
    bad = [
        (ValueError, dict(uvw=np.zeros((nrow, 2)))),
        (ValueError, dict(freq=np.ones(nchan + 1))),
        (TypeError, dict(freq=np.ones(nchan, dtype=complex))),
        (ValueError, dict(data=np.zeros((nrow, nchan), dtype=complex))),
        (ValueError, dict(weight=np.ones((nrow, nchan, 2)))),
        (ValueError, dict(nc="3")),
        (ValueError, dict(pol="elliptical")),
        (ValueError, dict(ant1=np.array([0, 0, 0, 1, 1, 9]))),
        (ValueError, dict(nx=0)),
        (ValueError, dict(pbeam=np.ones((4, 8, 8)))),            # two products, not four
        (ValueError, dict(model_vis=np.zeros((4, nrow, nchan), dtype=complex))),
        (ValueError, dict(weight_grid_out=True)),
        (TypeError, dict(w_diff=np.zeros(nrow, dtype=complex))),
        (TypeError, dict(model_vis=np.zeros((2, nrow, nchan)))),
        (ValueError, dict(epsilon=2.0)),
        (ValueError, dict(robustness=0.0, npix_super=-2)),
        (TypeError, dict(no_such_keyword=1)),
    ]
    for exc, change in bad:
        kw = dict(good)
        kw.update(change)
        with pytest.raises(exc):
            stokes_image_arrays(**kw)


def test_psf_rows_dev_refuses_a_ramp_sign_that_is_no_sign():
    from pfb_imaging_amd.wgridder import Gridder

    g = Gridder.__new__(Gridder)
    g._h = None
    with pytest.raises(ValueError, match="ramp_sign"):
        g.psf_rows_dev(None, None, ramp_sign=0.5)
