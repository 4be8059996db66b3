"""CPU tests of the device-resident visibility chunk: the library exports its entries, the Python layer refuses bad arguments
before it touches the device, and the numpy restatement of the reference's l2 reweighting (tests/_vischunk_ref.py), which
the GPU tests compare against, reproduces an example worked by hand."""

import ctypes as ct
from fractions import Fraction

import numpy as np
import pytest

from tests import _vischunk_ref as ref

NEW_SYMBOLS = ("pfbhip_gridder_vis2dirty_rows_dev", "pfbhip_gridder_psf_rows_dev", "pfbhip_gridder_set_weights_dev",
               "pfbhip_gridder_dirty2vis_rows_dev", "pfbhip_chunk_wsum_dev", "pfbhip_chunk_l2_reweight_dev",
               "pfbhip_imaging_weights_dev")


def test_library_exports_the_seven_new_symbols():
    from pfb_imaging_amd import _lib

    L = _lib.lib()
    assert [s for s in NEW_SYMBOLS if not hasattr(L, s)] == []
    assert set(NEW_SYMBOLS) <= set(_lib.SYMBOLS)


@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the refusals below must come first."""
    from pfb_imaging_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    # (every path to the device starts with one of these two; `lib` itself is bound by name in modules that import it)
    monkeypatch.setattr(_lib, "require_gpu", touched)
    monkeypatch.setattr(_lib.DeviceArray, "__init__", touched)


def fake_device_array(shape, dtype):
    from pfb_imaging_amd._lib import DeviceArray

    d = DeviceArray.__new__(DeviceArray)
    d.shape, d.dtype = tuple(shape), np.dtype(dtype)
    d.nbytes = int(np.prod(shape)) * d.dtype.itemsize
    d.ptr = ct.c_void_p(0)  # (free() and __del__ leave a NULL pointer alone)
    return d


def test_vischunk_refuses_wrong_shapes_and_dtypes_before_the_device(no_device):
    from pfb_imaging_amd.vischunk import VisChunk

    nrow, nchan = 4, 3
    uvw, freq = np.zeros((nrow, 3)), np.ones(nchan)
    vis, wgt = np.zeros((2, nrow, nchan), dtype=np.complex128), np.ones((2, nrow, nchan))
    mask = np.ones((nrow, nchan), dtype=np.uint8)
    bad = [
        (ValueError, dict(uvw=np.zeros((nrow, 2)))),
        (ValueError, dict(freq=np.ones((nchan, 1)))),
        (TypeError, dict(freq=np.ones(nchan, dtype=complex))),
        (ValueError, dict(vis=vis[0])),                                  # no correlation axis
        (ValueError, dict(vis=vis[:, :3])),
        (ValueError, dict(wgt=wgt[:1])),
        (ValueError, dict(mask=mask[:, :2])),
        (ValueError, dict(mask=np.ones((2, nrow, nchan), dtype=np.uint8))),
        (TypeError, dict(wgt=wgt.astype(complex))),
        (TypeError, dict(mask=mask.astype(float))),
        (TypeError, dict(vis=fake_device_array(vis.shape, np.complex64))),  # resident arrays are adopted, never converted
        (TypeError, dict(wgt=fake_device_array(wgt.shape, np.float32))),
        (ValueError, dict(mask=fake_device_array((nchan, nrow), np.uint8))),
    ]
    for exc, change in bad:
        kw = dict(uvw=uvw, freq=freq, vis=vis, wgt=wgt, mask=mask)
        kw.update(change)
        with pytest.raises(exc):
            VisChunk(**kw)


def test_chain_refuses_bad_arguments_before_the_device(no_device):
    from pfb_imaging_amd.operators.gridder import image_data_products_chunk
    from pfb_imaging_amd.vischunk import VisChunk

    ch = VisChunk.__new__(VisChunk)  # (a chunk that never saw a device: the refusals need only its sizes)
    ch.ncorr, ch.nrow, ch.nchan, ch.nvis = 2, 4, 3, 12
    ch.vis = ch.wgt = ch.mask = None
    args = (8, 8, 16, 16, 1e-5, 1e-5)
    with pytest.raises(TypeError, match="VisChunk"):
        image_data_products_chunk(dict(vis=None), *args)
    with pytest.raises(ValueError, match="do_psf"):
        image_data_products_chunk(ch, *args, do_psf=False, do_psfpars=True)
    with pytest.raises(ValueError, match="no model"):
        image_data_products_chunk(ch, *args, l2_reweight_dof=5)
    with pytest.raises(ValueError, match="model shape"):
        image_data_products_chunk(ch, *args, model=np.zeros((2, 8, 9)))
    with pytest.raises(TypeError, match="real"):
        image_data_products_chunk(ch, *args, model=np.zeros((2, 8, 8), dtype=complex))
    with pytest.raises(ValueError, match="beam shape"):
        image_data_products_chunk(ch, *args, beam=np.ones((1, 8, 8)))
    with pytest.raises(ValueError, match="closed"):
        image_data_products_chunk(ch, *args)


def test_dev_ptr_bounds():
    from pfb_imaging_amd import _lib

    d = fake_device_array((2, 6), np.complex128)
    d.ptr = ct.c_void_p(4096)
    assert _lib.dev_ptr(None) is None
    assert _lib.dev_ptr(d, 6, 6).value == 4096 + 6 * 16
    for off, count in ((7, 6), (-1, 1), (12, 1)):
        with pytest.raises(ValueError):
            _lib.dev_ptr(d, off, count)
    d.ptr = ct.c_void_p(0)


def test_restated_l2_reweighting_reproduces_a_hand_computed_example():
    """nrow = 2, nchan = 3, dof = 2, wgtp = 1.  Correlation 0: |r|^2 = [[1, 1, 4], [0, 2, 9]], mask = [[1, 1, 0], [1, 0, 1]]:
    ssq = 1 + 1 + 0 + 9 = 11, mask.sum() = 4, ovar = 11 / 4, factor = 4 / (2 + 4 |r|^2 / 11) = 44 / (22 + 4 |r|^2):
    22/13, 22/13, 22/19, 2, 22/15, 22/29 -- also on the two masked samples.  Correlation 1 has twice the residual: |r|^2 and
    ovar (= 11) are four times as large, the factors the same; a variance taken jointly over both would not give them."""
    r0 = np.array([[1.0, 1.0j, 2.0], [0.0, 1.0 + 1.0j, 3.0]])
    res = np.stack([r0, 2.0 * r0])
    mask = np.array([[1, 1, 0], [1, 0, 1]], dtype=np.uint8)
    wgt = np.stack([np.ones((2, 3)), np.full((2, 3), 3.0)])
    before = wgt.copy()
    got, ovar = ref.l2_reweight(res, wgt, mask, 2)
    factor = np.array([[Fraction(22, 13), Fraction(22, 13), Fraction(22, 19)], [Fraction(2), Fraction(22, 15), Fraction(22, 29)]],
                      dtype=object).astype(np.float64)
    np.testing.assert_allclose(ovar, [2.75, 11.0], rtol=1e-15)
    np.testing.assert_allclose(got, np.stack([factor, 3.0 * factor]), rtol=1e-15)
    assert np.array_equal(wgt, before)
    # wgtp as an array scales |r|^2 sample by sample: doubling it everywhere doubles ovar and changes no weight
    got2, ovar2 = ref.l2_reweight(res, wgt, mask, 2, np.full(res.shape, 2.0))
    np.testing.assert_allclose(ovar2, 2.0 * ovar, rtol=1e-15)
    np.testing.assert_allclose(got2, got, rtol=1e-15)
    with pytest.raises(ValueError, match="zero residual variance"):
        ref.l2_reweight(np.zeros_like(res), wgt, mask, 2)
