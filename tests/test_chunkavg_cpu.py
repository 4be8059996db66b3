"""CPU tests of chunk averaging (``VisChunk.average``, csrc/chunkavg.hip): the library exports the entry, the numpy restatement
the GPU tests compare against (tests/_chunkavg_ref.py) reproduces examples worked by hand in exact fractions, the Python
layer refuses bad arguments before it touches the device, and the host helpers (row bins, channel bins, mean uvw,
``rows_with_data``) give hand values."""

from fractions import Fraction as F

import numpy as np
import pytest

from tests import _chunkavg_ref as ref

LD = np.longdouble


def test_library_exports_the_averaging_entry():
    from pfb_imaging_amd import _lib

    assert hasattr(_lib.lib(), "pfbhip_chunk_average_dev")
    assert "pfbhip_chunk_average_dev" in _lib.SYMBOLS


def ld(fr):
    return LD(fr.numerator) / LD(fr.denominator)


def test_restatement_reproduces_a_hand_worked_channel_example():
    """2 rows x 5 channels, ncorr = 2, chan_bin = 2: bins [0, 1], [2, 3] and the partial [4].  Row 0 has a masked sample
    (channel 1, with values that would show) inside its first bin; row 1's second bin is fully masked; correlation 1 of row
    0's second bin has dead weights.  Correlation 1 carries twice the visibilities of correlation 0.

    c = 0, row 0: {ch 0}: w = 2, v = 1 + 2i.  {2, 3}: w = 1 + 2 = 3, v = (1 * 2 + 2 * 4i) / 3 = 2/3 + 8/3 i.  {4}: w = 4, v = -1 + i.
    c = 0, row 1: {0, 1}: w = 1 + 2 = 3, v = (1 * 3 + 2 * i) / 3 = 1 + 2/3 i.  {}: zeros, masked.  {4}: w = 2, v = 2 - 2i.
    c = 1, row 0: {0}: w = 1, v = 2 + 4i.  {2, 3}: w = 0 + 0: zeros, NOT masked.  {4}: w = 2, v = -2 + 2i.
    c = 1, row 1: {0, 1}: w = 2 + 5 = 7, v = (2 * 6 + 5 * 2i) / 7 = 12/7 + 10/7 i.  {}: zeros.  {4}: w = 1, v = 4 - 4i."""
    mask = np.array([[1, 0, 1, 1, 1], [1, 1, 0, 0, 1]], dtype=np.uint8)
    v0 = np.array([[1 + 2j, 9 + 9j, 2, 4j, -1 + 1j], [3, 1j, 8, 8, 2 - 2j]])
    vis = np.stack([v0, 2 * v0])
    wgt = np.array([[[2, 9, 1, 2, 4], [1, 2, 7, 7, 2]], [[1, 1, 0, 0, 2], [2, 5, 5, 5, 1]]], dtype=np.float64)
    v, w, m, absum, count = ref.average(vis, wgt, mask, 2)
    assert v.shape == (2, 2, 3, 2) and w.shape == (2, 2, 3) and m.shape == (2, 3)
    assert np.array_equal(m, [[1, 1, 1], [1, 0, 1]])
    assert np.array_equal(count, [[1, 2, 1], [2, 0, 1]])
    want_w = [[[2, 3, 4], [3, 0, 2]], [[1, 0, 2], [7, 0, 1]]]
    assert np.array_equal(w, np.array(want_w, dtype=LD))
    want_v = [[[(F(1), F(2)), (F(2, 3), F(8, 3)), (F(-1), F(1))], [(F(1), F(2, 3)), (F(0), F(0)), (F(2), F(-2))]],
              [[(F(2), F(4)), (F(0), F(0)), (F(-2), F(2))], [(F(12, 7), F(10, 7)), (F(0), F(0)), (F(4), F(-4))]]]
    for c in range(2):
        for R in range(2):
            for q in range(3):
                for part in range(2):
                    assert v[c, R, q, part] == ld(want_v[c][R][q][part]), (c, R, q, part)
    # sum_K w |v| of c = 0, row 0, bin 1: 1 * 2 + 2 * 4 = 10; of the dead-weight bin: 0
    assert absum[0, 0, 1] == 10 and absum[1, 0, 1] == 0
    vd, wd = ref.to_double(v, w)
    assert vd.dtype == np.complex128 and vd[0, 0, 1] == complex(2 / 3, 8 / 3) and wd[1, 1, 0] == 7.0


def test_restatement_reproduces_a_hand_worked_row_example():
    """4 rows x 1 channel, chan_bin = 1, row_map = [1, -1, 1, 0]: rows 0 and 2 form output 1, row 3 is output 0, row 1 is
    dropped (its values would show).  Output 1: w = 1 + 2 = 3, v = (1 * (1 + i) + 2 * (4 - 2i)) / 3 = 3 - i.  Output 0: w = 5,
    v = 7.  With row 2 masked output 1 is row 0 alone; with nrow_out = 3 a third output has no members: masked, zero."""
    vis = np.array([[[1 + 1j], [100 + 100j], [4 - 2j], [7]]])
    wgt = np.array([[[1.0], [50.0], [2.0], [5.0]]])
    mask = np.ones((4, 1), dtype=np.uint8)
    row_map = np.array([1, -1, 1, 0])
    v, w, m, _, count = ref.average(vis, wgt, mask, 1, row_map)
    assert np.array_equal(w[0, :, 0], [5, 3]) and np.array_equal(m[:, 0], [1, 1]) and np.array_equal(count[:, 0], [1, 2])
    assert np.array_equal(v[0, :, 0], np.array([[7, 0], [3, -1]], dtype=LD))
    mask[2] = 0
    v, w, m, _, _ = ref.average(vis, wgt, mask, 1, row_map, nrow_out=3)
    assert np.array_equal(w[0, :, 0], [5, 1, 0]) and np.array_equal(m[:, 0], [1, 1, 0])
    assert np.array_equal(v[0, :, 0], np.array([[7, 0], [1, 1], [0, 0]], dtype=LD))


# ---- the Python layer ------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the refusals below must come first."""
    from pfb_imaging_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "require_gpu", touched)
    monkeypatch.setattr(_lib.DeviceArray, "__init__", touched)


def hostless_chunk(nrow=4, nchan=3, ncorr=2, mask=None):
    """A chunk that never saw a device (and counts as closed): the refusals need only its sizes and host arrays."""
    from pfb_imaging_amd.vischunk import VisChunk

    ch = VisChunk.__new__(VisChunk)
    ch.ncorr, ch.nrow, ch.nchan, ch.nvis = ncorr, nrow, nchan, nrow * nchan
    ch.uvw, ch.freq = np.arange(3.0 * nrow).reshape(nrow, 3), 1e9 + 1e6 * np.arange(nchan)
    ch.mask_host = np.ones((nrow, nchan), dtype=np.uint8) if mask is None else mask
    ch.chan_width = None
    ch.vis = ch.wgt = ch.mask = None
    return ch


def test_average_refuses_bad_arguments_before_the_device(no_device):
    ch = hostless_chunk()
    ok = np.array([0, 0, -1, 1])
    bad = [
        (ValueError, "chan_bin", dict(chan_bin=0)),
        (ValueError, "chan_bin", dict(chan_bin=-2)),
        (TypeError, "chan_bin", dict(chan_bin=2.0)),
        (TypeError, "integer", dict(row_map=ok.astype(np.float64))),
        (ValueError, "row_map shape", dict(row_map=ok[:3])),
        (ValueError, "row_map shape", dict(row_map=ok.reshape(2, 2))),
        (ValueError, "row_map entries", dict(row_map=np.array([0, -2, 0, 1]))),
        (ValueError, "row_map entries", dict(row_map=ok, nrow_out=1)),
        (ValueError, "nrow_out", dict(row_map=ok, nrow_out=-1)),
        (ValueError, "nrow_out", dict(chan_bin=2, nrow_out=3)),                      # no map: the rows stay
        (ValueError, "uvw_out shape", dict(row_map=ok, uvw_out=np.zeros((3, 3)))),
        (ValueError, "uvw_out shape", dict(chan_bin=2, uvw_out=np.zeros((4, 2)))),
        (TypeError, "uvw_out", dict(chan_bin=2, uvw_out=np.zeros((4, 3), dtype=complex))),
        (ValueError, "chan_width shape", dict(chan_bin=2, chan_width=np.ones(4))),
        (TypeError, "chan_width", dict(chan_bin=2, chan_width=np.ones(3, dtype=complex))),
        (ValueError, "no-op", dict()),
        (ValueError, "no-op", dict(chan_bin=1, row_map=np.arange(4))),
        (ValueError, "closed", dict(chan_bin=2)),
        (ValueError, "closed", dict(row_map=ok, uvw_out=np.zeros((2, 3)), chan_width=np.ones(3))),
    ]
    for exc, match, kw in bad:
        with pytest.raises(exc, match=match):
            ch.average(**kw)


def test_from_weight_data_refuses_bad_averaging_arguments_before_the_device(no_device):
    from pfb_imaging_amd.vischunk import VisChunk

    args = (np.zeros((4, 3)), np.ones(3)) + (None,) * 12
    with pytest.raises(ValueError, match="chan_average"):
        VisChunk.from_weight_data(*args, chan_average=0)
    with pytest.raises(ValueError, match="chan_width shape"):
        VisChunk.from_weight_data(*args, chan_width=np.ones(2))


def test_rows_with_data():
    mask = np.array([[0, 0, 0], [0, 2, 0], [0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 1]], dtype=np.uint8)
    ch = hostless_chunk(nrow=6, mask=mask)
    got = ch.rows_with_data()
    assert got.dtype == np.int64 and np.array_equal(got, [-1, 0, -1, 1, -1, 2])
    assert np.array_equal(hostless_chunk().rows_with_data(), np.arange(4))
    assert np.array_equal(hostless_chunk(mask=np.zeros((4, 3), dtype=np.uint8)).rows_with_data(), [-1] * 4)


def test_row_bins_are_a_stable_csr():
    from pfb_imaging_amd.vischunk import row_bins

    row_start, members, nrow_out = row_bins(np.array([2, 0, -1, 2, 0, 2]), 6)
    assert nrow_out == 3 and row_start.dtype == np.int64 and members.dtype == np.int64
    assert np.array_equal(row_start, [0, 2, 2, 5])        # output 1 has no members
    assert np.array_equal(members, [1, 4, 0, 3, 5])       # ascending inside each bin
    row_start, members, nrow_out = row_bins(np.array([-1, -1]), 2)
    assert nrow_out == 0 and np.array_equal(row_start, [0]) and members.size == 0
    row_start, members, nrow_out = row_bins(np.array([0, 0], dtype=np.uint8), 2, nrow_out=2)
    assert np.array_equal(row_start, [0, 2, 2]) and np.array_equal(members, [0, 1])


def test_channel_bins_and_mean_uvw_against_hand_values():
    from pfb_imaging_amd.vischunk import channel_bins, mean_uvw, row_bins

    freq = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    width = np.array([1.0, 1.0, 2.0, 4.0, 8.0])
    f, w = channel_bins(freq, 2, width)
    assert np.array_equal(f, [1.5, 6.0, 16.0]) and np.array_equal(w, [2.0, 6.0, 8.0])
    f, w = channel_bins(freq, 7, None)
    assert np.array_equal(f, [6.2]) and w is None
    f, w = channel_bins(freq, 1, width)
    assert np.array_equal(f, freq) and np.array_equal(w, width)
    for chan_bin in (1, 2, 3, 5, 7):
        rf, rw = ref.channel_bins(freq, chan_bin, width)
        f, w = channel_bins(freq, chan_bin, width)
        np.testing.assert_allclose(f, rf, rtol=1e-15)
        np.testing.assert_allclose(w, rw, rtol=1e-15)
    uvw = np.array([[1.0, 2.0, 3.0], [10.0, 20.0, 30.0], [3.0, 6.0, 9.0], [0.0, 0.0, 7.0]])
    row_map = np.array([1, -1, 1, 0])
    got = mean_uvw(uvw, *row_bins(row_map, 4, 3)[:2])
    assert np.array_equal(got, [[0.0, 0.0, 7.0], [2.0, 4.0, 6.0], [0.0, 0.0, 0.0]])   # masked or not; no members: zero
    assert np.array_equal(got, ref.mean_uvw(uvw, row_map, 3))
