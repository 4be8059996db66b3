"""A visibility chunk that lives in HBM: the Stokes visibilities, weights and mask of one (time, band) chunk, uploaded (or
adopted from :func:`~pfb_imaging_amd.utils.weighting.weight_data_dev`) once and consumed on the device by every product of
:func:`~pfb_imaging_amd.operators.gridder.image_data_products_chunk`.

The array path (``image_data_products_arrays``) crosses PCIe once per correlation and per product; here the weights are
reduced (``WSUM``, gridder.py:584 of the reference), reweighted (:509-532) and turned into imaging weights (:534-576) where
they lie (csrc/vischunk.hip, csrc/weighting.hip), and the gridder reads its rows straight from the chunk
(``Gridder.vis2dirty_rows_dev`` and friends).

Memory held: ``ncorr * 24 + 1`` bytes per sample (complex128 visibilities, float64 weights, the uint8 mask);
``image_data_products_chunk`` holds ``ncorr * 16`` more per sample while a model is given (the residual visibilities).
"""

import ctypes as ct

import numpy as np

from . import _lib
from ._lib import DeviceArray, as_c, check, f64, lib, ptr


def _adopt(a, shape, dtype, name):
    """``a`` after its shape and dtype have been checked: a DeviceArray must have ``dtype`` exactly (resident arrays are adopted,
    never converted), a host array a dtype that converts to it without loss.  No device call: VisChunk.__init__ uploads only
    after every argument has passed."""
    dtype = np.dtype(dtype)
    if isinstance(a, DeviceArray):
        if a.dtype != dtype:
            raise TypeError(f"{name} on the device must be {dtype}, not {a.dtype}")
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name} shape {tuple(a.shape)} != {tuple(shape)}")
        return a
    a = np.asarray(a)
    kinds = {"c": "c", "f": "fiu", "u": "biu"}[dtype.kind]
    if a.dtype.kind not in kinds:
        raise TypeError(f"{name} must be convertible to {dtype} without loss, not {a.dtype}")
    if a.shape != tuple(shape):
        raise ValueError(f"{name} shape {a.shape} != {tuple(shape)}")
    return a


def _check_chan_bin(chan_bin, name="chan_bin"):
    if isinstance(chan_bin, bool) or not isinstance(chan_bin, (int, np.integer)):
        raise TypeError(f"{name} must be an integer, not {type(chan_bin).__name__}")
    if chan_bin < 1:
        raise ValueError(f"{name} = {chan_bin} must be at least 1")
    return int(chan_bin)


def _check_chan_width(chan_width, nchan):
    if chan_width is None:
        return None
    chan_width = np.asarray(chan_width)
    if chan_width.dtype.kind not in "fiu":
        raise TypeError(f"chan_width must be real, not {chan_width.dtype}")
    if chan_width.shape != (nchan,):
        raise ValueError(f"chan_width shape {chan_width.shape} != {(nchan,)}")
    return as_c(chan_width, np.float64)


def row_bins(row_map, nrow, nrow_out=None):
    """``(row_start (nrow_out + 1), members (nkept), nrow_out)`` int64: the CSR of ``row_map (nrow)``, whose entry ``r`` is the
    output row of input row ``r`` in ``[0, nrow_out)`` or ``-1`` to drop it.  A stable sort keeps the members of a bin in
    ascending input-row order.  ``nrow_out`` defaults to ``row_map.max() + 1``.  Host work only."""
    row_map = np.asarray(row_map)
    if row_map.dtype.kind not in "iu":
        raise TypeError(f"row_map must be of an integer type, not {row_map.dtype}")
    if row_map.shape != (nrow,):
        raise ValueError(f"row_map shape {row_map.shape} != {(nrow,)}")
    row_map = row_map.astype(np.int64, copy=False)
    if nrow_out is None:
        nrow_out = int(row_map.max()) + 1 if nrow else 0
    elif isinstance(nrow_out, bool) or not isinstance(nrow_out, (int, np.integer)) or nrow_out < 0:
        raise ValueError(f"nrow_out = {nrow_out!r} must be a non-negative integer")
    nrow_out = max(int(nrow_out), 0)
    if nrow and (row_map.min() < -1 or row_map.max() >= nrow_out):
        raise ValueError(f"row_map entries must lie in [-1, {nrow_out}), got [{row_map.min()}, {row_map.max()}]")
    kept = np.flatnonzero(row_map >= 0)
    members = kept[np.argsort(row_map[kept], kind="stable")].astype(np.int64)
    row_start = np.zeros(nrow_out + 1, dtype=np.int64)
    np.cumsum(np.bincount(row_map[kept], minlength=nrow_out), out=row_start[1:])
    return row_start, members, nrow_out


def channel_bins(freq, chan_bin, chan_width=None):
    """``(freq_out, chan_width_out)`` of channel bins ``[q chan_bin, min((q + 1) chan_bin, nchan))``: the mean of a bin's
    frequencies and the sum of its widths (``None`` without ``chan_width``)."""
    starts = np.arange(0, freq.size, chan_bin)
    counts = np.minimum(starts + chan_bin, freq.size) - starts
    freq_out = np.add.reduceat(freq, starts) / counts
    return freq_out, None if chan_width is None else np.add.reduceat(chan_width, starts)


def mean_uvw(uvw, row_start, members):
    """``(nrow_out, 3)``: the plain mean of every bin's member rows, masked or not, in float64; zeros for a bin without members"""
    counts = np.diff(row_start)
    out = np.zeros((counts.size, 3))
    rows = np.repeat(np.arange(counts.size), counts)
    for j in range(3):
        out[:, j] = np.bincount(rows, weights=uvw[members, j], minlength=counts.size)
    out[counts > 0] /= counts[counts > 0, None]
    return out


class VisChunk:
    """``uvw (nrow, 3)``, ``freq (nchan)`` (host), ``vis, wgt (ncorr, nrow, nchan)`` and ``mask (nrow, nchan)``: each of the
    last three a host array, uploaded once (``vis`` as complex128, ``wgt`` as float64, ``mask`` as uint8, non-zero = keep), or
    a :class:`~pfb_imaging_amd._lib.DeviceArray` of that dtype and shape, which the chunk adopts: :meth:`close` frees it.

    The chunk keeps a host copy of the mask, because a gridder plan is built from a host mask (``pfbhip_gridder_create``); a
    mask that starts on the device is downloaded once, one byte per sample.  The weights are updated in place by
    :meth:`l2_reweight` and :meth:`imaging_weights`."""

    def __init__(self, uvw, freq, vis, wgt, mask):
        uvw, freq = np.asarray(uvw), np.asarray(freq)
        if uvw.ndim != 2 or uvw.shape[1] != 3:
            raise ValueError(f"uvw must have shape (nrow, 3), got {uvw.shape}")
        if freq.ndim != 1 or freq.size < 1:
            raise ValueError(f"freq must be one-dimensional and not empty, got {freq.shape}")
        if uvw.dtype.kind not in "fiu" or freq.dtype.kind not in "fiu":
            raise TypeError("uvw and freq must be real")
        nrow, nchan = uvw.shape[0], freq.size
        vshape = tuple(vis.shape) if isinstance(vis, DeviceArray) else np.shape(vis)
        if len(vshape) != 3 or vshape[1:] != (nrow, nchan) or vshape[0] < 1:
            raise ValueError(f"vis must have shape (ncorr, {nrow}, {nchan}), got {vshape}")
        ncorr = vshape[0]
        vis = _adopt(vis, (ncorr, nrow, nchan), np.complex128, "vis")
        wgt = _adopt(wgt, (ncorr, nrow, nchan), np.float64, "wgt")
        mask = _adopt(mask, (nrow, nchan), np.uint8, "mask")
        # -- every argument has passed: the device from here on
        _lib.require_gpu()
        self.uvw, self.freq = as_c(uvw, np.float64), as_c(freq, np.float64)
        self.ncorr, self.nrow, self.nchan = ncorr, nrow, nchan
        self.nvis = nrow * nchan
        self.chan_width = None
        self.vis = self.wgt = self.mask = None
        try:
            self.vis = vis if isinstance(vis, DeviceArray) else DeviceArray.from_host(as_c(vis, np.complex128))
            self.wgt = wgt if isinstance(wgt, DeviceArray) else DeviceArray.from_host(as_c(wgt, np.float64))
            if isinstance(mask, DeviceArray):
                self.mask, self.mask_host = mask, mask.download(np.empty((nrow, nchan), dtype=np.uint8))
            else:
                self.mask_host = as_c(mask != 0 if mask.dtype == np.bool_ else mask, np.uint8)
                self.mask = DeviceArray.from_host(self.mask_host)
        except Exception:
            self.close()
            raise

    @classmethod
    def from_weight_data(cls, uvw, freq, data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, nc, wgt_mode,
                         chan_average=1, drop_flagged_rows=False, chan_width=None):
        """The chunk of raw correlations: ``weight_data_dev(corr_first=True, with_mask=True)`` (weighting.py:274-468 of the
        reference) leaves Stokes visibilities, weights and the mask ``~flag.any(-1)`` in HBM, and the chunk adopts them.

        ``chan_average > 1`` and ``drop_flagged_rows`` are steps 2 and 3 of ``pfb init`` (utils/stokes2vis.py:215-260): the
        chunk is averaged over ``chan_average`` channels and loses the rows without an unmasked sample
        (:meth:`average` with :meth:`rows_with_data`), and the chunk that comes back is the averaged one; the first is closed.
        ``chan_width (nchan)`` is kept as ``.chan_width`` and summed over the bins."""
        from .utils.weighting import weight_data_dev

        chan_average = _check_chan_bin(chan_average, "chan_average")
        chan_width = _check_chan_width(chan_width, np.size(freq))
        vis, wgt, mask = weight_data_dev(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, nc, wgt_mode,
                                         corr_first=True, with_mask=True)
        try:
            first = cls(uvw, freq, vis, wgt, mask)
        except Exception:
            for d in (vis, wgt, mask):
                d.free()
            raise
        first.chan_width = chan_width
        row_map = first.rows_with_data() if drop_flagged_rows else None
        if row_map is not None and (row_map >= 0).all():
            row_map = None
        if chan_average == 1 and row_map is None:
            return first
        try:
            return first.average(chan_average, row_map, chan_width=chan_width)
        finally:
            first.close()

    # -- lifetime ---------------------------------------------------------
    def close(self):
        for name in ("vis", "wgt", "mask"):
            d = getattr(self, name, None)
            if d is not None:
                d.free()
            setattr(self, name, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _open(self):
        if self.wgt is None:
            raise ValueError("the chunk is closed")

    def corr_offset(self, c):
        """Element offset of correlation ``c`` inside ``vis`` / ``wgt``."""
        if not 0 <= c < self.ncorr:
            raise ValueError(f"correlation {c} of {self.ncorr}")
        return c * self.nvis

    # -- averaging (utils/stokes2vis.py:215-286; csrc/chunkavg.hip) -------------------------------------------------------
    def rows_with_data(self):
        """The ``row_map`` that keeps, in order, the rows with at least one unmasked sample and drops the others: the
        reference's ``mrow`` (stokes2vis.py:217) for :meth:`average`.  From the host copy of the mask; no device call."""
        keep = self.mask_host.any(axis=1)
        return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)

    def average(self, chan_bin=1, row_map=None, nrow_out=None, uvw_out=None, chan_width=None):
        """A NEW chunk: this one averaged over channel bins of ``chan_bin`` channels (the last may be partial) and over the row
        bins of ``row_map (nrow)``, whose entry ``r`` is the output row of input row ``r`` or ``-1`` to drop it (``None``: every
        row stays where it is); ``nrow_out`` defaults to ``row_map.max() + 1``.  With ``K`` the unmasked samples of an output
        sample: ``wgt = sum_K wgt``, ``vis = sum_K wgt vis / wgt``, ``mask = K not empty``; an empty ``K`` or a zero weight sum
        gives exact zeros.  ``freq`` becomes the mean of each bin's frequencies, ``chan_width`` (``.chan_width`` of the new
        chunk, ``None`` if not given) the sum of its widths, ``uvw`` the plain mean of a bin's member rows unless ``uvw_out
        (nrow_out, 3)`` is given.  This chunk is untouched and stays the caller's to close."""
        chan_bin = _check_chan_bin(chan_bin)
        chan_width = _check_chan_width(chan_width, self.nchan)
        ident = row_map is None
        if ident:
            if nrow_out is not None and nrow_out != self.nrow:
                raise ValueError(f"nrow_out = {nrow_out} without a row_map must be nrow = {self.nrow}")
            nrow_out = self.nrow
        else:
            row_start, members, nrow_out = row_bins(row_map, self.nrow, nrow_out)
            ident = nrow_out == self.nrow and np.array_equal(members, np.arange(self.nrow)) and (np.diff(row_start) == 1).all()
        if ident and chan_bin == 1:
            raise ValueError("average(chan_bin=1) with the identity row map is a no-op: it would only copy the chunk")
        if uvw_out is not None:
            uvw_out = np.asarray(uvw_out)
            if uvw_out.dtype.kind not in "fiu":
                raise TypeError(f"uvw_out must be real, not {uvw_out.dtype}")
            if uvw_out.shape != (nrow_out, 3):
                raise ValueError(f"uvw_out shape {uvw_out.shape} != {(nrow_out, 3)}")
        elif ident:
            uvw_out = self.uvw
        else:
            uvw_out = mean_uvw(self.uvw, row_start, members)
        freq_out, width_out = channel_bins(self.freq, chan_bin, chan_width)
        self._open()
        # -- every argument has passed: the device from here on
        shape = (self.ncorr, nrow_out, freq_out.size)
        made = []
        try:
            for shp, dtype in ((shape, np.complex128), (shape, np.float64), (shape[1:], np.uint8)):
                made.append(DeviceArray(shp, dtype))
            vis, wgt, mask = made
            check(lib().pfbhip_chunk_average_dev(self.vis.ptr, self.wgt.ptr, self.mask.ptr, self.ncorr, self.nrow, self.nchan,
                                                 chan_bin, None if ident else ptr(row_start), None if ident else ptr(members),
                                                 self.nrow if ident else members.size, nrow_out, vis.ptr, wgt.ptr, mask.ptr))
            out = VisChunk(uvw_out, freq_out, vis, wgt, mask)
        except Exception:
            for d in made:
                d.free()
            raise
        out.chan_width = width_out
        return out

    # -- the weights, where they lie ----------------------------------------
    def wsum(self):
        """``wgt[:, mask != 0].sum(-1)`` (gridder.py:584); bit-identical from call to call."""
        self._open()
        out = np.empty(self.ncorr, dtype=np.float64)
        check(lib().pfbhip_chunk_wsum_dev(self.wgt.ptr, self.mask.ptr, self.ncorr, self.nvis, ptr(out)))
        return out

    def l2_reweight(self, resvis_dev, dof, wgtp=1.0):
        """The l2 reweighting of gridder.py:509-532 with the residual visibilities ``resvis_dev`` (complex128 DeviceArray,
        ``(ncorr, nrow, nchan)``) in HBM: per correlation ``ovar = sum_{mask > 0} wgtp |r|^2 / mask.sum()`` and ``wgt *= (dof +
        2) / (dof + wgtp |r|^2 / ovar)``.  ``wgtp`` is a scalar, a host array or a float64 DeviceArray of the chunk's shape.
        Returns ``ovar``; raises ``ValueError`` and leaves the weights as they are when a variance is zero."""
        self._open()
        shape = (self.ncorr, self.nrow, self.nchan)
        if not isinstance(resvis_dev, DeviceArray) or resvis_dev.dtype != np.complex128 or tuple(resvis_dev.shape) != shape:
            raise ValueError(f"resvis_dev must be a complex128 DeviceArray of shape {shape}")
        own = None
        if isinstance(wgtp, DeviceArray):
            if wgtp.dtype != np.float64 or tuple(wgtp.shape) != shape:
                raise ValueError(f"wgtp on the device must be float64 of shape {shape}")
            wp, scalar = wgtp, 1.0
        elif np.ndim(wgtp) == 0:
            wp, scalar = None, float(wgtp)
        else:
            own = wp = DeviceArray.from_host(np.broadcast_to(np.asarray(wgtp, dtype=np.float64), shape))
            scalar = 1.0
        ovar = np.empty(self.ncorr, dtype=np.float64)
        try:
            check(lib().pfbhip_chunk_l2_reweight_dev(resvis_dev.ptr, None if wp is None else wp.ptr, scalar, self.mask.ptr,
                                                     self.wgt.ptr, self.ncorr, self.nvis, float(dof), ptr(ovar)))
        finally:
            if own is not None:
                own.free()
        return ovar

    # -- the snapshot imager's steps (utils/stokes2im.py; csrc/snapshot.hip) ---------------------------------------------
    def _check_rephase(self, w_diff, model):
        """``(w_diff (nrow) float64 or None, model)`` after the checks; no device call"""
        if w_diff is not None:
            w_diff = np.asarray(w_diff)
            if w_diff.dtype.kind not in "fiu":
                raise TypeError(f"w_diff must be real, not {w_diff.dtype}")
            if w_diff.shape == (self.nrow, 1):
                w_diff = w_diff.reshape(self.nrow)
            if w_diff.shape != (self.nrow,):
                raise ValueError(f"w_diff shape {w_diff.shape} != {(self.nrow,)}")
            w_diff = as_c(w_diff, np.float64)
        if model is not None:
            model = _adopt(model, (self.ncorr, self.nrow, self.nchan), np.complex128, "model")
        return w_diff, model

    def rephase_residual(self, w_diff=None, model=None):
        """stokes2im.py:364-373 and :466-468 of the reference in one in-place pass: ``vis = (vis p - model p) * mask`` with ``p =
        exp(-2 pi i freq / c * w_diff[row])``.  ``w_diff (nrow)`` or ``(nrow, 1)`` [m] is a host array (``None``: ``p = 1``);
        ``model``, Stokes model visibilities ``(ncorr, nrow, nchan)``, a host array (uploaded for the call) or a complex128
        ``DeviceArray`` (left as it is).  The mask applies only with a model."""
        w_diff, model = self._check_rephase(w_diff, model)
        self._open()
        wd = md = None
        try:
            if w_diff is not None:
                wd = DeviceArray.from_host(w_diff)
            if model is not None:
                md = model if isinstance(model, DeviceArray) else DeviceArray.from_host(as_c(model, np.complex128))
            check(lib().pfbhip_chunk_rephase_residual_dev(self.vis.ptr, None if md is None else md.ptr, self.mask.ptr,
                                                          None if wd is None else wd.ptr, ptr(self.freq), self.ncorr, self.nrow,
                                                          self.nchan))
        finally:
            if wd is not None:
                wd.free()
            if md is not None and md is not model:
                md.free()

    def l2_reweight_joint(self, dof):
        """The l2 reweighting in ``stokes_image``'s form (stokes2im.py:470-481) with the chunk's visibilities as the residual:
        ``ovar = sum over every correlation of |vis|^2 mask / mask.sum()`` and ``wgt = (dof + 1) / (dof + |vis|^2 mask / ovar)
        / ovar`` -- the weights are replaced.  Returns ``ovar``; raises ``ValueError`` and leaves the weights as they are when
        the residual is exactly zero or the mask is empty.  ``dof`` must be positive: a masked sample gets ``(dof + 1) / dof / ovar``."""
        dof = float(dof)
        if not (dof > 0 and np.isfinite(dof)):
            raise ValueError(f"dof = {dof} must be positive and finite")
        self._open()
        ovar = f64(0.0)
        check(lib().pfbhip_chunk_l2_reweight_joint_dev(self.vis.ptr, self.mask.ptr, self.wgt.ptr, self.ncorr, self.nvis, dof,
                                                       ct.byref(ovar)))
        return ovar.value

    def inject_transients(self, uvw, freq, time, sources, all_times, all_freqs, w_diff=None, beam=None):
        """:func:`~pfb_imaging_amd.utils.transients.inject_transients` (stokes2im.py:491-558) into the chunk's first Stokes plane
        where it lies: one accumulating direct-DFT predict per source, no download.  ``uvw`` are the coordinates the sources
        are simulated at (the reference's ``uvw_old``); ``freq`` must be the chunk's."""
        from .dft import DFT
        from .utils.transients import accumulate_sources

        uvw, freq, time = np.asarray(uvw, dtype=np.float64), np.asarray(freq, dtype=np.float64), np.asarray(time, dtype=np.float64)
        if uvw.shape != (self.nrow, 3):
            raise ValueError(f"uvw shape {uvw.shape} != {(self.nrow, 3)}")
        if freq.shape != (self.nchan,) or not np.array_equal(freq, self.freq):
            raise ValueError("freq must be the chunk's frequencies")
        if time.shape != (self.nrow,):
            raise ValueError(f"time {time.shape} != {(self.nrow,)}")
        w_diff, _ = self._check_rephase(w_diff, None)
        if beam is not None:
            beam = np.asarray(beam, dtype=np.float64)
            if beam.shape != (len(sources), self.nchan):
                raise ValueError(f"beam {beam.shape} != {(len(sources), self.nchan)}")
        self._open()
        if not len(sources):
            return
        plane = _lib.DeviceView(self.vis, 0, (self.nrow, self.nchan))
        with DFT(uvw, freq) as d:
            accumulate_sources(d, plane, time, freq, sources, all_times, all_freqs, w_diff, beam)

    def imaging_weights(self, nx_pad, ny_pad, cellx, celly, robust, filter_level=5.0, npix_super=0, usign=1.0, vsign=-1.0,
                        return_counts=False):
        """:func:`~pfb_imaging_amd.utils.weighting.imaging_weights` (gridder.py:534-576) on the resident weights, in place; the
        final counts ``(ncorr, nx_pad, ny_pad)`` come back with ``return_counts``."""
        self._open()
        counts = _lib.result_empty((self.ncorr, nx_pad, ny_pad), np.float64) if return_counts else None
        check(lib().pfbhip_imaging_weights_dev(ptr(self.uvw), ptr(self.freq), self.mask.ptr, self.wgt.ptr, self.ncorr, self.nrow,
                                               self.nchan, nx_pad, ny_pad, cellx, celly, usign, vsign, robust,
                                               filter_level or 0.0, int(npix_super or 0), ptr(counts)))
        return counts

    def weights(self):
        """The weights ``(ncorr, nrow, nchan)`` on the host (a download)."""
        self._open()
        return self.wgt.download()
