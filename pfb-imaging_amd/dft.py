"""Direct DFT of point components on the device (``pfbhip_dft``, csrc/dft.hip).

The measurement equation summed source by source, exactly: the definition the gridder approximates, usable where the model
is a list of points -- a component model's pixels, a few bright sources, a transient -- and where flux is wanted at a list
of positions.  No image, no plan, no FFT and no ``epsilon``.

Conventions are the caller's: ``signs = (su, sv, sw)`` multiply the baseline coordinates and ``sgn`` is the sign of the
exponent.  :func:`lm_of_pixels` is the one place where the gridder's conventions (``flip_*``, ``center_*``, pixel ``n/2`` at
the centre) are turned into them; the gridder's ``dirty2vis`` has ``sgn = -1``.
"""

import ctypes as ct

import numpy as np

from . import _lib
from ._lib import DFTConv, DeviceArray, as_c, check, lib, ptr


def _shifts_and_signs(center_x, center_y, flip_u, flip_v, flip_w):
    """``(lshift, mshift, su, sv, sw)`` of the gridder's conventions"""
    return (-center_x if flip_u else center_x, -center_y if flip_v else center_y, -1.0 if flip_u else 1.0, -1.0 if flip_v else 1.0,
            -1.0 if flip_w else 1.0)


def lm_of_pixels(ix, iy, nx, ny, cellx, celly, center_x=0.0, center_y=0.0, flip_u=False, flip_v=False, flip_w=False):
    """``(lm, su, sv, sw)`` of the pixels ``(ix, iy)`` of an ``(nx, ny)`` image under the gridder's conventions: pixel
    ``(nx // 2, ny // 2)`` sits at ``(lshift, mshift)`` with ``lshift = -center_x if flip_u else center_x`` (the same for
    v), and a flip negates the baseline coordinate.  ``lm`` is ``(npix, 2)`` float64."""
    ix, iy = np.asarray(ix, dtype=np.int64), np.asarray(iy, dtype=np.int64)
    if ix.ndim != 1 or ix.shape != iy.shape:
        raise ValueError(f"ix {ix.shape} and iy {iy.shape} must be equal-length vectors")
    lshift, mshift, su, sv, sw = _shifts_and_signs(center_x, center_y, flip_u, flip_v, flip_w)
    lm = np.empty((ix.size, 2), dtype=np.float64)
    lm[:, 0] = lshift + (ix - int(nx) // 2).astype(np.float64) * cellx
    lm[:, 1] = mshift + (iy - int(ny) // 2).astype(np.float64) * celly
    return lm, su, sv, sw


def _sign(v, name):
    v = float(v)
    if v not in (1.0, -1.0):
        raise ValueError(f"{name} must be +1 or -1, not {v}")
    return v


class DFT:
    """``uvw (nrow, 3)`` [m], ``freq (nchan)`` [Hz] and an optional ``mask (nrow, nchan)`` resident on the device."""

    def __init__(self, uvw, freq, mask=None):
        uvw, freq = as_c(uvw, np.float64), as_c(freq, np.float64)
        if uvw.ndim != 2 or uvw.shape[1] != 3 or uvw.shape[0] < 1:
            raise ValueError(f"uvw {uvw.shape} must be (nrow, 3) with nrow >= 1")
        if freq.ndim != 1 or freq.size < 1:
            raise ValueError(f"freq {freq.shape} must be a vector of at least one channel")
        if mask is not None:
            mask = as_c(np.asarray(mask) != 0, np.uint8)
            if mask.shape != (uvw.shape[0], freq.size):
                raise ValueError(f"mask {mask.shape} != {(uvw.shape[0], freq.size)}")
        _lib.require_gpu()
        self.nrow, self.nchan = int(uvw.shape[0]), int(freq.size)
        self._h = ct.c_void_p()
        check(lib().pfbhip_dft_create(self.nrow, self.nchan, ptr(uvw), ptr(freq), ptr(mask), ct.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().pfbhip_dft_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- argument checks (all before the first device call) ---------------------------------------------------------------
    def _conv(self, signs, sgn, do_wgridding, divide_by_n, accumulate, chans):
        if len(signs) != 3:
            raise ValueError("signs must be (su, sv, sw)")
        chan0, nsel = 0, self.nchan
        if chans is not None:
            if not isinstance(chans, slice):
                raise ValueError("chans must be a slice of the handle's channels")
            chan0, stop, step = chans.indices(self.nchan)
            nsel = stop - chan0
            if step != 1 or nsel < 1:
                raise ValueError(f"chans {chans} must select at least one channel, contiguously")
        cv = DFTConv(_sign(signs[0], "su"), _sign(signs[1], "sv"), _sign(signs[2], "sw"), _sign(sgn, "sgn"), int(bool(do_wgridding)),
                     int(bool(divide_by_n)), int(bool(accumulate)), 0, chan0, nsel)
        return cv, nsel

    def _vector(self, a, shape, name):
        if a is None:
            return None
        a = as_c(a, np.float64)
        if a.shape != shape:
            raise ValueError(f"{name} {a.shape} != {shape}")
        return a

    def _off(self, off):
        if off is None:
            return None
        off = as_c(off, np.float64)
        if off.shape == (self.nrow, 1):
            off = off.reshape(self.nrow)
        if off.shape != (self.nrow,):
            raise ValueError(f"off {off.shape} != {(self.nrow,)}")
        return off

    def _wgt(self, wgt, nsel, dev):
        if wgt is None:
            return None
        if dev != isinstance(wgt, DeviceArray):
            raise ValueError("wgt must live where vis lives: both host arrays or both DeviceArrays")
        if not dev:
            wgt = as_c(wgt, np.float64)
        if tuple(wgt.shape) != (self.nrow, nsel) or wgt.dtype != np.float64:
            raise ValueError(f"wgt {tuple(wgt.shape)} {wgt.dtype} must be float64 {(self.nrow, nsel)}")
        return wgt

    def _target(self, out, nsel, accumulate):
        """(array, is_device) the visibilities go to"""
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs the visibilities to add to: pass out=")
            return _lib.result_empty((self.nrow, nsel), np.complex128), False
        dev = isinstance(out, DeviceArray)
        if tuple(out.shape) != (self.nrow, nsel) or out.dtype != np.complex128 or not (dev or out.flags.c_contiguous):
            raise ValueError(f"out must be C-contiguous complex128 of shape {(self.nrow, nsel)}")
        return out, dev

    @staticmethod
    def _p(a, dev):
        if a is None:
            return None
        return a.ptr if dev else ptr(a.view(np.float64) if a.dtype == np.complex128 else a)

    # -- the three operations -----------------------------------------------------------------------------------------
    def predict(self, lm, amp, rowf=None, chanf=None, off=None, wgt=None, signs=(1.0, 1.0, 1.0), sgn=-1.0, do_wgridding=True,
                divide_by_n=True, accumulate=False, out=None, chans=None):
        """``vis[r, c] (+)= wgt[r, c] sum_s amp[s] rowf[s, r] chanf[s, c] / N_s exp(sgn 2 pi i f_c / c0 (su u l_s + sv v m_s
        - sw w (n_s - 1) + off_r))`` for every unmasked sample.  ``lm (nsrc, 2)``, ``amp (nsrc)``, ``rowf (nsrc, nrow)``,
        ``chanf (nsrc, nchan)`` and ``off (nrow)`` [m] are host arrays; ``out`` / ``wgt`` are host arrays or
        :class:`DeviceArray`\\ s (both of the same kind).  Without ``accumulate`` masked samples are written as 0; with it
        they are left as they are.  ``chans`` (a slice) restricts the call to some of the handle's channels."""
        cv, nsel = self._conv(signs, sgn, do_wgridding, divide_by_n, accumulate, chans)
        lm, amp = as_c(lm, np.float64), as_c(amp, np.float64)
        if lm.ndim != 2 or lm.shape[1] != 2 or amp.shape != (lm.shape[0],):
            raise ValueError(f"lm {lm.shape} must be (nsrc, 2) and amp {amp.shape} (nsrc,)")
        nsrc = lm.shape[0]
        rowf = self._vector(rowf, (nsrc, self.nrow), "rowf")
        chanf = self._vector(chanf, (nsrc, nsel), "chanf")
        off = self._off(off)
        out, dev = self._target(out, nsel, accumulate)
        wgt = self._wgt(wgt, nsel, dev)
        f = lib().pfbhip_dft_predict_dev if dev else lib().pfbhip_dft_predict
        check(f(self._h, ct.byref(cv), nsrc, ptr(lm), ptr(amp), ptr(rowf), ptr(chanf), ptr(off), self._p(wgt, dev),
                self._p(out, dev)))
        return out

    def predict_comps(self, comps, bvec, cellx, celly, center_x=0.0, center_y=0.0, flip_u=False, flip_v=False, flip_w=False,
                      region=False, off=None, wgt=None, sgn=-1.0, do_wgridding=True, divide_by_n=True, accumulate=False, out=None,
                      chans=None):
        """:meth:`predict` of a resident :class:`~pfb_imaging_amd.comps.Comps` model under the gridder's conventions: sources
        at the handle's pixels (:func:`lm_of_pixels`), ``amp = bvec @ coeffs`` -- gated by the handle's region mask with
        ``region`` -- formed on the device.  Only ``bvec`` goes up."""
        lshift, mshift, su, sv, sw = _shifts_and_signs(center_x, center_y, flip_u, flip_v, flip_w)
        cv, nsel = self._conv((su, sv, sw), sgn, do_wgridding, divide_by_n, accumulate, chans)
        bvec = as_c(bvec, np.float64)
        if bvec.shape != (comps.nparam,):
            raise ValueError(f"basis vector shape {bvec.shape} != {(comps.nparam,)}")
        off = self._off(off)
        out, dev = self._target(out, nsel, accumulate)
        wgt = self._wgt(wgt, nsel, dev)
        f = lib().pfbhip_dft_predict_comps_dev if dev else lib().pfbhip_dft_predict_comps
        check(f(self._h, ct.byref(cv), comps._h, ptr(bvec), int(bool(region)), cellx, celly, lshift, mshift,
                ptr(off), self._p(wgt, dev), self._p(out, dev)))
        return out

    def image(self, lm, vis, wgt=None, off=None, signs=(1.0, 1.0, 1.0), sgn=-1.0, do_wgridding=True, divide_by_n=True, chans=None):
        """The adjoint of :meth:`predict` in ``amp`` (with ``rowf = chanf = 1``): ``out[s] = sum_{r, c} mask wgt Re(vis[r, c]
        exp(-sgn 2 pi i ...)) / N_s``, a host vector ``(nsrc,)``.  ``vis`` / ``wgt`` are host arrays or ``DeviceArray``\\ s.  The
        sums run in a fixed order: the same input gives the same bits."""
        cv, nsel = self._conv(signs, sgn, do_wgridding, divide_by_n, False, chans)
        lm = as_c(lm, np.float64)
        if lm.ndim != 2 or lm.shape[1] != 2:
            raise ValueError(f"lm {lm.shape} must be (nsrc, 2)")
        dev = isinstance(vis, DeviceArray)
        if not dev:
            vis = as_c(vis, np.complex128)
        if tuple(vis.shape) != (self.nrow, nsel) or vis.dtype != np.complex128:
            raise ValueError(f"vis {tuple(vis.shape)} {vis.dtype} must be complex128 {(self.nrow, nsel)}")
        wgt = self._wgt(wgt, nsel, dev)
        off = self._off(off)
        out = np.zeros(lm.shape[0], dtype=np.float64)
        f = lib().pfbhip_dft_image_dev if dev else lib().pfbhip_dft_image
        check(f(self._h, ct.byref(cv), lm.shape[0], ptr(lm), ptr(off), self._p(wgt, dev), self._p(vis, dev), ptr(out)))
        return out


def dft_dirty2vis(uvw, freq, dirty, pixsize_x, pixsize_y, center_x=0.0, center_y=0.0, flip_u=False, flip_v=False, flip_w=False,
                  do_wgridding=True, divide_by_n=True, rows=None, chans=None):
    """Exact visibilities of the non-zero pixels of a host image; the keywords of ``oracle.dft.dft_dirty2vis``.  ``rows`` /
    ``chans`` (equal-length index arrays) restrict the result to those (row, channel) pairs (returns 1-D)."""
    uvw, freq = as_c(uvw, np.float64), as_c(freq, np.float64)
    dirty = as_c(dirty, np.float64)
    if dirty.ndim != 2:
        raise ValueError(f"dirty {dirty.shape} must be 2-D")
    if (rows is None) != (chans is None):
        raise ValueError("rows and chans select (row, channel) pairs: give both or neither")
    ix, iy = np.nonzero(dirty)
    lm, su, sv, sw = lm_of_pixels(ix, iy, dirty.shape[0], dirty.shape[1], pixsize_x, pixsize_y, center_x, center_y, flip_u, flip_v,
                                  flip_w)
    kw = dict(signs=(su, sv, sw), sgn=-1.0, do_wgridding=do_wgridding, divide_by_n=divide_by_n)
    if rows is None:
        with DFT(uvw, freq) as d:
            return d.predict(lm, dirty[ix, iy], **kw)
    rows, chans = np.asarray(rows, dtype=np.int64), np.asarray(chans, dtype=np.int64)
    if rows.ndim != 1 or rows.shape != chans.shape:
        raise ValueError(f"rows {rows.shape} and chans {chans.shape} must be equal-length vectors")
    if rows.size == 0:
        return np.zeros(0, dtype=np.complex128)
    # the pairs as the unmasked samples of the (rows present) x (channels present) block
    ur, ri = np.unique(rows, return_inverse=True)
    uc, ci = np.unique(chans, return_inverse=True)
    mask = np.zeros((ur.size, uc.size), dtype=np.uint8)
    mask[ri, ci] = 1
    with DFT(uvw[ur], freq[uc], mask) as d:
        return d.predict(lm, dirty[ix, iy], **kw)[ri, ci]


def dft_vis2dirty(uvw, freq, vis, wgt, mask, npix_x, npix_y, pixsize_x, pixsize_y, center_x=0.0, center_y=0.0, flip_u=False,
                  flip_v=False, flip_w=False, do_wgridding=True, divide_by_n=True, pixels=None):
    """Exact dirty image ``(npix_x, npix_y)``, or its values at ``pixels = (ix, iy)`` (returns 1-D); the keywords of
    ``oracle.dft.dft_vis2dirty``."""
    if pixels is None:
        ix, iy = (a.ravel() for a in np.meshgrid(np.arange(int(npix_x)), np.arange(int(npix_y)), indexing="ij"))
    else:
        ix, iy = pixels
    lm, su, sv, sw = lm_of_pixels(ix, iy, npix_x, npix_y, pixsize_x, pixsize_y, center_x, center_y, flip_u, flip_v, flip_w)
    with DFT(uvw, freq, mask) as d:
        out = d.image(lm, vis, wgt=wgt, signs=(su, sv, sw), sgn=-1.0, do_wgridding=do_wgridding, divide_by_n=divide_by_n)
    return out.reshape(int(npix_x), int(npix_y)) if pixels is None else out
