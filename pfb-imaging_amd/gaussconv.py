"""Gaussian-resolution convolution and restore on the device (Python face of ``pfbhip_gaussconv_*``, csrc/restore.hip).

A ``GaussConvPlan`` belongs to one ``(nband, nx, ny, pfrac)``: it owns the padded plane, the spectra and the rocFFT plans of
that geometry.  ``cached_plan`` keeps the last two geometries used.  ``utils.misc.convolve2gaussres`` and
``utils.restoration.restore_arrays`` are the reference-signature entry points; DESIGN.md ("Gaussian-resolution convolution and
restore") lists the semantics kept.
"""

import collections
import ctypes as ct

import numpy as np

from . import _lib
from ._lib import as_c, check, i64, lib, ptr


def _pars(p, name):
    """(n, 3) float64 rows of (emaj, emin, pa); a single triple becomes one row."""
    p = as_c(p, np.float64)
    if p.ndim == 1:
        p = p[None]
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"{name} must be (emaj, emin, pa) or rows of it, not shape {p.shape}")
    return p


def _dptr(a):
    return None if a is None else a.ptr


class GaussConvPlan:
    def __init__(self, nband, nx, ny, pfrac=0.5):
        self.nband, self.nx, self.ny, self.pfrac = int(nband), int(nx), int(ny), float(pfrac)
        self._h = ct.c_void_p()
        st = lib().pfbhip_gaussconv_create(self.nband, self.nx, self.ny, self.pfrac, ct.byref(self._h))
        if st == 2:  # a geometry error (status 1) is reported as such with or without a device
            _lib.require_gpu()
        check(st)
        v = [i64(0) for _ in range(4)]
        check(lib().pfbhip_gaussconv_shape(self._h, *(ct.byref(x) for x in v)))
        self.nfft_x, self.nfft_y, self.padl_x, self.padl_y = (int(x.value) for x in v)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().pfbhip_gaussconv_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def shape(self):
        return (self.nband, self.nx, self.ny)

    def _host_cube(self, a, name, n=None):
        a = as_c(a, np.float64)
        want = (self.nband if n is None else n, self.nx, self.ny)
        if a.shape != want:
            raise ValueError(f"{name} shape {a.shape} != {want}")
        return a

    def _dev_cube(self, a, name, n=None):
        want = (self.nband if n is None else n, self.nx, self.ny)
        if not isinstance(a, _lib.DeviceArray) or a.dtype != np.float64 or tuple(a.shape) != want:
            raise ValueError(f"{name} must be a float64 DeviceArray of shape {want}")
        return a

    def _par_args(self, gaussparf, gausspari):
        pf = _pars(gaussparf, "gaussparf")
        pi = None if gausspari is None else _pars(gausspari, "gausspari")
        return pf, pi, (ptr(pf), pf.shape[0], ptr(pi), 0 if pi is None else pi.shape[0])

    def apply(self, image, gaussparf, gausspari=None, norm_kernel=False, scale=(1.0, 1.0), kernf=None, kerni=None, out=None):
        """Host cube in, host cube out.  ``scale``: the coordinate step of each axis (kernels are rendered on
        ``(-(n // 2) + arange(n)) * scale``); ``kernf`` / ``kerni``: kernels rendered by the caller instead."""
        image = self._host_cube(image, "image")
        pf, pi, pargs = self._par_args(gaussparf, gausspari)
        if kernf is not None:
            kernf = self._host_cube(kernf, "kernf", pf.shape[0])
        if kerni is not None:
            kerni = self._host_cube(kerni, "kerni")
        if out is None:
            out = _lib.result_empty(self.shape, np.float64)
        check(lib().pfbhip_gaussconv_apply(self._h, ptr(image), *pargs, int(bool(norm_kernel)), scale[0], scale[1], ptr(kernf),
                                           ptr(kerni), ptr(out)))
        return out

    def apply_dev(self, image_dev, out_dev, gaussparf, gausspari=None, norm_kernel=False, scale=(1.0, 1.0), kernf_dev=None,
                  kerni_dev=None):
        """:meth:`apply` between ``DeviceArray`` cubes."""
        self._dev_cube(image_dev, "image_dev")
        self._dev_cube(out_dev, "out_dev")
        pf, pi, pargs = self._par_args(gaussparf, gausspari)
        if kernf_dev is not None:
            self._dev_cube(kernf_dev, "kernf_dev", pf.shape[0])
        if kerni_dev is not None:
            self._dev_cube(kerni_dev, "kerni_dev")
        check(lib().pfbhip_gaussconv_apply_dev(self._h, image_dev.ptr, *pargs, int(bool(norm_kernel)), scale[0], scale[1],
                                               _dptr(kernf_dev), _dptr(kerni_dev), out_dev.ptr))

    def _restore_args(self, wsum, gausspari, gaussparf):
        w = as_c(wsum, np.float64).reshape(-1)
        if w.size != self.nband:
            raise ValueError(f"wsum holds {w.size} values for {self.nband} bands")
        pf, pi, _ = self._par_args(gaussparf, gausspari)
        return w, pi, pf, (ptr(w), ptr(pi), pi.shape[0], ptr(pf), pf.shape[0])

    def restore(self, model, residual, wsum, gausspari, gaussparf, out=None):
        """``conv(model; gaussparf) + rconv`` in one call (host cubes); see ``utils.restoration.restore_arrays``."""
        model, residual = self._host_cube(model, "model"), self._host_cube(residual, "residual")
        *keep, rargs = self._restore_args(wsum, gausspari, gaussparf)
        if out is None:
            out = _lib.result_empty(self.shape, np.float64)
        check(lib().pfbhip_gaussconv_restore(self._h, ptr(model), ptr(residual), *rargs, ptr(out)))
        return out

    def restore_dev(self, model_dev, residual_dev, image_dev, wsum, gausspari, gaussparf):
        for a, name in ((model_dev, "model_dev"), (residual_dev, "residual_dev"), (image_dev, "image_dev")):
            self._dev_cube(a, name)
        *keep, rargs = self._restore_args(wsum, gausspari, gaussparf)
        check(lib().pfbhip_gaussconv_restore_dev(self._h, model_dev.ptr, residual_dev.ptr, *rargs, image_dev.ptr))

    def debug_fill(self, byte=0xFF):
        """Test hook: every buffer of the plan filled with ``byte`` (0xFF: NaNs)."""
        check(lib().pfbhip_gaussconv_debug_fill(self._h, int(byte)))


_plans = collections.OrderedDict()
_MAX_PLANS = 2  # a plan at 8192^2, pfrac 0.2 holds 3.2 GB


def cached_plan(nband, nx, ny, pfrac):
    """The plan of this geometry, made on first use and kept while it is among the last two used."""
    key = (int(nband), int(nx), int(ny), float(pfrac))
    plan = _plans.get(key)
    if plan is None:
        plan = GaussConvPlan(*key)
        _plans[key] = plan
        while len(_plans) > _MAX_PLANS:
            _, old = _plans.popitem(last=False)
            old.close()
    else:
        _plans.move_to_end(key)
    return plan


def clear_cache():
    while _plans:
        _, p = _plans.popitem()
        p.close()
