"""Device-resident Hogbom and Clark CLEAN (Python face of ``pfbhip_clean_*``, csrc/clean.hip).

A ``CleanPlan`` keeps the PSF cube -- and, for Clark, psfhat in the slots of an internal PSF-convolution plan -- resident on
the GPU together with the dirty, residual and model cubes and the active-set buffers.  ``cached_plan`` returns the plan of a
(psf, psfhat) pair by content, so kclean's one ``clark`` call per major cycle uploads the PSF once.  The algorithms and the
reference quirks they keep are listed in DESIGN.md ("Device-resident CLEAN"); ``deconv.hogbom`` / ``deconv.clark`` are the
reference-signature entry points.
"""

import collections
import ctypes as ct

import numpy as np

from . import _lib
from ._lib import CleanInfo, as_c, check, lib, ptr

INFO_FIELDS = tuple(name for name, _ in CleanInfo._fields_)


class CleanPlan:
    """``psf`` (nband, nx_psf, ny_psf); ``psfhat`` (nband, nx_psf, ny_psf // 2 + 1) complex, or None for a Hogbom-only plan.
    The image size (nx, ny) is fixed by the first call; ``.info`` holds the last call's counters as a dict."""

    def __init__(self, psf, psfhat=None, nx=None, ny=None):
        _lib.require_gpu()
        psf = as_c(psf, np.float64)
        self.nband, self.nx_psf, self.ny_psf = psf.shape
        self.nx = int(nx if nx is not None else self.nx_psf)
        self.ny = int(ny if ny is not None else self.ny_psf)
        hat = None
        if psfhat is not None:
            hat = as_c(psfhat, np.complex128)
            if hat.shape != (self.nband, self.nx_psf, self.ny_psf // 2 + 1):
                raise ValueError(f"psfhat shape {hat.shape} != {(self.nband, self.nx_psf, self.ny_psf // 2 + 1)}")
        self.has_psfhat = hat is not None
        self.info = None
        self._h = ct.c_void_p()
        check(lib().pfbhip_clean_create(self.nband, self.nx, self.ny, self.nx_psf, self.ny_psf, ptr(psf), ptr(hat),
                                        ct.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().pfbhip_clean_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _cube(self, dirty):
        d = as_c(dirty, np.float64)
        if d.shape != (self.nband, self.nx, self.ny):
            raise ValueError(f"dirty shape {d.shape} != {(self.nband, self.nx, self.ny)}")
        return d

    def _finish(self, info):
        self.info = {name: getattr(info, name) for name in INFO_FIELDS}
        return info.status

    def hogbom(self, dirty, threshold=0.0, gamma=0.1, pf=0.1, maxit=10000, residual=False):
        """Returns ``(model, status)``, or ``(model, status, residual)`` with ``residual=True`` (float64)."""
        d = self._cube(dirty)
        model = np.empty_like(d)
        res = np.empty_like(d) if residual else None
        info = CleanInfo()
        check(lib().pfbhip_clean_hogbom(self._h, ptr(d), threshold, gamma, pf, int(maxit), ptr(model), ptr(res), ct.byref(info)))
        status = self._finish(info)
        return (model, status, res) if residual else (model, status)

    def clark(self, dirty, wsums, mask, threshold=0.0, gamma=0.05, pf=0.05, maxit=50, subpf=0.5, submaxit=1000,
              residual=False):
        """Returns ``(model, status)``, or ``(model, status, residual)`` with ``residual=True`` (float64)."""
        if not self.has_psfhat:
            raise ValueError("this CleanPlan was made without psfhat: Hogbom only")
        d = self._cube(dirty)
        w = as_c(wsums, np.float64).reshape(-1)
        m = as_c(np.broadcast_to(mask, (self.nx, self.ny)), np.float64)
        model = np.empty_like(d)
        res = np.empty_like(d) if residual else None
        info = CleanInfo()
        check(lib().pfbhip_clean_clark(self._h, ptr(d), ptr(w), ptr(m), threshold, gamma, pf, int(maxit), subpf, int(submaxit),
                                       ptr(model), ptr(res), ct.byref(info)))
        status = self._finish(info)
        return (model, status, res) if residual else (model, status)


_plans = collections.OrderedDict()
_MAX_PLANS = 2  # a plan at 4096^2 x 8 bands holds ~13 GB


def cached_plan(psf, psfhat, nx, ny):
    """The plan of this (psf, psfhat, image size), made on first use and kept while it is among the last two used."""
    key = (_lib.content_key(psf), _lib.content_key(psfhat), int(nx), int(ny))
    plan = _plans.get(key)
    if plan is None:
        plan = CleanPlan(psf, psfhat, nx, ny)
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
