"""``hogbom`` and ``clark`` with the signatures of pfb-imaging's deconv/hogbom.py and deconv/clark.py, run on the GPU.

Both return ``(model, status)`` (status 1 when the iteration limit was reached, else 0) with the model in ``dirty.dtype``.
float64 inputs are computed in float64 in the reference's order of operations: Hogbom matches the reference bit for bit,
Clark up to the last bits of the major cycle's FFT.  float32 inputs are widened and the model cast back, so those results are
not bit-comparable with a float32 run of the reference.

Kept from the reference on purpose (DESIGN.md "Device-resident CLEAN"):
- no stall stop: the reference's counter does ``stall_count += stall_count`` from 0 and never fires;
- Clark's sub-minor loop reads the PSF reflected, ``psf[nxo2 - (p_i - p), nyo2 - (q_i - q)]``, the opposite shift to Hogbom
  and to the major-cycle convolution;
- its ``xhat`` is a view into the active set, so active pixels after the peak (row-major) are reduced with the peak's value
  AFTER its own update, the peak and the pixels before it with the value before.
Where the reference would fail, arguments are checked up front and raise ``ValueError`` before any GPU work: a band whose
PSF peak is <= 0 (Hogbom), wsums that do not sum to 1 or are all zero, subpf outside (0, 1), gamma <= 0.  Clark leaves bands
with ``wsums == 0`` alone (the reference divides by their weight).  Without a GPU a valid call raises ``RuntimeError``.

Pinned to runs of the reference itself (tests/golden/clean_pins.npz, tests/test_gpu_clean_pins.py): the float64 bit identity
of Hogbom and of Clark's first major cycle, Clark over several major cycles within ten times the reference's own
numpy-FFT / scipy-FFT disagreement, the first maximum in row-major order (ties included), the missing stall stop, the
reflected sub-minor PSF and its in-range clip, the aliased ``xhat`` and the mask in the major search only.  Two claims are
NOT pinned, because the reference is undefined there, and rest on the numpy yardstick alone: bands with ``wsums == 0``
(the reference divides by zero) and a Hogbom PSF smaller than ``2 nx - 1`` (the reference's slice raises; here the PSF counts
as 0 outside its array).  The float32 path is pinned at a tolerance, not bit for bit: same support, k and status, the model
within ten times the difference between the reference's own float32 and float64 runs.
"""

import logging

import numpy as np

from . import _lib
from .clean import cached_plan

log = logging.getLogger(__name__)


def _cube(name, a):
    a = np.asarray(a)
    if a.ndim != 3 or min(a.shape) < 1:
        raise ValueError(f"{name} must be a non-empty (nband, nx, ny) cube, got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"{name} must be real floating point, got {a.dtype}")
    return a


def _common(dirty, psf, gamma, pf, maxit):
    dirty, psf = _cube("dirty", dirty), _cube("psf", psf)
    if psf.shape[0] != dirty.shape[0]:
        raise ValueError(f"psf has {psf.shape[0]} bands, dirty {dirty.shape[0]}")
    if not gamma > 0:
        raise ValueError(f"gamma must be > 0, got {gamma}")
    if not np.isfinite(pf):
        raise ValueError(f"pf must be finite, got {pf}")
    if int(maxit) < 0:
        raise ValueError(f"maxit must be >= 0, got {maxit}")
    return dirty, psf


def _report(status, k, rmax, residual, model, verbosity):
    if not verbosity:
        return
    resid_mfs = residual.sum(axis=0)
    empty = ~np.any(model, axis=0)
    rms = np.std(resid_mfs[empty]) if empty.any() else float("nan")
    if status:
        log.info(f"Max iters reached. Max resid = {rmax:.3e}, rms = {rms:.3e}")
    else:
        log.info(f"Success, converged after {k} iterations. Max resid = {rmax:.3e}, rms = {rms:.3e}")


def hogbom(dirty, psf, threshold=0, gamma=0.1, pf=0.1, maxit=10000, report_freq=1000, verbosity=1):
    """Hogbom CLEAN of ``dirty`` (nband, nx, ny) with ``psf`` (nband, nx_psf, ny_psf); see the module docstring."""
    del report_freq  # the loop runs on the device; progress is reported once at the end
    dirty, psf = _common(dirty, psf, gamma, pf, maxit)
    peaks = psf.reshape(psf.shape[0], -1).max(axis=1)
    if not np.all(peaks > 0):
        raise ValueError(f"every band's PSF needs a positive peak (max(psf[b]) = {peaks.tolist()})")
    _lib.require_gpu()
    plan = cached_plan(psf, None, dirty.shape[1], dirty.shape[2])
    out = plan.hogbom(dirty, threshold, gamma, pf, maxit, residual=bool(verbosity))  # the residual only feeds the log line
    model, status = out[0], out[1]
    _report(status, plan.info["iters"], plan.info["rmax"], out[-1], model, verbosity)
    return model.astype(dirty.dtype, copy=False), status


def clark(dirty, psf, psfhat, wsums, mask, threshold=0, gamma=0.05, pf=0.05, maxit=50, subpf=0.5, submaxit=1000,
          report_freq=1, verbosity=1, nthreads=1):
    """Clark CLEAN; ``psfhat`` (nband, nx_psf, ny_psf // 2 + 1) is the transform the major cycle convolves with, as in
    ``psf_convolve_cube``; ``wsums`` (nband,) sum to 1; ``mask`` (nx, ny) multiplies the major-cycle search image."""
    del report_freq, nthreads
    dirty, psf = _common(dirty, psf, gamma, pf, maxit)
    nband, nx, ny = dirty.shape
    _, nx_psf, ny_psf = psf.shape
    if nx_psf < nx or ny_psf < ny:
        raise ValueError(f"the PSF {psf.shape[1:]} must be at least the image size {(nx, ny)}")
    psfhat = np.asarray(psfhat)
    if psfhat.shape != (nband, nx_psf, ny_psf // 2 + 1):
        raise ValueError(f"psfhat shape {psfhat.shape} != {(nband, nx_psf, ny_psf // 2 + 1)}")
    wsums = np.asarray(wsums, dtype=np.float64).reshape(-1)
    if wsums.shape != (nband,):
        raise ValueError(f"wsums must have one entry per band ({nband}), got {wsums.size}")
    if np.any(wsums < 0) or not np.all(np.isfinite(wsums)):
        raise ValueError("wsums must be finite and non-negative")
    if not np.any(wsums > 0):
        raise ValueError("wsums are all zero")
    if not np.allclose(wsums.sum(), 1):
        raise ValueError(f"wsums must sum to 1, got {wsums.sum()}")
    try:
        mask = np.broadcast_to(np.asarray(mask, dtype=np.float64), (nx, ny))
    except ValueError:
        raise ValueError(f"mask of shape {np.shape(mask)} does not broadcast to {(nx, ny)}") from None
    if not 0 < subpf < 1:
        raise ValueError(f"subpf must be in (0, 1), got {subpf}")
    if int(submaxit) < 0:
        raise ValueError(f"submaxit must be >= 0, got {submaxit}")
    _lib.require_gpu()
    plan = cached_plan(psf, psfhat, nx, ny)
    out = plan.clark(dirty, wsums, mask, threshold, gamma, pf, maxit, subpf, submaxit, residual=bool(verbosity))
    model, status = out[0], out[1]
    _report(status, plan.info["iters"], plan.info["rmax"], out[-1], model, verbosity)
    return model.astype(dirty.dtype, copy=False), status
