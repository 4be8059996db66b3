"""Primary beams on the device (``pfbhip_beam_*``, csrc/beam.hip): the regrid of a beam onto the image grid and the
azimuthal average that builds the ``BEAM`` product.

``eval_beam`` is the reference's ``pfb_imaging.utils.beam.eval_beam`` (utils/beam.py:75-89); ``rotate_mean`` is the rotation
loop of utils/stokes2vis_msv4.py:405-409.  Both return page-locked arrays.
"""

import ctypes as ct

import numpy as np

from .. import _lib
from .._lib import as_c, check, f64, lib, ptr

DEFAULT_ANGLES = np.linspace(0, 359, 25)  # stokes2vis_msv4.py:405-406


def _nodes(a, name):
    a = as_c(a, np.float64)
    if a.ndim != 1 or a.size < 2:
        raise ValueError(f"{name} must be a 1-D array of at least two nodes, not shape {a.shape}")
    if not (np.diff(a) > 0.0).all():  # (NaN fails this too)
        raise ValueError(f"The points in dimension {name} must be strictly ascending")
    return a


def eval_beam(beam_image, l_in, m_in, l_out, m_out, info=None):
    """``beam_image`` on the nodes ``(l_in, m_in)`` interpolated linearly at the output coordinates, 1.0 outside the nodes
    and exact ones for a beam that is identically 1.0.

    ``l_out, m_out`` are 1-D axes ``(nx,), (ny,)`` of the output grid or 2-D coordinate arrays ``(nx, ny)``; the result is
    ``(nx, ny)``.  ``beam_image`` may also be a stack ``(ncorr, nl, nm)``: every correlation goes through one launch and
    the result is ``(ncorr, nx, ny)``.  ``info`` (a dict) receives ``device_ms``, the time of the kernels alone."""
    l_out, m_out = np.asarray(l_out), np.asarray(m_out)
    if l_out.ndim not in (1, 2):
        raise ValueError("Only 1 or 2D coordinates supported for beam evaluation")
    general = l_out.ndim == 2
    if general and m_out.shape != l_out.shape:
        raise ValueError(f"l_out {l_out.shape} and m_out {m_out.shape} must have the same shape")
    if not general and m_out.ndim != 1:
        raise ValueError(f"m_out must be 1-D like l_out, not shape {m_out.shape}")
    l_in, m_in = _nodes(l_in, "l_in"), _nodes(m_in, "m_in")
    beam = as_c(beam_image, np.float64)
    stack = beam.ndim == 3
    if beam.ndim not in (2, 3) or beam.shape[-2:] != (l_in.size, m_in.size):
        raise ValueError(f"beam_image {beam.shape} does not match the nodes ({l_in.size}, {m_in.size})")
    nx, ny = l_out.shape if general else (l_out.size, m_out.size)
    ncorr = beam.shape[0] if stack else 1
    if ncorr < 1 or nx < 1 or ny < 1:
        raise ValueError(f"nothing to evaluate: ncorr = {ncorr}, output ({nx}, {ny})")
    _lib.require_gpu()
    l_out, m_out = as_c(l_out, np.float64), as_c(m_out, np.float64)
    out = _lib.result_empty((ncorr, nx, ny) if stack else (nx, ny), np.float64)
    ms = f64(0.0)
    check(lib().pfbhip_beam_regrid(ptr(beam), ncorr, l_in.size, m_in.size, ptr(l_in), ptr(m_in), ptr(l_out), ptr(m_out),
                                   int(general), nx, ny, ptr(out), ct.byref(ms) if info is not None else None))
    if info is not None:
        info["device_ms"] = ms.value
    return out


def rotate_mean(beam0, angles=DEFAULT_ANGLES, info=None):
    """Mean over ``angles`` (degrees) of ``beam0`` rotated about its centre with cubic splines, the image kept at its shape
    and extended by its edge values: ``mean(ndimage.rotate(beam0, angle, reshape=False, mode="nearest"))`` in one pass.
    ``beam0`` is ``(n0, n1)`` or a stack ``(ncorr, n0, n1)``.  ``info`` (a dict) receives ``device_ms``."""
    beam = as_c(beam0, np.float64)
    if beam.ndim not in (2, 3) or 0 in beam.shape:
        raise ValueError(f"beam0 must be (n0, n1) or (ncorr, n0, n1), not shape {beam.shape}")
    angles = as_c(np.atleast_1d(angles), np.float64)
    if angles.ndim != 1 or angles.size < 1 or not np.isfinite(angles).all():
        raise ValueError("angles must be a non-empty 1-D array of finite values")
    _lib.require_gpu()
    ncorr = beam.shape[0] if beam.ndim == 3 else 1
    out = _lib.result_empty(beam.shape, np.float64)
    ms = f64(0.0)
    check(lib().pfbhip_beam_rotate_mean(ptr(beam), ncorr, beam.shape[-2], beam.shape[-1], ptr(angles), angles.size, ptr(out),
                                        ct.byref(ms) if info is not None else None))
    if info is not None:
        info["device_ms"] = ms.value
    return out
