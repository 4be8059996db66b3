"""Device-resident component model: pixel locations and coefficients in HBM (``pfbhip_comps``, csrc/comps.hip).

The reference keeps a model as ``(coefficients (nparam, ncomps), location_x, location_y)`` plus the strings of a
parametrisation (utils/modelspec.py of pfb-imaging).  Both parametrisations it writes are linear in the
coefficients, so a render at ``(t, f)`` is ``image[x_index, y_index] = b(t, f) . coeffs`` with ``b = modelf(t, f, *eye)``:
only the ``nparam`` numbers of ``b`` cross PCIe per render.  :func:`basis_vector` obtains ``b`` and refuses to do so for a
``modelf`` that is not linear.
"""

import ctypes as ct

import numpy as np

from . import _lib
from ._lib import as_c, check, cint, i64, lib, ptr

_EPS = 2.0**-53


def basis_vector(modelf, tt, ff, nparam, rng=None):
    """``b`` with ``modelf(tt, ff, *c) == b . c`` for every ``c``, or ``None`` when ``modelf`` is not linear in its parameters.

    ``b = modelf(tt, ff, *eye(nparam))``.  Two checks guard it: ``modelf(tt, ff, *0)`` must be 0, and a random coefficient
    vector ``r`` must reproduce ``b . r`` within ``8 nparam 2^-53 sum|b_k r_k|`` (the rounding of two orders of the same
    ``nparam`` products).  A nonlinear parametrisation is never silently linearised: the caller renders it on the host."""
    nparam = int(nparam)
    try:
        b = np.asarray(modelf(tt, ff, *np.eye(nparam)), dtype=np.float64)
        if b.ndim == 0:
            b = np.full(nparam, float(b))
        zero = np.asarray(modelf(tt, ff, *np.zeros(nparam)), dtype=np.float64)
        rng = np.random.default_rng(20240229) if rng is None else rng
        r = rng.uniform(0.5, 1.5, nparam) * rng.choice([-1.0, 1.0], nparam)
        direct = np.asarray(modelf(tt, ff, *r), dtype=np.float64)
    except Exception:  # (a modelf that cannot take these arguments is not one we can vouch for)
        return None
    if b.shape != (nparam,) or not np.isfinite(b).all() or zero.ndim != 0 or direct.ndim != 0:
        return None
    if float(zero) != 0.0:
        return None
    if not abs(float(direct) - float(b @ r)) <= 8 * nparam * _EPS * float(np.abs(b * r).sum()):
        return None
    return b


class Comps:
    """Component model resident on the device.  ``x_index, y_index, coeffs`` are the host copies."""

    def __init__(self, nx, ny, x_index, y_index, coeffs):
        _lib.require_gpu()
        x_index, y_index = as_c(x_index, np.int64), as_c(y_index, np.int64)
        coeffs = as_c(coeffs, np.float64)
        if coeffs.ndim != 2 or x_index.ndim != 1 or x_index.shape != y_index.shape or coeffs.shape[1] != x_index.size:
            raise ValueError(f"coeffs {coeffs.shape} must be (nparam, ncomps) with {x_index.size} locations")
        if coeffs.shape[0] < 1:
            raise ValueError("a component model needs at least one parameter")
        self._h = ct.c_void_p()
        check(lib().pfbhip_comps_create(int(nx), int(ny), x_index.size, coeffs.shape[0], ptr(x_index), ptr(y_index), ptr(coeffs),
                                        ct.byref(self._h)))
        self.nx, self.ny, self.ncomps, self.nparam = int(nx), int(ny), int(x_index.size), int(coeffs.shape[0])
        self.x_index, self.y_index, self.coeffs = x_index, y_index, coeffs
        self.host_renders = 0  # renders a caller had to make on the host (nonlinear modelf): see operators.gridder.comps2vis

    @classmethod
    def fit(cls, cube, A, shape=None):
        """Support mask, ``np.where`` compaction and ``coeffs = A @ cube[:, x_index, y_index]`` on the device.  ``cube`` is a
        host array ``(ns, nx, ny)`` or a :class:`~pfb_imaging_amd._lib.DeviceArray`; ``A`` is ``(nparam, ns)``.  ``shape``
        reads a cube of the same number of elements as ``(ns, nx, ny)`` (e.g. a device cube ``(ntime, nband, nx, ny)``)."""
        _lib.require_gpu()
        A = as_c(A, np.float64)
        dev = isinstance(cube, _lib.DeviceArray)
        if not dev:
            cube = as_c(cube, np.float64)
        if shape is None:
            shape = tuple(cube.shape)
        shape = tuple(int(v) for v in shape)
        if int(np.prod(shape, dtype=np.int64)) != int(np.prod(cube.shape, dtype=np.int64)):
            raise ValueError(f"shape {shape} does not hold the cube's {tuple(cube.shape)} elements")
        if len(shape) != 3 or A.ndim != 2 or A.shape[1] != shape[0]:
            raise ValueError(f"cube {shape} must be (ns, nx, ny) and A {A.shape} (nparam, ns)")
        if dev and cube.dtype != np.float64:
            raise ValueError("the device cube must be float64")
        ns, nx, ny = shape
        self = cls.__new__(cls)
        self._h = ct.c_void_p()
        n = i64(0)
        check(lib().pfbhip_comps_fit(None if dev else ptr(cube), cube.ptr if dev else None, ns, nx, ny, ptr(A), A.shape[0],
                                     ct.byref(self._h), ct.byref(n)))
        self.nx, self.ny, self.ncomps, self.nparam = nx, ny, int(n.value), int(A.shape[0])
        self.x_index, self.y_index = np.empty(self.ncomps, np.int64), np.empty(self.ncomps, np.int64)
        self.coeffs = np.empty((self.nparam, self.ncomps), np.float64)
        check(lib().pfbhip_comps_get(self._h, ptr(self.x_index), ptr(self.y_index), ptr(self.coeffs)))
        self.host_renders = 0
        return self

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().pfbhip_comps_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_region(self, region_mask):
        """Bind ``region_mask`` (nx, ny), uploaded once; ``None`` unbinds it."""
        if region_mask is None:
            check(lib().pfbhip_comps_set_region(self._h, None))
            return
        m = as_c(np.asarray(region_mask) != 0, np.uint8)
        if m.shape != (self.nx, self.ny):
            raise ValueError(f"region mask shape {m.shape} != {(self.nx, self.ny)}")
        check(lib().pfbhip_comps_set_region(self._h, ptr(m)))

    def _basis(self, b):
        b = as_c(b, np.float64)
        if b.shape != (self.nparam,):
            raise ValueError(f"basis vector shape {b.shape} != {(self.nparam,)}")
        return b

    def render(self, b, region=False, out=None):
        """Host image ``(nx, ny)`` of ``b . coeffs`` at the component locations, zero elsewhere (and outside the bound region
        mask when ``region``)."""
        if out is None:
            out = _lib.result_empty((self.nx, self.ny), np.float64)
        elif out.shape != (self.nx, self.ny) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of the image shape")
        check(lib().pfbhip_comps_render(self._h, ptr(self._basis(b)), int(bool(region)), ptr(out)))
        return out

    def render_dev(self, b, out_dev, region=False):
        """:meth:`render` into a ``DeviceArray`` of the image shape (every pixel is written)."""
        if tuple(out_dev.shape) != (self.nx, self.ny) or out_dev.dtype != np.float64:
            raise ValueError(f"out_dev must be a float64 DeviceArray of shape {(self.nx, self.ny)}")
        check(lib().pfbhip_comps_render_dev(self._h, ptr(self._basis(b)), int(bool(region)), out_dev.ptr))


def _regrid_args(nxi, nyi, cellxi, cellyi, x0i, y0i, nxo, nyo, cellxo, cellyo, x0o, y0o):
    return (int(nxi), int(nyi), cellxi, cellyi, x0i, y0i, int(nxo), int(nyo), cellxo, cellyo, x0o, y0o)


def regrid(image, cellxi, cellyi, x0i, y0i, nxo, nyo, cellxo, cellyo, x0o, y0o):
    """The second half of the reference's ``eval_coeffs_to_slice`` (modelspec.py:277-332) on a host image: bilinear
    interpolation onto the output grid times the pixel-area ratio, the input zero-extended as far as the output reaches; the
    image itself (zero-padded, no area ratio) when the reference's test finds nothing to interpolate."""
    image = as_c(image, np.float64)
    out = _lib.result_empty((int(nxo), int(nyo)), np.float64)
    check(lib().pfbhip_comps_regrid(ptr(image), *_regrid_args(image.shape[0], image.shape[1], cellxi, cellyi, x0i, y0i, nxo, nyo,
                                                              cellxo, cellyo, x0o, y0o), ptr(out), None))
    return out


def regrid_dev(in_dev, cellxi, cellyi, x0i, y0i, out_dev, cellxo, cellyo, x0o, y0o):
    """:func:`regrid` between two ``DeviceArray`` images; returns True when it interpolated."""
    flag = cint(0)
    check(lib().pfbhip_comps_regrid_dev(in_dev.ptr, *_regrid_args(in_dev.shape[0], in_dev.shape[1], cellxi, cellyi, x0i, y0i,
                                                                  out_dev.shape[0], out_dev.shape[1], cellxo, cellyo, x0o, y0o),
                                        out_dev.ptr, ct.byref(flag)))
    return bool(flag.value)
