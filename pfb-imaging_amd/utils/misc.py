"""Image-geometry helpers of ``pfb_imaging.utils.misc`` that sit on the hot path's boundary."""

import ctypes as ct
import logging

import numpy as np

from .. import _lib
from ..fft import good_size

LIGHTSPEED = 299792458.0
FWHM_CONV = 2 * np.sqrt(2 * np.log(2))


def _even_good_size(n):
    """Smallest even FFT-friendly size >= n (the reference bumps odd sizes by one and re-rounds until even)."""
    n = good_size(int(n))
    while n % 2:
        n = good_size(n + 1)
    return n


def set_image_size(max_blength, max_freq, field_of_view, super_resolution_factor, cell_size=None, nx=None, ny=None,
                   psf_oversize=2.0, log=None):
    """Cell size and image / PSF dimensions of an imaging run (/root/reference/src/pfb_imaging/utils/misc.py:888-953).

    ``max_blength`` [m] and ``max_freq`` [Hz] give the Nyquist cell ``cell_n = 1 / (2 uv_max)`` with
    ``uv_max = max_blength * max_freq / c``.  Without ``cell_size`` [arcsec] the cell is ``cell_n / super_resolution_factor``;
    without ``nx`` the image covers ``field_of_view`` [deg] with an even, FFT-friendly pixel count.  The PSF grid is
    ``psf_oversize`` times the image (128 pixels when ``psf_oversize`` is falsy), also even and FFT-friendly.

    Returns ``(nx, ny, nx_psf, ny_psf, cell_n, cell_rad, cell_deg)``; odd ``nx`` / ``ny`` raise ``NotImplementedError``.
    """
    if log is None:
        log = logging.getLogger(__name__)
    cell_n = 1.0 / (2.0 * max_blength * max_freq / LIGHTSPEED)
    arcsec = np.pi / (180.0 * 3600.0)
    if cell_size is None:
        cell_rad = cell_n / super_resolution_factor
        cell_size = cell_rad / arcsec
        log.info(f"Cell size set to {cell_size} arcseconds")
    else:
        cell_rad = cell_size * arcsec
        srf = cell_n / cell_rad
        if srf < 1:
            log.info(f"Warning - requested cell size of {cell_size} arcseconds could be sub-Nyquist.")
        log.info(f"Super resolution factor = {srf}")
    cell_deg = np.rad2deg(cell_rad)
    if nx is None:
        nx = ny = _even_good_size(int(field_of_view * 3600 / cell_size))
    else:
        ny = nx if ny is None else ny
        if nx % 2 or ny % 2:
            log.error("Only even number of pixels currently supported")
            raise NotImplementedError("Only even number of pixels currently supported")
        log.info(f"Field of view is ({nx * cell_deg:.3e},{ny * cell_deg:.3e}) degrees")
    nx_psf = _even_good_size(int(psf_oversize * nx)) if psf_oversize else 128
    ny_psf = _even_good_size(int(psf_oversize * ny)) if psf_oversize else 128
    return nx, ny, nx_psf, ny_psf, cell_n, cell_rad, cell_deg


def get_padding_info(nx, ny, pfrac):
    """``((left, right) per axis), unpad_x, unpad_y`` of a centred pad to ``good_size(n + int(pfrac * n), real=True)``
    (/root/reference/src/pfb_imaging/utils/misc.py:107-120): the left pad is the smaller half.  A right pad of zero makes the
    unpad slice ``slice(l, -0)``, which is empty -- the device plans refuse such a geometry."""
    padding = []
    for n in (nx, ny):
        extra = good_size(n + int(pfrac * n), True) - n
        padding.append((extra // 2, extra - extra // 2))
    (xl, xr), (yl, yr) = padding
    return tuple(padding), slice(xl, -xr), slice(yl, -yr)


def gaussian2d(xin, yin, gausspar=(1.0, 1.0, 0.0), normalise=True, nsigma=5):
    """Elliptical Gaussian on the coordinate grids ``xin, yin`` (/root/reference/src/pfb_imaging/utils/misc.py:468-502).

    ``gausspar = (emaj, emin, pa)``: FWHMs in the grids' units and the position angle in radians, in the rotation the
    reference uses for compatibility with FITS, ``[[-sin pa, -cos pa], [cos pa, -sin pa]]``.  The value is exactly zero outside
    ``x^2 + y^2 <= (nsigma * emaj / FWHM_CONV)^2``; ``normalise`` divides by the sum.  Host code: the device renders the same
    function inside ``convolve2gaussres`` (csrc/restore.hip)."""
    emaj, emin, pa = gausspar
    rot = np.array([[-np.sin(pa), -np.cos(pa)], [np.cos(pa), -np.sin(pa)]])
    quad = np.dot(np.dot(rot, np.array([[1.0 / emaj**2, 0], [0, 1.0 / emin**2]])), rot.T)
    x, y = xin.squeeze(), yin.squeeze()
    inside = np.where(x**2 + y**2 <= (nsigma * (emaj / FWHM_CONV)) ** 2)
    pts = np.array([x[inside].ravel(), y[inside].ravel()])
    kern = np.zeros(x.shape, dtype=np.float64)
    kern[inside] = np.exp(-0.5 * FWHM_CONV**2 * np.einsum("nb,bc,cn->n", pts.T, quad, pts))
    if normalise:
        kern /= np.sum(kern)
    return np.ascontiguousarray(kern.reshape(xin.shape), dtype=np.float64)


def _axis_scales(xx, yy, nx, ny):
    """``(sx, sy)`` when ``xx == (-(nx // 2) + arange(nx))[:, None] * sx`` and likewise ``yy`` along the second axis, element for
    element (the device then computes the very same coordinates); ``None`` for any other pair of grids."""
    scales = []
    for grid, n, axis in ((xx, nx, 0), (yy, ny, 1)):
        grid = np.asarray(grid, dtype=np.float64)
        if grid.shape != (nx, ny):
            return None
        off = (-(n // 2) + np.arange(n)).astype(np.float64)
        k = int(np.argmax(np.abs(off)))
        if off[k] == 0:  # a single pixel on this axis
            s = 1.0
        else:
            s = float(np.take(grid, k, axis=axis).flat[0] / off[k])
        want = (off * s)[:, None] if axis == 0 else (off * s)[None, :]
        if not (np.isfinite(s) and s != 0.0 and np.array_equal(grid, np.broadcast_to(want, grid.shape))):
            return None
        scales.append(s)
    return tuple(scales)


def convolve2gaussres(image, xx, yy, gaussparf, nthreads=1, gausspari=None, pfrac=0.5, norm_kernel=False):
    """Convolve the cube ``image`` (nband, nx, ny) to the resolution ``gaussparf`` on the GPU
    (/root/reference/src/pfb_imaging/utils/misc.py:123-192).

    ``gaussparf`` is one ``(emaj, emin, pa)`` or one per band, in the units of ``xx, yy``.  With ``gausspari`` (one triple per
    band: the resolution the cube has) the kernel is the ratio of the two Gaussians' transforms, zero where the denominator is.
    Grids that are scaled pixel offsets (``restore_image``'s, or those times a cell size) are rendered on the device; for any
    other grids the kernels come from :func:`gaussian2d` on the host and only the convolution runs on the device.  ``nthreads``
    is accepted and unused.  A ``pfrac`` that leaves no right pad raises ``ValueError`` (the reference returns an empty array)."""
    from ..gaussconv import cached_plan

    image = np.asarray(image)
    nband, nx, ny = image.shape
    if gausspari is not None and len(gausspari) != nband:
        raise ValueError("gausspari must be on length nband")
    gaussparf = np.asarray(gaussparf, dtype=np.float64)
    if gaussparf.shape not in ((3,), (nband, 3)):
        raise ValueError(f"gaussparf must be (emaj, emin, pa) or one such triple per band, not shape {gaussparf.shape}")
    plan = cached_plan(nband, nx, ny, pfrac)
    scales = _axis_scales(xx, yy, nx, ny)
    if scales is not None:
        return plan.apply(image, gaussparf, gausspari, norm_kernel=norm_kernel, scale=scales)
    kernf = np.stack([gaussian2d(xx, yy, p, normalise=norm_kernel) for p in gaussparf.reshape(-1, 3)])
    kerni = None if gausspari is None else np.stack([gaussian2d(xx, yy, p, normalise=norm_kernel) for p in gausspari])
    return plan.apply(image, gaussparf, gausspari, kernf=kernf, kerni=kerni)


def _finish_cleanbeam(pars, pixsize=1.0):
    """The reference's last step on the solver's results ``pars (nband, 3)`` in pixels, pixels, radians
    (reference utils/misc.py:615-625): a row whose first axis is the shorter one has its axes swapped and
    ``pi / 2`` added to its angle; the axes are scaled by ``pixsize``.  NaN rows (all-zero bands) stay NaN.  Host code."""
    pars = np.array(pars, dtype=np.float64).reshape(-1, 3)
    swap = pars[:, 0] < pars[:, 1]
    out = pars.copy()
    out[swap, 0], out[swap, 1] = pars[swap, 1], pars[swap, 0]
    out[swap, 2] = pars[swap, 2] + np.pi / 2
    out[:, :2] *= pixsize
    return out


def _cleanbeam_raw(psf, level=0.5, nsigma=10.0):
    """``(pars, info)`` of the device fit: ``pars (nband, 3)`` unswapped in pixel units and one dict per band of the
    ``pfbhip_cleanbeam_info`` record (``status`` as a name of ``_lib.CB_STATUS_NAMES``).  ``psf`` is a host array or a
    :class:`~pfb_imaging_amd._lib.DeviceArray`.  Refusals raise ``ValueError``; a fit that stops at a cap does not."""
    _lib.require_gpu()
    on_dev = isinstance(psf, _lib.DeviceArray)
    if not on_dev:
        psf = _lib.as_c(psf, np.float64)
    elif psf.dtype != np.float64:
        raise ValueError(f"the PSF cube on the device must be float64, not {psf.dtype}")
    if len(psf.shape) != 3:
        raise ValueError(f"psf must be (nband, nx, ny), not shape {psf.shape}")
    nband, nx, ny = psf.shape
    pars = np.empty((nband, 3), dtype=np.float64)
    info = (_lib.CleanbeamInfo * nband)()
    call = _lib.lib().pfbhip_cleanbeam_fit_dev if on_dev else _lib.lib().pfbhip_cleanbeam_fit
    _lib.check(call(psf.ptr if on_dev else _lib.ptr(psf), nband, nx, ny, level,
                    nsigma, _lib.ptr(pars), ct.cast(info, _lib.vp)))
    recs = [dict(status=_lib.CB_STATUS_NAMES[r.status], window=r.window, nit=r.nit, nlobe=r.nlobe, nfit=r.nfit, f=r.f,
                 p0=np.array(r.p0[:])) for r in info]
    return pars, recs


def _fitcleanbeam(psf, level, pixsize, nsigma):
    pars, recs = _cleanbeam_raw(psf, level, nsigma)
    for b, r in enumerate(recs):
        if r["status"] in ("iter_cap", "raise_cap"):  # (the reference prints its warning on L-BFGS-B's flag)
            logging.getLogger(__name__).warning(f"WARNING - psf fit of band {b} stopped at a cap ({r['status']}, {r['nit']} iterations)")
    return _finish_cleanbeam(pars, pixsize)


def fitcleanbeam(psf, level=0.5, pixsize=1.0, nsigma=10.0):
    """The Gaussian that approximates the main lobe of each band of ``psf (nband, nx, ny)``, fitted on the GPU
    (reference utils/misc.py:529-627; csrc/cleanbeam.hip).

    Per band: the main lobe is the 4-connected region above ``level`` of the peak around the centre pixel; its weighted second
    moments give the start; the Gaussian is fitted to the normalised PSF within ``nsigma`` standard deviations of the start's
    major axis.  Returns ``(nband, 3)`` rows ``(emaj * pixsize, emin * pixsize, pa)``, NaNs for an all-zero band.

    Two differences from the reference: a centre pixel that is not above ``level`` raises ``ValueError`` (the reference fits
    the background), and the result is the minimiser of the reference's objective under its bounds, not the point at which
    L-BFGS-B's ``factr=1e7`` stops -- for nearly circular beams the angles can differ by tenths of a radian at equal
    misfit.  A band whose maximum is not positive, or whose main lobe is wider than 256 pixels, raises ``ValueError``."""
    return _fitcleanbeam(psf, level, pixsize, nsigma)


def fitcleanbeam_dev(psf_dev, level=0.5, pixsize=1.0, nsigma=10.0):
    """:func:`fitcleanbeam` of a cube that is resident on the device (a float64 ``_lib.DeviceArray`` of shape
    ``(nband, nx, ny)``): nothing but the three numbers per band crosses to the host."""
    if not isinstance(psf_dev, _lib.DeviceArray):
        raise TypeError("fitcleanbeam_dev takes a _lib.DeviceArray; use fitcleanbeam for host arrays")
    return _fitcleanbeam(psf_dev, level, pixsize, nsigma)
