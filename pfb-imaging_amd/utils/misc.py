"""Image-geometry helpers of ``pfb_imaging.utils.misc`` that sit on the hot path's boundary."""

import logging

import numpy as np

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
