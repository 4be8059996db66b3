"""numpy statement of the Gaussian-resolution convolution and the restore step, and the inputs of the pinned cases.

Independent of the package: the padded sizes come from the oracle's ``good_size``, the transforms from ``numpy.fft`` (or any
module with ``rfft2`` / ``irfft2``, e.g. ``scipy.fft``).  tests/golden/make_restore_pins.py runs the reference's own functions
on :func:`case` 's inputs; the CPU test holds this statement against those runs, the GPU tests hold the device against both.
"""

import numpy as np

from oracle.wgridder import good_size

FWHM = 2.0 * np.sqrt(2.0 * np.log(2.0))
BOUND_FLOOR = 1e-11  # "double-precision FFTs of different factorisations" (tests/test_gpu_psf_hessian.py)


def offsets(nx, ny, sx=1.0, sy=1.0):
    """the coordinate grids restore_image builds, times a step per axis"""
    return np.meshgrid((-(nx // 2) + np.arange(nx)) * sx, (-(ny // 2) + np.arange(ny)) * sy, indexing="ij")


def pads(n, pfrac):
    nfft = good_size(n + int(pfrac * n), True)
    left = (nfft - n) // 2
    return nfft, left, nfft - n - left


def gaussian(xx, yy, par, normalise=False, nsigma=5):
    emaj, emin, pa = par
    rot = np.array([[-np.sin(pa), -np.cos(pa)], [np.cos(pa), -np.sin(pa)]])
    a = rot @ np.diag([1.0 / emaj**2, 1.0 / emin**2]) @ rot.T
    q = a[0, 0] * xx * xx + (a[0, 1] + a[1, 0]) * xx * yy + a[1, 1] * yy * yy
    k = np.where(xx**2 + yy**2 <= (nsigma * emaj / FWHM) ** 2, np.exp(-0.5 * FWHM**2 * q), 0.0)
    return k / k.sum() if normalise else k


def _hat(plane, nfx, lx, nfy, ly, fft):
    nx, ny = plane.shape
    p = np.zeros((nfx, nfy))
    p[lx:lx + nx, ly:ly + ny] = plane
    return fft.rfft2(np.fft.ifftshift(p))


def convolve(image, xx, yy, gaussparf, gausspari=None, pfrac=0.5, norm_kernel=False, fft=np.fft):
    nband, nx, ny = image.shape
    (nfx, lx, rx), (nfy, ly, ry) = pads(nx, pfrac), pads(ny, pfrac)
    assert rx > 0 and ry > 0
    gaussparf = np.asarray(gaussparf, dtype=float).reshape(-1, 3)
    out = np.empty_like(image, dtype=float)
    for b in range(nband):
        k = _hat(gaussian(xx, yy, gaussparf[b if len(gaussparf) > 1 else 0], norm_kernel), nfx, lx, nfy, ly, fft)
        if gausspari is not None:
            t = _hat(gaussian(xx, yy, gausspari[b], norm_kernel), nfx, lx, nfy, ly, fft)
            k = np.divide(k, t, out=np.zeros_like(k), where=np.abs(t) > 0)
        full = np.fft.fftshift(fft.irfft2(_hat(image[b], nfx, lx, nfy, ly, fft) * k, s=(nfx, nfy)))
        out[b] = full[lx:lx + nx, ly:ly + ny]
    return out


def restore(model, residual, wsum, gausspari, gaussparf, fft=np.fft):
    nband, nx, ny = model.shape
    xx, yy = offsets(nx, ny)
    gaussparf = np.asarray(gaussparf, dtype=float)
    if gaussparf.ndim == 1:
        gaussparf = np.tile(gaussparf, (nband, 1))
    res = residual / np.asarray(wsum)[:, None, None]
    out = convolve(model, xx, yy, gaussparf, pfrac=0.2, fft=fft)
    for b in range(nband):
        if np.allclose(gaussparf[b], gausspari[b]):
            out[b] += res[b]
        else:
            out[b] += convolve(res[b:b + 1], xx, yy, gaussparf[b], gausspari[b:b + 1], pfrac=0.2, fft=fft)[0]
    return out


# ---- the pinned cases ---------------------------------------------------------------------------------------------------
GAUSSPARI_C = np.array([[2.5, 2.0, 0.1], [2.4, 2.1, 0.9], [2.3, 2.2, 2.0]])
WSUM_D = np.array([2.0, 0.5, 1.0])  # powers of two: residual * wsum / wsum is exact


def point_model(nband, nx, ny):
    """a handful of point sources, two of them in opposite corners: wrap-around through the pad would show"""
    m = np.zeros((nband, nx, ny))
    for b in range(nband):
        m[b, 0, 0] = 1.0 + b
        m[b, nx - 1, ny - 1] = -2.5 + b
        m[b, nx // 2, ny // 2] = 3.0
        m[b, 3, ny - 4] = 0.75
        m[b, nx - 2, 5 + b] = -1.25
    return m


def case(name):
    """dict(image, xx, yy, gaussparf, gausspari, pfrac) of case A, B or C; D's dict(model, residual, wsum, gausspari, gaussparf)"""
    if name == "A":
        xx, yy = offsets(36, 50)
        return dict(image=point_model(3, 36, 50), xx=xx, yy=yy, gaussparf=np.array([6.0, 3.5, 0.7]), gausspari=None, pfrac=0.2)
    if name == "B":  # nband 2: the reference reads a (3, 3) gaussparf as ONE resolution (len(gaussparf) == 3, misc.py:153)
        xx, yy = offsets(40, 40)
        image = np.random.default_rng(40).standard_normal((2, 40, 40))
        # band 1: 5 sigma = 5 * 30 / 2.355 = 63.7 pixels, beyond the image's corners (28.3): the support test is never false
        return dict(image=image, xx=xx, yy=yy, gaussparf=np.array([[4.0, 3.0, 0.2], [30.0, 20.0, 1.1]]), gausspari=None, pfrac=0.5)
    if name == "C":
        xx, yy = offsets(36, 50)
        image = np.random.default_rng(3650).standard_normal((3, 36, 50))
        return dict(image=image, xx=xx, yy=yy, gaussparf=np.array([6.0, 5.0, 0.3]), gausspari=GAUSSPARI_C, pfrac=0.2)
    if name == "D":
        c = case("C")
        gaussparf = np.tile(c["gaussparf"], (3, 1))
        gaussparf[1] = GAUSSPARI_C[1]  # band 1 is at its final resolution already: the pass-through branch
        return dict(model=point_model(3, 36, 50), residual=c["image"] * WSUM_D[:, None, None], wsum=WSUM_D, gausspari=GAUSSPARI_C,
                    gaussparf=gaussparf)
    raise KeyError(name)


def rel_max(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def bound(disagreement):
    """ISSUE: the larger of 10 x the stored numpy-FFT / scipy-FFT disagreement of the reference runs and 1e-11"""
    return max(10.0 * float(disagreement), BOUND_FLOOR)
