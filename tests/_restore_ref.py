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


SHIFTS = (np.fft.ifftshift, np.fft.fftshift)  # on load, on store; they differ on an axis of odd length only


def _hat(plane, nfx, lx, nfy, ly, fft, ifftshift=np.fft.ifftshift):
    nx, ny = plane.shape
    p = np.zeros((nfx, nfy))
    p[lx:lx + nx, ly:ly + ny] = plane
    return fft.rfft2(ifftshift(p))


def convolve(image, xx, yy, gaussparf, gausspari=None, pfrac=0.5, norm_kernel=False, fft=np.fft, kernf=None, kerni=None,
             shifts=SHIFTS):
    """``kernf (1 or nband, nx, ny)`` / ``kerni (nband, nx, ny)``: kernel images used as they are in place of the Gaussians of
    ``gaussparf`` / ``gausspari``; ``shifts``: the two shifts, for the guard that exchanges them."""
    nband, nx, ny = image.shape
    (nfx, lx, rx), (nfy, ly, ry) = pads(nx, pfrac), pads(ny, pfrac)
    assert rx > 0 and ry > 0
    gaussparf = np.asarray(gaussparf, dtype=float).reshape(-1, 3)
    out = np.empty_like(image, dtype=float)
    for b in range(nband):
        kb = b if len(gaussparf) > 1 else 0
        k = _hat(gaussian(xx, yy, gaussparf[kb], norm_kernel) if kernf is None else kernf[kb], nfx, lx, nfy, ly, fft, shifts[0])
        if gausspari is not None:
            t = _hat(gaussian(xx, yy, gausspari[b], norm_kernel) if kerni is None else kerni[b], nfx, lx, nfy, ly, fft, shifts[0])
            k = np.divide(k, t, out=np.zeros_like(k), where=np.abs(t) > 0)
        full = shifts[1](fft.irfft2(_hat(image[b], nfx, lx, nfy, ly, fft, shifts[0]) * k, s=(nfx, nfy)))
        out[b] = full[lx:lx + nx, ly:ly + ny]
    return out


def thishat(c, norm_kernel=False, fft=np.fft):
    """the spectra of a ratio case's intrinsic kernels, padded and shifted as :func:`convolve` does: (nband, nfft_x, nfft_y // 2 + 1)"""
    nband, nx, ny = c["image"].shape
    (nfx, lx, _), (nfy, ly, _) = pads(nx, c["pfrac"]), pads(ny, c["pfrac"])
    return np.stack([_hat(gaussian(c["xx"], c["yy"], p, norm_kernel), nfx, lx, nfy, ly, fft) for p in c["gausspari"]])


def restore(model, residual, wsum, gausspari, gaussparf, fft=np.fft, shifts=SHIFTS):
    nband, nx, ny = model.shape
    xx, yy = offsets(nx, ny)
    gaussparf = np.asarray(gaussparf, dtype=float)
    if gaussparf.ndim == 1:
        gaussparf = np.tile(gaussparf, (nband, 1))
    res = residual / np.asarray(wsum)[:, None, None]
    out = convolve(model, xx, yy, gaussparf, pfrac=0.2, fft=fft, shifts=shifts)
    for b in range(nband):
        if np.allclose(gaussparf[b], gausspari[b]):
            out[b] += res[b]
        else:
            out[b] += convolve(res[b:b + 1], xx, yy, gaussparf[b], gausspari[b:b + 1], pfrac=0.2, fft=fft, shifts=shifts)[0]
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
    """dict(image, xx, yy, gaussparf, gausspari, pfrac) of a convolution case; dict(model, residual, wsum, gausspari, gaussparf)
    of the restores D and K"""
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
    if name in _EDGE:
        return _EDGE[name]()
    raise KeyError(name)


# ---- the edge cases: every launch form of csrc/restore.hip (kernel_forms below), pinned in restore_edge_pins.npz ------------
J_SCALE = (2.5e-5, -2.0e-5)  # a negative step on y: with pa != 0 the cross term of the quadratic form changes sign
J_RES = 2.0e-5               # the resolutions of J_scaled in the grids' units: one pixel of y


def _edge_image(nband, nx, ny, seed):
    """seeded standard-normal noise, on top of the point sources where they fit"""
    noise = np.random.default_rng(seed).standard_normal((nband, nx, ny))
    return noise + point_model(nband, nx, ny) if nx >= 6 and ny >= 12 else noise


def _edge(shape, pfrac, gaussparf, gausspari=None, seed=0, scale=(1.0, 1.0)):
    xx, yy = offsets(shape[1], shape[2], *scale)
    return dict(image=_edge_image(*shape, seed), xx=xx, yy=yy, gaussparf=np.asarray(gaussparf, dtype=float),
                gausspari=None if gausspari is None else np.asarray(gausspari, dtype=float), pfrac=pfrac)


def _case_k():
    gaussparf = np.tile([6.0, 5.0, 0.3], (2, 1))
    gaussparf[1] = GAUSSPARI_C[1]  # band 1 is at its final resolution already, as D's band 1
    wsum = np.array([4.0, 0.25])
    return dict(model=point_model(2, 7, 301), residual=_edge_image(2, 7, 301, 11) * wsum[:, None, None], wsum=wsum,
                gausspari=GAUSSPARI_C[:2], gaussparf=gaussparf)


_PAR_J = np.array([6.0, 5.0, 0.3])
_EDGE = {
    "E": lambda: _edge((1, 7, 301), 0.2, [6.0, 3.5, 0.7], seed=5),
    "F": lambda: _edge((2, 5, 520), 0.2, [[4.0, 3.0, 0.2], [30.0, 20.0, 1.1]], seed=6),
    "G": lambda: _edge((2, 6, 540), 0.5, [6.0, 5.0, 0.3], GAUSSPARI_C[:2], seed=7),
    "H": lambda: _edge((3, 2, 3), 0.5, [1.5, 1.2, 0.4], seed=8),
    "H_ratio": lambda: _edge((3, 2, 3), 0.5, [1.5, 1.2, 0.4], np.tile([1.0, 0.9, 0.1], (3, 1)), seed=8),
    "I": lambda: _edge((1, 5, 427), 0.2, [6.0, 3.5, 0.7], GAUSSPARI_C[:1], seed=9),
    "J": lambda: _edge((1, 7, 301), 0.2, _PAR_J, GAUSSPARI_C[2:3], seed=10),
    "J_scaled": lambda: _edge((1, 7, 301), 0.2, _PAR_J * [J_RES, J_RES, 1.0], GAUSSPARI_C[2:3] * [J_RES, J_RES, 1.0], seed=10,
                              scale=J_SCALE),
    "K": _case_k,
    # not in the issue's table, which has no odd padded row of one trip: 12 x 10 pads to 18 x 15.  Per-band gaussparf AND gausspari.
    "L": lambda: _edge((2, 12, 10), 0.5, [[4.0, 3.0, 0.2], [5.0, 4.0, 1.1]], GAUSSPARI_C[:2], seed=12),
}

# every pinned run: key of the fixture -> (case, norm_kernel).  D and K are restores, the others convolutions.
EDGE_RUNS = {"E_norm0": ("E", False), "E_norm1": ("E", True), "F": ("F", False), "G_norm0": ("G", False), "G_norm1": ("G", True),
             "H": ("H", False), "H_ratio": ("H_ratio", False), "I": ("I", False), "J": ("J", False), "J_scaled": ("J_scaled", False),
             "L": ("L", False)}
RUNS = {"A_norm0": ("A", False), "A_norm1": ("A", True), "B": ("B", False), "C": ("C", False), **EDGE_RUNS}
RESTORES = {"D": 0.2, "K": 0.2}  # case -> pfrac (restore_image's)


def geometry(name):
    """(nband, nx, ny, pfrac) of a case"""
    c = case(name)
    return (*(c["image"] if "image" in c else c["model"]).shape, c.get("pfrac", 0.2))


def kernel_forms(nband, nx, ny, pfrac):
    """The launch choices csrc/restore.hip makes for this geometry, restated: the elements per lane ``V`` of the pad and render
    passes (2 where the padded row is even) and of the crop pass (2 where the image row is even; a cube that is not 16-byte
    aligned takes 1 as well), the trips of the row loop ``for (j0 = lane * V; j0 < len; j0 += 256 * V)``, and the pads."""
    (nfx, lx, rx), (nfy, ly, ry) = pads(nx, pfrac), pads(ny, pfrac)
    vpad, vcrop = 2 - nfy % 2, 2 - ny % 2
    return dict(nband=nband, nfft=(nfx, nfy), pads=((lx, rx), (ly, ry)), odd=(nfx % 2 == 1, nfy % 2 == 1),
                pad_v=vpad, pad_trips=-(-nfy // (256 * vpad)), crop_v=vcrop, crop_trips=-(-ny // (256 * vcrop)),
                left_pad_zero=(lx == 0, ly == 0))


def rel_max(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def bound(disagreement):
    """ISSUE: the larger of 10 x the stored numpy-FFT / scipy-FFT disagreement of the reference runs and 1e-11"""
    return max(10.0 * float(disagreement), BOUND_FLOOR)
