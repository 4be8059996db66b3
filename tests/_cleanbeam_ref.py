"""Cases and a numpy restatement of the clean-beam fit (reference ``utils/misc.py:505-613``), shared by
``tests/golden/make_cleanbeam_pins.py``, ``tests/test_cleanbeam_cpu.py`` and ``tests/test_gpu_cleanbeam.py``.

numpy only, no random generator: every PSF is a rotated Gaussian plus a cosine ripple that vanishes at the centre, so the
peak is exactly 1 at ``(nx // 2, ny // 2)``; the ripple moves the minimiser off the Gaussian's own parameters and leaves a
non-zero residual.  The steps are those of DESIGN.md section 14: (a) normalise, (b) main lobe, (c) start point, (d) fit
region, (e) objective.  ``lm_fit`` restates the device's projected Levenberg-Marquardt iteration."""

import math
import os

import numpy as np

FWHM = 2 * np.sqrt(2 * np.log(2))
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cleanbeam_pins.npz")
LEVEL, NSIGMA = 0.5, 10.0

# name -> (shape, (emaj, emin, pa), ripple)
BEAMS = {
    "A": ((128, 128), (6.0, 3.5, 0.7), 0.05),
    "B": ((130, 96), (9.0, 8.5, 2.9), 0.05),
    "C": ((97, 128), (7.0, 4.0, 0.4), 0.05),
    "D": ((64, 64), (2.2, 1.8, 0.2), 0.03),
    "E": ((256, 256), (40.0, 25.0, 1.0), 0.05),
    "E2": ((256, 256), (80.0, 50.0, 1.0), 0.05),   # lobe half-length 40 > 32: the 64-window doubles
    "F": ((64, 60), (20.0, 12.0, 2.2), 0.05),
    "I2": ((128, 128), (5.0, 3.0, 2.0), 0.05),      # third band of case I
}
FITTED = ("A", "B", "C", "D", "E", "E2", "F", "G", "I2")   # cases with a pinned fit (one band each)
ALL = FITTED + ("H",)


def offsets(shape):
    nx, ny = shape
    return np.meshgrid(-(nx // 2) + np.arange(nx), -(ny // 2) + np.arange(ny), indexing="ij")


def quad(p, x, y):
    """q of psf_errorsq: [x y] R diag(1/emaj^2, 1/emin^2) R^T [x y]^T with R = [[-sin pa, -cos pa], [cos pa, -sin pa]]."""
    s, c = np.sin(p[2]), np.cos(p[2])
    u0, u1 = -s * x + c * y, -c * x - s * y
    return u0 * u0 / p[0] ** 2 + u1 * u1 / p[1] ** 2, u0, u1


def beam(shape, pars, ripple):
    xx, yy = offsets(shape)
    g = np.exp(-0.5 * FWHM**2 * quad(pars, xx, yy)[0])
    return g + ripple * np.cos(0.45 * np.sqrt(xx * xx + yy * yy)) * (1.0 - g)


def grow(above, seed):
    """4-connected component of the boolean image ``above`` that holds ``seed`` (all False when the seed is not set)."""
    lobe = np.zeros_like(above)
    lobe[seed] = above[seed]
    while True:
        nxt = lobe.copy()
        nxt[1:] |= lobe[:-1]
        nxt[:-1] |= lobe[1:]
        nxt[:, 1:] |= lobe[:, :-1]
        nxt[:, :-1] |= lobe[:, 1:]
        nxt &= above
        if (nxt == lobe).all():
            return lobe
        lobe = nxt


def _spiral(shape, turns=7, step=4):
    """A one-pixel-wide square spiral ridge from the centre outwards; arms ``step`` pixels apart."""
    img = np.zeros(shape)
    i, j = shape[0] // 2, shape[1] // 2
    img[i, j] = 1.0
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))
    for seg in range(4 * turns):
        di, dj = dirs[seg % 4]
        for _ in range(step * (seg // 2 + 1)):
            i, j = i + di, j + dj
            img[i, j] = 0.9
    return img


def _case_c():
    shape, pars, ripple = BEAMS["C"]
    psf = beam(shape, pars, ripple)
    cx, cy = shape[0] // 2, shape[1] // 2
    psf[cx + 30:cx + 34, cy - 45:cy - 41] = 0.8                  # an island far from the centre
    above = psf > LEVEL
    lobe = grow(above, (cx, cy))
    # the first pixel (row-major) that touches the lobe through a corner only and has no neighbour above the level
    for i in range(1, shape[0] - 1):
        for j in range(1, shape[1] - 1):
            if above[i, j] or above[i - 1, j] or above[i + 1, j] or above[i, j - 1] or above[i, j + 1]:
                continue
            if lobe[i - 1, j - 1] or lobe[i - 1, j + 1] or lobe[i + 1, j - 1] or lobe[i + 1, j + 1]:
                psf[i, j] = 0.8
                return psf
    raise AssertionError("case C: no diagonal-only neighbour of the lobe")


_cache = {}


def case(name):
    """``(nband, nx, ny)`` cube of the case (read-only, built once)."""
    if name not in _cache:
        if name == "G":
            psf = case("A") * 3.7
        elif name == "C":
            psf = _case_c()[None]
        elif name == "H":
            psf = _spiral((128, 128))[None]
        elif name == "I":
            psf = np.stack([case("A")[0], np.zeros((128, 128)), case("I2")[0]])
        else:
            psf = beam(*BEAMS[name])[None]
        psf = np.ascontiguousarray(psf, dtype=np.float64)
        psf.flags.writeable = False
        _cache[name] = psf
    return _cache[name]


def normalised(psf2d):
    return psf2d / psf2d.max()


def main_lobe(psfv, level=LEVEL):
    return grow(psfv > level, (psfv.shape[0] // 2, psfv.shape[1] // 2))


def start_point(psfv, lobe, total=np.sum):
    """(emaj0, emin0, pa0) of misc.py:569-591; ``total`` is the summation (``np.sum`` as the reference, or ``math.fsum``)."""
    xx, yy = offsets(psfv.shape)
    x, y, w = xx[lobe].astype(np.float64), yy[lobe].astype(np.float64), psfv[lobe]
    wsum = total(w)
    dx = x - total(w * x) / wsum
    dy = y - total(w * y) / wsum
    mxx, myy, mxy = total(w * dx**2) / wsum, total(w * dy**2) / wsum, total(w * dx * dy) / wsum
    pa0 = float(np.clip(np.pi / 2 + 0.5 * np.arctan2(2 * mxy, mxx - myy), 0.0, np.pi))
    ct, st = np.cos(np.pi / 2 + pa0), np.sin(np.pi / 2 + pa0)
    xr, yr = ct * dx + st * dy, -st * dx + ct * dy
    return np.array([max(xr.max() - xr.min(), 1.0), max(yr.max() - yr.min(), 1.0), pa0])


def fit_region(shape, emaj0, nsigma=NSIGMA):
    xx, yy = offsets(shape)
    return xx**2 + yy**2 < (nsigma * (emaj0 / FWHM)) ** 2


def residual_jac(p, data, x, y):
    """r = data - exp(-c^2 q / 2) and dr/dp (n, 3)."""
    q, u0, u1 = quad(p, x, y)
    m = np.exp(-0.5 * FWHM**2 * q)
    km = 0.5 * FWHM**2 * m
    jac = np.stack([km * (-2 * u0 * u0 / p[0] ** 3), km * (-2 * u1 * u1 / p[1] ** 3),
                    km * (2 * u0 * u1 * (1 / p[0] ** 2 - 1 / p[1] ** 2))], axis=1)
    return data - m, jac


def objective(p, data, x, y):
    r = data - np.exp(-0.5 * FWHM**2 * quad(p, x, y)[0])
    return float(np.dot(r, r))


def problem(name, band=0):
    """Steps (a)-(d) of one band: dict with psfv, lobe, p0, region and the fit's data ``(data, x, y)`` as float64 vectors."""
    key = ("problem", name, band)
    if key not in _cache:
        psfv = normalised(case(name)[band])
        lobe = main_lobe(psfv)
        p0 = start_point(psfv, lobe)
        region = fit_region(psfv.shape, p0[0])
        xx, yy = offsets(psfv.shape)
        _cache[key] = dict(psfv=psfv, lobe=lobe, p0=p0, region=region,
                           data=(psfv[region], xx[region].astype(np.float64), yy[region].astype(np.float64)))
    return _cache[key]


def f(p, name, band=0):
    """The reference's objective of the case at ``p``."""
    return objective(np.asarray(p, dtype=np.float64), *problem(name, band)["data"])


def window_for(lobe):
    """The window the device ends with: the smallest of 64, 128, 256 in which the lobe touches no edge that is not also
    an image edge (``None`` beyond 256)."""
    nx, ny = lobe.shape
    cx, cy = nx // 2, ny // 2
    ii, jj = np.nonzero(lobe)
    for w in (64, 128, 256):
        x0, x1, y0, y1 = max(cx - w // 2, 0), min(cx + w // 2, nx), max(cy - w // 2, 0), min(cy + w // 2, ny)
        if ii.min() < x0 or ii.max() >= x1 or jj.min() < y0 or jj.max() >= y1:
            continue
        touch = ((x0 > 0 and ii.min() == x0) or (x1 < nx and ii.max() == x1 - 1)
                 or (y0 > 0 and jj.min() == y0) or (y1 < ny and jj.max() == y1 - 1))
        if not touch:
            return w
    return None


def lm_fit(data, x, y, p0, max_iter=200, max_raise=30):
    """The device's iteration (csrc/cleanbeam.hip, k_cb_fit) restated: damped Gauss-Newton steps projected onto
    emaj >= 0, emin >= 0, 0 <= pa <= pi; a variable on a bound with the gradient pushing outwards is held.  Returns
    ``(p, f, nit, converged)``."""
    lo, hi = np.zeros(3), np.array([np.inf, np.inf, np.pi])

    def sums(p):
        r, jac = residual_jac(np.maximum(p, [1e-12, 1e-12, -np.inf]), data, x, y)
        return float(r @ r), jac.T @ r, jac.T @ jac

    p = np.array(p0, dtype=np.float64)
    fp, g, h = sums(p)
    lam = 1e-3
    for it in range(max_iter):
        fixed = ((p <= lo) & (g > 0)) | ((p >= hi) & (g < 0)) | ~(np.diag(h) > 0)
        moved = small = False
        for _ in range(max_raise):
            m = h + lam * np.diag(np.diag(h))
            rhs = -g.copy()
            for i in np.nonzero(fixed)[0]:
                m[i, :] = m[:, i] = 0.0
                m[i, i], rhs[i] = 1.0, 0.0
            try:
                d = np.linalg.solve(m, rhs)
            except np.linalg.LinAlgError:
                lam *= 10
                continue
            t = np.clip(p + d, lo, hi)
            small = bool(np.all(np.abs(t - p) <= 1e-12 * (1 + np.abs(p))))
            if small:
                break
            ft, gt, ht = sums(t)
            if ft <= fp:
                p, fp, g, h, lam, moved = t, ft, gt, ht, max(lam * 0.1, 1e-12), True
                break
            lam *= 10
        if small:
            return p, fp, it + 1, True
        if not moved:
            return p, fp, it + 1, False
    return p, fp, max_iter, False


def fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def load_pins():
    with np.load(PINS) as z:
        return {k: z[k] for k in z.files}
