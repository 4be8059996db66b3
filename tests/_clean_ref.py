"""Plain-numpy statement of Hogbom and Clark CLEAN: the yardstick the device loops are tested against.

It follows DESIGN.md "Device-resident CLEAN" step for step, in float64 and in the same order of operations as clean.hip:
the search image is (sum_b r_b)^2 with the bands added in order, the peak is the first maximum in row-major order,
rmax = sqrt(search[peak]) and the loop runs while rmax > tol and k < maxit.  Clark's sub-minor loop reads the PSF reflected
and, with ``copy_xhat=False`` (the default, as pfb-imaging does), reduces active pixels after the peak with the peak's value
after its own update.  The major cycle convolves with numpy.fft in the psf_convolve_cube convention (pad at [0:nx, 0:ny],
rfft2, multiply, irfft2 to (nx_psf, ny_psf), crop).
"""

import numpy as np


def search_image(cube):
    s = cube[0].copy()
    for b in range(1, cube.shape[0]):
        s = s + cube[b]
    return s * s


def peak(search):
    """(flat index, rmax) of the first maximum."""
    pq = int(np.argmax(search))
    return pq, np.sqrt(search.reshape(-1)[pq])


def hogbom(dirty, psf, threshold=0.0, gamma=0.1, pf=0.1, maxit=10000):
    """Returns (model, residual, k, status)."""
    nband, nx, ny = dirty.shape
    _, nxp, nyp = psf.shape
    nx0, ny0 = nxp // 2, nyp // 2
    wsums = psf.reshape(nband, -1).max(axis=1)
    model = np.zeros_like(dirty, dtype=np.float64)
    r = np.array(dirty, dtype=np.float64)
    pq, rmax = peak(search_image(r))
    p, q = divmod(pq, ny)
    tol = max(pf * rmax, threshold)
    k = 0
    while rmax > tol and k < maxit:
        g = gamma * (r[:, p, q] / wsums)
        model[:, p, q] += g
        i0, j0 = nx0 - p, ny0 - q  # PSF row / column of image pixel (0, 0); outside the PSF counts as 0
        ia, ib = max(0, -i0), min(nx, nxp - i0)
        ja, jb = max(0, -j0), min(ny, nyp - j0)
        if ia < ib and ja < jb:
            r[:, ia:ib, ja:jb] = r[:, ia:ib, ja:jb] - g[:, None, None] * psf[:, i0 + ia:i0 + ib, j0 + ja:j0 + jb]
        pq, rmax = peak(search_image(r))
        p, q = divmod(pq, ny)
        k += 1
    return model, r, k, int(k >= maxit)


def psf_convolve_cube(x, psfhat, ny_psf):
    nband, nx, ny = x.shape
    nx_psf = psfhat.shape[1]
    xpad = np.zeros((nband, nx_psf, ny_psf))
    xpad[:, :nx, :ny] = x
    out = np.fft.irfft2(np.fft.rfft2(xpad, axes=(1, 2)) * psfhat, s=(nx_psf, ny_psf), axes=(1, 2))
    return out[:, :nx, :ny]


def subminor(a, psf, pidx, qidx, model, wsums, gamma, th, maxit, copy_xhat=False):
    """Runs in place on the active set ``a`` (nband, A) and ``model``; returns the iteration count."""
    nband, nxp, nyp = psf.shape
    nxo2, nyo2 = nxp // 2, nyp // 2
    bands = [b for b in range(nband) if wsums[b] != 0]
    idx = np.arange(pidx.size)
    pq, amax = peak(search_image(a))
    p, q = pidx[pq], qidx[pq]
    k = 0
    while amax > th and k < maxit:
        pp = nxo2 - (pidx - p)
        qq = nyo2 - (qidx - q)
        inb = (pp >= 0) & (pp < nxp) & (qq >= 0) & (qq < nyp)
        after = idx[inb] > pq
        for b in bands:
            xb = a[b, pq]
            g = gamma * xb
            model[b, p, q] += g / wsums[b]
            if copy_xhat:
                gi = g
            else:
                g2 = gamma * (xb - (g * psf[b, nxo2, nyo2]) / wsums[b])
                gi = np.where(after, g2, g)
            a[b, inb] = a[b, inb] - (gi * psf[b, pp[inb], qq[inb]]) / wsums[b]
        pq, amax = peak(search_image(a))
        p, q = pidx[pq], qidx[pq]
        k += 1
    return k


def clark(dirty, psf, psfhat, wsums, mask, threshold=0.0, gamma=0.05, pf=0.05, maxit=50, subpf=0.5, submaxit=1000,
          copy_xhat=False):
    """Returns (model, residual, k, status, minor_iters)."""
    nband, nx, ny = dirty.shape
    ny_psf = psf.shape[2]
    dirty = np.asarray(dirty, dtype=np.float64)
    model = np.zeros_like(dirty)
    residual = dirty.copy()
    search = search_image(residual) * mask
    pq, rmax = peak(search)
    tol = max(pf * rmax, threshold)
    k = nminor = 0
    while rmax > tol and k < maxit:
        subth = subpf * rmax
        pidx, qidx = np.where(search > subth * subth)
        a = residual[:, pidx, qidx]
        nminor += subminor(a, psf, pidx, qidx, model, wsums, gamma, subth, submaxit, copy_xhat)
        residual = dirty - psf_convolve_cube(model, psfhat, ny_psf)
        search = search_image(residual) * mask
        pq, rmax = peak(search)
        k += 1
    return model, residual, k, int(k >= maxit), nminor
