"""The inputs of the CLEAN pins (tests/golden/clean_pins.npz): what make_clean_pins.py feeds the reference and what the CPU and
GPU tests feed the yardstick and the device.  Both sides must hold the same bits, so everything is integer arithmetic over
powers of two: tent-shaped PSFs floored to multiples of 2^-10 on a 2^-6 pedestal (nonzero up to the PSF's edge, so clipping
decides values) with an off-centre lobe (so reflection shows), sources as shifted PSF crops times dyadic fluxes, "noise" from
an integer hash of the pixel index.  No exp, no random generator, no FFT; psfhat is rfft2(ifftshift(psf)) by numpy where needed.

``case(name)`` returns dict(kind, cls, dirty, psf, wsums, mask, kw[, path]); class "E" cases are compared bit for bit, class
"T" cases (Clark with several major cycles, an FFT inside the loop) at the tolerance ``t_bound``, the one class "F" case
(float32 inputs) at ``f_bound``.  The paths of csrc/clean.hip each case is there to reach are in DESIGN.md section 8.
"""

import functools

import numpy as np

NX, NY = 97, 81          # 7857 pixels: 30 workgroups of 256 and a ragged 31st
BX, BY = 515, 511        # 263 165 pixels > 1024 * 256: the grid-stride second trip; chunk = 257 in the compaction
TRIP = 1024 * 256
C3_CHUNK = 257        # ceil(BX * BY / 1024): the pixels one workgroup of k_cl_count / k_cl_compact owns
PERM = 1009              # prime, coprime to every image size here: t -> t * PERM mod npix is a bijection
W3 = (0.25, 0.25, 0.5)
T_FLOOR = 64 * np.finfo(np.float64).eps


def hashed(idx, salt):
    """integers in [-32768, 32768) from an integer hash of ``idx``"""
    m = np.uint64(0xFFFFFFFF)
    h = (np.asarray(idx).astype(np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B1)) & m
    h = (h * np.uint64(2654435761)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m
    h ^= h >> np.uint64(13)
    return (h & np.uint64(0xFFFF)).astype(np.int64) - 32768


def noise(nband, nx, ny, salt, log2den):
    """hashed / 2^log2den per band (amplitude 2^(15 - log2den))"""
    t = np.arange(nx * ny).reshape(nx, ny)
    return np.stack([hashed(t, salt + 7 * b) for b in range(nband)]) / float(2 ** log2den)


def _tent(n, c, w):
    return np.maximum(0, w - np.abs(np.arange(n) - c))


@functools.lru_cache(maxsize=None)
def tent_psf(nband, nxp, nyp, lobe=True, scale=None, skirt=None):
    """Band b: floor(1024 tent_x tent_y) / 1024 with half-widths (5 + b, 4 + b), plus a lobe of 3/8 at (+7, -5) from the
    centre, plus 2^-6 everywhere; times ``scale[b]`` (Clark: the band's wsum).  ``skirt = (wx, wy)`` moves a quarter of the
    core into a pyramid 1 - max(|x| / wx, |y| / wy) of that half-width."""
    out = np.empty((nband, nxp, nyp))
    cx, cy = nxp // 2, nyp // 2
    for b in range(nband):
        wx, wy = 5 + b % 8, 4 + b % 8
        core = (1024 * _tent(nxp, cx, wx)[:, None] * _tent(nyp, cy, wy)[None, :]) // (wx * wy)
        if skirt is not None:
            sx, sy = skirt
            pyr = np.minimum(_tent(nxp, cx, sx)[:, None] * sy, _tent(nyp, cy, sy)[None, :] * sx)
            core = (3 * core) // 4 + (256 * pyr) // (sx * sy)
        if lobe:
            core = core + (384 * _tent(nxp, cx + 7, 3)[:, None] * _tent(nyp, cy - 5, 3)[None, :]) // 9
        out[b] = (core + 16) / 1024.0
        if scale is not None:
            out[b] *= scale[b]
    out.setflags(write=False)
    return out


def psfhat(psf):
    return np.fft.rfft2(np.fft.ifftshift(psf, axes=(1, 2)), axes=(1, 2))


def shifted(psf, i, j, nx, ny):
    """The PSF centred on image pixel (i, j), cropped to the image; zero where the PSF does not reach."""
    nband, nxp, nyp = psf.shape
    i0, j0 = nxp // 2 - i, nyp // 2 - j
    ia, ib = max(0, -i0), min(nx, nxp - i0)
    ja, jb = max(0, -j0), min(ny, nyp - j0)
    out = np.zeros((nband, nx, ny))
    out[:, ia:ib, ja:jb] = psf[:, i0 + ia:i0 + ib, j0 + ja:j0 + jb]
    return out


def sky(psf, nx, ny, sources, band_flux, salt, log2den=20):
    """sum of flux * band_flux[b] * shifted PSF, plus hash noise"""
    d = noise(psf.shape[0], nx, ny, salt, log2den)
    for i, j, f in sources:
        d += f * np.asarray(band_flux)[:, None, None] * shifted(psf, i, j, nx, ny)
    return d


def corner_sources(nx, ny):
    return [(0, 0, 4.0), (nx - 1, ny - 1, 3.5), (nx // 2, ny - 1, 3.0), (nx - 1, 0, 2.5), (5, 3, -2.25)]


def plateau(nband, nx, ny, n_on, salt):
    """``n_on`` scattered pixels within 1/8 of 1, the others within 1/16 of 1/4, in every band; with subpf = 1/2 the first
    active set is exactly the ``n_on`` pixels.  Returns (cube, flat indices of the n_on pixels in row-major order)."""
    npix = nx * ny
    t = np.arange(npix)
    on = (t * PERM) % npix < n_on
    cube = np.stack([np.where(on, 1.0 + hashed(t, salt + 7 * b) / 2.0 ** 18, 0.25 + hashed(t, salt + 7 * b) / 2.0 ** 19)
                     for b in range(nband)]).reshape(nband, nx, ny)
    return cube, np.flatnonzero(on)


def _hogbom(dirty, psf, cls="E", **kw):
    base = dict(threshold=0.0, gamma=0.2, pf=0.05, maxit=300)
    base.update(kw)
    return dict(kind="hogbom", cls=cls, dirty=dirty, psf=psf, wsums=None, mask=None, kw=base)


def _clark(dirty, psf, wsums, mask=None, cls="E", path=None, **kw):
    base = dict(threshold=0.0, gamma=0.25, pf=0.05, maxit=1, subpf=0.5, submaxit=40)
    base.update(kw)
    mask = np.ones(dirty.shape[1:]) if mask is None else mask
    return dict(kind="clark", cls=cls, dirty=dirty, psf=psf, wsums=np.asarray(wsums, dtype=np.float64), mask=mask, kw=base,
                path=path)


def _ties(nband, nx, ny, psf, pairs, maxit, salt):
    """hash noise below 1/4 per band; the flat pixels ``pairs`` = ((t, value), ...) set in every band"""
    d = noise(nband, nx, ny, salt, 17)
    flat = d.reshape(nband, -1)
    for t, v in pairs:
        flat[:, t] = v
    return _hogbom(d, psf, gamma=0.5, pf=0.1, maxit=maxit)


def _plateau_case(nband, nx, ny, nxp, nyp, n_on, wsums, salt, path, ties=(), **kw):
    """Clark, maxit = 1.  ``ties`` = ((position in the active set, value), ...) overwrite plateau pixels in every band."""
    d, on = plateau(nband, nx, ny, n_on, salt)
    for pos, v in ties:
        d.reshape(nband, -1)[:, on[pos]] = v
    return _clark(d, tent_psf(nband, nxp, nyp, True, tuple(wsums)), wsums, path=path, **kw), on


def _blob(nx, ny, cx, cy, wx, wy):
    """an extended tent, floored to multiples of 2^-10"""
    return ((1024 * _tent(nx, cx, wx)[:, None] * _tent(ny, cy, wy)[None, :]) // (wx * wy)) / 1024.0


def _t_dirty(psf):
    src = corner_sources(NX, NY) + [(40, 33, 3.25), (41, 35, 1.5), (70, 12, 2.0), (80, 20, 5.0)]  # (80, 20) is masked out
    return sky(psf, NX, NY, src, (1.0, 0.75, 1.25), salt=31, log2den=21)


def _t_mask():
    mask = np.ones((NX, NY))
    mask[70:90, 5:30] = 0.0
    return mask


HOGBOM_CASES = ("H1", "H2_odd", "H2_big", "H3", "H4_wave_1", "H4_wave_2", "H4_sign_1", "H4_sign_2", "H4_group_1", "H4_group_2",
                "H4_trip_1", "H4_trip_2", "H5_nband1", "H5_threshold", "H5_maxit0")
CLARK_E_CASES = ("C1_4096", "C1_4097", "C2_192", "C2_193", "C3", "C4_6", "C4_5", "C4G_6", "C4G_5", "C5_adjacent", "C5_far_lds",
                 "C5_far_grid", "C5_masked_peak", "C5_half_mask", "C5_submaxit0")
CLARK_T_CASES = ("T1", "T2", "T3")
F32_CASES = ("H6",)
E_CASES = HOGBOM_CASES + CLARK_E_CASES
ALL_CASES = E_CASES + CLARK_T_CASES + F32_CASES


def case(name):
    head, _, tail = name.partition("_")
    if name in ("H1", "H2_odd", "H2_big"):  # every side of the subtraction window clipped; npix not a multiple of 256
        nxp, nyp = {"H1": (2 * NX, 2 * NY), "H2_odd": (2 * NX - 1, 2 * NY - 1), "H2_big": (2 * NX + 2, 2 * NY)}[name]
        psf = tent_psf(2, nxp, nyp)
        return _hogbom(sky(psf, NX, NY, corner_sources(NX, NY), (1.0, 0.75), salt=1), psf)
    if name == "H3":  # two equal peaks on the second grid-stride trip, smaller sources on the first
        psf = tent_psf(2, 2 * BX, 2 * BY)
        d = sky(psf, BX, BY, [(10, 10, 2.0), (200, 400, 1.5), (513, 200, 1.0), (514, 300, 1.0)], (1.0, 0.75), salt=2)
        d[:, 513, 5] = d[:, 514, 300] = 2.5  # flat 262148 and 262954, both >= TRIP
        assert 513 * BY + 5 >= TRIP
        return _hogbom(d, psf, maxit=30)
    if head == "H4":
        kind, maxit = tail.split("_")
        if kind == "trip":  # the same thread on two grid-stride trips
            return _ties(2, BX, BY, tent_psf(2, 2 * BX, 2 * BY), ((700, 1.0), (700 + TRIP, 1.0)), int(maxit), salt=3)
        pairs = {"wave": ((1000, 1.0), (1010, 1.0)),        # one 64-pixel run
                 "sign": ((3000, -1.0), (5000, 1.0)),       # (-v)^2 == v^2: the earlier pixel, whatever its sign
                 "group": ((2000, 1.0), (2256, 1.0))}[kind]  # the same thread of neighbouring workgroups
        return _ties(2, NX, NY, tent_psf(2, 2 * NX, 2 * NY), pairs, int(maxit), salt=4)
    if name == "H5_nband1":
        psf = tent_psf(1, 2 * NX, 2 * NY)
        return _hogbom(sky(psf, NX, NY, corner_sources(NX, NY), (1.0,), salt=5), psf)
    if name in ("H5_threshold", "H5_maxit0"):
        c = case("H1")
        c["kw"].update(dict(threshold=3.0) if name == "H5_threshold" else dict(maxit=0))  # 3.0 > pf * rmax_0 = 0.05 * 7.1
        return c
    if name == "H6":  # H1 in float32 (every input value is a float32 number), twenty iterations
        c = case("H1")
        c.update(cls="F", dirty=c["dirty"].astype(np.float32), psf=c["psf"].astype(np.float32))
        c["kw"]["maxit"] = 20
        return c
    if head == "C1":  # PSF smaller than twice the image: the in-range clip decides; lds_max = 98304 / 24 = 4096
        n_on = int(tail)
        return _plateau_case(3, NX, NY, 121, 101, n_on, W3, 11, "lds" if n_on <= 4096 else "grid")[0]
    if head == "C2":  # nband = CL_MAXB = 64: lds_max = 192
        n_on = int(tail)
        nxp, nyp = (48, 40) if n_on == 192 else (31, 27)
        return _plateau_case(64, 24, 20, nxp, nyp, n_on, (1.0 / 64,) * 64, 12, "lds" if n_on <= 192 else "grid", submaxit=12)[0]
    if name == "C3":
        # k_cl_active's second trip; k_cl_count / k_cl_compact with chunk 257: two loop trips, one pixel in the second, whose
        # slot is the running base plus the first trip's total.  The strongest pixel opens a chunk (t = 300 * 257) and the second
        # strongest closes one (t = 700 * 257 + 256): a compaction that forgets the first trip's total writes the closing pixel
        # over its chunk's opening one, so the opening pixel of every chunk -- the strongest among them -- is lost.
        c, on = _plateau_case(1, BX, BY, 2 * BX, 2 * BY, 262200, (1.0,), 13, "grid", submaxit=3)
        for t, v in ((300 * C3_CHUNK, 1.5), (700 * C3_CHUNK + C3_CHUNK - 1, 1.375)):
            assert t in on
            c["dirty"].reshape(1, -1)[:, t] = v
        return c
    if head == "C4G":
        # C4's spikes on a plateau of 6200 pixels, two bands: lds_max = 6144, so the same conventions decide in k_cl_active.
        c, on = _plateau_case(2, NX, NY, 2 * NX, 2 * NY, 6200, (0.5, 0.5), 17, "grid", gamma=0.25, pf=0.01, subpf=0.125,
                              submaxit=int(tail))
        for (i, j), v in (((40, 33), 4.0), ((47, 28), 2.125), ((33, 38), 2.0)):
            c["dirty"][:, i, j] = v * np.array([1.0, 0.75])
        return c
    if head == "C4":
        # An extended source under an asymmetric PSF, the sub-minor loop cut short at 6 and at 5.  Three spikes on it: the
        # strongest is taken three times running (so its own update, i == pq, decides the next step), the other two sit at
        # plus and minus the lobe's offset (7, -5) from it (so the direction the PSF is read in decides their values).
        psf = tent_psf(2, 2 * NX, 2 * NY, True, (0.5, 0.5))
        d = 0.5 * np.stack([_blob(NX, NY, 40, 33, 14, 11), 0.75 * _blob(NX, NY, 41, 32, 12, 13)]) + noise(2, NX, NY, 14, 22)
        for (i, j), v in (((40, 33), 2.0), ((47, 28), 1.0625), ((33, 38), 1.0)):
            d[:, i, j] = v * np.array([1.0, 0.75])
        return _clark(d, psf, (0.5, 0.5), gamma=0.25, pf=0.01, subpf=0.125, submaxit=int(tail), path="lds")
    if name == "C5_adjacent":  # equal neighbours in the active set
        return _plateau_case(3, NX, NY, 121, 101, 4096, W3, 15, "lds", ties=((2000, 1.25), (2001, 1.25)), submaxit=8)[0]
    if name == "C5_far_lds":   # 1024 apart: the same thread of the one-workgroup loop, two strides
        return _plateau_case(3, NX, NY, 121, 101, 4096, W3, 15, "lds", ties=((1500, 1.25), (2524, 1.25)), submaxit=8)[0]
    if name == "C5_far_grid":  # different workgroups of k_cl_active
        return _plateau_case(3, NX, NY, 121, 101, 4097, W3, 15, "grid", ties=((1500, 1.25), (3700, 1.25)), submaxit=8)[0]
    if name in ("C5_masked_peak", "C5_half_mask", "C5_submaxit0"):
        # position 3000 of the active set holds 1.5 per band, position 100 holds 1.25
        c, on = _plateau_case(3, NX, NY, 121, 101, 4000, W3, 16, "lds", ties=((3000, 1.5), (100, 1.25)), submaxit=8)
        p, q = divmod(int(on[3000]), NY)
        if name == "C5_masked_peak":   # the masked search decides p, q and the active set loses the global peak
            c["mask"][p, q] = 0.0
        elif name == "C5_half_mask":   # 1.5^2 / 2 < 1.25^2: position 100 sets rmax, position 3000 stays active and leads the sub-minor loop
            c["mask"][max(0, p - 2):p + 3, max(0, q - 2):q + 3] = 0.5
        else:
            c["kw"]["submaxit"] = 0
        return c
    if name in ("T1", "T2"):
        nxp, nyp = (2 * NX + 2, 2 * NY) if name == "T1" else (121, 101)
        psf = tent_psf(3, nxp, nyp, True, W3)
        return _clark(_t_dirty(psf), psf, W3, _t_mask(), cls="T", gamma=0.25, pf=0.05, maxit=8, subpf=0.5, submaxit=60)
    if name == "T3":
        # A plateau at 0.55 under 40 spikes near 1, eight cleaned per major cycle: rmax stays near 1 while the PSF's broad skirt
        # sinks the plateau, so the active sets are 7857, 4197 (k_cl_active), then 1248, 693, 536, 722 (k_cl_sub_lds).
        psf = tent_psf(3, 2 * NX + 2, 2 * NY, False, W3, skirt=(40, 34))
        d = np.asarray(W3)[:, None, None] * (0.55 + noise(3, NX, NY, 33, 22))
        for n in range(40):
            d.reshape(3, -1)[:, (n * 1237 + 400) % (NX * NY)] = np.asarray(W3) * (1.0 - n / 256.0)
        return _clark(d, psf, W3, cls="T", gamma=0.25, pf=0.05, maxit=6, subpf=0.5, submaxit=8)
    raise KeyError(name)


def perturbed(dirty):
    """dirty * (1 + 1e-9 h), h the integer hash in [-1, 1): the condition a class T case must pass unchanged"""
    nband, nx, ny = dirty.shape
    return dirty * (1.0 + 1e-9 * noise(nband, nx, ny, 99, 15))


def sparse(model):
    idx = np.flatnonzero(model)
    return idx.astype(np.int64), model.reshape(-1)[idx]


def dense(idx, val, shape, dtype=np.float64):
    out = np.zeros(int(np.prod(shape)), dtype=dtype)
    out[idx] = val
    return out.reshape(shape)


def t_bound(disagreement):
    """class T: ten times the reference's own numpy-FFT / scipy-FFT disagreement, not below 64 eps"""
    return max(10.0 * float(disagreement), T_FLOOR)


def f_bound(disagreement):
    """class F: ten times the reference's own float32-run / float64-run disagreement on the same numbers (the factor of class T)"""
    return 10.0 * float(disagreement)


def rel_max(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())
