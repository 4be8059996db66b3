"""Every shape of the hand-written row FFT (csrc/rowfft.hpp: RF_FOR_SHAPES, RF_FOR_SHAPES2) in every family and kernel form
it is instantiated in.

Part 1 -- the plain kernel on both shape families (pfbhip_debug_rowfft_shape: family 0 = RfShape<L, K>, family 1 =
RfShape<L, K, false>, what the fused second-axis kernels are built on) against numpy.fft in complex128: noise rows, a unit
impulse at N - 1 and one at N / 2 + 1 (every twiddle and every output position counts, nothing averages out) and a constant
row.  Bound: the project's 5e-15 relative L2 (test_handwritten_row_fft_matches_numpy), per batch and per structured row; element-
wise 8e-15 of the row's largest output -- an output of an impulse row is a product of unit-modulus factors: per pass the table
twiddle (rounded, u = 1.1e-16), up to 15 successive complex multiplications for its powers and one with the data, at most five
passes.  If every error lined up that would be 5 * (16 * sqrt(5) u + u) = 2.1e-14; the roundings are independent, each of rms
<= u, so an output's error has rms <= sqrt(85) u = 1.0e-15, and six of those -- a Gaussian tail of 2e-9 per value, 3e-4 over
the 1.3e5 outputs of the impulse rows of the longest length -- is 6.1e-15; numpy's own error, O(log2 N) u, takes it to 8e-15.

Parts 2 and 3 -- plans whose fused second axis (fft_mode & 2) or transposing first axis (fft_mode & 8) has the length under
test.  A plan works on the transposed problem and reports its grid in the caller's orientation (pfbhip_gridder_get_info): the
second axis -- the rows of the cropped plane B, the axis of the fused kernels and of the occupancy blocks -- runs along the
caller's y, its length is info["nv"]; the first axis is info["nu"].  Images of the second-axis legs are therefore (other, n_y)
with info["nv"] == N, those of part 3 (n_x, other) with info["nu"] == N.  The forms launch_crop / launch_pad (csrc/rowfft.hip)
distinguish:
  a  polynomial planes (wmode 1), 5 of them: a four-plane launch of k_fused_fft_crop<S, true> / k_fused_pad_fft<S, true> with the
     LDS image row and a trailing one-plane launch (read-modify-write crop; persistent pad kernel on the raw image), the other
     axis 1024 points and transposing (tpitch > 0).  Proof: wmode == 1, nplanes == 5, screen_composite >= 1 (== 2 at
     epsilon = 1e-9, where the one-plane launch has a composite screen too), fft_mode & 8.
  b  ES-kernel planes (wmode 0, > 4 planes: the plane buffer is cleared and reused per pass), separable screens
     (screen_separable > 0) or, for one shape per lead family, the general path (both screen counters 0): <S, false>.
  c  one-plane launches on the raw image, the persistent k_fused_pad_fft_p<S, SC, BEAM>: do_wgridding=False (SC = false;
     nplanes == 1, no screens) and the one-plane scheme (SC = true; wmode == 2, screen_composite == 1), Hessian with a beam
     and without one.
  d  leg a under PFBHIP_FUSED_LDSROW=0: read-modify-write crop and prepared-image pad, what grids too large for the LDS row take
     by themselves.
The LDS-row forms of leg a and the persistent kernels of leg c exist only where the image row fits next to the exchange buffer
(lds_row_fits, asserted per case).  12288 and 14336 points get there on a wider grid (sigma = 1.8, 2.5); 15360 and 16384
points cannot at any tabulated sigma (NO_LDS_ROW): their legs a and c run the read-modify-write / prepared-image forms.
  3  leg a transposed: k_rowfft_a2b / k_rowfft_b2a<RfShape<L, K>> at every length, and 20480 points in both orientations.
References, every case: the same plan on the unfused path (PFBHIP_FUSED_FFT=0, PFBHIP_ROWFFT=0: rocFFT and the separate pad /
crop kernels) to the plan's rounding budget (tests/test_gpu_wide_field._hessian_tol); the direct DFT at sampled pixels and
visibilities to the plan's epsilon; for the smallest shape of each lead family the CPU restatement to 2e-9.
"""

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dft  # noqa: E402
from oracle import wgridder as owg  # noqa: E402

# RF_FOR_SHAPES / RF_FOR_SHAPES2 (csrc/rowfft.hpp): (LEAD, K); N = LEAD * 2^K, doubled: 2 * LEAD * 2^K
# (tests/test_rowfft_shapes_cpu.py holds these tables to the header)
RF_SHAPES = [(1, 10), (1, 11), (1, 12), (1, 13), (1, 14), (3, 9), (3, 10), (3, 11), (3, 12), (5, 8), (5, 9), (5, 10), (5, 11),
             (7, 8), (7, 9), (7, 10), (7, 11), (9, 7), (9, 8), (9, 9), (9, 10), (15, 7), (15, 8), (15, 9), (15, 10)]
RF_DOUBLED = [(5, 11), (3, 12), (1, 14)]
PLAIN_NS = sorted(lead << k for lead, k in RF_SHAPES)
DOUBLED_NS = sorted(2 * (lead << k) for lead, k in RF_DOUBLED)
# smallest shape of each lead family
LEAD_SMALLEST = {lead: min(l << k for l, k in RF_SHAPES if l == lead) for lead in (1, 3, 5, 7, 9, 15)}
SMALLEST_NS = sorted(LEAD_SMALLEST.values())  # 1024, 1152, 1280, 1536, 1792, 1920

# Oversampling of the forced kernel-table row: 1.5, except where the image that lands on the length at 1.5 leaves no LDS room
# for the image row of the fused kernels (fused_row_fits, csrc/rowfft.hip: (NL + n_pix) * 8 <= 160 KiB) while a tabulated
# wider grid does: 12288 points at 1.8 (n_pix <= 7680), 14336 at 2.5 (n_pix <= 5888).
SIGMA = 1.5
SIGMA_OF = {12288: 1.8, 14336: 2.5}
# Unreachable in principle: 15360 points have room for n_pix <= 4992 and 16384 for n_pix <= 3072, i.e. sigma >= 3.08 and 5.33,
# past the kernel table (sigma <= 2.5).  There the fused kernels always take the read-modify-write crop and the prepared-image
# pad: legs a and d coincide, and leg c runs k_fused_pad_fft on a prepared image, not the persistent k_fused_pad_fft_p.
NO_LDS_ROW = (15360, 16384)
# Image size along the axis under test: the largest even n_pix <= N / sigma that is no multiple of 64 and for which both of the
# plan's grid candidates (2 * smooth(ceil(sigma n_pix / 2)) and the smallest row-FFT length >= sigma n_pix) are N.
FUSED_NX = {1024: 682, 1152: 766, 1280: 852, 1536: 1022, 1792: 1194, 1920: 1278, 2048: 1364, 2304: 1534, 2560: 1706,
            3072: 2046, 3584: 2388, 3840: 2558, 4096: 2730, 4608: 3070, 5120: 3412, 6144: 4094, 7168: 4778, 7680: 5118,
            8192: 5460, 9216: 6142, 10240: 6826, 12288: 6826, 14336: 5734, 15360: 10238, 16384: 10922}
NY_1024 = {1.5: 680, 1.8: 568, 2.5: 408}  # other axis of leg a / part 3: grid 1024 (a row-FFT length: transposing first axis)
NY_THIN = 48    # other axis of legs b - d: grid 72 (90, 120 at sigma = 1.8, 2.5), rocFFT first axis
NX_20480 = 13652  # 20480 points at sigma = 1.5


def sigma_of(n):
    return SIGMA_OF.get(n, SIGMA)


def grid_size(npix, sigma):
    """csrc/eskernel.cpp: grid_size -- twice the smallest 2-3-5-7-smooth number >= sigma npix / 2"""
    n = math.ceil(0.5 * sigma * npix - 1e-9)
    while True:
        m = n
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        if m == 1:
            return max(2 * n, 32)
        n += 1


def lds_row_fits(n, npix):
    """fused_row_fits(RfShape<L, K, false>::LDS_BYTES, npix) of csrc/rowfft.hip restated: the exchange buffer holds one
    component, NL doubles (csrc/rowfft.hpp: N, plus RF_XPAD = 2 per 16 LEAD positions for LEAD > 1 and K >= 8, plus N / 16 for
    powers of two from 4096 on), and the image row npix more; 160 KiB of LDS."""
    lead, k = next((l, kk) for l, kk in RF_SHAPES if l << kk == n)
    nl = n + ((2 * (n // (16 * lead)) if k >= 8 else 0) if lead > 1 else (n // 16 if n >= 4096 else 0))
    return (nl + npix) * 8 <= 160 * 1024

BOUND_L2 = 5e-15
BOUND_ELEM = 8e-15


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# part 1: the plain kernel on both shape families
# ---------------------------------------------------------------------------------------------------------------------

_ROWS = {}


def _rows(n):
    """(input, forward reference, inverse reference) of length n: 5 noise rows, impulses at n - 1 and n / 2 + 1, a constant row.
    One entry is kept (the cases of a length run back to back)."""
    if n not in _ROWS:
        _ROWS.clear()
        rng = np.random.default_rng(n)
        a = np.zeros((8, n), dtype=np.complex128)
        a[:5] = rng.standard_normal((5, n)) + 1j * rng.standard_normal((5, n))
        a[5, n - 1] = 1.0
        a[6, n // 2 + 1] = 1.0
        a[7] = 0.75 - 0.5j
        a.setflags(write=False)
        _ROWS[n] = (a, np.fft.fft(a, axis=1), np.fft.ifft(a, axis=1) * n)
    return _ROWS[n]


def _transform(a, inverse, family):
    import ctypes as ct

    from pfb_imaging_amd._lib import check, cint, i64, lib, ptr

    b = np.array(a, dtype=np.complex128, order="C")
    ms = ct.c_double(0.0)
    check(lib().pfbhip_debug_rowfft_shape(ptr(b), i64(b.shape[1]), i64(b.shape[0]), cint(inverse), cint(family), ct.byref(ms)))
    return b


@pytest.mark.parametrize("family", [0, 1])
@pytest.mark.parametrize("n", PLAIN_NS + DOUBLED_NS)
def test_plain_kernel_both_families_vs_numpy(n, family):
    a, fwd, inv = _rows(n)
    for inverse, ref in ((0, fwd), (1, inv)):
        b = _transform(a, inverse, family)
        l2 = rel(b[:5], ref[:5])
        rows = [rel(b[r], ref[r]) for r in (5, 6, 7)]
        elem = [np.abs(b[r] - ref[r]).max() / np.abs(ref[r]).max() for r in (5, 6, 7)]
        print(f"ROWFFT_SHAPE n={n} family={family} inverse={inverse} noise_l2={l2:.3e} row_l2={max(rows):.3e} "
              f"elem={max(elem):.3e}")
        assert l2 < BOUND_L2, (n, family, inverse, l2)
        assert max(rows) < BOUND_L2, (n, family, inverse, rows)
        assert max(elem) < BOUND_ELEM, (n, family, inverse, elem)


@pytest.mark.parametrize("family", [0, 1])
@pytest.mark.parametrize("n", SMALLEST_NS)
def test_plain_kernel_single_row(n, family):
    """One workgroup alone: nothing may depend on a neighbouring row."""
    a, fwd, inv = _rows(n)
    for inverse, ref in ((0, fwd), (1, inv)):
        for r in (0, 5):
            b = _transform(a[r:r + 1], inverse, family)
            assert rel(b[0], ref[r]) < BOUND_L2, (n, family, inverse, r)
            assert np.abs(b[0] - ref[r]).max() < BOUND_ELEM * np.abs(ref[r]).max(), (n, family, inverse, r)


def test_plain_kernel_rejects_bad_length_and_family():
    bad = np.zeros((1, 1000), dtype=np.complex128)
    for family in (0, 1):
        with pytest.raises(ValueError):
            _transform(bad, 0, family)
        with pytest.raises(ValueError):
            _transform(np.zeros((1, 18432), dtype=np.complex128), 0, family)  # 9 * 2^11: not in the list
    ok = np.ones((1, 1024), dtype=np.complex128)
    for family in (2, -1):
        with pytest.raises(ValueError):
            _transform(ok, 0, family)
    assert rel(_transform(ok, 0, 1)[0], np.fft.fft(ok[0])) < BOUND_L2  # (the library is usable after the refusals)


# ---------------------------------------------------------------------------------------------------------------------
# parts 2 and 3: plans whose fused second axis / transposing first axis has the length under test
# ---------------------------------------------------------------------------------------------------------------------

FREQ = np.array([1.0e9])
LAM = 299792458.0 / FREQ[0]
NROW = 1500


def _poly_planes_needed(omega, eps):
    """csrc/gridder.hip: poly_planes_needed (planes of the polynomial w-scheme for the phase range omega)."""
    bound, k = omega, 1
    while bound > eps:
        k += 1
        bound *= omega / (2.0 * k)
    return k


def _tmax(nx, ny, px, py):
    """The plan's tmax of an on-axis image: n - 1 runs from its value at the corner to 0 and is shifted to the middle of that
    range (nshift), so the largest |n - 1 + nshift| is half the corner's 1 - n."""
    r2 = (nx // 2 * px) ** 2 + (ny // 2 * py) ** 2
    return 0.5 * r2 / (1.0 + math.sqrt(1.0 - r2))


def _fmt(info):
    keys = ("nu", "nv", "nx", "ny", "W", "sigma", "wmode", "nplanes", "nderiv", "fft_mode", "occ_rows", "screen_poly",
            "screen_composite", "screen_separable", "dw", "whalf", "wcenter")
    return " ".join(f"{k}={info[k]}" for k in keys)


def _case(nx, ny, nu, nv, half_field, w_centre, w_half, seed, sigma=SIGMA):
    """Core-and-ring uv coverage (tests/test_gpu_fuzz.py: test_uv_coverages_with_holes_and_wraps) scaled to the grid: a core
    below 8 % and a ring at 70 - 75 % of the grid's half-width, which leaves the 32-column blocks between the ring and the edge
    empty, and 40 samples per axis within four cells of the wrap-around edge, whose footprints wrap.  The ring's samples are
    stratified along the long axis (at most two strata, 41 cells at 20480 points, between neighbours: no tile row inside the
    ring is left out, so the plan keeps its occupancy -- with more than four runs of blocks it would transform every row; for
    the same reason no ring sample is flagged and w >= 0, since the plan mirrors a sample with w < 0 through the origin).
    w (wavelengths) fills [w_centre - w_half, w_centre + w_half] >= 0 with both ends present (the plan folds w < 0 onto w > 0).
    Dense Gaussian image, 3 % of the samples flagged."""
    rng = np.random.default_rng(seed)
    px = py = half_field / (max(nx, ny) // 2)
    ang = rng.random(NROW) * 2 * np.pi
    rad = rng.random(NROW) * 0.08
    fu, fv = 0.5 * rad * np.cos(ang), 0.5 * rad * np.sin(ang)  # cycles per pixel, |f| < 0.5
    nring = NROW // 2
    r = 0.5 * (0.70 + 0.05 * rng.random(nring))
    along = 0.375 * (2.0 * (rng.permutation(nring) + rng.random(nring)) / nring - 1.0)
    across = np.where(rng.random(nring) < 0.5, -1.0, 1.0) * np.sqrt(np.maximum(r * r - along * along, 0.0))
    fu[nring:2 * nring], fv[nring:2 * nring] = (along, across) if nu > nv else (across, along)
    sgn = np.where(rng.random(80) < 0.5, -1.0, 1.0)
    fu[:40] = sgn[:40] * (0.5 - (1.0 + 3.0 * rng.random(40)) / nu)
    fv[40:80] = sgn[40:] * (0.5 - (1.0 + 3.0 * rng.random(40)) / nv)
    w = w_centre + w_half * (2.0 * rng.random(NROW) - 1.0)
    w[80], w[81] = w_centre - w_half, w_centre + w_half
    uvw = np.stack([fu / px, fv / py, w], axis=1) * LAM
    mask = (rng.random((NROW, 1)) > 0.06).astype(np.uint8)  # (flags in the core only: a flagged ring sample would open a gap)
    mask[:82] = 1
    mask[nring:] = 1
    c = dict(uvw=uvw, freq=FREQ, mask=mask, nx=nx, ny=ny, px=px, py=py, sigma=sigma,
             vis=rng.standard_normal((NROW, 1)) + 1j * rng.standard_normal((NROW, 1)), wgt=rng.random((NROW, 1)) + 0.5,
             x=rng.standard_normal((nx, ny)), beam=0.5 + rng.random((nx, ny)))
    # sampled references' positions: 30 random pixels, the four corners, the two pixels either side of n / 2 on each axis
    c["ix"] = np.concatenate([rng.integers(0, nx, 30), [0, 0, nx - 1, nx - 1], [nx // 2 - 1, nx // 2], rng.integers(0, nx, 2)])
    c["iy"] = np.concatenate([rng.integers(0, ny, 30), [0, ny - 1, 0, ny - 1], rng.integers(0, ny, 2), [ny // 2 - 1, ny // 2]])
    good = np.flatnonzero(mask[:, 0])
    c["rows"] = np.concatenate([[0, 45, 80, 81], rng.choice(good[good > 81], 12, replace=False)])
    return c


_DFT = {}


def _dft_refs(key, c, do_w):
    """(dirty at the sampled pixels, visibilities at the sampled rows) by the direct DFT; one entry is kept."""
    if key not in _DFT:
        _DFT.clear()
        args = (c["px"], c["py"], 0.0, 0.0, False, True, False, do_w, False)
        refd = dft.dft_vis2dirty(c["uvw"], FREQ, c["vis"], c["wgt"], c["mask"], c["nx"], c["ny"], *args, pixels=(c["ix"], c["iy"]))
        refv = dft.dft_dirty2vis(c["uvw"], FREQ, c["x"], *args, rows=c["rows"], chans=np.zeros_like(c["rows"]))
        _DFT[key] = (refd, refv)
    return _DFT[key]


def _products(g, c, beams):
    """vis2dirty, dirty2vis, the Hessian with every beam of `beams` (non-trivial eta and wsum), and x then 2x on the one handle
    (tests/test_gpu_gridder._hessian_twice: a plane region left uncleared by the first apply shows in the second)."""
    from tests.test_gpu_gridder import _hessian_twice

    d, v = g.vis2dirty(c["vis"], c["wgt"]), g.dirty2vis(c["x"])
    g.set_weights(c["wgt"])
    hs = [g.hessian(c["x"], beam=c["beam"] if b else None, eta=0.3, wsum=7.0) for b in beams]
    _hessian_twice(g, c)
    return [d, v] + hs


_UNFUSED = {}


def _run(monkeypatch, key, c, n, axis, expect, *, eps=1e-7, W=13, force_wmode=None, do_w=True, ldsrow=None, beams=(True,),
         restate=False, leg=""):
    """One case: the plan on the fused path (its info checked by `expect`), the same plan on the unfused path, the DFT."""
    from pfb_imaging_amd.wgridder import Gridder
    from tests.test_gpu_wide_field import _hessian_tol

    kw = dict(npix_x=c["nx"], npix_y=c["ny"], pixsize_x=c["px"], pixsize_y=c["py"], center_x=0.0, center_y=0.0, epsilon=eps,
              flip_u=False, flip_v=True, flip_w=False, do_wgridding=do_w, divide_by_n=False, force=(c["sigma"], W),
              force_wmode=force_wmode)
    for name in ("PFBHIP_FUSED_FFT", "PFBHIP_ROWFFT", "PFBHIP_TFFT", "PFBHIP_FUSED_LDSROW", "PFBHIP_FUSED_DOUBLED",
                 "PFBHIP_SEPSCREEN", "PFBHIP_WMODE2"):
        monkeypatch.delenv(name, raising=False)
    if ldsrow is not None:
        monkeypatch.setenv("PFBHIP_FUSED_LDSROW", ldsrow)
    g = Gridder(c["uvw"], FREQ, c["mask"], **kw)
    try:
        info = dict(g.info, nx=c["nx"], ny=c["ny"])
        # the shape under test is on the path under test, on some blocks only, wrap-around edge included (by construction)
        assert info["W"] == W and info["sigma"] == c["sigma"], _fmt(info)
        assert info["nv" if axis == "second" else "nu"] == n, _fmt(info)
        assert info["fft_mode"] & 2, _fmt(info)
        if axis == "second" and n in FUSED_NX:
            # launch_crop / launch_pad take the LDS image row (several planes) and the persistent pad kernel (one plane on the raw
            # image) exactly where the row fits -- unless PFBHIP_FUSED_LDSROW=0 (leg d) -- and that is everywhere but NO_LDS_ROW
            assert lds_row_fits(n, c["ny"]) == (n not in NO_LDS_ROW), (n, c["ny"], _fmt(info))
        assert 0 < info["occ_rows"] < info["nv"], _fmt(info)  # occupied 32-column blocks of B, in rows of the plane
        for col, pix, size in ((0, "px", "nu"), (1, "py", "nv")):
            f = np.abs(c["uvw"][:, col] / LAM * c[pix]).max()
            assert f * info[size] + 0.5 * W > 0.5 * info[size], f"no footprint wraps around the edge of {size}"
        expect(info)
        tol = _hessian_tol(info)
        fused = _products(g, c, beams)
        if restate:
            o = owg.Plan(c["uvw"], FREQ, c["mask"], c["nx"], c["ny"], c["px"], c["py"], 0.0, 0.0, eps, False, True, False, do_w,
                         False, params=g.oracle_params())
            r_d, r_v = rel(fused[0], o.vis2dirty(c["vis"], c["wgt"])), rel(fused[1], o.dirty2vis(c["x"]))
            print(f"ROWFFT_LEG leg={leg} n={n} restatement d={r_d:.3e} v={r_v:.3e}")
            assert r_d < 2e-9 and r_v < 2e-9, (info, r_d, r_v)
    finally:
        g.close()
    if key not in _UNFUSED:  # (legs a and d of a length run back to back and share it)
        _UNFUSED.clear()
        monkeypatch.setenv("PFBHIP_FUSED_FFT", "0")
        monkeypatch.setenv("PFBHIP_ROWFFT", "0")
        g0 = Gridder(c["uvw"], FREQ, c["mask"], **kw)
        try:
            i0 = g0.info
            assert i0["fft_mode"] == 0, i0
            assert all(i0[k] == info[k] for k in ("nu", "nv", "W", "sigma", "wmode", "nplanes", "nderiv")), (i0, info)
            _UNFUSED[key] = (beams, _products(g0, c, beams))
        finally:
            g0.close()
        monkeypatch.delenv("PFBHIP_FUSED_FFT")
        monkeypatch.delenv("PFBHIP_ROWFFT")
    ubeams, unfused = _UNFUSED[key]
    assert ubeams == beams
    ratios = [rel(a, b) / tol for a, b in zip(fused, unfused)]
    refd, refv = _dft_refs(key, c, do_w)
    dd = [rel(r[0][c["ix"], c["iy"]], refd) / eps for r in (fused, unfused)]
    dv = [rel(r[1][c["rows"], 0], refv) / eps for r in (fused, unfused)]
    print(f"ROWFFT_LEG leg={leg} n={n} wmode={info['wmode']} planes={info['nplanes']} vs_unfused/tol={max(ratios):.3e} "
          f"dft_dirty/eps={max(dd):.3e} dft_vis/eps={max(dv):.3e}")
    assert max(ratios) < 1.0, (info, tol, ratios)
    assert max(dd) < 1.0 and max(dv) < 1.0, (info, dd, dv)


def _w_for_planes(c_geom, planes, eps):
    """w half-range (wavelengths) at which the polynomial w-scheme needs `planes` planes: the phase range omega =
    2 pi w_half tmax 5 % above the lower end of the interval of that plane count.  Small phases: the composite screen
    polynomials, at most 8 coefficients to 1e-14, take about 0.12 rad, and with w in [0, 2 w_half] the highest plane of five at
    epsilon = 1e-7 has 0.123 rad or more -- the first four planes get composite screens, the fifth may not."""
    budget = 2.0 * eps / 3.0
    lo = hi = None
    for om in np.geomspace(1e-4, 10.0, 4000):
        k = _poly_planes_needed(om, budget)
        if k == planes:
            lo = om if lo is None else lo
            hi = om
    assert 1.05 * lo < hi
    return 1.05 * lo / (2.0 * math.pi * c_geom)


def _leg_a_case(n, eps, axis="second"):
    """(680, n_y) pixels for the second axis, (n_x, 680) for the first (680: the size that lands on 1024 points at the length's
    sigma)"""
    sigma = sigma_of(n)
    nx, ny = NY_1024[sigma], (FUSED_NX[n] if n in FUSED_NX else NX_20480)
    half = 0.01
    px = half / (ny // 2)
    w_half = _w_for_planes(_tmax(nx, ny, px, px), 5, eps)
    nu, nv = 1024, n
    if axis == "first":
        nx, ny, nu, nv = ny, nx, nv, nu
    return _case(nx, ny, nu, nv, half, w_half, w_half, seed=n + (7 if axis == "first" else 0), sigma=sigma)


def _expect_a(other, composite):
    def expect(info):
        assert info["wmode"] == 1 and info["nplanes"] == 5, _fmt(info)  # a four-plane and a one-plane launch
        # composite screens in the four-plane launch; at epsilon = 1e-9 (smaller phases) in the one-plane launch too
        assert info["screen_composite"] >= composite and info["screen_composite"] + info["screen_separable"] <= 2, _fmt(info)
        assert info["fft_mode"] & 8, _fmt(info)                                        # transposing first axis: tpitch > 0
        assert info[other] == 1024, _fmt(info)
    return expect


@pytest.mark.parametrize("ldsrow", [None, "0"], ids=["a", "d"])
@pytest.mark.parametrize("n", PLAIN_NS)
def test_second_axis_composite_planes(n, ldsrow, monkeypatch):
    """Legs a and d (the two legs of a length run back to back: one unfused plan and one set of DFT values serve both).  At the
    lengths of NO_LDS_ROW leg a cannot have the LDS image row and runs leg d's form."""
    c = _leg_a_case(n, 1e-7)
    _run(monkeypatch, ("a", n), c, n, "second", _expect_a("nu", 1), force_wmode=1, ldsrow=ldsrow,
         restate=(n in SMALLEST_NS and ldsrow is None), leg="a" if ldsrow is None else "d")


@pytest.mark.parametrize("n", SMALLEST_NS)
def test_second_axis_composite_planes_tight_epsilon(n, monkeypatch):
    """Leg a at epsilon = 1e-9 (W = 15), one shape per lead family."""
    c = _leg_a_case(n, 1e-9)
    _run(monkeypatch, ("a9", n), c, n, "second", _expect_a("nu", 2), eps=1e-9, W=15, force_wmode=1, leg="a9")


def _thin_case(n, half, w_centre, w_half, seed):
    sigma = sigma_of(n)
    return _case(NY_THIN, FUSED_NX[n], grid_size(NY_THIN, sigma), n, half, w_centre, w_half, seed, sigma=sigma)


@pytest.mark.parametrize("n", PLAIN_NS)
def test_second_axis_es_planes_separable(n, monkeypatch):
    """Leg b: ES-kernel planes, up to 3 cycles of w-phase at the corner of a field of 0.03 rad half-width -- too many for the
    composite polynomials away from w = 0, while what is left behind the linear term (w z^2 / 8: 1e-3 cycles) fits the separable
    form."""
    half = 0.03
    ny = FUSED_NX[n]
    t = _tmax(NY_THIN, ny, half / (ny // 2), half / (ny // 2))
    c = _thin_case(n, half, 1.5 / t, 1.5 / t, seed=2 * n)

    def expect(info):
        assert info["wmode"] == 0 and info["nplanes"] > 4, _fmt(info)
        assert info["screen_separable"] > 0, _fmt(info)
        assert not info["fft_mode"] & 8, _fmt(info)

    _run(monkeypatch, ("b", n), c, n, "second", expect, force_wmode=0, restate=n in SMALLEST_NS, leg="b")


@pytest.mark.parametrize("n", SMALLEST_NS)
def test_second_axis_es_planes_general_screen(n, monkeypatch):
    """Leg b, general path (n - 1 polynomial and sincos per pixel and plane): a field of 0.44 rad half-width under w around 400
    wavelengths -- no plane near w = 0, two cycles left behind the linear term: neither polynomial form fits."""
    half = 0.44
    c = _thin_case(n, half, 400.0, 15.0, seed=3 * n)

    def expect(info):
        assert info["wmode"] == 0 and info["nplanes"] > 4, _fmt(info)
        assert info["screen_composite"] == 0 and info["screen_separable"] == 0 and info["screen_poly"] > 0, _fmt(info)

    _run(monkeypatch, ("bg", n), c, n, "second", expect, force_wmode=0, leg="b-general")


@pytest.mark.parametrize("n", PLAIN_NS)
@pytest.mark.parametrize("scheme", ["flat", "one-plane"])
def test_second_axis_single_plane_launches(n, scheme, monkeypatch):
    """Leg c: k_fused_pad_fft_p<S, SC, BEAM> -- SC by the scheme, BEAM by the Hessian's beam -- and the one-plane crop.  The
    persistent kernel needs the LDS image row (asserted in _run): at the lengths of NO_LDS_ROW it cannot run, and the case covers
    k_fused_pad_fft<S, SC> on a prepared image with one plane instead."""
    half = 0.01
    ny = FUSED_NX[n]
    t = _tmax(NY_THIN, ny, half / (ny // 2), half / (ny // 2))
    w_half = 0.01 / (2.0 * math.pi * t)  # phase range 0.01: three or four kernel functions at epsilon = 1e-7
    c = _thin_case(n, half, 8.0 * w_half, w_half, seed=5 * n)
    if scheme == "flat":
        def expect(info):
            assert info["nplanes"] == 1 and info["screen_composite"] == 0 and info["screen_separable"] == 0, _fmt(info)
        _run(monkeypatch, ("c0", n), c, n, "second", expect, do_w=False, beams=(True, False), leg="c-flat")
    else:
        def expect(info):
            assert info["wmode"] == 2 and info["nplanes"] == 1 and 2 <= info["nderiv"] <= 4, _fmt(info)
            assert info["screen_composite"] == 1 and info["screen_separable"] == 0, _fmt(info)
        _run(monkeypatch, ("c2", n), c, n, "second", expect, force_wmode=2, beams=(True, False), leg="c-one-plane")


@pytest.mark.parametrize("n", PLAIN_NS)
def test_first_axis_transposing(n, monkeypatch):
    """Part 3: the image of leg a transposed -- the length under test is the first axis, the fused second axis has 1024 points."""
    c = _leg_a_case(n, 1e-7, axis="first")
    _run(monkeypatch, ("t", n), c, n, "first", _expect_a("nv", 1), force_wmode=1, leg="3")


@pytest.mark.parametrize("axis", ["second", "first"])
def test_doubled_20480_both_orientations(axis, monkeypatch):
    """20480 points, the one doubled length that transposes, on its default path (the stashing doubled kernels; they take the
    general screen form: no composite screens)."""
    c = _leg_a_case(20480, 1e-7, axis=axis)

    def expect(info):
        assert info["wmode"] == 1 and info["nplanes"] == 5, _fmt(info)
        assert info["fft_mode"] & 8, _fmt(info)
        assert info["nu" if axis == "second" else "nv"] == 1024, _fmt(info)

    _run(monkeypatch, ("t2", axis), c, 20480, axis, expect, force_wmode=1, leg="3-doubled")
