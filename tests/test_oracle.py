"""CPU tests that pin the oracle (no GPU): the algorithm restatement against the exact DFT, the
reference's analytic identities, and the committed golden vectors."""

import numpy as np
import pytest

from oracle import dft, fftconv
from oracle import weighting as ow
from oracle import wgridder as owg
from pfb_imaging_amd.utils import synth


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def _case(nrow=2000, nchan=2, npix=48, zscale=0.3, widen=40.0, seed=1):
    c = synth.make_case(nrow, nchan, npix, zscale=zscale, seed=seed)
    c["cell"] *= widen
    return c


@pytest.mark.parametrize("K, widen, eps", [(2, 30.0, 1e-4), (3, 130.0, 1e-7), (4, 200.0, 1e-7), (3, 60.0, 1e-9)])
def test_one_plane_scheme_vs_dft(K, widen, eps):
    """wmode 2: one uv-plane, the w-term in differentiated gridding kernels (oracle/pfb_oracle.c: pfbo_grid_plane_wd)."""
    c = synth.make_case(2500, 2, 64, zscale=1e-3, seed=5)
    cell = c["cell"] * widen
    plan = owg.Plan(c["uvw"], c["freq"], c["mask"], 64, 60, cell, cell * 1.1, 0.0, 0.0, eps, False, True, False, True, False,
                    force_wmode=2)
    assert plan.p.wmode == 2 and plan.p.nplanes == 1 and plan.p.nderiv == K
    x = c["x"][:, :60]
    ref = dft.dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], c["mask"], 64, 60, cell, cell * 1.1, 0, 0, False, True, False,
                            True, False)
    assert rel(plan.vis2dirty(c["vis"], c["wgt"]), ref) < eps
    refv = dft.dft_dirty2vis(c["uvw"], c["freq"], x, cell, cell * 1.1, 0, 0, False, True, False, True, False)
    refv[c["mask"] == 0] = 0
    v = plan.dirty2vis(x)
    assert rel(v, refv) < eps
    y = c["vis"] * c["mask"]
    lhs = np.vdot(v, y).real
    assert abs(lhs - np.vdot(x, plan.vis2dirty(y))) < 1e-12 * abs(lhs)
    with pytest.raises(ValueError):  # off-axis phase centres are not admissible (t is not a function of l^2 + m^2)
        owg.Plan(c["uvw"], c["freq"], c["mask"], 64, 60, cell, cell, 0.01, 0.0, eps, False, True, False, True, False, force_wmode=2)


@pytest.mark.parametrize("wmode", [0, 1])
@pytest.mark.parametrize("center", [(0.0, 0.0), (0.01, -0.02)])
def test_restatement_vs_dft(wmode, center):
    c = _case()
    kw = dict(uvw=c["uvw"], freq=c["freq"], pixsize_x=c["cell"], pixsize_y=c["cell"], center_x=center[0],
              center_y=center[1], epsilon=1e-7, flip_v=True, do_wgridding=True, divide_by_n=False, force_wmode=wmode)
    d = owg.vis2dirty(vis=c["vis"], wgt=c["wgt"], mask=c["mask"], npix_x=48, npix_y=48, **kw)
    ref = dft.dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], c["mask"], 48, 48, c["cell"], c["cell"], center[0],
                            center[1], False, True, False, True, False)
    assert rel(d, ref) < 1e-7
    v = owg.dirty2vis(dirty=c["x"], mask=c["mask"], **kw)
    refv = dft.dft_dirty2vis(c["uvw"], c["freq"], c["x"], c["cell"], c["cell"], center[0], center[1], False, True, False,
                             True, False)
    refv[c["mask"] == 0] = 0
    assert rel(v, refv) < 1e-7


def test_mode_choice_and_exact_kernel_option():
    """Narrow fields pick polynomial w-planes (fewer planes than the kernel support) -- or, with the phase centre on axis,
    ONE plane with that many kernel functions --, wide fields the ES-kernel planes; the polynomial kernel form agrees with
    the exact kernel."""
    narrow = _case(zscale=1e-3, widen=1.0)
    p = owg.Plan(narrow["uvw"], narrow["freq"], narrow["mask"], 48, 48, narrow["cell"], narrow["cell"], epsilon=1e-7,
                 flip_v=True, divide_by_n=False)
    assert p.p.wmode == 2 and p.p.nplanes == 1 and 2 <= p.p.nderiv < p.p.W
    p = owg.Plan(narrow["uvw"], narrow["freq"], narrow["mask"], 48, 48, narrow["cell"], narrow["cell"], 1e-4, 0.0, epsilon=1e-7,
                 flip_v=True, divide_by_n=False)
    assert p.p.wmode == 1 and p.p.nplanes < p.p.W
    wide = _case()
    q = owg.Plan(wide["uvw"], wide["freq"], wide["mask"], 48, 48, wide["cell"], wide["cell"], 0.01, -0.02, epsilon=1e-7,
                 flip_v=True, divide_by_n=False)
    assert q.p.wmode == 0 and q.p.nplanes > q.p.W
    q2 = owg.Plan(wide["uvw"], wide["freq"], wide["mask"], 48, 48, wide["cell"], wide["cell"], 0.01, -0.02,
                  epsilon=1e-7, flip_v=True, divide_by_n=False, use_poly_kernel=False)
    assert rel(q.vis2dirty(wide["vis"], wide["wgt"]), q2.vis2dirty(wide["vis"], wide["wgt"])) < 1e-9


# ---- wide, near-coplanar fields (shared with tests/test_gpu_wide_field.py) ----------------------------------------------------


def compact_case(nx, ny, half, dw, eps, w0=0.0, center=(0.0, 0.0), divide_by_n=False, nrow=600, seed=0):
    """A compact array observed at one channel of 100 MHz: uv uniform with max |u| cell ~ 0.4, |w| uniform over
    [w0, w0 + dw] wavelengths (random signs: the Hermitian fold runs), 5 % of the rows masked.  The image is nx x ny with the
    larger axis reaching `half` off its centre (pixel i at (i - n // 2) cell).  Returns the data, the geometry keywords of
    owg.Plan / Gridder (flip_v=True) and the largest l^2 + m^2 of an on-axis image (smax)."""
    rng = np.random.default_rng(seed)
    cell = half / (max(nx, ny) // 2)
    lam = owg.SPEED_OF_LIGHT / 1e8
    uv = rng.uniform(-0.4 / cell, 0.4 / cell, (nrow, 2))
    w = (w0 + dw * rng.random(nrow)) * rng.choice([-1.0, 1.0], nrow)
    kw = dict(npix_x=nx, npix_y=ny, pixsize_x=cell, pixsize_y=cell, center_x=center[0], center_y=center[1], epsilon=eps,
              flip_u=False, flip_v=True, flip_w=False, do_wgridding=True, divide_by_n=divide_by_n)
    if divide_by_n:  # n = 0 (the horizon) gives inf on both sides: keep every pixel well off it
        ls, ms = center[0], -center[1]
        r2 = ((ls + (np.arange(nx) - nx // 2) * cell)[:, None] ** 2 + (ms + (np.arange(ny) - ny // 2) * cell)[None, :] ** 2)
        assert np.abs(1.0 - r2).min() > 1e-6, "divide_by_n geometry with a pixel on the horizon"
    return dict(uvw=np.column_stack([uv, w]) * lam, freq=np.array([1e8]), vis=(rng.standard_normal((nrow, 1)) +
                1j * rng.standard_normal((nrow, 1))), wgt=np.exp(rng.standard_normal((nrow, 1))),
                mask=(rng.random((nrow, 1)) > 0.05).astype(np.uint8), x=rng.standard_normal((nx, ny)), kw=kw,
                smax=owg.wd_smax(nx, ny, cell, cell))


# (nx, ny, half-field, w spread dw, w0, epsilon, centre, divide_by_n).  Half-fields 0.8 and 0.9 (and 0.75 at the corners) reach
# past the horizon; the first five rows were wrong under the one-plane admission by the linear-phase bound alone (NaN images:
# nodes past s = 1; 1.2-8 epsilon: the curvature of n(s) for a small w spread); the last two put the image corner at
# l^2 + m^2 = 0.49 and 0.51, either side of the fitted n - 1 screen's gate (rowfft.hip: fused_geom_fit).
WIDE_FIELD_CASES = [
    (64, 64, 0.8, 3e-3, 0.0, 1e-3, (0.0, 0.0), False),
    (64, 64, 0.9, 0.03, 0.0, 1e-3, (0.0, 0.0), False),
    (64, 64, 0.5, 1e-4, 0.0, 1e-7, (0.0, 0.0), False),
    (48, 48, 0.2, 0.3, 0.0, 1e-9, (0.0, 0.0), False),
    (64, 64, 0.6, 0.36, 0.0, 1e-4, (0.0, 0.0), False),
    (64, 64, 0.75, 30.0, 0.0, 1e-5, (0.0, 0.0), False),
    (64, 64, 0.9, 3.0, 0.0, 1e-7, (0.0, 0.0), True),
    (50, 41, 0.3, 10.0, 0.0, 1e-6, (0.3, -0.4), False),
    (64, 64, 0.05, 0.5, 0.0, 1e-7, (0.0, 0.0), False),
    (63, 63, 0.05, 0.0, 0.0, 1e-5, (0.0, 0.0), False),
    (64, 48, 0.2, 0.0, 5.0, 1e-6, (0.0, 0.0), False),
    (64, 64, 0.35, 1.0, 0.0, 1e-7, (0.0, 0.0), False),
    (64, 64, 0.35, 0.05, 0.0, 1e-9, (0.0, 0.0), False),
    (48, 64, 0.5, 2.0, 0.0, 1e-5, (0.0, 0.0), True),
    (64, 64, 0.69, 0.1, 0.0, 1e-6, (0.0, 0.0), True),
    (64, 64, 0.69, 1.0, 0.0, 1e-3, (0.0, 0.0), False),
    (64, 64, 0.75, 0.01, 0.0, 1e-7, (0.0, 0.0), False),
    (64, 64, 0.8, 30.0, 0.0, 1e-4, (0.0, 0.0), False),
    (65, 65, 0.9, 0.3, 0.0, 1e-5, (0.0, 0.0), False),
    (64, 64, 0.2, 5.0, 0.0, 1e-6, (0.2, 0.1), False),
    (64, 64, 0.35, 0.3, 0.0, 1e-4, (0.2, 0.1), True),
    (64, 64, 0.5, 0.0, 0.0, 1e-7, (0.0, 0.0), False),
    (64, 64, 0.5, 0.0, 2.0, 1e-7, (0.0, 0.0), False),
    (64, 64, 0.5, 0.02, 0.0, 1e-9, (0.0, 0.0), True),
    (64, 64, float(np.sqrt(0.245)), 0.5, 3.0, 1e-7, (0.0, 0.0), False),
    (64, 64, float(np.sqrt(0.255)), 0.5, 3.0, 1e-7, (0.0, 0.0), False),
]


def wide_field_id(g):
    nx, ny, half, dw, w0, eps, center, divn = g
    return (f"{nx}x{ny}-h{half:.3g}-dw{dw:g}" + (f"-w0{w0:g}" if w0 else "") + f"-eps{eps:g}" +
            (f"-c{center[0]:g},{center[1]:g}" if center != (0.0, 0.0) else "") + ("-divn" if divn else ""))


def wide_field_refs(c):
    """DFT dirty image (weighted, masked) and masked visibilities of c["x"]."""
    k = c["kw"]
    geo = (k["pixsize_x"], k["pixsize_y"], k["center_x"], k["center_y"], k["flip_u"], k["flip_v"], k["flip_w"], True,
           k["divide_by_n"])
    ref = dft.dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], c["mask"], k["npix_x"], k["npix_y"], *geo)
    refv = dft.dft_dirty2vis(c["uvw"], c["freq"], c["x"], *geo)
    refv[c["mask"] == 0] = 0
    return ref, refv


@pytest.mark.parametrize("geom", WIDE_FIELD_CASES, ids=wide_field_id)
def test_wide_field_schemes_vs_dft(geom):
    """The automatic choice and every w-scheme the plan admits meet epsilon against the DFT at wide, near-coplanar fields (up to
    and past the horizon); the one-plane scheme is refused -- ValueError, never a NaN image -- where its interpolation in
    s = l^2 + m^2 cannot reach its share of epsilon or the image reaches the horizon."""
    nx, ny, half, dw, w0, eps, center, divn = geom
    c = compact_case(nx, ny, half, dw, eps, w0=w0, center=center, divide_by_n=divn)
    k = c["kw"]
    ref, refv = wide_field_refs(c)
    admitted = {}
    for fw in (None, 0, 1, 2):
        try:
            plan = owg.Plan(c["uvw"], c["freq"], c["mask"], k["npix_x"], k["npix_y"], k["pixsize_x"], k["pixsize_y"],
                            k["center_x"], k["center_y"], eps, k["flip_u"], k["flip_v"], k["flip_w"], True, divn,
                            force_wmode=fw)
        except ValueError:
            assert fw is not None, "the automatic choice must always find a scheme"
            continue
        admitted[fw] = plan.p.wmode
        d = plan.vis2dirty(c["vis"], c["wgt"])
        v = plan.dirty2vis(c["x"])
        assert np.isfinite(d).all() and np.isfinite(v).all(), (fw, plan.p)
        assert rel(d, ref) <= eps, (fw, plan.p, rel(d, ref) / eps)
        assert rel(v, refv) <= eps, (fw, plan.p, rel(v, refv) / eps)
        if plan.p.wmode == 2:
            assert c["smax"] < 1.0 and center == (0.0, 0.0)
            K = plan.p.nderiv
            assert owg.wd_interp_error(K, c["smax"], plan.p.whalf, plan.p.nshift) <= 2.0 / 3.0 * eps
    assert admitted[0] == 0 and admitted[None] in (0, 1, 2)
    if c["smax"] >= 1.0 or center != (0.0, 0.0) or dw == 0.0:
        assert 2 not in admitted, "the one-plane scheme admitted past the horizon, off axis or without a w spread"


def test_wide_field_one_plane_interp_error():
    """The measured interpolation error of the one-plane scheme: infinite (inadmissible) at and past the horizon, and for a
    wide field with a small w spread far above the linear-phase bound poly_planes_needed sized K by."""
    assert owg.wd_interp_error(2, 1.0, 0.01, 0.0) == np.inf and owg.wd_interp_error(4, 1.28, 0.01, 0.0) == np.inf
    assert owg.wd_choose_K(2, 1.28, 1e-3, 0.0, 1.0) is None
    # 64^2, half-field 0.5 (smax 0.5), w spread 1e-4: omega = 2 pi 0.5e-4 tmax ~ 9e-5 -> K = 2 by the bound (~2e-9 < 6.7e-8)
    lo, hi = owg.nm1_range(64, 64, 0.5 / 32, 0.5 / 32, 0.0, 0.0)
    nshift = -0.5 * (lo + hi)
    omega = 2.0 * np.pi * 0.5e-4 * max(abs(lo + nshift), abs(hi + nshift))
    assert owg.cheb_planes_needed(omega, 2e-7 / 3.0) == 2
    e2 = owg.wd_interp_error(2, owg.wd_smax(64, 64, 0.5 / 32, 0.5 / 32), 0.5e-4, nshift)
    assert e2 > 10 * omega ** 2 / 4.0 and e2 > 2e-7 / 3.0
    assert owg.wd_choose_K(2, owg.wd_smax(64, 64, 0.5 / 32, 0.5 / 32), 0.5e-4, nshift, 2e-7 / 3.0) in (3, 4)


def test_adjointness_linearity_no_wgridding():
    c = _case()
    p = owg.Plan(c["uvw"], c["freq"], c["mask"], 48, 48, c["cell"], c["cell"], 0.0, 0.0, 1e-7, False, True, False,
                 False, False)
    y = c["vis"] * c["mask"]
    lhs = np.vdot(p.dirty2vis(c["x"]), y).real
    rhs = np.vdot(c["x"], p.vis2dirty(y))
    assert abs(lhs - rhs) < 1e-12 * abs(rhs)
    ref = dft.dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], c["mask"], 48, 48, c["cell"], c["cell"], 0, 0, False,
                            True, False, False, False)
    assert rel(p.vis2dirty(c["vis"], c["wgt"]), ref) < 1e-7


def test_reference_conventions_golden(golden_dir):
    """test_wgridder_conventions (test_hessian_approx.py:128-185) on the golden vectors: restatement
    within atol 1e-4 at epsilon 1e-6 (two of the five offsets to keep the CPU suite short); the
    golden vectors themselves equal the reference's explicit formula."""
    gold = np.load(f"{golden_dir}/conventions_two_sources.npz")
    uvw, freq, npix, pix = gold["uvw"], gold["freq"], int(gold["npix"]), float(gold["pixsize"])
    dirty = np.zeros((npix, npix))
    dirty[npix // 2, npix // 2] = 1.0
    dirty[npix // 4, npix // 4] = 1.0
    for k in (0, 2):
        l0, m0 = gold["offsets"][k]
        # explicit_wdegridder, test_hessian_approx.py:44-67
        ve = np.zeros_like(gold["vis"][k])
        for xi, yi in ((npix // 2, npix // 2), (npix // 4, npix // 4)):
            lc = -l0 + (-npix / 2 + xi) * pix
            mc = m0 + (-npix / 2 + yi) * pix
            nc = np.sqrt(1 - lc * lc - mc * mc)
            ph = (uvw[:, 0:1] * lc - uvw[:, 1:2] * mc - uvw[:, 2:3] * (nc - 1)) * freq[None, :] / 299792458.0
            ve += np.exp(-2j * np.pi * ph) / nc
        assert np.abs(ve - gold["vis"][k]).max() < 1e-8
        vis = owg.dirty2vis(uvw=uvw, freq=freq, dirty=dirty, pixsize_x=pix, pixsize_y=pix, center_x=-l0, center_y=-m0,
                            epsilon=1e-6, do_wgridding=True, flip_u=False, flip_v=True, flip_w=False, divide_by_n=True)
        np.testing.assert_allclose(vis.real, gold["vis"][k].real, atol=1e-4)
        np.testing.assert_allclose(vis.imag, gold["vis"][k].imag, atol=1e-4)


def test_hessian_equals_psf_convolution():
    """test_hessian (test_hessian_approx.py:234-307): grid o degrid of a delta (no w-gridding) equals
    the FFT convolution with the PSF gridded from unit visibilities."""
    c = synth.make_case(1500, 2, 32, seed=3)
    nx = ny = 32
    nxp = nyp = 64
    cell = c["cell"]
    kw = dict(uvw=c["uvw"], freq=c["freq"], pixsize_x=cell, pixsize_y=cell, epsilon=1e-10, flip_v=True,
              do_wgridding=False, divide_by_n=False)
    psf = owg.vis2dirty(vis=np.ones_like(c["vis"]), npix_x=nxp, npix_y=nyp, **kw)
    psfhat = np.fft.rfft2(np.fft.ifftshift(psf))
    x = np.zeros((nx, ny))
    x[nx // 2, ny // 2] = 1.0
    res1 = owg.vis2dirty(vis=owg.dirty2vis(dirty=x, **kw), npix_x=nx, npix_y=ny, **kw)
    res2 = fftconv.psf_convolve(x, psfhat, nxp, nyp)
    scale = np.abs(res2).max()
    assert np.allclose(1 + (res2 - res1) / scale, 1)


def test_synth_partition_and_wstack_golden(golden_dir):
    g = np.load(f"{golden_dir}/synth_partition.npz")
    d = owg.vis2dirty(uvw=g["uvw"], freq=g["freq"], vis=g["vis"][0], wgt=g["wgt"][0], mask=g["mask"], npix_x=16,
                      npix_y=16, pixsize_x=float(g["cell"]), pixsize_y=float(g["cell"]), epsilon=1e-7, flip_v=True,
                      do_wgridding=True, divide_by_n=False)
    assert np.abs(d - g["dirty"]).max() < 1e-7 * np.abs(g["dirty"]).max()
    w = np.load(f"{golden_dir}/wstack_small.npz")
    p = owg.Plan(w["uvw"], w["freq"], w["mask"], 48, 48, float(w["cell"]), float(w["cell"]), w["center"][0],
                 w["center"][1], 1e-7, False, True, False, True, False)
    assert rel(p.vis2dirty(w["vis"], w["wgt"]), w["dirty"]) < 1e-7
    assert rel(p.dirty2vis(w["x"]), w["mvis"]) < 1e-7
    assert rel(p.vis2dirty(p.dirty2vis(w["x"]), w["wgt"]), w["hess"]) < 2e-7


def test_fftconv_identities():
    """HessianTree identities of test_hessian_tree.py:20-66 on the numpy restatement, and pcg."""
    rng = np.random.default_rng(0)
    nx = ny = 16
    nxp = nyp = 32
    x = rng.standard_normal((1, nx, ny))
    one = [{"psfhat": np.ones((1, nxp, nyp // 2 + 1)), "beam": np.ones((1, nx, ny)), "wsum": np.ones(1)}]
    np.testing.assert_allclose(fftconv.hessian_tree_dot(x, one, nxp, nyp), x, atol=1e-12)
    np.testing.assert_allclose(fftconv.hessian_tree_dot(x, one, nxp, nyp, eta=0.5), 1.5 * x, atol=1e-12)
    np.testing.assert_allclose(fftconv.hessian_tree_dot(x, one + one, nxp, nyp), x, atol=1e-12)
    a = rng.standard_normal((3, 20, 20))
    assert rel(fftconv.c2r(fftconv.r2c(a), 20), a) < 1e-14
    d = 1.0 + rng.random((nx, ny))
    sol = fftconv.pcg(lambda z: d * z, d * x[0], tol=1e-12, maxit=100, minit=1)
    np.testing.assert_allclose(sol, x[0], atol=1e-8)


@pytest.mark.parametrize("srf", [1.0, 2.0, 3.2])
def test_counts_uniform_recount(srf):
    """test_counts (test_weighting.py:47-118): uniform imaging weights make every occupied cell count 1."""
    c = synth.make_case(3000, 4, 128, seed=4)
    rng = np.random.default_rng(420)
    cell = c["cell"] * 2.0 / srf
    wgt = np.exp(rng.standard_normal((2,) + c["mask"].shape))
    mask = np.ones_like(c["mask"])
    nx = ny = 150
    counts = ow.compute_counts(c["uvw"], c["freq"], mask, wgt, nx, ny, cell, cell, usign=1.0, vsign=-1.0)
    assert np.isclose(counts.sum(), wgt[:, ow.uvcell_index(c["uvw"], c["freq"], mask, nx, ny, cell, cell) >= 0].sum())
    imwgt = ow.counts_to_weights(counts.copy(), c["uvw"], c["freq"], np.ones_like(wgt), mask, nx, ny, cell, cell, -3,
                                 usign=1.0, vsign=-1.0)
    counts2 = ow.compute_counts(c["uvw"], c["freq"], mask, wgt * imwgt, nx, ny, cell, cell, usign=1.0, vsign=-1.0)
    assert np.allclose(counts2[counts2 > 0], 1.0, rtol=1e-8, atol=1e-8)


def test_uv2xy_golden(golden_dir):
    """test_uv2xy (test_weighting.py:121-137) on the committed vectors, numpy formula and C index map."""
    gold = np.load(f"{golden_dir}/uv2xy.npz")
    for key in gold.files:
        _, nx, cellx = key.split("_")
        nx, cellx = int(nx), float(cellx)
        u = gold[key]
        ucell = 1.0 / (nx * cellx)
        umax = np.abs(1 / cellx / 2)
        assert ((np.floor((u + umax) / ucell) - np.arange(nx)) == 0).all()
        uvw = np.stack([u, np.full(nx, 0.25 / cellx), np.zeros(nx)], axis=1)
        cell = ow.uvcell_index(uvw, np.array([299792458.0]), np.ones((nx, 1), np.uint8), nx, 4, cellx, cellx, 1.0, 1.0)
        assert np.array_equal(cell[:, 0] // 4, np.arange(nx))


def test_kernel_table_and_poly():
    tab = owg.kernel_table()
    assert len(tab) == 15 * 13
    for r in tab:
        assert r["eps"] <= r["eps_max"] and 4 <= r["W"] <= 16
    # errors decrease with W at fixed sigma until the double-precision floor
    s2 = sorted((r for r in tab if r["sigma"] == 2.0), key=lambda r: r["W"])
    assert all(a["eps"] > b["eps"] for a, b in zip(s2[:9], s2[1:10]))
    W, beta = 12, next(r["beta"] for r in tab if r["W"] == 12 and r["sigma"] == 1.5)
    kt = owg.kernel_poly_table(W, beta)
    f = np.linspace(0, 1, 101)
    for a in range(W):
        x = (a + 1 - W / 2 - f) * 2 / W
        exact = np.exp(beta * (np.sqrt(np.maximum(1 - x * x, 0)) - 1))
        approx = np.polynomial.polynomial.polyval(2 * f - 1, kt[a])
        assert np.abs(exact - approx).max() < 1e-11
    assert owg.good_size(11468) == 11520 and owg.good_size(1025, True) == 1080


def test_psi_oracle_pins():
    """oracle/psi.py has no reference fixtures (PyWavelets is not installed): it is pinned by the algebra the
    reference's own tests check (tests/test_wavelets.py:72-132: perfect reconstruction) plus adjointness,
    hand-worked Haar values and the bookkeeping formulas of operators/psi.py:73-113."""
    from oracle import psi as opsi

    # Haar by hand: pywt.dwt([1,2,3,4], 'db1') -> cA = [3, 7]/sqrt2, cD = [-1, -1]/sqrt2
    lo, hi, rlo, rhi = opsi.filters("db1")
    x = np.array([[1.0, 2.0, 3.0, 4.0]])
    assert np.allclose(opsi.down_conv(x, lo, 1), np.array([[3.0, 7.0]]) / np.sqrt(2))
    assert np.allclose(opsi.down_conv(x, hi, 1), np.array([[-1.0, -1.0]]) / np.sqrt(2))
    # db2 analytic scaling filter
    s3 = np.sqrt(3.0)
    assert np.allclose(opsi.filters("db2")[2], np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2)), atol=1e-15)
    # bookkeeping for 64 x 48, db2, 3 levels (psi.py:73-113 by hand: 33/18/10 and 25/14/8 coefficients per level)
    bk = opsi.Bookkeeping(64, 48, ("self", "db2"), 3)
    assert list(bk.sx[0]) == [33, 18, 10] and list(bk.sy[0]) == [25, 14, 8]
    assert bk.ntotx[0] == 71 and bk.ntoty[0] == 55 and (bk.nxmax, bk.nymax) == (71, 55)
    assert list(bk.ix[0, :, 1]) == [71, 38, 20] and list(bk.spx[0]) == [64, 34, 18]
    rng = np.random.default_rng(0)
    for bases, nl, shape in ((("self", "db1", "db2", "db3"), 3, (64, 48)), (("db4", "db5"), 2, (128, 256))):
        nx, ny = shape
        P = opsi.Psi(2, nx, ny, bases, nl)
        x = rng.standard_normal((2, nx, ny))
        a = np.zeros((2, P.nbasis, P.nxmax, P.nymax))
        P.dot(x, a)
        xr = np.zeros_like(x)
        P.hdot(a, xr)
        assert np.abs(xr / len(bases) - x).max() < 1e-13
        b = rng.standard_normal(a.shape)
        xb = np.zeros_like(x)
        P.hdot(b, xb)
        assert abs(np.vdot(a, b) - np.vdot(x, xb)) < 1e-10 * abs(np.vdot(x, xb))


# ---------------------------------------------------------------------------------------------------------
# Reference-RUN fixtures (tests/golden/ref_pins.npz, conventions_two_sources.npz): outputs of the reference's own
# undecorated numpy / scipy functions, executed by tests/golden/make_ref_pins.py in the build container.  These
# tests need neither /root/reference nor a GPU.
# ---------------------------------------------------------------------------------------------------------

def test_oracle_vs_reference_run_fixtures(golden_dir):
    """oracle/dft.py, oracle/psi.py (prox_21m, dual_update), oracle/weighting.py (filter / box sum), oracle/fftconv.py
    (taperf, power_method) reproduce what the REFERENCE's functions returned on the same inputs.

    Tolerances: 1e-12 (absolute, on O(1) values) wherever the arithmetic is well conditioned; the two-point-source
    visibilities of the reference's own test geometry carry phases of ~1e6 rad, whose f64 rounding alone is 1e-10, so
    that case is held to 2e-9 (the reference's own test holds ducc0 to 1e-4 there)."""
    pins = np.load(f"{golden_dir}/ref_pins.npz")
    conv = np.load(f"{golden_dir}/conventions_two_sources.npz")
    assert "reference" in str(conv["source"])

    # -- measurement equation: the reference's test geometry, all five offsets, both conventions ------------------
    uvw, freq, npix, pix = conv["uvw"], conv["freq"], int(conv["npix"]), float(conv["pixsize"])
    dirty = np.zeros((npix, npix))
    dirty[npix // 2, npix // 2] = 1.0
    dirty[npix // 4, npix // 4] = 1.0
    for k, (l0, m0) in enumerate(conv["offsets"]):
        # explicit_wdegridder (flip_v = True, centre = wgridder_conventions(l0, m0))
        v = dft.dft_dirty2vis(uvw, freq, dirty, pix, pix, -l0, -m0, False, True, False, True, True)
        assert np.abs(v - conv["vis"][k]).max() < 2e-9
        # explicit_degridder, "casa" convention = ducc0's defaults (no flips), centre (-l0, -m0)
        v = dft.dft_dirty2vis(uvw, freq, dirty, pix, pix, -l0, -m0, False, False, False, True, True)
        assert np.abs(v - conv["vis_casa"][k]).max() < 2e-9
        assert np.abs(v - conv["vis_casa_negw"][k]).max() < 2e-9

    # -- the same on a dense, well-conditioned wide-field case: every pixel, 1e-12 ---------------------------------
    px, py = pins["dense_pix"]
    img = pins["dense_img"]
    for k, (l0, m0) in enumerate(pins["conv_lm"][:3]):
        v = dft.dft_dirty2vis(pins["dense_uvw"], pins["dense_freq"], img, px, py, -l0, -m0, False, True, False, True, True)
        assert np.abs(v - pins["dense_vis_w"][k]).max() < 1e-12 * np.abs(pins["dense_vis_w"][k]).max()
        v = dft.dft_dirty2vis(pins["dense_uvw"], pins["dense_freq"], img, px, py, -l0, -m0, False, False, False, True, True)
        assert np.abs(v - pins["dense_vis_casa"][k]).max() < 1e-12 * np.abs(pins["dense_vis_casa"][k]).max()
        # and the adjoint the oracle defines from it: <R x, y> == <x, R^H y> ties dft_vis2dirty to the pinned direction
        y = pins["dense_vis_w"][k]
        d = dft.dft_vis2dirty(pins["dense_uvw"], pins["dense_freq"], y, None, None, img.shape[0], img.shape[1], px, py,
                              -l0, -m0, False, True, False, True, True)
        lhs = np.vdot(pins["dense_vis_w"][k], y).real
        assert abs(np.vdot(img, d) - lhs) < 1e-11 * abs(lhs)

    # -- l21 prox / dual update ------------------------------------------------------------------------------------
    from oracle import psi as opsi

    for i in range(3):
        v, w, s = pins[f"prox{i}_v"], pins[f"prox{i}_w"], float(pins[f"prox{i}_sigma"])
        assert np.abs(opsi.prox_21m(v, s, weight=w) - pins[f"prox{i}_out"]).max() < 1e-12
        assert np.abs(opsi.prox_21m(v, s) - pins[f"prox{i}_out_w1"]).max() < 1e-12
    # dual_update (allocating form, prox_21m.py:64-71) == the fused in-place form the oracle restates
    # (dual_update_numba_fast, :105-135) given the analysis coefficients of x
    q, x = pins["du_q"], pins["du_x"]
    coeffs = np.stack([x, np.einsum("ij,bjk->bik", q, x)], axis=1)
    got = opsi.dual_update(pins["du_v"].copy(), coeffs, float(pins["du_lam"]), float(pins["du_sigma"]), pins["du_w"])
    assert np.abs(got - pins["du_out"]).max() < 1e-12

    # -- counts filters ----------------------------------------------------------------------------------------------
    for lvl in (10.0, 2.0, 0.0):
        got = ow.filter_extreme_counts(pins["cnt_in"].copy(), level=lvl)
        assert np.abs(got - pins[f"cnt_filter_{lvl}"]).max() < 1e-12
    for s in (0, 1, 2, 5):
        got = ow.box_sum_counts(pins["cnt_in"].copy(), s)
        assert np.abs(got - pins[f"cnt_box_{s}"]).max() < 1e-12 * max(1.0, np.abs(pins[f"cnt_box_{s}"]).max())

    # -- taper, power method -------------------------------------------------------------------------------------------
    for key in [k for k in pins.files if k.startswith("taper_")]:
        _, n0, n1, width = key.split("_")
        assert np.abs(fftconv.taperf((int(n0), int(n1)), int(width)) - pins[key]).max() < 1e-15
    a, b = pins["pm_a"], pins["pm_b"]
    beta, vec, _ = fftconv.power_method(lambda z: a @ z @ b, pins["pm_b0"].shape, pins["pm_b0"].copy(), tol=1e-10, maxit=400)
    assert abs(beta - float(pins["pm_beta"])) < 1e-12 * abs(beta)
    assert np.abs(vec - pins["pm_vec"]).max() < 1e-12


def test_product_host_code_vs_reference_run_fixtures(golden_dir):
    """The product's HOST-side mirrors (no device work in them) against the same reference-run fixtures:
    wgridder_conventions, taperf, the host loops of power_method and of the legacy primal_dual."""
    from pfb_imaging_amd import opt
    from pfb_imaging_amd.operators import gridder as pg
    from pfb_imaging_amd.operators import hessian as ph

    pins = np.load(f"{golden_dir}/ref_pins.npz")
    for (l0, m0), want in zip(pins["conv_lm"], pins["conv_out"]):
        assert [float(v) for v in pg.wgridder_conventions(l0, m0)] == list(want)
    for key in [k for k in pins.files if k.startswith("taper_")]:
        _, n0, n1, width = key.split("_")
        assert np.abs(ph.taperf((int(n0), int(n1)), int(width)) - pins[key]).max() < 1e-15
    a, b = pins["pm_a"], pins["pm_b"]
    beta, vec = opt.power_method(lambda z: a @ z @ b, pins["pm_b0"].shape, b0=pins["pm_b0"].copy(), tol=1e-10, maxit=400,
                                 verbosity=0)
    assert abs(beta - float(pins["pm_beta"])) < 1e-12 * abs(beta)
    assert np.abs(vec - pins["pm_vec"]).max() < 1e-12

    from oracle import psi as opsi

    q, h, rhs, w = pins["pd_q"], pins["pd_h"], pins["pd_b"], pins["pd_w"]
    nband, nym, nxm = h.shape
    for pos in (0, 1, 2):
        x, v = opt.primal_dual(np.zeros((nband, nym, nxm)), np.zeros((nband, 2, nym, nxm)), float(pins["pd_lam"]),
                               lambda c: c[:, 0] + np.einsum("ji,bjk->bik", q, c[:, 1]),
                               lambda z: np.stack([z, np.einsum("ij,bjk->bik", q, z)], axis=1), float(h.max()),
                               lambda c, s: opsi.prox_21m(c, s, weight=w), lambda z: h * z - rhs, nu=2.0, tol=1e-9,
                               maxit=60, minit=10, positivity=pos, verbosity=0)
        assert np.abs(x - pins[f"pd_x_{pos}"]).max() < 1e-12
        assert np.abs(v - pins[f"pd_v_{pos}"]).max() < 1e-12
