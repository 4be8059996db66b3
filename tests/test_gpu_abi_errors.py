"""Host-side refusals of the C ABI that come after the call has enqueued copies from or into the caller's arrays.

The psfconv, comps and gridder entry points run what they enqueue inside one stream scope (``synced`` of
csrc/abi_scope.hpp) that waits for the stream also when the body throws, so an error status is never returned while a
copy is still in flight.  These tests walk error paths that scope owns: the refused call raises ``ValueError`` with the
library's message, the handle stays usable, and a valid call after the refusal computes what it should.

They cannot show the early return itself: copies of this size (a 32 x 32 image, a 64 x 64 padded PSF, 900 x 2
visibilities) finish long before Python looks at the arrays, so the tests would most likely pass without the scope too.
That defect is shown from the code; what is checked here is that the rewritten paths still refuse, recover and compute
correctly.

What "correctly" means: the psfconv and comps kernels are deterministic, so the valid call after the refusal returns bit
for bit what the same handle returned before it.  The gridder's scatter kernels add with floating-point atomics, two
valid calls need not agree in the last bits, and so every valid gridder result is held to the CPU oracle instead, with
the tolerances of tests/test_gpu_gridder.py at the plan's epsilon (1e-7): 1e-10 relative L2 against the algorithm's
restatement (oracle.wgridder), epsilon against the direct DFT (oracle.dft), 1e-6 for the CG solution and the power
method's vector and 1e-8 for its eigenvalue against their restatements (oracle.fftconv).  The float32 Hessian takes
float32-representable inputs and rounds its float64 result once, to nearest: 2^-24 relative per pixel, hence 2^-24 in
relative L2, on top of the 1e-10.  The gridder plan is the one of test_gridder_power_method_matches_oracle there (900
rows x 2 channels, a 32 x 32 image, w-gridding on), the smallest that file builds a handle for.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import dft  # noqa: E402
from oracle.fftconv import pcg, power_method as pm_oracle  # noqa: E402
from tests.test_gpu_gridder import gpu_plan, make, oracle_plan, rel  # noqa: E402

NX = NY = 32
NXP = NYP = 64
EPS = 1e-7  # gpu_plan's epsilon


@pytest.fixture()
def psfconv():
    from pfb_imaging_amd.psfconv import PsfConv

    rng = np.random.default_rng(11)
    psf = rng.standard_normal((NXP, NYP))
    p = PsfConv(NX, NY, NXP, NYP)
    p.set_psfhat(0, np.abs(np.fft.rfft2(np.fft.ifftshift(psf))) + 1.0)
    p.set_beam(0, 0.5 + rng.random((NX, NY)))  # the taper of direct()
    p.set_beam(1, 0.5 + rng.random((NX, NY)))
    yield p, rng.standard_normal((NX, NY))
    p.close()


def test_psfconv_direct_unbound_beam_slot(psfconv):
    p, x = psfconv
    raw0, raw1, raw2 = (np.full((NX, NY), np.nan) for _ in range(3))
    before = p.direct(x, 0, 0, 1.0, beam_slot=1, min_beam=0.6, raw=raw0).copy()
    with pytest.raises(ValueError, match="beam slot 3 is not bound"):
        p.direct(x, 0, 0, 1.0, beam_slot=3, min_beam=0.6, raw=raw1)  # raw is copied out before the slot is looked at
    after = p.direct(x, 0, 0, 1.0, beam_slot=1, min_beam=0.6, raw=raw2).copy()
    assert np.isfinite(before).all() and np.isfinite(raw0).all()
    assert np.array_equal(after, before) and np.array_equal(raw2, raw0)


def test_psfconv_apply_unbound_psf_slot(psfconv):
    p, x = psfconv
    before = p.apply(x, 0, beam_slot=1, scale=0.5, eta=0.1).copy()
    with pytest.raises(ValueError, match="psfhat slot 5 is not bound"):
        p.apply(x, 5, beam_slot=1, scale=0.5, eta=0.1)
    after = p.apply(x, 0, beam_slot=1, scale=0.5, eta=0.1).copy()
    assert np.isfinite(before).all() and np.abs(before).max() > 0.0
    assert np.array_equal(after, before)


def test_comps_render_region_not_bound():
    from pfb_imaging_amd.comps import Comps

    rng = np.random.default_rng(5)
    pix = rng.choice(NX * NY, size=40, replace=False)
    comps = Comps(NX, NY, pix // NY, pix % NY, rng.standard_normal((3, pix.size)))
    b = np.array([1.0, -0.5, 0.25])
    try:
        before = comps.render(b).copy()
        with pytest.raises(ValueError, match="no region mask bound: call pfbhip_comps_set_region first"):
            comps.render(b, region=True)
        after = comps.render(b).copy()
    finally:
        comps.close()
    assert np.count_nonzero(before) == pix.size
    assert np.array_equal(after, before)


# ---- the gridder: refusals that come after the entry has enqueued uploads, and the profile it keeps per handle ----------------
ETA_H, ETA_CG, ETA_PM = 0.05, 0.5, 0.1


@pytest.fixture(scope="module")
def small():
    """The case, its CPU restatement (run with the plan's own kernel and plane choice) and every reference, computed once."""
    c = make(nrow=900, npix=32, widen=20.0)
    g, kw, mask = gpu_plan(c)
    o = oracle_plan(c, g, kw, mask)
    g.close()
    wsum = c["wgt"][mask != 0].sum()
    rng = np.random.default_rng(3)

    def hess(z, eta, beam=1.0):
        return o.vis2dirty(o.dirty2vis(z * beam), c["wgt"]) / wsum * beam + eta * z

    # (float32-representable image and beam: the float64 and the float32 entry then see the same numbers)
    x = c["x"].astype(np.float32).astype(np.float64)
    beam = (0.5 + rng.random((c["nx"], c["ny"]))).astype(np.float32).astype(np.float64)
    b0 = rng.standard_normal((c["nx"], c["ny"]))
    rhs = hess(c["x"], ETA_CG)
    return dict(c=c, wsum=wsum, x=x, beam=beam, b0=b0, rhs=rhs, hessian=hess(x, ETA_H, beam),
                dirty=o.vis2dirty(c["vis"], c["wgt"]),
                dirty_dft=dft.dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], mask, c["nx"], c["ny"], c["cell"], c["cell"],
                                            0.0, 0.0, False, True, False, True, False),
                cg=pcg(lambda z: hess(z, ETA_CG), rhs, tol=1e-9, maxit=200, minit=1),
                pm=pm_oracle(lambda z: hess(z, ETA_PM), b0.shape, b0.copy(), tol=0.0, maxit=6))


@pytest.fixture()
def gridder(small):
    g = gpu_plan(small["c"])[0]
    yield g
    g.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gridder_hessian_before_set_weights(small, gridder, dtype):
    """The refusal comes from apply_op, after the entry has queued the uploads of x and beam."""
    x, beam = small["x"].astype(dtype), small["beam"].astype(dtype)
    with pytest.raises(ValueError, match="call pfbhip_gridder_set_weights before the Hessian"):
        gridder.hessian(x, beam=beam, eta=ETA_H, wsum=small["wsum"])
    gridder.set_weights(small["c"]["wgt"])
    got = gridder.hessian(x, beam=beam, eta=ETA_H, wsum=small["wsum"])
    err = rel(got, small["hessian"])
    print(f"hessian {np.dtype(dtype).name}: rel-l2 vs restatement = {err:.3e}")
    assert got.dtype == dtype
    assert err < 1e-10 + (2.0 ** -24 if dtype is np.float32 else 0.0)


def test_gridder_solvers_before_set_weights(small, gridder):
    c, wsum = small["c"], small["wsum"]
    with pytest.raises(ValueError, match="call pfbhip_gridder_set_weights before the CG solve"):
        gridder.cg(small["rhs"], eta=ETA_CG, wsum=wsum, tol=1e-9, maxit=200, minit=1)
    with pytest.raises(ValueError, match="call pfbhip_gridder_set_weights before the power method"):
        gridder.power_method(small["b0"], eta=ETA_PM, wsum=wsum, tol=0.0, maxit=6)
    fresh = gpu_plan(c)[0]  # a handle that was never refused
    try:
        runs = []
        for g in (gridder, fresh):
            g.set_weights(c["wgt"])
            sol = g.cg(small["rhs"], eta=ETA_CG, wsum=wsum, tol=1e-9, maxit=200, minit=1)
            runs.append((sol, g.last_cg))
    finally:
        fresh.close()
    (sol, info), (sol_fresh, info_fresh) = runs
    print(f"cg: {info}, fresh handle {info_fresh}; rel-l2 vs pcg restatement = {rel(sol, small['cg']):.3e}, vs x = {rel(sol, c['x']):.3e}")
    assert (info["status"], info["iters"]) == (info_fresh["status"], info_fresh["iters"]) and info["status"] == 0
    assert rel(sol, small["cg"]) < 1e-6 and rel(sol, c["x"]) < 1e-6
    assert rel(sol_fresh, small["cg"]) < 1e-6
    rbeta, rb, rk = small["pm"]
    beta, b = gridder.power_method(small["b0"], eta=ETA_PM, wsum=wsum, tol=0.0, maxit=6)
    print(f"power method: beta {beta!r} against {rbeta!r}, vector rel-l2 = {rel(b, rb):.3e}")
    assert gridder.last_pm["iters"] == 6 == rk
    assert abs(beta - rbeta) < 1e-8 * rbeta and rel(b, rb) < 1e-6


def test_gridder_grid_plane_out_of_range(small, gridder):
    c = small["c"]
    with pytest.raises(ValueError, match="out of range"):
        gridder.grid_plane(c["vis"], c["wgt"], gridder.info["nplanes"])
    d = gridder.vis2dirty(c["vis"], c["wgt"])
    print(f"vis2dirty: rel-l2 vs restatement = {rel(d, small['dirty']):.3e}, vs DFT = {rel(d, small['dirty_dft']):.3e}")
    assert rel(d, small["dirty"]) < 1e-10
    assert rel(d, small["dirty_dft"]) < EPS


def test_gridder_profile_round_trip(small, gridder):
    """The stage times and counts live in the handle; the events that feed them are the shared StageTimer's."""
    gridder.set_weights(small["c"]["wgt"])
    gridder.profile(True)
    gridder.hessian(small["x"], eta=ETA_H, wsum=small["wsum"])
    prof = gridder.profile_get(reset=True)
    print(f"profile of one Hessian apply: {prof}, info {gridder.info}")
    assert all(np.isfinite(ms) and ms >= 0.0 and n >= 0 for ms, n in prof.values())
    # the transforms of both halves: one fused kernel per half (fft_mode & 2), else the crop / pad kernels
    grid_side, degrid_side = ("fft_crop", "pad_fft") if gridder.info["fft_mode"] & 2 else ("crop", "pad")
    assert prof["grid"][1] > 0 and prof[grid_side][1] > 0 and prof[degrid_side][1] > 0
    # (one-plane plans may gather inside the scatter's launches: no gather launch of its own then)
    assert prof["degrid"][1] > 0 or gridder.info["wmode"] == 2
    assert all(v == (0.0, 0) for v in gridder.profile_get(reset=True).values())
    gridder.profile(False)
    gridder.hessian(small["x"], eta=ETA_H, wsum=small["wsum"])
    assert all(v == (0.0, 0) for v in gridder.profile_get(reset=True).values())
