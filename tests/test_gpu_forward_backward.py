"""The forward-backward backward solver (opt/forward_backward.py of the reference) on the GPU: the reference's analytic
lasso through both paths, the device loop against a numpy statement of the loop over the CPU oracle (tests/_fb_ref.py)
and against the generic path, convergence events with weight updates, the make_ista / make_sara compositions
(deconv/presets.py:81-144) and the fallbacks of the kernels."""

import numpy as np
import pytest

from oracle import fftconv
from oracle import psi as opsi
from tests._fb_ref import fb_ref

pytestmark = pytest.mark.gpu

rel = lambda a, b: np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)  # noqa: E731


def _psf_problem(nband, nx, ny, seed, use_beam=False, eta=None):
    from pfb_imaging_amd.operators.hessian import HessPSF

    rng = np.random.default_rng(seed)
    nyp = 2 * ny
    psf = np.zeros((nband, 2 * nx, nyp))
    psf[:, 0, 0] = 1.0
    psf += 0.02 * rng.standard_normal(psf.shape)
    abspsf = np.abs(np.fft.rfft2(psf, axes=(1, 2)))
    beam = 0.8 + 0.2 * rng.random((nband, nx, ny)) if use_beam else None
    eta = np.linspace(0.05, 0.1, nband) if eta is None else eta
    hess = HessPSF(nx, ny, abspsf, beam=beam, eta=eta)
    href = lambda z: fftconv.hess_psf_dot(z, abspsf, nyp, beam=beam, eta=eta)  # noqa: E731
    hessnorm = float(abspsf.max() * (beam.max() ** 2 if beam is not None else 1.0) + np.max(eta))
    model = np.abs(rng.standard_normal((nband, nx, ny))) * (rng.random((nband, nx, ny)) > 0.9)
    xtilde = model + 0.3 * rng.standard_normal(model.shape)
    return hess, href, hessnorm, model, xtilde, rng


def _solve(reg, grad, hessnorm, x0, lam, generic=False, **kw):
    from pfb_imaging_amd.opt import ForwardBackward

    kw.setdefault("verbosity", 0)
    fb = ForwardBackward(**kw)
    fb.setup(reg, hessnorm)
    fb.set_grad((lambda z: grad(z)) if generic else grad)
    dev = fb._device_path()
    assert (dev is None) == generic
    return fb.solve(np.array(x0), lam), fb


@pytest.mark.parametrize("acceleration", [True, False])
@pytest.mark.parametrize("lam", [0.1, 1.0])
def test_lasso_analytic(acceleration, lam):
    """min 1/2 ||x - b||^2 + lam ||x||_1 = soft threshold of b (the reference's analytic lasso), generic and device."""
    from pfb_imaging_amd.operators.hessian import HessPSF
    from pfb_imaging_amd.operators.psi import IdentityPsi
    from pfb_imaging_amd.opt import L1, PsfGrad

    nband, nx, ny = 2, 48, 40
    b = np.random.default_rng(11).standard_normal((nband, nx, ny))
    expect = np.sign(b) * np.maximum(np.abs(b) - lam, 0.0)
    kw = dict(tol=1e-10, maxit=500, gamma=0.45, acceleration=acceleration)
    x, _ = _solve(L1(IdentityPsi(nband, nx, ny)), lambda z: z - b, 1.0, np.zeros_like(b), lam, generic=True, **kw)
    assert np.abs(x - expect).max() < 1e-4
    psf = np.zeros((nband, 2 * nx, 2 * ny))
    psf[:, 0, 0] = 1.0  # delta PSF and eta = 0: H = I
    hess = HessPSF(nx, ny, np.abs(np.fft.rfft2(psf, axes=(1, 2))), eta=0.0)
    x, fb = _solve(L1(IdentityPsi(nband, nx, ny)), PsfGrad(hess, b, 1.0), 1.0, np.zeros_like(b), lam, **kw)
    assert np.abs(x - expect).max() < 1e-4
    assert fb.last["status"] == 0


@pytest.mark.parametrize("acceleration", [True, False])
@pytest.mark.parametrize("use_beam", [True, False])
@pytest.mark.parametrize("positivity", [0, 1, 2])
@pytest.mark.parametrize("layout", ["psi", "nocopyt"])
def test_device_loop_matches_reference(layout, positivity, use_beam, acceleration):
    from pfb_imaging_amd import prox
    from pfb_imaging_amd.operators.psi import Psi, PsiNocopyt
    from pfb_imaging_amd.opt import L21, PsfGrad

    nband, nx, ny = 2, 64, 48
    bases, nlevel = ("self", "db1", "db2"), 2
    hess, href, hessnorm, model, xtilde, rng = _psf_problem(nband, nx, ny, 21, use_beam)
    psi = (Psi if layout == "psi" else PsiNocopyt)(nband, nx, ny, bases, nlevel, 1)
    reg = L21(psi, bases, nu=float(len(bases)))
    reg.l1weight = 0.5 + rng.random(reg.l1weight.shape)
    lam, gamma = 0.02, 0.45
    # 15 iterations: under the positivity clamp this problem amplifies rounding differences ~1e3-fold by iteration 20 and
    # ~1e7-fold by iteration 40 (perturbing the oracle's own Hessian by 1e-15 shows it), which would swamp the comparison
    kw = dict(tol=1e-6, maxit=15, gamma=gamma, acceleration=acceleration, primal_prox=prox.positivity_prox(positivity))
    got, fb = _solve(reg, PsfGrad(hess, xtilde, 1.0), hessnorm, model, lam, **kw)
    o = opsi.Psi(nband, nx, ny, bases, nlevel)
    w = reg.l1weight if layout == "nocopyt" else reg.l1weight.transpose(0, 2, 1)
    xr, kr, er, _ = fb_ref(model, lam, o, w, href, xtilde, 1.0, fb.step, reg.nu, 1e-6, 15, positivity, acceleration)
    assert fb.last["iters"] == kr
    assert rel(got, xr) < 1e-9
    got2, fb2 = _solve(reg, PsfGrad(hess, xtilde, 1.0), hessnorm, model, lam, generic=True, **kw)
    assert fb2.last["iters"] == kr and rel(got, got2) < 1e-7


def test_generic_tight_frame_matches_handcoded_l21():
    from pfb_imaging_amd.operators.psi import Psi
    from pfb_imaging_amd.opt import L21, ForwardBackward
    from pfb_imaging_amd.prox import prox_21m_numba

    nband, nx, ny, bases = 3, 40, 56, ("self", "db1", "db4")
    rng = np.random.default_rng(9)
    psi = Psi(nband, nx, ny, bases, 2, 1)
    reg = L21(psi, bases, nu=2.5)
    reg.l1weight = 0.5 + rng.random(reg.l1weight.shape)
    fb = ForwardBackward(gamma=0.8, verbosity=0)
    fb.setup(reg, 1.3)
    x = rng.standard_normal((nband, nx, ny))
    lam = 0.3
    got = fb._apply_prox(x.copy(), lam)
    alpha = np.zeros(reg.coeff_shape())
    psi.dot(x, alpha)
    out = np.zeros_like(alpha)
    prox_21m_numba(alpha, out, fb.step * lam, sigma=1.0, weight=reg.l1weight)
    xo = np.zeros_like(x)
    psi.hdot(out - alpha, xo)
    assert rel(got, x + xo / 2.5) < 1e-13


class _Reweight:
    """ReweightOnConverge (deconv/pfb.py:14-60) restated: update the weights and go on, up to ``maxreweight`` times."""

    def __init__(self, reg, maxreweight):
        self.reg, self.maxreweight, self.calls = reg, maxreweight, []

    def __call__(self, x, k, eps):
        self.calls.append(k)
        if len(self.calls) <= self.maxreweight:
            self.reg.update_weights(x)
            return False
        return True


def test_on_converge_on_device():
    from pfb_imaging_amd.operators.psi import PsiNocopyt
    from pfb_imaging_amd.opt import L21, PsfGrad

    nband, nx, ny = 2, 64, 48
    bases = ("self", "db1", "db2")
    hess, href, hessnorm, model, xtilde, rng = _psf_problem(nband, nx, ny, 4)
    psi = PsiNocopyt(nband, nx, ny, bases, 2, 1)
    # ISTA: with FISTA momentum these small problems keep eps above 1e-4 for hundreds of iterations
    kw = dict(tol=1e-4, maxit=300, gamma=0.45, acceleration=False)
    fired = []

    def cb(x, k, eps):
        fired.append((k, eps))
        return len(fired) > 2

    reg = L21(psi, bases, nu=3.0)
    _, fb = _solve(reg, PsfGrad(hess, xtilde, 1.0), hessnorm, model, 0.02, on_converge=cb, **kw)
    assert len(fired) == 3 and fb.last["events"] == 3 and fb.last["status"] == 0
    assert all(e < 1e-4 for _, e in fired) and fired[-1][0] == fb.last["iters"]
    res = {}
    update = rng.standard_normal(model.shape)
    for name in ("device", "generic"):
        reg = L21(psi, bases, nu=3.0, rmsfactor=0.5)
        reg.init_reweighting(update)
        rw = _Reweight(reg, 2)
        x, fb = _solve(reg, PsfGrad(hess, xtilde, 1.0), hessnorm, model, 0.02, generic=name == "generic", on_converge=rw, **kw)
        res[name] = (x, fb.last["iters"], rw.calls, fb.last["events"], reg.l1weight.copy())
    assert res["device"][1] == res["generic"][1] and res["device"][2] == res["generic"][2]
    assert res["device"][3] == res["generic"][3] == 3
    assert rel(res["device"][0], res["generic"][0]) < 1e-9 and rel(res["device"][4], res["generic"][4]) < 1e-9
    # the weights were re-uploaded: without the update the solve takes another course
    reg = L21(psi, bases, nu=3.0)
    x0, _ = _solve(reg, PsfGrad(hess, xtilde, 1.0), hessnorm, model, 0.02, **kw)
    assert rel(res["device"][0], x0) > 1e-6


def _tree_parts(nband, nx, ny, rng, nparts=2):
    nxp, nyp = 2 * nx, 2 * ny
    parts = []
    for _ in range(nband):
        pb = []
        for _ in range(nparts):
            psf = np.zeros((1, nxp, nyp))
            psf[:, 0, 0] = 1.0
            psf += 0.02 * rng.standard_normal(psf.shape)
            pb.append({"psfhat": np.abs(np.fft.rfft2(psf, axes=(1, 2))), "beam": 0.8 + 0.2 * rng.random((1, nx, ny)),
                       "wsum": np.array([1.0 + rng.random()])})
        parts.append(pb)
    # a valid bound on ||H||: sum_p max|psfhat_p| max(beam_p)^2 / sum_p wsum_p (+ eta, added by the caller)
    bound = max(sum(p["psfhat"].max() * p["beam"].max() ** 2 for p in pb) / sum(p["wsum"][0] for p in pb) for pb in parts)
    return parts, nxp, nyp, float(bound)


def test_make_ista_composition():
    """L1(IdentityPsi) + HessTreeRay (two partitions per band) + ISTA + positivity: the ista preset."""
    from pfb_imaging_amd import prox
    from pfb_imaging_amd.operators.hessian import HessTreeRay
    from pfb_imaging_amd.operators.psi import IdentityPsi
    from pfb_imaging_amd.opt import L1, PsfGrad

    nband, nx, ny = 3, 48, 40
    rng = np.random.default_rng(5)
    parts, nxp, nyp, bound = _tree_parts(nband, nx, ny, rng)
    hess = HessTreeRay(parts, nx, ny, nxp, nyp, etas=[0.05, 0.1, 0.02])
    model = np.abs(rng.standard_normal((nband, nx, ny))) * (rng.random((nband, nx, ny)) > 0.8)
    xtilde = model + 0.3 * rng.standard_normal(model.shape)
    reg = L1(IdentityPsi(nband, nx, ny))
    reg.weight = 0.5 + rng.random(reg.weight.shape)
    kw = dict(tol=1e-7, maxit=25, gamma=0.45, acceleration=False, primal_prox=prox.positivity)
    g = PsfGrad(hess, xtilde, 1.0)
    xd, fbd = _solve(reg, g, bound + 0.1, model, 0.01, **kw)
    xg, fbg = _solve(reg, g, bound + 0.1, model, 0.01, generic=True, **kw)
    assert fbd.last["iters"] == fbg.last["iters"] and rel(xd, xg) < 1e-9


def test_make_sara_fb_composition():
    """L21(PsiNocopytRay) over a single-process BandWorkerPool + HessTreeRay on the same pool + the reweighting callback."""
    from pfb_imaging_amd.operators.band_worker import BandWorkerPool
    from pfb_imaging_amd.operators.hessian import HessTreeRay
    from pfb_imaging_amd.operators.psi import PsiNocopytRay
    from pfb_imaging_amd.opt import L21, PsfGrad

    nband, nx, ny = 2, 48, 64
    bases = ("self", "db1", "db3")
    rng = np.random.default_rng(8)
    parts, nxp, nyp, bound = _tree_parts(nband, nx, ny, rng)
    pool = BandWorkerPool(nband)
    hess = HessTreeRay(parts, nx, ny, nxp, nyp, etas=0.05, workers=pool)
    psi = PsiNocopytRay(nband, nx, ny, bases, 2, 1, workers=pool)
    model = np.abs(rng.standard_normal((nband, nx, ny))) * (rng.random((nband, nx, ny)) > 0.8)
    xtilde = model + 0.3 * rng.standard_normal(model.shape)
    update = rng.standard_normal(model.shape)
    res = {}
    for name in ("device", "generic"):
        reg = L21(psi, bases, nu=float(len(bases)), rmsfactor=0.5)
        reg.init_reweighting(update)
        rw = _Reweight(reg, 2)
        # no primal prox: on this problem a positivity clamp after the (not exactly tight) wavelet prox keeps eps above tol
        kw = dict(tol=1e-4, maxit=300, gamma=0.45, acceleration=False, on_converge=rw)
        x, fb = _solve(reg, PsfGrad(hess, xtilde, 1.0), bound + 0.05, model, 0.02, generic=name == "generic", **kw)
        res[name] = (x, fb.last["iters"], rw.calls)
    assert res["device"][1] == res["generic"][1] and res["device"][2] == res["generic"][2] and len(res["device"][2]) == 3
    assert rel(res["device"][0], res["generic"][0]) < 1e-9
    pool.close()


def test_l1_over_wavelets_and_nu():
    from pfb_imaging_amd.operators.psi import Psi
    from pfb_imaging_amd.opt import L1, PsfGrad

    nband, nx, ny = 2, 64, 64
    bases = ("self", "db2")
    hess, href, hessnorm, model, xtilde, rng = _psf_problem(nband, nx, ny, 13)
    psi = Psi(nband, nx, ny, bases, 2, 1)
    reg = L1(psi, nu=1.7)
    reg.weight = 0.5 + rng.random(reg.weight.shape)
    kw = dict(tol=1e-7, maxit=30, gamma=0.45)
    xd, fb = _solve(reg, PsfGrad(hess, xtilde, 1.0), hessnorm, model, 0.01, **kw)
    o = opsi.Psi(nband, nx, ny, bases, 2)
    xr, kr, _, _ = fb_ref(model, 0.01, o, reg.weight.transpose(0, 2, 1), href, xtilde, 1.0, fb.step, 1.7, 1e-7, 30, l1=True)
    assert fb.last["iters"] == kr and rel(xd, xr) < 1e-9
    xg, fbg = _solve(reg, PsfGrad(hess, xtilde, 1.0), hessnorm, model, 0.01, generic=True, **kw)
    assert fbg.last["iters"] == kr and rel(xd, xg) < 1e-7


@pytest.mark.parametrize("identity", [False, True])
def test_many_bands_fallback(identity):
    """nband = 18 > 16: the two-pass shrink, the positivity-2 fallback of the step and the identity's unfused path."""
    from pfb_imaging_amd import prox
    from pfb_imaging_amd.operators.psi import IdentityPsi, PsiNocopyt
    from pfb_imaging_amd.opt import L21, PsfGrad

    nband, nx, ny = 18, 32, 40
    bases = ("self", "db1")
    hess, href, hessnorm, model, xtilde, rng = _psf_problem(nband, nx, ny, 3)
    model = np.abs(model) + 0.05  # keep pixels alive under positivity 2 across 18 bands
    xtilde = model + 0.02 * rng.standard_normal(model.shape)
    psi = IdentityPsi(nband, nx, ny) if identity else PsiNocopyt(nband, nx, ny, bases, 2, 1)
    reg = L21(psi, ("self",) if identity else bases, nu=1.0 if identity else 2.0)
    reg.l1weight = 0.5 + rng.random(reg.l1weight.shape)
    # positivity 2 over 18 bands zeroes every pixel of the identity problem: the identity case clamps per pixel instead
    kw = dict(tol=1e-8, maxit=25, gamma=0.45, primal_prox=prox.positivity if identity else prox.positivity_band)
    xd, fb = _solve(reg, PsfGrad(hess, xtilde, 1.0), hessnorm, model, 0.01, **kw)
    o = None if identity else opsi.Psi(nband, nx, ny, bases, 2)
    w = reg.l1weight[0] if identity else reg.l1weight
    xr, kr, _, _ = fb_ref(model, 0.01, o, w, href, xtilde, 1.0, fb.step, reg.nu, 1e-8, 25, 1 if identity else 2)
    assert fb.last["iters"] == kr and rel(xd, xr) < 1e-9
    assert np.count_nonzero(xd) > 0


def test_zero_start_maxit_and_stages():
    """x = xtilde = 0 stays 0: eps = 1 every iteration, the loop ends at maxit (status 1, iters maxit - 1); the stage
    clocks of a short run count every launch."""
    from pfb_imaging_amd.operators.psi import PsiNocopyt
    from pfb_imaging_amd.opt import L21, PsfGrad

    nband, nx, ny = 2, 32, 48
    bases = ("self", "db1")
    hess, *_ = _psf_problem(nband, nx, ny, 1)
    psi = PsiNocopyt(nband, nx, ny, bases, 2, 1)
    reg = L21(psi, bases, nu=2.0)
    zero = np.zeros((nband, nx, ny))
    x, fb = _solve(reg, PsfGrad(hess, zero, 1.0), 1.2, zero, 0.1, tol=1e-5, maxit=7, gamma=0.45)
    assert not x.any()
    assert fb.last["status"] == 1 and fb.last["iters"] == 6 and fb.last["eps"] == 1.0 and fb.last["events"] == 0
    st = fb.last["stages"]
    assert st["forward_hessian"][1] == 7 * nband and st["shrink"][1] == 7 and st["step"][1] == 7
    assert st["psi_analysis"][1] == 7 and st["psi_synthesis"][1] == 7
    assert all(ms >= 0.0 for ms, _ in st.values())
    # a converging run from a non-zero start: fewer iterations than maxit, status 0
    hess2, _, hn, model, xtilde, _ = _psf_problem(nband, nx, ny, 2)
    _, fb = _solve(reg, PsfGrad(hess2, xtilde, 1.0), hn, model, 0.02, tol=1e-3, maxit=300, gamma=0.45, acceleration=False)
    assert fb.last["status"] == 0 and fb.last["iters"] < 299 and fb.last["eps"] < 1e-3


def test_device_matches_generic_at_size():
    """4 bands of 2048^2, L21 over self,db1,db2,db3 (3 levels), 10 iterations."""
    from pfb_imaging_amd import prox
    from pfb_imaging_amd.operators.hessian import HessPSF
    from pfb_imaging_amd.operators.psi import PsiNocopyt
    from pfb_imaging_amd.opt import L21, PsfGrad

    nband, nx = 4, 2048
    bases = ("self", "db1", "db2", "db3")
    rng = np.random.default_rng(0)
    abspsf = 1.0 + 0.1 * np.abs(rng.standard_normal((nband, 2 * nx, nx + 1)))
    hess = HessPSF(nx, nx, abspsf, beam=None, eta=0.01)
    psi = PsiNocopyt(nband, nx, nx, bases, 3, 1)
    reg = L21(psi, bases, nu=float(len(bases)))
    model = np.abs(rng.standard_normal((nband, nx, nx))) * (rng.random((nband, nx, nx)) > 0.99)
    xtilde = model + 0.1 * rng.standard_normal(model.shape)
    kw = dict(tol=0.0, maxit=10, gamma=0.45, primal_prox=prox.positivity)
    hn = float(abspsf.max() + 0.01)
    xd, fbd = _solve(reg, PsfGrad(hess, xtilde, 1.0), hn, model, 1e-3, **kw)
    xg, fbg = _solve(reg, PsfGrad(hess, xtilde, 1.0), hn, model, 1e-3, generic=True, **kw)
    assert fbd.last["iters"] == fbg.last["iters"] == 9
    assert rel(xd, xg) < 1e-9
