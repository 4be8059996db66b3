"""Convergence events of the device-resident primal-dual loop (pfbhip_pd_*): PrimalDual.solve with an ``on_converge``
callback stays on the device, resumes as the reference's loop does (opt/primal_dual.py:430-435), takes reweighted l1 weights
from HBM, and moves only the iterate per event and the dual once across PCIe.  The yardstick is tests/_pd_ref.py over the
CPU oracle's dictionary and PSF Hessians."""

import numpy as np
import pytest

from oracle import fftconv
from oracle import psi as opsi
from tests._pd_ref import pd_ref, reweight_ref, rms_ref

pytestmark = pytest.mark.gpu

rel = lambda a, b: np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)  # noqa: E731

NBAND, NX, NY = 2, 64, 48
BASES, NLEVEL = ("self", "db1", "db2"), 2
# Chosen with the numpy yardstick on the CPU: at tol 1e-3 this problem fires its first event after 24-33 iterations and
# three more within 13, for every positivity mode, and the reweighted iterate differs from the unweighted one by ~1e-2.
# The bands share most of their signal: the reference's l21 prox couples them through the band SUM, and with uncorrelated
# bands the loop does not settle below 1e-3 at all.
TOL, MAXIT, LAM, GAMMA = 1e-3, 200, 0.02, 1.0


def _images(rng):
    common = np.abs(rng.standard_normal((NX, NY))) * (rng.random((NX, NY)) > 0.9)
    model = common[None] * (1.0 + 0.1 * rng.random((NBAND, NX, NY)))
    xtilde = model + 0.3 * rng.standard_normal((1, NX, NY)) + 0.02 * rng.standard_normal(model.shape)
    return model, xtilde, rng.standard_normal(model.shape)


def _problem(kind, use_beam=True, seed=21):
    """(hess, href, hessnorm, model, xtilde, update): HessPSF or a single-process HessTreeRay with two partitions per band."""
    from pfb_imaging_amd.operators.hessian import HessPSF, HessTreeRay

    rng = np.random.default_rng(seed)
    nxp, nyp = 2 * NX, 2 * NY
    if kind == "psf":
        psf = np.zeros((NBAND, nxp, nyp))
        psf[:, 0, 0] = 1.0
        psf += 0.02 * rng.standard_normal(psf.shape)
        abspsf = np.abs(np.fft.rfft2(psf, axes=(1, 2)))
        beam = 0.8 + 0.2 * rng.random((NBAND, NX, NY)) if use_beam else None
        eta = np.linspace(0.05, 0.1, NBAND)
        hess = HessPSF(NX, NY, abspsf, beam=beam, eta=eta)
        href = lambda z: fftconv.hess_psf_dot(z, abspsf, nyp, beam=beam, eta=eta)  # noqa: E731
        hessnorm = float(abspsf.max() * (beam.max() ** 2 if beam is not None else 1.0) + eta.max())
    else:
        parts = []
        for _ in range(NBAND):
            pb = []
            for _ in range(2):
                psf = np.zeros((1, nxp, nyp))
                psf[:, 0, 0] = 1.0
                psf += 0.02 * rng.standard_normal(psf.shape)
                pb.append({"psfhat": np.abs(np.fft.rfft2(psf, axes=(1, 2))), "beam": 0.8 + 0.2 * rng.random((1, NX, NY)),
                           "wsum": np.array([1.0 + rng.random()])})
            parts.append(pb)
        etas = [0.05, 0.1]
        hess = HessTreeRay(parts, NX, NY, nxp, nyp, etas=etas)
        href = lambda z: np.stack([fftconv.hessian_tree_dot(z[b], parts[b], nxp, nyp, eta=etas[b])[0]  # noqa: E731
                                   for b in range(NBAND)])
        # a valid bound on ||H||: sum_p max|psfhat_p| max(beam_p)^2 / sum_p wsum_p + eta
        hessnorm = max(sum(p["psfhat"].max() * p["beam"].max() ** 2 for p in pb) / sum(p["wsum"][0] for p in pb)
                       for pb in parts) + max(etas)
    model, xtilde, update = _images(rng)
    return hess, href, float(hessnorm), model, xtilde, update


def _psi(layout):
    from pfb_imaging_amd.operators.psi import Psi, PsiNocopyt

    return (Psi if layout == "psi" else PsiNocopyt)(NBAND, NX, NY, BASES, NLEVEL, 1)


def _solver(reg, hess, xtilde, hessnorm, positivity, on_converge, generic=False, tol=TOL, maxit=MAXIT):
    from pfb_imaging_amd import prox
    from pfb_imaging_amd.opt import PrimalDual, PsfGrad

    pd = PrimalDual(tol=tol, maxit=maxit, verbosity=0, gamma=GAMMA, primal_prox=prox.positivity_prox(positivity),
                    on_converge=on_converge)
    pd.setup(reg, hessnorm)
    g = PsfGrad(hess, xtilde, GAMMA)
    pd.set_grad((lambda z: g(z)) if generic else g)
    assert (pd._device_path() is None) == generic
    return pd


class _Reweight:
    """ReweightOnConverge (deconv/pfb.py:14-54) restated: update the weights and go on, up to ``maxreweight`` times."""

    def __init__(self, reg, maxreweight):
        self.reg, self.maxreweight, self.calls = reg, maxreweight, []

    def __call__(self, x, k, eps):
        self.calls.append(k)
        if len(self.calls) <= self.maxreweight:
            self.reg.update_weights(x)
            return False
        return True


def test_callback_keeps_the_device_loop():
    """Fails on a build without the feature: ``_device_path()`` is None with a callback and ``last`` has no ``events``."""
    from pfb_imaging_amd.opt import L21

    hess, _, hessnorm, model, xtilde, _ = _problem("psf")
    fired = []

    def cb(x, k, eps):
        fired.append((k, eps))
        return len(fired) > 2

    reg = L21(_psi("nocopyt"), BASES, nu=np.sqrt(len(BASES)))
    pd = _solver(reg, hess, xtilde, hessnorm, 1, cb)
    assert pd._device_path() == 1
    pd.solve(model.copy(), LAM)
    assert len(fired) == 3 and pd.last["events"] == 3 and pd.last["status"] == 0
    assert all(e < TOL for _, e in fired) and fired[-1][0] == pd.last["iters"]


@pytest.mark.parametrize("layout,kind,positivity", [("nocopyt", "psf", 0), ("psi", "psf", 1), ("nocopyt", "psf", 2),
                                                     ("psi", "psf", 2), ("nocopyt", "tree", 1), ("psi", "tree", 0)])
def test_reweighting_run_matches_generic_loop_and_yardstick(layout, kind, positivity):
    from pfb_imaging_amd.opt import L21

    hess, href, hessnorm, model, xtilde, update = _problem(kind, use_beam=positivity != 1)
    psi = _psi(layout)
    nu = float(np.sqrt(len(BASES)))
    res = {}
    for name in ("device", "generic"):
        reg = L21(psi, BASES, nu=nu, rmsfactor=0.5)
        reg.init_reweighting(update)
        rw = _Reweight(reg, 3)
        pd = _solver(reg, hess, xtilde, hessnorm, positivity, rw, generic=name == "generic")
        x = pd.solve(model.copy(), LAM)
        w = reg.l1weight if layout == "nocopyt" else reg.l1weight.transpose(0, 2, 1)
        v = pd._v if layout == "nocopyt" else pd._v.transpose(0, 1, 3, 2)
        res[name] = (x, pd.last["iters"], rw.calls, pd.last["events"], w.copy(), v.copy(), reg._rms_comps.copy())
    # the yardstick: the reference loop over the oracle's dictionary and Hessian, the event rule of ReweightOnConverge
    o = opsi.Psi(NBAND, NX, NY, BASES, NLEVEL)
    rms, _ = rms_ref(o, update)
    calls = []

    def cb(x, k, eps, w):
        calls.append(k)
        return (False, reweight_ref(o, x, rms, 0.5, 2.0)) if len(calls) <= 3 else (True, w)

    v0 = np.zeros((NBAND, o.nbasis, o.nxmax, o.nymax))
    sigma, tau = pd.sigma, pd.tau
    xr, vr, kr, _, events, fired = pd_ref(model, v0, LAM, o, np.ones(v0.shape[1:]), href, xtilde, GAMMA, sigma, tau, TOL, MAXIT,
                                          positivity, cb)
    wr = reweight_ref(o, np.asarray(_event_iterate(model, v0, o, href, xtilde, sigma, tau, positivity, rms, 3)), rms, 0.5, 2.0)
    # condition: the problem fires at least 3 events before maxit and the weights matter
    assert events == 4 and kr < MAXIT - 1
    x0, _, _, _, _, _ = pd_ref(model, v0, LAM, o, np.ones(v0.shape[1:]), href, xtilde, GAMMA, sigma, tau, TOL, MAXIT, positivity)
    assert rel(xr, x0) > 1e-6
    for name, xtol in (("device", 1e-9), ("generic", 1e-7)):
        x, iters, fired_k, ev, w, v, rms_got = res[name]
        print(name, "x", rel(x, xr), "w", rel(w, wr), "v", rel(v, vr), "rms", rel(rms_got, rms))
        assert iters == kr and fired_k == fired and ev == events
        assert rel(rms_got, rms) < 1e-12
        assert rel(x, xr) < xtol
        assert rel(w, wr) < 1e-9
        assert rel(v, vr) < 1e-6
    assert rel(res["device"][0], res["generic"][0]) < 1e-7


def _event_iterate(model, v0, o, href, xtilde, sigma, tau, positivity, rms, n):
    """The yardstick's iterate at its n-th event (the one the last weight update saw)."""
    seen = []

    def cb(x, k, eps, w):
        seen.append(x.copy())
        return (False, reweight_ref(o, x, rms, 0.5, 2.0)) if len(seen) < n else (True, w)

    pd_ref(model, v0, LAM, o, np.ones(v0.shape[1:]), href, xtilde, GAMMA, sigma, tau, TOL, MAXIT, positivity, cb)
    return seen[-1]


def test_pcie_accounting():
    from pfb_imaging_amd.opt import L21

    hess, _, hessnorm, model, xtilde, update = _problem("psf")
    psi = _psi("nocopyt")
    nu = float(np.sqrt(len(BASES)))
    # reweighting on the device: the iterate comes down once per run, the dual once, nothing goes up
    reg = L21(psi, BASES, nu=nu, rmsfactor=0.5)
    reg.init_reweighting(update)
    rw = _Reweight(reg, 3)
    pd = _solver(reg, hess, xtilde, hessnorm, 1, rw)
    x = pd.solve(model.copy(), LAM)
    last = pd.last
    assert last["events"] == 4 and last["status"] == 0
    assert last["h2d_bytes"] == 0
    assert last["d2h_bytes"] == last["events"] * x.nbytes + pd._v.nbytes  # (the final x is the last event's)
    assert last["norm_bytes"] == (last["iters"] + 1) * 3 * 1024 * 8
    assert reg._l1weight is None and reg._wdev is not None  # the weights never left HBM
    # (h2d_bytes counts the image uploads of update_weights too: 0 means the lent device iterate was read.)  A callback
    # that hands update_weights a COPY of the iterate uploads one image cube per reweighting
    reg = L21(psi, BASES, nu=nu, rmsfactor=0.5)
    reg.init_reweighting(update)
    calls = []

    def copying(x, k, eps):
        calls.append(k)
        if len(calls) <= 3:
            reg.update_weights(x.copy())
            return False
        return True

    pd2 = _solver(reg, hess, xtilde, hessnorm, 1, copying)
    x2 = pd2.solve(model.copy(), LAM)
    assert pd2.last["events"] == 4 and pd2.last["h2d_bytes"] == 3 * x2.nbytes
    assert np.array_equal(x2, x) and calls == rw.calls  # the same solve either way
    # a callback that assigns host weights and never stops: one upload per event, and one more download for the
    # iterate of the run that ended on maxit
    reg = L21(psi, BASES, nu=nu)
    rng = np.random.default_rng(1)

    def cb(x, k, eps):
        reg.l1weight = 0.5 + rng.random(reg.l1weight.shape)
        return False

    pd = _solver(reg, hess, xtilde, hessnorm, 1, cb, maxit=60)
    x = pd.solve(model.copy(), LAM)
    last = pd.last
    # maxit is reached between two events here (the yardstick fires its last event at iteration 58)
    assert last["events"] >= 2 and last["status"] == 1 and last["iters"] == 59
    assert last["h2d_bytes"] == last["events"] * reg.l1weight.nbytes
    assert last["d2h_bytes"] == (last["events"] + 1) * x.nbytes + pd._v.nbytes


@pytest.mark.parametrize("positivity", [0, 2])
def test_stopping_and_resuming_changes_nothing(positivity):
    """Run A stops at every event (callback returns False, weights untouched), run B never stops (tol = 0); a solve without
    a callback (pfbhip_primal_dual) runs the same kernels in the same order."""
    from pfb_imaging_amd.opt import L21

    hess, _, hessnorm, model, xtilde, _ = _problem("psf")
    psi = _psi("nocopyt")
    rng = np.random.default_rng(2)
    w = 0.5 + rng.random((len(BASES), psi.nxmax, psi.nymax))
    n = 45
    out = {}
    for name, tol, cb in (("a", TOL, lambda x, k, eps: False), ("b", 0.0, lambda x, k, eps: False), ("c", 0.0, None)):
        reg = L21(psi, BASES, nu=float(np.sqrt(len(BASES))))
        reg.l1weight = w
        pd = _solver(reg, hess, xtilde, hessnorm, positivity, cb, tol=tol, maxit=n)
        out[name] = (pd.solve(model.copy(), LAM), pd._v.copy(), dict(pd.last))
    assert out["a"][2]["events"] >= 3 and out["b"][2]["events"] == 0
    for name in ("a", "b", "c"):
        assert out[name][2]["iters"] == n - 1
    assert np.array_equal(out["a"][0], out["b"][0]) and np.array_equal(out["a"][1], out["b"][1])
    assert np.array_equal(out["c"][0], out["b"][0]) and np.array_equal(out["c"][1], out["b"][1])
    assert out["b"][2]["status"] == 1  # (maxit reached BETWEEN events: test_pcie_accounting's second run)


def test_warm_start_and_second_solve():
    """The dual comes back as warm-start state and a weight left in HBM by the previous solve's last update is used by the
    next solve without a download: two solves in a row equal the generic loop's two solves."""
    from pfb_imaging_amd.opt import L21

    hess, _, hessnorm, model, xtilde, update = _problem("psf")
    psi = _psi("psi")
    res = {}
    for name in ("device", "generic"):
        reg = L21(psi, BASES, nu=float(np.sqrt(len(BASES))), rmsfactor=0.5)
        reg.init_reweighting(update)
        rw = _Reweight(reg, 1)
        pd = _solver(reg, hess, xtilde, hessnorm, 1, rw, generic=name == "generic")
        x1 = pd.solve(model.copy(), LAM).copy()
        rw.calls.clear()
        x2 = pd.solve(x1.copy(), LAM)
        res[name] = (x1, x2, pd.last["iters"], pd._v.copy())
    assert res["device"][2] == res["generic"][2]
    assert rel(res["device"][0], res["generic"][0]) < 1e-7 and rel(res["device"][1], res["generic"][1]) < 1e-7
    assert rel(res["device"][3], res["generic"][3]) < 1e-6
