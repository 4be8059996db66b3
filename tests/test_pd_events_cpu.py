"""CPU checks of the primal-dual event protocol: the numpy yardstick of tests/_pd_ref.py keeps the semantics of the
reference's loop (opt/primal_dual.py:406-448: event iterations, continuation after False, the ``maxit`` bound) on a
diagonal problem whose steps can be restated by hand, and the C-ABI header declares the new entry points."""

import os
import re

import numpy as np

from tests._pd_ref import DiagPsi, dual_update, pd_ref, reweight_ref, rms_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed=3, nband=2, nx=6, ny=5):
    rng = np.random.default_rng(seed)
    h = 0.5 + rng.random((nband, nx, ny))  # diagonal Hessian
    psi = DiagPsi(nx, ny)
    # the bands share most of their signal: the l21 prox of the reference couples them through the band SUM, and
    # uncorrelated bands keep the loop from settling
    xtilde = rng.standard_normal((1, nx, ny)) + 0.1 * rng.standard_normal((nband, nx, ny))
    hessnorm, nu2 = float(h.max()), sum(c * c for c in psi.c)
    sigma = hessnorm / 2.0 / np.sqrt(nu2)
    tau = 0.98 / (hessnorm / 2.0 + sigma * nu2)
    w = 0.5 + rng.random((psi.nbasis, nx, ny))
    x0 = np.zeros((nband, nx, ny))
    v0 = np.zeros((nband, psi.nbasis, nx, ny))
    return dict(x0=x0, v0=v0, lam=0.05, psi=psi, weight=w, hess=lambda z: h * z, xtilde=xtilde, gamma=1.0, sigma=sigma, tau=tau), h


def _by_hand(p, h, tol, maxit, on_converge=None):
    """The reference loop written out elementwise (no dictionary object): xp / vp copies exactly as primal_dual.py:417-435."""
    c = p["psi"].c
    x, v = p["x0"].copy(), p["v0"].copy()
    xp, vp = x.copy(), v.copy()
    w, fired = p["weight"], []
    k = 0
    for k in range(maxit):
        for b in range(len(c)):
            v[:, b] = c[b] * xp
        v[...] = dual_update(vp, v, p["lam"], p["sigma"], w)
        vp[...] = 2.0 * v - vp
        xout = sum(c[b] * vp[:, b] for b in range(len(c))) - h * (p["xtilde"] - xp) / p["gamma"]
        x[...] = xp - p["tau"] * xout
        eps = float(np.sqrt(((x - xp) ** 2).sum() / max((x**2).sum(), 1e-12))) if x.any() else 1.0
        if eps < tol:
            fired.append(k)
            if on_converge is None:
                break
            stop, w = on_converge(x, k, eps, w)
            if stop:
                break
        np.copyto(xp, x)
        np.copyto(vp, v)
    return x, v, k, fired


def test_yardstick_matches_the_loop_by_hand():
    p, h = _problem()
    x, v, k, eps, events, fired = pd_ref(**p, tol=1e-6, maxit=500)
    xh, vh, kh, fh = _by_hand(p, h, 1e-6, 500)
    assert 0 < k < 499 and k == kh and fired == fh == [k] and events == 1 and eps < 1e-6
    assert np.array_equal(x, xh) and np.array_equal(v, vh)


def test_events_continue_after_false_and_maxit_bounds_the_total():
    p, h = _problem()
    calls = []

    def cb(x, k, eps, w):
        calls.append((k, eps))
        return len(calls) >= 3, 0.5 * w  # a new weight at every event: the loop has to move on, then converge again

    x, v, k, eps, events, fired = pd_ref(**p, tol=1e-4, maxit=2000, on_converge=cb)
    assert events == 3 and fired == [c[0] for c in calls] and k == fired[-1] and all(e < 1e-4 for _, e in calls)
    assert fired[0] < fired[1] < fired[2]
    calls2 = []

    def cb2(x, k, eps, w):
        calls2.append((k, eps))
        return len(calls2) >= 3, 0.5 * w

    xh, vh, kh, fh = _by_hand(p, h, 1e-4, 2000, cb2)
    assert fh == fired and np.array_equal(x, xh) and np.array_equal(v, vh)
    # a callback that never stops and leaves the weight alone: same iterates as a run without events (tol = 0), and
    # maxit bounds the total
    n = fired[0] + 5
    xa, va, ka, ea, eva, fa = pd_ref(**p, tol=1e-4, maxit=n, on_converge=lambda x, k, eps, w: (False, w))
    xb, vb, kb, eb, evb, fb = pd_ref(**p, tol=0.0, maxit=n)
    assert ka == kb == n - 1 and eva >= 1 and evb == 0 and fa[0] == fired[0]
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)


def test_reweighting_reference_formulas():
    rng = np.random.default_rng(0)
    psi = DiagPsi(4, 3, c=(1.0, 0.0))  # the second basis has no nonzero entry: rms stays 1, count 0
    upd = rng.standard_normal((3, 4, 3))
    rms, count = rms_ref(psi, upd)
    assert list(count) == [12, 0] and rms[1] == 1.0 and np.isclose(rms[0], np.std(upd.sum(axis=0)))
    w = reweight_ref(psi, upd, rms, 0.7, 2.0)
    assert np.allclose(w[0], 1.7 / (1 + upd.sum(axis=0) ** 2 / rms[0] ** 2)) and np.all(w[1] == 1.7)


def test_header_declares_the_event_entry_points():
    text = open(os.path.join(ROOT, "include", "pfbhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pfbhip_[a-z0-9_]+)\s*\(", text))
    need = {"pfbhip_pd_create", "pfbhip_pd_run", "pfbhip_pd_set_weight", "pfbhip_pd_set_weight_dev", "pfbhip_pd_get_dual",
            "pfbhip_pd_get_traffic", "pfbhip_pd_iterate_dev", "pfbhip_pd_destroy", "pfbhip_fb_set_weight_dev",
            "pfbhip_fb_iterate_dev", "pfbhip_l21_reweight_dev", "pfbhip_l21_rms_dev", "pfbhip_l21_reweight", "pfbhip_l21_rms"}
    assert need <= declared
    from pfb_imaging_amd import _lib

    assert need <= set(_lib.SYMBOLS)
    # the traffic counters live in a struct of their own: pfbhip_pd_info keeps its layout
    assert [f[0] for f in _lib.PDInfo._fields_] == ["iters", "status", "eps", "loop_ms", "stage_ms", "stage_calls"]
    assert [f[0] for f in _lib.PDTraffic._fields_] == ["events", "h2d_bytes", "d2h_bytes", "norm_bytes"]
