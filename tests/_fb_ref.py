"""A numpy statement of the forward-backward loop (opt/forward_backward.py:95-133 of the reference) over the CPU oracle's
dictionary (oracle/psi.py) and PSF Hessian (oracle/fftconv.py): the yardstick of the device loop in
test_gpu_forward_backward.py.  Coefficients are in the oracle's x-first layout (nband, nbasis, nxmax, nymax)."""

import numpy as np

from oracle import psi as opsi


def prox_l21(alpha, thr):
    """prox of thr * ||.||_{2,1} with the band SUM as the coupling (prox_21m.py:5-26): 0 where the band sum is 0."""
    return opsi.prox_21m(alpha, 1.0, weight=thr)


def prox_l1(alpha, thr):
    return np.sign(alpha) * np.maximum(np.abs(alpha) - thr, 0.0)


def fb_ref(x0, lam, psi, weight, hess, xtilde, g, step, nu, tol, maxit, positivity=0, acceleration=True, l1=False,
           on_converge=None):
    """Returns (x, k, eps, events).  ``psi`` None is the identity; ``hess(z)`` the PSF Hessian; grad(y) = -hess(xtilde - y) / g;
    ``on_converge(x, k, eps, weight) -> (stop, weight)`` models a callback that may replace the weight."""
    xp = np.array(x0, dtype=np.float64)
    y = xp.copy()
    t, eps, k, events = 1.0, 1.0, 0, 0
    prox = prox_l1 if l1 else prox_l21
    for k in range(maxit):
        xg = y + step * hess(xtilde - y) / g
        if psi is None:
            a = xg[:, None]
        else:
            a = np.zeros((xg.shape[0], psi.nbasis, psi.nxmax, psi.nymax))
            psi.dot(xg, a)
        diff = prox(a, step * lam * weight) - a
        if psi is None:
            xo = diff[:, 0]
        else:
            xo = np.zeros_like(xg)
            psi.hdot(diff, xo)
        x = xg + xo / nu
        if positivity == 1:
            x[x < 0.0] = 0.0
        elif positivity == 2:
            x[:, (x <= 0.0).any(axis=0)] = 0.0
        eps = float(np.sqrt(((x - xp) ** 2).sum() / max((x**2).sum(), 1e-12))) if x.any() else 1.0
        if eps < tol:
            events += 1
            if on_converge is None:
                break
            stop, weight = on_converge(x, k, eps, weight)
            if stop:
                break
        if acceleration:
            tp = t
            t = (1.0 + np.sqrt(1.0 + 4.0 * tp * tp)) / 2.0
            y = x + (tp - 1.0) / t * (x - xp)
        else:
            y = x.copy()
        xp = x
    return x, k, eps, events
