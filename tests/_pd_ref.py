"""A numpy statement of the primal-dual loop with convergence events (opt/primal_dual.py:406-448 of the reference; the
event rule is :430-435) and of the l1 reweighting (prox/l21.py:52-88, utils/misc.py:742-755): the yardstick of the device
loop in test_gpu_pd_events.py.  ``psi`` is any dictionary with ``dot(x, out)`` / ``hdot(alpha, out)`` and ``nbasis``,
``nxmax``, ``nymax`` (the CPU oracle's, in its x-first layout (nband, nbasis, nxmax, nymax)); ``hess(z)`` the Hessian."""

import numpy as np


def dual_update(vp, v, lam, sigma, weight):
    """dual_update_numba_fast (prox_21m.py:105-135): vtilde * min(1, lam w / |sum_band vtilde|), vtilde = vp + sigma v."""
    vt = vp + sigma * v
    s = np.abs(vt.sum(axis=0))
    thr = lam * weight
    return vt * np.where(s > thr, thr / np.where(s > 0, s, 1.0), 1.0)[None]


def pd_ref(x0, v0, lam, psi, weight, hess, xtilde, gamma, sigma, tau, tol, maxit, positivity=0, on_converge=None):
    """Returns (x, v, k, eps, events, fired): ``events`` counts the iterations with eps < tol, ``fired`` lists them.
    ``on_converge(x, k, eps, weight) -> (stop, weight)`` models a callback that may replace the weight; when it does not
    stop, the loop goes on as after any other iteration (xp <- x, vp <- v) and ``maxit`` bounds the total."""
    xp, vp = np.array(x0, dtype=np.float64), np.array(v0, dtype=np.float64)
    x, v = xp.copy(), vp.copy()
    eps, k, events, fired = 1.0, 0, 0, []
    for k in range(maxit):
        v = np.zeros_like(vp)
        psi.dot(xp, v)
        v = dual_update(vp, v, lam, sigma, weight)
        xout = np.zeros_like(xp)
        psi.hdot(2.0 * v - vp, xout)
        xout = xout - hess(xtilde - xp) / gamma
        x = xp - tau * xout
        if positivity == 1:
            x[x < 0.0] = 0.0
        elif positivity == 2:
            x[:, (x <= 0.0).any(axis=0)] = 0.0
        eps = float(np.sqrt(((x - xp) ** 2).sum() / max((x**2).sum(), 1e-12))) if x.any() else 1.0
        if eps < tol:
            events += 1
            fired.append(k)
            if on_converge is None:
                break
            stop, weight = on_converge(x, k, eps, weight)
            if stop:
                break
        xp, vp = x, v
    return x, v, k, eps, events, fired


def band_sum(psi, x):
    a = np.zeros((x.shape[0], psi.nbasis, psi.nxmax, psi.nymax))
    psi.dot(x, a)
    return np.sum(a, axis=0)


def rms_ref(psi, update):
    """(rms, count) per basis: np.std of the nonzero band sums, 1 where there is none (l21.py:56-65)."""
    s = band_sum(psi, update)
    rms, count = np.ones(psi.nbasis), np.zeros(psi.nbasis, dtype=np.int64)
    for i in range(psi.nbasis):
        nz = s[i][s[i] != 0]
        count[i] = nz.size
        if nz.size:
            rms[i] = np.std(nz)
    return rms, count


def reweight_ref(psi, x, rms, rmsfactor, alpha):
    """(1 + rmsfactor) / (1 + |sum_band Psi^T x|^alpha / rms^alpha) (misc.py:742-755)."""
    return (1 + rmsfactor) / (1 + np.abs(band_sum(psi, x)) ** alpha / rms[:, None, None] ** alpha)


class DiagPsi:
    """A two-basis dictionary of diagonal maps, alpha[b] = c_b x on an unpadded frame: with a diagonal Hessian every step of
    the loop is elementwise and can be checked by hand (test_pd_events_cpu.py)."""

    def __init__(self, nx, ny, c=(1.0, 0.5)):
        self.c, self.nbasis, self.nxmax, self.nymax = tuple(c), len(c), nx, ny

    def dot(self, x, out):
        for b, c in enumerate(self.c):
            out[:, b] = c * x

    def hdot(self, alpha, out):
        out[...] = sum(c * alpha[:, b] for b, c in enumerate(self.c))
