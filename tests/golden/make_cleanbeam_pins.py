"""Writes tests/golden/cleanbeam_pins.npz: the reference's clean-beam fit (utils/misc.py:529-613) restated in numpy and
scipy on the cases of tests/_cleanbeam_ref.py.  Run once, by hand: ``python tests/golden/make_cleanbeam_pins.py``.

The reference's own function needs jax for the gradient; the restatement uses the analytic gradient of the same objective
and otherwise the same calls: ``scipy.ndimage.label`` (default structure), ``fmin_l_bfgs_b`` with the bounds
``((0, None), (0, None), (0, pi))`` and ``factr=1e7`` from the same start.  Per fitted case the file holds

  nlobe, nfit, p0      the main lobe's size, the fit region's size, the start point (np.sum, as the reference)
  p0_disagreement      |p0(np.sum) - p0(math.fsum)| per parameter: what the order of summation alone moves
  p_ref, f_ref         where L-BFGS-B stops, and the objective there
  p_exact, f_exact     the minimiser: least_squares, trf, the same bounds, all tolerances 1e-15
  exact_spread         |trf - dogbox| per parameter, dogbox from a start perturbed by 5 %
  window               the window the device must end with (see _cleanbeam_ref.window_for)

and ``H_nlobe`` for the spiral.  The generator refuses a case in which the restated reference raises its warning flag, ends
further than 1e-4 from the minimiser in any parameter, or whose beam is rounder than emaj / emin = 1.05."""

import os
import sys

import numpy as np
from scipy.ndimage import label
from scipy.optimize import fmin_l_bfgs_b, least_squares

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _cleanbeam_ref as ref  # noqa: E402


def lobe_by_label(psfv):
    islands, _ = label(np.where(psfv > ref.LEVEL, 1.0, 0))
    ncenter = islands[psfv.shape[0] // 2, psfv.shape[1] // 2]
    assert ncenter != 0, "centre pixel below the level"
    return islands == ncenter


def pin_case(name, band=0):
    pr = ref.problem(name, band)
    psfv = pr["psfv"]
    lobe = lobe_by_label(psfv)
    assert np.array_equal(lobe, pr["lobe"]), f"{name}: label and the restated flood fill disagree"
    p0 = ref.start_point(psfv, lobe)
    p0_fsum = ref.start_point(psfv, lobe, total=ref.fsum)
    data, x, y = pr["data"]
    # the region's edge must not sit within rounding of an integer radius^2, or nfit would depend on the summation order
    r2 = (ref.NSIGMA * (p0[0] / ref.FWHM)) ** 2
    assert abs(r2 - round(r2)) > 1e-6 * max(r2, 1.0) or r2 > 2 * max(psfv.shape) ** 2, f"{name}: fit radius^2 {r2} too near an integer"

    def fun_grad(p):
        r, jac = ref.residual_jac(p, data, x, y)
        return float(r @ r), 2.0 * (jac.T @ r)

    bounds = ((0, None), (0, None), (0, np.pi))
    p_ref, f_ref, d = fmin_l_bfgs_b(fun_grad, p0.copy(), bounds=bounds, factr=1e7)
    assert d["warnflag"] == 0, f"{name}: warnflag {d['warnflag']}"
    lsq = dict(jac=lambda p: ref.residual_jac(p, data, x, y)[1], bounds=([0, 0, 0], [np.inf, np.inf, np.pi]),
               xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    res = lambda p: ref.residual_jac(p, data, x, y)[0]  # noqa: E731
    ex = least_squares(res, p0.copy(), method="trf", **lsq)
    start2 = np.clip(p0 * 1.05, [0, 0, 0], [np.inf, np.inf, np.pi])
    ex2 = least_squares(res, start2, method="dogbox", **lsq)
    p_exact, spread = ex.x, np.abs(ex.x - ex2.x)
    f_exact = ref.objective(p_exact, data, x, y)
    dev = np.abs(p_ref - p_exact)
    print(f"{name:3s} nlobe {lobe.sum():5d} nfit {data.size:6d} p0 {p0} p_ref {p_ref} |p_ref-p_exact| {dev.max():.2e} "
          f"spread {spread.max():.2e} (f_ref-f_exact)/f {(f_ref - f_exact) / f_exact:.2e} nit {d['nit']} window {ref.window_for(lobe)}")
    assert dev.max() <= 1e-4, f"{name}: the restated reference is {dev} from the minimiser"
    assert max(p_exact[:2]) / min(p_exact[:2]) >= 1.05, f"{name}: beam too round"
    assert spread.max() <= 1e-6, f"{name}: the minimiser itself is uncertain by {spread}"
    return dict(nlobe=np.int64(lobe.sum()), nfit=np.int64(data.size), p0=p0, p0_disagreement=np.abs(p0 - p0_fsum),
                p_ref=p_ref, f_ref=np.float64(f_ref), p_exact=p_exact, f_exact=np.float64(f_exact), exact_spread=spread,
                window=np.int64(ref.window_for(lobe)))


def main():
    out = {}
    for name in ref.FITTED:
        for k, v in pin_case(name).items():
            out[f"{name}_{k}"] = v
    h = ref.normalised(ref.case("H")[0])
    lobe = lobe_by_label(h)
    assert np.array_equal(lobe, ref.main_lobe(h))
    out["H_nlobe"] = np.int64(lobe.sum())
    out["H_window"] = np.int64(ref.window_for(lobe))
    print("H nlobe", out["H_nlobe"], "of", int((h > ref.LEVEL).sum()), "window", out["H_window"])
    np.savez(ref.PINS, **out)
    print("wrote", ref.PINS, os.path.getsize(ref.PINS), "bytes")


if __name__ == "__main__":
    main()
