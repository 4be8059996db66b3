#!/usr/bin/env python3
"""Reference-RUN fixtures of the conjugate-gradient solver and the power method: ``cg_pins.npz``.

Like make_numba_pins.py, this reads the reference's files AT GENERATION TIME and executes what it takes from them AS IT
STANDS.  No reference text is stored: only inputs, outputs and ``cites`` go into the ``.npz``.

The stand-in, exactly: make_numba_pins.py's ``install_standin()`` (``njit(**kw)`` is the identity decorator, every option --
nogil, cache, parallel, fastmath -- ignored; ``prange = range``), and its ``take_numba()``: the file's imports are executed one
by one (the unsatisfiable ones skipped), then the named module-level assignment, then the named functions, unmodified, every
decorator asserted to be the stand-in.  So what runs is CPython evaluating the reference's statements one by one in IEEE
double or in ``np.longdouble`` (80-bit): no fastmath reassociation, sums in index order.

What is taken (``cites`` in the file has the line ranges):

  opt/pcg.py            ``_FAST_JIT`` (the decorators' argument), ``_nb_fused_alpha_update``, ``_nb_fused_beta_update``,
                        ``_nb_norm_diff``, ``pcg_numba``
  opt/power_method.py   ``_FAST_JIT``, ``_nb_vdot_pair``, ``_nb_normalize``, ``power_method_numba``; ``norm`` is scipy.linalg's,
                        as the file imports it.  ``log`` (the file binds it from a module absent here) is bound to a stub whose
                        ``info`` appends the message to a list.

The operator is diagonal: ``aop = lambda v: d * v`` with ``d = sum_parts beam_part**2 * scale + eta`` (scale 1, eta 0.25), which
is what ``PsfConv.apply`` computes when every bound psfhat is identically 1.

The reference returns only ``x`` (and ``r`` with ``return_resid=True``).  The rest is observed from outside:

  iters    the number of ``aop`` calls minus one
  status   from the message ``pcg_numba`` prints (stdout captured): "Success" 0, "Max iters" 1, "Stalled" 2, "Initial
           residual is zero" 3; for the power method from its log line: "Maximum iterations reached" 1, "Success" 0
  eps      every return value of ``_nb_norm_diff``: the name is rebound, in the taken namespace, to a wrapper that calls the
           original and logs what it returns.  For the power method the return values of ``_nb_vdot_pair`` are logged the
           same way and eps_k = |beta_k - beta_{k-1}| / beta_{k-1} recomputed from them (the reference's own expression)
  phi      ``r.r / phi0`` from the returned ``r``, with ``phi0 = r0.r0`` of the start residual, as the reference has it

The pinned ``x``, ``eps``, ``phi`` (``beta``, ``b``) are the longdouble run rounded to float64; ``*_floor`` is the float64
run's relative distance from it (relative l2 for vectors).

Inputs are dyadic, stored as small integers: ``beam = (64 + integers[0, 128]) / 128``, ``b = integers[-512, 512] / 64``,
``x0 = integers[-256, 256] / 64``, from ``default_rng(n)`` with n = nx * ny, beam drawn before b, b before x0.  The two-part
case and the power method (a two-band cube) draw a ``(2, nx, ny)`` beam; the power method's ``b0 = integers[1, 64] / 64``.

Assertions made before anything is written, for every CG case (none had to be changed: every case stands as first chosen):

  * the float64 and the longdouble run agree in ``iters`` and ``status``, and the status is the one the case is there for
  * every eps_k differs from tol by more than 1e-6 relative
  * every |eps_k - eps_{k-1}| (eps_0 = 1) differs from 1e-3 tol by more than 1e-6 relative
  * every p.Ap > 0 and every iterate finite (the operator wrapper checks both on each call)
  * x_floor <= 1e-13

and for the power method: the two runs agree in ``iters`` and ``status``; in the ``tol = 1e-4`` run every eps_k differs from
tol by more than 1e-6 relative.

Run from the repo root in the build container:  python tests/golden/make_cg_pins.py
"""

import contextlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_mnp = _load("make_numba_pins")
REF, SRC = _mnp.REF, _mnp.SRC

from tests import _cg_pins as cp  # noqa: E402  (the case table and the input recipe, shared with the reader)

LD = np.longdouble
MESSAGES = (("Success", 0), ("Max iters", 1), ("Stalled", 2), ("Initial residual is zero", 3))


def load_reference():
    standin = _mnp.install_standin()
    try:
        rel_cg, rel_pm = f"{SRC}/opt/pcg.py", f"{SRC}/opt/power_method.py"
        cg_ns, cg_found = _mnp.take_numba(rel_cg, ["_nb_fused_alpha_update", "_nb_fused_beta_update", "_nb_norm_diff", "pcg_numba"],
                                          ("_FAST_JIT",), standin)
        pm_ns, pm_found = _mnp.take_numba(rel_pm, ["_nb_vdot_pair", "_nb_normalize", "power_method_numba"], ("_FAST_JIT",), standin)
    finally:
        sys.modules.pop("numba", None)
        sys.modules.pop("numba.extending", None)
    assert "norm" in pm_ns and pm_ns["norm"].__module__.startswith("scipy.linalg")
    cites = [f"{rel_cg}:{a}-{b} {k}" for k, (a, b) in sorted(cg_found.items())]
    cites += [f"{rel_pm}:{a}-{b} {k}" for k, (a, b) in sorted(pm_found.items())]
    cites += ["numba: njit = identity, prange = range; _FAST_JIT executed as it stands and ignored",
              "power_method.py: log = stub(info = list.append); norm = scipy.linalg.norm as imported",
              "iters = aop calls - 1; status from the printed / logged message; eps = logged returns of _nb_norm_diff",
              "phi = r.r / r0.r0 from return_resid=True"]
    return cg_ns, pm_ns, cites


def run_cg(ns, d, b, x0, tol, maxit, minit, dtype):
    """One run of the reference's pcg_numba on the diagonal operator: dict(x, eps, phi, iters, status)."""
    d, b = d.astype(dtype), b.astype(dtype)
    x0 = None if x0 is None else x0.astype(dtype)
    calls, eps_log = [], []

    def aop(v):
        out = d * v
        assert np.isfinite(v).all() and out.dtype == dtype
        if calls:                                     # every call after the first is aop(p)
            assert (v * out).sum() > 0, "p.Ap <= 0"
        calls.append(1)
        return out

    orig = ns["_nb_norm_diff"]

    def logged(x, xp):
        e = orig(x, xp)
        eps_log.append(e)
        return e

    r0 = d * (np.zeros_like(b) if x0 is None else x0) - b
    phi0 = (r0 * r0).sum()
    ns["_nb_norm_diff"] = logged
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf), np.errstate(all="raise"):
            x, r = ns["pcg_numba"](aop, b, x0=x0, tol=tol, maxit=maxit, minit=minit, verbosity=1, return_resid=True)
    finally:
        ns["_nb_norm_diff"] = orig
    msg = buf.getvalue().strip().splitlines()
    assert len(msg) == 1, msg
    status = [s for m, s in MESSAGES if msg[0].startswith(m)]
    assert len(status) == 1, msg
    assert x.dtype == dtype and np.isfinite(x).all() and (x0 is None or x is x0)
    iters = len(calls) - 1
    assert iters == len(eps_log)
    return dict(x=x, eps=np.array(eps_log, dtype=dtype), phi=(r * r).sum() / phi0, iters=iters, status=status[0])


def rel(a64, ald):
    """Relative distance of the float64 run from the longdouble run (relative l2 for vectors), as float64."""
    dlt = np.asarray(a64, dtype=LD) - ald
    return float(np.sqrt((dlt * dlt).sum()) / np.sqrt((np.asarray(ald) ** 2).sum()))


def away(values, mark):
    return all(abs(v - mark) > 1e-6 * mark for v in values)


def cg_pins(out, ns):
    for name in cp.CG_CASES:
        c = cp.cg_inputs(name)
        tol, maxit, minit = c["params"]
        runs = {dt: run_cg(ns, c["d"], c["b"], c["x0"], tol, maxit, minit, dt) for dt in (np.float64, LD)}
        f64, ld = runs[np.float64], runs[LD]
        assert (f64["iters"], f64["status"]) == (ld["iters"], ld["status"]), f"{name}: float64 and longdouble decide differently"
        assert ld["status"] == c["want_status"], f"{name}: status {ld['status']}"
        for r in runs.values():
            e = [float(v) for v in r["eps"]]
            assert away(e, tol), f"{name}: an eps sits on tol"
            assert away([abs(a - b) for a, b in zip([1.0] + e[:-1], e)], 1e-3 * tol), f"{name}: a stall decision sits on its threshold"
        x_floor = rel(f64["x"], ld["x"])
        assert x_floor <= 1e-13, f"{name}: x_floor {x_floor}"
        eps_floor = float(abs(LD(f64["eps"][-1]) - ld["eps"][-1]) / ld["eps"][-1])
        phi_floor = float(abs(LD(f64["phi"]) - ld["phi"]) / ld["phi"])
        out.update({f"{name}_x": ld["x"].astype(np.float64), f"{name}_eps": ld["eps"].astype(np.float64),
                    f"{name}_phi": np.float64(ld["phi"]), f"{name}_iters": np.int64(ld["iters"]),
                    f"{name}_status": np.int64(ld["status"]), f"{name}_floor": np.array([x_floor, eps_floor, phi_floor])})
        print(f"{name:14s} iters {ld['iters']:3d} status {ld['status']} eps {float(ld['eps'][-1]):.3e} phi {float(ld['phi']):.3e} "
              f"floors x {x_floor:.1e} eps {eps_floor:.1e} phi {phi_floor:.1e}")
    for size in cp.SIZES:                       # inputs once per size; the special cases carry their own
        raw = cp.draw(size, 1)
        out[f"{size[0]}x{size[1]}_beam_num"], out[f"{size[0]}x{size[1]}_b_num"] = raw["beam_num"][0], raw["b_num"]
    raw = cp.draw(cp.SPECIAL_SIZE, 1)
    out["x0_num"] = raw["x0_num"]
    raw = cp.draw(cp.SPECIAL_SIZE, 2)
    out["two_beam_num"], out["two_b_num"] = raw["beam_num"], raw["b_num"]


def run_pm(ns, d, b0, tol, maxit, dtype):
    d, b0 = d.astype(dtype), b0.astype(dtype)
    calls, betas, log = [], [], []
    orig = ns["_nb_vdot_pair"]

    def logged(bp, b):
        num, den = orig(bp, b)
        betas.append(num / den)
        return num, den

    def aop(v):
        calls.append(1)
        assert np.isfinite(v).all()
        return d * v

    ns["_nb_vdot_pair"], ns["log"] = logged, types.SimpleNamespace(info=log.append)
    try:
        with np.errstate(all="raise"):
            beta, b = ns["power_method_numba"](aop, d.shape, b0=b0, tol=tol, maxit=maxit, verbosity=1)
    finally:
        ns["_nb_vdot_pair"] = orig
        del ns["log"]
    assert len(log) == 1 and b.dtype == dtype and beta == betas[-1]
    status = 1 if log[0].startswith("Maximum iterations reached") else 0
    assert status or log[0].startswith("Success")
    prev = [dtype(1.0)] + betas[:-1]
    eps = [abs(bk - bp) / bp for bk, bp in zip(betas, prev)]
    return dict(beta=beta, b=b, iters=len(calls), status=status, eps=eps)


def pm_pins(out, ns):
    for size in cp.SIZES:
        c = cp.pm_inputs(size)
        tag = f"pm_{size[0]}x{size[1]}"
        for run, (tol, maxit) in cp.PM_RUNS.items():
            f64, ld = (run_pm(ns, c["d"], c["b0"], tol, maxit, dt) for dt in (np.float64, LD))
            assert (f64["iters"], f64["status"]) == (ld["iters"], ld["status"]), f"{tag}_{run}"
            if tol > 0:
                assert away([float(e) for e in f64["eps"] + ld["eps"]], tol), f"{tag}_{run}: an eps sits on tol"
                assert ld["status"] == 0
            else:
                assert ld["iters"] == maxit and ld["status"] == 1
            floors = [float(abs(LD(f64["beta"]) - ld["beta"]) / ld["beta"]), rel(f64["b"], ld["b"])]
            out.update({f"{tag}_{run}_beta": np.float64(ld["beta"]), f"{tag}_{run}_iters": np.int64(ld["iters"]),
                        f"{tag}_{run}_status": np.int64(ld["status"]), f"{tag}_{run}_floor": np.array(floors)})
            if run == "fixed":
                out[f"{tag}_{run}_b"] = ld["b"].astype(np.float64)
            print(f"{tag}_{run:6s} iters {ld['iters']:3d} status {ld['status']} beta {float(ld['beta']):.15f} floors {floors[0]:.1e} {floors[1]:.1e}")
        raw = cp.draw(size, 2, pm=True)
        out[tag + "_beam_num"], out[tag + "_b0_num"] = raw["beam_num"], raw["b0_num"]


def compute():
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the 80-bit format here"
    cg_ns, pm_ns, cites = load_reference()
    out = {}
    cg_pins(out, cg_ns)
    pm_pins(out, pm_ns)
    out["cases"] = np.array(cp.CG_CASES)
    out["cites"] = np.array(cites)
    return out


def main():
    out = compute()
    path = os.path.join(HERE, "cg_pins.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:      # fixed member times: the file regenerates byte for byte
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print("\n".join(out["cites"]))
    print("cg_pins.npz", os.path.getsize(path))
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("make_cg_pins.py needs the reference checkout (build container only); the committed .npz travels instead")
    main()
