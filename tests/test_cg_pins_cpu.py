"""CPU tests of the conjugate-gradient and power-method pins (tests/golden/cg_pins.npz, made by tests/golden/make_cg_pins.py
from reference runs of ``pcg_numba`` and ``power_method_numba`` on a diagonal operator).

Every host loop of this project that restates those two functions must reproduce every pinned run -- the iteration count and
the status exactly, so every branch of the stopping rule (``minit`` forcing iterations, ``maxit``, five stalls) is decided as
the reference decides it: ``opt._cg_host`` (what ``pcg_numba`` falls back to for arbitrary callables and every preconditioned
solve), ``oracle.fftconv.pcg`` / ``power_method`` (the reference of the existing GPU tests), the host loop of
``opt.power_method`` around a bare callable, and ``cg_ref`` / ``power_ref`` of tests/_cg_pins.py (the reference of the GPU tests
at shapes beyond the fixtures).

Tolerances, as in test_gpu_cg_pins.py: x relative l2 <= 1e-11; eps and phi relative <= max(100 floors, 1e-11), the floor being
the float64 reference run's distance from the longdouble run that the generator measured; beta 1e-11; b 1e-9."""

import numpy as np
import pytest

from tests import _cg_pins as cp

X_TOL, BETA_TOL, B_TOL = 1e-11, 1e-11, 1e-9


def _rel(a, ref):
    return abs(float(a) - ref) / abs(ref)


def _check_cg(c, x, eps, phi, iters, status, what):
    assert (iters, status) == (c["iters"], c["status"]), f"{what} {c['name']}: iters / status {(iters, status)} != pin {(c['iters'], c['status'])}"
    dx, de, dp = cp.rel_l2(x, c["x"]), _rel(eps, c["eps"][-1]), _rel(phi, c["phi"])
    assert dx <= X_TOL, f"{what} {c['name']}: x {dx:.3e}"
    assert de <= cp.bound(c["eps_floor"]), f"{what} {c['name']}: eps {de:.3e} > {cp.bound(c['eps_floor']):.3e}"
    assert dp <= cp.bound(c["phi_floor"]), f"{what} {c['name']}: phi {dp:.3e} > {cp.bound(c['phi_floor']):.3e}"


def test_pins_are_well_formed(golden_dir):
    p = cp.load(golden_dir)
    strings = sorted(k for k, a in p.items() if a.dtype.kind in "USO")
    assert strings == ["cases", "cites"] and all(len(s) < 160 and "\n" not in s for s in p["cites"])
    seen = set()
    for name in cp.CG_CASES:
        c, want = cp.cg_case(p, name), cp.cg_inputs(name)
        tol, maxit, minit = c["params"]
        for key in ("beam", "b", "x0"):                       # the stored inputs are the recipe's
            assert (c[key] is None and want[key] is None) or np.array_equal(c[key], want[key]), (name, key)
        assert c["status"] == c["want_status"] and c["eps"].shape == (c["iters"],) and c["iters"] <= maxit
        assert c["status"] == 2 or minit <= c["iters"]        # (five stalls end the loop whatever minit says)
        assert c["x"].shape == (c["nx"], c["ny"]) and np.isfinite(c["x"]).all()
        assert c["x_floor"] <= 1e-13 and 0 <= c["eps_floor"] < 1e-9 and 0 <= c["phi_floor"] < 1e-9
        # the reference alone decides every branch: no eps on tol, no stall decision on its threshold
        e = np.concatenate([[1.0], c["eps"]])
        assert (np.abs(e[1:] - tol) > 1e-6 * tol).all() and (np.abs(np.abs(np.diff(e)) - 1e-3 * tol) > 1e-9 * tol).all()
        # and the stored history leads to the stored end through the reference's rule
        stalls = int((np.abs(np.diff(e)) < 1e-3 * tol).sum())
        assert c["status"] == (1 if c["iters"] >= maxit else (2 if stalls >= 5 else 0))
        if c["status"] == 0:
            assert c["eps"][-1] <= tol and (c["iters"] == minit or c["eps"][-2] > tol)
        seen.add((name.split("_")[1], c["status"]))
    assert {("conv", 0), ("minit", 0), ("maxit", 1), ("stall", 2), ("loose", 0), ("x0", 0), ("two", 0)} == seen
    c = cp.cg_case(p, "37x29_minit")
    assert (c["eps"][:-1] <= c["params"][0]).any(), "minit must be what keeps this case going"
    assert cp.cg_case(p, "37x29_two")["beam"].shape[0] == 2 and np.any(cp.cg_case(p, "37x29_x0")["x0"])
    for size in cp.SIZES:
        c, want = cp.pm_case(p, size), cp.pm_inputs(size)
        assert np.array_equal(c["beam"], want["beam"]) and np.array_equal(c["b0"], want["b0"])
        assert c["fixed"]["iters"] == 8 and c["fixed"]["status"] == 1 and c["tol"]["status"] == 0 and 1 < c["tol"]["iters"] < 500
        assert abs(np.linalg.norm(c["b"]) - 1.0) <= 1e-15
        assert max(c[r][f] for r in cp.PM_RUNS for f in ("beta_floor", "b_floor")) < 1e-13
        assert c["d"].min() < c["tol"]["beta"] <= c["d"].max()


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["f64", "ld"])
@pytest.mark.parametrize("name", cp.CG_CASES)
def test_cg_ref_reproduces_the_pins(golden_dir, name, dtype):
    c = cp.cg_case(cp.load(golden_dir), name)
    got = cp.cg_ref(c["d"], c["b"], c["x0"], *c["params"], dtype=dtype)
    _check_cg(c, got["x"], got["eps"][-1], got["phi"], got["iters"], got["status"], "cg_ref")
    de = np.abs(got["eps"].astype(np.float64) - c["eps"]) / c["eps"]       # every iteration's eps, not only the last
    assert de.max() <= 1e-9, f"eps history {de.max():.3e}"


@pytest.mark.parametrize("name", cp.CG_CASES)
def test_cg_host_reproduces_the_pins(golden_dir, name):
    from pfb_imaging_amd import opt

    c = cp.cg_case(cp.load(golden_dir), name)
    d, calls = c["d"], []

    def aop(v):
        calls.append(1)
        return d * v

    x0 = np.zeros_like(c["b"]) if c["x0"] is None else c["x0"].copy()
    r0 = d * x0 - c["b"]
    tol, maxit, minit = c["params"]
    x, r = opt._cg_host(aop, c["b"], x0, None, tol, maxit, minit, 0, 10, True, "host")
    assert x is x0, "x0 is the iterate: updated in place and returned"
    last = opt._cg_host.last
    assert len(calls) - 1 == last["iters"]
    _check_cg(c, x, last["eps"], np.vdot(r, r) / np.vdot(r0, r0), last["iters"], last["status"], "_cg_host")


@pytest.mark.parametrize("name", cp.CG_CASES)
def test_oracle_pcg_reproduces_the_pins(golden_dir, name):
    """(The oracle's pcg returns a new array and leaves x0 alone: the GPU tests that use it pass start vectors they read again.)"""
    from oracle import fftconv

    c = cp.cg_case(cp.load(golden_dir), name)
    d, calls = c["d"], []

    def aop(v):
        calls.append(1)
        return d * v

    tol, maxit, minit = c["params"]
    x = fftconv.pcg(aop, c["b"], x0=c["x0"], tol=tol, maxit=maxit, minit=minit)
    last = fftconv.pcg.last
    assert len(calls) - 1 == last["iters"]
    _check_cg(c, x, last["eps"], last["phi"], last["iters"], last["status"], "oracle.fftconv.pcg")


def test_host_loops_report_a_zero_start_residual(golden_dir, capsys):
    from oracle import fftconv
    from pfb_imaging_amd import opt

    c = cp.cg_case(cp.load(golden_dir), "37x29_x0")
    d = c["d"]
    b = d * c["x0"]
    x0 = c["x0"].copy()
    assert opt._cg_host(lambda v: d * v, b, x0, None, 1e-5, 500, 1, 1, 10, False, "host") is x0 and np.array_equal(x0, c["x0"])
    assert "Initial residual is zero" in capsys.readouterr().out
    assert np.array_equal(fftconv.pcg(lambda v: d * v, b, x0=x0), c["x0"]) and fftconv.pcg.last["status"] == 3
    got = cp.cg_ref(d, b, c["x0"], 1e-5, 500, 1)
    assert (got["status"], got["iters"]) == (3, 0) and np.array_equal(got["x"], c["x0"])


def _check_pm(c, run, beta, b, iters, status, what):
    pin = c[run]
    assert (iters, status) == (pin["iters"], pin["status"]), f"{what} {run}: {(iters, status)} != pin {(pin['iters'], pin['status'])}"
    assert _rel(beta, pin["beta"]) <= BETA_TOL, f"{what} {run}: beta {_rel(beta, pin['beta']):.3e}"
    assert abs(float(np.sqrt((np.asarray(b) ** 2).sum())) - 1.0) <= 1e-12
    if run == "fixed":
        assert cp.rel_l2(b, c["b"]) <= B_TOL, f"{what}: b {cp.rel_l2(b, c['b']):.3e}"


@pytest.mark.parametrize("run", list(cp.PM_RUNS))
@pytest.mark.parametrize("size", cp.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_power_loops_reproduce_the_pins(golden_dir, size, run):
    """power_ref (float64 and longdouble), oracle.fftconv.power_method and the host loop of opt.power_method around a bare
    callable (importing it needs no device; only the bound methods of this package's operators go to the device)."""
    from oracle import fftconv
    from pfb_imaging_amd import opt

    c = cp.pm_case(cp.load(golden_dir), size)
    d, shape = c["d"], c["d"].shape
    tol, maxit = cp.PM_RUNS[run]
    for dtype in (np.float64, np.longdouble):
        got = cp.power_ref(d, c["b0"], tol, maxit, dtype=dtype)
        _check_pm(c, run, got["beta"], got["b"], got["iters"], got["status"], f"power_ref {dtype.__name__}")
    beta, b, k = fftconv.power_method(lambda v: d * v, shape, c["b0"].copy(), tol=tol, maxit=maxit)
    _check_pm(c, run, beta, b, k, int(k == maxit), "oracle.fftconv.power_method")
    b0 = c["b0"].copy()
    beta, b = opt.power_method(lambda v: d * v, shape, b0=b0, tol=tol, maxit=maxit, verbosity=0)
    assert np.array_equal(b0, c["b0"]), "the caller's b0 is not modified"
    _check_pm(c, run, beta, b, opt.power_method.last["iters"], opt.power_method.last["status"], "opt.power_method (host loop)")
