"""Reader of tests/golden/cg_pins.npz (made by tests/golden/make_cg_pins.py: the reference's ``pcg_numba`` and
``power_method_numba`` run as plain Python on a diagonal operator), the recipe of its inputs, and plain numpy restatements of
the two loops for shapes beyond the fixtures.  Shared by test_cg_pins_cpu.py and test_gpu_cg_pins.py; loads once per directory
and hands out read-only arrays.

The operator is ``A v = d * v`` with ``d = sum_parts beam_part**2 + eta``, ``eta = 0.25``: what ``PsfConv.apply`` (scale 1)
computes when every bound psfhat is identically 1, at any padding."""

import functools
import os

import numpy as np

ETA = 0.25
BEAM_DEN, B_DEN = 128.0, 64.0
# (nx, ny): n = 63 (less than a wave), 65 (a wave plus one), 255 / 257 (a workgroup minus / plus one), 1073 (several
# workgroups and a ragged tail)
SIZES = ((3, 21), (5, 13), (3, 85), (1, 257), (37, 29))
SPECIAL_SIZE = (37, 29)
# name: ((tol, maxit, minit), status the case is there for)
PARAMS = {"conv": ((1e-5, 500, 1), 0), "minit": ((1e-2, 500, 12), 0), "maxit": ((1e-12, 7, 1), 1), "stall": ((0.5, 100, 40), 2),
          "loose": ((1e-3, 500, 1), 0)}
# the cases the generator writes (asserted against the file's own list in load()); "x0": a non-zero start, "two": two beams
CG_CASES = tuple(f"{nx}x{ny}_{p}" for nx, ny in SIZES for p in PARAMS) + ("37x29_x0", "37x29_two")
PM_RUNS = {"fixed": (0.0, 8), "tol": (1e-4, 500)}


def draw(size, nparts, pm=False):
    """The integers behind one case: default_rng(nx * ny), beam before b before x0 (CG) or beam before b0 (power method)."""
    nx, ny = size
    rng = np.random.default_rng(nx * ny)
    beam_num = (64 + rng.integers(0, 129, size=(nparts, nx, ny))).astype(np.uint8)
    if pm:
        return dict(beam_num=beam_num, b0_num=rng.integers(1, 65, size=(nparts, nx, ny)).astype(np.uint8))
    return dict(beam_num=beam_num, b_num=rng.integers(-512, 513, size=(nx, ny)).astype(np.int16),
                x0_num=rng.integers(-256, 257, size=(nx, ny)).astype(np.int16))


def diagonal(beam):
    """d of the operator for beams (nparts, nx, ny); eta enters once."""
    return (np.asarray(beam, dtype=np.float64) ** 2).sum(axis=0) + ETA


def _cg_case(name, beam_num, b_num, x0_num):
    size, kind = name.split("_")
    nx, ny = (int(v) for v in size.split("x"))
    params, want = PARAMS["conv" if kind in ("x0", "two") else kind]
    beam = beam_num / BEAM_DEN
    return dict(name=name, nx=nx, ny=ny, params=params, want_status=want, beam=beam, d=diagonal(beam), b=b_num / B_DEN,
                x0=None if x0_num is None else x0_num / B_DEN)


def cg_inputs(name):
    """The inputs of a case from the recipe alone (the generator's side; the tests read them from the file)."""
    size, kind = name.split("_")
    raw = draw(tuple(int(v) for v in size.split("x")), 2 if kind == "two" else 1)
    return _cg_case(name, raw["beam_num"], raw["b_num"], raw["x0_num"] if kind == "x0" else None)


def pm_inputs(size):
    raw = draw(size, 2, pm=True)
    beam = raw["beam_num"] / BEAM_DEN
    return dict(nx=size[0], ny=size[1], beam=beam, d=beam ** 2 + ETA, b0=raw["b0_num"] / B_DEN)


@functools.lru_cache(maxsize=None)
def load(golden_dir):
    with np.load(os.path.join(golden_dir, "cg_pins.npz")) as z:
        p = {k: z[k] for k in z.files}
    for a in p.values():
        a.setflags(write=False)
    assert tuple(p["cases"]) == CG_CASES
    return p


def cg_case(p, name):
    """One pinned CG case: inputs, and x / eps (every iteration) / phi / iters / status of the longdouble reference run with
    the float64 run's relative distances x_floor, eps_floor, phi_floor."""
    size, kind = name.split("_")
    if kind == "two":
        c = _cg_case(name, p["two_beam_num"], p["two_b_num"], None)
    else:
        c = _cg_case(name, p[size + "_beam_num"][None], p[size + "_b_num"], p["x0_num"] if kind == "x0" else None)
    fl = p[name + "_floor"]
    for a in (c["beam"], c["d"], c["b"], c["x0"]):
        if a is not None:
            a.setflags(write=False)
    c.update(x=p[name + "_x"], eps=p[name + "_eps"], phi=float(p[name + "_phi"]), iters=int(p[name + "_iters"]),
             status=int(p[name + "_status"]), x_floor=float(fl[0]), eps_floor=float(fl[1]), phi_floor=float(fl[2]))
    return c


def pm_case(p, size):
    tag = f"pm_{size[0]}x{size[1]}"
    beam = p[tag + "_beam_num"] / BEAM_DEN
    c = dict(nx=size[0], ny=size[1], beam=beam, d=beam ** 2 + ETA, b0=p[tag + "_b0_num"] / B_DEN, b=p[tag + "_fixed_b"])
    for a in (c["beam"], c["d"], c["b0"]):
        a.setflags(write=False)
    for run in PM_RUNS:
        fl = p[f"{tag}_{run}_floor"]
        c[run] = dict(beta=float(p[f"{tag}_{run}_beta"]), iters=int(p[f"{tag}_{run}_iters"]), status=int(p[f"{tag}_{run}_status"]),
                      beta_floor=float(fl[0]), b_floor=float(fl[1]))
    return c


def rel_l2(a, ref):
    ref = np.asarray(ref)
    d = np.asarray(a, dtype=ref.dtype) - ref
    return float(np.sqrt((d * d).sum()) / max(float(np.sqrt((ref * ref).sum())), 1e-300))


def bound(floor):
    """The bound on a relative distance whose floor the generator measured: 100 floors (another summation order, the FFT's
    rounding of the operator), never below the 1e-11 of FFT-based operators."""
    return max(100.0 * floor, 1e-11)


# ---- the two loops in plain numpy, any float dtype ----------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum()


def cg_ref(d, b, x0, tol, maxit, minit, dtype=np.longdouble):
    """pcg_numba without preconditioner (opt/pcg.py:88-199 of the reference) on ``A v = d * v``: dict(x, r, eps (every
    iteration), phi, iters, status).  ``eps`` is the computed ``||x - xp|| / ||x||`` with ``||x||^2`` floored at 1e-12."""
    d, b = np.asarray(d, dtype=dtype), np.asarray(b, dtype=dtype)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=dtype)
    r = d * x - b
    if not r.any():
        return dict(x=x, r=r, eps=np.zeros(0, dtype=dtype), phi=dtype(0.0), iters=0, status=3)
    p = -r
    rnorm = _dot(r, r)
    phi0 = dtype(1.0) if (np.isnan(rnorm) or rnorm == 0.0) else rnorm
    k, eps, stall, hist = 0, dtype(1.0), 0, []
    while (eps > tol or k < minit) and k < maxit and stall < 5:
        xp = x.copy()
        ap = d * p
        alpha = _dot(r, r) / _dot(p, ap)
        x = xp + alpha * p
        r = r + alpha * ap
        rnorm_next = _dot(r, r)
        p = (rnorm_next / rnorm) * p - r
        rnorm = rnorm_next
        k += 1
        epsp = eps
        eps = np.sqrt(_dot(x - xp, x - xp) / max(_dot(x, x), dtype(1e-12)))
        hist.append(eps)
        if abs(epsp - eps) < 1e-3 * tol:
            stall += 1
    status = 1 if k >= maxit else (2 if stall >= 5 else 0)
    return dict(x=x, r=r, eps=np.array(hist, dtype=dtype), phi=rnorm / phi0, iters=k, status=status)


def power_ref(d, b0, tol, maxit, dtype=np.longdouble):
    """power_method_numba (opt/power_method.py:40-93 of the reference) on ``A v = d * v``: dict(beta, b, eps, iters, status)."""
    d, b0 = np.asarray(d, dtype=dtype), np.asarray(b0, dtype=dtype)
    b = b0 / np.sqrt(_dot(b0, b0))
    beta, eps, k, hist = dtype(1.0), dtype(1.0), 0, []
    bp = b.copy()
    while eps > tol and k < maxit:
        b = d * bp
        bnorm = np.sqrt(_dot(b, b))
        betap = beta
        beta = _dot(bp, b) / _dot(bp, bp)
        b = b * (dtype(1.0) / bnorm)
        eps = abs(beta - betap) / betap
        hist.append(eps)
        k += 1
        bp = b.copy()
    return dict(beta=beta, b=b, eps=np.array(hist, dtype=dtype), iters=k, status=int(k == maxit))
