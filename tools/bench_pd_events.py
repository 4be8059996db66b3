#!/usr/bin/env python3
"""Secondary measurement: the primal-dual solve with convergence events and l1 reweighting (BASELINE config C4 shape).

    python tools/bench_pd_events.py [--nx 4096] [--nband 4] [--iters 57] [--events 3] [--reps 3]

Uses only the public classes, so it runs unchanged on a build without the device event loop (where a callback sends the
solve to the generic loop) -- alternate the two builds in one session to compare.  Convergence cannot be scheduled on random
data, so the "60-iteration solve with 3 reweightings" is timed as two solves whose sum it is:
  plain   ``iters`` iterations, no callback (tol 0): the device loop of pfbhip_primal_dual
  quiet   ``iters`` iterations with a callback installed that never fires (tol 0)
  events  ``events + 1`` iterations at tol = inf: every iteration is an event, the callback reweights ``events`` times, then stops
  update  one ``L21.update_weights(x)`` on a host array (upload included), and ``init_reweighting``
``solve_with_events_ms`` = quiet + events: two solves, so one create / upload / get-dual more than a single solve pays.  On a
build without the device event loop the quiet leg is ``iters * (reps + 1)`` generic iterations (about 2 s each at C4): give
that build a small ``--iters``.  Prints one JSON line; times are the median of ``reps`` after one warm-up.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--nband", type=int, default=4)
    ap.add_argument("--iters", type=int, default=57)
    ap.add_argument("--events", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    from pfb_imaging_amd import _lib, prox
    from pfb_imaging_amd.operators.hessian import HessPSF
    from pfb_imaging_amd.operators.psi import PsiNocopyt
    from pfb_imaging_amd.opt import L21, PrimalDual, PsfGrad

    _lib.require_gpu()
    nx = ny = args.nx
    nband, bases = args.nband, ("self", "db1", "db2", "db3")
    rng = np.random.default_rng(0)
    abspsf = 1.0 + 0.1 * np.abs(rng.standard_normal((nband, 2 * nx, ny + 1)))
    hess = HessPSF(nx, ny, abspsf, beam=None, eta=0.01)
    psi = PsiNocopyt(nband, nx, ny, bases, 3, 1)
    reg = L21(psi, bases, nu=np.sqrt(len(bases)), rmsfactor=1.0, alpha=2.0)
    model = np.abs(rng.standard_normal((nband, nx, ny))) * (rng.random((nband, nx, ny)) > 0.99)
    xtilde = model + 0.1 * rng.standard_normal(model.shape)
    hessnorm = float(abspsf.max() + 0.01)

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e3, (max(ts) - min(ts)) * 1e3

    def solve(tol, maxit, cb):
        pd = PrimalDual(tol=tol, maxit=maxit, verbosity=0, gamma=1.0, primal_prox=prox.positivity, on_converge=cb)
        pd.setup(reg, hessnorm)
        pd.set_grad(PsfGrad(hess, xtilde, 1.0))
        pd.solve(model.copy(), 1e-3)
        return pd

    out = {"label": args.label, "config": {"nband": nband, "image": [nx, ny], "bases": bases, "nlevel": 3, "positivity": 1,
                                           "iters": args.iters, "events": args.events}}
    t0 = time.perf_counter()
    reg.init_reweighting(xtilde)
    out["init_reweighting_ms_first"] = (time.perf_counter() - t0) * 1e3
    out["init_reweighting_ms"], _ = timed(lambda: reg.init_reweighting(xtilde))
    out["update_weights_ms"], out["update_weights_spread_ms"] = timed(lambda: reg.update_weights(model))
    ones = np.ones(reg.l1weight.shape)
    reg.l1weight = ones
    out["plain_ms"], out["plain_spread_ms"] = timed(lambda: solve(0.0, args.iters, None))
    out["plain_ms_per_iteration"] = out["plain_ms"] / args.iters
    out["quiet_ms"], out["quiet_spread_ms"] = timed(lambda: solve(0.0, args.iters, lambda x, k, eps: True))
    last = {}

    def events():
        calls = []

        def cb(x, k, eps):
            calls.append(k)
            if len(calls) <= args.events:
                reg.update_weights(x)
                return False
            return True

        reg.l1weight = ones
        pd = solve(float("inf"), args.events + 2, cb)
        last.update({k: v for k, v in pd.last.items() if k != "stages"})

    out["events_ms"], out["events_spread_ms"] = timed(events)
    out["events_last"] = last
    out["solve_with_events_ms"] = out["quiet_ms"] + out["events_ms"]
    out["iterations_total"] = args.iters + args.events + 1
    print(json.dumps(out))


if __name__ == "__main__":
    main()
