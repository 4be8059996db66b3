#!/usr/bin/env python3
"""Secondary measurement: device-resident forward-backward iterations at the C4 shape on ONE GPU.

    python tools/bench_fb.py [--nx 4096] [--nband 4] [--iters 20] [--generic-iters 3]

nband bands of nx^2 pixels, PSF 2x oversized, bases self,db1,db2,db3, 3 levels, positivity mode 1.  One FB iteration =
per band one PSF-approximate Hessian apply, Psi^H and Psi; the shrink over the coefficient cube and one streaming step over
the images (pfbhip_fb_*).  Also measured in the same process: FB without acceleration, the IdentityPsi ISTA form (Hessian
plus one streaming pass), the primal-dual device loop (pfbhip_primal_dual) and a few iterations of the generic loop (the
reference's loop over the GPU operators, cubes over PCIe every iteration).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--nband", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--generic-iters", type=int, default=3)
    args = ap.parse_args()
    from pfb_imaging_amd import _lib, prox
    from pfb_imaging_amd.operators.hessian import HessPSF
    from pfb_imaging_amd.operators.psi import IdentityPsi, PsiNocopyt
    from pfb_imaging_amd.opt import L1, L21, ForwardBackward, PrimalDual, PsfGrad

    _lib.require_gpu()
    nx = ny = args.nx
    nband, bases, n = args.nband, ("self", "db1", "db2", "db3"), args.iters
    rng = np.random.default_rng(0)
    abspsf = 1.0 + 0.1 * np.abs(rng.standard_normal((nband, 2 * nx, ny + 1)))
    hess = HessPSF(nx, ny, abspsf, beam=None, eta=0.01)
    hessnorm = float(abspsf.max() + 0.01)
    psi = PsiNocopyt(nband, nx, ny, bases, 3, 1)
    l21 = L21(psi, bases, nu=float(len(bases)))
    l1 = L1(IdentityPsi(nband, nx, ny))
    model = np.abs(rng.standard_normal((nband, nx, ny))) * (rng.random((nband, nx, ny)) > 0.99)
    xtilde = model + 0.1 * rng.standard_normal(model.shape)
    grad = PsfGrad(hess, xtilde, 1.0)

    def fb_run(reg, acceleration, maxit, wrap=False):
        fb = ForwardBackward(tol=0.0, maxit=maxit, verbosity=0, gamma=0.45, acceleration=acceleration,
                             primal_prox=prox.positivity)
        fb.setup(reg, hessnorm)
        fb.set_grad((lambda z: grad(z)) if wrap else grad)
        fb.solve(model, 1e-3)
        return fb.last

    out = {"metric": "forward-backward iterations (device-resident)", "config": {
        "nband": nband, "image": [nx, ny], "psf": [2 * nx, 2 * ny], "bases": bases, "nlevel": 3, "positivity": 1}}
    fb_run(l21, True, 2)  # warm-up: plans, allocator cache
    last = fb_run(l21, True, n)
    out["fb_ms_per_iteration"] = last["loop_ms"] / n
    stages = {k: v[0] / n for k, v in last["stages"].items() if v[1]}
    out["fb_stage_ms_per_iteration"] = stages
    out["fb_noaccel_ms_per_iteration"] = fb_run(l21, False, n)["loop_ms"] / n
    ista = fb_run(l1, False, n)
    out["ista_ms_per_iteration"] = ista["loop_ms"] / n
    out["ista_stage_ms_per_iteration"] = {k: v[0] / n for k, v in ista["stages"].items() if v[1]}
    # compulsory bytes of the two streaming kernels: shrink alpha read + written once; step xg, xout, xp, xtilde read and
    # x, y, d written (7 image cubes)
    ncoef = nband * len(bases) * psi.nxmax * psi.nymax
    nimg = nband * nx * ny
    out["shrink_tb_per_s"] = 2 * 8 * ncoef / (stages["shrink"] * 1e-3) / 1e12
    out["step_tb_per_s"] = 7 * 8 * nimg / (stages["step"] * 1e-3) / 1e12
    pd = PrimalDual(tol=0.0, maxit=n, verbosity=0, gamma=1.0, primal_prox=prox.positivity)
    pd.setup(l21, hessnorm)
    pd.set_grad(grad)
    pd.solve(model.copy(), 1e-3)
    out["pd_ms_per_iteration"] = pd.last["loop_ms"] / n
    ng = args.generic_iters
    t0 = time.perf_counter()
    fb_run(l21, True, ng, wrap=True)
    out["generic_ms_per_iteration"] = (time.perf_counter() - t0) * 1e3 / ng
    out["fb_vs_pd"] = out["fb_ms_per_iteration"] / out["pd_ms_per_iteration"]
    out["ista_vs_hessian"] = out["ista_ms_per_iteration"] / out["ista_stage_ms_per_iteration"]["forward_hessian"]
    out["generic_vs_device"] = out["generic_ms_per_iteration"] / out["fb_ms_per_iteration"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
