#!/usr/bin/env python3
"""Timings of the direct DFT for DESIGN.md §13 (not part of bench.py, not a test threshold).

  kernels:    DFT.predict and DFT.image on device arrays at --nrow x --nchan visibilities for each of --nsrc sources, in
              Gsource.vis/s (host wall time around synchronous calls, mean of --reps after one warm call)
  comps2vis:  operators.gridder.comps2vis(method="dft") against method="grid" on the same inputs -- one time chunk, one band of
              --c2-nrow x --c2-nchan visibilities, an --npix^2 model of --ncomps components -- plan creation INCLUDED on the
              gridded side (the plan cache is cleared before every call: a chunk's plan is used once)

Prints one JSON line.  Example:  python tools/bench_dft.py
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, before=None):
    from pfb_imaging_amd import _lib

    fn()
    total = 0.0
    for _ in range(reps):
        if before is not None:
            before()
        _lib.check(_lib.lib().pfbhip_synchronize())
        t0 = time.perf_counter()
        fn()
        _lib.check(_lib.lib().pfbhip_synchronize())
        total += time.perf_counter() - t0
    return total / reps * 1e3


def ints(s):
    return [int(v) for v in s.split(",") if v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nrow", type=int, default=100000)
    ap.add_argument("--nchan", type=int, default=10)
    ap.add_argument("--nsrc", type=ints, default=[1, 64, 1024, 16384])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--npix", type=int, default=8192)
    ap.add_argument("--c2-nrow", type=int, default=1000000)
    ap.add_argument("--c2-nchan", type=int, default=10)
    ap.add_argument("--ncomps", type=ints, default=[10, 100, 1000, 10000])
    ap.add_argument("--c2-reps", type=int, default=2)
    a = ap.parse_args()

    from pfb_imaging_amd import _lib, wgridder
    from pfb_imaging_amd.dft import DFT
    from pfb_imaging_amd.operators.gridder import comps2vis

    _lib.require_gpu()
    rng = np.random.default_rng(0)
    res = dict(nvis=a.nrow * a.nchan, kernels=[], comps2vis=[])
    uvw = rng.standard_normal((a.nrow, 3)) * np.array([2000.0, 2000.0, 20.0])
    freq = np.linspace(1.0e9, 1.05e9, a.nchan)
    vis = _lib.DeviceArray.from_host(rng.standard_normal((a.nrow, a.nchan)) + 1j * rng.standard_normal((a.nrow, a.nchan)))
    with DFT(uvw, freq) as d:
        for nsrc in a.nsrc:
            lm, amp = rng.uniform(-0.02, 0.02, (nsrc, 2)), rng.standard_normal(nsrc)
            reps = a.reps if nsrc <= 1024 else max(a.reps // 3, 1)
            p_ms = timed(lambda: d.predict(lm, amp, out=vis), reps)
            i_ms = timed(lambda: d.image(lm, vis), reps)
            work = nsrc * a.nrow * a.nchan / 1e6
            res["kernels"].append(dict(nsrc=nsrc, predict_ms=p_ms, predict_gsv_s=work / p_ms, image_ms=i_ms, image_gsv_s=work / i_ms))
    vis.free()

    n = a.npix
    uvw = rng.standard_normal((a.c2_nrow, 3)) * np.array([2000.0, 2000.0, 20.0])
    freq = np.linspace(1.0e9, 1.05e9, a.c2_nchan)
    cell = 0.4 / (2 * np.abs(uvw[:, :2]).max() * freq.max() / 299792458.0)
    one = np.array([0])
    args = (uvw, np.array([0.0]), freq, one, np.array([a.c2_nrow]), one, np.array([1]), one, np.array([a.c2_nchan]))
    region = np.ones((n, n), dtype=bool)
    ident = lambda v: v  # noqa: E731
    for ncomps in a.ncomps:
        flat = np.sort(rng.choice(n * n, ncomps, replace=False))
        coeffs, b = rng.standard_normal((4, ncomps)), rng.standard_normal(4)
        mds = dict(coefficients=coeffs, location_x=flat // n, location_y=flat % n,
                   attrs=dict(cell_rad_x=cell, npix_x=n, npix_y=n, center_x=0.0, center_y=0.0, flip_u=False, flip_v=True, flip_w=False))

        def modelf(t, f, *c):
            return sum(bk * ck for bk, ck in zip(b, c))

        def run(method):
            return comps2vis(*args, region, mds, modelf, ident, ident, epsilon=1e-7, method=method)

        dft_ms = timed(lambda: run("dft"), a.c2_reps)
        grid_ms = timed(lambda: run("grid"), a.c2_reps, before=wgridder.clear_cache)
        v_dft, v_grid = run("dft"), run("grid")
        rel = float(np.linalg.norm(v_dft - v_grid) / np.linalg.norm(v_dft))
        res["comps2vis"].append(dict(ncomps=ncomps, dft_ms=dft_ms, grid_ms=grid_ms, rel_l2=rel))
    res.update(npix=n, c2_nvis=a.c2_nrow * a.c2_nchan)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
