#!/usr/bin/env python3
"""Timings of the component-model path for DESIGN.md §11 (not part of bench.py, not a test threshold).

  render / regrid:  device time and achieved GB/s of Comps.render_dev and comps.regrid_dev at --npix^2 with --ncomps
                    components and --nparam parameters (bytes as counted in DESIGN.md §11)
  comps2vis:        one (time chunk, band) of operators.gridder.comps2vis against the host composition it replaces
                    (numpy render + the stateless dirty2vis), plans warm in both

Prints one JSON line.  Example:  python tools/bench_comps.py --npix 8192 --ncomps 100000 --nparam 6 --nrow 1000000 --nchan 10
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    from pfb_imaging_amd import _lib

    fn()
    _lib.check(_lib.lib().pfbhip_synchronize())
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    _lib.check(_lib.lib().pfbhip_synchronize())
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npix", type=int, default=8192)
    ap.add_argument("--ncomps", type=int, default=100000)
    ap.add_argument("--nparam", type=int, default=6)
    ap.add_argument("--nrow", type=int, default=1000000)
    ap.add_argument("--nchan", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()

    from pfb_imaging_amd import _lib, wgridder
    from pfb_imaging_amd.comps import Comps, regrid_dev
    from pfb_imaging_amd.operators.gridder import comps2vis

    _lib.require_gpu()
    rng = np.random.default_rng(0)
    n = a.npix
    flat = np.sort(rng.choice(n * n, a.ncomps, replace=False))
    xi, yi = flat // n, flat % n
    coeffs = rng.standard_normal((a.nparam, a.ncomps))
    b = rng.standard_normal(a.nparam)
    comps = Comps(n, n, xi, yi, coeffs)
    img, out = _lib.DeviceArray((n, n)), _lib.DeviceArray((n, n))
    res = dict(npix=n, ncomps=a.ncomps, nparam=a.nparam)
    ms = timed(lambda: comps.render_dev(b, img), a.reps)
    nbytes = 8 * n * n + a.ncomps * (16 + 8 * a.nparam)
    res.update(render_ms=ms, render_gbs=nbytes / ms / 1e6)
    cell = 1e-6
    ms = timed(lambda: regrid_dev(img, cell, cell, 0.0, 0.0, out, 0.99 * cell, 0.99 * cell, 0.3 * cell, -0.2 * cell), a.reps)
    res.update(regrid_ms=ms, regrid_gbs=16 * n * n / ms / 1e6)  # (one read of the input through the caches, one write)
    comps.close()

    # one (time chunk, band) of comps2vis against the host composition
    uvw = rng.standard_normal((a.nrow, 3)) * np.array([2000.0, 2000.0, 20.0])
    freq = np.linspace(1.0e9, 1.05e9, a.nchan)
    ccell = 0.4 / (2 * np.abs(uvw[:, :2]).max() * freq.max() / 299792458.0)
    one = np.array([0])
    args = (uvw, np.array([0.0]), freq, one, np.array([a.nrow]), one, np.array([1]), one, np.array([a.nchan]))
    mds = dict(coefficients=coeffs, location_x=xi, location_y=yi,
               attrs=dict(cell_rad_x=ccell, npix_x=n, npix_y=n, center_x=0.0, center_y=0.0, flip_u=False, flip_v=True, flip_w=False))
    region = np.ones((n, n), dtype=bool)

    def modelf(t, f, *c):
        return sum(bk * ck for bk, ck in zip(b, c))

    ident = lambda v: v  # noqa: E731

    def device():
        return comps2vis(*args, region, mds, modelf, ident, ident, epsilon=1e-7)

    def host():
        image = np.zeros((n, n))
        image[xi, yi] = modelf(0.0, 0.0, *coeffs)
        image = np.where(region, image, 0.0)
        return wgridder.dirty2vis(uvw=uvw, freq=freq, dirty=image, pixsize_x=ccell, pixsize_y=ccell, epsilon=1e-7, flip_v=True,
                                  do_wgridding=True, divide_by_n=False)

    res.update(nrow=a.nrow, nchan=a.nchan, comps2vis_ms=timed(device, max(a.reps // 3, 1)),
               host_composition_ms=timed(host, max(a.reps // 3, 1)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
