#!/usr/bin/env python3
"""Timings of the Gaussian-resolution convolution and the restore step for DESIGN.md §12 (not part of bench.py, not a test
threshold).

For each --npix at --nband bands and pfrac = 0.2: ms per call of ``convolve2gaussres`` / ``restore_arrays`` on host arrays and of
``GaussConvPlan.apply_dev`` / ``restore_dev`` on device-resident cubes, plans warm.  ``--port`` adds the numpy composition of
tests/_restore_ref.py on the host as the yardstick, labelled ``kind: "port"`` (ducc0 is not installed: its speed is unknown).
Per-kernel times come from running this script under ``rocprofv3 --kernel-trace --stats`` with ``--dev-only``.

Prints one JSON line per size.  Example:  python tools/bench_restore.py --npix 4096 8192 --nband 8 --port
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npix", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--nband", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dev-only", action="store_true")
    ap.add_argument("--port", action="store_true")
    a = ap.parse_args()

    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.gaussconv import cached_plan, clear_cache
    from pfb_imaging_amd.utils.misc import convolve2gaussres
    from pfb_imaging_amd.utils.restoration import restore_arrays

    _lib.require_gpu()
    rng = np.random.default_rng(0)
    for n in a.npix:
        nb = a.nband
        model = np.zeros((nb, n, n))
        model[:, rng.integers(0, n, 2000), rng.integers(0, n, 2000)] = 1.0
        residual = rng.standard_normal((nb, n, n))
        wsum = np.linspace(1.0, 2.0, nb)
        pari = np.stack([np.linspace(2.5, 3.0, nb), np.linspace(2.0, 2.4, nb), np.linspace(0.0, 1.0, nb)], axis=1)
        parf = np.array([6.0, 5.0, 0.3])
        off = -(n // 2) + np.arange(n)
        xx, yy = np.meshgrid(off, off, indexing="ij")
        plan = cached_plan(nb, n, n, 0.2)
        res = dict(npix=n, nband=nb, pfrac=0.2, nfft=[plan.nfft_x, plan.nfft_y])
        m_dev, r_dev, o_dev = _lib.DeviceArray.from_host(model), _lib.DeviceArray.from_host(residual), _lib.DeviceArray((nb, n, n))
        res["convolve_dev_ms"] = timed(lambda: plan.apply_dev(m_dev, o_dev, parf), a.reps)
        res["convolve_ratio_dev_ms"] = timed(lambda: plan.apply_dev(r_dev, o_dev, parf, pari), a.reps)
        res["restore_dev_ms"] = timed(lambda: plan.restore_dev(m_dev, r_dev, o_dev, wsum, pari, parf), a.reps)
        for d in (m_dev, r_dev, o_dev):
            d.free()
        if not a.dev_only:
            res["convolve2gaussres_ms"] = timed(lambda: convolve2gaussres(model, xx, yy, parf, pfrac=0.2), a.reps)
            res["restore_arrays_ms"] = timed(lambda: restore_arrays(model, residual, wsum, pari, parf), a.reps)
        print(json.dumps(res), flush=True)
        if a.port:
            from tests import _restore_ref as ref

            t0 = time.perf_counter()
            ref.convolve(model, xx, yy, parf, pfrac=0.2)
            t1 = time.perf_counter()
            ref.restore(model, residual, wsum, pari, parf)
            t2 = time.perf_counter()
            print(json.dumps(dict(kind="port", what="tests/_restore_ref.py (numpy.fft, one thread)", npix=n, nband=nb,
                                  convolve_ms=(t1 - t0) * 1e3, restore_ms=(t2 - t1) * 1e3)), flush=True)
        clear_cache()


if __name__ == "__main__":
    main()
