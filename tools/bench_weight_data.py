#!/usr/bin/env python3
"""Rate of the weight_data kernel for DESIGN.md §16 (not part of bench.py, not a test threshold).

For each case -- nc = 4, ns = 1, diagonal Jones and nc = 4, ns = 4, full Jones, double precision, --nrow x --nchan samples
(10^7 by default), --nant antennas, --ntime Jones time slots, 5 % of the samples flagged -- the time of one warm launch of
the kernel between device events (the smallest of --reps calls), the bytes that launch has to move
(nc (16 + 8 + 1) read and ns 24 written per sample, plus the Jones terms once), and in the same process the time of a
16-byte-per-lane device copy of the same byte count (half read, half written).  The CPU figure is this repository's numpy
oracle (tests/_stokes_ref.py) on a --cpu-frac share of the samples, NOT the reference's numba kernel, which is not
installed where this was written.

Prints one JSON line.  Example:  python tools/bench_weight_data.py
"""

import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nrow", type=int, default=10000)
    ap.add_argument("--nchan", type=int, default=1000)
    ap.add_argument("--nant", type=int, default=64)
    ap.add_argument("--ntime", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-frac", type=float, default=0.01)
    a = ap.parse_args()

    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.utils.weighting import weight_data_dev
    from tests import _stokes_ref as ref

    _lib.require_gpu()
    rng = np.random.default_rng(0)
    nrow, nchan, n = a.nrow, a.nchan, a.nrow * a.nchan
    data = (rng.standard_normal((nrow, nchan, 4)) + 1j * rng.standard_normal((nrow, nchan, 4)))
    weight = rng.uniform(0.1, 2.0, (nrow, nchan, 4))
    flag = rng.random((nrow, nchan, 4)) < 0.0127  # any of four: 5 %
    per = nrow // a.ntime
    tbin_idx, tbin_counts = np.arange(a.ntime) * per, np.full(a.ntime, per)
    tbin_counts[-1] = nrow - tbin_idx[-1]
    ant1, ant2 = rng.integers(0, a.nant, nrow).astype(np.int32), rng.integers(0, a.nant, nrow).astype(np.int32)
    out = {"nsamples": n, "nrow": nrow, "nchan": nchan, "cases": []}
    for name, full, product in (("nc4_ns1_diag", False, "I"), ("nc4_ns4_full", True, "IQUV")):
        jones = ref.random_jones(rng, (a.ntime, a.nant, nchan, 1), full)
        ns = len(product)
        nbytes = n * (4 * 25 + ns * 24) + jones.nbytes  # (every sample reads two Jones terms, from an array that stays in cache)
        times = []
        for _ in range(a.reps):
            info = {}
            vis, wgt, _ = weight_data_dev(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, "linear", product, "4", "l2",
                                          corr_first=False, with_mask=False, info=info)
            times.append(info["device_ms"])
            vis.free(), wgt.free()
        ms = ct.c_double(0.0)
        copy_bytes = (nbytes // 32) * 32
        _lib.check(_lib.lib().pfbhip_debug_copy16(ct.c_int64(copy_bytes // 2), ct.c_int32(10), ct.byref(ms)))
        sub = max(int(nrow * a.cpu_frac), 1)
        t0 = time.perf_counter()
        ref.weight_data(data[:sub], weight[:sub], flag[:sub], jones, tbin_idx[:1], np.array([sub]), ant1[:sub], ant2[:sub], "linear",
                        product)
        cpu_ms = (time.perf_counter() - t0) * 1e3 * nrow / sub
        k = min(times)
        out["cases"].append({"case": name, "kernel_ms": k, "kernel_ms_all": times, "bytes": nbytes, "kernel_TBps": nbytes / k / 1e9,
                             "copy16_ms": ms.value, "copy16_TBps": copy_bytes / ms.value / 1e9, "kernel_over_copy": k / ms.value,
                             "numpy_oracle_ms_extrapolated": cpu_ms})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
