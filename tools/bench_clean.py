"""Device Hogbom / Clark CLEAN at kclean sizes: one JSON line per case (GPU box).

Hogbom: ms per iteration and the bandwidth of the step against 3 * nband * nx * ny * 8 bytes (residual read + written, PSF window
read).  Clark (4096^2 x 8 bands, subpf 0.5): ms per major step split into psfconv / search / compaction, ms per sub-minor
iteration per path, at an active set just under and just over the LDS path's limit and at a large one.  One CPU line
(kind "port") times the numpy yardstick's Hogbom step at 2048^2 x 4.  Skies are seeded and synthetic.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pfb_imaging_amd  # noqa: E402,F401
from pfb_imaging_amd.clean import CleanPlan  # noqa: E402


def gauss_psf(nband, nxp, nyp, s0=2.0):
    x = (np.arange(nxp) - nxp // 2)[:, None]
    y = (np.arange(nyp) - nyp // 2)[None, :]
    return np.stack([np.exp(-0.5 * (x / (s0 + 0.2 * b)) ** 2 - 0.5 * (y / (s0 + 0.15 * b)) ** 2) for b in range(nband)])


def point_sky_dirty(psf, nx, ny, npts, rng):
    """sum of shifted PSFs of npts point sources plus noise: no FFT needed"""
    nband, nxp, nyp = psf.shape
    d = 0.001 * rng.standard_normal((nband, nx, ny))
    for _ in range(npts):
        i, j, f = int(rng.integers(nx // 8, 7 * nx // 8)), int(rng.integers(ny // 8, 7 * ny // 8)), rng.uniform(0.2, 1.0)
        d += f * psf[:, nxp // 2 - i:nxp // 2 - i + nx, nyp // 2 - j:nyp // 2 - j + ny]
    return d


def blob_dirty(nband, nx, ny, sigma):
    x = (np.arange(nx) - nx // 2)[:, None]
    y = (np.arange(ny) - ny // 2)[None, :]
    return np.exp(-0.5 * (x * x + y * y) / sigma**2)[None].repeat(nband, 0) * np.linspace(1.0, 0.8, nband)[:, None, None]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def hogbom_case(n, nband, iters, rng):
    psf = gauss_psf(nband, 2 * n, 2 * n)
    dirty = point_sky_dirty(psf, n, n, 50, rng)
    plan = CleanPlan(psf, None, n, n)
    plan.hogbom(dirty, gamma=0.1, pf=1e-9, maxit=10)  # warm-up
    plan.hogbom(dirty, gamma=0.1, pf=1e-9, maxit=iters)
    info = plan.info
    ms = info["loop_ms"] / max(info["iters"], 1)
    nbytes = 3 * nband * n * n * 8
    emit(kind="device", case=f"hogbom_{n}x{n}x{nband}", iters=info["iters"], ms_per_iter=round(ms, 4),
         GBps=round(nbytes / (ms * 1e-3) / 1e9, 1), bytes_per_iter=nbytes, idle_launches=info["idle_launches"])
    plan.close()


def clark_case(n, nband, label, dirty, psf, psfhat, maxit, submaxit):
    w = np.full(nband, 1.0 / nband)
    mask = np.ones((n, n))
    plan = CleanPlan(psf, psfhat, n, n)
    plan.clark(dirty, w, mask, gamma=0.05, pf=1e-9, maxit=1, subpf=0.5, submaxit=5)  # warm-up
    plan.clark(dirty, w, mask, gamma=0.05, pf=1e-9, maxit=maxit, subpf=0.5, submaxit=submaxit)
    i = plan.info
    nmaj = i["iters"] + 1  # the initial search / active set plus one per major iteration
    emit(kind="device", case=f"clark_{n}x{n}x{nband}_{label}", major_iters=i["iters"], minor_iters=i["minor_iters"],
         nsub_lds=i["nsub_lds"], nsub_grid=i["nsub_grid"],
         ms_psfconv_per_major=round(i["conv_ms"] / max(i["iters"], 1), 3), ms_search_per_major=round(i["search_ms"] / nmaj, 3),
         ms_compact_per_major=round(i["compact_ms"] / nmaj, 3),
         us_per_sub_iter_lds=round(1e3 * i["sub_lds_ms"] / i["minor_iters"], 2) if i["nsub_lds"] else None,
         us_per_sub_iter_grid=round(1e3 * i["sub_grid_ms"] / i["minor_iters"], 2) if i["nsub_grid"] else None,
         idle_launches=i["idle_launches"], loop_ms=round(i["loop_ms"], 1))
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal)")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    big, nb = (512, 2) if a.quick else (4096, 8)
    hogbom_case(256 if a.quick else 2048, 2 if a.quick else 4, 50 if a.quick else 200, rng)
    hogbom_case(big, nb, 50 if a.quick else 200, rng)
    psf = gauss_psf(nb, 2 * big, 2 * big)
    psfhat = np.fft.rfft2(np.fft.ifftshift(psf, axes=(1, 2)), axes=(1, 2))
    lds_max = 96 * 1024 // (8 * nb)
    # a Gaussian blob keeps ~4.36 sigma^2 pixels above half its peak: active sets just under / over the LDS limit, and large
    for label, a_target in (("A_lds", 0.9 * lds_max), ("A_grid_small", 1.15 * lds_max), ("A_large", 40000)):
        sigma = np.sqrt(a_target / (2 * np.pi * np.log(2)))
        clark_case(big, nb, label, blob_dirty(nb, big, big, sigma), psf, psfhat, 1, 200)
    clark_case(big, nb, "points", point_sky_dirty(psf, big, big, 30, rng), psf, psfhat, 5, 200)
    # the numpy yardstick's Hogbom step on the CPU (a port of the algorithm, not the reference's numba code)
    from tests import _clean_ref as ref

    n, nband = (256, 2) if a.quick else (2048, 4)
    p = gauss_psf(nband, 2 * n, 2 * n)
    d = point_sky_dirty(p, n, n, 20, rng)
    t0 = time.perf_counter()
    ref.hogbom(d, p, gamma=0.1, pf=1e-9, maxit=3)
    emit(kind="port", case=f"hogbom_{n}x{n}x{nband}_numpy_yardstick", ms_per_iter=round((time.perf_counter() - t0) * 1e3 / 3, 1))


if __name__ == "__main__":
    main()
