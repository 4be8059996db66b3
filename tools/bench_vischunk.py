"""Times the product chain of one (time, band) chunk both ways: ``image_data_products_arrays`` (host arrays, uploads per
correlation and per product) against ``image_data_products_chunk`` on a :class:`VisChunk` that is already resident, and the
upload that builds the chunk.  The two paths alternate inside one process, after a warm-up of each; every timed call ends
in a device synchronise (each library entry returns with its stream idle).  Prints one JSON line per setting and the bytes
each path moves over PCIe, counted from the shapes (``pcie_bytes``).

    python tools/bench_vischunk.py --config C2 --ncorr 4 --repeats 5 [--out FILE]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pcie_bytes(ncorr, nvis, nrow, nx, ny, nx_psf, ny_psf, model, robust, do_psf, do_weight=True):
    """(arrays path, chunk path) bytes over PCIe for one chain run, plan creation (uvw, freq, mask: the same on both) left
    out.  Per sample: visibilities 16, weights 8, mask 1."""
    img, psf = nx * ny * 8, nx_psf * ny_psf * 8
    psfhat = nx_psf * (ny_psf // 2 + 1) * 16
    a = c = 0
    if model:
        a += ncorr * (img + nvis * 16)          # model up, model visibilities down
        c += ncorr * img                        # model up
    if robust:
        a += nrow * 24 + nvis * (1 + 2 * ncorr * 8)  # uvw, mask, weights up; weights down
        c += nrow * 24                          # uvw up
    c += ncorr * 8                              # WSUM down
    if do_weight:
        c += ncorr * nvis * 8                   # WEIGHT down
    a += ncorr * (nvis * 24 + img)              # DIRTY: visibilities and weights up, image down
    c += ncorr * img
    if model:
        a += ncorr * (nvis * 24 + img)          # RESIDUAL
        c += ncorr * img
    if do_psf:
        a += ncorr * (nvis * 24 + psf)          # PSF visibilities and weights up, image down
        c += ncorr * psf
        a += ncorr * (psf + psfhat)             # PSFHAT: fft.r2c takes and returns host arrays, on both paths
        c += ncorr * (psf + psfhat)
    return a, c


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(min_ms=round(float(ts.min()), 2), median_ms=round(float(np.median(ts)), 2), max_ms=round(float(ts.max()), 2), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--ncorr", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--psf-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from pfb_imaging_amd import _lib
    from pfb_imaging_amd.operators.gridder import image_data_products_arrays, image_data_products_chunk
    from pfb_imaging_amd.utils import synth
    from pfb_imaging_amd.vischunk import VisChunk

    if a.config in synth.CONFIGS:
        c = synth.make_config(a.config)
    else:
        nrow, nchan, npix = (int(v) for v in a.config.split(","))
        c = synth.make_case(nrow, nchan, npix, seed=1)
    _lib.require_gpu()
    rng = np.random.default_rng(17)
    ncorr, nx, ny = a.ncorr, c["nx"], c["ny"]
    nrow, nchan = c["mask"].shape
    nvis = nrow * nchan
    vis = np.stack([c["vis"] * (1.0 + 0.1 * k) for k in range(ncorr)])
    wgt = np.stack([c["wgt"] * (1.0 + 0.05 * k) for k in range(ncorr)])
    model = np.zeros((ncorr, nx, ny))
    model[:, rng.integers(0, nx, 200), rng.integers(0, ny, 200)] = rng.random((ncorr, 200))
    geom = (nx, ny, 2 * nx, 2 * ny, c["cell"], c["cell"])
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    t0 = time.perf_counter()
    ch = VisChunk(c["uvw"], c["freq"], vis, wgt, c["mask"])
    first_upload = time.perf_counter() - t0
    ch.close()
    ups = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ch = VisChunk(c["uvw"], c["freq"], vis, wgt, c["mask"])
        ups.append(time.perf_counter() - t0)
        ch.close()
    emit(dict(what="chunk upload", config=a.config, ncorr=ncorr, nvis=nvis, bytes=nvis * (ncorr * 24 + 1), first_ms=round(first_upload * 1e3, 2),
              **stats(ups)))

    settings = [("natural", None, False, a.repeats), ("robust0", 0.0, False, a.repeats), ("natural+psf", None, True, a.psf_repeats)]
    for name, robust, do_psf, reps in settings:
        kw = dict(model=model, robustness=robust, do_psf=do_psf)
        ta, tc, tu = [], [], []
        worst = 0.0
        for it in range(reps + 1):  # (iteration 0 warms both paths up)
            t0 = time.perf_counter()
            pa, _ = image_data_products_arrays(c["uvw"], c["freq"], vis, wgt, c["mask"], *geom, **kw)
            t1 = time.perf_counter()
            ch = VisChunk(c["uvw"], c["freq"], vis, wgt, c["mask"])  # (the chain changes the chunk's weights: a fresh one per run)
            t2 = time.perf_counter()
            pc, _ = image_data_products_chunk(ch, *geom, **kw)
            t3 = time.perf_counter()
            ch.close()
            if it == 0:
                for key in ("DIRTY", "RESIDUAL") + (("PSF",) if do_psf else ()):
                    worst = max(worst, float(np.linalg.norm(pc[key] - pa[key]) / np.linalg.norm(pa[key])))
            else:
                ta.append(t1 - t0)
                tu.append(t2 - t1)
                tc.append(t3 - t2)
            del pa, pc
        ba, bc = pcie_bytes(ncorr, nvis, nrow, nx, ny, 2 * nx, 2 * ny, True, robust is not None, do_psf)
        emit(dict(what="chain", setting=name, config=a.config, ncorr=ncorr, nx=nx, nvis=nvis, arrays=stats(ta), chunk=stats(tc),
                  chunk_upload=stats(tu), arrays_pcie_bytes=ba, chunk_pcie_bytes=bc, chunk_build_bytes=nvis * (ncorr * 24 + 1),
                  max_rel_l2_chunk_vs_arrays=worst))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
