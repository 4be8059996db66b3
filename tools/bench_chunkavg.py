"""Times ``pfbhip_chunk_average_dev`` (``VisChunk.average``, csrc/chunkavg.hip) on a resident chunk against a device copy of
the same byte count and against the host way (download, numpy averaging, upload), and the product chain on the averaged
chunk against the unaveraged one.  DESIGN §17.4's protocol: one process, the paths alternate after one untimed run of each,
host clock around calls that return with their streams idle, median (min - max) of ``--repeats``.  Bytes are counted from
the shapes: every input sample ``ncorr * 24 + 1`` read once, every output sample ``ncorr * 24 + 1`` written once.

    python tools/bench_chunkavg.py [--nrow 156250 --nchan 64 --ncorr 4 --npix 8192 --repeats 5 --out FILE]
"""

import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(ts.min()), 3), max_ms=round(float(ts.max()), 3), n=len(ts))


def host_average(vis, wgt, mask, chan_bin, rows_per_bin):
    """What a caller does without the entry: numpy sums over channel bins (``np.add.reduceat``) and over ``rows_per_bin``
    consecutive rows, masked samples left out; the semantics of ``VisChunk.average``"""
    live = mask != 0
    w = np.where(live, wgt, 0.0)
    wv = w * vis
    cnt = live.astype(np.int64)
    if chan_bin > 1:
        starts = np.arange(0, mask.shape[1], chan_bin)
        w, wv, cnt = (np.add.reduceat(a, starts, axis=-1) for a in (w, wv, cnt))
    if rows_per_bin > 1:
        starts = np.arange(0, mask.shape[0], rows_per_bin)
        w, wv, cnt = (np.add.reduceat(a, starts, axis=-2) for a in (w, wv, cnt))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(w != 0, wv / w, 0.0)
    return v, w, (cnt > 0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nrow", type=int, default=156_250)
    ap.add_argument("--nchan", type=int, default=64)
    ap.add_argument("--ncorr", type=int, default=4)
    ap.add_argument("--npix", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from pfb_imaging_amd import _lib
    from pfb_imaging_amd._lib import DeviceArray, check, lib, ptr
    from pfb_imaging_amd.operators.gridder import image_data_products_chunk
    from pfb_imaging_amd.utils import synth
    from pfb_imaging_amd.vischunk import VisChunk, row_bins

    _lib.require_gpu()
    ncorr, nrow, nchan = a.ncorr, a.nrow, a.nchan
    c = synth.make_case(nrow, nchan, a.npix, seed=2002, with_vis=False)  # C2's sample count at 64 channels by default
    rng = np.random.default_rng(17)
    vis = np.exp(2j * np.pi * rng.random((ncorr, nrow, nchan)))
    wgt = rng.uniform(0.5, 2.0, (ncorr, nrow, nchan))
    mask = (rng.random((nrow, nchan)) > 0.05).astype(np.uint8)
    per_sample = ncorr * 24 + 1
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    ch = VisChunk(c["uvw"], c["freq"], vis, wgt, mask)
    settings = [(2, 1), (8, 1), (16, 1), (1, 4)]  # (chan_bin, rows per bin)
    for chan_bin, rpb in settings:
        nrow_out, nchan_out = -(-nrow // rpb), -(-nchan // chan_bin)
        rs = mem = None
        if rpb > 1:
            rs, mem, _ = row_bins(np.arange(nrow) // rpb, nrow)
        moved = (nrow * nchan + nrow_out * nchan_out) * per_sample
        outs = [DeviceArray((ncorr, nrow_out, nchan_out), np.complex128), DeviceArray((ncorr, nrow_out, nchan_out), np.float64),
                DeviceArray((nrow_out, nchan_out), np.uint8)]
        src, dst = DeviceArray(moved // 2, np.uint8), DeviceArray(moved // 2, np.uint8)  # a copy reads and writes: half each
        src.zero()

        def entry():
            check(lib().pfbhip_chunk_average_dev(ch.vis.ptr, ch.wgt.ptr, ch.mask.ptr, ncorr, nrow, nchan, chan_bin, ptr(rs), ptr(mem),
                                                 nrow if mem is None else mem.size, nrow_out, outs[0].ptr, outs[1].ptr, outs[2].ptr))

        def copy():
            check(lib().pfbhip_memcpy_d2d(dst.ptr, src.ptr, ct.c_size_t(moved // 2)))
            check(lib().pfbhip_synchronize())

        def host():
            hv, hw, hm = host_average(ch.vis.download(), ch.wgt.download(), ch.mask.download(), chan_bin, rpb)
            made = [DeviceArray.from_host(x) for x in (hv, hw, hm)]
            for d in made:
                d.free()
            return hv, hw, hm

        te, tc, th = [], [], []
        for it in range(a.repeats + 1):  # (iteration 0 warms every path up)
            for fn, ts in ((entry, te), (copy, tc), (host, th)):
                t0 = time.perf_counter()
                res = fn()
                t1 = time.perf_counter()
                if it:
                    ts.append(t1 - t0)
                elif fn is host:
                    gv = outs[0].download()
                    worst = float(np.abs(gv - res[0]).max())
                    assert np.array_equal(outs[2].download(), res[2])
                res = None  # (the host result is freed outside the next timed window)
        e, cp = stats(te), stats(tc)
        emit(dict(what="average", chan_bin=chan_bin, rows_per_bin=rpb, ncorr=ncorr, nrow=nrow, nchan=nchan, bytes=moved, entry=e,
                  entry_GBps=round(moved / e["median_ms"] / 1e6, 1), copy=cp, copy_GBps=round(moved / cp["median_ms"] / 1e6, 1),
                  entry_over_copy_rate=round(cp["median_ms"] / e["median_ms"], 3), host=stats(th), max_abs_vis_diff_vs_host=worst))
        for d in outs + [src, dst]:
            d.free()

    if not a.no_chain:
        geom = (a.npix, a.npix, 2 * a.npix, 2 * a.npix, c["cell"], c["cell"])
        kw = dict(do_psf=False)
        for chan_bin in (1, 2, 8, 16):
            ts = []
            for it in range(a.repeats + 1):
                av = ch.average(chan_bin) if chan_bin > 1 else VisChunk(c["uvw"], c["freq"], vis, wgt, mask)
                t0 = time.perf_counter()
                image_data_products_chunk(av, *geom, **kw)
                t1 = time.perf_counter()
                av.close()
                if it:
                    ts.append(t1 - t0)
            emit(dict(what="chain, natural weights, no PSF", chan_bin=chan_bin, nx=a.npix, nvis=nrow * (-(-nchan // chan_bin)), **stats(ts)))
    ch.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
