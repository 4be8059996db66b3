"""numpy restatement of ``VisChunk.average``, the yardstick of tests/test_gpu_chunkavg.py: plain loops over
``(R, q, c)`` that can be read against the definition, every sum in ``np.longdouble``.

For output sample ``(R, q)`` let ``K`` be the input samples ``(r, k)`` with ``row_map[r] == R``, ``k`` in
``[q chan_bin, min((q + 1) chan_bin, nchan))`` and ``mask[r, k] != 0``.  Then, per correlation ``c``::

    wgt_out[c] = sum_K wgt[c, r, k]
    vis_out[c] = sum_K wgt[c, r, k] vis[c, r, k] / wgt_out[c]
    mask_out   = 1 if K is not empty else 0

``K`` empty: everything zero.  ``K`` not empty but ``wgt_out[c] == 0``: ``vis_out[c] = wgt_out[c] = 0``, ``mask_out`` stays 1.
"""

import numpy as np

LD = np.longdouble


def average(vis, wgt, mask, chan_bin, row_map=None, nrow_out=None):
    """``(vis_out, wgt_out, mask_out, absum, count)``: the first two in longdouble (complex as a trailing axis of 2: real,
    imaginary), ``absum[c, R, q] = sum_K wgt |vis|`` (what the error bounds are stated in) and ``count[R, q] = |K|``."""
    ncorr, nrow, nchan = vis.shape
    if row_map is None:
        row_map = np.arange(nrow)
    if nrow_out is None:
        nrow_out = int(row_map.max()) + 1
    nchan_out = -(-nchan // chan_bin)
    vis_out = np.zeros((ncorr, nrow_out, nchan_out, 2), dtype=LD)
    wgt_out = np.zeros((ncorr, nrow_out, nchan_out), dtype=LD)
    absum = np.zeros((ncorr, nrow_out, nchan_out), dtype=LD)
    mask_out = np.zeros((nrow_out, nchan_out), dtype=np.uint8)
    count = np.zeros((nrow_out, nchan_out), dtype=np.int64)
    rows_of = [[] for _ in range(nrow_out)]  # members in ascending input-row order
    for r in range(nrow):
        if row_map[r] >= 0:
            rows_of[row_map[r]].append(r)
    for R in range(nrow_out):
        rows = rows_of[R]
        for q in range(nchan_out):
            K = [(r, k) for r in rows for k in range(q * chan_bin, min((q + 1) * chan_bin, nchan)) if mask[r, k] != 0]
            count[R, q] = len(K)
            if not K:
                continue
            mask_out[R, q] = 1
            for c in range(ncorr):
                sw, sre, sim, sab = LD(0), LD(0), LD(0), LD(0)
                for r, k in K:
                    w, v = LD(wgt[c, r, k]), vis[c, r, k]
                    sw += w
                    sre += w * LD(v.real)
                    sim += w * LD(v.imag)
                    sab += w * np.hypot(LD(v.real), LD(v.imag))
                if sw == 0:
                    continue
                wgt_out[c, R, q] = sw
                vis_out[c, R, q] = sre / sw, sim / sw
                absum[c, R, q] = sab
    return vis_out, wgt_out, mask_out, absum, count


def to_double(vis_out, wgt_out):
    """The restatement's results rounded to complex128 / float64"""
    v = vis_out.astype(np.float64)
    return v[..., 0] + 1j * v[..., 1], wgt_out.astype(np.float64)


def channel_bins(freq, chan_bin, chan_width=None):
    nchan_out = -(-freq.size // chan_bin)
    f = np.array([np.mean(freq[q * chan_bin:(q + 1) * chan_bin]) for q in range(nchan_out)])
    w = None if chan_width is None else np.array([np.sum(chan_width[q * chan_bin:(q + 1) * chan_bin]) for q in range(nchan_out)])
    return f, w


def mean_uvw(uvw, row_map, nrow_out):
    out = np.zeros((nrow_out, 3))
    for R in range(nrow_out):
        rows = np.flatnonzero(np.asarray(row_map) == R)
        if rows.size:
            out[R] = uvw[rows].mean(axis=0)
    return out


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))
