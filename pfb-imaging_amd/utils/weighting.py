"""uv-cell counts and Briggs weights on the GPU.

Mirrors /root/reference/src/pfb_imaging/utils/weighting.py: ``_compute_counts`` (:81-140) and
``counts_to_weights`` (:143-208).  The integer uv-cell index is bit-exact against the CPU
oracle; the counts are a sorted, segmented sum without atomics: they agree with the reference to summation order and are
bit-identical from call to call.

``weight_data`` (:274-468) forms the Stokes visibilities and weights the rest consumes (csrc/stokes.hip).
"""

import ctypes as ct

import numpy as np

from .. import _lib
from .._lib import as_c, check, f64, i32, lib, ptr


def uvcell_index(uvw, freq, mask, nx, ny, cell_size_x, cell_size_y, usign=1.0, vsign=-1.0):
    """Flat index ``u_idx*ny + v_idx`` per visibility, -1 when masked or out of bounds."""
    _lib.require_gpu()
    uvw, freq, mask = as_c(uvw, np.float64), as_c(freq, np.float64), as_c(mask, np.uint8)
    nrow, nchan = mask.shape
    cell = np.empty((nrow, nchan), dtype=np.int64)
    check(lib().pfbhip_uvcell_index(ptr(uvw), ptr(freq), ptr(mask), nrow, nchan, nx, ny, cell_size_x, cell_size_y, usign, vsign,
                                    ptr(cell)))
    return cell


def _compute_counts(uvw, freq, mask, wgt, nx, ny, cell_size_x, cell_size_y, dtype, ngrid=1, usign=1.0, vsign=-1.0):
    """weighting.py:81-140.  ``ngrid`` (private per-thread grids on the CPU) is irrelevant here."""
    _lib.require_gpu()
    uvw, freq, mask = as_c(uvw, np.float64), as_c(freq, np.float64), as_c(mask, np.uint8)
    wgt = as_c(wgt, np.float64)
    ncorr, nrow, nchan = wgt.shape
    counts = np.zeros((ncorr, nx, ny), dtype=np.float64)
    check(lib().pfbhip_compute_counts(ptr(uvw), ptr(freq), ptr(mask), ptr(wgt), ncorr, nrow, nchan, nx, ny, cell_size_x,
                                      cell_size_y, usign, vsign, ptr(counts)))
    return counts.astype(dtype, copy=False)


def counts_to_weights(counts, uvw, freq, weight, mask, nx, ny, cell_size_x, cell_size_y, robust, usign=1.0,
                      vsign=-1.0):
    """weighting.py:143-208; mutates ``counts`` and ``weight`` in place like the reference."""
    if not counts.any():
        return weight
    _lib.require_gpu()
    ncorr, nrow, nchan = weight.shape
    if robust > -2:
        numsqrt = 5 * 10 ** (-robust)
        avgwnum = (counts.reshape(ncorr, -1) ** 2).sum(axis=1)
        avgwden = counts.reshape(ncorr, -1).sum(axis=1)
        # a dead plane (all-zero counts) beside a live one is the reference's 0 / 0: NaN counts, weights left alone
        with np.errstate(invalid="ignore", divide="ignore"):
            ssq = numsqrt * numsqrt * avgwden / avgwnum
        counts *= ssq[:, None, None]
        counts += 1
    uvw, freq, mask = as_c(uvw, np.float64), as_c(freq, np.float64), as_c(mask, np.uint8)
    w = weight if (weight.flags.c_contiguous and weight.dtype == np.float64) else np.array(weight, dtype=np.float64)
    c = as_c(counts, np.float64)
    check(lib().pfbhip_counts_divide(ptr(uvw), ptr(freq), ptr(mask), ptr(c), ncorr, nrow, nchan, nx, ny, cell_size_x, cell_size_y,
                                     usign, vsign, ptr(w)))
    if w is not weight:
        weight[...] = w
    return weight


def filter_extreme_counts(counts, level=10.0):
    """weighting.py:212-226: positive counts below ``median(positive)/level`` are raised to it (in place)."""
    if not level:
        return counts
    _lib.require_gpu()
    c = counts if (counts.flags.c_contiguous and counts.dtype == np.float64) else np.array(counts, dtype=np.float64)
    check(lib().pfbhip_filter_extreme_counts(ptr(c), c.size, level, None))
    if c is not counts:
        counts[...] = c
    return counts


def box_sum_counts(counts, npix_super):
    """weighting.py:229-254: (2 npix_super + 1)^2 box sum with zero padding; identity when disabled."""
    if npix_super is None or npix_super <= 0:
        return counts
    assert np.issubdtype(counts.dtype, np.floating), (
        f"box_sum_counts requires a floating-point counts array; got dtype={counts.dtype}"
    )
    _lib.require_gpu()
    c = as_c(counts, np.float64)
    ncorr, nx, ny = c.shape
    out = _lib.result_empty(c.shape, np.float64)
    check(lib().pfbhip_box_sum_counts(ptr(c), ncorr, nx, ny, int(npix_super), ptr(out)))
    return out.astype(counts.dtype, copy=False)


def imaging_weights(uvw, freq, mask, weight, nx_pad, ny_pad, cell_size_x, cell_size_y, robust, filter_level=5.0,
                    npix_super=0, usign=1.0, vsign=-1.0, return_counts=False):
    """The whole imaging-weight chain of ``image_data_products`` (operators/gridder.py:534-576) in one device pipeline:
    ``_compute_counts`` -> ``filter_extreme_counts`` -> ``box_sum_counts`` -> ``counts_to_weights``.  ``weight``
    ``(ncorr, nrow, nchan)`` is updated in place and returned (with the final counts when ``return_counts``); the counts
    grid never visits the host otherwise and uvw / mask / weights are uploaded once instead of three times."""
    _lib.require_gpu()
    uvw, freq, mask = as_c(uvw, np.float64), as_c(freq, np.float64), as_c(mask, np.uint8)
    ncorr, nrow, nchan = weight.shape
    w = weight if (weight.flags.c_contiguous and weight.dtype == np.float64) else np.array(weight, dtype=np.float64)
    counts = _lib.result_empty((ncorr, nx_pad, ny_pad), np.float64) if return_counts else None
    check(lib().pfbhip_imaging_weights(ptr(uvw), ptr(freq), ptr(mask), ptr(w), ncorr, nrow, nchan, nx_pad, ny_pad, cell_size_x,
                                       cell_size_y, usign, vsign, robust, filter_level or 0.0, int(npix_super or 0), ptr(counts)))
    if w is not weight:
        weight[...] = w
    return (weight, counts) if return_counts else weight


def as_contiguous_readonly_view(a):
    """A C-contiguous view of ``a`` that cannot be written through; a copy only where ``a`` is not contiguous
    (weighting.py:508-520: how the reference's callers hand their arrays to ``weight_data``)."""
    v = np.ascontiguousarray(a).view()
    v.flags.writeable = False
    return v


def _antennas(ant, nrow, name):
    ant = np.asarray(ant)
    if ant.shape != (nrow,):
        raise ValueError(f"{name} {ant.shape} != {(nrow,)}")
    if ant.dtype.kind not in "iu":
        raise TypeError(f"{name} must be an integer array, not {ant.dtype}")
    if ant.dtype != np.int32:
        # (the library checks the range against nant; this keeps a wide index from wrapping into it)
        if ant.size and (int(ant.min()) < -(2**31) or int(ant.max()) >= 2**31):
            raise ValueError(f"{name} holds indices that are no antenna numbers")
    return as_c(ant, np.int32)


def _weight_data_args(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, nc, wgt_mode, corr_first):
    """Everything ``weight_data`` and ``weight_data_dev`` check and convert before the library is called."""
    from .stokes import STOKES, stokes_products

    data, jones = np.asarray(data), np.asarray(jones)
    chosen = stokes_products(product, pol, nc, wgt_mode, jones.ndim)
    ncorr = int(nc)
    if data.ndim != 3 or data.shape[2] != ncorr:
        raise ValueError(f"data {data.shape} must be (nrow, nchan, {ncorr})")
    if data.dtype not in (np.complex64, np.complex128):
        raise TypeError(f"data must be complex64 or complex128, not {data.dtype}")
    single = data.dtype == np.complex64
    nrow, nchan, _ = data.shape
    weight, flag = np.asarray(weight), np.asarray(flag)
    if weight.shape != data.shape or flag.shape != data.shape:
        raise ValueError(f"weight {weight.shape} and flag {flag.shape} must have the shape of data {data.shape}")
    full = jones.ndim == 6
    if jones.shape[2] != nchan or jones.shape[3] < 1 or jones.shape[4:] != ((2, 2) if full else (2,)):
        raise ValueError(f"jones {jones.shape} must be (ntime, nant, {nchan}, ndir, {'2, 2' if full else '2'})")
    ntime, nant = jones.shape[:2]
    if nant < 1:
        raise ValueError("jones has no antennas")
    tbin_idx, tbin_counts = as_c(tbin_idx, np.int64), as_c(tbin_counts, np.int64)
    if tbin_idx.ndim != 1 or tbin_idx.shape != tbin_counts.shape:
        raise ValueError(f"tbin_idx {tbin_idx.shape} and tbin_counts {tbin_counts.shape} must be equal-length vectors")
    if not chosen:
        raise ValueError(f"product {product!r} selects no Stokes parameter")
    # The library refuses bad indices itself (pfbhip_weight_data); the same checks here come before the device entry
    # allocates its outputs.
    if tbin_idx.size > ntime:
        raise ValueError(f"jones has {ntime} time slots for {tbin_idx.size} time bins")
    start = tbin_idx - tbin_idx.min() if tbin_idx.size else tbin_idx
    bad = np.flatnonzero((tbin_counts < 0) | (start + tbin_counts > nrow))
    if bad.size:
        t = int(bad[0])
        raise ValueError(f"time bin {t} covers rows [{start[t]}, {start[t] + tbin_counts[t]}) of {nrow}")
    edges = np.zeros(nrow + 1, dtype=np.int64)
    np.add.at(edges, start, 1)
    np.add.at(edges, start + tbin_counts, -1)
    covered = np.cumsum(edges)[:nrow] > 0
    for name, ant in (("ant1", ant1), ("ant2", ant2)):
        a = np.asarray(ant)
        if a.shape == (nrow,) and a.dtype.kind in "iu" and ((a[covered] < 0) | (a[covered] >= nant)).any():
            raise ValueError(f"{name} holds antennas outside [0, {nant})")
    spec = _lib.StokesSpec(ncorr, int(full), int(pol == "circular"), len(chosen), (i32 * 4)(*[STOKES.index(s) for s in chosen]),
                           int(bool(corr_first)), 0)
    real = np.float32 if single else np.float64
    arrays = (as_c(data, data.dtype), as_c(weight, real), as_c(flag != 0 if flag.dtype != np.bool_ else flag, np.uint8),
              as_c(jones[:, :, :, 0], np.complex128), tbin_idx, tbin_counts, _antennas(ant1, nrow, "ant1"), _antennas(ant2, nrow, "ant2"))
    sizes = (nrow, nchan, nant, ntime, tbin_idx.size)
    return spec, sizes, arrays, (nrow, nchan, len(chosen)), single


def weight_data(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, nc, wgt_mode, info=None):
    """Stokes visibilities and weights from raw correlations with the Jones correction applied (weighting.py:274-468), on the
    device (``pfbhip_weight_data``, csrc/stokes.hip).

    ``data, weight, flag`` are ``(nrow, nchan, nc)``; ``jones`` is ``(ntime, nant, nchan, ndir, 2)`` (diagonal) or
    ``(..., 2, 2)``, of which direction 0 is used; rows ``tbin_idx[t] - tbin_idx.min() ... + tbin_counts[t]`` belong to
    Jones time ``t``.  Returns ``(vis, wgt)`` of shape ``(nrow, nchan, ns)`` with the products in the order I, Q, U, V; ``vis``
    has the dtype of ``data`` and ``wgt`` its real dtype.  Samples with any correlation flagged and rows in no bin are zero.
    Inputs may be read-only and need not be contiguous.  ``info`` (a dict) receives ``device_ms``, the kernel's time."""
    spec, sizes, arrays, shape, single = _weight_data_args(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol,
                                                          product, nc, wgt_mode, False)
    vis = _lib.result_empty(shape, np.complex64 if single else np.complex128)
    wgt = _lib.result_empty(shape, np.float32 if single else np.float64)
    ms = f64(0.0)
    f = lib().pfbhip_weight_data_sp if single else lib().pfbhip_weight_data
    check(f(ct.byref(spec), *sizes, *(ptr(a) for a in arrays), ptr(vis), ptr(wgt), None, ct.byref(ms) if info is not None else None))
    if info is not None:
        info["device_ms"] = ms.value
    return vis, wgt


def weight_data_dev(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, nc, wgt_mode, corr_first=True,
                    with_mask=True, info=None):
    """:func:`weight_data` with the results left on the device: ``(vis, wgt, mask)`` as ``DeviceArray``\\ s, complex128 and
    float64 of shape ``(ns, nrow, nchan)`` with ``corr_first`` (the layout ``grid_partition`` takes), else
    ``(nrow, nchan, ns)``; ``mask`` is ``~flag.any(-1)`` as uint8 ``(nrow, nchan)``, or None without ``with_mask``.
    complex64 data is widened on the host first."""
    data = np.asarray(data)
    if data.dtype == np.complex64:
        data = data.astype(np.complex128)
    spec, sizes, arrays, (nrow, nchan, ns), _ = _weight_data_args(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol,
                                                                  product, nc, wgt_mode, corr_first)
    shape = (ns, nrow, nchan) if corr_first else (nrow, nchan, ns)
    vis, wgt = _lib.DeviceArray(shape, np.complex128), _lib.DeviceArray(shape, np.float64)
    mask = _lib.DeviceArray((nrow, nchan), np.uint8) if with_mask else None
    ms = f64(0.0)
    check(lib().pfbhip_weight_data_dev(ct.byref(spec), *sizes, *(ptr(a) for a in arrays), vis.ptr, wgt.ptr,
                                       mask.ptr if with_mask else None, ct.byref(ms) if info is not None else None))
    if info is not None:
        info["device_ms"] = ms.value
    return vis, wgt, mask
