"""Snapshot imaging on a resident chunk: the array core of ``pfb hci``.

``stokes_image`` of the reference (``src/pfb_imaging/utils/stokes2im.py:175-783``) images one short snapshot -- one or a few
integrations, one band, 1-4 Stokes parameters -- and is called thousands of times per run.  :func:`snapshot_image_chunk` is
its array work on a :class:`~pfb_imaging_amd.vischunk.VisChunk` that stays in HBM from the Stokes conversion to the float32
cube, in the reference's order:

  1. rephase by ``w_diff`` and subtract the model (:364-373, :466-468)            ``VisChunk.rephase_residual``
  2. joint l2 reweighting (:470-481)                                               ``VisChunk.l2_reweight_joint``
  3. transient injection into the first Stokes (:491-558)                          ``VisChunk.inject_transients``
  4. imaging weights on the padded grid (:563-604)                                 ``VisChunk.imaging_weights``
  5. ``wsum`` (:632)                                                               ``VisChunk.wsum``
  6. per Stokes ``vis2dirty`` of the data and of the PSF visibilities (:635-683)   ``Gridder.vis2dirty_rows_dev / psf_rows_dev``
  7. PSF-peak normalisation, rms, beam weighting, float32 transposed cube          ``pfbhip_snapshot_finish_dev``
     (:684-692, :707-708, :731-737, :750-753)
  8. clean-beam fit of the normalised PSF planes where they lie (:695)             ``fitcleanbeam_dev``

Only the float32 outputs and O(ns) scalars cross PCIe (and the counts with ``weight_grid_out``).
:func:`stokes_image_arrays` is the face that starts from raw correlations (``VisChunk.from_weight_data``).

Three deliberate differences from the reference:
  * :472 multiplies ``(nrow, nchan, ncorr)`` by the ``(nrow, nchan)`` mask, which broadcasts only for degenerate shapes; the
    evident intent ``mask[:, :, None]`` is built.
  * :481 sets ``weight = None`` for an empty mask and fails later; here that is a ``ValueError`` at once.
  * :686-692 nests the normalisation loop inside the per-Stokes loop, so Stokes gridded earlier are divided again by the
    1.0 their normalised PSF peaks at and report ``weight = 1.0``; here each Stokes is normalised once and ``weight`` is its
    own PSF peak.

Not built: ``natural_grad`` (the reference's call mixes ``2 nx`` with ``nx_psf``, and it is jax), ``synthesize_uvw`` (casacore
measures: the caller supplies ``w_diff`` and the chunk holds the new ``uvw``), the feed-plane beam reprojection (the caller
supplies ``pbeam`` on the image grid), xarray / zarr / astropy I/O, and a single-precision device path.
"""

import ctypes as ct

import numpy as np

from .. import _lib
from .._lib import DeviceArray, DeviceView, check, f64, lib, ptr

PSF_MIN_SIZE = 128  # stokes2im.py:606


def _even_good_size(n):
    """stokes2im.py:567-572, :611-616: the smallest even good size >= n"""
    from ..fft import good_size

    n = good_size(n)
    while n % 2:
        n = good_size(n + 1)
    return n


def pad_size(n, min_padding):
    """``nx_pad`` of stokes2im.py:567-569"""
    return _even_good_size(int(min_padding * n))


def psf_size(nx, ny, psf_relative_size):
    """``(nx_psf, ny_psf)`` of stokes2im.py:606-619"""
    if psf_relative_size is None:
        return PSF_MIN_SIZE, PSF_MIN_SIZE
    nx_psf, ny_psf = _even_good_size(int(nx * psf_relative_size)), _even_good_size(int(ny * psf_relative_size))
    if nx_psf < PSF_MIN_SIZE or ny_psf < PSF_MIN_SIZE:
        return PSF_MIN_SIZE, PSF_MIN_SIZE
    return nx_psf, ny_psf


def _check_snapshot_args(ns, nrow, nchan, nx, ny, cell_rad, x0, y0, model_vis, w_diff, l2_reweight_dof, transients, robustness,
                         npix_super, filter_counts_level, min_padding, psf_relative_size, pbeam, eta, epsilon, weight_grid_out,
                         out_dtype):
    """Every refusal of :func:`snapshot_image_chunk` that needs no device.  Returns ``(pbeam as float64 or None, out dtype)``."""
    if int(nx) != nx or int(ny) != ny or nx < 1 or ny < 1:
        raise ValueError(f"nx, ny = {nx}, {ny} must be positive integers")
    if not cell_rad > 0:
        raise ValueError(f"cell_rad = {cell_rad} must be positive")
    if not x0 * x0 + y0 * y0 < 1.0:
        raise ValueError(f"the centre ({x0}, {y0}) is not on the sphere")
    if not min_padding >= 1.0:
        raise ValueError(f"min_padding = {min_padding} must be at least 1")
    if psf_relative_size is not None and not psf_relative_size > 0:
        raise ValueError(f"psf_relative_size = {psf_relative_size} must be positive")
    out_dtype = np.dtype(out_dtype)
    if out_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"out_dtype must be float32 or float64, not {out_dtype}")
    if not 0 < epsilon < 1:
        raise ValueError(f"epsilon = {epsilon} must lie in (0, 1)")
    if npix_super is not None and (int(npix_super) != npix_super or npix_super < 0):
        raise ValueError(f"npix_super = {npix_super} must be a non-negative integer")
    if filter_counts_level is not None and not filter_counts_level >= 0:
        raise ValueError(f"filter_counts_level = {filter_counts_level} must not be negative")
    if robustness is not None and not np.isfinite(robustness):
        raise ValueError(f"robustness = {robustness} must be finite")
    if model_vis is not None:
        shape = tuple(model_vis.shape) if isinstance(model_vis, DeviceArray) else np.shape(model_vis)
        if shape != (ns, nrow, nchan):
            raise ValueError(f"model_vis shape {shape} != {(ns, nrow, nchan)}")
        if isinstance(model_vis, DeviceArray):
            if model_vis.dtype != np.complex128:
                raise TypeError(f"model_vis on the device must be complex128, not {model_vis.dtype}")
        elif np.asarray(model_vis).dtype.kind != "c":
            raise TypeError(f"model_vis must be complex, not {np.asarray(model_vis).dtype}")
    if w_diff is not None:
        if np.shape(w_diff) not in ((nrow,), (nrow, 1)):
            raise ValueError(f"w_diff shape {np.shape(w_diff)} != {(nrow,)}")
        if np.asarray(w_diff).dtype.kind not in "fiu":
            raise TypeError(f"w_diff must be real, not {np.asarray(w_diff).dtype}")
    if l2_reweight_dof is not None and not (l2_reweight_dof >= 0 and np.isfinite(l2_reweight_dof)):
        raise ValueError(f"l2_reweight_dof = {l2_reweight_dof} must be finite and not negative (0 or None: no reweighting)")
    if transients is not None:
        missing = [k for k in ("uvw", "time", "sources", "all_times", "all_freqs") if k not in transients]
        if missing:
            raise ValueError(f"transients lacks {missing}")
        if np.shape(transients["uvw"]) != (nrow, 3) or np.shape(transients["time"]) != (nrow,):
            raise ValueError(f"transients: uvw must be {(nrow, 3)} and time {(nrow,)}")
    if weight_grid_out and robustness is None:
        raise ValueError("weight_grid_out needs robustness: the grid of weights is that of the imaging weights")
    if pbeam is not None:
        pbeam = np.asarray(pbeam)
        if pbeam.shape != (ns, nx, ny):
            raise ValueError(f"pbeam shape {pbeam.shape} != {(ns, nx, ny)}")
        if pbeam.dtype.kind not in "fiu":
            raise TypeError(f"pbeam must be real, not {pbeam.dtype}")
        if not eta >= 0:
            raise ValueError(f"eta = {eta} must not be negative")
        pbeam = _lib.as_c(pbeam, np.float64)
    return pbeam, out_dtype


def snapshot_finish(residual_dev, psf_dev, wsum, pbeam_dev=None, eta=1e-5, psf_out=False, out_dtype=np.float32, info=None):
    """``pfbhip_snapshot_finish_dev`` on ``residual_dev (ns, nx, ny)`` and ``psf_dev (ns, nxp, nyp)`` (float64 DeviceArrays,
    normalised in place): ``dict(cube, psf (with psf_out), beam_weight (with a beam), psf_max, rms)``, the images transposed
    and of ``out_dtype``.  ``info`` (a dict) receives ``device_ms``, the kernels' time without the downloads."""
    out_dtype = np.dtype(out_dtype)
    for name, a in (("residual_dev", residual_dev), ("psf_dev", psf_dev)) + ((("pbeam_dev", pbeam_dev),) if pbeam_dev is not None else ()):
        if not isinstance(a, DeviceArray) or a.dtype != np.float64 or len(a.shape) != 3:
            raise ValueError(f"{name} must be a float64 DeviceArray (ns, nx, ny)")
    ns, nx, ny = residual_dev.shape
    nxp, nyp = psf_dev.shape[1:]
    wsum = _lib.as_c(wsum, np.float64)
    if psf_dev.shape[0] != ns or wsum.shape != (ns,) or (pbeam_dev is not None and tuple(pbeam_dev.shape) != (ns, nx, ny)):
        raise ValueError("residual_dev, psf_dev, pbeam_dev and wsum disagree in their shapes")
    if out_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"out_dtype must be float32 or float64, not {out_dtype}")
    ms = f64(0.0)
    out = dict(cube=_lib.result_empty((ns, ny, nx), out_dtype), psf_max=np.empty(ns), rms=np.empty(ns))
    if psf_out:
        out["psf"] = _lib.result_empty((ns, nyp, nxp), out_dtype)
    if pbeam_dev is not None:
        out["beam_weight"] = _lib.result_empty((ns, ny, nx), out_dtype)
    check(lib().pfbhip_snapshot_finish_dev(residual_dev.ptr, psf_dev.ptr, None if pbeam_dev is None else pbeam_dev.ptr, ptr(wsum),
                                           ns, nx, ny, nxp, nyp, float(eta),
                                           int(out_dtype == np.float64), ptr(out["cube"]), ptr(out.get("psf")),
                                           ptr(out.get("beam_weight")), ptr(out["psf_max"]), ptr(out["rms"]),
                                           ct.byref(ms) if info is not None else None))
    if info is not None:
        info["device_ms"] = ms.value
    return out


def snapshot_image_chunk(chunk, nx, ny, cell_rad, *, x0=0.0, y0=0.0, model_vis=None, w_diff=None, l2_reweight_dof=None,
                         transients=None, robustness=None, npix_super=0, filter_counts_level=5.0, min_padding=1.7,
                         psf_relative_size=None, pbeam=None, eta=1e-5, epsilon=1e-7, do_wgridding=True, psf_out=False,
                         weight_grid_out=False, pixsize_deg=None, out_dtype=np.float32):
    """One snapshot of ``chunk`` (a :class:`~pfb_imaging_amd.vischunk.VisChunk` whose ``uvw`` are those of the imaging centre)
    as the reference's ``data_vars``: ``cube (ns, ny, nx)``, ``psf`` (with ``psf_out``), ``wgtgrid`` (with
    ``weight_grid_out``), ``weight`` (the PSF peak, as in the reference), ``beam_weight`` (with ``pbeam``), ``rms``,
    ``nonzero``, ``psf_maj / psf_min / psf_pa`` (degrees) and ``x0, y0``.  See the module docstring for the steps.

    ``x0, y0`` are the gridder's ``center_x / center_y``; ``model_vis (ns, nrow, nchan)`` Stokes model visibilities (host or
    ``DeviceArray``); ``w_diff (nrow)`` [m] the rephasing delays; ``transients`` a dict of
    :meth:`VisChunk.inject_transients`' arguments (``uvw, time, sources, all_times, all_freqs`` and optionally ``beam``;
    ``w_diff`` is this call's); ``pbeam (ns, nx, ny)`` the primary beam on the image grid.  The chunk's visibilities and
    weights are updated in place.  ``out_dtype=np.float64`` skips the float32 cast (for tests)."""
    from ..operators.gridder import wgridder_conventions
    from ..vischunk import VisChunk
    from ..wgridder import Gridder
    from .misc import fitcleanbeam_dev

    if not isinstance(chunk, VisChunk):
        raise TypeError(f"chunk must be a VisChunk, not {type(chunk).__name__}")
    ns, nrow, nchan = chunk.ncorr, chunk.nrow, chunk.nchan
    pbeam, out_dtype = _check_snapshot_args(ns, nrow, nchan, nx, ny, cell_rad, x0, y0, model_vis, w_diff, l2_reweight_dof, transients,
                                            robustness, npix_super, filter_counts_level, min_padding, psf_relative_size, pbeam, eta, epsilon,
                                            weight_grid_out, out_dtype)
    w_diff, model_vis = chunk._check_rephase(w_diff, model_vis)
    chunk._open()
    nx, ny = int(nx), int(ny)
    flip_u, flip_v, flip_w, _, _ = wgridder_conventions(0, 0)
    nx_psf, ny_psf = psf_size(nx, ny, psf_relative_size)
    # -- 1-3: the visibilities
    if w_diff is not None or model_vis is not None:
        chunk.rephase_residual(w_diff, model_vis)
    if l2_reweight_dof:
        chunk.l2_reweight_joint(l2_reweight_dof)
    if transients is not None:
        chunk.inject_transients(transients["uvw"], chunk.freq, transients["time"], transients["sources"], transients["all_times"],
                                transients["all_freqs"], w_diff=w_diff, beam=transients.get("beam"))
    # -- 4, 5: the weights
    counts = None
    if robustness is not None:
        counts = chunk.imaging_weights(pad_size(nx, min_padding), pad_size(ny, min_padding), cell_rad, cell_rad, robustness,
                                       filter_level=filter_counts_level, npix_super=npix_super, usign=1.0 if flip_u else -1.0,
                                       vsign=1.0 if flip_v else -1.0, return_counts=bool(weight_grid_out))
    wsum = chunk.wsum()
    # -- 6-8: the images
    common = dict(pixsize_x=cell_rad, pixsize_y=cell_rad, center_x=x0, center_y=y0, epsilon=epsilon, flip_u=flip_u, flip_v=flip_v,
                  flip_w=flip_w, do_wgridding=do_wgridding, divide_by_n=True, sigma_min=min_padding)
    g = gp = res_dev = psf_dev = pb_dev = None
    try:
        res_dev, psf_dev = DeviceArray((ns, nx, ny), np.float64), DeviceArray((ns, nx_psf, ny_psf), np.float64)
        if wsum.any():
            g = Gridder(chunk.uvw, chunk.freq, chunk.mask_host, npix_x=nx, npix_y=ny, **common)
            gp = Gridder(chunk.uvw, chunk.freq, chunk.mask_host, npix_x=nx_psf, npix_y=ny_psf, **common)
        for c in range(ns):
            if wsum[c] == 0:
                continue
            off = chunk.corr_offset(c)
            g.vis2dirty_rows_dev(chunk.vis, chunk.wgt, DeviceView(res_dev, c * nx * ny, (nx, ny)), vis_offset=off, wgt_offset=off)
            gp.psf_rows_dev(chunk.wgt, DeviceView(psf_dev, c * nx_psf * ny_psf, (nx_psf, ny_psf)), wgt_offset=off, ramp_sign=-1.0)
        if pbeam is not None:
            pb_dev = DeviceArray.from_host(pbeam)
        fin = snapshot_finish(res_dev, psf_dev, wsum, pb_dev, eta, psf_out, out_dtype)
        if pixsize_deg is None:
            pixsize_deg = np.rad2deg(cell_rad)
        gausspars = fitcleanbeam_dev(psf_dev, level=0.5, pixsize=pixsize_deg)
    finally:
        for h in (g, gp):
            if h is not None:
                h.close()
        for d in (res_dev, psf_dev, pb_dev):
            if d is not None:
                d.free()
    out = dict(cube=fin["cube"])
    if psf_out:
        out["psf"] = fin["psf"]
    if weight_grid_out:
        if counts is None:  # (every sample masked: imaging_weights had nothing to count)
            counts = np.zeros((ns, pad_size(nx, min_padding), pad_size(ny, min_padding)))
        wgtgrid = np.zeros_like(counts)
        np.divide(1.0, counts, out=wgtgrid, where=counts > 0)
        out["wgtgrid"] = np.ascontiguousarray(np.transpose(wgtgrid.astype(np.float32), axes=(0, 2, 1)))
    out["weight"] = fin["psf_max"]
    if pbeam is not None:
        out["beam_weight"] = fin["beam_weight"]
    out["rms"] = fin["rms"].astype(np.float32) if out_dtype == np.float32 else fin["rms"]
    out["nonzero"] = fin["psf_max"] > 0
    ptype = np.float32 if out_dtype == np.float32 else np.float64
    out["psf_maj"] = gausspars[:, 0].astype(ptype)
    out["psf_min"] = gausspars[:, 1].astype(ptype)
    out["psf_pa"] = (gausspars[:, 2] * 180 / np.pi).astype(ptype)
    out["x0"], out["y0"] = x0, y0
    return out


def stokes_image_arrays(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, uvw, freq, pol, product, nc, wgt_mode, nx, ny,
                        cell_rad, **kw):
    """:func:`snapshot_image_chunk` from raw correlations: ``VisChunk.from_weight_data`` (``weight_data`` with the Jones
    correction, stokes2im.py:447-464) followed by the snapshot.  ``uvw`` are those of the imaging centre; the keywords are
    :func:`snapshot_image_chunk`'s.  Every argument is checked before the device is touched."""
    from ..vischunk import VisChunk
    from .stokes import stokes_products

    unknown = set(kw) - set(snapshot_image_chunk.__kwdefaults__)
    if unknown:
        raise TypeError(f"unknown keywords {sorted(unknown)}")
    uvw, freq = np.asarray(uvw), np.asarray(freq)
    ns = len(stokes_products(product, pol, nc, wgt_mode, np.ndim(jones)))
    data_shape = np.shape(data)
    if len(data_shape) != 3:
        raise ValueError(f"data {data_shape} must be (nrow, nchan, ncorr)")
    nrow, nchan = data_shape[:2]
    if uvw.shape != (nrow, 3) or freq.shape != (nchan,):
        raise ValueError(f"uvw {uvw.shape} and freq {freq.shape} must be {(nrow, 3)} and {(nchan,)}")
    if uvw.dtype.kind not in "fiu" or freq.dtype.kind not in "fiu":
        raise TypeError("uvw and freq must be real")
    opts = dict(snapshot_image_chunk.__kwdefaults__)
    opts.update(kw)
    _check_snapshot_args(ns, nrow, nchan, nx, ny, cell_rad, opts["x0"], opts["y0"], opts["model_vis"], opts["w_diff"],
                         opts["l2_reweight_dof"], opts["transients"], opts["robustness"], opts["npix_super"], opts["filter_counts_level"],
                         opts["min_padding"], opts["psf_relative_size"], opts["pbeam"], opts["eta"], opts["epsilon"], opts["weight_grid_out"],
                         opts["out_dtype"])
    # (from_weight_data checks the raw arrays itself before its first device call)
    with VisChunk.from_weight_data(uvw, freq, data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, nc,
                                   wgt_mode) as chunk:
        return snapshot_image_chunk(chunk, nx, ny, cell_rad, **kw)
