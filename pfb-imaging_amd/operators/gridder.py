"""Gridder call sites of ``pfb_imaging.operators.gridder`` on the GPU.

Mirrors /root/reference/src/pfb_imaging/operators/gridder.py:
    wgridder_conventions      :23-34
    vis2im / im2vis           :37-144
    comps2vis                 :276-367   (the numpy-level _comps2vis_impl; the dask layer :148-273 stays with the reference)
    grid_partition            :760-923   (dirty, PSF, PSFHAT, beam, wsum, imaging weights per partition)
    residual_from_partitions  :926-1016  (dirty - sum_p R_p^H W_p R_p (beam_p model))
    compute_residual_arrays   the arithmetic of compute_residual :1060-1117 on in-memory arrays
    image_data_products_arrays / _chunk   the arithmetic of image_data_products :375-757 on host arrays / on a resident VisChunk
The zarr / xarray / dask / ray plumbing around these (reading ``.xds``/``.dds`` stores, writing
results) is orchestration and stays with the reference; partitions are accepted either as
xarray-like objects (``part.UVW.values``, ``part.attrs``) or as plain dicts of numpy arrays.
"""

import numpy as np

from .. import _lib
from .. import fft as _fft
from ..misc import resize_thread_pool
from ..utils.beam import eval_beam
from ..utils.misc import fitcleanbeam
from ..utils.weighting import counts_to_weights, imaging_weights
from ..wgridder import Gridder, _get_gridder, dirty2vis, vis2dirty

lightspeed = 299792458.0
ifftshift = np.fft.ifftshift


def wgridder_conventions(l0, m0):
    """flip_u, flip_v, flip_w, x0, y0 (https://github.com/mreineck/ducc/issues/34); gridder.py:23-34."""
    return False, True, False, -l0, -m0


def vis2im(uvw, freq, vis, wgt, mask, nx, ny, cellx, celly, l0, m0, epsilon, precision, do_wgridding, divide_by_n,
           nthreads, sigma_min, sigma_max, double_precision_accumulation):
    """gridder.py:37-100."""
    uvw = np.require(uvw, dtype=np.float64)
    freq = np.require(freq, np.float64)
    if precision.lower() == "single":
        real_type, complex_type = np.float32, np.complex64
    elif precision.lower() == "double":
        real_type, complex_type = np.float64, np.complex128
    else:
        raise ValueError(f"unknown precision {precision}")
    vis = np.require(vis, dtype=complex_type)
    if wgt is not None:
        wgt = np.require(wgt, dtype=real_type)
    if mask is not None:
        mask = np.require(mask, dtype=np.uint8)
    flip_u, flip_v, flip_w, x0, y0 = wgridder_conventions(l0, m0)
    return vis2dirty(uvw=uvw, freq=freq, vis=vis, wgt=wgt, mask=mask, npix_x=nx, npix_y=ny, pixsize_x=cellx,
                     pixsize_y=celly, center_x=x0, center_y=y0, epsilon=epsilon, flip_u=flip_u, flip_v=flip_v,
                     flip_w=flip_w, do_wgridding=do_wgridding, divide_by_n=divide_by_n, nthreads=nthreads,
                     sigma_min=sigma_min, sigma_max=sigma_max,
                     double_precision_accumulation=double_precision_accumulation)


def im2vis(uvw, freq, image, cellx, celly, freq_bin_idx, freq_bin_counts, l0=0, m0=0, epsilon=1e-7, do_wgridding=True,
           divide_by_n=False, nthreads=1):
    """gridder.py:103-144: per-band degridding into channel slices."""
    freq_bin_idx2 = freq_bin_idx - freq_bin_idx.min()
    flip_u, flip_v, flip_w, x0, y0 = wgridder_conventions(l0, m0)
    nband, nx, ny = image.shape
    nrow = uvw.shape[0]
    nchan = freq.size
    vis = np.zeros((nrow, nchan), dtype=np.result_type(image, np.complex64))
    for i in range(nband):
        ind = slice(freq_bin_idx2[i], freq_bin_idx2[i] + freq_bin_counts[i])
        vis[:, ind] = dirty2vis(uvw=uvw, freq=freq[ind], dirty=image[i], pixsize_x=cellx, pixsize_y=celly, center_x=x0,
                                center_y=y0, flip_u=flip_u, flip_v=flip_v, flip_w=flip_w, epsilon=epsilon,
                                nthreads=nthreads, do_wgridding=do_wgridding, divide_by_n=divide_by_n)
    return vis


# -- partition access: xarray-like object or dict ---------------------------------------------

def _field(part, name):
    if isinstance(part, dict):
        return np.asarray(part[name])
    return getattr(part, name).values


def _attr(part, name, default=0.0):
    if isinstance(part, dict):
        return part.get("attrs", {}).get(name, part.get(name, default))
    return part.attrs.get(name, default)


def comps2vis(uvw, utime, freq, rbin_idx, rbin_cnts, tbin_idx, tbin_cnts, fbin_idx, fbin_cnts, region_mask, mds, modelf, tfunc,
              ffunc, epsilon=1e-7, nthreads=1, do_wgridding=True, divide_by_n=False, freq_min=-np.inf, freq_max=np.inf,
              product="I", info=None, _dirty2vis=None, method="grid"):
    """Model visibilities of a component model, ``_comps2vis_impl`` of the reference (gridder.py:276-367) with the render and
    the degrid on the device: per (time chunk, band) the ``nparam`` numbers of the basis vector go up, the image is formed in
    HBM from the resident coefficients and degridded there (``Gridder.dirty2vis_dev``), the visibilities come down.

    ``mds`` is a dict or an attribute object with ``coefficients (nparam, ncomps)``, ``location_x``, ``location_y`` and the
    attributes ``cell_rad_x, npix_x, npix_y, center_x, center_y, flip_u, flip_v, flip_w``.  ``info`` (a dict, optional)
    receives ``device_renders``, ``host_renders`` and ``plans`` (and ``dft_predicts`` with ``method="dft"``).

    ``method="dft"`` sums the measurement equation directly over the components instead (:class:`pfb_imaging_amd.dft.DFT`): no
    image, no plan, no ``epsilon`` -- one handle per time chunk's rows, one ``predict_comps`` per band, the same bookkeeping.
    It is the cheaper path below some number of components (DESIGN.md "Direct DFT of point components" has the measurement);
    nothing chooses it automatically.

    ``modelf`` is checked once per call to be linear in its parameters (:func:`pfb_imaging_amd.comps.basis_vector`); one that
    is not is evaluated on the host as the reference does and the image uploaded -- never linearised.

    The reference's behaviour is kept where it is peculiar:
      * ``celly`` is ``mds.cell_rad_x`` (:321-322): pixels are square whatever ``cell_rad_y`` says;
      * the row slice of a time chunk runs from the first row of its first time to the last row of its last (:335);
      * nothing is degridded -- the output stays zero -- when ``region_mask`` has no set pixel (:347) or no channel of the band
        lies in ``[freq_min, freq_max]`` (:340), and nothing at all when no channel of ``freq`` does (:315);
      * the same visibilities are written to every entry of ``product`` (:349-350; no Stokes conversion);
      * the output dtype is ``result_type(coefficients, complex64)`` (:314).
    One difference: the reference degrids ALL rows of ``uvw`` for every time chunk (:351) and assigns the result to the
    chunk's row slice, which only fits when the call holds one time chunk (as its dask layer arranges, core/degrid.py:266-279);
    here each chunk degrids its own rows ``uvw[indr]``, the same thing for one chunk and the evident intent for several.

    ``_dirty2vis`` (tests) replaces the device: a callable with ``dirty2vis``'s keywords; images are then rendered on the host.
    """
    if method not in ("grid", "dft"):
        raise ValueError(f"method must be 'grid' or 'dft', not {method!r}")
    if method == "dft" and _dirty2vis is not None:
        raise ValueError("_dirty2vis stands in for the gridder: it has no meaning with method='dft'")
    resize_thread_pool(nthreads)
    coeffs = _field(mds, "coefficients")
    nstokes = len(product)
    vis = np.zeros((uvw.shape[0], freq.size, nstokes), dtype=np.result_type(coeffs.dtype, np.complex64))
    stats = dict(device_renders=0, host_renders=0, plans=0)
    if method == "dft":
        stats["dft_predicts"] = 0
    if info is not None:
        info.update(stats)
    in_range = (freq >= freq_min) & (freq <= freq_max)
    if not in_range.any() or not np.any(region_mask):
        return vis  # (with an empty region mask the reference renders every image and then degrids none)
    xloc, yloc = _field(mds, "location_x"), _field(mds, "location_y")
    cell = _attr(mds, "cell_rad_x")  # both pixel sizes: the reference reads cell_rad_x for x and for y
    nx, ny = int(_attr(mds, "npix_x")), int(_attr(mds, "npix_y"))
    plan_kw = dict(npix_x=nx, npix_y=ny, pixsize_x=float(cell), pixsize_y=float(cell), center_x=float(_attr(mds, "center_x")),
                   center_y=float(_attr(mds, "center_y")), epsilon=float(epsilon), flip_u=bool(_attr(mds, "flip_u")),
                   flip_v=bool(_attr(mds, "flip_v")), flip_w=bool(_attr(mds, "flip_w")), do_wgridding=bool(do_wgridding),
                   divide_by_n=bool(divide_by_n), sigma_min=1.1, sigma_max=2.6)

    def host_image(tt, ff):
        values = modelf(tt, ff, *coeffs)
        image = np.zeros((nx, ny), dtype=coeffs.dtype)
        image[xloc, yloc] = values
        return np.where(region_mask, image, 0.0)

    # bin starts are relative to the first bin of this call (the caller may hand over a block of a larger problem)
    row0, time0, chan0 = rbin_idx.min(), tbin_idx.min(), fbin_idx.min()
    bands = []
    for first, count in zip(fbin_idx - chan0, fbin_cnts):
        chans = slice(int(first), int(first + count))
        if in_range[chans].any():
            bands.append(chans)
    if method == "dft":
        _comps2vis_dft(vis, uvw, utime, freq, rbin_idx - row0, rbin_cnts, tbin_idx - time0, tbin_cnts, bands, region_mask, coeffs,
                       xloc, yloc, plan_kw, modelf, tfunc, ffunc, stats, info)
        return vis
    handle = image_dev = None
    linear = None  # decided at the first render; a modelf that fails once stays on the host for the whole call
    plans = set()
    try:
        if _dirty2vis is None:
            from ..comps import Comps, basis_vector

            handle = Comps(nx, ny, xloc, yloc, coeffs)
            handle.set_region(region_mask)
            image_dev = _lib.DeviceArray((nx, ny), np.float64)
        for first, count in zip(tbin_idx - time0, tbin_cnts):
            times = slice(int(first), int(first + count))
            starts, counts = rbin_idx[times] - row0, rbin_cnts[times]
            rows = slice(int(starts[0]), int(starts[-1] + counts[-1]))
            uvw_rows = np.ascontiguousarray(uvw[rows], dtype=np.float64)
            tt = tfunc(np.mean(utime[times]))
            for chans in bands:
                ff = ffunc(np.mean(freq[chans]))
                bvec = None
                if handle is not None and linear is not False:
                    bvec = basis_vector(modelf, tt, ff, coeffs.shape[0])
                    if linear is None:
                        linear = bvec is not None
                if bvec is not None:
                    handle.render_dev(bvec, image_dev, region=True)
                    stats["device_renders"] += 1
                else:
                    image = host_image(tt, ff)
                    stats["host_renders"] += 1
                    if handle is not None:
                        handle.host_renders += 1
                        image_dev.upload(image)
                if handle is None:
                    kw = {k: v for k, v in plan_kw.items() if k not in ("npix_x", "npix_y", "sigma_min", "sigma_max")}
                    out = _dirty2vis(uvw=uvw_rows, freq=freq[chans], dirty=image, nthreads=nthreads, **kw)
                else:
                    g, cached = _get_gridder(uvw_rows, freq[chans], None, **plan_kw)
                    plans.add(id(g))
                    try:
                        out = g.dirty2vis_dev(image_dev)
                    finally:
                        if not cached:
                            g.close()
                vis[rows, chans, :] = np.asarray(out)[:, :, None]
    finally:
        stats["plans"] = len(plans)
        if info is not None:
            info.update(stats)
        if handle is not None:
            handle.close()
        if image_dev is not None:
            image_dev.free()
    return vis


def _comps2vis_dft(vis, uvw, utime, freq, rbin_idx, rbin_cnts, tbin_idx, tbin_cnts, bands, region_mask, coeffs, xloc, yloc, plan_kw,
                   modelf, tfunc, ffunc, stats, info):
    """``comps2vis(method="dft")``: fills ``vis`` in place; bin starts are already relative to this call's first bins."""
    from ..comps import Comps, basis_vector
    from ..dft import DFT, lm_of_pixels

    geom = dict(cellx=plan_kw["pixsize_x"], celly=plan_kw["pixsize_y"], center_x=plan_kw["center_x"], center_y=plan_kw["center_y"],
                flip_u=plan_kw["flip_u"], flip_v=plan_kw["flip_v"], flip_w=plan_kw["flip_w"])
    conv = dict(sgn=-1.0, do_wgridding=plan_kw["do_wgridding"], divide_by_n=plan_kw["divide_by_n"])
    nx, ny = plan_kw["npix_x"], plan_kw["npix_y"]
    handle = Comps(nx, ny, xloc, yloc, coeffs)
    linear = None  # as in the gridded path: decided at the first render
    try:
        handle.set_region(region_mask)
        for first, count in zip(tbin_idx, tbin_cnts):
            times = slice(int(first), int(first + count))
            starts, counts = rbin_idx[times], rbin_cnts[times]
            rows = slice(int(starts[0]), int(starts[-1] + counts[-1]))
            tt = tfunc(np.mean(utime[times]))
            with DFT(uvw[rows], freq) as d:
                for chans in bands:
                    ff = ffunc(np.mean(freq[chans]))
                    bvec = None
                    if linear is not False:
                        bvec = basis_vector(modelf, tt, ff, coeffs.shape[0])
                        if linear is None:
                            linear = bvec is not None
                    if bvec is not None:
                        out = d.predict_comps(handle, bvec, region=True, chans=chans, **geom, **conv)
                        stats["device_renders"] += 1
                    else:  # a nonlinear modelf: its values on the host, as the reference forms them, then the same sum
                        values = np.where(np.asarray(region_mask)[xloc, yloc], modelf(tt, ff, *coeffs), 0.0)
                        lm, su, sv, sw = lm_of_pixels(xloc, yloc, nx, ny, **geom)
                        out = d.predict(lm, values, signs=(su, sv, sw), chans=chans, **conv)
                        stats["host_renders"] += 1
                        handle.host_renders += 1
                    stats["dft_predicts"] += 1
                    vis[rows, chans, :] = out[:, :, None]
    finally:
        if info is not None:
            info.update(stats)
        handle.close()


def psf_visibilities(uvw, freq, x0, y0, flip_u=False, flip_v=True, dtype=np.complex128):
    """PSF visibilities: ones at the phase centre, else the phase ramp of gridder.py:616-629 / 878-884."""
    if x0 or y0:
        signu = -1.0 if flip_u else 1.0
        signv = -1.0 if flip_v else 1.0
        signx = -1.0 if flip_u else 1.0
        signy = -1.0 if flip_v else 1.0
        n = np.sqrt(1 - x0**2 - y0**2)
        freqfactor = 2j * np.pi * freq[None, :] / lightspeed
        return np.exp(freqfactor * (signu * uvw[:, 0:1] * x0 * signx + signv * uvw[:, 1:2] * y0 * signy
                                    - uvw[:, 2:] * (n - 1)))
    return np.ones((uvw.shape[0], freq.size), dtype=dtype)


def _eval_beam(beam_image, l_in, m_in, ll, mm):
    """/root/reference/src/pfb_imaging/utils/beam.py:75-89 on the host: grid_partition takes it only when no device is present."""
    if (beam_image == 1.0).all():
        return np.ones_like(ll)
    from scipy.interpolate import RegularGridInterpolator

    beamo = RegularGridInterpolator((l_in, m_in), beam_image, bounds_error=False, method="linear", fill_value=1.0)
    return beamo((ll, mm))


def grid_partition(part, counts, nx, ny, nx_psf, ny_psf, cell_rad, robustness=None, nx_pad=None, ny_pad=None, l0=0.0,
                   m0=0.0, nthreads=1, epsilon=1e-7, do_wgridding=True, double_accum=True, do_psfpars=False):
    """Image-space products of one data partition (gridder.py:760-923): ``DIRTY``, ``PSF``,
    ``PSFHAT``, ``BEAM``, ``WSUM`` and the imaging ``WEIGHT``.  One :class:`Gridder` handle per
    output grid serves all correlations (the tile sort is weight-independent).  ``PSFPARSN``
    (the clean-beam fit of the PSF in pixel units, utils/misc.fitcleanbeam on the device) is
    added with ``do_psfpars=True``."""
    resize_thread_pool(nthreads)
    flip_u, flip_v, flip_w, x0, y0 = wgridder_conventions(l0, m0)
    uvw = _field(part, "UVW")
    vis = _field(part, "VIS")
    wgt = np.array(_field(part, "WEIGHT"), dtype=np.float64)
    mask = _field(part, "MASK")
    freq = _field(part, "FREQ")
    ncorr = wgt.shape[0]

    if robustness is not None:
        wgt = counts_to_weights(counts.copy(), uvw, freq, wgt, mask, nx_pad, ny_pad, cell_rad, cell_rad, robustness,
                                usign=1.0 if flip_u else -1.0, vsign=1.0 if flip_v else -1.0)
    wsum = wgt[:, mask.astype(bool)].sum(axis=-1)

    x = (-nx / 2 + np.arange(nx)) * cell_rad + x0
    y = (-ny / 2 + np.arange(ny)) * cell_rad + y0
    beam_in = _field(part, "BEAM")
    if beam_in.shape[-2:] == (nx, ny):
        beam = np.array(beam_in, dtype=float)
    elif _lib.device_count() > 0:  # every correlation in one device call (utils/beam.py, csrc/beam.hip)
        beam = eval_beam(np.asarray(beam_in)[:ncorr], _field(part, "l_beam"), _field(part, "m_beam"), np.rad2deg(x), np.rad2deg(y))
    else:
        xx, yy = np.meshgrid(np.rad2deg(x), np.rad2deg(y), indexing="ij")
        l_beam, m_beam = _field(part, "l_beam"), _field(part, "m_beam")
        beam = np.zeros((ncorr, nx, ny), dtype=float)
        for c in range(ncorr):
            beam[c] = _eval_beam(beam_in[c], l_beam, m_beam, xx, yy)

    common = dict(pixsize_x=cell_rad, pixsize_y=cell_rad, center_x=x0, center_y=y0, epsilon=epsilon, flip_u=flip_u,
                  flip_v=flip_v, flip_w=flip_w, do_wgridding=do_wgridding, divide_by_n=False, sigma_min=1.1,
                  sigma_max=3.0)
    g = Gridder(uvw, freq, mask, npix_x=nx, npix_y=ny, **common)
    try:
        dirty = _lib.result_empty((ncorr, nx, ny), np.float64)
        for c in range(ncorr):
            g.vis2dirty(vis[c], wgt[c], out=dirty[c])
    finally:
        g.close()

    psf_vis = psf_visibilities(uvw, freq, x0, y0, flip_u, flip_v, dtype=np.complex128)
    g = Gridder(uvw, freq, mask, npix_x=nx_psf, npix_y=ny_psf, **common)
    try:
        psf = _lib.result_empty((ncorr, nx_psf, ny_psf), np.float64)
        for c in range(ncorr):
            g.vis2dirty(psf_vis, wgt[c], out=psf[c])
    finally:
        g.close()
    if nx_psf % 2 == 0 and ny_psf % 2 == 0:  # (the shift as a checkerboard sign on the spectrum, on the device)
        psfhat = _fft.r2c(psf, axes=(1, 2), nthreads=nthreads, forward=True, inorm=0, centred=True)
    else:
        psfhat = _fft.r2c(ifftshift(psf, axes=(1, 2)), axes=(1, 2), nthreads=nthreads, forward=True, inorm=0)
    out = {"DIRTY": dirty, "PSF": psf, "PSFHAT": psfhat, "BEAM": beam, "WSUM": wsum, "WEIGHT": wgt}
    if do_psfpars:
        out["PSFPARSN"] = fitcleanbeam(psf, level=0.5, pixsize=1.0)
    return out


class PartitionResidual:
    """Device-resident state for the exact residual of one band: one :class:`Gridder` per
    partition with the per-correlation weights, so every major cycle is pure device work
    (the reference re-derives everything inside ducc0 on each call; gridder.py:962-1016)."""

    def __init__(self, parts, nx, ny, cell_rad, epsilon=1e-7, do_wgridding=True):
        self.nx, self.ny = nx, ny
        self.items = []
        self._beams_dev = self._m_dev = self._a_dev = None
        for part in parts:
            uvw, wgt, mask = _field(part, "UVW"), _field(part, "WEIGHT"), _field(part, "MASK")
            freq, beam = _field(part, "FREQ"), _field(part, "BEAM")
            l0, m0 = _attr(part, "l0", 0.0), _attr(part, "m0", 0.0)
            flip_u, flip_v, flip_w, x0, y0 = wgridder_conventions(l0, m0)
            # dirty2vis is called WITHOUT a mask in the reference (gridder.py:972-989) and vis2dirty
            # with it; masked visibilities do not survive the gridding step, so one masked handle
            # gives the identical product.
            g = Gridder(uvw, freq, mask, npix_x=nx, npix_y=ny, pixsize_x=cell_rad, pixsize_y=cell_rad, center_x=x0,
                        center_y=y0, epsilon=epsilon, flip_u=flip_u, flip_v=flip_v, flip_w=flip_w,
                        do_wgridding=do_wgridding, divide_by_n=False, sigma_min=1.1, sigma_max=3.0)
            self.items.append((g, np.asarray(wgt, dtype=np.float64), np.asarray(beam, dtype=np.float64)))

    def convim(self, model):
        ncorr = model.shape[0]
        out = np.zeros((ncorr, self.nx, self.ny), dtype=np.float64)
        for g, wgt, beam in self.items:
            for c in range(ncorr):
                g.set_weights(wgt[c])
                # beam applied once, on the degrid side (gridder.py:975, 1070)
                out[c] += g.hessian(beam[c] * model[c], beam=None, eta=0.0, wsum=0.0)
        return out

    def residual(self, dirty, model, out=None):
        """``dirty - convim(model)`` with the chain over the partitions on the device: per correlation the model and the
        dirty image go up once, every partition subtracts its ``R^H W R (beam * model)`` in the epilogue of its own apply
        (``pfbhip_gridder_residual_dev``), and the result comes down once -- no image-sized numpy pass on the host.  The
        beams stay resident in HBM from the first call on.  ``out`` (C-contiguous float64, e.g. a band of the caller's
        page-locked cube) receives the result in place."""
        ncorr = model.shape[0]
        shape = (self.nx, self.ny)
        if out is not None and (out.shape != (ncorr,) + shape or out.dtype != np.float64 or not out.flags.c_contiguous):
            raise ValueError("out must be a C-contiguous float64 array of the model's shape")
        if not self.items:
            if out is None:
                return dirty - np.zeros_like(dirty)
            out[...] = dirty
            return out
        if self._beams_dev is None:
            self._beams_dev = [[_lib.DeviceArray.from_host(np.ascontiguousarray(beam[c], dtype=np.float64)) for c in range(beam.shape[0])]
                               for _, _, beam in self.items]
            self._m_dev, self._a_dev = _lib.DeviceArray(shape, np.float64), _lib.DeviceArray(shape, np.float64)
        if out is None:
            out = _lib.result_empty((ncorr,) + shape, np.float64)
        for c in range(ncorr):
            self._m_dev.upload(model[c])
            self._a_dev.upload(dirty[c])
            for (g, wgt, _), beams in zip(self.items, self._beams_dev):
                g.set_weights(wgt[c])
                g.residual_dev(self._m_dev, self._a_dev, self._a_dev, beam_dev=beams[c])
            self._a_dev.download(out[c])
        return out

    def close(self):
        for g, _, _ in self.items:
            g.close()
        self.items = []
        for d in [b for row in (self._beams_dev or []) for b in row] + [self._m_dev, self._a_dev]:
            if d is not None:
                d.free()
        self._beams_dev = self._m_dev = self._a_dev = None


def residual_from_partitions(dirty, parts, model, cell_rad, nthreads=1, epsilon=1e-7, do_wgridding=True,
                             double_accum=True):
    """``dirty - sum_p R_p^H W_p R_p (beam_p * model)`` (gridder.py:926-1016)."""
    resize_thread_pool(nthreads)
    ncorr, nx, ny = dirty.shape
    if not _lib.any_nonzero(model):
        # degridding a zero model gives zero visibilities; skip the device entirely
        return dirty - np.zeros_like(dirty)
    state = PartitionResidual(parts, nx, ny, cell_rad, epsilon=epsilon, do_wgridding=do_wgridding)
    try:
        return state.residual(np.ascontiguousarray(dirty, dtype=np.float64), model)
    finally:
        state.close()


def compute_residual_arrays(dirty, model, uvw, freq, wgt, mask, beam, cell_rad, x0=0.0, y0=0.0, flip_u=False,
                            flip_v=True, flip_w=False, epsilon=1e-7, do_wgridding=True):
    """The arithmetic of ``compute_residual`` (gridder.py:1060-1117) on in-memory arrays:
    per correlation ``dirty2vis(beam*model)`` -> ``vis2dirty`` -> ``dirty - convim``."""
    ncorr, nx, ny = dirty.shape
    # (the plan cache of the stateless calls: the reference computes the residual of the same uvw once per major cycle)
    g, cached = _get_gridder(uvw, freq, mask, npix_x=int(nx), npix_y=int(ny), pixsize_x=float(cell_rad), pixsize_y=float(cell_rad),
                             center_x=float(x0), center_y=float(y0), epsilon=float(epsilon), flip_u=bool(flip_u), flip_v=bool(flip_v),
                             flip_w=bool(flip_w), do_wgridding=bool(do_wgridding), divide_by_n=False, sigma_min=1.1, sigma_max=3.0)
    devs = []
    try:
        # dirty - R^H W R (beam * model) in one device call per correlation: the beam is applied by the degridding side's
        # prepare step and the subtraction by the apply's last kernel (pfbhip_gridder_residual_dev)
        residual = _lib.result_empty(dirty.shape, np.float64)
        devs = [_lib.DeviceArray((nx, ny), np.float64) for _ in range(3)]
        m_dev, b_dev, a_dev = devs
        for c in range(ncorr):
            g.set_weights(wgt[c])
            m_dev.upload(model[c])
            b_dev.upload(beam[c])
            a_dev.upload(dirty[c])
            g.residual_dev(m_dev, a_dev, a_dev, beam_dev=b_dev)
            a_dev.download(residual[c])
    finally:
        for d in devs:
            d.free()
        if not cached:
            g.close()
    return residual


def image_data_products_arrays(uvw, freq, vis, wgt, mask, nx, ny, nx_psf, ny_psf, cellx, celly, model=None, beam=None,
                               robustness=None, l0=0.0, m0=0.0, nthreads=1, epsilon=1e-7, do_wgridding=True, double_accum=True,
                               l2_reweight_dof=None, wgtp=1.0, do_dirty=True, do_psf=True, do_residual=True, do_weight=True,
                               do_noise=False, do_beam=False, min_padding=1.7, filter_counts_level=5.0, npix_super=0, rng=None,
                               do_psfpars=False):
    """The arithmetic of ``image_data_products`` (gridder.py:375-757) on in-memory arrays of one (time, band) chunk:
    ``vis, wgt (ncorr, nrow, nchan)``, ``mask (nrow, nchan)``, ``model / beam (ncorr, nx, ny)``.

    Order of operations as in the reference: model visibilities (un-weighted ``dirty2vis``) -> residual visibilities ->
    optional l2 reweighting -> imaging weights on the ``min_padding``-padded grid (one device pipeline,
    :func:`~pfb_imaging_amd.utils.weighting.imaging_weights`) -> ``WSUM`` -> ``DIRTY`` -> ``PSF`` (+ ``PSFHAT =
    r2c(ifftshift(PSF))``) -> ``RESIDUAL`` -> ``NOISE``.  One device plan per output grid serves every correlation and
    every product on that grid (the tile sort does not depend on weights or values).  The zarr / xarray side
    (dataset concatenation, beam interpolation, writing ``dso``) stays with the caller.  ``do_psfpars=True`` (needs
    ``do_psf``) adds ``PSFPARSN = fitcleanbeam(PSF, level=0.5, pixsize=1.0)`` as gridder.py:666 stores it, fitted on the device.

    Returns ``(products, outputs)``: ``products`` holds the arrays the reference stores in ``dso`` (``WEIGHT, UVW, MASK,
    WSUM, DIRTY, PSF, PSFHAT, MODEL, RESIDUAL, NOISE, BEAM`` as requested) and ``outputs`` its return dict
    (``residual``, ``psf``, ``wsum``).
    """
    resize_thread_pool(nthreads)
    flip_u, flip_v, flip_w, x0, y0 = wgridder_conventions(l0, m0)
    uvw = np.require(uvw, dtype=np.float64)
    freq = np.require(freq, dtype=np.float64)
    vis = np.asarray(vis)
    wgt = np.array(wgt, dtype=np.float64)  # (a copy: the chain updates the weights in place)
    mask = np.require(mask, dtype=np.uint8)
    ncorr, nrow, nchan = vis.shape
    common = dict(pixsize_x=cellx, pixsize_y=celly, center_x=x0, center_y=y0, epsilon=epsilon, flip_u=flip_u, flip_v=flip_v,
                  flip_w=flip_w, do_wgridding=do_wgridding, divide_by_n=False, sigma_min=1.1, sigma_max=3.0)
    products, g = {}, None
    need_img_plan = do_dirty or model is not None or do_noise
    try:
        if need_img_plan:
            g = Gridder(uvw, freq, mask, npix_x=nx, npix_y=ny, **common)
        residual_vis = None
        if model is None:
            if l2_reweight_dof:
                raise ValueError("Requested l2 reweight but no model passed in. Perhaps transfer model from somewhere?")
        else:
            # model visibilities are not weighted (gridder.py:480-507); the masked plan leaves flagged samples at zero,
            # which the gridding step discards anyway
            residual_vis = np.empty(vis.shape, dtype=np.complex128)
            for c in range(ncorr):
                residual_vis[c] = vis[c] - g.dirty2vis(np.ascontiguousarray(model[c], dtype=np.float64))
        if l2_reweight_dof:
            ressq = (residual_vis * wgtp * residual_vis.conj()).real
            ssq = ressq[:, mask > 0].sum(axis=-1)
            ovar = ssq / mask.sum()
            if np.all(ovar):
                wgt *= (l2_reweight_dof + 2) / (l2_reweight_dof + ressq / ovar[:, None, None])
            else:
                raise ValueError("l2 reweighting: zero residual variance")
        if robustness is not None:
            nx_pad = int(np.ceil(min_padding * nx))
            nx_pad += nx_pad % 2
            ny_pad = int(np.ceil(min_padding * ny))
            ny_pad += ny_pad % 2
            wgt = imaging_weights(uvw, freq, mask, wgt, nx_pad, ny_pad, cellx, celly, robustness,
                                  filter_level=filter_counts_level, npix_super=npix_super,
                                  usign=1.0 if flip_u else -1.0, vsign=1.0 if flip_v else -1.0)
        if do_weight:
            products.update(WEIGHT=wgt, UVW=uvw, MASK=mask)
        wsum = wgt[:, mask.astype(bool)].sum(axis=-1)
        products["WSUM"] = wsum
        # (every correlation's image comes down straight into its slice of a page-locked cube: no np.stack copy)
        if do_dirty:
            products["DIRTY"] = _lib.result_empty((ncorr, nx, ny), np.float64)
            for c in range(ncorr):
                g.vis2dirty(vis[c], wgt[c], out=products["DIRTY"][c])
        if do_residual and model is not None:
            products["MODEL"] = np.asarray(model)
            products["RESIDUAL"] = _lib.result_empty((ncorr, nx, ny), np.float64)
            for c in range(ncorr):
                g.vis2dirty(residual_vis[c], wgt[c], out=products["RESIDUAL"][c])
        if do_noise:
            rng = np.random.default_rng() if rng is None else rng
            noise = np.empty((ncorr, nx, ny))
            for c in range(ncorr):
                nvis = rng.standard_normal((nrow, nchan)) + 1j * rng.standard_normal((nrow, nchan))
                pos = wgt[c] > 0.0
                nvis[pos] /= np.sqrt(wgt[c][pos])
                nvis[~pos] = 0j
                noise[c] = g.vis2dirty(nvis, wgt[c])
            products["NOISE"] = noise
    finally:
        if g is not None:
            g.close()
    if do_psf:
        psf_vis = psf_visibilities(uvw, freq, x0, y0, flip_u, flip_v, dtype=np.complex128)
        gp = Gridder(uvw, freq, mask, npix_x=nx_psf, npix_y=ny_psf, **common)
        try:
            psf = _lib.result_empty((ncorr, nx_psf, ny_psf), np.float64)
            for c in range(ncorr):
                gp.vis2dirty(psf_vis, wgt[c], out=psf[c])
        finally:
            gp.close()
        products["PSF"] = psf
        # r2c(ifftshift(psf)): for the even PSF sizes the shift is a checkerboard sign on the spectrum, applied on the device
        if nx_psf % 2 == 0 and ny_psf % 2 == 0:
            products["PSFHAT"] = _fft.r2c(psf, axes=(1, 2), nthreads=nthreads, forward=True, inorm=0, centred=True)
        else:
            products["PSFHAT"] = _fft.r2c(ifftshift(psf, axes=(1, 2)), axes=(1, 2), nthreads=nthreads, forward=True, inorm=0)
        if do_psfpars:
            products["PSFPARSN"] = fitcleanbeam(psf, level=0.5, pixsize=1.0)
    elif do_psfpars:
        raise ValueError("do_psfpars needs do_psf: PSFPARSN is fitted to the PSF")
    if do_beam:
        products["BEAM"] = np.ones((ncorr, nx, ny)) if beam is None else np.asarray(beam)
    outputs = {"residual": products["RESIDUAL"] if (do_residual and model is not None) else products.get("DIRTY"),
               "wsum": wsum}
    if do_psf:
        outputs["psf"] = products["PSF"]
    return products, outputs


def image_data_products_chunk(chunk, nx, ny, nx_psf, ny_psf, cellx, celly, model=None, beam=None, robustness=None, l0=0.0, m0=0.0,
                              nthreads=1, epsilon=1e-7, do_wgridding=True, l2_reweight_dof=None, wgtp=1.0, do_dirty=True,
                              do_psf=True, do_residual=True, do_weight=True, do_beam=False, min_padding=1.7,
                              filter_counts_level=5.0, npix_super=0, do_psfpars=False):
    """:func:`image_data_products_arrays` of a chunk that is resident in HBM (:class:`~pfb_imaging_amd.vischunk.VisChunk`): the
    same order of operations (gridder.py:375-757 of the reference), the same ``(products, outputs)`` and keys, no
    per-correlation, per-product upload of visibilities and weights.

    Model visibilities are degridded from the uploaded model straight into the residual visibilities
    (``Gridder.dirty2vis_rows_dev`` with the chunk's visibilities as the minuend), which stay in HBM; the l2 reweighting and
    the imaging weights run in place on ``chunk.wgt`` (so the chunk's weights are the products' ``WEIGHT`` afterwards, as the
    reference's ``wgt`` is); ``WSUM`` is reduced on the device; ``DIRTY``, ``RESIDUAL`` and ``PSF`` are gridded from the
    chunk's rows, the PSF's visibilities being formed inside the sort kernel.  One plan per output grid serves every
    correlation.  What crosses PCIe: the model, once per correlation, up; the images and ``WSUM`` down; ``WEIGHT`` down only
    with ``do_weight``; the PSF up again for ``PSFHAT`` (``fft.r2c`` takes host arrays) and ``PSFPARSN``.

    ``do_noise`` is not offered: its random draw is the host's (``rng.standard_normal`` per correlation), so its visibilities
    would be uploaded like the array path's; use :func:`image_data_products_arrays` for it.  ``wgtp`` is a scalar, a host
    array or a float64 ``DeviceArray`` of the chunk's shape.

    Device memory held: the chunk's ``ncorr * 24 + 1`` bytes per sample, ``ncorr * 16`` more per sample while a model is
    given, one image per grid and the plans."""
    from ..vischunk import VisChunk

    if not isinstance(chunk, VisChunk):
        raise TypeError(f"chunk must be a VisChunk, not {type(chunk).__name__}")
    if do_psfpars and not do_psf:
        raise ValueError("do_psfpars needs do_psf: PSFPARSN is fitted to the PSF")
    ncorr = chunk.ncorr
    if model is None:
        if l2_reweight_dof:
            raise ValueError("Requested l2 reweight but no model passed in. Perhaps transfer model from somewhere?")
    else:
        model = np.asarray(model)
        if model.shape != (ncorr, nx, ny):
            raise ValueError(f"model shape {model.shape} != {(ncorr, nx, ny)}")
        if model.dtype.kind not in "fiu":
            raise TypeError(f"model must be real, not {model.dtype}")
    if beam is not None and np.shape(beam) != (ncorr, nx, ny):
        raise ValueError(f"beam shape {np.shape(beam)} != {(ncorr, nx, ny)}")
    chunk._open()
    resize_thread_pool(nthreads)
    flip_u, flip_v, flip_w, x0, y0 = wgridder_conventions(l0, m0)
    uvw, freq, mask = chunk.uvw, chunk.freq, chunk.mask_host
    common = dict(pixsize_x=cellx, pixsize_y=celly, center_x=x0, center_y=y0, epsilon=epsilon, flip_u=flip_u, flip_v=flip_v,
                  flip_w=flip_w, do_wgridding=do_wgridding, divide_by_n=False, sigma_min=1.1, sigma_max=3.0)
    products, g, res_dev, img_dev = {}, None, None, None
    try:
        if do_dirty or model is not None:
            g = Gridder(uvw, freq, mask, npix_x=nx, npix_y=ny, **common)
            img_dev = _lib.DeviceArray((nx, ny), np.float64)
        if model is not None:
            # residual visibilities = vis - R model, un-weighted (gridder.py:480-507), formed by the un-sort of the degrid
            res_dev = _lib.DeviceArray((ncorr, chunk.nrow, chunk.nchan), np.complex128)
            for c in range(ncorr):
                off = chunk.corr_offset(c)
                img_dev.upload(model[c])
                g.dirty2vis_rows_dev(img_dev, res_dev, minuend_dev=chunk.vis, vis_offset=off, minuend_offset=off)
        if l2_reweight_dof:
            chunk.l2_reweight(res_dev, l2_reweight_dof, wgtp)
        if robustness is not None:
            nx_pad = int(np.ceil(min_padding * nx))
            nx_pad += nx_pad % 2
            ny_pad = int(np.ceil(min_padding * ny))
            ny_pad += ny_pad % 2
            chunk.imaging_weights(nx_pad, ny_pad, cellx, celly, robustness, filter_level=filter_counts_level,
                                  npix_super=npix_super, usign=1.0 if flip_u else -1.0, vsign=1.0 if flip_v else -1.0)
        if do_weight:
            products.update(WEIGHT=chunk.weights(), UVW=uvw, MASK=mask)
        wsum = chunk.wsum()
        products["WSUM"] = wsum
        if do_dirty:
            products["DIRTY"] = _lib.result_empty((ncorr, nx, ny), np.float64)
            for c in range(ncorr):
                off = chunk.corr_offset(c)
                g.vis2dirty_rows_dev(chunk.vis, chunk.wgt, img_dev, vis_offset=off, wgt_offset=off)
                img_dev.download(products["DIRTY"][c])
        if do_residual and model is not None:
            products["MODEL"] = model
            products["RESIDUAL"] = _lib.result_empty((ncorr, nx, ny), np.float64)
            for c in range(ncorr):
                off = chunk.corr_offset(c)
                g.vis2dirty_rows_dev(res_dev, chunk.wgt, img_dev, vis_offset=off, wgt_offset=off)
                img_dev.download(products["RESIDUAL"][c])
    finally:
        if g is not None:
            g.close()
        for d in (res_dev, img_dev):
            if d is not None:
                d.free()
    if do_psf:
        gp, psf_dev = Gridder(uvw, freq, mask, npix_x=nx_psf, npix_y=ny_psf, **common), None
        try:
            psf_dev = _lib.DeviceArray((nx_psf, ny_psf), np.float64)
            psf = _lib.result_empty((ncorr, nx_psf, ny_psf), np.float64)
            for c in range(ncorr):
                gp.psf_rows_dev(chunk.wgt, psf_dev, wgt_offset=chunk.corr_offset(c))
                psf_dev.download(psf[c])
        finally:
            gp.close()
            if psf_dev is not None:
                psf_dev.free()
        products["PSF"] = psf
        if nx_psf % 2 == 0 and ny_psf % 2 == 0:
            products["PSFHAT"] = _fft.r2c(psf, axes=(1, 2), nthreads=nthreads, forward=True, inorm=0, centred=True)
        else:
            products["PSFHAT"] = _fft.r2c(ifftshift(psf, axes=(1, 2)), axes=(1, 2), nthreads=nthreads, forward=True, inorm=0)
        if do_psfpars:
            products["PSFPARSN"] = fitcleanbeam(psf, level=0.5, pixsize=1.0)
    if do_beam:
        products["BEAM"] = np.ones((ncorr, nx, ny)) if beam is None else np.asarray(beam)
    outputs = {"residual": products["RESIDUAL"] if (do_residual and model is not None) else products.get("DIRTY"),
               "wsum": wsum}
    if do_psf:
        outputs["psf"] = products["PSF"]
    return products, outputs
