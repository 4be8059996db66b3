"""Times one `pfb hci` snapshot both ways: ``utils.stokes2im.stokes_image_arrays`` (the chunk stays in HBM from the Stokes
conversion to the float32 cube) against the same chain written with the host-array entry points that existed before it --
``weight_data``, numpy rephase / subtract / reweight, ``imaging_weights``, ``wgridder.vis2dirty`` twice per Stokes with the
conjugated host ramp, numpy normalise / std / cast / transpose, ``fitcleanbeam``.  The protocol of tools/bench_vischunk.py: one
process, the two paths alternate after an untimed run of each, host clock around calls that return with their streams
idle, median (min - max).  PCIe bytes are counted from the shapes, plan creation (equal on both paths) left out.

The finish entry and the rephase pass are also timed alone against device-to-device copies in the same process; rates count
every byte read and written (a copy of B bytes moves 2 B).  The finish kernels are bracketed by device events inside the
entry (``info["device_ms"]``) and held against a copy that moves the same number of bytes.

    python tools/bench_snapshot.py [--nrow 2016 --nchan 64 --npix 2048 --repeats 5 --out FILE]
"""

import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C0 = 299792458.0


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(min_ms=round(float(ts.min()), 3), median_ms=round(float(np.median(ts)), 3), max_ms=round(float(ts.max()), 3), n=len(ts))


def timed(f, n):
    f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return ts


def host_chain(raw, uvw, freq, model, w_diff, dof, nx, ny, cell, robust, min_padding=1.7):
    """The snapshot with the entry points the package had before utils/stokes2im.py"""
    from pfb_imaging_amd.utils.misc import fitcleanbeam
    from pfb_imaging_amd.utils.stokes2im import pad_size, psf_size
    from pfb_imaging_amd.utils.weighting import imaging_weights, weight_data
    from pfb_imaging_amd.wgridder import clear_cache, vis2dirty

    clear_cache()  # (every snapshot of a run has its own uvw: no plan is ever reused; the resident path builds its two as well)
    flag = raw[2]
    data, weight = weight_data(*raw, "linear", "IQUV", "4", "l2")
    mask = (~flag.any(axis=-1)).astype(np.uint8)
    p = np.exp(-2j * np.pi * freq[None, :] / C0 * w_diff[:, None])[:, :, None]
    data = (data * p - model * p) * mask[:, :, None]
    ressq = (data * data.conj()).real * mask[:, :, None]
    ovar = ressq.sum() / mask.sum()
    weight = (dof + 1) / (dof + ressq / ovar) / ovar
    data = np.ascontiguousarray(data.transpose(2, 0, 1))
    weight = np.ascontiguousarray(weight.transpose(2, 0, 1))
    weight = imaging_weights(uvw, freq, mask, weight, pad_size(nx, min_padding), pad_size(ny, min_padding), cell, cell, robust,
                             filter_level=5.0, npix_super=0, usign=-1.0, vsign=1.0)
    nxp, nyp = psf_size(nx, ny, None)
    psf_vis = np.ones((uvw.shape[0], freq.size), dtype=np.complex128)  # (the conjugated ramp at the phase centre)
    ns = weight.shape[0]
    residual, psf, rms, wsum = np.zeros((ns, nx, ny)), np.zeros((ns, nxp, nyp)), np.zeros(ns), np.zeros(ns)
    kw = dict(uvw=uvw, freq=freq, mask=mask, pixsize_x=cell, pixsize_y=cell, center_x=0.0, center_y=0.0, epsilon=1e-7, flip_u=False,
              flip_v=True, flip_w=False, do_wgridding=True, divide_by_n=True, sigma_min=min_padding)
    for c in range(ns):
        vis2dirty(vis=data[c], wgt=weight[c], npix_x=nx, npix_y=ny, dirty=residual[c], **kw)
        vis2dirty(vis=psf_vis, wgt=weight[c], npix_x=nxp, npix_y=nyp, dirty=psf[c], **kw)
    for c in range(ns):
        wsum[c] = psf[c].max()
        psf[c] /= wsum[c]
        residual[c] /= wsum[c]
        rms[c] = np.std(residual[c])
    pars = fitcleanbeam(psf, level=0.5, pixsize=np.rad2deg(cell))
    return dict(cube=np.ascontiguousarray(np.transpose(residual.astype(np.float32), (0, 2, 1))),
                psf=np.ascontiguousarray(np.transpose(psf.astype(np.float32), (0, 2, 1))), weight=wsum, rms=rms, pars=pars)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nrow", type=int, default=2016)
    ap.add_argument("--nchan", type=int, default=64)
    ap.add_argument("--npix", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from pfb_imaging_amd import _lib
    from pfb_imaging_amd._lib import DeviceArray
    from pfb_imaging_amd.utils import synth
    from pfb_imaging_amd.utils.stokes2im import pad_size, snapshot_finish, stokes_image_arrays
    from pfb_imaging_amd.vischunk import VisChunk

    _lib.require_gpu()
    nrow, nchan, nx = a.nrow, a.nchan, a.npix
    ny, ns, nant, ntime = nx, 4, 64, 1
    rng = np.random.default_rng(5)
    s = synth.make_case(nrow, nchan, nx, zscale=0.05, seed=3, with_vis=False)
    uvw, freq, cell = s["uvw"], s["freq"], s["cell"]
    shape = (nrow, nchan, 4)
    data = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    weight = rng.uniform(0.5, 2.0, shape)
    flag = rng.random(shape) < 0.01
    jones = np.zeros((ntime, nant, nchan, 1, 2, 2), dtype=np.complex128)
    jones[..., 0, 0] = jones[..., 1, 1] = 1.0
    jones += 0.1 * (rng.standard_normal(jones.shape) + 1j * rng.standard_normal(jones.shape))
    ant1, ant2 = rng.integers(0, nant, nrow), rng.integers(0, nant, nrow)
    raw = (data, weight, flag, jones, np.array([0]), np.array([nrow]), ant1, ant2)
    model3 = 0.1 * (rng.standard_normal((nrow, nchan, ns)) + 1j * rng.standard_normal((nrow, nchan, ns)))
    model = np.ascontiguousarray(model3.transpose(2, 0, 1))
    w_diff = rng.uniform(-20.0, 20.0, nrow)
    kw = dict(model_vis=model, w_diff=w_diff, l2_reweight_dof=5, robustness=0.0, psf_out=True)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    th, td, worst = [], [], {}
    for it in range(a.repeats + 1):  # (iteration 0 warms both paths up)
        t0 = time.perf_counter()
        h = host_chain(raw, uvw, freq, model3, w_diff, 5, nx, ny, cell, 0.0)
        t1 = time.perf_counter()
        d = stokes_image_arrays(*raw, uvw, freq, "linear", "IQUV", "4", "l2", nx, ny, cell, **kw)
        t2 = time.perf_counter()
        if it == 0:
            for key in ("cube", "psf", "weight", "rms"):
                worst[key] = float(np.linalg.norm(d[key].astype(np.float64) - h[key]) / np.linalg.norm(h[key]))
        else:
            th.append(t1 - t0)
            td.append(t2 - t1)
        del h, d
    nvis = nrow * nchan
    img, psf = nx * ny, 128 * 128
    npad = pad_size(nx, 1.7)
    raw_up = nvis * 4 * (16 + 8 + 1) + jones.nbytes + nrow * 8
    host_bytes = (raw_up + nvis * ns * 24                                  # weight_data: raw up, Stokes visibilities and weights down
                  + nrow * 24 + nvis * (1 + 2 * ns * 8)                    # imaging_weights: uvw, mask, weights up; weights down
                  + ns * (2 * nvis * 24 + (img + psf) * 8)                 # two vis2dirty per Stokes: vis, weights up; images down
                  + ns * psf * 8 + ns * 24)                                # fitcleanbeam: PSF up, parameters down
    dev_bytes = (raw_up + nvis                                             # raw up, the mask down once (the plans are built from it)
                 + nvis * ns * 16 + nrow * 8                               # model and w_diff up
                 + nrow * 24                                               # uvw up for the imaging weights
                 + ns * (img + psf) * 4 + ns * (8 + 8 + 8 + 24))           # float32 cube and PSF down; wsum, psf_max, rms, beam
    emit(dict(what="snapshot chain", nrow=nrow, nchan=nchan, ns=ns, nx=nx, npad=npad, robustness=0.0, host_arrays=stats(th),
              resident=stats(td), host_pcie_bytes=host_bytes, resident_pcie_bytes=dev_bytes, rel_l2_resident_vs_host=worst))

    # -- the finish entry alone, against copies of the same bytes
    res = DeviceArray.from_host(rng.standard_normal((ns, nx, ny)))
    pf = DeviceArray.from_host(rng.uniform(0.1, 1.0, (ns, 128, 128)))
    cp = DeviceArray((ns, nx, ny), np.float64)
    out32 = DeviceArray((ns, nx, ny), np.float32)
    host32 = _lib.result_empty((ns, nx, ny), np.float32)
    small = DeviceArray.from_host(rng.standard_normal((ns, 32, 32)))
    try:
        info, dev_ms = {}, []

        def fin():
            snapshot_finish(res, pf, np.ones(ns), psf_out=True, info=info)
            dev_ms.append(info["device_ms"])

        t_fin = timed(fin, a.repeats)
        dev_ms = np.asarray(dev_ms[1:]) * 1e-3  # (timed() runs one untimed call first)
        t_d2h = timed(lambda: out32.download(host32), a.repeats)
        kernel_bytes = ns * (img * (16 + 8 + 4) + psf * (8 + 16 + 4))  # normalise r+w, rms pass r, cube w; PSF: max r, normalise r+w, w
        # the yardstick moves the same bytes: a device copy of kernel_bytes / 2 reads and writes kernel_bytes (the residual
        # cube copied as often as it takes, the rest as a partial copy)
        full, rest = divmod(kernel_bytes // 2, res.nbytes)

        def copy_same_bytes():
            for _ in range(full):
                _lib.check(_lib.lib().pfbhip_memcpy_d2d(cp.ptr, res.ptr, ct.c_size_t(res.nbytes)))
            if rest:
                _lib.check(_lib.lib().pfbhip_memcpy_d2d(cp.ptr, res.ptr, ct.c_size_t(rest)))
            _lib.check(_lib.lib().pfbhip_synchronize())

        t_d2d = timed(copy_same_bytes, a.repeats)
        # the same entry on 32 x 32 planes: its seven launches, its small copies and the wait, next to no bytes
        t_fixed = timed(lambda: snapshot_finish(small, pf, np.ones(ns), psf_out=True), a.repeats)
        emit(dict(what="finish entry", ns=ns, nx=nx, entry=stats(t_fin), kernels_device_events=stats(dev_ms),
                  d2h_of_the_float32_cube=stats(t_d2h), d2d_copy_of_the_same_bytes=stats(t_d2d), entry_on_32x32_planes=stats(t_fixed),
                  kernel_bytes=kernel_bytes, kernels_GBps=round(kernel_bytes / np.median(dev_ms) / 1e9, 1),
                  copy_GBps=round(kernel_bytes / np.median(t_d2d) / 1e9, 1)))
    finally:
        for x in (res, pf, cp, out32, small):
            x.free()

    # -- the rephase pass alone
    vis = np.ascontiguousarray(model)
    ch = VisChunk(uvw, freq, vis, np.ones((ns, nrow, nchan)), np.ones((nrow, nchan), dtype=np.uint8))
    md, cp = DeviceArray.from_host(model), DeviceArray(model.shape, np.complex128)
    wd = DeviceArray.from_host(w_diff)
    try:
        call = lambda: _lib.check(_lib.lib().pfbhip_chunk_rephase_residual_dev(  # noqa: E731
            ch.vis.ptr, md.ptr, ch.mask.ptr, wd.ptr, _lib.ptr(ch.freq), _lib.i64(ns), _lib.i64(nrow), _lib.i64(nchan)))
        t_re = timed(call, 4 * a.repeats)
        t_cp = timed(lambda: (_lib.check(_lib.lib().pfbhip_memcpy_d2d(cp.ptr, md.ptr, ct.c_size_t(md.nbytes))),
                              _lib.check(_lib.lib().pfbhip_synchronize())), 4 * a.repeats)
        nb = ns * nvis * 48 + nvis
        emit(dict(what="rephase pass (entry: fc upload, kernel, wait)", bytes=nb, entry=stats(t_re), d2d_copy_of_the_model=stats(t_cp),
                  entry_GBps=round(nb / np.median(t_re) / 1e9, 1), copy_GBps=round(2 * md.nbytes / np.median(t_cp) / 1e9, 1)))
    finally:
        ch.close()
        for x in (md, cp, wd):
            x.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
