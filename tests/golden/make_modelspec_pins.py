#!/usr/bin/env python3
"""Reference-RUN fixtures of the component model: ``modelspec_pins.npz``.

Like make_ref_pins.py (whose ``take()`` this script imports; that module only runs its ``main()`` as a script), this reads
the reference's files AT GENERATION TIME, takes undecorated top-level functions out of the parsed modules and executes them
AS THEY STAND.  No reference source text is stored: only inputs and outputs go into the ``.npz``.

What is pinned (reference file:line -> what has to reproduce it):

  utils/modelspec.py:12-137     fit_image_cube        -> utils/modelspec.py, csrc/comps.hip (mask, compaction, fit)
  utils/modelspec.py:223-240    eval_coeffs_to_cube   -> utils/modelspec.py, csrc/comps.hip (render)
  utils/modelspec.py:243-332    eval_coeffs_to_slice  -> utils/modelspec.py, csrc/comps.hip (render, regrid)
  operators/gridder.py:276-367  _comps2vis_impl       -> operators/gridder.py comps2vis

``_comps2vis_impl`` is executed with ``dirty2vis`` bound to this repository's direct-DFT oracle (oracle/dft.py) and
``resize_thread_pool`` bound to a no-op.  That pins the row / time / channel bookkeeping, the region-mask and
frequency-range rules and the replication over ``product``.  It does NOT pin ducc0's arithmetic (wheel absent).

``_comps2vis_impl`` degrids every row of the ``uvw`` it is given for each time chunk and assigns the result to that chunk's
row slice (:335, :350-351), so a call that holds two time chunks fails with a shape error; the attempt is recorded
(``c2v_whole_call_raises``).  The reference's dask layer never makes such a call: it hands the function one time chunk at a
time (core/degrid.py:266-279: ``tidx`` / ``tcnts`` in chunks of 1, rows and unique times in chunks of one image).  The two
time chunks of the fixture are therefore pinned the way that layer calls the function -- one call per time chunk with that
chunk's blocks of uvw / utime / rbin / tbin, all bands in the call -- and stacked along the rows.

Every pinned fit asserts ``cond(hess_coeffs) < 1e8`` (times 1000 + [0, 300, 600], frequencies 1e9 [1, 1.1, 1.2, 1.3]);
``hess_coeffs`` is recomputed here from the reference's formula through tests/_modelspec_ref.py, and the restatement's
coefficients are checked against the reference's before anything is written.

Run from the repo root in the build container:  python tests/golden/make_modelspec_pins.py
"""

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("make_ref_pins", os.path.join(HERE, "make_ref_pins.py"))
_mrp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mrp)
take, REF = _mrp.take, _mrp.REF

TIME = 1000.0 + np.array([0.0, 300.0, 600.0])
FREQ = 1e9 * np.array([1.0, 1.1, 1.2, 1.3])
# (method, with wgt, sigmasq): both methods, each with and without weights and with and without the regulariser
FIT_CASES = (("poly", False, 0), ("poly", True, 1e-3), ("Legendre", True, 0), ("Legendre", False, 1e-3))


def fit_cube(rng):
    """(3, 4, 300, 260), about 3000 support pixels, values k / 8 with small integer k (the file compresses)."""
    nt, nb, nx, ny = 3, 4, 300, 260
    cube = np.zeros((nt, nb, nx, ny))

    def vals(n):
        v = rng.integers(-40, 41, size=(nt, nb, n)).astype(float)
        v[v == 0] = 3.0
        return v / 8.0

    zero_rows = np.arange(100, 121)  # 21 rows * 260 = 5460 all-zero pixels: more than five 1024-pixel workgroups
    free = np.setdiff1d(np.arange(nx), np.concatenate([zero_rows, [50]]))
    px = rng.choice(free, 2740)
    py = rng.integers(0, ny, 2740)
    cube[:, :, px, py] = vals(2740)
    cube[:, :, 50, :] = vals(ny)                       # one full image row
    cube[:, :, 0, 0] = vals(1)[:, :, 0]                # first and last pixel
    cube[:, :, nx - 1, ny - 1] = vals(1)[:, :, 0]
    cube[:, :, 10, 7] = 0.0                            # nonzero in exactly one plane
    cube[2, 1, 10, 7] = -1.25
    cube[:, :, 11, 200] = 0.0                          # nonzero values that sum to zero
    cube[0, 0, 11, 200], cube[1, 2, 11, 200], cube[2, 3, 11, 200] = 2.5, -1.5, -1.0
    cube[:, :, zero_rows, :] = 0.0
    return cube


def small_cube(rng, nx, ny, ncomp):
    cube = np.zeros((3, 4, nx, ny))
    px, py = rng.integers(0, nx, ncomp), rng.integers(0, ny, ncomp)
    cube[:, :, px, py] = rng.integers(-40, 41, size=(3, 4, ncomp)) / 8.0
    cube[:, :, 0, 0] = 1.5
    cube[:, :, nx - 1, ny - 1] = -2.25
    cube[:, :, 0, ny - 1] = 0.75
    cube[:, :, nx - 1, 0] = 1.0
    return cube


def sparse(name, cube):
    """The cube as its shape, the flat indices of its support pixels and, per plane, the values there in eighths (int8: every
    fixture value is k / 8 with |k| <= 40).  tests/_modelspec_pins.py puts it together again."""
    nt, nb, nx, ny = cube.shape
    flat = np.flatnonzero(np.any(cube != 0, axis=(0, 1)).ravel())
    eighths = cube.reshape(nt, nb, -1)[:, :, flat] * 8
    assert np.array_equal(eighths, np.round(eighths)) and np.abs(eighths).max() <= 127
    return {f"{name}_shape": np.array(cube.shape), f"{name}_flat": flat.astype(np.int32), f"{name}_eighths": eighths.astype(np.int8)}


def main():
    from oracle.dft import dft_dirty2vis
    from tests import _modelspec_ref as ref

    rng = np.random.default_rng(314159)
    out, cites = {}, []
    m_ns, found = take("src/pfb_imaging/utils/modelspec.py", ["fit_image_cube", "eval_coeffs_to_cube", "eval_coeffs_to_slice"])
    cites += [f"src/pfb_imaging/utils/modelspec.py:{a}-{b} {k}" for k, (a, b) in sorted(found.items())]
    fit_image_cube, to_cube, to_slice = m_ns["fit_image_cube"], m_ns["eval_coeffs_to_cube"], m_ns["eval_coeffs_to_slice"]

    # ---- fit / compaction -------------------------------------------------------------------------------------
    cube = fit_cube(rng)
    wgt = 0.5 + rng.random((3, 4))
    out.update(time=TIME, freq=FREQ, fit_wgt=wgt, **sparse("fit_cube", cube))
    ratios = []

    def pin_fit(tag, time, freq, img, w, nbt, nbf, method, sigmasq):
        coeffs, xi, yi, expr, params, tf, ff = fit_image_cube(time.copy(), freq.copy(), img, wgt=w, nbasist=nbt, nbasisf=nbf,
                                                              method=method, sigmasq=sigmasq)
        xfit, wv, hess, _ = ref.design(time, freq, w, nbt, nbf, method, sigmasq)
        cond = float(np.linalg.cond(hess))
        assert cond < 1e8, (tag, cond)
        mine, _ = ref.fit(img.reshape(-1, *img.shape[2:]), ref.fit_matrix(xfit, wv, hess), xi, yi)
        ratios.append(np.abs(mine - coeffs).max() / (cond * ref.EPS * np.abs(coeffs).max()))
        out.update({f"{tag}_coeffs": coeffs, f"{tag}_x": xi, f"{tag}_y": yi, f"{tag}_cond": cond,
                    f"{tag}_strings": np.array([expr, tf, ff] + list(params))})
        return coeffs, xi, yi, expr, params, tf, ff

    for method, with_w, sigmasq in FIT_CASES:
        pin_fit(f"fit_{method}_{int(with_w)}_{int(bool(sigmasq))}", TIME, FREQ, cube, wgt if with_w else None, 2, 3, method, sigmasq)
    pin_fit("fit_t1_Legendre", TIME[:1], FREQ, cube[:1], None, 1, 3, "Legendre", 0)
    try:  # ntime == nband == 1: the reference's "nothing to fit" branch leaves xfit / tfunc / ffunc unbound
        fit_image_cube(TIME[:1], FREQ[:1], cube[:1, :1])
        out["fit_11_raises"] = ""
    except Exception as e:
        out["fit_11_raises"] = type(e).__name__

    # ---- render to a cube, render + regrid to a slice ---------------------------------------------------------
    nxi, nyi = 40, 28
    small = small_cube(rng, nxi, nyi, 60)
    out.update(sparse("small_cube", small))
    etime, efreq = np.array([1100.0, 1555.5]), np.array([1.05e9, 1.27e9])
    out.update(eval_time=etime, eval_freq=efreq)
    cell = 2.0e-5
    # (nxo, nyo, cellxo, cellyo, x0o, y0o): finer + shifted (zero padding on all four sides), coarser inside, odd sizes, identical
    grids = ((50, 37, 0.9 * cell, 0.9 * cell, 1.3 * cell, -0.7 * cell), (16, 12, 1.7 * cell, 1.6 * cell, 0.5 * cell, 0.25 * cell),
             (33, 21, 1.1 * cell, 1.3 * cell, -0.4 * cell, 0.9 * cell), (nxi, nyi, cell, cell, 0.0, 0.0))
    out["slice_grids"] = np.array(grids)
    out["slice_in"] = np.array([nxi, nyi, cell, cell, 0.0, 0.0])
    for method in ("poly", "Legendre"):
        coeffs, xi, yi, expr, params, tf, ff = pin_fit(f"small_{method}", TIME, FREQ, small, None, 2, 3, method, 0)
        out[f"cube_{method}"] = to_cube(etime, efreq, nxi, nyi, coeffs, xi, yi, expr, params, tf, ff)
        for k, (nxo, nyo, cxo, cyo, x0o, y0o) in enumerate(grids):
            out[f"slice_{method}_{k}"] = to_slice(etime[1], efreq[0], coeffs, xi, yi, expr, params, tf, ff, nxi, nyi, cell, cell, 0.0,
                                                  0.0, nxo, nyo, cxo, cyo, x0o, y0o)

    # ---- comps2vis bookkeeping --------------------------------------------------------------------------------
    g_ns, found = take("src/pfb_imaging/operators/gridder.py", ["_comps2vis_impl"])
    cites += [f"src/pfb_imaging/operators/gridder.py:{a}-{b} {k}" for k, (a, b) in sorted(found.items())]
    c2v = g_ns["_comps2vis_impl"]
    g_ns["resize_thread_pool"] = lambda n: None

    def dft(uvw, freq, dirty, pixsize_x, pixsize_y, center_x, center_y, flip_u, flip_v, flip_w, epsilon, do_wgridding, divide_by_n,
            nthreads):
        return dft_dirty2vis(uvw, freq, dirty, pixsize_x, pixsize_y, center_x, center_y, flip_u, flip_v, flip_w, do_wgridding,
                             divide_by_n)

    g_ns["dirty2vis"] = dft
    nx, ny, nrow = 64, 48, 400
    # Components at least 8 pixels inside the border.  The w-gridder divides the image by its kernel's transform, which at
    # this plan (sigma 1.25, W 15) amplifies a 2e-16 relative change of an EDGE pixel to 3e-12 in the visibilities (5e-16 for
    # these inner ones; measured on the existing dirty2vis): with edge components the comparison of two
    # equally rounded renders at 1e-12 would measure the gridder's edge conditioning, not comps2vis.  Corner and edge
    # components are covered by the fit / render / regrid fixtures above.
    ccube = np.zeros((3, 4, nx, ny))
    ccube[:, :, 8:-8, 8:-8] = small_cube(rng, nx - 16, ny - 16, 40)
    coeffs, xi, yi, expr, params, tf, ff = pin_fit("c2v_fit", TIME, FREQ, ccube, None, 2, 3, "Legendre", 0)
    import sympy as sm
    from sympy.parsing.sympy_parser import parse_expr
    from sympy.utilities.lambdify import lambdify

    syms = sm.symbols(("t", "f")) + sm.symbols(tuple(params))
    modelf, tfunc, ffunc = lambdify(syms, parse_expr(expr)), lambdify(syms[0], parse_expr(tf)), lambdify(syms[1], parse_expr(ff))
    utime = 1000.0 + 150.0 * np.arange(4)                 # 2 time chunks of 2 unique times
    rbin_cnts = np.array([90, 110, 120, 80])
    rbin_idx = np.concatenate([[0], np.cumsum(rbin_cnts)[:-1]])
    tbin_idx, tbin_cnts = np.array([0, 2]), np.array([2, 2])
    cfreq = 1e9 * np.array([1.0, 1.04, 1.1, 1.14, 1.2, 1.24])  # 3 bands of 2 channels
    fbin_idx, fbin_cnts = np.array([0, 2, 4]), np.array([2, 2, 2])
    uvw = rng.standard_normal((nrow, 3)) * np.array([300.0, 300.0, 30.0])
    ccell = 4.0e-5
    region = np.ones((nx, ny), dtype=bool)
    region[:, : ny // 3] = False                           # removes some components
    assert 0 < region[xi, yi].sum() < xi.size
    attrs = dict(cell_rad_x=ccell, cell_rad_y=7 * ccell, npix_x=nx, npix_y=ny, center_x=1.0e-4, center_y=-2.0e-4, flip_u=False,
                 flip_v=True, flip_w=False)
    mds = types.SimpleNamespace(coefficients=types.SimpleNamespace(values=coeffs, dtype=coeffs.dtype),
                                location_x=types.SimpleNamespace(values=xi), location_y=types.SimpleNamespace(values=yi), **attrs)
    kw = dict(epsilon=1e-7, nthreads=1, do_wgridding=True, divide_by_n=False, product="IQ")
    args = (rbin_idx, rbin_cnts, tbin_idx, tbin_cnts, fbin_idx, fbin_cnts)
    try:
        c2v(uvw, utime, cfreq, *args, region, mds, modelf, tfunc, ffunc, **kw)
        out["c2v_whole_call_raises"] = ""
    except ValueError as e:
        out["c2v_whole_call_raises"] = type(e).__name__
    print("whole call with two time chunks:", repr(str(out["c2v_whole_call_raises"])))

    def per_chunk(region_mask, mf, **extra):
        """one call per time chunk, the blocks the reference's dask layer hands to _comps2vis (core/degrid.py:266-279)"""
        rows = []
        for t in range(tbin_idx.size):
            ts = slice(tbin_idx[t], tbin_idx[t] + tbin_cnts[t])
            rs = slice(rbin_idx[ts][0], rbin_idx[ts][-1] + rbin_cnts[ts][-1])
            rows.append(c2v(uvw[rs], utime[ts], cfreq, rbin_idx[ts], rbin_cnts[ts], tbin_idx[t:t + 1], tbin_cnts[t:t + 1], fbin_idx,
                            fbin_cnts, region_mask, mds, mf, tfunc, ffunc, **kw, **extra))
        return np.concatenate(rows, axis=0)

    frange = dict(freq_min=0.99e9, freq_max=1.15e9)        # the third band lies outside
    out["c2v_vis"] = per_chunk(region, modelf, **frange)
    out["c2v_vis_zero_region"] = per_chunk(np.zeros((nx, ny), dtype=bool), modelf, **frange)
    out["c2v_vis_nonlinear"] = per_chunk(region, ref.nonlinear_modelf, **frange)
    assert not out["c2v_vis_zero_region"].any() and not out["c2v_vis"][:, 4:].any() and out["c2v_vis"][:, :4].all()
    assert np.array_equal(out["c2v_vis"][..., 0], out["c2v_vis"][..., 1])
    out.update(c2v_uvw=uvw, c2v_utime=utime, c2v_freq=cfreq, c2v_rbin_idx=rbin_idx, c2v_rbin_cnts=rbin_cnts, c2v_tbin_idx=tbin_idx,
               c2v_tbin_cnts=tbin_cnts, c2v_fbin_idx=fbin_idx, c2v_fbin_cnts=fbin_cnts, c2v_region=region,
               c2v_attr_names=np.array(sorted(attrs)), c2v_attr_values=np.array([float(attrs[k]) for k in sorted(attrs)]),
               c2v_frange=np.array([frange["freq_min"], frange["freq_max"]]))

    print("fit: restatement vs reference, |diff| / (cond eps |coeffs|_inf), per pinned fit:", np.array(ratios))
    out["fit_ratio_observed"] = np.array(ratios)
    out["cites"] = np.array(cites)
    path = os.path.join(HERE, "modelspec_pins.npz")
    np.savez_compressed(path, **out)
    print("\n".join(cites))
    print("modelspec_pins.npz", os.path.getsize(path))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("make_modelspec_pins.py needs the reference checkout (build container only); the committed .npz travels instead")
    main()
