"""Access to tests/golden/modelspec_pins.npz (written by tests/golden/make_modelspec_pins.py) for the CPU and GPU tests of the
component model: the fit cases with their inputs, and the comps2vis fixture."""

import functools
import os

import numpy as np

from . import _modelspec_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modelspec_pins.npz")

# tag -> (cube key, leading-axis slice of time, with wgt, nbasist, nbasisf, method, sigmasq)
FIT_CASES = {
    "fit_poly_0_0": ("fit_cube", 3, False, 2, 3, "poly", 0),
    "fit_poly_1_1": ("fit_cube", 3, True, 2, 3, "poly", 1e-3),
    "fit_Legendre_1_0": ("fit_cube", 3, True, 2, 3, "Legendre", 0),
    "fit_Legendre_0_1": ("fit_cube", 3, False, 2, 3, "Legendre", 1e-3),
    "fit_t1_Legendre": ("fit_cube", 1, False, 1, 3, "Legendre", 0),
    "small_poly": ("small_cube", 3, False, 2, 3, "poly", 0),
    "small_Legendre": ("small_cube", 3, False, 2, 3, "Legendre", 0),
    "c2v_fit": (None, 3, False, 2, 3, "Legendre", 0),  # (its cube is not stored: only coefficients and strings are used)
}


@functools.lru_cache(maxsize=1)
def pins():
    """The arrays of the file; the cubes, stored as support indices and values in eighths, come back dense."""
    with np.load(GOLDEN) as z:
        p = {k: z[k] for k in z.files}
    for name in ("fit_cube", "small_cube"):
        nt, nb, nx, ny = (int(v) for v in p.pop(f"{name}_shape"))
        cube = np.zeros((nt, nb, nx * ny))
        cube[:, :, p.pop(f"{name}_flat")] = p.pop(f"{name}_eighths") / 8.0
        p[name] = cube.reshape(nt, nb, nx, ny)
    return p


def fit_inputs(tag):
    """``time, freq, image (ntime, nband, nx, ny), wgt or None, nbasist, nbasisf, method, sigmasq`` of a pinned fit."""
    key, nt, with_w, nbt, nbf, method, sigmasq = FIT_CASES[tag]
    p = pins()
    return (p["time"][:nt].copy(), p["freq"].copy(), p[key][:nt], p["fit_wgt"][:nt] if with_w else None, nbt, nbf, method, sigmasq)


def fit_outputs(tag):
    """``coeffs, x_index, y_index, expr, params, texpr, fexpr, cond`` as the reference returned them."""
    p = pins()
    s = [str(v) for v in p[f"{tag}_strings"]]
    return p[f"{tag}_coeffs"], p[f"{tag}_x"], p[f"{tag}_y"], s[0], s[3:], s[1], s[2], float(p[f"{tag}_cond"])


def basis_of(tag):
    _, nt, _, nbt, nbf, method, _ = FIT_CASES[tag]
    p = pins()
    return ref.Basis(p["time"][:nt], p["freq"], nbt, nbf, method)


def c2v_fixture():
    """Arguments of the comps2vis fixture: ``(uvw, utime, freq, rbin_idx, rbin_cnts, tbin_idx, tbin_cnts, fbin_idx, fbin_cnts)``,
    the region mask, the model dataset as a dict, and the frequency range."""
    p = pins()
    coeffs, xi, yi = fit_outputs("c2v_fit")[:3]
    attrs = {str(k): float(v) for k, v in zip(p["c2v_attr_names"], p["c2v_attr_values"])}
    for k in ("npix_x", "npix_y"):
        attrs[k] = int(attrs[k])
    for k in ("flip_u", "flip_v", "flip_w"):
        attrs[k] = bool(attrs[k])
    mds = dict(coefficients=coeffs, location_x=xi, location_y=yi, attrs=attrs)
    args = tuple(p["c2v_" + k] for k in ("uvw", "utime", "freq", "rbin_idx", "rbin_cnts", "tbin_idx", "tbin_cnts", "fbin_idx",
                                         "fbin_cnts"))
    return args, p["c2v_region"], mds, dict(freq_min=float(p["c2v_frange"][0]), freq_max=float(p["c2v_frange"][1]))
