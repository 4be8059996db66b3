#!/usr/bin/env python3
"""Reference-RUN fixtures for the Stokes conventions (pfb_imaging_amd/utils/stokes.py, csrc/stokes.hip): stokes_pins.npz.

Run from the repo root in the build container, where the reference checkout is present:
    python tests/golden/make_stokes_pins.py

``stokes_expr_funcs``, ``stokes_to_corr``, ``corr_to_stokes`` and ``mueller_to_stokes`` (utils/stokes.py of the reference) are
taken out of the parsed module at generation time and executed as they stand, the way make_ref_pins.py takes its functions;
no source text is stored, only results and ``cites``.

  * ``stokes_expr_funcs`` looks its functions up in ``CONVERT_FNS``, generated code of another package that is absent here.
    It runs against a stand-in whose values are their own keys, so what is recorded is WHICH expressions it selects, in
    which order, or the class of the exception it raises: ``sel_case`` holds ``product|pol|nc|wgt_mode|ndim`` and
    ``sel_result`` either ``!<ExceptionClass>`` or ``<vis keys>#<weight keys>``, a key written ``KIND/POL/JONES/S`` and keys
    joined by commas.  The sweep is every combination of PRODUCTS x POLS x NCS x MODES x NDIMS below.
  * the two ``T`` matrices are read back out of ``mueller_to_stokes`` by feeding it unit Mueller matrices.
  * ``stokes_to_corr`` / ``corr_to_stokes`` run on a small random cube, along axis 0 and along axis 1.
"""

import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

PRODUCTS = ("I", "Q", "U", "V", "IQ", "QU", "UV", "IQUV", "VQI", "IX")
POLS = ("linear", "circular", "elliptical")
NCS = ("1", "2", "3", "4")
MODES = ("l2", "minvar", "huber")
NDIMS = (4, 5, 6)


class KeysAsValues(dict):
    def __missing__(self, key):
        return key


def main():
    from make_ref_pins import take

    rel = "src/pfb_imaging/utils/stokes.py"
    ns, found = take(rel, ["stokes_expr_funcs", "stokes_to_corr", "corr_to_stokes", "mueller_to_stokes"])
    cites = [f"{rel}:{a}-{b} {k}" for k, (a, b) in sorted(found.items())]
    ns["CONVERT_FNS"] = KeysAsValues()
    out = {}

    cases, results = [], []
    for product, pol, nc, mode, ndim in itertools.product(PRODUCTS, POLS, NCS, MODES, NDIMS):
        cases.append(f"{product}|{pol}|{nc}|{mode}|{ndim}")
        try:
            vis_keys, wgt_keys = ns["stokes_expr_funcs"](product, pol, nc, mode, ndim)
        except Exception as e:  # the class is the record
            results.append("!" + type(e).__name__)
            continue
        assert len(vis_keys) == len(wgt_keys)
        results.append("#".join(",".join("/".join(key) for key in keys) for keys in (vis_keys, wgt_keys)))
    out["sel_case"], out["sel_result"] = np.array(cases), np.array(results)

    # T[j, i] = mueller_to_stokes(E_ij)[i] + 1j * mueller_to_stokes(-1j E_ij)[i]: the function returns sum_j M_ij T_ji, real part
    units = np.zeros((4, 4, 16), dtype=np.complex128)
    for i, j in itertools.product(range(4), range(4)):
        units[i, j, 4 * i + j] = 1.0
    for pol in ("linear", "circular"):
        re, im = ns["mueller_to_stokes"](units, poltype=pol), ns["mueller_to_stokes"](-1j * units, poltype=pol)
        t = np.zeros((4, 4), dtype=np.complex128)
        for i, j in itertools.product(range(4), range(4)):
            t[j, i] = re[i, 4 * i + j] + 1j * im[i, 4 * i + j]
        out[f"T_{pol}"] = t

    rng = np.random.default_rng(20261020)
    stokes = rng.standard_normal((4, 3, 5))
    corr = rng.standard_normal((4, 3, 5)) + 1j * rng.standard_normal((4, 3, 5))
    out.update(cube_stokes=stokes, cube_corr=corr, cube_wsum=2.5)
    out["s2c_axis0"] = ns["stokes_to_corr"](stokes, axis=0)
    out["s2c_axis1"] = ns["stokes_to_corr"](np.moveaxis(stokes, 0, 1), axis=1)
    out["c2s_axis0"] = ns["corr_to_stokes"](corr, wsum=2.5, axis=0)
    out["c2s_axis1"] = ns["corr_to_stokes"](np.moveaxis(corr, 0, 1), wsum=2.5, axis=1)
    for f in ("stokes_to_corr", "corr_to_stokes"):
        try:
            ns[f](stokes, poltype="circular")
            raise AssertionError("circular feeds were expected to be refused")
        except NotImplementedError:
            pass

    out["cites"] = np.array(cites)
    path = os.path.join(HERE, "stokes_pins.npz")
    np.savez_compressed(path, **out)
    print("\n".join(cites))
    print("stokes_pins.npz", os.path.getsize(path), "bytes,", len(cases), "selector cases,",
          sum(r.startswith("!") for r in results), "refusals")


if __name__ == "__main__":
    from make_ref_pins import REF

    if not os.path.isdir(REF):
        sys.exit("make_stokes_pins.py needs the reference checkout (build container only); the committed .npz travels instead")
    main()
