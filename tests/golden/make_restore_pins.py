#!/usr/bin/env python3
"""Reference-RUN fixtures of the Gaussian-resolution convolution and the restore step: ``restore_pins.npz``.

Like make_ref_pins.py (whose ``take()`` this script imports), this reads the reference's files AT GENERATION TIME, takes the
undecorated top-level functions ``gaussian2d``, ``get_padding_info`` and ``convolve2gaussres`` out of the parsed module and
executes them AS THEY STAND.  No reference source text is stored: only outputs and ``cites`` go into the ``.npz``; the inputs
are rebuilt from tests/_restore_ref.py ``case()`` by whoever compares.

``convolve2gaussres`` calls ducc0's ``r2c`` / ``c2r`` / ``good_size`` (wheel absent).  Those three names are bound to stand-ins
with ducc0's argument meaning (``axes``, ``forward``, ``inorm``: 0 none, 2 the full 1/N, ``lastsize``, ``out``) over an FFT
module, and to the oracle's ``good_size``; ``ifftshift`` / ``fftshift`` are bound to numpy's as the reference's module does
(misc.py:25-26).  Every convolution is run twice, over ``numpy.fft`` and over ``scipy.fft``; both outputs are stored, and
their disagreement relative to the output's max norm is the yardstick of the device tests.  This pins the padding, the
shifts, the kernel, the mask and the composition.  It does NOT pin ducc0's arithmetic.

Case D's reference is composed the way ``restore_image`` composes it (restoration.py:71-88), one band at a time as that function
is called: ``conv(model; gaussparf) + rconv``, with case C's outputs as ``rconv`` (D's residual is C's image times wsum, and wsum
holds powers of two) and the residual itself on the band whose two resolutions agree.

Run from the repo root in the build container:  python tests/golden/make_restore_pins.py
"""

import importlib.util
import os
import sys

import numpy as np
import scipy.fft

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("make_ref_pins", os.path.join(HERE, "make_ref_pins.py"))
_mrp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mrp)
take, REF = _mrp.take, _mrp.REF

PAD_CASES = ((36, 50, 0.2), (40, 40, 0.5), (8192, 8192, 0.2), (4096, 4096, 0.2), (17, 22, 0.5), (100, 7, 0.0), (33, 33, 0.05),
             (1, 1, 0.5), (8192, 4096, 0.5))
# (emaj, emin, pa), normalise, (sx, sy) on a (17, 22) grid
GAUSS_CASES = (((6.0, 3.5, 0.7), False, (1.0, 1.0)), ((6.0, 3.5, 0.7), True, (1.0, 1.0)), ((2.5, 2.0, 0.1), False, (1.0, 1.0)),
               ((30.0, 20.0, 1.1), True, (1.0, 1.0)), ((1.5e-4, 1.0e-4, -2.3), False, (2.5e-5, 2.0e-5)), ((4.0, 4.0, 0.0), True, (1.0, 1.0)))


def standins(fft):
    def r2c(a, axes, forward=True, nthreads=1, inorm=0, out=None):
        assert forward and inorm == 0
        res = fft.rfftn(a, axes=axes)
        if out is None:
            return res
        out[...] = res
        return out

    def c2r(a, axes, forward=False, lastsize=None, inorm=2, nthreads=1):
        assert not forward and inorm == 2 and lastsize is not None
        s = [a.shape[ax] for ax in axes]
        s[-1] = lastsize
        return fft.irfftn(a, s=s, axes=axes)  # carries the 1/N of inorm=2

    return r2c, c2r


def compute():
    """every array of the fixture, by name"""
    from oracle.wgridder import good_size
    from tests import _restore_ref as ref

    rel = "src/pfb_imaging/utils/misc.py"
    ns, found = take(rel, ["gaussian2d", "get_padding_info", "convolve2gaussres"])
    cites = [f"{rel}:{a}-{b} {k}" for k, (a, b) in sorted(found.items())]
    cites += [f"{rel}:25-26 ifftshift / fftshift bound to numpy.fft's, as there",
              "ducc0.fft.r2c / c2r bound to numpy.fft (_np) and scipy.fft (_sp) stand-ins with ducc0's axes / inorm / lastsize / out",
              "ducc0.fft.good_size bound to oracle.wgridder.good_size"]
    ns.update(good_size=good_size, ifftshift=np.fft.ifftshift, fftshift=np.fft.fftshift)
    out = {}

    # ---- padding and kernel ----------------------------------------------------------------------------------------
    pad = []
    for nx, ny, pfrac in PAD_CASES:
        padding, ux, uy = ns["get_padding_info"](nx, ny, pfrac)
        pad.append([padding[0][0], padding[0][1], padding[1][0], padding[1][1], ux.start, ux.stop, uy.start, uy.stop])
    out["pad_cases"] = np.array(PAD_CASES)
    out["pad_out"] = np.array(pad, dtype=np.int64)
    for k, (par, normalise, (sx, sy)) in enumerate(GAUSS_CASES):
        xx, yy = ref.offsets(17, 22, sx, sy)
        out[f"gauss_{k}"] = ns["gaussian2d"](xx, yy, par, normalise=normalise)
    out["gauss_cases"] = np.array([list(p) + [float(n), sx, sy] for p, n, (sx, sy) in GAUSS_CASES])

    # ---- convolutions ----------------------------------------------------------------------------------------------
    def run(tag, c, **kw):
        res = {}
        for name, fft in (("np", np.fft), ("sp", scipy.fft)):
            ns["r2c"], ns["c2r"] = standins(fft)
            res[name] = ns["convolve2gaussres"](c["image"].copy(), c["xx"], c["yy"], c["gaussparf"], gausspari=c["gausspari"],
                                                pfrac=c["pfrac"], **kw)
            out[f"{tag}_{name}"] = res[name]
        out[f"{tag}_disagreement"] = ref.rel_max(res["sp"], res["np"])
        mine = ref.convolve(c["image"], c["xx"], c["yy"], c["gaussparf"], c["gausspari"], c["pfrac"], kw.get("norm_kernel", False))
        print(f"{tag}: numpy vs scipy stand-ins {out[f'{tag}_disagreement']:.3e}; tests/_restore_ref.py vs numpy run "
              f"{ref.rel_max(mine, res['np']):.3e}")
        return res

    a = ref.case("A")
    run("A_norm0", a, norm_kernel=False)
    run("A_norm1", a, norm_kernel=True)
    run("B", ref.case("B"), norm_kernel=False)
    c = ref.case("C")
    # what makes case C comparable at all: the division stays away from the zero crossings of the truncated Gaussians' spectra
    ratios = []
    for p in c["gausspari"]:
        hat = np.abs(ref._hat(ref.gaussian(c["xx"], c["yy"], p), *sum((list(ref.pads(n, c["pfrac"])[:2]) for n in (36, 50)), []),
                              np.fft))
        ratios.append(hat.min() / hat.max())
    assert min(ratios) >= 1e-6, ratios
    out["C_min_over_max_thishat"] = np.array(ratios)
    rc = run("C", c, norm_kernel=False)
    assert out["C_disagreement"] <= 1e-8, out["C_disagreement"]

    # ---- restore, composed per band as restore_image is called -----------------------------------------------------
    d = ref.case("D")
    for name, fft in (("np", np.fft), ("sp", scipy.fft)):
        ns["r2c"], ns["c2r"] = standins(fft)
        img = np.empty_like(d["model"])
        for b in range(3):
            residual = d["residual"][b:b + 1] / d["wsum"][b:b + 1, None, None]
            assert np.array_equal(residual, c["image"][b:b + 1])
            if np.allclose(d["gaussparf"][b], d["gausspari"][b]):
                rconv = residual
            else:
                rconv = rc[name][b:b + 1]
            mconv = ns["convolve2gaussres"](d["model"][b:b + 1].copy(), c["xx"], c["yy"], d["gaussparf"][b], pfrac=0.2, norm_kernel=False)
            img[b] = (mconv + rconv)[0]
        out[f"D_{name}"] = img
    out["D_disagreement"] = ref.rel_max(out["D_sp"], out["D_np"])
    print(f"D: numpy vs scipy stand-ins {out['D_disagreement']:.3e}; tests/_restore_ref.py vs numpy run "
          f"{ref.rel_max(ref.restore(d['model'], d['residual'], d['wsum'], d['gausspari'], d['gaussparf']), out['D_np']):.3e}")

    out["cites"] = np.array(cites)
    return out


def main():
    out = compute()
    path = os.path.join(HERE, "restore_pins.npz")
    np.savez_compressed(path, **out)
    print("\n".join(out["cites"]))
    print("restore_pins.npz", os.path.getsize(path))
    assert os.path.getsize(path) < 500_000


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("make_restore_pins.py needs the reference checkout (build container only); the committed .npz travels instead")
    main()
