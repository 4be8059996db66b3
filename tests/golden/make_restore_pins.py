#!/usr/bin/env python3
"""Reference-RUN fixtures of the Gaussian-resolution convolution and the restore step: ``restore_pins.npz`` (cases A-D) and
``restore_edge_pins.npz`` (the edge cases E-L of tests/_restore_ref.py; of each only the numpy-FFT output, the scalar
disagreement with the scipy-FFT run and min / max ``|thishat|``; K is composed per band as D is).

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


def reference():
    """the namespace of the reference's functions with their imports bound, and the cites"""
    from oracle.wgridder import good_size

    rel = "src/pfb_imaging/utils/misc.py"
    ns, found = take(rel, ["gaussian2d", "get_padding_info", "convolve2gaussres"])
    cites = [f"{rel}:{a}-{b} {k}" for k, (a, b) in sorted(found.items())]
    cites += [f"{rel}:25-26 ifftshift / fftshift bound to numpy.fft's, as there",
              "ducc0.fft.r2c / c2r bound to numpy.fft (_np) and scipy.fft (_sp) stand-ins with ducc0's axes / inorm / lastsize / out",
              "ducc0.fft.good_size bound to oracle.wgridder.good_size"]
    ns.update(good_size=good_size, ifftshift=np.fft.ifftshift, fftshift=np.fft.fftshift)
    return ns, cites


def compute_edge():
    """every array of ``restore_edge_pins.npz``: per run of ``_restore_ref.EDGE_RUNS`` and for the restore K the numpy-FFT
    output, its disagreement with the scipy-FFT run (a scalar) and, of a ratio run, min / max of ``|thishat|`` per band"""
    from tests import _restore_ref as ref

    ns, cites = reference()
    out = {}

    def both(image, xx, yy, gaussparf, gausspari, pfrac, norm):
        res = []
        for fft in (np.fft, scipy.fft):
            ns["r2c"], ns["c2r"] = standins(fft)
            res.append(ns["convolve2gaussres"](image.copy(), xx, yy, gaussparf, gausspari=gausspari, pfrac=pfrac, norm_kernel=norm))
        return res

    for tag, (name, norm) in ref.EDGE_RUNS.items():
        c = ref.case(name)
        out[f"{tag}_np"], sp = both(c["image"], c["xx"], c["yy"], c["gaussparf"], c["gausspari"], c["pfrac"], norm)
        out[f"{tag}_disagreement"] = ref.rel_max(sp, out[f"{tag}_np"])
        mine = ref.convolve(c["image"], c["xx"], c["yy"], c["gaussparf"], c["gausspari"], c["pfrac"], norm)
        line = f"{tag}: numpy vs scipy stand-ins {out[f'{tag}_disagreement']:.3e}; tests/_restore_ref.py vs numpy run " \
               f"{ref.rel_max(mine, out[f'{tag}_np']):.3e}"
        if c["gausspari"] is not None:
            hat = np.abs(ref.thishat(c, norm))
            out[f"{tag}_min_over_max_thishat"] = hat.min(axis=(1, 2)) / hat.max(axis=(1, 2))
            assert out[f"{tag}_min_over_max_thishat"].min() >= 1e-6, (tag, out[f"{tag}_min_over_max_thishat"])
            line += f"; min / max |thishat| {out[f'{tag}_min_over_max_thishat'].min():.1e}"
        print(line)

    # K, composed per band as restore_image is called (see D below)
    k = ref.case("K")
    xx, yy = ref.offsets(*k["model"].shape[1:])
    img = [np.empty_like(k["model"]), np.empty_like(k["model"])]
    hats = []
    for b in range(k["model"].shape[0]):
        residual = k["residual"][b:b + 1] / k["wsum"][b:b + 1, None, None]
        mconv = both(k["model"][b:b + 1], xx, yy, k["gaussparf"][b], None, 0.2, False)
        if np.allclose(k["gaussparf"][b], k["gausspari"][b]):
            rconv = [residual, residual]
        else:
            rconv = both(residual, xx, yy, k["gaussparf"][b], k["gausspari"][b:b + 1], 0.2, False)
            hat = np.abs(ref.thishat(dict(image=residual, xx=xx, yy=yy, gausspari=k["gausspari"][b:b + 1], pfrac=0.2)))
            hats.append(hat.min() / hat.max())
        for i in range(2):
            img[i][b] = (mconv[i] + rconv[i])[0]
    out["K_np"], out["K_disagreement"], out["K_min_over_max_thishat"] = img[0], ref.rel_max(img[1], img[0]), np.array(hats)
    assert min(hats) >= 1e-6, hats
    print(f"K: numpy vs scipy stand-ins {out['K_disagreement']:.3e}; tests/_restore_ref.py vs numpy run "
          f"{ref.rel_max(ref.restore(**k), img[0]):.3e}; min / max |thishat| {min(hats):.1e}")
    out["cites"] = np.array(cites)
    return out


def compute():
    """every array of ``restore_pins.npz``, by name"""
    from tests import _restore_ref as ref

    ns, cites = reference()
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


def same(path, out):
    """whether the file at ``path`` holds exactly ``out`` (a fixture that would not change is not written again: the
    archive's time stamps would change its bytes)"""
    if not os.path.exists(path):
        return False
    old = np.load(path)
    return sorted(old.files) == sorted(out) and all(np.array_equal(old[k], np.asarray(out[k])) for k in old.files)


def main():
    for name, out in (("restore_pins.npz", compute()), ("restore_edge_pins.npz", compute_edge())):
        path = os.path.join(HERE, name)
        if same(path, out):
            print(name, "unchanged")
        else:
            np.savez_compressed(path, **out)
        print("\n".join(out["cites"]))
        print(name, os.path.getsize(path))
        assert os.path.getsize(path) < 500_000


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("make_restore_pins.py needs the reference checkout (build container only); the committed .npz travels instead")
    main()
