"""Worker of tests/test_gpu_psffft.py::test_admission_neighbours: PSF plans at the padded sizes next to the row-FFT family that
must take the rocFFT fallback (the doubled row-FFT lengths, sizes below 1024, good_size-padded ones, and on x the radix-3/7/15
leads above 10240), on each axis with the other at 1024.  Each plan reports uses_rowfft and, where it falls back, is compared
with numpy (rel L2 and max|err| / max|ref|).  One JSON line per plan on stdout.

It runs in a process of its own, which launches no kernel of the row-FFT pipeline: rocFFT compiles and loads a module for each
kernel of these plans and unloads it when the plan is destroyed (some 270 loads and unloads for these sizes), and a row-FFT kernel
whose code object was first loaded after that sequence, in the same process, was once stopped with an illegal-instruction
error (see the test's docstring)."""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pfb_imaging_amd import _lib  # noqa: E402
from pfb_imaging_amd.fft import good_size  # noqa: E402
from pfb_imaging_amd.psfconv import PsfConv  # noqa: E402


def main():
    _lib.require_gpu()
    os.environ.pop("PFBHIP_PSF_ROWFFT", None)
    sizes = [int(s) for s in sys.argv[1].split(",")]
    rng = np.random.default_rng(7)
    for axis in ("x", "y"):
        for n in sizes + [good_size(2 * 1100)]:
            nxp, nyp = (n, 1024) if axis == "x" else (1024, n)
            nx, ny = min(nxp, 77), min(nyp, 91)
            pc = PsfConv(nx, ny, nxp, nyp)
            rec = {"axis": axis, "n": n, "nxp": nxp, "nyp": nyp, "uses_rowfft": pc.uses_rowfft}
            if not pc.uses_rowfft:
                ph = 1.0 + rng.random((nxp, nyp // 2 + 1))
                neg = (-np.arange(nxp)) % nxp
                for c in (0, nyp // 2):  # the precondition: edge columns even in kx
                    ph[:, c] = 0.5 * (ph[:, c] + ph[neg, c])
                x = rng.standard_normal((nx, ny))
                pc.set_psfhat(0, ph)
                got = pc.apply(x, 0)
                xp = np.zeros((nxp, nyp))
                xp[:nx, :ny] = x
                want = np.fft.irfft2(np.fft.rfft2(xp) * ph, s=(nxp, nyp))[:nx, :ny]
                err = got - want
                rec["rel"] = float(np.linalg.norm(err) / np.linalg.norm(want))
                rec["max"] = float(np.abs(err).max() / np.abs(want).max())
            pc.close()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
