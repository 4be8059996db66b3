"""The restore step of an imaging run on arrays: model and residual brought to one Gaussian resolution and added."""

import numpy as np

from ..gaussconv import cached_plan

RESTORE_PFRAC = 0.2  # the padding restore_image asks convolve2gaussres for


def restore_arrays(model, residual, wsum, gausspari, gaussparf, nthreads=1):
    """``(image, gaussparf)`` with ``image = conv(model; gaussparf) + rconv``: the arithmetic of the reference's
    ``restore_image`` (/root/reference/src/pfb_imaging/utils/restoration.py:48-88) without its dataset reading and writing.

    ``model`` and ``residual`` are (nband, nx, ny); ``residual`` is divided by ``wsum`` (nband) first.  ``gausspari`` (nband, 3)
    is the intrinsic resolution of each band (``PSFPARSN``: pixels, pixels, radians), ``gaussparf`` the final one, a single
    triple (tiled over the bands) or one per band.  ``rconv`` is the residual convolved with the ratio of the two Gaussians;
    a band whose two resolutions are ``np.allclose`` keeps its residual as it is.  Model and residual each go through the
    device once and the sum is formed in the pass that crops the model's convolution.  ``nthreads`` is accepted and unused."""
    model = np.asarray(model)
    nband = model.shape[0]
    gaussparf = np.array(gaussparf, dtype=np.float64)
    if gaussparf.ndim == 1:
        gaussparf = np.tile(gaussparf, (nband, 1))
    if gaussparf.shape != (nband, 3):
        raise ValueError(f"gaussparf should have shape ({nband}, 3), not {gaussparf.shape}")
    gausspari = np.asarray(gausspari, dtype=np.float64)
    if gausspari.shape != (nband, 3):
        raise ValueError(f"gausspari should have shape ({nband}, 3), not {gausspari.shape}")
    plan = cached_plan(nband, model.shape[1], model.shape[2], RESTORE_PFRAC)
    return plan.restore(model, residual, wsum, gausspari, gaussparf), gaussparf
