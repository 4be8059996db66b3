"""Host references for the device-resident visibility chunk (tests/test_gpu_vischunk.py, tests/test_vischunk_cpu.py).

``l2_reweight`` restates, in numpy, lines 509-532 of the reference's ``operators/gridder.py`` (the l2 reweighting inside
``image_data_products``).  It is a restatement, written from reading those lines; no source text is stored here.  The
block cannot be taken out of the reference and run the way ``make_ref_pins.take`` takes whole functions: it sits in the
middle of a function that reads and writes zarr datasets, and it uses that function's locals.  Line by line:

    :516      ressq = (residual_vis * wgtp * residual_vis.conj()).real
    :519      ssq = ressq[:, mask > 0].sum(axis=-1)          (per correlation)
    :520      ovar = ssq / mask.sum()                         (one mask for every correlation)
    :521      "if ovar": proceed only with a non-zero variance
    :527      denom = dof + ressq / ovar[:, None, None]
    :530      wgt *= (dof + 2) / denom                        (every sample, masked ones included)
    :531-532  else: no weights (here: ValueError, as image_data_products_arrays raises it)
"""

import numpy as np


def l2_reweight(residual_vis, wgt, mask, dof, wgtp=1.0):
    """``(new weights, ovar)`` for ``residual_vis, wgt (ncorr, nrow, nchan)``, ``mask (nrow, nchan)`` and ``wgtp`` a scalar or an
    array that broadcasts against them; ``wgt`` is not modified."""
    ressq = (residual_vis * wgtp * residual_vis.conj()).real
    ssq = ressq[:, mask > 0].sum(axis=-1)
    ovar = ssq / mask.sum()
    if not np.all(ovar):
        raise ValueError("l2 reweighting: zero residual variance")
    denom = dof + ressq / ovar[:, None, None]
    return wgt * ((dof + 2) / denom), ovar


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)
