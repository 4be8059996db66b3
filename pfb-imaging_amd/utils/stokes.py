"""Stokes conventions: which products a data set can give, and the coherency <-> Stokes maps on host arrays.

``stokes_products`` answers what ``stokes_expr_funcs`` of the reference answers (utils/stokes.py:89-155) with the names of
the products instead of generated functions: the device kernel (csrc/stokes.hip) takes the matrix ``T`` below, not
expressions.  ``corr_to_stokes`` / ``stokes_to_corr`` keep the reference's signatures (utils/stokes.py:48-77).
"""

import numpy as np

STOKES = "IQUV"

# coherency from Stokes, rows = correlations (00, 01, 10, 11), columns = I, Q, U, V (utils/stokes.py:33, :35)
T_LINEAR = np.array([[1, 1, 0, 0], [0, 0, 1, 1j], [0, 0, 1, -1j], [1, -1, 0, 0]], dtype=np.complex128)
T_CIRCULAR = np.array([[1, 0, 0, 1], [0, 1, 1j, 0], [0, 1, -1j, 0], [1, 0, 0, -1]], dtype=np.complex128)

# what the parallel hands alone give
_TWO_CORR = {"linear": "IQ", "circular": "IV"}


def coherency_matrix(pol):
    """``T`` with ``vec(V) = T (I, Q, U, V)`` for ``pol`` in ("linear", "circular"); ``inv(T) = T^H / 2``."""
    if pol == "linear":
        return T_LINEAR
    if pol == "circular":
        return T_CIRCULAR
    raise ValueError(f"Unknown polarisation type {pol}")


def stokes_products(product, pol, nc, wgt_mode, jones_ndim):
    """The products ``weight_data`` computes for these arguments, as a tuple of letters in the order I, Q, U, V whatever
    the order in ``product``; or the reference's refusal, checked in the reference's order.

    ``nc`` is the number of correlations as a string.  ``wgt_mode="minvar"`` is a valid mode that this package cannot
    serve: ``NotImplementedError`` for either Jones form."""
    coherency_matrix(pol)
    if nc not in ("1", "2", "4"):
        raise ValueError(f"Unsupported number of correlations {nc}")
    if wgt_mode not in ("l2", "minvar"):
        raise ValueError(f"Unknown weighting mode {wgt_mode}")
    chosen = tuple(s for s in STOKES if s in product)
    for s in chosen:
        if nc == "2" and s not in _TWO_CORR[pol]:
            raise ValueError(f"{s} is not available in {pol} polarisation with 2 correlations")
    unknown = product.strip(STOKES)
    if unknown:
        raise ValueError(f"Unknown polarisation product {unknown}")
    if jones_ndim == 6:
        if wgt_mode == "minvar":
            raise NotImplementedError("Minvar weighting not yet implemented for full-Stokes")
        if nc != "4":
            raise ValueError("Full 2x2 jones mode requires 4 correlation data")
    elif jones_ndim == 5:
        if nc == "1":
            raise ValueError(f"Selected product is only available from 2 or 4 correlation data while you have ncorr={nc}.")
        if wgt_mode == "minvar":
            raise NotImplementedError("minvar weighting is not available: its weight expressions are generated code that "
                                      "could not be read on the build machine (DESIGN.md section 16); use wgt_mode='l2'")
    else:
        raise ValueError("Jones term has incorrect number of dimensions")
    return chosen


def _four(x, axis, poltype):
    if poltype.lower() != "linear":
        raise NotImplementedError("Only linear polarisation is implemented")
    x = np.asarray(x)
    if x.shape[axis] != 4:
        raise ValueError(f"Expected 4 polarisation products, got {x.shape[axis]}")
    return tuple(np.take(x, k, axis=axis) for k in range(4))


def corr_to_stokes(x, wsum=1.0, axis=0, poltype="linear"):
    """Real Stokes images ``[I, Q, U, V]`` from the four correlation images ``[I+Q, U+iV, U-iV, I-Q]`` along ``axis``, each
    divided by ``wsum``.  The sums are not halved, as in the reference."""
    xx, xy, yx, yy = _four(x, axis, poltype)
    return np.stack(((xx + yy).real / wsum, (xx - yy).real / wsum, (xy + yx).real / wsum, (xy - yx).imag / wsum), axis=axis)


def stokes_to_corr(x, axis=0, poltype="linear"):
    """The four correlations ``[I+Q, U+iV, U-iV, I-Q]`` of ``[I, Q, U, V]`` along ``axis``."""
    i, q, u, v = _four(x, axis, poltype)
    return np.stack((i + q, u + 1j * v, u - 1j * v, i - q), axis=axis)
