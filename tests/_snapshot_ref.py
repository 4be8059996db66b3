"""numpy restatement of the array work of the reference's ``stokes_image`` (src/pfb_imaging/utils/stokes2im.py), written from
reading lines 364-373, 462-486, 606-625, 631-692, 707-708 and 731-737; no source text is stored here.  The block cannot be run
as it stands: it sits in the middle of a function that reads zarr datasets, calls casacore and ducc0.

Arrays are correlation-first here, ``(ncorr, nrow, nchan)``, the chunk's layout (the reference holds ``(nrow, nchan, ncorr)``
until :561).  Two oddities of the reference are not restated (pfb_imaging_amd/utils/stokes2im.py names them): the mask is
broadcast over the correlations, ``mask[:, :, None]`` there and ``mask[None]`` here, and every Stokes is normalised once.
Gridding goes through the direct DFT (oracle/dft.py) with ``divide_by_n=True`` and the shifted centre; every phase is formed in
long double and reduced to a fraction of a turn before it meets pi, as tests/_dft_ref.py does, so the restatement carries no
error worth counting against the device's bounds.
"""

import numpy as np

from oracle import dft

C0 = 299792458.0
FLIP_U, FLIP_V, FLIP_W = False, True, False  # wgridder_conventions(0, 0), :347


def good_size(n):
    """The smallest 2-3-5-7-11-smooth integer >= n (ducc0.fft.good_size)"""
    n = max(int(n), 1)
    while True:
        m = n
        for p in (2, 3, 5, 7, 11):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def pad_size(n, min_padding):
    """:567-569"""
    npad = good_size(int(min_padding * n))
    while npad % 2:
        npad = good_size(npad + 1)
    return npad


def psf_size(nx, ny, psf_relative_size, psf_min_size=128):
    """:606-619"""
    if psf_relative_size is None:
        return psf_min_size, psf_min_size
    nx_psf = good_size(int(nx * psf_relative_size))
    while nx_psf % 2:
        nx_psf = good_size(nx_psf + 1)
    ny_psf = good_size(int(ny * psf_relative_size))
    while ny_psf % 2:
        ny_psf = good_size(ny_psf + 1)
    if nx_psf < psf_min_size or ny_psf < psf_min_size:
        nx_psf = ny_psf = psf_min_size
    return nx_psf, ny_psf


def _cis_turns(turns):
    """exp(-2 pi i turns) for long-double turns"""
    frac = (turns - np.rint(turns)).astype(np.float64)
    return np.exp(-2j * np.pi * frac)


def rephase_phasor(freq, w_diff):
    """exp(freqfactor * w_diff) of :354, :371: (nrow, nchan)"""
    ld = np.longdouble
    return _cis_turns(np.asarray(w_diff, dtype=np.float64).reshape(-1).astype(ld)[:, None] * (freq.astype(ld) / ld(C0))[None, :])


def rephase_residual(data, mask, freq, w_diff=None, model=None):
    """:371-373 and :467-468: ``(data p - model p) * mask``; the mask only with a model"""
    p = 1.0 if w_diff is None else rephase_phasor(freq, w_diff)[None]
    data = data * p
    if model is not None:
        data = (data - model * p) * mask[None]
    return data


def l2_reweight_joint(data, mask, dof):
    """:472-479: ``(weight, ovar)``"""
    ressq = (data * data.conj()).real * mask[None]
    wcount = mask.sum()
    if not wcount:
        raise ValueError("empty mask")
    ovar = ressq.sum() / wcount
    if not ovar > 0:
        raise ValueError("Residual visibilities are exactly zero. Cannot compute L2 reweighting.")
    return (dof + 1) / (dof + ressq / ovar) / ovar, ovar


def psf_vis(uvw, freq, x0, y0):
    """:483-486 (signu * signx == signv * signy == 1)"""
    ld = np.longdouble
    n = np.sqrt(ld(1) - ld(x0) ** 2 - ld(y0) ** 2)
    delay = uvw[:, 0].astype(ld) * ld(x0) + uvw[:, 1].astype(ld) * ld(y0) - uvw[:, 2].astype(ld) * (n - 1)
    return _cis_turns(delay[:, None] * (freq.astype(ld) / ld(C0))[None, :])


def std(x):
    """np.std of :692 in long double, two-pass"""
    x = np.asarray(x).astype(np.longdouble)
    return float(np.sqrt(((x - x.mean()) ** 2).mean()))


def image(uvw, freq, data, weight, mask, nx, ny, cell_rad, x0=0.0, y0=0.0, psf_relative_size=None, pbeam=None, eta=1e-5):
    """:606-692, :707-708, :731-737 on ``data, weight (ns, nrow, nchan)``: ``dict(cube, psf, weight, rms, beam_weight, residual64,
    psf64)`` -- ``cube / psf / beam_weight`` float32 and transposed as the reference stores them, ``residual64 / psf64`` the
    float64 planes ``(ns, nx, ny)`` before the cast."""
    ns = weight.shape[0]
    nx_psf, ny_psf = psf_size(nx, ny, psf_relative_size)
    pv = psf_vis(uvw, freq, x0, y0)
    wsum = np.zeros(ns)
    residual, psf, rms = np.zeros((ns, nx, ny)), np.zeros((ns, nx_psf, ny_psf)), np.zeros(ns)
    conv = (x0, y0, FLIP_U, FLIP_V, FLIP_W, True, True)
    for c in range(ns):
        wsum[c] = weight[c, mask != 0].sum()
        if wsum[c] == 0:
            continue
        residual[c] = dft.dft_vis2dirty(uvw, freq, data[c], weight[c], mask, nx, ny, cell_rad, cell_rad, *conv)
        psf[c] = dft.dft_vis2dirty(uvw, freq, pv, weight[c], mask, nx_psf, ny_psf, cell_rad, cell_rad, *conv)
    for c in range(ns):  # (once, not once per gridded Stokes)
        if wsum[c] > 0:
            psf_max = psf[c].max()
            wsum[c] = psf_max
            psf[c] /= psf_max
            residual[c] /= psf_max
            rms[c] = std(residual[c])
    out = dict(psf64=psf.copy(), weight=wsum, rms=rms)
    if pbeam is not None:
        residual = residual * (pbeam / (pbeam**2 + eta))
        out["beam_weight"] = np.transpose((pbeam**2 + eta).astype(np.float32), axes=(0, 2, 1))
    out["residual64"] = residual
    out["cube"] = np.transpose(residual.astype(np.float32), axes=(0, 2, 1))
    out["psf"] = np.transpose(psf.astype(np.float32), axes=(0, 2, 1))
    return out


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)
