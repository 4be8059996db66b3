"""numpy oracle of ``weight_data`` (pfb_imaging_amd.utils.weighting, csrc/stokes.hip): complex128, vectorised over samples,
in the closed form of DESIGN.md section 16:

    s   = Tinv vec(Jp^-1 V Jq^-H)            Tinv = T^H / 2
    W_s = sum_c w_c |A_cs|^2                 A = (Jp (x) conj(Jq)) T

The inverses are written out as adjugates over determinants (``stokes_of_samples``); ``via_inverses`` evaluates the same
statement through ``numpy.linalg.inv`` and a 4x4 matrix product, ``normal_equations`` solves the weighted least-squares
problem, and ``diagonal_formulas`` is the written-out diagonal case.  The three serve tests/test_stokes_cpu.py only.
"""

import functools

import numpy as np

T = {
    "linear": np.array([[1, 1, 0, 0], [0, 0, 1, 1j], [0, 0, 1, -1j], [1, -1, 0, 0]], dtype=np.complex128),
    "circular": np.array([[1, 0, 0, 1], [0, 1, 1j, 0], [0, 1, -1j, 0], [1, 0, 0, -1]], dtype=np.complex128),
}
STOKES = "IQUV"


def full_of_diag(j):
    """(..., 2) diagonal Jones terms as (..., 2, 2) matrices"""
    out = np.zeros(j.shape + (2,), dtype=np.complex128)
    out[..., 0, 0], out[..., 1, 1] = j[..., 0], j[..., 1]
    return out


def widen(v, w):
    """two correlations as four: (v0, 0, 0, v1) with weights (w0, 1, 1, w1)"""
    if v.shape[-1] == 4:
        return v.astype(np.complex128), w.astype(np.float64)
    v4, w4 = np.zeros(v.shape[:-1] + (4,), dtype=np.complex128), np.ones(w.shape[:-1] + (4,), dtype=np.float64)
    v4[..., 0], v4[..., 3], w4[..., 0], w4[..., 3] = v[..., 0], v[..., 1], w[..., 0], w[..., 1]
    return v4, w4


def stokes_of_samples(v, w, jp, jq, pol, diag):
    """All four Stokes visibilities ``(n, 4)`` and weights ``(n, 4)`` of ``n`` samples: ``v, w (n, 4)``, ``jp, jq (n, 2, 2)``.
    ``diag`` takes the plain quotients a diagonal Jones allows; sums run in index order."""
    t = T[pol]
    tinv = t.conj().T / 2
    cq = jq.conj()
    if diag:
        g = np.stack([jp[:, 0, 0] * cq[:, 0, 0], jp[:, 0, 0] * cq[:, 1, 1], jp[:, 1, 1] * cq[:, 0, 0], jp[:, 1, 1] * cq[:, 1, 1]], axis=1)
        x = v / g
    else:
        p00, p01, p10, p11 = jp[:, 0, 0], jp[:, 0, 1], jp[:, 1, 0], jp[:, 1, 1]
        c00, c01, c10, c11 = cq[:, 0, 0], cq[:, 0, 1], cq[:, 1, 0], cq[:, 1, 1]
        y00, y01 = p11 * v[:, 0] - p01 * v[:, 2], p11 * v[:, 1] - p01 * v[:, 3]
        y10, y11 = p00 * v[:, 2] - p10 * v[:, 0], p00 * v[:, 3] - p10 * v[:, 1]
        z = np.stack([y00 * c11 - y01 * c01, y01 * c00 - y00 * c10, y10 * c11 - y11 * c01, y11 * c00 - y10 * c10], axis=1)
        det = (p00 * p11 - p01 * p10) * (c00 * c11 - c01 * c10)
        x = z / det[:, None]
    s = np.zeros((v.shape[0], 4), dtype=np.complex128)
    wout = np.zeros((v.shape[0], 4), dtype=np.float64)
    for k in range(4):
        for c in range(4):
            s[:, k] += tinv[k, c] * x[:, c]
    for c in range(4):
        i, j = c >> 1, c & 1
        m = [jp[:, i, 0] * cq[:, j, 0], jp[:, i, 0] * cq[:, j, 1], jp[:, i, 1] * cq[:, j, 0], jp[:, i, 1] * cq[:, j, 1]]
        for k in range(4):
            a = np.zeros(v.shape[0], dtype=np.complex128)
            for ell in range(4):
                a += m[ell] * t[ell, k]
            wout[:, k] += w[:, c] * (a.real**2 + a.imag**2)
    return s, wout


def mueller(jp, jq):
    """Jp (x) conj(Jq), (n, 4, 4)"""
    return np.einsum("nik,njl->nijkl", jp, jq.conj()).reshape(-1, 4, 4)


def via_inverses(v, w, jp, jq, pol):
    """The same statement through numpy.linalg.inv and matrix products"""
    x = np.linalg.inv(jp) @ v.reshape(-1, 2, 2) @ np.linalg.inv(jq).conj().transpose(0, 2, 1)
    s = np.einsum("kc,nc->nk", np.linalg.inv(T[pol]), x.reshape(-1, 4))
    a = mueller(jp, jq) @ T[pol]
    return s, np.einsum("nc,ncs->ns", w, np.abs(a) ** 2)


def normal_equations(v, w, jp, jq, pol):
    """argmin_s (v - A s)^H diag(w) (v - A s) and diag(A^H diag(w) A)"""
    a = mueller(jp, jq) @ T[pol]
    ah = a.conj().transpose(0, 2, 1) * w[:, None, :]
    lhs = ah @ a
    s = np.linalg.solve(lhs, (ah @ v[:, :, None]))[:, :, 0]
    return s, np.einsum("nss->ns", lhs).real


def diagonal_formulas(v, w, jp, jq):
    """The written-out diagonal case, linear feeds: jp, jq (n, 2)"""
    a, b = jp[:, 0] * jq[:, 0].conj(), jp[:, 0] * jq[:, 1].conj()
    c, d = jp[:, 1] * jq[:, 0].conj(), jp[:, 1] * jq[:, 1].conj()
    s = np.stack([(v[:, 0] / a + v[:, 3] / d) / 2, (v[:, 0] / a - v[:, 3] / d) / 2, (v[:, 1] / b + v[:, 2] / c) / 2,
                  (v[:, 1] / b - v[:, 2] / c) / 2j], axis=1)
    wi = w[:, 0] * np.abs(a) ** 2 + w[:, 3] * np.abs(d) ** 2
    wu = w[:, 1] * np.abs(b) ** 2 + w[:, 2] * np.abs(c) ** 2
    return s, np.stack([wi, wi, wu, wu], axis=1)


def sample_scales(s, w):
    """What a sample's errors are measured against: the norm of its four Stokes visibilities (= |vec(X)| / sqrt(2): every
    product is a sum over the corrected coherencies, and rounds at their size, however small it is itself) and its largest
    Stokes weight."""
    return np.sqrt((np.abs(s) ** 2).sum(axis=1)), w.max(axis=1)


def rel_diff(s, w, s_ref, w_ref):
    """Largest difference of (s, w) from (s_ref, w_ref) relative to the reference sample's scales"""
    vs, ws = sample_scales(s_ref, w_ref)
    return max((np.abs(s - s_ref) / vs[:, None]).max(), (np.abs(w - w_ref) / ws[:, None]).max())


def random_jones(rng, shape, full):
    """Invertible Jones terms: diagonal amplitudes in [0.5, 2] with random phases, off-diagonals of scale 0.2"""
    diag = rng.uniform(0.5, 2.0, shape + (2,)) * np.exp(2j * np.pi * rng.uniform(size=shape + (2,)))
    if not full:
        return diag
    j = full_of_diag(diag)
    off = 0.2 * (rng.standard_normal(shape + (2,)) + 1j * rng.standard_normal(shape + (2,)))
    j[..., 0, 1], j[..., 1, 0] = off[..., 0], off[..., 1]
    return j


def row_to_bin(tbin_idx, tbin_counts, nrow):
    out = np.full(nrow, -1, dtype=np.int64)
    start = np.asarray(tbin_idx) - np.min(tbin_idx) if len(tbin_idx) else np.zeros(0, dtype=np.int64)
    for t, (r0, n) in enumerate(zip(start, tbin_counts)):
        out[r0:r0 + n] = t
    return out


def weight_data(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, full_stokes=False):
    """``(vis, wgt)`` as the device entry returns them, ``(nrow, nchan, ns)`` complex128 / float64, products in the order
    I, Q, U, V; with ``full_stokes`` also the per-sample scales ``(vscale, wscale)`` of shape ``(nrow, nchan)``."""
    data, weight, flag, jones = np.asarray(data), np.asarray(weight), np.asarray(flag), np.asarray(jones)
    nrow, nchan, _ = data.shape
    diag = jones.ndim == 5
    jm = full_of_diag(jones[:, :, :, 0]) if diag else jones[:, :, :, 0].astype(np.complex128)
    bins = row_to_bin(tbin_idx, tbin_counts, nrow)
    live = (bins >= 0)[:, None] & ~(flag != 0).any(axis=-1)
    r, c = np.nonzero(live)
    v, w = widen(data[r, c], weight[r, c])
    jp, jq = jm[bins[r], np.asarray(ant1)[r], c], jm[bins[r], np.asarray(ant2)[r], c]
    s, ws = stokes_of_samples(v, w, jp, jq, pol, diag)
    sel = [STOKES.index(k) for k in STOKES if k in product]
    vis = np.zeros((nrow, nchan, len(sel)), dtype=np.complex128)
    wgt = np.zeros((nrow, nchan, len(sel)), dtype=np.float64)
    vis[r, c], wgt[r, c] = s[:, sel], ws[:, sel]
    if not full_stokes:
        return vis, wgt
    vscale, wscale = np.ones((nrow, nchan)), np.ones((nrow, nchan))
    vscale[r, c], wscale[r, c] = sample_scales(s, ws)
    return vis, wgt, vscale, wscale


@functools.lru_cache(maxsize=None)
def rounding_scale():
    """``d``: the largest relative difference (``rel_diff``) between the oracle through explicit adjugates and through matrix
    inverses, over 80 000 random samples with full Jones terms and both feed types.  The device evaluates the same algebra
    in a third order; its tolerance is a multiple of ``d``."""
    rng = np.random.default_rng(20261020)
    n = 40000
    d = 0.0
    for pol in ("linear", "circular"):
        v = rng.standard_normal((n, 4)) + 1j * rng.standard_normal((n, 4))
        w = rng.uniform(0.1, 2.0, (n, 4))
        jp, jq = random_jones(rng, (n,), True), random_jones(rng, (n,), True)
        s, ws = stokes_of_samples(v, w, jp, jq, pol, False)
        s2, ws2 = via_inverses(v, w, jp, jq, pol)
        d = max(d, rel_diff(s2, ws2, s, ws))
    return d
