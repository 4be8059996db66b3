"""numpy restatement of the two primary-beam operations of csrc/beam.hip (no scipy: the fixtures of
tests/golden/beam_pins.npz carry scipy's answers).

regrid       utils/beam.py:75-89 of the reference (eval_beam: RegularGridInterpolator, linear, fill_value 1.0)
rotate_mean  utils/stokes2vis_msv4.py:399-409 (mean of ndimage.rotate(beam0, angle, reshape=False, mode="nearest")),
             restated as edge pad by 12 -> cubic B-spline prefilter (reflect initialisation) -> 4x4 B-spline
             evaluation at the rotated coordinates.

The rule for samples outside the padded array (found against scipy's map_coordinates): the
COORDINATE is NOT clamped -- the four B-spline weights come from its own fractional part and the support starts at
floor(x) - 1 -- and each of the four SUPPORT INDICES is clamped to [0, N - 1].  Far outside, all four indices fall on
the edge sample and the value is that coefficient.  Clamping the coordinate as well is what differs at the 1e-10 level.
"""

import numpy as np

PAD = 12
POLE = np.sqrt(3.0) - 2.0


def locate(nodes, x):
    """scipy's find_indices: i with nodes[i] <= x < nodes[i + 1], clipped to [0, n - 2]; t; and the out-of-bounds mask."""
    nodes = np.asarray(nodes, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    i = np.clip(np.searchsorted(nodes, x, side="right") - 1, 0, nodes.size - 2)
    t = (x - nodes[i]) / (nodes[i + 1] - nodes[i])
    outside = (x < nodes[0]) | (x > nodes[-1])
    return i, t, outside


def regrid(beam, l_in, m_in, l_out, m_out):
    """``eval_beam`` on a ``(nl, nm)`` beam or a ``(ncorr, nl, nm)`` stack; ``l_out`` 1-D (separable) or 2-D."""
    beam = np.asarray(beam, dtype=np.float64)
    l_out, m_out = np.asarray(l_out, dtype=np.float64), np.asarray(m_out, dtype=np.float64)
    if l_out.ndim == 1:
        ll, mm = np.meshgrid(l_out, m_out, indexing="ij")
    elif l_out.ndim == 2:
        ll, mm = l_out, m_out
    else:
        raise ValueError("Only 1 or 2D coordinates supported for beam evaluation")
    if beam.ndim == 3:
        return np.stack([regrid(b, l_in, m_in, ll, mm) for b in beam])
    if (beam == 1.0).all():
        return np.ones_like(ll)
    i, tx, ox = locate(l_in, ll)
    j, ty, oy = locate(m_in, mm)
    lo = (1.0 - ty) * beam[i, j] + ty * beam[i, j + 1]
    hi = (1.0 - ty) * beam[i + 1, j] + ty * beam[i + 1, j + 1]
    out = (1.0 - tx) * lo + tx * hi
    out[ox | oy] = 1.0
    return out


def prefilter_axis0(c):
    """Cubic B-spline prefilter along axis 0 with scipy's reflect initialisation (spline_filter1d, mode "nearest")."""
    z = POLE
    c = np.array(c, dtype=np.float64) * ((1.0 - z) * (1.0 - 1.0 / z))
    n = c.shape[0]
    zn = z**n
    acc = np.zeros_like(c[0])
    for i in range(n):
        acc = acc + z**i * (c[i] + zn * c[n - 1 - i])
    c[0] = c[0] + z / (1.0 - zn * zn) * acc
    for i in range(1, n):
        c[i] = c[i] + z * c[i - 1]
    c[n - 1] = c[n - 1] * (z / (z - 1.0))
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def coefficients(beam0):
    """B-spline coefficients of the edge-padded beam, shape ``(n0 + 24, n1 + 24)``."""
    p = np.pad(np.asarray(beam0, dtype=np.float64), PAD, mode="edge")
    p = prefilter_axis0(p)
    return np.ascontiguousarray(prefilter_axis0(p.T).T)


def cos_sin_deg(angles):
    """cos and sin of angles in degrees, exact at the multiples of 90 (as scipy.special.cosdg / sindg are)."""
    a = np.mod(np.asarray(angles, dtype=np.float64), 360.0)
    c, s = np.cos(np.deg2rad(a)), np.sin(np.deg2rad(a))
    for q, (cq, sq) in enumerate(((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))):
        hit = a == 90.0 * q
        c[hit], s[hit] = cq, sq
    return c, s


def _weights(x):
    y = x - np.floor(x)
    z = 1.0 - y
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    return w0, w1, w2, 1.0 - w0 - w1 - w2


def sample_coordinates(shape, angles):
    """Unclamped padded-array coordinates ``ii, jj (nangle, n0, n1)`` of every sample."""
    n0, n1 = shape
    c0, c1 = (n0 - 1) / 2.0, (n1 - 1) / 2.0
    c, s = cos_sin_deg(angles)
    i, j = np.meshgrid(np.arange(n0, dtype=np.float64), np.arange(n1, dtype=np.float64), indexing="ij")
    c, s = c[:, None, None], s[:, None, None]
    ii = c * (i - c0) + s * (j - c1) + c0 + PAD
    jj = -s * (i - c0) + c * (j - c1) + c1 + PAD
    return ii, jj


def inside_mask(shape, angles):
    """Pixels all of whose sample positions lie inside the padded array."""
    ii, jj = sample_coordinates(shape, angles)
    big0, big1 = shape[0] + 2 * PAD, shape[1] + 2 * PAD
    return ((ii >= 0) & (ii <= big0 - 1) & (jj >= 0) & (jj <= big1 - 1)).all(axis=0)


def rotate_mean(beam0, angles=None):
    """Mean over ``angles`` (degrees) of the cubic-spline rotations of ``beam0 (n0, n1)`` or a ``(ncorr, n0, n1)`` stack."""
    angles = np.linspace(0, 359, 25) if angles is None else np.atleast_1d(np.asarray(angles, dtype=np.float64))
    beam0 = np.asarray(beam0, dtype=np.float64)
    if beam0.ndim == 3:
        return np.stack([rotate_mean(b, angles) for b in beam0])
    coef = coefficients(beam0)
    big0, big1 = coef.shape
    ii, jj = sample_coordinates(beam0.shape, angles)
    acc = np.zeros(beam0.shape)
    for a in range(angles.size):
        x, y = ii[a], jj[a]
        wx, wy = _weights(x), _weights(y)
        sx, sy = np.floor(x).astype(np.int64) - 1, np.floor(y).astype(np.int64) - 1
        val = np.zeros(beam0.shape)
        for p in range(4):
            row = np.zeros(beam0.shape)
            ip = np.clip(sx + p, 0, big0 - 1)
            for q in range(4):
                row = row + wy[q] * coef[ip, np.clip(sy + q, 0, big1 - 1)]
            val = val + wx[p] * row
        acc = acc + val
    return acc / angles.size
