"""Cases and a plain reference for the imaging-weight chain (csrc/weighting.hip, utils/weighting.py, VisChunk.imaging_weights).

No ctypes and no device code: tests/test_weighting_edges_cpu.py holds the oracle's C loops against this module,
tests/test_gpu_weighting_edges.py the device.

The chain (utils/weighting.py:81-254 of the reference): counts of the weights on the (nx, ny) uv-grid -> positive counts below
``median(positive) / level`` raised to it -> (2 s + 1)^2 box sum with zero padding -> Briggs scaling
``counts * (5 * 10^-R)^2 sum(c) / sum(c^2) + 1`` when ``R > -2`` -> ``weight /= counts[cell]`` where ``counts > 0``.

The restatement (:func:`reference`) takes the cell index with numpy's ``floor`` from the reference's expressions in the
reference's order, and does everything after it in ``np.longdouble``; each stage is handed back rounded to float64.

EXACT cases.  Grid 8 x 16 with ``cell_x = 2^-10``, ``cell_y = 2^-11``: ``u_cell = v_cell = 128``, ``umax = 512``, ``vmax =
1024``.  ``freq = c * (1, 1.25, 1.5, 1.75, 2)``, so ``freq / c`` is exact; ``u, v`` are integer multiples of 32 (a quarter
cell), so every product, sum and quotient of the index map is exact and many samples sit exactly on a cell boundary, on
``ug == nx``, ``ug == 0``, ``v == +-0`` and ``vg == ny``.  Weights are integer multiples of 2^-10 below 64, so every sum of
them is exact in float64 in any order, and the filter level is a power of two, so ``median / level`` is exact as well.
With ``R <= -2`` the final weights are one correctly rounded division of exact operands: exact cases are compared with
``np.array_equal``.  Everything else is compared within :func:`bounds`.
"""

from functools import lru_cache

import numpy as np

LIGHTSPEED = 299792458.0
U = 2.0 ** -53
LD = np.longdouble
DEFAULT_SIGNS = ((1.0, -1.0), (-1.0, 1.0))  # utils/weighting.py's defaults and the gridder callers' (flip_v)


# ---- the restatement -----------------------------------------------------------------------------------------------------

def geometry(nx, ny, cell_x, cell_y):
    """``u_cell, umax, v_cell, vmax`` (weighting.py:84-92)"""
    return 1 / (nx * cell_x), np.abs(1 / cell_x / 2), 1 / (ny * cell_y), np.abs(1 / cell_y / 2)


def grid_coords(uvw, freq, nx, ny, cell_x, cell_y, usign, vsign):
    """``(v_tmp before the fold, ug, vg)`` per sample, ``(nrow, nchan)`` each: weighting.py:115-123, same order of operations"""
    u_cell, umax, v_cell, vmax = geometry(nx, ny, cell_x, cell_y)
    nf = np.asarray(freq, dtype=np.float64) / LIGHTSPEED
    u = uvw[:, 0, None] * nf[None, :] * usign
    v0 = uvw[:, 1, None] * nf[None, :] * vsign
    neg = v0 < 0
    u = np.where(neg, -u, u)
    v = np.where(neg, -v0, v0)
    return v0, (u + umax) / u_cell, (v + vmax) / v_cell


def ref_index(uvw, freq, mask, nx, ny, cell_x, cell_y, usign, vsign):
    """Flat cell ``u_idx * ny + v_idx``, -1 where masked or out of range (weighting.py:112-135)"""
    _, ug, vg = grid_coords(uvw, freq, nx, ny, cell_x, cell_y, usign, vsign)
    fu, fv = np.floor(ug), np.floor(vg)
    ok = (np.asarray(mask) != 0) & (fu >= 0) & (fu < nx) & (fv >= 0) & (fv < ny)
    cell = np.full(ug.shape, -1, dtype=np.int64)
    cell[ok] = fu[ok].astype(np.int64) * ny + fv[ok].astype(np.int64)
    return cell


def ref_counts(cell, wgt, nx, ny):
    """longdouble ``(ncorr, nx, ny)``"""
    ncorr = wgt.shape[0]
    counts = np.zeros((ncorr, nx * ny), dtype=LD)
    ok = cell >= 0
    for k in range(ncorr):
        np.add.at(counts[k], cell[ok], wgt[k][ok].astype(LD))
    return counts.reshape(ncorr, nx, ny)


def ref_filter(counts, level):
    """The median is taken over the positive entries of the WHOLE array (weighting.py:220-225); a new longdouble array"""
    out = np.array(counts, dtype=LD)
    pos = out > 0
    if not level or not pos.any():
        return out
    lowval = np.median(out[pos]) / LD(level)
    out[pos] = np.maximum(out[pos], lowval)
    return out


def ref_box(counts, s):
    """Explicit zero-padded window sums (weighting.py:229-254); a new longdouble array"""
    counts = np.array(counts, dtype=LD)
    if s is None or s <= 0:
        return counts
    s = int(s)
    ncorr, nx, ny = counts.shape
    pad = np.zeros((ncorr, nx + 2 * s, ny + 2 * s), dtype=LD)
    pad[:, s:s + nx, s:s + ny] = counts
    out = np.zeros_like(counts)
    for dx in range(2 * s + 1):
        for dy in range(2 * s + 1):
            out += pad[:, dx:dx + nx, dy:dy + ny]
    return out


def ref_briggs(counts, robust):
    """weighting.py:146-147, 162-174: ``(counts, changed)``.  All-zero counts change nothing.  With ``robust > -2`` a dead plane
    beside a live one is ``0 / 0``: its counts come out NaN."""
    counts = np.array(counts, dtype=LD)
    if not counts.any():
        return counts, False
    if robust > -2:
        numsqrt = LD(5) * LD(10) ** (-LD(robust))
        num = (counts * counts).sum(axis=(1, 2))
        den = counts.sum(axis=(1, 2))
        with np.errstate(invalid="ignore", divide="ignore"):
            ssq = numsqrt * numsqrt * den / num
            counts = counts * ssq[:, None, None] + 1
    return counts, True


def ref_divide(counts, cell, wgt):
    """``wgt / counts[cell]`` where the cell is valid and ``counts > 0`` (weighting.py:203-206), rounded to float64 once: where
    the longdouble counts are a float64 exactly, the quotient is taken in float64 (correctly rounded) so that no second
    rounding enters"""
    out = np.array(wgt, dtype=np.float64)
    ncorr = out.shape[0]
    flat = counts.reshape(ncorr, -1)
    ok = cell >= 0
    for k in range(ncorr):
        c = flat[k][cell[ok]]
        w = out[k][ok]
        div = c > 0
        c64 = c.astype(np.float64)
        same = c64.astype(LD) == c
        q = np.where(same, w / np.where(div, c64, 1.0), (w.astype(LD) / np.where(div, c, LD(1))).astype(np.float64))
        out[k][ok] = np.where(div, q, w)
    return out


def reference(case):
    """Every stage of the chain for a chain case, rounded to float64: ``cell``, ``counts``, ``filtered``, ``boxed``, ``final`` (the
    counts ``imaging_weights(return_counts=True)`` returns), ``weights``, ``changed`` and ``h``, the largest number of samples in
    one cell."""
    c = case
    cell = ref_index(c["uvw"], c["freq"], c["mask"], c["nx"], c["ny"], c["cell_x"], c["cell_y"], c["usign"], c["vsign"])
    counts = ref_counts(cell, c["wgt"], c["nx"], c["ny"])
    filtered = ref_filter(counts, c["level"])
    boxed = ref_box(filtered, c["sup"])
    final, changed = ref_briggs(boxed, c["robust"])
    weights = ref_divide(final, cell, c["wgt"]) if changed else np.array(c["wgt"], dtype=np.float64)
    hits = np.bincount(cell[cell >= 0], minlength=1)
    out = dict(cell=cell, counts=counts.astype(np.float64), filtered=filtered.astype(np.float64), boxed=boxed.astype(np.float64),
               final=final.astype(np.float64), weights=weights, changed=changed, h=int(hits.max()))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def bounds(h, s, per, scaled):
    """Relative, elementwise bounds of the stages for float64 arithmetic in any summation order, with ``u = 2^-53``, ``h`` the
    largest number of samples the restatement puts in one cell, ``s`` the box half-width, ``per = nx * ny`` and ``scaled``
    whether the Briggs scaling runs (``robust > -2``).

    Every term summed is non-negative, so a float64 sum of ``m`` of them in any order is within ``m u`` of the exact sum,
    relatively (every partial sum is an exact sum rounded once; the restatement's own rounding to float64 is one of the m).

      counts    h u
      filtered  (h + 1) u: a cell near the threshold is either left alone or set to median / level, and these two coincide to
                that accuracy exactly when the choice can differ
      boxed     + (2 s + 1)^2 u: the window's terms
      final     + (2 per + 16) u when scaled: two sums of ``per`` terms, the squares, ``pow``, the multiply-add
      weights   + u: the division
    """
    b = {"counts": h * U}
    b["filtered"] = (h + 1) * U
    b["boxed"] = b["filtered"] + (2 * max(int(s or 0), 0) + 1) ** 2 * U
    b["final"] = b["boxed"] + ((2 * per + 16) * U if scaled else 0.0)
    b["weights"] = b["final"] + U
    return b


def worst(got, ref, bound):
    """``max |got - ref| / (bound |ref|)`` over the entries where ``ref`` is finite and not zero; ``inf`` when NaNs or zeros do
    not sit in the same places.  ``bound == 0`` asks for equality."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return np.inf
    fin = ~np.isnan(ref)
    g, r = got[fin], ref[fin]
    zero = r == 0
    if (g[zero] != 0).any():
        return np.inf
    err = np.abs(g[~zero] - r[~zero]) / np.abs(r[~zero])
    if not err.size:
        return 0.0
    if bound == 0:
        return 0.0 if not err.any() else np.inf
    return float(err.max() / bound)


# ---- chain cases -----------------------------------------------------------------------------------------------------------

EXACT_GRID = dict(nx=8, ny=16, cell_x=2.0 ** -10, cell_y=2.0 ** -11)
EXACT_FACTORS = (1.0, 1.25, 1.5, 1.75, 2.0)


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def dyadic_weights(rng, shape):
    """integer multiples of 2^-10, positive and below 64"""
    return rng.integers(1, 1 << 16, size=shape).astype(np.float64) / 1024.0


def exact_case(nrow, nchan, ncorr, signs=(1.0, -1.0), robust=-3.0, level=4.0, sup=0, seed=0, fixed=True, masked=0.1,
               promises=()):
    """An exact case (module docstring).  ``fixed`` sets the first rows by hand, in the coordinates after the signs: (0, 0),
    (umax / 2, 0.0), (-umax / 2, -0.0), (+-umax, v_cell), (u_cell, vmax / 2), (u_cell, vmax), one in the last cell
    ``(nx - 1, ny - 1)`` and (-umax, 0.0), which lies in cell ``(0, ny / 2)``."""
    g = EXACT_GRID
    u_cell, umax, v_cell, vmax = geometry(g["nx"], g["ny"], g["cell_x"], g["cell_y"])
    assert (u_cell, umax, v_cell, vmax) == (128.0, 512.0, 128.0, 1024.0)
    rng = np.random.default_rng(seed)
    usign, vsign = signs
    uvw = np.empty((nrow, 3))
    uvw[:, 0] = rng.integers(-16, 17, nrow) * (u_cell / 4)
    uvw[:, 1] = rng.integers(-32, 33, nrow) * (v_cell / 4)
    uvw[:, 2] = rng.standard_normal(nrow)
    rows = [(0.0, 0.0), (umax / 2, 0.0), (-umax / 2, -0.0), (umax, v_cell), (-umax, v_cell), (u_cell, vmax / 2), (u_cell, vmax),
            (umax - u_cell / 2, vmax - v_cell / 4), (-umax, 0.0)]
    nfix = min(len(rows), nrow) if fixed else 0
    for r in range(nfix):
        uvw[r, 0], uvw[r, 1] = rows[r][0] * usign, rows[r][1] * vsign  # (signs are +-1: the product undoes itself exactly)
    freq = LIGHTSPEED * np.array(EXACT_FACTORS[:nchan] if nchan > 1 else (1.0,))
    assert freq.size == nchan and np.array_equal(freq / LIGHTSPEED, EXACT_FACTORS[:nchan])
    mask = (rng.random((nrow, nchan)) >= masked).astype(np.uint8)
    mask[:nfix] = 1
    wgt = dyadic_weights(rng, (ncorr, nrow, nchan))
    return _freeze(dict(uvw=uvw, freq=freq, mask=mask, wgt=wgt, usign=usign, vsign=vsign, robust=robust, level=level, sup=sup,
                        exact=True, promises=dict(promises), **g))


def general_case(nrow, nchan, ncorr, nx, ny, signs, robust=0.0, level=5.0, sup=0, seed=0, cell_x=1.3e-3, cell_y=0.9e-3, spread=0.45,
                 dyadic=False, masked=0.08, promises=()):
    """Unequal cells, Gaussian uv-coordinates of which some fall out of range, lognormal weights (dyadic ones on request)"""
    rng = np.random.default_rng(seed)
    _, umax, _, vmax = geometry(nx, ny, cell_x, cell_y)
    freq = np.linspace(0.9e9, 1.3e9, nchan) if nchan > 1 else np.array([1.1e9])
    nf = freq.mean() / LIGHTSPEED
    uvw = rng.standard_normal((nrow, 3)) * np.array([spread * umax / nf, spread * vmax / nf, 1.0])
    mask = (rng.random((nrow, nchan)) >= masked).astype(np.uint8)
    wgt = dyadic_weights(rng, (ncorr, nrow, nchan)) if dyadic else np.exp(rng.standard_normal((ncorr, nrow, nchan)))
    return _freeze(dict(uvw=uvw, freq=freq, mask=mask, wgt=wgt, nx=nx, ny=ny, cell_x=cell_x, cell_y=cell_y, usign=signs[0],
                        vsign=signs[1], robust=robust, level=level, sup=sup, exact=False, promises=dict(promises)))


def _with(case, **kw):
    """A copy of ``case`` with fields replaced (arrays frozen again)"""
    out = dict(case)
    out["promises"] = dict(kw.pop("promises", case["promises"]))
    out.update(kw)
    return _freeze(out)


def _one_cell(n=300):
    """all ``n`` samples in ONE cell of the exact grid: atomic contention on a single address"""
    c = exact_case(n, 1, 2, robust=-2.0, level=4.0, fixed=False, masked=0.0, seed=3, promises=dict(cells=1, in_range=n))
    uvw = np.array(c["uvw"])
    uvw[:, 0], uvw[:, 1] = 160.0, -96.0   # v_tmp = +96 with vsign = -1: cell (5, 8), no fold
    return _with(c, uvw=uvw)


def _heavy_cells():
    """3000 samples of which 1200 lie in one cell and 1400 in another: each of the two spans more than one chunk of 1024 sorted
    samples of the device's segmented sum, and the chunk boundaries fall inside them; the other 400 are spread"""
    c = exact_case(3000, 1, 2, (-1.0, 1.0), robust=-2.0, level=4.0, sup=1, fixed=False, seed=15, promises=dict(max_in_cell=1400))
    uvw, mask = np.array(c["uvw"]), np.array(c["mask"])
    uvw[:1200, 0], uvw[:1200, 1] = -160.0, 96.0       # (signs (-1, 1): u_tmp = 160, v_tmp = 96, cell (5, 8))
    uvw[1200:2600, 0], uvw[1200:2600, 1] = 96.0, 352.0   # u_tmp = -96, v_tmp = 352: cell (3, 10)
    mask[:2600] = 1
    return _with(c, uvw=uvw, mask=mask)


def _out_of_range():
    """every sample unmasked and off the grid: u beyond umax, or v beyond vmax, or both"""
    c = exact_case(67, 5, 2, robust=0.0, seed=9, fixed=False, masked=0.0)
    uvw = np.array(c["uvw"])
    uvw[0::2, 0] += 4096.0
    uvw[1::2, 1] -= 8192.0
    uvw[2::4, 1] += 8192.0
    return _with(c, uvw=uvw, promises=dict(in_range=0, out_of_range=335, masked=0))


def _stride():
    """513 x 512, one plane: the smallest grid on which the per-plane reduction's blocks stride (more than 1024 blocks of 256).
    Twenty samples lie in the last row, which only the second trip of the stride loop reads.  Dyadic weights and a
    power-of-two level keep everything before the Briggs sums exact."""
    c = general_case(300, 1, 1, 513, 512, (-1.0, 1.0), robust=0.0, level=4.0, sup=0, seed=24, dyadic=True)
    _, umax, _, vmax = geometry(513, 512, c["cell_x"], c["cell_y"])
    nf = c["freq"][0] / LIGHTSPEED
    uvw, mask = np.array(c["uvw"]), np.array(c["mask"])
    uvw[:20, 0] = c["usign"] * umax * (1 - 1 / 1026) / nf            # ug = 512.5
    uvw[:20, 1] = c["vsign"] * vmax * np.linspace(0.05, 0.9, 20) / nf
    mask[:20] = 1
    return _with(c, uvw=uvw, mask=mask, promises=dict(per=513 * 512, past_1024_blocks=20))


def _dead(case, planes):
    wgt = np.array(case["wgt"])
    wgt[list(planes)] = 0.0
    return _with(case, wgt=wgt, promises=dict(case["promises"], dead=len(planes)))


_EDGES = dict(ug_integral=40, ug_eq_nx=3, ug_eq_0=3, v_zero=10, v_negzero=1, vg_eq_ny=2, masked=10, out_of_range=40,
              last_cell=1, cell_0_half=1)

CHAIN = {
    # -- exact: the index edges, either sign pair, through the whole chain
    "exact-(1,-1)": lambda: exact_case(67, 5, 2, (1.0, -1.0), robust=-3.0, level=4.0, sup=1, seed=1, promises=_EDGES),
    "exact-(-1,1)": lambda: exact_case(67, 5, 2, (-1.0, 1.0), robust=-2.0, level=8.0, sup=0, seed=2, promises=_EDGES),
    "exact-(1,1)": lambda: exact_case(67, 5, 3, (1.0, 1.0), robust=-3.0, level=8.0, sup=2, seed=3, promises=_EDGES),
    # -- shapes (nrow, nchan): 0, 1, 255, 256 and 257 samples; a row that straddles a workgroup is in 67 x 5 above
    "nrow0": lambda: exact_case(0, 3, 2, robust=0.0, promises=dict(nvis=0)),
    "nvis1": lambda: exact_case(1, 1, 1, robust=0.0, level=4.0, promises=dict(nvis=1, in_range=1)),
    "nvis255": lambda: exact_case(51, 5, 4, (-1.0, 1.0), robust=-3.0, level=4.0, sup=1, seed=5, promises=dict(nvis=255)),
    "nvis256": lambda: exact_case(64, 4, 3, (1.0, -1.0), robust=-2.0, level=8.0, seed=6, promises=dict(nvis=256)),
    "nvis257": lambda: exact_case(257, 1, 1, (-1.0, 1.0), robust=0.0, level=4.0, sup=1, seed=7, promises=dict(nvis=257)),
    "one-cell-300": _one_cell,
    "one-cell-2500": lambda: _with(_one_cell(2500), promises=dict(cells=1, in_range=2500, max_in_cell=2500)),
    "heavy-cells-3000": _heavy_cells,
    "heavy-cells-lognormal": lambda: _with(_heavy_cells(), wgt=np.exp(np.random.default_rng(16).standard_normal((2, 3000, 1))),
                                           exact=False, robust=0.0, level=5.0),
    "all-masked": lambda: _with(exact_case(67, 5, 2, robust=0.0, seed=8), mask=np.zeros((67, 5), np.uint8),
                                promises=dict(in_range=0, masked=335)),
    "all-out-of-range": lambda: _out_of_range(),
    "all-zero-weight": lambda: _dead(exact_case(67, 5, 2, robust=0.0, seed=10), (0, 1)),
    # -- Briggs on exact counts: the threshold of the scaling and either side of it
    "robust-3": lambda: exact_case(67, 5, 2, (-1.0, 1.0), robust=-3.0, level=0.0, sup=1, seed=11),
    "robust-2": lambda: exact_case(67, 5, 2, (-1.0, 1.0), robust=-2.0, level=4.0, sup=1, seed=11),
    "robust-2+": lambda: exact_case(67, 5, 2, (-1.0, 1.0), robust=float(np.nextafter(-2.0, 0.0)), level=4.0, sup=1, seed=11),
    "robust0": lambda: exact_case(67, 5, 2, (-1.0, 1.0), robust=0.0, level=4.0, sup=1, seed=11),
    "robust2": lambda: exact_case(67, 5, 2, (-1.0, 1.0), robust=2.0, level=4.0, sup=1, seed=11),
    # -- dead planes beside live ones
    "dead-1of3": lambda: _dead(exact_case(67, 5, 3, (-1.0, 1.0), robust=0.0, level=4.0, sup=1, seed=12), (1,)),
    "dead-1of2": lambda: _dead(exact_case(67, 5, 2, (1.0, -1.0), robust=0.0, level=8.0, seed=13), (1,)),
    "dead-1of3-unscaled": lambda: _dead(exact_case(67, 5, 3, (-1.0, 1.0), robust=-3.0, level=4.0, sup=1, seed=12), (1,)),
    "dead-general": lambda: _dead(general_case(67, 5, 3, 10, 14, (-1.0, 1.0), robust=0.5, level=5.0, sup=1, seed=14), (0,)),
    # -- general: unequal cells, lognormal weights, the callers' defaults
    "general-10x14": lambda: general_case(67, 5, 2, 10, 14, (1.0, -1.0), robust=0.0, level=5.0, sup=0, seed=20),
    "general-23x18": lambda: general_case(257, 1, 4, 23, 18, (-1.0, 1.0), robust=-1.0, level=10.0, sup=2, seed=21),
    "general-15x12": lambda: general_case(51, 5, 3, 15, 12, (1.0, -1.0), robust=1.0, level=10.0, sup=1, seed=22),
    "general-unscaled": lambda: general_case(64, 4, 1, 23, 18, (-1.0, 1.0), robust=-3.0, level=5.0, sup=3, seed=23),
    "stride-513x512": _stride,
}


@lru_cache(maxsize=None)
def chain_case(name):
    return CHAIN[name]()


@lru_cache(maxsize=None)
def chain_reference(name):
    """computed once per process and read-only"""
    return reference(chain_case(name))


def census(case):
    """How many unmasked samples of ``case`` sit on each edge of the index map, with ``masked``, ``out_of_range`` (unmasked, no
    cell), ``in_range``, ``cells`` (distinct cells hit), hits in the last cell ``(nx - 1, ny - 1)`` and in ``(0, ny / 2)``,
    in cells past the first 1024 * 256 of a plane, ``max_in_cell`` (the most samples in one cell), ``dead`` (planes without weight), ``nvis`` and ``per``."""
    c = case
    nx, ny = c["nx"], c["ny"]
    v0, ug, vg = grid_coords(c["uvw"], c["freq"], nx, ny, c["cell_x"], c["cell_y"], c["usign"], c["vsign"])
    m = np.asarray(c["mask"]) != 0
    cell = ref_index(c["uvw"], c["freq"], c["mask"], nx, ny, c["cell_x"], c["cell_y"], c["usign"], c["vsign"])
    n = lambda cond: int((cond & m).sum())  # noqa: E731
    return dict(ug_integral=n(ug == np.floor(ug)), ug_eq_nx=n(ug == nx), ug_eq_0=n(ug == 0), v_zero=n(v0 == 0),
                v_negzero=n((v0 == 0) & np.signbit(v0)), vg_eq_ny=n(vg == ny), masked=int((~m).sum()),
                out_of_range=int((m & (cell < 0)).sum()), in_range=int((cell >= 0).sum()), cells=int(np.unique(cell[cell >= 0]).size),
                last_cell=int((cell == nx * ny - 1).sum()), cell_0_half=int((cell == ny // 2).sum()),
                past_1024_blocks=int((cell >= 1024 * 256).sum()), max_in_cell=int(np.bincount(cell[cell >= 0], minlength=1).max()),
                dead=int((~np.asarray(c["wgt"]).reshape(c["wgt"].shape[0], -1).any(axis=1)).sum()), nvis=int(m.size), per=nx * ny)


# promises that are exact figures; every other one is a minimum
EXACT_PROMISES = ("nvis", "in_range", "cells", "dead", "per", "past_1024_blocks")


# ---- filter cases: counts handed in ----------------------------------------------------------------------------------------

def _dy(rng, n, lo=1, hi=1 << 14):
    return rng.integers(lo, hi, size=n).astype(np.float64) / 1024.0


def _scatter(shape, values, seed):
    """``values`` at random places of a zero array of ``shape``"""
    a = np.zeros(int(np.prod(shape)))
    a[np.random.default_rng(seed).permutation(a.size)[:len(values)]] = values
    return a.reshape(shape)


def _joint_planes():
    """Two planes of different scale.  Joint median 8 (of 1, 2, 4, 8, 512, 1024, 2048), level 4: threshold 2, raises the 1.
    Per plane the medians are 2 and 768 (thresholds 0.5 and 192): plane 0 would stay as it is and plane 1's 8 would rise."""
    a = np.zeros((2, 5, 7))
    a[0, 1, 2], a[0, 3, 3], a[0, 4, 6] = 1.0, 2.0, 4.0
    a[1, 0, 0], a[1, 2, 5], a[1, 3, 1], a[1, 4, 4] = 8.0, 512.0, 1024.0, 2048.0
    joint = ref_filter(a, 4.0)
    per_plane = np.stack([ref_filter(a[k:k + 1], 4.0)[0] for k in range(2)])
    assert not np.array_equal(joint, per_plane) and joint[0, 1, 2] == 2.0 and per_plane[0, 1, 2] == 1.0 and per_plane[1, 0, 0] == 192.0
    return a


def filter_cases():
    """``name -> (counts, level, npos, bound)``: ``bound`` 0 asks for equality (dyadic values and a power-of-two level make
    median / level exact).  The general case has level 10: the device rounds the mean of the two middle values and the
    quotient, the restatement rounds once: 3 u."""
    rng = np.random.default_rng(30)
    tie = _scatter((1, 6, 9), [1.0, 2.0, 2.0 + 2.0 ** -40, 8.0, 8.0, 30.0, 31.0], 31)   # median 8, level 4: a value == 2
    out = {
        "one-positive": (_scatter((1, 5, 7), [3.0], 32), 4.0, 1, 0),
        "odd": (_scatter((2, 5, 7), _dy(rng, 7), 33), 4.0, 7, 0),
        "even": (_scatter((2, 5, 7), _dy(rng, 8), 34), 8.0, 8, 0),
        "all-equal": (_scatter((1, 6, 9), [2.5] * 20, 35), 4.0, 20, 0),
        "tie-at-threshold": (tie, 4.0, 7, 0),
        "not-a-multiple-of-256": (_scatter((3, 7, 13), _dy(rng, 150), 36), 8.0, 150, 0),
        "joint-median": (_joint_planes(), 4.0, 7, 0),
        "none-positive": (np.zeros((2, 5, 7)), 4.0, 0, 0),
        "general-level-10": (_scatter((2, 23, 18), np.exp(2.0 * rng.standard_normal(400)), 37), 10.0, 400, 3 * U),
    }
    for a, _, _, _ in out.values():
        a.setflags(write=False)
    return out


# ---- box cases: counts handed in -------------------------------------------------------------------------------------------

def _boundary_planes():
    """Three planes with mass only in each plane's last row and the next plane's first row: a window that ran across a plane
    boundary would pick up the neighbour's mass"""
    a = np.zeros((3, 4, 6))
    rng = np.random.default_rng(40)
    for k in range(3):
        a[k, -1] = rng.integers(1, 100, 6)
        if k + 1 < 3:
            a[k + 1, 0] = rng.integers(100, 200, 6)
    return a


def box_cases():
    """``name -> (counts, s, bound)``: integer-valued counts sum exactly (bound 0); the general case holds (2 s + 1)^2 u"""
    rng = np.random.default_rng(41)
    ints = rng.integers(0, 50, (2, 5, 9)).astype(np.float64)
    line = rng.integers(0, 50, (2, 1, 11)).astype(np.float64)
    out = {f"5x9-s{s}": (ints, s, 0) for s in (1, 3, 5, 9, 12)}   # s = 5 >= nx, s = 9 >= ny, s = 12 beyond both
    out["1xN-s2"] = (line, 2, 0)
    out["Nx1-s2"] = (np.ascontiguousarray(line.transpose(0, 2, 1)), 2, 0)
    out["plane-boundaries-s1"] = (_boundary_planes(), 1, 0)
    out["plane-boundaries-s4"] = (_boundary_planes(), 4, 0)
    out["general-23x18-s2"] = (np.exp(rng.standard_normal((3, 23, 18))), 2, 25 * U)
    for a, _, _ in out.values():
        a.setflags(write=False)
    return out
