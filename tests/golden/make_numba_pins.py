#!/usr/bin/env python3
"""Reference-RUN fixtures of the reference's numba kernels: ``numba_pins.npz``.

make_ref_pins.py cannot take decorated functions: numba is not installed.  The reference's numba functions are, however,
plain Python under their decorators.  This script puts a STAND-IN ``numba`` into ``sys.modules`` and then executes the
reference's files AS THEY STAND at generation time.  No reference text is stored: only inputs, outputs and ``cites``.

The stand-in, exactly:

  * ``numba`` is a ``types.ModuleType`` with ``njit`` / ``jit`` (``njit(f)`` returns ``f``; ``njit(**kw)`` returns the
    identity decorator: every option -- nogil, cache, parallel, fastmath, inline, error_model -- is ignored),
    ``prange = range`` and ``literally = lambda x: x``;
  * ``numba.extending`` has ``overload(*a, **kw)``, which returns the identity decorator, and ``register_jitable``, which is
    the same function as ``njit`` above (bare, or with options that are ignored); nothing is registered;
  * ``pfb_imaging`` and ``pfb_imaging.wavelets`` are empty package stubs, present only while ``wavelets/convolutions.py``
    and ``wavelets/wavelets.py`` are loaded WHOLE (importlib, unmodified) under their own dotted names, so that the second
    file's ``from pfb_imaging.wavelets.convolutions import ...`` finds the first.  All of it is removed from ``sys.modules``
    afterwards.

So what runs is CPython evaluating the reference's statements one by one in IEEE double (or ``np.longdouble``): no fastmath
reassociation, no FMA contraction, loops in program order.

``utils/weighting.py`` and ``prox/prox_21m.py`` are not loaded whole (the first imports modules absent here): the functions
are taken with make_ref_pins.py's ``take()`` recipe -- the file's imports are executed one by one and the unsatisfiable ones
skipped -- extended to (a) execute the named module-level assignments the decorators need (``JIT_OPTIONS``) and (b) accept
decorated functions whose decorators resolve to the stand-in (asserted).

What is pinned (``cites`` in the file has the line ranges):

  wavelets/wavelets.py      dwt2d_nocopyt / idwt2d_nocopyt, in float64 AND in np.longdouble (the functions run unmodified on
                            80-bit arrays).  The pin is the longdouble result rounded to float64; ``psi_floor`` holds the
                            float64 run's max-abs and relative-l2 distance from the longdouble run.  One case also runs the
                            older transposed dwt2d / idwt2d (with copyt): the two layouts are transposes of each other.
  operators/psi.py          the level loop and the final max of _build_wavelet_bookkeeping, executed statement by statement
                            (the function itself needs pywt and numba typed lists): ix iy sx sy spx spy ntotx ntoty nxmax nymax.
  utils/weighting.py        _compute_counts (ngrid 1 and 3), counts_to_weights (robust -3, 0.0, 2.0) on inputs whose every
                            edge the reference alone decides; the cell index of a visibility is read off a run of
                            _compute_counts on that visibility alone, with a unit weight.
  prox/prox_21m.py          dual_update_numba_fast, dyadic inputs, entries with |sum| == lam w exactly.

NOT pinned: the filters come from oracle/wavelet_filters.json (PyWavelets is absent, its tables stay unpinned); ducc0.

Inputs are stored as small integers (``*_num``) over a power of two (``X_DEN``, ``C_DEN`` ...), so they compress.

Run from the repo root in the build container:  python tests/golden/make_numba_pins.py
"""

import ast
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
SRC = "src/pfb_imaging"

sys.path.insert(0, ROOT)
from oracle import psi as opsi  # noqa: E402  (the filter tables of oracle/wavelet_filters.json)

X_DEN, C_DEN = 4.0, 2.0          # image = x_num / X_DEN, hdot input = c_num / C_DEN
LIGHTSPEED = 299792458.0          # scipy.constants.c; the frequencies below are exact multiples of it

# (wavelet, nlevel, nx, ny)
PSI_CASES = (
    # every db1..db8 at a level count that is its deepest on that size: (L - 1) 2^nlevel on the short axis
    ("db1", 1, 2, 2), ("db2", 2, 12, 20), ("db3", 1, 12, 10), ("db4", 1, 14, 16), ("db5", 1, 20, 18), ("db6", 1, 22, 24),
    ("db7", 1, 28, 26), ("db8", 2, 60, 62),
    ("db1", 5, 32, 96),                                                  # sx goes down to 1
    ("db1", 1, 2, 514), ("db1", 1, 514, 2), ("db2", 1, 6, 1030),         # sy and 2 sy cross 256, tiny other axis
    # odd sx / sy at every one of three levels, so that the padded size nx = cx + cx % 2 feeds a second padded level and the
    # ix / iy offsets accumulate over two of them: db2 sx 19, 11, 7 against sy 27, 15, 9 (nx < ny); db1 sx 17, 9, 5 against
    # sy 9, 5, 3 (nx > ny) and the other way round.  For db2 such chains start at 20, 36, 52; 20 admits two levels only, so
    # (36, 52) is the smallest (35 KB; with (52, 36) too, or db5 on (74, 90) at 150 KB, the file would pass its limit)
    ("db2", 3, 36, 52), ("db1", 3, 34, 18), ("db1", 3, 18, 34),
    # the members of the multi-basis handles, one level on the smallest size that admits db8 (two levels need (60, 62) for
    # every member: 140 KB more than the file has)
    ("db8", 1, 30, 32), ("db1", 1, 30, 32), ("db3", 1, 30, 32),
)
ALL_ODD = (("db2", 3, 36, 52), ("db1", 3, 34, 18), ("db1", 3, 18, 34), ("db2", 2, 12, 20))
COPYT_CASE = ("db2", 2, 12, 20)

# (ncorr, nx, ny, usign, vsign).  A covering design, not the product ncorr {1, 2, 4} x two sizes x two sign pairs: the product
# is twelve cases and about 220 KB, which does not fit beside the wavelet pins under 400 KB.  Every value of every factor
# appears, both sizes with both sign pairs; the correlation index enters the reference (and the kernels) only as the leading
# index of weight and counts, independently of the geometry, so (16, 16) meeting only ncorr 1 loses no path.
WGT_CASES = ((1, 16, 16, 1.0, -1.0), (2, 23, 18, -1.0, 1.0), (4, 23, 18, 1.0, -1.0), (1, 16, 16, -1.0, 1.0))
WGT_NROW, WGT_NCHAN = 199, 3      # 597 visibilities: not a multiple of 256
WGT_CELL = 2.0 ** -10
ROBUST = (-3, 0.0, 2.0)
W_DEN = 1024.0                    # weights are multiples of 2^-10 below 64: every count is an exact sum in any order

DUAL_NBAND = (1, 3, 17)
DUAL_SHAPE = (3, 7, 5)            # n = 105, not a multiple of 256
V_DEN = 8.0


# ---- the stand-in ---------------------------------------------------------------------------------------------------
def _njit(*args, **kw):
    if len(args) == 1 and callable(args[0]) and not kw:
        return args[0]
    return lambda f: f


def install_standin():
    numba = types.ModuleType("numba")
    numba.njit = numba.jit = _njit
    numba.prange = range
    numba.literally = lambda x: x
    ext = types.ModuleType("numba.extending")
    ext.overload = lambda *a, **kw: (lambda f: f)
    ext.register_jitable = _njit
    numba.extending = ext
    sys.modules["numba"], sys.modules["numba.extending"] = numba, ext
    return {_njit, ext.overload}


def load_wavelets():
    """The reference's wavelets/convolutions.py and wavelets/wavelets.py, loaded whole and unmodified."""
    stubs = ("pfb_imaging", "pfb_imaging.wavelets")
    for name in stubs:
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    mods = {}
    try:
        for leaf in ("convolutions", "wavelets"):
            name = f"pfb_imaging.wavelets.{leaf}"
            spec = importlib.util.spec_from_file_location(name, os.path.join(REF, SRC, "wavelets", leaf + ".py"))
            mods[leaf] = importlib.util.module_from_spec(spec)
            sys.modules[name] = mods[leaf]
            spec.loader.exec_module(mods[leaf])
    finally:
        for name in list(sys.modules):
            if name == "pfb_imaging" or name.startswith("pfb_imaging."):
                del sys.modules[name]
    return mods["wavelets"]


def take_numba(relpath, names, assigns, standin):
    """make_ref_pins.take() for decorated functions: imports one by one (failures skipped), the module-level assignments
    ``assigns``, then the functions ``names`` unmodified; every decorator must resolve to the stand-in."""
    path = os.path.join(REF, relpath)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    ns = {"__name__": "numbapin_" + os.path.basename(relpath)[:-3]}
    for node in tree.body:
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            try:
                exec(compile(ast.Module([node], []), path, "exec"), ns)
            except Exception:  # module absent here: the names stay unbound
                pass
        elif isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id in assigns for t in node.targets):
            exec(compile(ast.Module([node], []), path, "exec"), ns)
    found = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            for dec in node.decorator_list:
                target = dec.func if isinstance(dec, ast.Call) else dec
                obj = eval(compile(ast.Expression(target), path, "eval"), ns)
                assert obj in standin, f"{relpath}:{node.name}: decorator is not the stand-in"
            exec(compile(ast.Module([node], []), path, "exec"), ns)
            found[node.name] = (node.lineno, node.end_lineno)
    missing = set(names) - set(found)
    assert not missing, f"{relpath}: {missing} not found"
    return ns, found


def bookkeeping_statements():
    """The statements of _build_wavelet_bookkeeping's per-wavelet loop that are pure arithmetic (those naming pywt, its
    wavelet object, the typed filter lists or max_level are left out), and the final max() after the loop; unmodified."""
    rel = f"{SRC}/operators/psi.py"
    path = os.path.join(REF, rel)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_build_wavelet_bookkeeping")
    loop = next(n for n in fn.body if isinstance(n, ast.For) and isinstance(n.target, ast.Tuple)
                and [e.id for e in n.target.elts] == ["wi_idx", "wavelet"])
    skip = {"pywt", "wvlt", "max_level", "dec_lo_list", "dec_hi_list", "rec_lo_list", "rec_hi_list"}
    body = [s for s in loop.body if not ({n.id for n in ast.walk(s) if isinstance(n, ast.Name)} & skip)]
    tail = [s for s in fn.body if s.lineno > loop.end_lineno and isinstance(s, ast.Assign)]
    cite = [f"{rel}:{body[0].lineno}-{body[-1].end_lineno} _build_wavelet_bookkeeping (level loop, statement by statement)",
            f"{rel}:{tail[0].lineno}-{tail[-1].end_lineno} _build_wavelet_bookkeeping (nxmax, nymax)"]
    code = compile(ast.Module(body + tail, []), path, "exec")
    return code, cite


def run_bookkeeping(code, wv, wavelet, nlevel, nx, ny):
    z = lambda *s: np.zeros(s, dtype=np.int64)
    ns = dict(np=np, coeff_size=wv.coeff_size, signal_size=wv.signal_size, wavelet=wavelet, wi_idx=0, nxi=nx, nyi=ny,
              nlevel=nlevel, nxmax=0, nymax=0, ix_arr=z(1, nlevel, 2), iy_arr=z(1, nlevel, 2), sx_arr=z(1, nlevel),
              sy_arr=z(1, nlevel), spx_arr=z(1, nlevel), spy_arr=z(1, nlevel), ntotx_arr=z(1), ntoty_arr=z(1))
    exec(code, ns)
    return {k[:-4]: ns[k][0] for k in ns if k.endswith("_arr")} | {"nxmax": int(ns["nxmax"]), "nymax": int(ns["nymax"])}


def filters(name, dtype):
    return [np.ascontiguousarray(f, dtype=dtype) for f in opsi.filters(name)]


def dist(a64, ald):
    d = np.asarray(a64, dtype=np.longdouble) - ald
    nrm = np.sqrt((ald * ald).sum())
    return float(np.abs(d).max()), float(np.sqrt((d * d).sum()) / (nrm if nrm > 0 else 1))


def psi_pins(out, cites, wv, rng):
    code, cite = bookkeeping_statements()
    cites += cite
    cases, tots, floors = [], [], []
    images = {}      # one image per size: the bases of a multi-basis handle analyse the same image
    for wavelet, nlevel, nx, ny in PSI_CASES:
        tag = f"{wavelet}_{nlevel}_{nx}_{ny}"
        bk = run_bookkeeping(code, wv, wavelet, nlevel, nx, ny)
        if (wavelet, nlevel, nx, ny) in ALL_ODD:
            assert (bk["sx"] % 2).all() and (bk["sy"] % 2).all(), tag
        ntx, nty = int(bk["ntotx"]), int(bk["ntoty"])
        if (nx, ny) not in images:
            images[(nx, ny)] = rng.integers(-3, 4, size=(nx, ny)).astype(np.int8)
        x_num = images[(nx, ny)]
        c_num = rng.integers(-1, 2, size=(ntx, nty)).astype(np.int8)   # nonzero in the layout's margins too
        res = {}
        for dt in (np.float64, np.longdouble):
            dlo, dhi, rlo, rhi = filters(wavelet, dt)
            x, c = (x_num / X_DEN).astype(dt), (c_num / C_DEN).astype(dt)
            alpha = np.zeros((ntx, nty), dtype=dt)
            cbuff = np.zeros((bk["nxmax"], 2 * int(bk["sy"].max())), dtype=dt)
            wv.dwt2d_nocopyt(x, alpha, cbuff, bk["ix"], bk["iy"], bk["sx"], bk["sy"], dlo, dhi, nlevel)
            img = np.zeros((nx, ny), dtype=dt)
            keep = c.copy()
            wv.idwt2d_nocopyt(c, img, np.zeros_like(c), np.zeros_like(cbuff), bk["ix"], bk["iy"], bk["sx"], bk["sy"],
                              bk["spx"], bk["spy"], rlo, rhi, nlevel)
            assert np.array_equal(c, keep) and alpha.dtype == dt and img.dtype == dt
            res[dt] = (alpha, img)
        out[tag + "_x_num"], out[tag + "_c_num"] = x_num, c_num
        out[tag + "_alpha"] = res[np.longdouble][0].astype(np.float64)
        out[tag + "_img"] = res[np.longdouble][1].astype(np.float64)
        out[tag + "_bk"] = np.concatenate([bk["ix"], bk["iy"], bk["sx"][:, None], bk["sy"][:, None], bk["spx"][:, None],
                                           bk["spy"][:, None]], axis=1)      # (nlevel, 8)
        cases.append(tag)
        tots.append((ntx, nty, bk["nxmax"], bk["nymax"]))
        floors.append(dist(res[np.float64][0], res[np.longdouble][0]) + dist(res[np.float64][1], res[np.longdouble][1]))
        if (wavelet, nlevel, nx, ny) == COPYT_CASE:     # the older layout: (ntoty, ntotx) coefficients, scratch + copyt
            dt = np.longdouble
            dlo, dhi, rlo, rhi = filters(wavelet, dt)
            nxm, nym = bk["nxmax"], bk["nymax"]
            z = lambda *s: np.zeros(s, dtype=dt)
            at = z(nty, ntx)
            wv.dwt2d((x_num / X_DEN).astype(dt), at, z(nxm, nym), z(nym, nxm), bk["ix"], bk["iy"], bk["sx"], bk["sy"], dlo,
                     dhi, nlevel, z(nxm, nym))
            it = z(nx, ny)
            ct = np.ascontiguousarray((c_num / C_DEN).astype(dt).T)
            wv.idwt2d(ct, it, z(nty, ntx), z(nxm, nym), z(nym, nxm), bk["ix"], bk["iy"], bk["sx"], bk["sy"], bk["spx"],
                      bk["spy"], rlo, rhi, nlevel)
            out["copyt_case"] = np.array(tag)
            out["copyt_alpha"], out["copyt_img"] = at.astype(np.float64), it.astype(np.float64)
    out["psi_cases"], out["psi_tot"], out["psi_floor"] = np.array(cases), np.array(tots, dtype=np.int64), np.array(floors)
    out["psi_den"] = np.array([X_DEN, C_DEN])


def wgt_inputs(nx, ny, rng):
    """(uvw, freq, mask): rows whose cell the reference's own arithmetic decides.  freq / c is exactly 1, 1.5, 2."""
    freq = np.array([1.0, 1.5, 2.0]) * LIGHTSPEED
    umax, vmax = abs(1 / WGT_CELL / 2), abs(1 / WGT_CELL / 2)
    ucell, vcell = 1 / (nx * WGT_CELL), 1 / (ny * WGT_CELL)
    # |u f / c| reaches past umax = 512 on the last channel; every point comes four times (with other weights and masks), so
    # that cells are shared and the weights' outputs, one value per cell and correlation, compress
    nb = -(-WGT_NROW // 4)
    u = np.tile(rng.integers(-2400, 2401, size=nb) / 8.0, 4)[:WGT_NROW]
    v = np.tile(rng.integers(-2400, 2401, size=nb) / 8.0, 4)[:WGT_NROW]
    sp = []
    for j in (0, 1, nx // 2, nx - 1, nx):                        # ug an integer (exactly so where nx is a power of two)
        sp += [(j * ucell - umax, 33.125), (-(j * ucell - umax), -33.125)]
    for j in (ny // 2, ny // 2 + 1, ny - 1):                     # vg an integer
        sp += [(17.5, j * vcell - vmax), (-17.5, -(j * vcell - vmax))]
    tiny = 5e-324
    sp += [(100.125, 0.0), (-100.125, 0.0), (100.125, -0.0), (100.125, tiny), (100.125, -tiny), (-200.25, tiny), (-200.25, -tiny)]
    # one cell outside on every side: u below -umax, u == umax, v == vmax (either sign of v: the fold maps -vmax onto it)
    sp += [(-umax - ucell / 2, 40.0), (umax + ucell / 2, -40.0), (umax, 40.0), (-umax, 40.0), (3.0, vmax), (3.0, -vmax),
           (-3.0, vmax + vcell / 2), (3.0, -vmax - vcell / 2), (umax - ucell, 8.0), (3.0, vmax - vcell)]
    sp = np.array(sp)
    u[:len(sp)], v[:len(sp)] = sp[:, 0], sp[:, 1]
    u[len(sp):len(sp) + len(sp) // 2] = sp[:len(sp) // 2, 0] / 2   # the same edges met by the last channel (f / c == 2)
    v[len(sp):len(sp) + len(sp) // 2] = sp[:len(sp) // 2, 1] / 2
    uvw = np.stack([u, v, rng.integers(-8, 9, size=WGT_NROW) / 8.0], axis=1)
    mask = (rng.random((WGT_NROW, WGT_NCHAN)) > 0.15).astype(np.uint8)
    mask[:len(sp)] = 1
    mask[len(sp) - 3:len(sp), 1] = 0
    return uvw, freq, mask


def weighting_pins(out, cites, standin, rng):
    rel = f"{SRC}/utils/weighting.py"
    ns, found = take_numba(rel, ["_compute_counts", "counts_to_weights"], ("JIT_OPTIONS",), standin)
    cites += [f"{rel}:{a}-{b} {k}" for k, (a, b) in sorted(found.items())]
    assert ns["lightspeed"] == LIGHTSPEED
    cc, c2w = ns["_compute_counts"], ns["counts_to_weights"]
    names = []
    for ncorr, nx, ny, us, vs in WGT_CASES:
        tag = f"wgt_{ncorr}_{nx}_{ny}_{int(us)}_{int(vs)}"
        names.append(tag)
        uvw, freq, mask = wgt_inputs(nx, ny, rng)
        shape = (ncorr, WGT_NROW, WGT_NCHAN)
        w_num = rng.integers(1, 65536, size=shape)
        w_num[rng.random(shape) < 0.1] = 0
        geo = (nx, ny, WGT_CELL, WGT_CELL)
        # the cell of every visibility, read off the reference one visibility at a time
        cell = np.full((WGT_NROW, WGT_NCHAN), -1, dtype=np.int64)
        one = np.ones((1, 1, 1))
        for r in range(WGT_NROW):
            for f in range(WGT_NCHAN):
                g = cc(uvw[r:r + 1], freq[f:f + 1], mask[r:r + 1, f:f + 1], one, *geo, np.float64, usign=us, vsign=vs)
                hit = np.flatnonzero(g[0])
                assert hit.size <= 1
                if hit.size:
                    cell[r, f] = hit[0]
        # the cells that rows 60..63 fall into hold nothing but zero weights: a count of zero
        empty = np.unique(cell[60:64][cell[60:64] >= 0])
        assert empty.size >= 2
        w_num[:, np.isin(cell, empty)] = 0
        w_num = w_num.astype(np.uint16)
        wgt = w_num / W_DEN
        counts = cc(uvw, freq, mask, wgt, *geo, np.float64, ngrid=1, usign=us, vsign=vs)
        counts3 = cc(uvw, freq, mask, wgt, *geo, np.float64, ngrid=3, usign=us, vsign=vs)
        assert np.array_equal(counts, counts3), "dyadic weights: the sum must be exact in any order"
        # the weights handed to counts_to_weights are not the gridded ones: zero-count cells must leave them alone
        i_num = (2 ** rng.integers(0, 4, size=shape)).astype(np.uint8)      # 1/4 .. 2: powers of two, so the outputs compress
        out[tag + "_uvw"], out[tag + "_freq"], out[tag + "_mask"] = uvw, freq, mask
        out[tag + "_w_num"], out[tag + "_i_num"] = w_num, i_num
        out[tag + "_counts"], out[tag + "_cell"] = counts, cell.astype(np.int16)
        for rb in ROBUST:
            cnt = counts.copy()
            with np.errstate(all="ignore"):
                res = c2w(cnt, uvw, freq, i_num / 4.0, mask, *geo, rb, usign=us, vsign=vs)
            out[f"{tag}_imw_{rb}"] = res
        # all-masked: counts.any() is false, the weights come back unchanged
        nomask = np.zeros_like(mask)
        c0 = cc(uvw, freq, nomask, wgt, *geo, np.float64, usign=us, vsign=vs)
        assert not c0.any()
        w_in = i_num / 4.0
        res = c2w(c0, uvw, freq, w_in.copy(), mask, *geo, 0.0, usign=us, vsign=vs)
        assert np.array_equal(res, w_in)
    out["wgt_cases"] = np.array(names)
    out["wgt_den"] = np.array([W_DEN, 4.0, WGT_CELL])


def dual_pins(out, cites, standin, rng):
    rel = f"{SRC}/prox/prox_21m.py"
    ns, found = take_numba(rel, ["dual_update_numba_fast"], (), standin)
    cites += [f"{rel}:{a}-{b} {k}" for k, (a, b) in sorted(found.items())]
    fn = ns["dual_update_numba_fast"]
    lam, sigma = 0.75, 1.5
    for nband in DUAL_NBAND:
        shape = (nband,) + DUAL_SHAPE
        vp_num = rng.integers(-32, 33, size=shape)
        v_num = rng.integers(-32, 33, size=shape)
        # lam w = 0.75 * (4 k / 8) = 3 k / 8, exact; the range grows with the band sums so that about half is scaled
        w_num = rng.integers(0, 41, size=DUAL_SHAPE) * 4 * {1: 1, 3: 2, 17: 4}[nband]
        w_num[0, 0, :] = 0                                    # zero weights
        v_num[:, 1, 0, :] = 0                                 # zero band sums: vp cancels over the bands, or is zero
        vp_num[:, 1, 0, :] = 0
        if nband > 1:
            vp_num[0, 1, 0, :], vp_num[1, 1, 0, :] = 5, -5
        w_num[1, 0, 3:] = 0                                   # zero sum and zero weight
        vp, v, w = vp_num / V_DEN, v_num / V_DEN, w_num / V_DEN
        s = np.abs((vp + sigma * v).sum(axis=0))              # exact
        # |sum| == lam w exactly: w = |sum| / lam wherever that is a multiple of 1/8 (|sum| = k / 32 with 3 | k)
        k = np.round(s * 32).astype(np.int64)
        eq = (k % 3 == 0) & (rng.random(DUAL_SHAPE) < 0.8) & (k > 0)
        eq[0, 0, :] = eq[1, 0, :] = False
        w_num = np.where(eq, (k // 3) * 4, w_num * 4)         # denominators of 32 from here on
        w = w_num / 32.0
        assert np.array_equal((lam * w)[eq], s[eq]) and eq.sum() >= 5
        got = v.copy()
        fn(vp, got, lam, sigma=sigma, weight=w)
        assert np.array_equal(got[:, eq], (vp + sigma * v)[:, eq])
        tag = f"dual_{nband}"
        out[tag + "_vp_num"], out[tag + "_v_num"] = vp_num.astype(np.int8), v_num.astype(np.int8)
        out[tag + "_w_num"], out[tag + "_eq"], out[tag + "_out"] = w_num.astype(np.int16), eq, got
    out["dual_par"] = np.array([lam, sigma, V_DEN, 32.0])


def compute():
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not the 80-bit format here"
    standin = install_standin()
    try:
        wv = load_wavelets()
        rel = f"{SRC}/wavelets/"
        cites = [rel + "wavelets.py:216-343 dwt2d_nocopyt / idwt2d_nocopyt (file loaded whole under the stand-in numba)",
                 rel + "wavelets.py:14-25,38-205 copyt, dwt2d / idwt2d (one case)",
                 rel + "convolutions.py (file loaded whole): the 1-D kernels the above call"]
        out = {}
        rng = np.random.default_rng(20261017)
        psi_pins(out, cites, wv, rng)
        weighting_pins(out, cites, standin, rng)
        dual_pins(out, cites, standin, rng)
    finally:
        sys.modules.pop("numba", None)
        sys.modules.pop("numba.extending", None)
    out["cites"] = np.array(cites)
    return out


def main():
    out = compute()
    path = os.path.join(HERE, "numba_pins.npz")
    np.savez_compressed(path, **out)
    print("\n".join(out["cites"]))
    for tag, fl in zip(out["psi_cases"], out["psi_floor"]):
        print(f"{tag:18s} f64 floor: alpha max-abs {fl[0]:.2e} rel-l2 {fl[1]:.2e} | img max-abs {fl[2]:.2e} rel-l2 {fl[3]:.2e}")
    size = os.path.getsize(path)
    print("numba_pins.npz", size)
    assert size < 400 * 1024, "numba_pins.npz must stay under 400 KB"


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("make_numba_pins.py needs /root/reference (build container only); the committed .npz travels instead")
    main()
