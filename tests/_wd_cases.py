"""The case table of tests/test_gpu_wd_instantiations.py and what it shares with its CPU guard (tests/test_wd_cases_cpu.py).

csrc/gridder_wd.hip builds the one-plane kernels k_grid_wd<W, K, BC>, k_degrid_wd<W, K> and k_hess_wd<W, K, BC> for every
support W of with_W, every term count K of with_K (csrc/dispatch.hpp) and the block edges of with_BC.  A forced kernel row
``force=(SIGMA, W)`` with ``force_wmode=2`` pins W; K follows from the field of view and epsilon alone (choose_kernel: wd_K), so
the table crosses every W with one (field widening, epsilon) per K, at two plan sizes:

* ``small``: a 64 x 60 image, 2500 rows x 2 channels -- one scatter launch of 768-thread workgroups with the atomic tile flush,
  the 768-thread gather, and the gather / scatter pair inside a Hessian apply;
* ``coloured``: a 512 x 512 image on a 768 x 768 grid (whole tile pairs), 60000 rows x 2 channels, PFBHIP_WD_COLOURS=1 -- four
  colour launches of 256-thread workgroups and the fused Hessian kernel wherever wd_hessian_supported admits (W, block edge).

Both sizes once more under PFBHIP_WD_BLOCK=4 at W = 14, 15: the BC = 4 scatter on 3 x 20 lanes, which with_BC builds beside the
BC = 2 one of those supports and which the fused kernel does not take.
"""

import collections
import functools
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pfb-imaging_amd", "csrc")

SIGMA = 1.5  # oracle/es_kernel_table.json has this row for every W = 4 .. 16; a 512 image then gets a 768 grid
SUPPORTS = tuple(range(4, 17))
# K: (field widening, epsilon), as test_one_plane_w_scheme (64) and test_fused_hessian_term_counts (512) choose them
TERMS = {"small": {2: (30.0, 1e-4), 3: (130.0, 1e-7), 4: (200.0, 1e-7)},
         "coloured": {2: (10.0, 1e-4), 3: (16.0, 1e-7), 4: (30.0, 1e-7)}}
# size: (rows, channels, image edge of make_case, nx, ny, pixel aspect py / px, seed, scatter launches)
SIZES = {"small": (2500, 2, 64, 64, 60, 1.1, 5, 1), "coloured": (60000, 2, 512, 512, 512, 1.0, 11, 4)}
PIXEL_STRIDE, ROW_STRIDE = 41, 29  # the strided DFT subsets of the coloured size (test_one_plane_scatter_frames / _w_scheme)

Case = collections.namedtuple("Case", "size W K widen eps block")  # block: None (the plan's own block edge) or 4


def _cases():
    out = [Case(size, W, K, *TERMS[size][K], None) for size in ("small", "coloured") for W in SUPPORTS for K in (2, 3, 4)]
    # (the BC = 4 scatter of W = 14, 15 exists beside their BC = 2 one: both launch shapes of it as well)
    out += [Case(size, W, K, *TERMS[size][K], 4) for size in ("coloured", "small") for W in (14, 15) for K in (2, 3, 4)]
    return out


ONE_PLANE_CASES = _cases()

# The multi-plane register-frame scatters (k_grid_blk / k_grid_rec, csrc/gridder_kernels_mp.hpp) below the supports that
# test_multi_plane_scatter_frames pins: (wmode, field widening, zscale) as there, every W = 4 .. 12 at SIGMA.
MULTI_PLANE_SUPPORTS = tuple(range(4, 13))
MULTI_PLANE_GEOMETRIES = ((0, 30.0, 0.5), (1, 8.0, 0.02))
MULTI_PLANE_MODES = ("block", "rec_es")


def case_id(c):
    return f"{c.size}-W{c.W}-K{c.K}" + ("" if c.block is None else f"-block{c.block}")


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


# ---- what a case runs -------------------------------------------------------------------------------------------------------
def block_edge(c):
    """the scatter frame's block edge: 2 x 2-cell anchoring at W = 14, 15 unless PFBHIP_WD_BLOCK=4 (sort_key_sub, csrc/gridder.hip)"""
    return 2 if (c.W in (14, 15) and c.block is None) else 4


def runs_fused(c):
    """coloured plans whose frame fits a 16-lane row run k_hess_wd, every other plan the gather / scatter pair"""
    return c.size == "coloured" and c.W + block_edge(c) - 1 <= 16


def covered(cases=None):
    """the device functions the table reaches: {("grid", W, K, BC)}, {("degrid", W, K)}, {("hess", W, K, BC)}, each with the
    launch shape ("small": 768 threads, atomic flush; "coloured": 256 threads, colour launches) it is reached in"""
    out = set()
    for c in ONE_PLANE_CASES if cases is None else cases:
        out.add(("grid", c.W, c.K, block_edge(c), c.size))
        out.add(("degrid", c.W, c.K, c.size))
        if runs_fused(c):
            out.add(("hess", c.W, c.K, block_edge(c)))
    return out


# ---- what the sources build -------------------------------------------------------------------------------------------------
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int_range(src, fn):
    m = re.search(r"void " + fn + r"\([^)]*\)\s*\{\s*with_int<(\d+),\s*(\d+)>", src)
    assert m, fn
    return range(int(m.group(1)), int(m.group(2)) + 1)


def _c_predicate(expr, names):
    """a C++ boolean expression over ints as a Python function of ``names``"""
    py = expr.replace("&&", " and ").replace("||", " or ")
    assert re.fullmatch(r"[\w\s()<>=+\-,]*", py), expr
    return lambda *a, **env: bool(eval(py, {"__builtins__": {}}, dict(zip(names, a), **env)))  # noqa: S307 (checked above)


def built():
    """every one-plane device function csrc/gridder_wd.hip instantiates, read from the sources: with_W, with_K, with_BC
    (csrc/dispatch.hpp), wd_hessian_supported and the block edge wd_launch_hessian builds the fused kernel with"""
    disp, wd, kern = _read("dispatch.hpp"), _read("gridder_wd.hip"), _read("gridder_kernels_wd.hpp")
    Ws, Ks = _int_range(disp, "with_W"), _int_range(disp, "with_K")
    m = re.search(r"void with_BC\(int bc, F &&f\)\s*\{\s*if constexpr \(([^)]*)\) \{\s*if \(bc == (\d+)\) return \(void\)f\(std::integral_constant<int, "
                  r"(\d+)>\{\}\);\s*\}\s*f\(std::integral_constant<int, (\d+)>\{\}\);\s*\}", disp)
    assert m and m.group(2) == m.group(3), "with_BC changed its form: restate it here"
    fine_at, fine, coarse = _c_predicate(m.group(1), ["W"]), int(m.group(2)), int(m.group(4))
    # the three launchers go through exactly these dispatchers
    for fn, uses in (("wd_launch_grid", ("with_W", "with_K", "with_BC<W>")), ("wd_launch_degrid", ("with_W", "with_K")),
                     ("wd_launch_hessian", ("with_W", "with_K"))):
        body = wd[wd.index("void " + fn):]
        body = body[:body.index("\n}\n")]
        assert all(u + "(" in body for u in uses), fn
    m = re.search(r"constexpr bool wd_hess_fits\(int W, int BC\) \{ return ([^;]*); \}", kern)
    assert m, "wd_hess_fits"
    fits = _c_predicate(m.group(1), ["W", "BC"])
    m = re.search(r"bool wd_hessian_supported\(int W, int bc\) \{ return ([^;]*); \}", wd)
    assert m, "wd_hessian_supported"
    supported = _c_predicate(m.group(1), ["W", "bc"])
    body = wd[wd.index("void wd_launch_hessian"):]
    m = re.search(r"if constexpr \(([^)]*)\) \{[^\n]*\n\s*constexpr int BC = ([^?;]*) \? (\d+) : (\d+);", body)
    assert m, "wd_launch_hessian: the block edge the fused kernel is built with"
    hess_built, hess_fine_at, hess_bc = _c_predicate(m.group(1), ["W"]), _c_predicate(m.group(2), ["W"]), (int(m.group(3)), int(m.group(4)))
    out = set()
    for W in Ws:
        for K in Ks:
            for bc in {coarse} | ({fine} if fine_at(W) else set()):
                out.update(("grid", W, K, bc, size) for size in SIZES)
            out.update(("degrid", W, K, size) for size in SIZES)
            if hess_built(W):
                bc = hess_bc[0] if hess_fine_at(W) else hess_bc[1]
                assert supported(W, bc, wd_hess_fits=fits), (W, bc)  # (what is built is what the plan may select ...)
                out.add(("hess", W, K, bc))
        # (... and nothing the plan may select is left unbuilt: the launcher would fall through without a kernel)
        for bc in (fine, coarse):
            if supported(W, bc, wd_hess_fits=fits):
                assert hess_built(W) and bc == (hess_bc[0] if hess_fine_at(W) else hess_bc[1]), (W, bc)
    return out


# ---- inputs, geometry and references ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eps_sup(W, sigma=SIGMA):
    """the forced row's worst-position error (oracle/es_kernel_table.json), the quantity choose_kernel admits rows on"""
    with open(os.path.join(ROOT, "oracle", "es_kernel_table.json")) as f:
        rows = json.load(f)["rows"]
    (r,) = [r for r in rows if r["W"] == W and abs(r["sigma"] - sigma) < 1e-9]
    return r["eps_sup"]


def dft_tolerance(c):
    """against the direct DFT: a forced row skips the plan's admission test, so the bound is the row's own error where that
    exceeds the requested epsilon"""
    return max(c.eps, eps_sup(c.W))


@functools.lru_cache(maxsize=None)
def inputs(size):
    from pfb_imaging_amd.utils import synth

    nrow, nchan, npix, nx, ny, _, seed, _ = SIZES[size]
    c = synth.make_case(nrow, nchan, npix, zscale=1e-3, seed=seed)
    c["x"] = np.ascontiguousarray(c["x"][:nx, :ny])
    return c


def geometry(c):
    """the plan keywords of a case (Gridder and, without force_wmode, oracle.wgridder.Plan)"""
    _, _, _, nx, ny, aspect, _, _ = SIZES[c.size]
    cell = inputs(c.size)["cell"] * c.widen
    return dict(npix_x=nx, npix_y=ny, pixsize_x=cell, pixsize_y=cell * aspect, center_x=0.0, center_y=0.0, epsilon=c.eps,
                flip_u=False, flip_v=True, flip_w=False, do_wgridding=True, divide_by_n=False)


def subsets(size):
    """pixels (ix, iy) and rows (of channel 0) the DFT is evaluated at: all of them at the small size (None), strided at 512"""
    nrow, _, _, nx, ny, _, _, _ = SIZES[size]
    if size == "small":
        return None, None
    p = np.arange(0, nx * ny, PIXEL_STRIDE)
    return (p // ny, p % ny), np.arange(0, nrow, ROW_STRIDE)


@functools.lru_cache(maxsize=None)
def dft_reference(size, K):
    """(dirty image or its pixel subset, visibilities or their row subset of channel 0; masked ones zero) of the direct DFT:
    a function of the size and the field of view (K) only, so six references serve the whole table"""
    from oracle import dft

    c = inputs(size)
    kw = geometry(Case(size, 0, K, *TERMS[size][K], None))
    pix, rows = subsets(size)
    args = (kw["pixsize_x"], kw["pixsize_y"], 0.0, 0.0, False, True, False, True, False)
    d = dft.dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], c["mask"], kw["npix_x"], kw["npix_y"], *args, pixels=pix)
    if rows is None:
        v = dft.dft_dirty2vis(c["uvw"], c["freq"], c["x"], *args)
        v[c["mask"] == 0] = 0
    else:
        v = dft.dft_dirty2vis(c["uvw"], c["freq"], c["x"], *args, rows=rows, chans=np.zeros_like(rows)) * c["mask"][rows, 0]
    return d, v


def against_dft(c, dirty, vis):
    """relative L2 distances of a full dirty image / visibility array to the DFT reference of the case"""
    d, v = dft_reference(c.size, c.K)
    pix, rows = subsets(c.size)
    return rel(dirty if pix is None else dirty[pix], d), rel(vis if rows is None else vis[rows, 0], v)


def restatement(c, params=None):
    """the CPU restatement of the algorithm (oracle.wgridder.Plan): with a plan's own parameters, or forced to the case's row"""
    from oracle import wgridder as owg

    i, kw = inputs(c.size), geometry(c)
    force = {} if params is not None else dict(force=(SIGMA, c.W), force_wmode=2)
    return owg.Plan(i["uvw"], i["freq"], i["mask"], kw["npix_x"], kw["npix_y"], kw["pixsize_x"], kw["pixsize_y"], kw["center_x"],
                    kw["center_y"], kw["epsilon"], kw["flip_u"], kw["flip_v"], kw["flip_w"], kw["do_wgridding"], kw["divide_by_n"],
                    params=params, **force)
