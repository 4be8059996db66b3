"""The case table of tests/test_gpu_mp_instantiations.py and what it shares with its CPU guard (tests/test_mp_cases_cpu.py).

csrc/gridder_kernels_mp.hpp holds the kernels of every plan that is not on the one-plane w-scheme: the scatters k_grid_mp<W, KP>,
k_grid_blk<W, KP, BC>, k_grid_rec<W, KP, BC> and the gathers k_degrid_mp<W, KP>, k_degrid_rw<W, KP>, built by launch_grid /
launch_degrid (csrc/gridder.hip) for every support W of with_W, every number KP of planes per pass of with_KP and the block edges
of with_BC (csrc/dispatch.hpp).  A forced kernel row ``force=(SIGMA, W)`` pins W; KP follows from the plane count, which the
geometry (field widening, w spread of the baselines, epsilon) decides:

* a plan of ``n`` planes runs passes of ``min(4, n)`` planes and a tail of ``n % 4`` (``passes``);
* the register-frame scatters are launched with blk_threads(planes per pass of the PLAN) threads: k_grid_blk / k_grid_rec<W, KP <= 3>
  run on 768 threads in a plan of up to three planes and on 512 as the tail pass of a longer one;
* single-pass plans without ES-kernel planes take the row-walk gather, whose epilogue inside a Hessian apply of a record-scatter
  plan writes the scatter's values instead of accumulating (``values``); every other plan the walk gather.

So the table crosses every W with polynomial-plane geometries of 1 .. 7 planes (forced wmode 1: the count does not depend on W), one
plan without w-gridding, and ES-kernel plane stacks (forced wmode 0) of W + 0 .. 3 planes, whose tail W + c mod 4 takes every value
at every W -- each under PFBHIP_SCATTER = walk, block and rec (rec_es where the plan has ES planes or several passes), and the
polynomial geometries once more under PFBHIP_WD_BLOCK=4 at W = 14, 15 (the BC = 4 frame beside the BC = 2 one of those supports).
All of it on a 128 x 128 image, 3000 rows x 2 channels, whose 192 x 192 grid (six tiles a side) takes the four colour launches
with the plain tile flush.  Three supports (16-lane frame, 2 x 2 anchoring, 3 x 20 lanes) also run a single-pass and a multi-pass
plan on a 160 grid (five tiles: one launch, atomic flush) and on a 180 grid (partial last tile, the periodic wrap inside it).
"""

import collections
import functools
import re

import numpy as np

from tests._wd_cases import ROOT, SIGMA, _c_predicate, _int_range, _read, eps_sup, rel  # noqa: F401 (rel, ROOT: for the tests)

SUPPORTS = tuple(range(4, 17))
NROW, NCHAN, SEED = 3000, 2, 1
TILE = 32  # (csrc/plan_layout.hpp)
ES_EPSILON = 1e-7

# name: (image edge, field widening, zscale of synth.make_case, epsilon, do_wgridding, forced wmode, planes -- beyond W for wmode 0)
Geometry = collections.namedtuple("Geometry", "npix widen zscale eps do_w wmode planes")
GEOMETRIES = {
    "poly1": Geometry(128, 4.0, 0.02, 1e-3, True, 1, 1),
    "poly2": Geometry(128, 4.0, 0.02, 1e-5, True, 1, 2),
    "poly3": Geometry(128, 4.0, 0.1, 1e-7, True, 1, 3),
    "poly4": Geometry(128, 4.0, 0.1, 1e-10, True, 1, 4),
    "poly5": Geometry(128, 8.0, 0.5, 1e-10, True, 1, 5),
    "poly6": Geometry(128, 8.0, 1.0, 1e-10, True, 1, 6),
    "poly7": Geometry(128, 16.0, 0.5, 1e-10, True, 1, 7),
    "flat": Geometry(128, 4.0, 0.02, 1e-7, False, 0, 1),  # no w-gridding: one plane, wmode 0
    "es+0": Geometry(128, 30.0, 0.5, ES_EPSILON, True, 0, 0),
    "es+1": Geometry(128, 60.0, 0.5, ES_EPSILON, True, 0, 1),
    "es+2": Geometry(128, 60.0, 0.75, ES_EPSILON, True, 0, 2),
    "es+3": Geometry(128, 60.0, 1.0, ES_EPSILON, True, 0, 3),
    # grids that cannot take the colour launches: five tiles a side (160), a partial last tile (180); one pass and two
    "odd3": Geometry(106, 4.0, 0.1, 1e-7, True, 1, 3),
    "odd5": Geometry(106, 8.0, 0.5, 1e-10, True, 1, 5),
    "part3": Geometry(120, 4.0, 0.1, 1e-7, True, 1, 3),
    "part5": Geometry(120, 8.0, 0.5, 1e-10, True, 1, 5),
}
MAIN = tuple(k for k, g in GEOMETRIES.items() if g.npix == 128)
POLY = tuple(k for k in MAIN if k.startswith("poly"))
GRID_SHAPES = tuple(k for k, g in GEOMETRIES.items() if g.npix != 128)
GRID_SHAPE_SUPPORTS = (6, 14, 16)  # 16-lane frame; 2 x 2 anchoring; 3 x 20 lanes
GRID_EDGE = {128: 192, 106: 160, 120: 180}

Case = collections.namedtuple("Case", "W geom block")  # block: None (the plan's own block edge) or 4 (PFBHIP_WD_BLOCK=4)


def _cases():
    out = [Case(W, k, None) for W in SUPPORTS for k in MAIN]
    out += [Case(W, k, 4) for W in (14, 15) for k in POLY]
    out += [Case(W, k, None) for W in GRID_SHAPE_SUPPORTS for k in GRID_SHAPES]
    return out


CASES = _cases()


def case_id(c):
    return f"W{c.W}-{c.geom}" + ("" if c.block is None else f"-block{c.block}")


# ---- what a case runs -------------------------------------------------------------------------------------------------------
def nplanes(c):
    g = GEOMETRIES[c.geom]
    return g.planes + (c.W if (g.do_w and g.wmode == 0) else 0)


def passes(n, kp_most=4):
    """(planes per pass of the plan, [planes of each pass]): full passes of min(4, n) planes, then the tail"""
    kp_max = min(kp_most, n)
    return kp_max, [kp_max] * (n // kp_max) + ([n % kp_max] if n % kp_max else [])


def blk_threads(kp_max, few=3, wide=768, narrow=512):
    return wide if kp_max <= few else narrow


def row_walk(c):
    """single-pass plans without ES-kernel planes (choose_kernels: rec_mode): the row-walk gather, the record scatter on request"""
    g = GEOMETRIES[c.geom]
    return nplanes(c) <= passes(nplanes(c))[0] and (not g.do_w or g.wmode >= 1)


def forms(c):
    """the values of PFBHIP_SCATTER a case runs under: rec is honoured by row-walk plans, rec_es by every other one"""
    return ("walk", "block", "rec" if row_walk(c) else "rec_es")


def block_edge(c, form):
    """2 x 2-cell anchoring at W = 14, 15 wherever the sort key carries the blocks (not PFBHIP_SCATTER=walk, not PFBHIP_WD_BLOCK=4)"""
    return 2 if (c.W in (14, 15) and c.block is None and form != "walk") else 4


def launches(c, form):
    """scatter launches per pass: one per tile colour where the register-frame scatters meet whole tile pairs, else one"""
    edge = GRID_EDGE[GEOMETRIES[c.geom].npix]
    return 4 if (form != "walk" and edge % TILE == 0 and (edge // TILE) % 2 == 0) else 1


SCATTER_MODE = {"walk": 0, "block": 1, "rec": 2, "rec_es": 2}


def covered(cases=None):
    """the device functions the table reaches, with the launch shape they are reached in:
    ("grid_mp", W, KP); ("grid_blk" | "grid_rec", W, KP, BC, threads); ("degrid_mp", W, KP);
    ("degrid_rw", W, KP, "accumulate" | "values")"""
    out = set()
    for c in CASES if cases is None else cases:
        kp_max, kps = passes(nplanes(c))
        for form in forms(c):
            for kp in kps:
                if form == "walk":
                    out.add(("grid_mp", c.W, kp))
                else:
                    out.add(("grid_blk" if form == "block" else "grid_rec", c.W, kp, block_edge(c, form), blk_threads(kp_max)))
                if row_walk(c):
                    out.add(("degrid_rw", c.W, kp, "accumulate"))  # (dirty2vis, and the Hessian applies of the other two forms)
                    if form == "rec":
                        out.add(("degrid_rw", c.W, kp, "values"))  # (ApplyState::gather_values: the pval_out epilogue)
                else:
                    out.add(("degrid_mp", c.W, kp))
    return out


# ---- what the sources build -------------------------------------------------------------------------------------------------
def _member(src, name):
    m = re.search(r"\n    (?:void|bool) " + name + r"\(", src)
    assert m, name
    body = src[m.start():]
    return body[:body.index("\n    }\n")]


def built():
    """every multi-plane device function launch_grid / launch_degrid (csrc/gridder.hip) instantiate, in every launch shape a plan
    can give it, read from the sources: with_W, with_KP, with_BC (csrc/dispatch.hpp), KP_MAX and blk_threads
    (csrc/gridder_kernels_mp.hpp), the pass loop and choose_kernels' rule"""
    disp, grd, kern = _read("dispatch.hpp"), _read("gridder.hip"), _read("gridder_kernels_mp.hpp")
    Ws, KPs = _int_range(disp, "with_W"), _int_range(disp, "with_KP")
    m = re.search(r"void with_BC\(int bc, F &&f\)\s*\{\s*if constexpr \(([^)]*)\) \{\s*if \(bc == (\d+)\) return \(void\)f\(std::integral_constant<int, "
                  r"(\d+)>\{\}\);\s*\}\s*f\(std::integral_constant<int, (\d+)>\{\}\);\s*\}", disp)
    assert m and m.group(2) == m.group(3), "with_BC changed its form: restate it here"
    fine_at, fine, coarse = _c_predicate(m.group(1), ["W"]), int(m.group(2)), int(m.group(4))
    m = re.search(r"constexpr int KP_MAX = (\d+);", kern)
    assert m, "KP_MAX"
    kp_most = int(m.group(1))
    assert KPs == range(1, kp_most + 1), (KPs, kp_most)
    m = re.search(r"constexpr int blk_threads\(int KP\) \{ return KP <= (\d+) \? (\d+) : (\d+); \}", kern)
    assert m, "blk_threads changed its form: restate it here"
    threads = functools.partial(blk_threads, few=int(m.group(1)), wide=int(m.group(2)), narrow=int(m.group(3)))
    # the two launchers go through exactly these dispatchers and kernels, the scatters on blk_threads(planes per pass of the plan)
    grid, degrid = _member(grd, "launch_grid"), _member(grd, "launch_degrid")
    for body, uses in ((grid, ("with_W(", "with_KP(", "with_BC<W>(", "(k_grid_mp<W, KP>)", "(k_grid_blk<W, KP, BC>)", "(k_grid_rec<W, KP, BC>)",
                               "block(blk_threads(kp_max))")),
                       (degrid, ("with_W(", "with_KP(", "(k_degrid_rw<W, KP>)", "(k_degrid_mp<W, KP>)"))):
        assert all(u in body for u in uses), [u for u in uses if u not in body]
    assert set(re.findall(r"\(k_(?:de)?grid_\w+<[^>]*>\)", grid + degrid)) == {"(k_grid_mp<W, KP>)", "(k_grid_blk<W, KP, BC>)", "(k_grid_rec<W, KP, BC>)",
                                                                           "(k_degrid_rw<W, KP>)", "(k_degrid_mp<W, KP>)"}
    # passes of kp_max = min(KP_MAX, planes) planes and a tail, in both directions
    assert "g->kp_max = int(std::min<int64_t>(KP_MAX, info.nplanes));" in grd
    for fn in ("grid_all_planes", "degrid_all_planes"):
        body = _member(grd, fn)
        assert "for (int p0 = 0; p0 < info.nplanes; p0 += kp_max) {" in body, fn
        assert "const int kp = int(std::min<int64_t>(kp_max, info.nplanes - p0));" in body, fn
    # choose_kernels' rule, as row_walk / forms / covered restate it
    for line in ("const bool rec_mode = info.nplanes <= kp_max && (!prm.do_wgridding || info.wmode >= 1) && has_work;",
                 "const bool rec = (rec_mode || rec_es) && blk && sw.scatter != ScatterForce::Block;",
                 "p.scatter = !blk ? Scatter::Walk : info.wmode == 2 ? Scatter::OnePlane : rec ? Scatter::Rec : Scatter::Block;",
                 "p.gather = info.wmode == 2 ? Gather::OnePlane : rec_mode ? Gather::RowWalk : Gather::Walk;",
                 "p.gather_values = rec_mode && rec && !p.hess_fused;"):
        assert line in grd, "choose_kernels changed: restate it here (" + line + ")"
    # (planes of a pass, planes per pass of its plan): a plan of kp_max planes per pass runs passes of kp_max and, where more
    # planes than KP_MAX exist, a tail of fewer; ES-kernel stacks have at least min(with_W) >= KP_MAX planes, so a plan of fewer
    # planes than KP_MAX is a single-pass plan on the row-walk gather
    assert min(Ws) >= kp_most
    shapes = {(kp, kp) for kp in KPs} | {(kp, kp_most) for kp in KPs}
    out = set()
    for W in Ws:
        for kp, kp_max in shapes:
            for bc in {coarse} | ({fine} if fine_at(W) else set()):
                out.update((k, W, kp, bc, threads(kp_max)) for k in ("grid_blk", "grid_rec"))
        for kp in KPs:
            out.add(("grid_mp", W, kp))
            out.add(("degrid_mp", W, kp))  # (as a tail below KP_MAX; KP_MAX itself in every ES stack and every longer plan)
            out.update(("degrid_rw", W, kp, how) for how in ("accumulate", "values"))
    return out


# ---- inputs, geometry and references ----------------------------------------------------------------------------------------
def dft_tolerance(c):
    """against the direct DFT (tests/_wd_cases.py: dft_tolerance): a forced row skips the plan's admission test, so the bound is
    the row's own worst-position error where that exceeds the requested epsilon"""
    return max(GEOMETRIES[c.geom].eps, eps_sup(c.W))


@functools.lru_cache(maxsize=None)
def inputs(geom):
    from pfb_imaging_amd.utils import synth

    g = GEOMETRIES[geom]
    c = synth.make_case(NROW, NCHAN, 128, zscale=g.zscale, seed=SEED)
    c["x"] = np.ascontiguousarray(c["x"][:g.npix, :g.npix])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def geometry(geom):
    """the plan keywords of a geometry (Gridder and oracle.wgridder.Plan)"""
    g = GEOMETRIES[geom]
    cell = inputs(geom)["cell"] * g.widen
    return dict(npix_x=g.npix, npix_y=g.npix, pixsize_x=cell, pixsize_y=cell, center_x=0.0, center_y=0.0, epsilon=g.eps, flip_u=False,
                flip_v=True, flip_w=False, do_wgridding=g.do_w, divide_by_n=False)


def forcing(c):
    """the keywords that pin a case's kernel row and w-scheme"""
    g = GEOMETRIES[c.geom]
    return dict(force=(SIGMA, c.W), force_wmode=g.wmode if g.do_w else None)


@functools.lru_cache(maxsize=None)
def dft_reference(geom):
    """(dirty image, visibilities with the masked ones zero) of the direct DFT: a function of the geometry only"""
    from oracle import dft

    c, kw = inputs(geom), geometry(geom)
    args = (kw["pixsize_x"], kw["pixsize_y"], 0.0, 0.0, False, True, False, kw["do_wgridding"], False)
    d = dft.dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], c["mask"], kw["npix_x"], kw["npix_y"], *args)
    v = dft.dft_dirty2vis(c["uvw"], c["freq"], c["x"], *args)
    v[c["mask"] == 0] = 0
    d.setflags(write=False)
    v.setflags(write=False)
    return d, v


def against_dft(c, dirty, vis):
    d, v = dft_reference(c.geom)
    return rel(dirty, d), rel(vis, v)


def choose(c):
    """oracle.wgridder.choose_params forced to the case's row and w-scheme"""
    from oracle import wgridder as owg

    i, kw = inputs(c.geom), geometry(c.geom)
    return owg.choose_params(i["uvw"], i["freq"], i["mask"], kw["npix_x"], kw["npix_y"], kw["pixsize_x"], kw["pixsize_y"], 0.0, 0.0,
                             kw["epsilon"], kw["do_wgridding"], False, True, False, **forcing(c))


def restatement(c, params=None):
    """the CPU restatement of the algorithm (oracle.wgridder.Plan): with a plan's own parameters, or forced to the case's row"""
    from oracle import wgridder as owg

    i, kw = inputs(c.geom), geometry(c.geom)
    return owg.Plan(i["uvw"], i["freq"], i["mask"], kw["npix_x"], kw["npix_y"], kw["pixsize_x"], kw["pixsize_y"], kw["center_x"],
                    kw["center_y"], kw["epsilon"], kw["flip_u"], kw["flip_v"], kw["flip_w"], kw["do_wgridding"], kw["divide_by_n"],
                    params=params, **({} if params is not None else forcing(c)))


def regimes(iu0, iv0, n, W):
    """of a bin map: first taps per tile, on local cell 31, footprints across the grid edge, in the last, partial tile"""
    iu, iv = np.mod(iu0, n), np.mod(iv0, n)
    nt = -(-n // TILE)
    lu, lv = iu % TILE, iv % TILE
    return {"most in a tile": int(np.bincount((iu // TILE) * nt + iv // TILE).max()),
            "last cell u": int(np.count_nonzero(lu == 31)), "last cell v": int(np.count_nonzero(lv == 31)),
            "corner first taps": int(np.count_nonzero((lu == 31) & (lv == 31))),
            "wrap u": int(np.count_nonzero(iu + W > n)), "wrap v": int(np.count_nonzero(iv + W > n)),
            "in the partial tile": int(np.count_nonzero((iu // TILE == nt - 1) | (iv // TILE == nt - 1))) if n % TILE else 0}
