"""Every one-plane kernel csrc/gridder_wd.hip builds -- k_grid_wd<W, K, BC>, k_degrid_wd<W, K>, k_hess_wd<W, K, BC> for W = 4 .. 16,
K = 2 .. 4 -- in both launch shapes, against the CPU restatement of the algorithm and against the direct DFT.

The case table is tests/_wd_cases.py (its docstring describes the two plan sizes); tests/test_wd_cases_cpu.py fails if the
table misses an instantiation the sources build.  Per case, on one plan forced to the kernel row (1.5, W) in wmode 2:

1. vis2dirty and dirty2vis against the restatement run with the plan's parameters: 1e-10 relative L2, the contract of
   tests/test_gpu_gridder.py (same arithmetic, other summation order);
2. both against the direct DFT at max(epsilon, eps_sup): a forced row skips the plan's admission test, so below W = 11 the
   bound is the row's own worst-position error eps_sup (oracle/es_kernel_table.json), the quantity choose_kernel admits rows on;
3. adjointness of the pair at 1e-10 (tests/test_gpu_fullsize.py);
4. the Hessian apply, with and without beam / eta / wsum, against the composition of the plan's own halves and against the
   restatement's composition, both 1e-10: the second is the check of the fused kernel k_hess_wd that does not go through the
   gather / scatter pair.  Coloured plans whose frame fits a 16-lane row (W + block edge - 1 <= 16) must have run the fused
   kernel (no gather launch in the profile), every other plan the pair; fused plans are rebuilt under PFBHIP_WD_FUSED=0 and held
   to the pair at the 2e-11 of tests/test_gpu_hessian_fused.py;
5. nothing of a Hessian apply carries over: dirty2vis, vis2dirty and hessian after it repeat the ones before it to 1e-12
   (atomic flushes add in no fixed order).

The coloured cases also assert, from the plan's bin map, that the read pipeline of k_hess_wd meets what its regimes differ in
(wd_hess_read_depth: every row in flight for W < 8, depth 8 with refills from W = 8, depth 4 at K = 4, W = 10 .. 12, depth 2 at
K = 4, W >= 13): tiles of more than 16 records (row streams longer than one record, so rows of the next record are requested
while the current one is worked on) and first taps on local cell 31 of both axes (footprints in the last rows / columns of the
48 x 48 tile image).

The restatement alone against the DFT, measured on the CPU with the plan forced to (1.5, W): relative L2 of vis2dirty,
of dirty2vis, the bound max(epsilon, eps_sup), and bound / worse of the two.  Coloured size (every 41st pixel, every 29th row):

     W | K = 2, eps 1e-4, field x 10      | K = 3, eps 1e-7, field x 16      | K = 4, eps 1e-7, field x 30
     4 | 2.4e-03 2.4e-03 7.5e-03    3.1 | 2.4e-03 2.4e-03 7.5e-03    3.1 | 2.4e-03 2.4e-03 7.5e-03    3.1
     5 | 4.0e-04 3.9e-04 1.4e-03    3.4 | 4.1e-04 4.0e-04 1.4e-03    3.4 | 4.0e-04 4.1e-04 1.4e-03    3.4
     6 | 6.8e-05 6.7e-05 2.4e-04    3.6 | 6.9e-05 6.8e-05 2.4e-04    3.5 | 6.8e-05 6.9e-05 2.4e-04    3.6
     7 | 1.2e-05 1.1e-05 1.0e-04    8.4 | 1.2e-05 1.2e-05 4.1e-05    3.4 | 1.2e-05 1.2e-05 4.1e-05    3.4
     8 | 2.1e-06 2.0e-06 1.0e-04   47.7 | 2.0e-06 2.0e-06 6.5e-06    3.3 | 2.0e-06 2.1e-06 6.5e-06    3.1
     9 | 4.8e-07 4.7e-07 1.0e-04  207.2 | 3.4e-07 3.4e-07 1.2e-06    3.5 | 3.4e-07 3.5e-07 1.2e-06    3.4
    10 | 3.3e-07 3.3e-07 1.0e-04  305.0 | 5.9e-08 5.9e-08 2.3e-07    3.8 | 6.2e-08 6.1e-08 2.3e-07    3.7
    11 | 3.2e-07 3.2e-07 1.0e-04  310.1 | 1.0e-08 1.0e-08 1.0e-07    9.6 | 1.1e-08 1.0e-08 1.0e-07    9.5
    12 | 3.2e-07 3.2e-07 1.0e-04  310.3 | 2.2e-09 2.3e-09 1.0e-07   44.0 | 1.8e-09 1.7e-09 1.0e-07   55.2
    13 | 3.2e-07 3.2e-07 1.0e-04  310.2 | 1.4e-09 1.5e-09 1.0e-07   67.5 | 3.3e-10 3.3e-10 1.0e-07  301.7
    14 | 3.2e-07 3.2e-07 1.0e-04  310.2 | 1.4e-09 1.5e-09 1.0e-07   68.8 | 1.2e-10 1.3e-10 1.0e-07  763.6
    15 | 3.2e-07 3.2e-07 1.0e-04  310.2 | 1.4e-09 1.5e-09 1.0e-07   68.9 | 1.1e-10 1.2e-10 1.0e-07  823.1
    16 | 3.2e-07 3.2e-07 1.0e-04  310.2 | 1.4e-09 1.5e-09 1.0e-07   68.9 | 1.1e-10 1.2e-10 1.0e-07  825.3

(kernel error up to W = 10, the interpolation error of the K functions in w above.)  The small size (all pixels, all
visibilities) sits between 2.8 and 3.4 below the bound up to W = 10 and further above; tests/test_wd_cases_cpu.py holds every
small case a factor 2 inside the bound on every machine.

test_multi_plane_frames_below_13 gives the register-frame scatters of the multi-plane schemes (k_grid_blk, k_grid_rec) the
supports W = 4 .. 12 that test_multi_plane_scatter_frames (tests/test_gpu_gridder.py, W = 13 .. 16) leaves to the plan's choice.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pfb_imaging_amd.utils import synth  # noqa: E402
from tests import _wd_cases as wc  # noqa: E402
from tests._wd_cases import rel  # noqa: E402

TOL_RESTATEMENT = 1e-10  # GPU against the CPU restatement and against its own composition (tests/test_gpu_gridder.py)
TOL_ADJOINT = 1e-10  # (tests/test_gpu_fullsize.py)
TOL_FUSED_PAIR = 2e-11  # (tests/test_gpu_hessian_fused.py)
TOL_REPEAT = 1e-12
BEAM_ARGS = dict(eta=0.3, wsum=7.0)


def gpu_plan(c):
    from pfb_imaging_amd.wgridder import Gridder

    i = wc.inputs(c.size)
    g = Gridder(i["uvw"], i["freq"], i["mask"], force=(wc.SIGMA, c.W), force_wmode=2, **wc.geometry(c))
    g.set_weights(i["wgt"])
    return g


def check_plan(c, info):
    """the case runs the instantiation it claims"""
    assert info["wmode"] == 2 and info["nplanes"] == 1 and info["gather_mode"] == 2, info
    assert info["W"] == c.W and info["nderiv"] == c.K and abs(info["sigma"] - wc.SIGMA) < 1e-12, info
    assert info["scatter_launches"] == wc.SIZES[c.size][7], info
    assert info["scatter_block"] == wc.block_edge(c), info
    if c.size == "coloured":
        assert info["nu"] == 768 and info["nv"] == 768, info  # (whole tile pairs: what the colour launches need)


def check_pipeline_regimes(g, c):
    """tiles of more than 16 records and first taps on the last local cell of both axes (see the module docstring)"""
    bm, nu, nv = g.binmap(), g.info["nu"], g.info["nv"]
    on = wc.inputs(c.size)["mask"].ravel() != 0
    iu, iv = np.mod(bm["iu0"][on], nu), np.mod(bm["iv0"][on], nv)
    per_tile = np.bincount((iu // 32) * (nv // 32 + 1) + iv // 32)
    assert per_tile.max() > 16, per_tile.max()
    lu, lv = iu % 32, iv % 32
    assert np.count_nonzero(lu == 31) > 100 and np.count_nonzero(lv == 31) > 100
    assert np.count_nonzero((lu == 31) & (lv == 31)) > 0


def hessians(g, x, beam):
    """the Hessian apply with and without beam / eta / wsum, and the number of gather launches the two made"""
    g.profile(True)
    g.profile_get(reset=True)
    hb = g.hessian(x, beam=beam, **BEAM_ARGS)
    h = g.hessian(x)
    gathers = g.profile_get(reset=True)["degrid"][1]
    g.profile(False)
    return hb, h, gathers


@pytest.mark.parametrize("c", wc.ONE_PLANE_CASES, ids=wc.case_id)
def test_one_plane_instantiation(c, monkeypatch):
    i = wc.inputs(c.size)
    x, vis, wgt = i["x"], i["vis"], i["wgt"]
    for name, val in (("PFBHIP_WD_COLOURS", "1" if c.size == "coloured" else None), ("PFBHIP_WD_BLOCK", None if c.block is None else str(c.block)),
                      ("PFBHIP_WD_FUSED", None), ("PFBHIP_WMODE2", None)):
        monkeypatch.delenv(name, raising=False) if val is None else monkeypatch.setenv(name, val)
    g = gpu_plan(c)
    info = dict(g.info)
    check_plan(c, info)
    if c.size == "coloured":
        check_pipeline_regimes(g, c)
    o = wc.restatement(c, params=g.oracle_params())
    beam = 0.5 + np.random.default_rng(2).random(x.shape)
    fig = {}

    # 1, 2: the two halves
    d, v = g.vis2dirty(vis, wgt), g.dirty2vis(x)
    fig["scatter / restatement"] = rel(d, o.vis2dirty(vis, wgt)), TOL_RESTATEMENT
    fig["gather / restatement"] = rel(v, o.dirty2vis(x)), TOL_RESTATEMENT
    ed, ev = wc.against_dft(c, d, v)
    fig["scatter / DFT"] = ed, wc.dft_tolerance(c)
    fig["gather / DFT"] = ev, wc.dft_tolerance(c)
    assert np.all(v[i["mask"] == 0] == 0)
    # 3: adjointness
    y = vis * i["mask"]
    lhs, rhs = np.vdot(v, y).real, np.vdot(x, g.vis2dirty(y))
    fig["adjointness"] = abs(lhs - rhs) / max(abs(lhs), abs(rhs)), TOL_ADJOINT
    # 4: the Hessian apply
    hb, h, gathers = hessians(g, x, beam)
    fig["hessian(beam, eta, wsum) / own halves"] = rel(hb, beam * g.vis2dirty(g.dirty2vis(beam * x), wgt) / BEAM_ARGS["wsum"] +
                                                       BEAM_ARGS["eta"] * x), TOL_RESTATEMENT
    fig["hessian / own halves"] = rel(h, g.vis2dirty(v, wgt)), TOL_RESTATEMENT
    fig["hessian(beam, eta, wsum) / restatement"] = rel(hb, beam * o.vis2dirty(o.dirty2vis(beam * x), wgt) / BEAM_ARGS["wsum"] +
                                                        BEAM_ARGS["eta"] * x), TOL_RESTATEMENT
    fig["hessian / restatement"] = rel(h, o.vis2dirty(o.dirty2vis(x), wgt)), TOL_RESTATEMENT
    # 5: nothing carries over
    fig["dirty2vis repeated"] = rel(g.dirty2vis(x), v), TOL_REPEAT
    fig["vis2dirty repeated"] = rel(g.vis2dirty(vis, wgt), d), TOL_REPEAT
    hb1, h1, gathers1 = hessians(g, x, beam)
    fig["hessian(beam, eta, wsum) repeated"] = rel(hb1, hb), TOL_REPEAT
    fig["hessian repeated"] = rel(h1, h), TOL_REPEAT
    g.close()
    fused = wc.runs_fused(c)
    if fused:
        monkeypatch.setenv("PFBHIP_WD_FUSED", "0")
        g = gpu_plan(c)
        check_plan(c, g.info)
        pb, p, gathers0 = hessians(g, x, beam)
        g.close()
        fig["fused / pair (beam, eta, wsum)"] = rel(hb, pb), TOL_FUSED_PAIR
        fig["fused / pair"] = rel(h, p), TOL_FUSED_PAIR

    for k, (val, tol) in fig.items():
        print(f"{wc.case_id(c)}: {k}: {val:.3e} (bound {tol:.3e})")
    # fused: no gather launch in any apply; the pair: gather launches in every one
    assert (gathers == 0) == fused and (gathers1 == 0) == fused, (info, gathers, gathers1)
    if fused:
        assert gathers0 > 0, gathers0
    bad = {k: f for k, f in fig.items() if not f[0] < f[1]}
    assert not bad, (wc.case_id(c), bad)


@pytest.mark.parametrize("W", wc.MULTI_PLANE_SUPPORTS)
@pytest.mark.parametrize("mode", wc.MULTI_PLANE_MODES)
@pytest.mark.parametrize("wmode, widen, zscale", wc.MULTI_PLANE_GEOMETRIES)
def test_multi_plane_frames_below_13(W, mode, wmode, widen, zscale, monkeypatch):
    """k_grid_blk (PFBHIP_SCATTER=block) and k_grid_rec (rec_es) -- csrc/gridder_kernels_mp.hpp, 16 x 16 cells on 4 x 16 lanes -- at the
    supports below those of test_multi_plane_scatter_frames, with its inputs: an ES-kernel plane stack (wmode 0) and polynomial
    planes in one pass (wmode 1), forced to the row (1.5, W), against the restatement run with the plan's parameters."""
    from oracle import wgridder as owg
    from pfb_imaging_amd.wgridder import Gridder

    c = synth.make_case(3000, 2, 256, zscale=zscale, seed=1)
    cell = c["cell"] * widen
    monkeypatch.setenv("PFBHIP_WMODE2", "0")
    monkeypatch.setenv("PFBHIP_SCATTER", mode)
    monkeypatch.delenv("PFBHIP_WD_BLOCK", raising=False)
    kw = dict(npix_x=256, npix_y=256, pixsize_x=cell, pixsize_y=cell, center_x=0.0, center_y=0.0, epsilon=1e-7, flip_u=False, flip_v=True,
              flip_w=False, do_wgridding=True, divide_by_n=False)
    g = Gridder(c["uvw"], c["freq"], c["mask"], force=(wc.SIGMA, W), force_wmode=wmode, **kw)
    info = dict(g.info)
    assert info["wmode"] == wmode and info["W"] == W and abs(info["sigma"] - wc.SIGMA) < 1e-12, info
    assert (info["nplanes"] > 4) == (wmode == 0), info
    assert info["scatter_block"] == 4 and info["scatter_mode"] == (1 if mode == "block" else 2), info
    o = owg.Plan(c["uvw"], c["freq"], c["mask"], 256, 256, cell, cell, 0.0, 0.0, 1e-7, False, True, False, True, False,
                 params=g.oracle_params())
    d, v = g.vis2dirty(c["vis"], c["wgt"]), g.dirty2vis(c["x"])
    g.set_weights(c["wgt"])
    h = g.hessian(c["x"], eta=0.1, wsum=3.0)
    g.close()
    fig = {"scatter / restatement": rel(d, o.vis2dirty(c["vis"], c["wgt"])), "gather / restatement": rel(v, o.dirty2vis(c["x"])),
           "hessian / restatement": rel(h, o.vis2dirty(o.dirty2vis(c["x"]), c["wgt"]) / 3.0 + 0.1 * c["x"])}
    for k, val in fig.items():
        print(f"W = {W}, {mode}, wmode {wmode}: {k}: {val:.3e}")
    bad = {k: val for k, val in fig.items() if not val < TOL_RESTATEMENT}
    assert not bad, bad
