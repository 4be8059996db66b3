"""Every multi-plane kernel launch_grid / launch_degrid (csrc/gridder.hip) build from csrc/gridder_kernels_mp.hpp -- k_grid_mp<W, KP>,
k_grid_blk<W, KP, BC>, k_grid_rec<W, KP, BC>, k_degrid_mp<W, KP>, k_degrid_rw<W, KP> for W = 4 .. 16, KP = 1 .. 4 -- in every launch
shape a plan can give it, against the CPU restatement of the algorithm and against the direct DFT.

The case table is tests/_mp_cases.py (its docstring describes what it crosses); tests/test_mp_cases_cpu.py fails if the table
misses an instantiation the sources build or a geometry stops giving its plane count.  Per case, for each scatter form
(PFBHIP_SCATTER = walk, block, rec / rec_es) on one plan forced to the kernel row (1.5, W) and the case's w-scheme, PFBHIP_WMODE2=0:

1. the plan runs what the table claims: W, sigma, wmode, nplanes, scatter_mode, scatter_block, scatter_launches, gather_mode, and the
   launch counts of one vis2dirty, one dirty2vis and one Hessian apply (passes x launches per pass; passes for the gather);
2. vis2dirty and dirty2vis against the restatement run with the plan's parameters: 1e-10 relative L2, the contract of
   tests/test_gpu_gridder.py (same arithmetic, other summation order); both against the direct DFT at max(epsilon, eps_sup) (a forced
   row skips the plan's admission test: tests/_wd_cases.py, dft_tolerance); masked visibilities exactly zero;
3. adjointness of the pair at 1e-10;
4. the Hessian apply, with and without beam / eta / wsum, against the composition of the plan's own halves and against the
   restatement's composition, both 1e-10 -- on single-pass record plans the check of k_degrid_rw's epilogue that writes the
   scatter's values (ApplyState::gather_values);
5. nothing of a Hessian apply carries over: dirty2vis, vis2dirty and hessian after it repeat the ones before it to 1e-12 (single-pass
   plans clear the second plane buffer on a side stream, multi-pass plans reuse one buffer);
6. the forms agree with each other at 1e-10 (summation order only).

From the plan's bin map the 192-grid cases also assert what the kernels' edges need: tiles of more than 16 visibilities, first taps
on local cell 31 of both axes (footprints in the halo) and footprints across the grid edge on both axes; the 180-grid cases
visibilities in the partial last tile.

The restatement alone against the DFT, measured on the CPU with the plan forced to (1.5, W): bound max(epsilon, eps_sup) over the
worse of the two directions' relative L2 (tests/test_mp_cases_cpu.py prints both and holds every one of these a factor 2 inside):

     W | poly1  poly2  poly3  poly4  poly5  poly6  poly7   flat | es+0  es+1  es+2  es+3 | odd3  odd5 part3 part5
     4 |   3.1    3.1    3.1    3.1    3.1    3.1    3.2    3.1 |  2.6   2.7   2.7   2.7 |  3.2   3.2   3.2   3.2
     7 |   9.9    3.5    3.5    3.5    3.4    3.4    3.5    3.5 |  2.9   3.0   3.0   2.9 |  3.6   3.6   3.4   3.4
    10 |  10.0    164    3.7    3.7    3.7    3.7    3.7    3.7 |  3.1   3.1   3.2   3.2 |  4.0   3.9   3.7   3.7
    13 |  10.0   1880    333    4.8    4.9    4.9    4.9    334 |  284   285   288   288 |  374   5.2   347   4.9
    16 |  10.0   1884   3232   75.5   42.1   76.1   77.1  75509 | 6e4   6e4   6e4   6e4  | 9837  72.2  4754  61.6

(the kernel row's error where the ratio is 3 .. 5, epsilon's share of the plane interpolation or nothing but rounding above.)

Measured on the MI355X: 182 cases in 31 s (0.15 .. 0.8 s each); worst figure over its bound 4e-3 against the restatement (4.0e-13,
W = 16, ES stack of 16 planes), 0.16 for the repeats (1.6e-13, walk scatter: atomics add in no fixed order), 0.38 against the DFT
(W = 4, ES stack: the row's own error).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import _mp_cases as mc  # noqa: E402
from tests._mp_cases import rel  # noqa: E402

TOL_RESTATEMENT = 1e-10  # GPU against the CPU restatement, against its own composition and between the forms (tests/test_gpu_gridder.py)
TOL_ADJOINT = 1e-10  # (tests/test_gpu_fullsize.py)
TOL_REPEAT = 1e-12
BEAM_ARGS = dict(eta=0.3, wsum=7.0)
SWITCHES = ("PFBHIP_SCATTER", "PFBHIP_WD_BLOCK", "PFBHIP_WMODE2", "PFBHIP_WD_COLOURS", "PFBHIP_WD_FUSED", "PFBHIP_ROWFFT", "PFBHIP_FUSED_FFT",
            "PFBHIP_FUSED_DOUBLED", "PFBHIP_SEPSCREEN", "PFBHIP_TFFT")


def gpu_plan(c, form, monkeypatch):
    from pfb_imaging_amd.wgridder import Gridder

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PFBHIP_WMODE2", "0")
    monkeypatch.setenv("PFBHIP_SCATTER", form)
    if c.block is not None:
        monkeypatch.setenv("PFBHIP_WD_BLOCK", str(c.block))
    i = mc.inputs(c.geom)
    g = Gridder(i["uvw"], i["freq"], i["mask"], **mc.forcing(c), **mc.geometry(c.geom))
    g.set_weights(i["wgt"])
    return g


def check_plan(c, form, info):
    """the case runs the instantiation it claims"""
    geo = mc.GEOMETRIES[c.geom]
    edge = mc.GRID_EDGE[geo.npix]
    assert info["W"] == c.W and abs(info["sigma"] - mc.SIGMA) < 1e-12 and info["nu"] == edge and info["nv"] == edge, info
    assert info["wmode"] == geo.wmode and info["nplanes"] == mc.nplanes(c), info
    assert info["scatter_mode"] == mc.SCATTER_MODE[form] and info["scatter_block"] == mc.block_edge(c, form), (form, info)
    assert info["scatter_launches"] == mc.launches(c, form), (form, info)
    assert info["gather_mode"] == (1 if mc.row_walk(c) else 0), info


def check_regimes(g, c):
    geo = mc.GEOMETRIES[c.geom]
    bm = g.binmap()
    on = mc.inputs(c.geom)["mask"].ravel() != 0
    reg = mc.regimes(bm["iu0"][on], bm["iv0"][on], g.info["nu"], c.W)
    if geo.npix == 128:
        assert reg["most in a tile"] > 16 and reg["last cell u"] > 20 and reg["last cell v"] > 20 and reg["corner first taps"] > 0, reg
        assert reg["wrap u"] > 0 and reg["wrap v"] > 0, reg
    if mc.GRID_EDGE[geo.npix] % mc.TILE:
        assert reg["in the partial tile"] > 0, reg


def counted(g, fn):
    """fn() and the (scatter, gather) launches it made"""
    g.profile_get(reset=True)
    out = fn()
    p = g.profile_get(reset=True)
    return out, (p["grid"][1], p["degrid"][1])


def hessian_refs(o, x, vis, wgt, beam):
    """the restatement's halves and compositions, once per (W, geometry)"""
    d, v = o.vis2dirty(vis, wgt), o.dirty2vis(x)
    hb = beam * o.vis2dirty(o.dirty2vis(beam * x), wgt) / BEAM_ARGS["wsum"] + BEAM_ARGS["eta"] * x
    return d, v, hb, o.vis2dirty(v, wgt)


@pytest.mark.parametrize("c", mc.CASES, ids=mc.case_id)
def test_multi_plane_instantiation(c, monkeypatch):
    i = mc.inputs(c.geom)
    x, vis, wgt, mask = i["x"], i["vis"], i["wgt"], i["mask"]
    beam = 0.5 + np.random.default_rng(2).random(x.shape)
    y = vis * mask
    npass = len(mc.passes(mc.nplanes(c))[1])
    fig, counts, params, ref, first = {}, {}, None, None, None

    for form in mc.forms(c):
        g = gpu_plan(c, form, monkeypatch)
        info = dict(g.info)
        check_plan(c, form, info)
        if params is None:
            check_regimes(g, c)
            params = g.oracle_params()
            ref = hessian_refs(mc.restatement(c, params=params), x, vis, wgt, beam)
        assert g.oracle_params() == params, (form, g.oracle_params(), params)
        od, ov, ohb, oh = ref
        f = lambda name: f"{form}: {name}"  # noqa: E731

        # 1: launch counts; 2: the two halves
        g.profile(True)
        d, n_d = counted(g, lambda: g.vis2dirty(vis, wgt))
        v, n_v = counted(g, lambda: g.dirty2vis(x))
        hb, n_h = counted(g, lambda: g.hessian(x, beam=beam, **BEAM_ARGS))
        g.profile(False)
        ngrid = npass * mc.launches(c, form)
        counts[form] = ((n_d, n_v, n_h), ((ngrid, 0), (0, npass), (ngrid, npass)))
        h = g.hessian(x)
        fig[f("scatter / restatement")] = rel(d, od), TOL_RESTATEMENT
        fig[f("gather / restatement")] = rel(v, ov), TOL_RESTATEMENT
        ed, ev = mc.against_dft(c, d, v)
        fig[f("scatter / DFT")] = ed, mc.dft_tolerance(c)
        fig[f("gather / DFT")] = ev, mc.dft_tolerance(c)
        assert np.all(v[mask == 0] == 0), form
        # 3: adjointness
        lhs, rhs = np.vdot(v, y).real, np.vdot(x, g.vis2dirty(y))
        fig[f("adjointness")] = abs(lhs - rhs) / max(abs(lhs), abs(rhs)), TOL_ADJOINT
        # 4: the Hessian apply
        fig[f("hessian(beam, eta, wsum) / own halves")] = rel(hb, beam * g.vis2dirty(g.dirty2vis(beam * x), wgt) / BEAM_ARGS["wsum"] +
                                                               BEAM_ARGS["eta"] * x), TOL_RESTATEMENT
        fig[f("hessian / own halves")] = rel(h, g.vis2dirty(v, wgt)), TOL_RESTATEMENT
        fig[f("hessian(beam, eta, wsum) / restatement")] = rel(hb, ohb), TOL_RESTATEMENT
        fig[f("hessian / restatement")] = rel(h, oh), TOL_RESTATEMENT
        # 5: nothing carries over
        fig[f("dirty2vis repeated")] = rel(g.dirty2vis(x), v), TOL_REPEAT
        fig[f("vis2dirty repeated")] = rel(g.vis2dirty(vis, wgt), d), TOL_REPEAT
        fig[f("hessian(beam, eta, wsum) repeated")] = rel(g.hessian(x, beam=beam, **BEAM_ARGS), hb), TOL_REPEAT
        fig[f("hessian repeated")] = rel(g.hessian(x), h), TOL_REPEAT
        g.close()
        # 6: the forms agree
        if first is None:
            first = (form, d, v, hb, h)
        else:
            for name, a, b in zip(("vis2dirty", "dirty2vis", "hessian(beam, eta, wsum)", "hessian"), (d, v, hb, h), first[1:]):
                fig[f(f"{name} / {first[0]}")] = rel(a, b), TOL_RESTATEMENT

    for k, (val, tol) in fig.items():
        print(f"{mc.case_id(c)}: {k}: {val:.3e} (bound {tol:.3e})")
    for form, (got, want) in counts.items():
        print(f"{mc.case_id(c)}: {form}: (scatter, gather) launches of vis2dirty, dirty2vis, hessian: {got} (expected {want})")
    wrong = {form: gw for form, gw in counts.items() if gw[0] != gw[1]}
    assert not wrong, (mc.case_id(c), wrong)
    bad = {k: f for k, f in fig.items() if not f[0] < f[1]}
    assert not bad, (mc.case_id(c), bad)
