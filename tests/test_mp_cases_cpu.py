"""CPU guard of tests/test_gpu_mp_instantiations.py: its case table (tests/_mp_cases.py) reaches every multi-plane device function
the launchers build in every launch shape a plan can give it, every geometry gives the plane count the table claims for it, and
the bound the GPU is held to against the direct DFT -- max(epsilon, eps_sup) of the forced kernel row -- leaves the CPU restatement
of the algorithm a factor 2 of room."""

import numpy as np
import pytest

from tests import _mp_cases as mc

GUARD_SUPPORTS = (4, 7, 10, 13, 16)


def test_table_covers_every_built_instantiation():
    """with_W x with_KP for the walk scatter and the walk gather, twice that for the row-walk gather (accumulating; writing the
    scatter's values), and with_W x with_BC x {KP planes on blk_threads(KP) threads, KP planes on blk_threads(KP_MAX) threads} for the
    two register-frame scatters: a support, plane count or block edge added to csrc/dispatch.hpp without a case fails here"""
    built, covered = mc.built(), mc.covered()
    # (13 supports x 4 plane counts: walk scatter, walk gather, two forms of the row-walk gather; 13 + 2 (W, block edge) pairs x
    # 7 (planes, threads) shapes x 2 kernels -- the count pins the parser, not the sources: a wider range changes it with the table)
    assert len(built) == 52 + 52 + 104 + 15 * 7 * 2, len(built)
    # (the 276 device functions of the family: the launch shapes left aside)
    assert len({k[:4] if k[0] in ("grid_blk", "grid_rec") else k[:3] for k in built}) == 13 * 4 * 3 + 15 * 4 * 2
    assert not built - covered, sorted(built - covered)
    assert not covered - built, sorted(covered - built)  # (no case claims a kernel that does not exist)
    assert len({mc.case_id(c) for c in mc.CASES}) == len(mc.CASES)


@pytest.mark.parametrize("W, geom", [(4, "poly2"), (9, "poly3"), (12, "poly4"), (16, "poly2")])
def test_guard_notices_a_missing_case(W, geom):
    """the polynomial geometries of 2 .. 4 planes are the only ones that reach the launch shapes of their plane count"""
    cases = [c for c in mc.CASES if not (c.W == W and c.geom == geom)]
    assert mc.built() - mc.covered(cases)


@pytest.mark.parametrize("W", (5, 14))
@pytest.mark.parametrize("tail", (1, 2, 3))
def test_guard_notices_a_missing_tail(W, tail):
    """(a tail pass comes from a polynomial geometry of 5 .. 7 planes and from one of the ES-kernel stacks: without both the guard fails)"""
    cases = [c for c in mc.CASES if not (c.W == W and mc.nplanes(c) > 4 and mc.nplanes(c) % 4 == tail)]
    assert mc.built() - mc.covered(cases)
    assert not mc.built() - mc.covered([c for c in mc.CASES if not (c.W == W and c.geom == f"poly{4 + tail}" and c.block is None)])


def test_guard_notices_a_missing_block_edge():
    assert mc.built() - mc.covered([c for c in mc.CASES if c.block is None])
    assert mc.built() - mc.covered([c for c in mc.CASES if c.block is not None or c.W != 15])


@pytest.mark.parametrize("old, new", [("with_int<4, 16>(W,", "with_int<4, 17>(W,"), ("with_int<4, 16>(W,", "with_int<3, 16>(W,"),
                                      ("with_int<1, 4>(kp,", "with_int<1, 5>(kp,"), ("(W == 14 || W == 15)", "(W == 13 || W == 14 || W == 15)")])
def test_guard_notices_a_wider_dispatcher(old, new, monkeypatch):
    """a support, a plane count or a block edge added to csrc/dispatch.hpp: the table no longer covers what is built, or the parser
    says what it can no longer restate (planes per pass beyond KP_MAX, supports below it)"""
    read = mc._read

    def edited(name):
        src = read(name)
        if name == "dispatch.hpp":
            assert src.count(old) == 1, old
            src = src.replace(old, new)
        return src

    monkeypatch.setattr(mc, "_read", edited)
    try:
        built = mc.built()
    except AssertionError:
        return
    assert built - mc.covered()


def test_passes():
    assert mc.passes(1) == (1, [1]) and mc.passes(3) == (3, [3]) and mc.passes(4) == (4, [4])
    assert mc.passes(5) == (4, [4, 1]) and mc.passes(7) == (4, [4, 3]) and mc.passes(8) == (4, [4, 4]) and mc.passes(19) == (4, [4] * 4 + [3])
    # the four ES stacks give every tail at every support
    for W in mc.SUPPORTS:
        tails = {mc.nplanes(mc.Case(W, k, None)) % 4 for k in mc.MAIN if mc.GEOMETRIES[k].wmode == 0 and mc.GEOMETRIES[k].do_w}
        assert tails == {0, 1, 2, 3}, (W, tails)


@pytest.mark.parametrize("geom", sorted(mc.GEOMETRIES))
def test_geometry_gives_its_plane_count(geom):
    """oracle.wgridder.choose_params, forced to the row and the w-scheme as the GPU plan is, returns the grid, the w-scheme and the
    plane count the table claims -- at every support (the polynomial count does not depend on it, the ES stack's is W + c)"""
    g = mc.GEOMETRIES[geom]
    for W in mc.SUPPORTS:
        c = mc.Case(W, geom, None)
        p = mc.choose(c)
        assert (p.W, p.wmode, p.nplanes) == (W, g.wmode, mc.nplanes(c)) and abs(p.sigma - mc.SIGMA) < 1e-12, (W, p)
        assert p.nu == p.nv == mc.GRID_EDGE[g.npix], p
        assert 0 < mc.eps_sup(W) < 1e-2 and mc.dft_tolerance(c) == max(g.eps, mc.eps_sup(W))


def test_regimes_of_the_inputs():
    """what tests/test_gpu_mp_instantiations.py asserts of the GPU plan's bin map holds for the restatement's (same mapping)"""
    for c in mc.CASES:
        if c.block is not None:
            continue
        o = mc.restatement(c)
        reg = mc.regimes(o.iu0[o.active], o.iv0[o.active], o.p.nu, c.W)
        if o.p.nu == 192:
            assert reg["most in a tile"] > 16 and reg["last cell u"] > 20 and reg["last cell v"] > 20 and reg["corner first taps"] > 0, (c, reg)
            assert reg["wrap u"] > 0 and reg["wrap v"] > 0, (c, reg)
        if o.p.nu % mc.TILE:
            assert reg["in the partial tile"] > 0, (c, reg)


@pytest.mark.parametrize("c", [mc.Case(W, k, None) for W in GUARD_SUPPORTS for k in mc.GEOMETRIES], ids=mc.case_id)
def test_restatement_against_dft(c):
    """the restatement forced to the case's row is adjoint to 1e-12 and sits a factor 2 inside the bound the GPU is held to, in
    both directions (the measured ratios: docstring of tests/test_gpu_mp_instantiations.py)"""
    i = mc.inputs(c.geom)
    o = mc.restatement(c)
    assert (o.p.wmode, o.p.nplanes, o.p.W) == (mc.GEOMETRIES[c.geom].wmode, mc.nplanes(c), c.W), o.p
    d, v = o.vis2dirty(i["vis"], i["wgt"]), o.dirty2vis(i["x"])
    ed, ev = mc.against_dft(c, d, v)
    tol = mc.dft_tolerance(c)
    print(f"{mc.case_id(c)}: vis2dirty {ed:.3e}, dirty2vis {ev:.3e}, bound {tol:.3e}, ratio {tol / max(ed, ev):.1f}")
    assert 2.0 * max(ed, ev) < tol, (ed, ev, tol)
    assert np.all(v[i["mask"] == 0] == 0)
    y = i["vis"] * i["mask"]
    lhs, rhs = np.vdot(v, y).real, np.vdot(i["x"], o.vis2dirty(y))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
