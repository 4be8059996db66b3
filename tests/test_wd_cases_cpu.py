"""CPU guard of tests/test_gpu_wd_instantiations.py: its case table (tests/_wd_cases.py) reaches every one-plane device function
the sources build, and the bound its cases hold the GPU to against the direct DFT -- max(epsilon, eps_sup) of the forced kernel
row -- leaves the CPU restatement of the algorithm a factor 2 of room at the small size (each case well under a second)."""

import re

import numpy as np
import pytest

from tests import _wd_cases as wc


def test_table_covers_every_built_instantiation():
    """with_W x with_K x with_BC for the scatter, with_W x with_K for the gather, each in both launch shapes, and every
    k_hess_wd<W, K, BC> that wd_launch_hessian builds: a support, term count or block edge added to csrc/dispatch.hpp or
    csrc/gridder_wd.hip without a case fails here"""
    built, covered = wc.built(), wc.covered()
    # (13 supports x 3 term counts: scatter and gather in two launch shapes, the BC = 2 scatters of W = 14, 15 beside the BC = 4 ones,
    # the fused kernel up to W = 15 -- the count pins the parser, not the sources: a wider range must change it together with the table)
    assert len(built) == 2 * (39 + 6) + 2 * 39 + 36, len(built)
    assert not built - covered, sorted(built - covered)
    assert not covered - built, sorted(covered - built)  # (no case claims a kernel that does not exist)
    assert len({wc.case_id(c) for c in wc.ONE_PLANE_CASES}) == len(wc.ONE_PLANE_CASES)


@pytest.mark.parametrize("size", sorted(wc.SIZES))
@pytest.mark.parametrize("W, K", [(4, 2), (9, 3), (12, 4), (16, 4)])
def test_guard_notices_a_missing_pair(size, W, K):
    cases = [c for c in wc.ONE_PLANE_CASES if not (c.size == size and c.W == W and c.K == K)]
    assert wc.built() - wc.covered(cases)


def test_multi_plane_supports_join_the_pinned_ones():
    """test_multi_plane_frames_below_13 and test_multi_plane_scatter_frames (tests/test_gpu_gridder.py) between them pin every
    support of with_W"""
    with open(wc.ROOT + "/tests/test_gpu_gridder.py") as f:
        m = re.search(r'parametrize\("W, sigma", (\[[^\]]*\])\)\n@pytest[^\n]*\ndef test_multi_plane_scatter_frames', f.read())
    assert m
    pinned = {int(w) for w, _ in re.findall(r"\((\d+), ([\d.]+)\)", m.group(1))}
    assert pinned | set(wc.MULTI_PLANE_SUPPORTS) == set(wc._int_range(wc._read("dispatch.hpp"), "with_W"))


def test_every_case_has_its_row_and_bound():
    for c in wc.ONE_PLANE_CASES:
        assert 0 < wc.eps_sup(c.W) < 1e-2
        assert wc.dft_tolerance(c) == max(c.eps, wc.eps_sup(c.W))


@pytest.mark.parametrize("c", [c for c in wc.ONE_PLANE_CASES if c.size == "small" and c.block is None], ids=wc.case_id)
def test_restatement_against_dft_small(c):
    """the restatement forced to the case's row lands on the case's (W, K), is adjoint to 1e-12 and sits a factor 2 inside the
    bound the GPU is held to, in both directions (measured: 2.8 .. 3.4 below it up to W = 10, 8 and more above)"""
    i = wc.inputs(c.size)
    o = wc.restatement(c)
    assert (o.p.wmode, o.p.nplanes, o.p.W, o.p.nderiv) == (2, 1, c.W, c.K) and abs(o.p.sigma - wc.SIGMA) < 1e-12, o.p
    d, v = o.vis2dirty(i["vis"], i["wgt"]), o.dirty2vis(i["x"])
    ed, ev = wc.against_dft(c, d, v)
    print(f"{wc.case_id(c)}: vis2dirty {ed:.3e}, dirty2vis {ev:.3e}, bound {wc.dft_tolerance(c):.3e}")
    assert 2.0 * max(ed, ev) < wc.dft_tolerance(c), (ed, ev, wc.dft_tolerance(c))
    y = i["vis"] * i["mask"]
    lhs, rhs = np.vdot(v, y).real, np.vdot(i["x"], o.vis2dirty(y))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
