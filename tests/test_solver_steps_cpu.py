"""What lets tests/test_gpu_solver_steps.py mean something, checked on the yardstick alone: the one-iteration functions of
tests/_step_cases.py are the loops of tests/_fb_ref.py / tests/_pd_ref.py bit for bit; the case table reaches every built
instantiation, every fallback and every second trip it claims to (sizes read from the sources); and every case's inputs make
the threshold, the positivity step and its band coupling do something in each iteration that is compared -- away from the one
discontinuity of the loop, positivity mode 2 at zero."""

import collections
import functools
import os
import re

import numpy as np
import pytest

from oracle import psi as opsi
from tests import _step_cases as sc
from tests._fb_ref import fb_ref
from tests._pd_ref import pd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pfb-imaging_amd", "csrc")
IDS = [c.id for c in sc.CASES]


def _niter(case):
    return 1 if case.id in sc.BIG else 3


@functools.lru_cache(maxsize=None)
def _records(cid):
    """Computed once per case and shared (read-only) by the tests below; the arrays of the large cases are dropped."""
    case = sc.BY_ID[cid]
    p = sc.problem(case)
    recs = sc.run_ref(p, _niter(case))
    st = [sc.stats(p, r) for r in recs]
    zeros = [int((r["pre"] == 0.0).sum()) for r in recs]
    last = recs[-1]
    keep = dict(x=last["x"], eps=last["eps"], v=last.get("v"))
    return st, zeros, keep


def _const(path, name):
    m = re.search(r"constexpr int " + name + r" = (\d+);", open(os.path.join(CSRC, path)).read())
    assert m, name
    return int(m.group(1))


# ---- the one-step functions are the yardsticks --------------------------------------------------------------------------


@pytest.mark.parametrize("cid", IDS)
def test_chained_steps_are_the_reference_loop(cid):
    case = sc.BY_ID[cid]
    p = sc.problem(case)
    k = _niter(case)
    _, _, got = _records(cid)
    if case.solver == "fb":
        w = p.weight
        x, kr, eps, _ = fb_ref(p.x0, case.lam, p.psi, w, p.href, p.xtilde, 1.0, p.step, case.nu, 0.0, k, case.pos, case.accel,
                               case.reg == "l1")
    else:
        v0 = np.zeros((case.nband, p.psi.nbasis, p.psi.nxmax, p.psi.nymax))
        x, v, kr, eps, _, _ = pd_ref(p.x0, v0, case.lam, p.psi, p.weight, p.href, p.xtilde, sc.GAMMA_PD, p.sigma, p.tau, 0.0, k,
                                     case.pos)
        assert np.array_equal(got["v"], v)
    assert kr == k - 1
    assert np.array_equal(got["x"], x) and got["eps"] == eps


# ---- the table ------------------------------------------------------------------------------------------------------------


def test_geometries():
    """Cube and pixel-count parities as tests/_step_cases.py claims them, from the oracle's bookkeeping."""
    e = opsi.Psi(1, *sc.SMALL, sc.DICTS["E"], sc.NLEVEL)
    o = opsi.Psi(1, *sc.SMALL, sc.DICTS["O"], sc.NLEVEL)
    s = opsi.Psi(1, *sc.SMALL, sc.DICTS["S"], sc.NLEVEL)
    assert e.nbasis * e.nxmax * e.nymax == 960 and o.nbasis * o.nxmax * o.nymax == 2175
    assert (s.nbasis, s.nxmax, s.nymax) == (1,) + sc.SMALL
    assert sc.SMALL[0] * sc.SMALL[1] % 2 == 0 and sc.SMALL_ODD[0] * sc.SMALL_ODD[1] % 2 == 1
    # two padded geometries for the small cases -- one plan size --, row-FFT sizes for the rest
    small = [c for c in sc.CASES if c.group != "e"]
    assert {c.pad for c in small} == {sc.SMALL_PAD} and {c.img for c in small} == {sc.SMALL, sc.SMALL_ODD}
    assert all(c.img[0] <= c.pad[0] and c.img[1] <= c.pad[1] for c in sc.CASES)
    assert {c.pad for c in sc.CASES if c.group == "e"} == {(1024, 1024), (2048, 2048)}
    assert len(sc.BIG) == 3 and all((c.ks == (1, 3)) == (c.id in sc.BIG) and c.ks in ((1, 3), (1, 2, 3)) for c in sc.CASES)


def test_table_reaches_every_kernel():
    maxb = _const("devloop.hpp", "LOOP_MAXB")
    assert maxb == sc.MAXB
    by_kernel = collections.defaultdict(list)
    for c in sc.CASES:
        for k in sc.kernels(c, maxb):
            by_kernel[k].append(c)
    # the three template families, NB = 1..16; the shrink and the identity step with l21 (the band sum) for every NB
    for nb in range(1, maxb + 1):
        for name in (f"k_fb_shrink<{nb}>", f"k_fb_step<{nb},false>", f"k_fb_step<{nb},true>"):
            assert by_kernel[name], name
        assert any(c.reg == "l21" for c in by_kernel[f"k_fb_shrink<{nb}>"])
        assert any(c.reg == "l21" for c in by_kernel[f"k_fb_step<{nb},true>"])
    # groups a and b run nothing but the templates
    for c in sc.CASES:
        if c.group == "a":
            assert sc.kernels(c, maxb) == {f"k_fb_shrink<{c.nband}>", f"k_fb_step<{c.nband},false>"}
        if c.group == "b":
            assert sc.kernels(c, maxb) == {f"k_fb_step<{c.nband},true>"}
    for group in "ab":
        cs = [c for c in sc.CASES if c.group == group]
        pairs = collections.Counter((c.pos, c.reg) for c in cs)
        assert all(pairs[(pos, reg)] >= 2 for pos in (0, 1, 2) for reg in ("l21", "l1")), pairs
        assert {c.accel for c in cs} == {True, False}
    assert {1.0, 1.25} <= {c.nu for c in sc.CASES if c.group == "b"}
    # every fallback at one band more than the templates hold, and at the mixed paths
    for name in ("k_fb_bandsum", "k_fb_shrink_gen", "k_fb_step_gen", "k_fb_flag", "k_pd_primal", "k_pd_norms", "k_positivity"):
        assert any(c.nband == maxb + 1 for c in by_kernel[name]), name
    mixed = [c for c in sc.CASES if c.dic == "O" and c.nband <= maxb]
    assert {c.nband for c in mixed if c.solver == "fb"} == {1, maxb}
    assert all(sc.kernels(c, maxb) >= {"k_fb_shrink_gen", f"k_fb_step<{c.nband},false>"} for c in mixed if c.solver == "fb")
    odd = [c for c in sc.CASES if c.img == sc.SMALL_ODD]
    assert {(c.nband, c.pos, c.reg) for c in odd} == {(n, p, r) for n in (1, 2, maxb) for p in (0, 1, 2) for r in ("l21", "l1")}
    assert all(sc.kernels(c, maxb) >= {"k_fb_shrink_gen", "k_fb_step_gen"} for c in odd)
    assert any(c.reg == "l1" for c in by_kernel["k_fb_shrink_gen"]) and any(not c.accel for c in by_kernel["k_fb_step_gen"])
    # "<= 0" against "< 0" in positivity 2 shows only where a band is exactly 0 beside positive ones: l1 over the identity at nu = 1
    for name in ("k_fb_flag", "k_fb_step<10,true>"):
        assert any(c.reg == "l1" and c.pos == 2 and c.nu == 1.0 and c.nband > 1 for c in by_kernel[name]), name
    seventeen = [c for c in sc.CASES if c.group == "c" and c.nband == maxb + 1]
    assert {c.dic for c in seventeen} == {"E", "I"} and {c.pos for c in seventeen} == {1, 2}
    assert any(not c.accel for c in seventeen) and any(c.reg == "l1" for c in seventeen)
    # primal-dual: both dictionaries, the last count of k_pd_step and the two after it, both layouts on each branch
    d = [c for c in sc.CASES if c.group == "d"]
    assert {(c.dic, c.nband, c.pos) for c in d} == {(x, n, p) for x in "EO" for n in (1, 2, maxb, maxb + 1, maxb + 2)
                                                    for p in (0, 1, 2)}
    for branch in ("k_pd_step", "k_pd_norms"):
        assert {c.layout for c in by_kernel[branch] if c.group == "d"} == {"psi", "nocopyt"}


def test_stride_cases_exceed_their_thresholds():
    stride = _const("devcg.hpp", "CG_BLOCKS") * _const("devcg.hpp", "CG_THREADS")
    src = open(os.path.join(CSRC, "fb.hip")).read()
    m = re.search(r"static void launch_shrink\(.*?ceil_div\(n / 2, (\d+)\), (\d+)\)", src, re.S)
    assert m
    shrink_stride = int(m.group(1)) * int(m.group(2))
    assert stride == 262144 and shrink_stride == 8192 * 256
    assert f"i += int64_t(gridDim.x) * {m.group(1)}" in src

    def second_trip_with_tail(n, s, trips=2):
        return (trips - 1) * s < n < trips * s

    e = {c.id: c for c in sc.CASES if c.group == "e"}
    for cid in ("e-fb-nb17-128x122", "e-pd-nb17-128x122"):  # k_fb_step_gen / k_pd_norms run over nband * npix
        c = e[cid]
        assert c.nband * c.img[0] * c.img[1] == 265472 and second_trip_with_tail(265472, stride)
        assert ("k_fb_step_gen" if c.solver == "fb" else "k_pd_norms") in sc.kernels(c)
    for cid, kern in (("e-fb-nb1-E-1024x514", "k_fb_step<1,false>"), ("e-fb-nb1-I-1024x514", "k_fb_step<1,true>")):
        c = e[cid]  # two pixels per thread
        assert second_trip_with_tail(c.img[0] * c.img[1] // 2, stride) and kern in sc.kernels(c)
    c = e["e-pd-nb1-1024x514"]
    assert second_trip_with_tail(c.img[0] * c.img[1], stride, trips=3) and "k_pd_step" in sc.kernels(c)
    for cid in ("e-fb-nb1-l21-2048x1028", "e-fb-nb1-l1-2048x1028"):  # two coefficients per thread
        c = e[cid]
        assert sc.cube_of(c) == 4210688 and second_trip_with_tail(sc.cube_of(c) // 2, shrink_stride)
        assert "k_fb_shrink<1>" in sc.kernels(c)
    assert {e["e-fb-nb1-l21-2048x1028"].reg, e["e-fb-nb1-l1-2048x1028"].reg} == {"l21", "l1"}
    assert len(e) == 7


# ---- the inputs -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cid", IDS)
def test_inputs_exercise_the_kernels(cid):
    case = sc.BY_ID[cid]
    st, zeros, _ = _records(cid)
    x0 = sc.problem(case).x0
    assert x0[:, 0, 0].all() and x0[:, -1, -1].all()  # a norm that drops an end element differs in iteration 1
    for k, (s, nzero) in enumerate(zip(st, zeros), 1):
        print(f"{cid} iteration {k}: {s} exact zeros before the clamp {nzero}")
        assert s["nonzero"]
        assert 0.1 <= s["bite"] <= 0.9
        if case.pos:
            assert s["low"] >= 0.01 and s["high"] >= 0.1
        if case.pos == 2:
            # off the edge of the one discontinuity: exactly 0 (a thresholded identity element at nu = 1) or well away
            assert s["edge"] >= 1e-9
            if not (case.dic == "I" and case.nu == 1.0):
                assert nzero == 0
            elif case.reg == "l1" and case.nband > 1:
                assert s["only_le"] >= 5  # pixels that tell "<= 0" from "< 0"


def test_tie_inputs():
    for nband in sc.TIE_BANDS + (sc.TIE_COMM_BANDS,):
        x0, w = sc.tie_inputs(nband)
        vt, s, thr, v = sc.tie_expected(nband)
        assert np.array_equal(x0 * 8, np.round(x0 * 8)) and np.abs(x0).max() < 64
        wnz = w[w != 0]
        assert np.array_equal(np.log2(wnz), np.round(np.log2(wnz))) and np.log2(sc.TIE_LAM) == round(np.log2(sc.TIE_LAM))
        # every vtilde and band sum is a small multiple of 1/16: exact in any order of summation
        for a in (vt, vt.sum(axis=0), np.cumsum(vt, axis=0), np.cumsum(vt[::-1], axis=0)):
            assert np.array_equal(a * 16, np.round(a * 16)) and np.abs(a).max() < 2**20
        ties = (s == thr) & (thr > 0)
        assert ties.sum() >= 5 and (w == 0).sum() >= 5
        assert np.array_equal(v[:, ties], vt[:, ties])  # unscaled
        assert ((s > thr) & (s <= thr + 1.0 / 16.0) & (thr > 0)).sum() >= 5  # and the nearest value above is scaled
        assert ((s > thr).mean() > 0.1) and ((s <= thr).mean() > 0.1)
        # it is the yardstick's dual update
        p = sc.problem(sc.tie_case(nband))._replace(x0=x0, weight=w)
        _, rec = sc.pd_step_ref(sc.pd_start(p), p, sigma=sc.TIE_SIGMA, tau=0.1)
        assert np.array_equal(rec["v"], v) and np.array_equal(rec["vt"], vt)
