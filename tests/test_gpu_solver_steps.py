"""The step kernels of the device-resident backward solvers, one iteration at a time: the forward-backward loop (csrc/fb.hip)
and the primal-dual loop (csrc/pd.hip with the l21 kernels of csrc/psi.hip) at every built band count and at every size edge,
through the public classes only (ForwardBackward / PrimalDual with PsfGrad(HessPSF), L21 / L1 over PsiNocopyt, Psi or
IdentityPsi).  The yardstick is one iteration of tests/_fb_ref.py / tests/_pd_ref.py at a time (tests/_step_cases.py) over the
CPU oracle's dictionary and fftconv.hess_psf_dot; tests/test_solver_steps_cpu.py holds the case table and the inputs to what
this module relies on.

Every case runs ``tol = 0, maxit = k`` for k = 1, 2, 3 from the same start (a fresh solver each time, so the dual starts at
zero; k = 1 and 3 for the three cases with the slowest yardstick): iteration 1 has beta = 0, iteration 3 is the first whose
forward step reads the y and d that a step kernel wrote with beta != 0.  Compared: x, ``last["eps"]``, ``last["iters"] == k - 1``
and, for the primal-dual loop, the dual.

Bounds, from this project's own component bounds (never from the loop under test), with TOL = 4e-13:
  x     rel-l2(x_k) <= k TOL.  One iteration is one PSF-Hessian apply per band (1e-13: BOUND of test_gpu_psffft.py, fallback
        included), the analysis and the synthesis (1e-14 each: test_gpu_psi.py) and about ten elementwise roundings: about
        1.3e-13, times 3.  Every later map is non-expansive except FISTA's extrapolation (1 + 2 beta < 1.6 up to iteration 3).
  eps   |eps - eps_ref| <= 3 k TOL (the difference of two iterates carries at most twice the iterate error, relative to |x|).
  dual  |v_k - v_ref|_2 <= 4 k sigma sqrt(nbasis) (k TOL) max_j |x_j|_2.
The soft thresholds, the l21 ratio, the dual clip and positivity mode 1 are continuous; positivity mode 2 is not, and the
inputs keep the yardstick 1e-9 max|x| away from its edge (test_solver_steps_cpu.py).

What each test launches (tests/_step_cases.kernels restates the choices of the launchers), and the largest ratio to its bound
measured on an MI355X (x / eps / dual):
  test_fb_every_instantiation           k_fb_shrink<NB> + k_fb_step<NB, false>, NB = 1..16: every NB with l21, every second
                                        one with l1 too; positivity 0 / 1 / 2, FISTA and ISTA, both layouts
  test_fb_identity_every_instantiation  k_fb_step<NB, true>, NB = 1..16, nu = 1 and 1.25
  test_fb_fallbacks                     k_fb_bandsum + k_fb_shrink_gen with the fast step (odd cube); the identity's copy +
                                        k_fb_shrink_gen + k_fb_flag + k_fb_step_gen (odd pixel count); all of them at 17 bands
  test_pd                               k_l21_fused with k_pd_step (1, 2, 16 bands) and with k_pd_primal + k_positivity +
                                        k_pd_norms (17, 18 bands), even and odd cube, both layouts
  test_stride_tails                     the second trip, with a partial tail, of k_fb_step_gen and k_pd_norms (17 bands,
                                        265472 elements), k_fb_step<1, false / true> (263168 pixel pairs), k_pd_step (526336
                                        pixels: three trips) and k_fb_shrink<1> (2105344 coefficient pairs)
  test_ties_in_the_fused_dual_update    k_l21_fused at |sum| == lam w and at w = 0, dyadic inputs: bit-equal
  test_ties_through_the_communicator    k_l21_localsum + k_l21_apply on a forced 1-rank communicator: bit-equal to the plain run
  test_many_band_positivity_at_exact_zero  k_positivity at a band of exactly 0 beside positive ones (which the loop cannot reach)
  test_pd_zero_iterate                  x = xtilde = 0 stays 0 on both branches of pd_iteration
Largest measured ratio to the bound, over the cases and k of each test (every test prints its figures before it asserts):
  test_fb_every_instantiation           x 2.8e-4, eps 4.6e-5
  test_fb_identity_every_instantiation  x 2.5e-4, eps 2.3e-5
  test_fb_fallbacks                     x 3.0e-4, eps 4.6e-5
  test_pd                               x 3.2e-4, eps 4.6e-5, dual 1.7e-5
  test_stride_tails                     x 3.3e-4, eps 1.4e-4, dual 1.2e-5
  test_ties_in_the_fused_dual_update    dual: 0 bits differ; x 1.3e-3
  test_ties_through_the_communicator    0 elements differ
The iterates agree to 1e-16 (relative): the bounds above are the components' own and leave three orders of magnitude, and no
case needed the generic loop as a second yardstick.  What the bounds do resolve was checked on a scratch build with four
defects at once: band 5 of k_fb_step<7, false> reading band 6, "<" for "<=" in k_fb_flag, the second trip of k_fb_step_gen
ending 100 elements early, and k_pd_norms leaving out its last element fail, respectively, a-E-nb7-l21-p0 alone; the two
odd-identity l1 positivity-2 cases with more than one band (nu = 1: a band at exactly 0 beside positive ones); e-fb-nb17-128x122
alone; and all 13 cases with 17 or 18 primal-dual bands -- each defect exactly the cases that can see it, 17 of 115 in all.
"""

import numpy as np
import pytest

from tests import _step_cases as sc

pytestmark = pytest.mark.gpu

TOL = 4e-13


def _ids(group):
    return [c.id for c in sc.CASES if c.group == group]


def _device(case, p):
    """(hess, reg) of a case on the device: the weight goes in in the layout of the dictionary."""
    from pfb_imaging_amd.operators.hessian import HessPSF
    from pfb_imaging_amd.operators.psi import IdentityPsi, Psi, PsiNocopyt
    from pfb_imaging_amd.opt import L1, L21

    nx, ny = case.img
    hess = HessPSF(nx, ny, p.abspsf, beam=p.beam, eta=p.eta, taper_width=8)
    if case.dic == "I":
        psi, bases, w = IdentityPsi(case.nband, nx, ny), ("self",), p.weight[None]
    else:
        bases = sc.DICTS[case.dic]
        psi = (Psi if case.layout == "psi" else PsiNocopyt)(case.nband, nx, ny, bases, sc.NLEVEL, 1)
        w = p.weight.transpose(0, 2, 1) if case.layout == "psi" else p.weight
    w = np.ascontiguousarray(w)
    if case.reg == "l1":
        reg = L1(psi, nu=case.nu)
        reg.weight = w
    else:
        reg = L21(psi, bases, nu=case.nu)
        assert reg.l1weight.shape == w.shape
        reg.l1weight = w
    return hess, reg


def _solve(case, p, hess, reg, k, sigma=None, maxit=None, tol=0.0, comm=None):
    """One run of the device loop from the case's start; returns (x, last, dual in the oracle's layout or None)."""
    from pfb_imaging_amd import prox
    from pfb_imaging_amd.opt import ForwardBackward, PrimalDual, PsfGrad

    pp = prox.positivity_prox(case.pos)
    if case.solver == "fb":
        s = ForwardBackward(tol=tol, maxit=k, gamma=sc.GAMMA_FB, acceleration=case.accel, primal_prox=pp, verbosity=0)
        s.setup(reg, p.hessnorm)
        assert s.step == p.step
        s.set_grad(PsfGrad(hess, p.xtilde, 1.0))
        assert s._device_path() == case.pos
        return s.solve(p.x0.copy(), case.lam), s.last, None
    s = PrimalDual(tol=tol, maxit=k, gamma=sc.GAMMA_PD, sigma=sigma, primal_prox=pp, verbosity=0)
    s.setup(reg, p.hessnorm)
    if sigma is None:
        assert s.sigma == p.sigma and s.tau == p.tau
    s.set_grad(PsfGrad(hess, p.xtilde, sc.GAMMA_PD))
    assert s._device_path() == case.pos
    if comm is not None:  # a 1-rank communicator is "world_size 1": force the collective code path
        bands, _, local = s._hess_bands(hess, case.nband)
        s._hess_bands = lambda h, n: (bands, comm, local)
    x = s.solve(p.x0.copy(), case.lam)
    v = s._v.transpose(0, 1, 3, 2) if case.layout == "psi" else s._v
    return x, s.last, v.copy(), s


def _check(case):
    p = sc.problem(case)
    recs = sc.run_ref(p, max(case.ks))
    hess, reg = _device(case, p)
    xnorm = [np.linalg.norm(p.x0)] + [np.linalg.norm(r["x"]) for r in recs]
    failed = []
    try:
        for k in case.ks:
            x, last, v = _solve(case, p, hess, reg, k)[:3]
            ref = recs[k - 1]
            assert ref["x"].any()
            ex = np.linalg.norm(x - ref["x"]) / np.linalg.norm(ref["x"])
            ee = abs(last["eps"] - ref["eps"])
            line = f"RATIO {case.id} k={k} x {ex:.2e} / {k * TOL:.1e} = {ex / (k * TOL):.1e}  eps {ee:.2e} / {3 * k * TOL:.1e} = " \
                   f"{ee / (3 * k * TOL):.1e}"
            ok = ex <= k * TOL and ee <= 3 * k * TOL and last["iters"] == k - 1 and last["status"] == 1
            if v is not None:
                ev = np.linalg.norm(v - ref["v"])
                bv = 4 * k * p.sigma * np.sqrt(p.psi.nbasis) * (k * TOL) * max(xnorm[:k + 1])
                line += f"  dual {ev:.2e} / {bv:.1e} = {ev / bv:.1e}"
                ok = ok and ev <= bv
            print(line + f"  iters {last['iters']} nonzero {np.count_nonzero(x)} / {x.size}")
            if not ok:
                failed.append(line)
    finally:
        hess._plan.close()
    assert not failed, failed


@pytest.mark.parametrize("cid", _ids("a"))
def test_fb_every_instantiation(cid):
    _check(sc.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("b"))
def test_fb_identity_every_instantiation(cid):
    _check(sc.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("c"))
def test_fb_fallbacks(cid):
    _check(sc.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("d"))
def test_pd(cid):
    _check(sc.BY_ID[cid])


@pytest.mark.parametrize("cid", _ids("e"))
def test_stride_tails(cid):
    _check(sc.BY_ID[cid])


def _bits_equal(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _tie_run(nband, comm=None):
    case = sc.tie_case(nband)
    x0, w = sc.tie_inputs(nband)
    p = sc.problem(case)._replace(x0=x0, weight=w)
    hess, reg = _device(case, p)
    try:
        x, last, v, s = _solve(case, p, hess, reg, 1, sigma=sc.TIE_SIGMA, comm=comm)
    finally:
        hess._plan.close()
    assert s.sigma == sc.TIE_SIGMA and last["iters"] == 0
    return p, x, v, s


@pytest.mark.parametrize("nband", sc.TIE_BANDS)
def test_ties_in_the_fused_dual_update(nband):
    """Dyadic inputs, the dual starting at zero, sigma = 1/2: vtilde and its band sum are exact and the update is one division
    and one multiply per element (the header of tests/test_gpu_numba_pins.py), so the dual comes back bit-equal to
    vt * where(|s| > thr, thr / |s|, 1).  The strict > is pinned by coefficients with |s| == thr exactly (unscaled) beside
    coefficients one step of 1/16 above; w = 0 zeroes the coefficient."""
    vt, s, thr, want = sc.tie_expected(nband)
    p, x, v, solver = _tie_run(nband)
    ties = (s == thr) & (thr > 0)
    zero_w = thr == 0
    diff = np.ascontiguousarray(v).view(np.int64) != np.ascontiguousarray(want).view(np.int64)
    print(f"ties nband {nband}: {ties.sum()} ties, {zero_w.sum()} zero weights, {(s > thr).sum()} clipped of {s.size}; "
          f"{diff.sum()} elements differ in their bits, max |diff| {np.abs(v - want).max():.2e}")
    assert ties.sum() >= 5 and zero_w.sum() >= 5
    assert _bits_equal(v[:, ties], vt[:, ties])
    assert not v[:, zero_w & (s > 0)].any()
    assert _bits_equal(v, want)
    # and the iterate of that one iteration, to the bound of every other case
    _, rec = sc.pd_step_ref(sc.pd_start(p), p, sigma=solver.sigma, tau=solver.tau)
    ex = np.linalg.norm(x - rec["x"]) / np.linalg.norm(rec["x"])
    print(f"RATIO f-S-nb{nband} k=1 x {ex:.2e} / {TOL:.1e} = {ex / TOL:.1e}")
    assert ex <= TOL


def test_ties_through_the_communicator():
    """The same inputs at two bands through the band-per-rank form (k_l21_localsum, the all-reduce, k_l21_apply): bit-equal to
    the plain run, which is bit-equal to the expected dual."""
    from pfb_imaging_amd.parallel import BandComm

    nband = sc.TIE_COMM_BANDS
    vt, s, thr, want = sc.tie_expected(nband)
    _, x_plain, v_plain, _ = _tie_run(nband)
    comm = BandComm.from_env(transport="rccl")
    try:
        _, x_comm, v_comm, _ = _tie_run(nband, comm=comm)
    finally:
        comm.close()
    ties = (s == thr) & (thr > 0)
    print(f"ties through the communicator: {ties.sum()} ties; dual differs from the plain run in "
          f"{(v_comm != v_plain).sum()} elements, x in {(x_comm != x_plain).sum()}")
    assert ties.sum() >= 5
    assert _bits_equal(v_plain, want)
    assert _bits_equal(v_comm, v_plain) and _bits_equal(x_comm, x_plain)
    assert _bits_equal(v_comm[:, ties], vt[:, ties])


def test_many_band_positivity_at_exact_zero():
    """The "<= 0" of k_positivity, the kernel of the primal-dual loop's many-band branch.  Inside that loop x = xp - tau xout
    never lands on 0 exactly beside positive bands, so the loop cannot tell "<=" from "<"; the same kernel through
    ``prox.positivity_band`` at 17 bands can: a band at +0 or -0, every other band positive, zeroes the pixel."""
    from oracle import psi as opsi
    from pfb_imaging_amd import prox

    rng = np.random.default_rng(17)
    x = 0.1 + rng.random((sc.MAXB + 1,) + sc.SMALL_ODD)
    x[3, 5, 7], x[sc.MAXB, -1, -1], x[0, 0, 0], x[8, 10, 11] = 0.0, 0.0, -0.0, -1.0
    want = opsi.positivity_band(x.copy())
    zeroed = [(5, 7), (-1, -1), (0, 0), (10, 11)]
    assert all(not want[:, i, j].any() for i, j in zeroed) and np.count_nonzero(want) == x.size - 4 * (sc.MAXB + 1)
    got = x.copy()
    prox.positivity_band(got)
    print(f"positivity 2 at exact zeros: {np.count_nonzero(got != want)} elements differ")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("nband,pos", [(2, 1), (sc.MAXB + 1, 2)])
def test_pd_zero_iterate(nband, pos):
    """x = xtilde = 0 stays exactly 0 in k_pd_step and in the many-band branch: eps = 1 every iteration, the loop ends on maxit."""
    case = sc.BY_ID[f"d-E-nb{nband}-p{pos}"]
    p = sc.problem(case)
    zero = np.zeros_like(p.x0)
    p = p._replace(x0=zero, xtilde=zero)
    hess, reg = _device(case, p)
    try:
        x, last, v = _solve(case, p, hess, reg, 4, tol=1e-5)[:3]
    finally:
        hess._plan.close()
    print(f"zero iterate nband {nband}: nonzero x {np.count_nonzero(x)}, nonzero dual {np.count_nonzero(v)}, last {last['eps']}, "
          f"{last['status']}, {last['iters']}")
    assert not x.any() and not v.any()
    assert last["eps"] == 1.0 and last["status"] == 1 and last["iters"] == 3
