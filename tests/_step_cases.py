"""The cases, inputs and one-iteration yardsticks of the solver step tests (tests/test_gpu_solver_steps.py on the device,
tests/test_solver_steps_cpu.py on the yardstick alone).  numpy only.

``CASES`` lists every (solver, band count, dictionary, regulariser, positivity, ...) combination; ``problem(case)`` builds its
inputs; ``fb_step_ref`` / ``pd_step_ref`` restate ONE iteration of tests/_fb_ref.fb_ref / tests/_pd_ref.pd_ref and hand back
the intermediates (the pre-clamp x, the band sums against their thresholds, eps, the dual); ``run_ref`` chains them.

Geometries.  Small: the image (24, 20), or (21, 23) for an odd pixel count, on a (48, 40) PSF -- the rocFFT fallback, one
plan size for all of them.  Dictionary E = (self, db1), 2 levels: cube 960, even.  Dictionary O = (self, db1, db2): cube 2175,
odd.  I = the identity.  S = (self,): Psi^T is a copy (the tie cases).  Stride: padded sizes of the row-FFT family only.

Inputs (in the style of ``_psf_problem`` / ``_images`` of the neighbouring GPU tests): the bands share most of their signal (the
l21 prox couples them through the band SUM), PSF = delta + 0.02 noise, beam in [0.8, 1], one eta per band, weights
0.5 + U(0, 1), ``hessnorm`` the valid bound max|psfhat| max(beam)^2 + max(eta).

``nu``.  Over a wavelet dictionary with nu = nbasis, a pixel all of whose coefficients are thresholded comes out as
xg - xg (1 +- 1e-16): rounding noise around zero, which positivity mode 2 (zero the pixel in EVERY band if ANY band is <= 0)
turns into a coin toss.  The positivity-2 cases over wavelets therefore take nu = 1.25 nbasis, where such a pixel is 0.2 xg.
Over the identity at nu = 1 a thresholded element is xg - xg = 0 exactly, on the device as in numpy.

``lam`` was tuned per family on the CPU (tests/test_solver_steps_cpu.py holds the conditions): the threshold bites on 10-90 %
of the coefficients, positivity clamps some elements and leaves some, x != 0, for every iteration compared.
"""

import collections
import functools

import numpy as np

from oracle import fftconv
from oracle import psi as opsi
from tests._fb_ref import prox_l1, prox_l21
from tests._pd_ref import dual_update

NLEVEL = 2
DICTS = {"E": ("self", "db1"), "O": ("self", "db1", "db2"), "S": ("self",)}
SMALL, SMALL_ODD, SMALL_PAD = (24, 20), (21, 23), (48, 40)
GAMMA_FB, GAMMA_PD = 0.45, 1.0
MAXB = 16  # LOOP_MAXB of csrc/devloop.hpp (test_solver_steps_cpu.py reads it from the source)

Case = collections.namedtuple("Case", "id group solver nband img pad dic layout reg pos accel nu lam seed ks")


def nbasis_of(dic):
    return 1 if dic == "I" else len(DICTS[dic])


def _nu_fb(dic, pos, alt):
    if dic == "I":
        return 1.25 if alt else 1.0
    nb = float(nbasis_of(dic))
    return 1.25 * nb if (pos == 2 or alt) else nb


def _lam(solver, dic, reg, nband, img):
    """The per-family tuning: l21 thresholds the band SUM, which grows with the band count; l1 each band on its own.  The
    PSF noise of the stride cases has a spectrum 20-40 times the small cases', so their hessnorm is that much larger and
    their steps that much shorter."""
    if solver == "pd":
        base = {24: 0.1, 21: 0.1, 128: 2.0, 1024: 4.0}[img[0]]
        return base * nband
    base = {24: 0.5, 21: 0.5, 128: 12.0, 1024: 12.0, 2048: 25.0}[img[0]] * (0.6 if dic == "I" else 1.0)
    return base * (nband if reg == "l21" else 1.0)


def _case(cid, group, solver, nband, dic, reg="l21", pos=0, accel=True, alt=False, layout="nocopyt", img=SMALL, pad=SMALL_PAD,
          seed=0, ks=(1, 2, 3)):
    nu = _nu_fb(dic, pos, alt) if solver == "fb" else float(np.sqrt(nbasis_of(dic)))
    return Case(cid, group, solver, nband, img, pad, dic, layout, reg, pos, accel, nu, _lam(solver, dic, reg, nband, img),
                seed, ks)


def _table():
    t = []
    # a / b: every instantiation of k_fb_shrink<NB> + k_fb_step<NB, false> (E) and of k_fb_step<NB, true> (I): every NB with
    # l21, every second NB with l1 as well; positivity cycles, acceleration and nu alternate
    for group, dic in (("a", "E"), ("b", "I")):
        for nb in range(1, MAXB + 1):
            t.append(_case(f"{group}-{dic}-nb{nb}-l21-p{(nb - 1) % 3}", group, "fb", nb, dic, "l21", (nb - 1) % 3, nb % 2 == 1,
                           alt=nb % 4 >= 2, layout="psi" if nb % 5 == 0 else "nocopyt", seed=100 + nb))
            if nb % 2 == 0:
                t.append(_case(f"{group}-{dic}-nb{nb}-l1-p{(nb // 2) % 3}", group, "fb", nb, dic, "l1", (nb // 2) % 3,
                               (nb // 2) % 2 == 0, alt=nb % 4 == 0, layout="psi" if nb % 6 == 0 else "nocopyt", seed=200 + nb))
    # c: the fallbacks.  O (odd cube): k_fb_bandsum + k_fb_shrink_gen with the fast step
    i = 0
    for nb in (1, MAXB):
        for reg in ("l21", "l1"):
            t.append(_case(f"c-O-nb{nb}-{reg}-p{(i + 1) % 3}", "c", "fb", nb, "O", reg, (i + 1) % 3, i % 2 == 0, seed=300 + i))
            i += 1
    # the identity on an odd pixel count: the copy, k_fb_shrink_gen, k_fb_flag (positivity 2), k_fb_step_gen.  l1 with
    # positivity 2 takes nu = 1: a band thresholded to exactly 0 beside positive ones is what tells <= from < in k_fb_flag
    for nb in (1, 2, MAXB):
        for pos in (0, 1, 2):
            for reg in ("l21", "l1"):
                t.append(_case(f"c-Iodd-nb{nb}-{reg}-p{pos}", "c", "fb", nb, "I", reg, pos, i % 2 == 0,
                               alt=(reg == "l21") if pos == 2 else i % 3 == 0, img=SMALL_ODD, seed=300 + i))
                i += 1
    # one band more than the templates hold
    t.append(_case("c-E-nb17-l21-p2", "c", "fb", MAXB + 1, "E", "l21", 2, False, seed=340))
    t.append(_case("c-I-nb17-l1-p1", "c", "fb", MAXB + 1, "I", "l1", 1, True, seed=341))
    # d: primal-dual; 16 is the last count of k_pd_step, 17 and 18 take k_pd_primal + k_positivity + k_pd_norms
    for dic in ("E", "O"):
        for nb in (1, 2, MAXB, MAXB + 1, MAXB + 2):
            for pos in (0, 1, 2):
                t.append(_case(f"d-{dic}-nb{nb}-p{pos}", "d", "pd", nb, dic, "l21", pos,
                               layout="psi" if (nb in (2, MAXB + 1) and pos == 1) else "nocopyt", seed=400 + nb * 3 + pos))
    # e: the grid-stride loops take a second trip with a partial tail
    big = dict(pad=(1024, 1024))
    t.append(_case("e-fb-nb17-128x122", "e", "fb", MAXB + 1, "E", "l21", 1, True, img=(128, 122), seed=500, ks=(1, 3), **big))
    t.append(_case("e-pd-nb17-128x122", "e", "pd", MAXB + 1, "E", "l21", 2, img=(128, 122), seed=501, **big))
    t.append(_case("e-fb-nb1-E-1024x514", "e", "fb", 1, "E", "l21", 1, True, img=(1024, 514), seed=502, **big))
    t.append(_case("e-fb-nb1-I-1024x514", "e", "fb", 1, "I", "l21", 2, True, img=(1024, 514), seed=503, **big))
    t.append(_case("e-pd-nb1-1024x514", "e", "pd", 1, "E", "l21", 1, img=(1024, 514), seed=504, **big))
    for reg, pos, seed in (("l21", 2, 505), ("l1", 1, 506)):
        t.append(_case(f"e-fb-nb1-{reg}-2048x1028", "e", "fb", 1, "E", reg, pos, True, img=(2048, 1028), pad=(2048, 2048),
                       seed=seed, ks=(1, 3)))
    return t


CASES = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# the three cases whose yardstick takes longest (0.6 - 1 s per iteration): k = 1 and 3 on the device, k = 1 in the CPU conditions
BIG = ("e-fb-nb17-128x122", "e-fb-nb1-l21-2048x1028", "e-fb-nb1-l1-2048x1028")
assert all(i in BY_ID for i in BIG)


def kernels(case, maxb=MAXB):
    """The step kernels a case launches: the choices of pfbhip_fb_run (csrc/fb.hip) and pd_iteration (csrc/pd.hip) restated."""
    nb, npix, cube = case.nband, case.img[0] * case.img[1], cube_of(case)
    out = set()
    if case.solver == "pd":
        out.add("k_l21_fused")
        if nb <= maxb:
            out.add("k_pd_step")
        else:
            out |= {"k_pd_primal", "k_pd_norms"} | ({"k_positivity"} if case.pos else set())
        return out
    fast = nb <= maxb and npix % 2 == 0
    if case.dic == "I" and fast:
        return {f"k_fb_step<{nb},true>"}
    if nb <= maxb and cube % 2 == 0:
        out.add(f"k_fb_shrink<{nb}>")
    else:
        out |= {"k_fb_shrink_gen"} | ({"k_fb_bandsum"} if case.reg == "l21" else set())
    if fast:
        out.add(f"k_fb_step<{nb},false>")
    else:
        out |= {"k_fb_step_gen"} | ({"k_fb_flag"} if case.pos == 2 else set())
    return out


def oracle_psi(case):
    """The CPU oracle's dictionary in its x-first layout, None for the identity."""
    if case.dic == "I":
        return None
    return opsi.Psi(case.nband, case.img[0], case.img[1], DICTS[case.dic], NLEVEL)


def cube_of(case):
    """Coefficients per band."""
    if case.dic == "I":
        return case.img[0] * case.img[1]
    o = oracle_psi(case)
    return o.nbasis * o.nxmax * o.nymax


def support(o):
    """The coefficients a basis really has, as a mask over (nbasis, nxmax, nymax): the rest of the cube is padding."""
    m = np.zeros((o.nbasis, o.nxmax, o.nymax), dtype=bool)
    w = 0
    for i, name in enumerate(o.bk.bases):
        if name == "self":
            m[i, :o.nx, :o.ny] = True
        else:
            m[i, :o.bk.ntotx[w], :o.bk.ntoty[w]] = True
            w += 1
    return m


Problem = collections.namedtuple("Problem", "case psi abspsf beam eta hessnorm href x0 xtilde weight step sigma tau")


@functools.lru_cache(maxsize=4)
def problem(case):
    """The inputs of a case.  ``weight`` is (nbasis, nxmax, nymax) in the oracle's layout, (nx, ny) for the identity."""
    rng = np.random.default_rng(case.seed)
    nband, (nx, ny), (nxp, nyp) = case.nband, case.img, case.pad
    psf = 0.02 * rng.standard_normal((nband, nxp, nyp))
    psf[:, 0, 0] += 1.0
    abspsf = np.abs(np.fft.rfft2(psf, axes=(1, 2)))
    del psf
    beam = 0.8 + 0.2 * rng.random((nband, nx, ny))
    eta = np.linspace(0.05, 0.1, nband)
    hessnorm = float(abspsf.max() * beam.max() ** 2 + eta.max())
    common = np.abs(rng.standard_normal((nx, ny))) * (rng.random((nx, ny)) > 0.9)
    common[0, 0] += 1.0  # the first and the last element of every band reach the norms of iteration 1 even if it zeroes them
    common[-1, -1] += 1.0
    x0 =common[None] * (1.0 + 0.1 * rng.random((nband, nx, ny)))
    xtilde = x0 + 0.3 * rng.standard_normal((1, nx, ny)) + 0.02 * rng.standard_normal(x0.shape)
    o = oracle_psi(case)
    weight = 0.5 + rng.random((nx, ny) if o is None else (o.nbasis, o.nxmax, o.nymax))

    def href(z):
        return fftconv.hess_psf_dot(z, abspsf, nyp, beam=beam, eta=eta)

    step = 2.0 * GAMMA_FB / hessnorm  # ForwardBackward.setup
    half = hessnorm / (2.0 * GAMMA_PD)  # PrimalDual.setup
    sigma = half / case.nu
    tau = 0.98 / (half + sigma * case.nu**2)
    return Problem(case, o, abspsf, beam, eta, hessnorm, href, x0, xtilde, weight, step, sigma, tau)


# ---- one iteration at a time ------------------------------------------------------------------------------------------


def _eps(x, xp):
    return float(np.sqrt(((x - xp) ** 2).sum() / max((x**2).sum(), 1e-12))) if x.any() else 1.0


def _positivity(x, mode):
    if mode == 1:
        x[x < 0.0] = 0.0
    elif mode == 2:
        x[:, (x <= 0.0).any(axis=0)] = 0.0


def fb_start(p):
    return dict(xp=np.array(p.x0, dtype=np.float64), y=np.array(p.x0, dtype=np.float64), t=1.0)


def fb_step_ref(state, p):
    """One iteration of ``fb_ref``, operation for operation.  Returns (next state, dict(x, pre, s, thr, eps)): ``pre`` is x
    before the positivity step, ``s`` what the threshold ``thr`` is compared with (the band sum for l21, every coefficient
    for l1) in the coefficient layout (.., nbasis, nxmax, nymax) (nbasis = 1 for the identity); ``thr`` broadcasts against it."""
    c = p.case
    xp, y, t = state["xp"], state["y"], state["t"]
    xg = y + p.step * p.href(p.xtilde - y) / 1.0
    if p.psi is None:
        a = xg[:, None]
    else:
        a = np.zeros((xg.shape[0], p.psi.nbasis, p.psi.nxmax, p.psi.nymax))
        p.psi.dot(xg, a)
    thr = p.step * c.lam * p.weight
    diff = (prox_l1 if c.reg == "l1" else prox_l21)(a, thr) - a
    if p.psi is None:
        xo = diff[:, 0]
    else:
        xo = np.zeros_like(xg)
        p.psi.hdot(diff, xo)
    x = xg + xo / c.nu
    pre = x.copy()
    _positivity(x, c.pos)
    eps = _eps(x, xp)
    if c.accel:
        tp = t
        t = (1.0 + np.sqrt(1.0 + 4.0 * tp * tp)) / 2.0
        y = x + (tp - 1.0) / t * (x - xp)
    else:
        y = x.copy()
    s = a if c.reg == "l1" else a.sum(axis=0)
    return dict(xp=x, y=y, t=t), dict(x=x, pre=pre, s=s, thr=thr, eps=eps)


def pd_start(p, v0=None):
    o = p.psi
    v = np.zeros((p.case.nband, o.nbasis, o.nxmax, o.nymax)) if v0 is None else np.array(v0, dtype=np.float64)
    return dict(xp=np.array(p.x0, dtype=np.float64), vp=v)


def pd_step_ref(state, p, sigma=None, tau=None, lam=None, weight=None):
    """One iteration of ``pd_ref``.  Returns (next state, dict(x, pre, s, thr, eps, v, vt)): ``s`` the band sum of
    vtilde = vp + sigma Psi^T xp, ``thr`` = lam w, ``v`` the updated dual."""
    c = p.case
    sigma = p.sigma if sigma is None else sigma
    tau = p.tau if tau is None else tau
    lam = c.lam if lam is None else lam
    weight = p.weight if weight is None else weight
    xp, vp = state["xp"], state["vp"]
    v = np.zeros_like(vp)
    p.psi.dot(xp, v)
    vt = vp + sigma * v
    v = dual_update(vp, v, lam, sigma, weight)
    xout = np.zeros_like(xp)
    p.psi.hdot(2.0 * v - vp, xout)
    xout = xout - p.href(p.xtilde - xp) / GAMMA_PD
    x = xp - tau * xout
    pre = x.copy()
    _positivity(x, c.pos)
    eps = _eps(x, xp)
    return dict(xp=x, vp=v), dict(x=x, pre=pre, s=vt.sum(axis=0), thr=lam * weight, eps=eps, v=v, vt=vt)


def run_ref(p, k):
    """The records of iterations 1..k from the case's start (the dual starts at zero)."""
    fb = p.case.solver == "fb"
    state = fb_start(p) if fb else pd_start(p)
    out = []
    for _ in range(k):
        state, rec = (fb_step_ref if fb else pd_step_ref)(state, p)
        out.append(rec)
    return out


def stats(p, rec):
    """What one iteration's record says about its inputs: ``bite`` the fraction of the dictionary's coefficients (padding
    left out) the threshold acts on -- zeroed by the forward-backward prox, clipped by the dual update --, ``low`` / ``high``
    the fractions of elements (positivity 1) or pixels (positivity 2) that the positivity step zeroes / leaves positive,
    ``edge`` the smallest nonzero |pre-clamp value| over max|x|."""
    c = p.case
    s, thr = np.abs(rec["s"]), np.broadcast_to(rec["thr"], rec["s"].shape)
    live = np.ones(s.shape, dtype=bool) if p.psi is None else np.broadcast_to(support(p.psi), s.shape)
    hit = (s <= thr) if c.solver == "fb" else (s > thr)
    pre = rec["pre"]
    if c.pos == 2:
        bad = (pre <= 0.0).any(axis=0)
        low, high = bad.mean(), 1.0 - bad.mean()
    else:
        low, high = (pre < 0.0).mean(), (pre > 0.0).mean()
    nz = np.abs(pre[pre != 0.0])
    # pixels that only the "<= 0" of positivity 2 zeroes ("< 0" would keep them): a band at exactly 0, the others positive
    only_le = ((pre == 0.0).any(axis=0) & (pre > 0.0).any(axis=0) & ~(pre < 0.0).any(axis=0)).sum()
    return dict(bite=float(hit[live].mean()), low=float(low), high=float(high), nonzero=bool(rec["x"].any()), only_le=int(only_le),
                edge=float(nz.min() / np.abs(rec["x"]).max()) if rec["x"].any() else 0.0)


# ---- the tie inputs (dyadic) -------------------------------------------------------------------------------------------

TIE_SIGMA, TIE_LAM, TIE_BANDS, TIE_COMM_BANDS = 0.5, 0.25, (1, 3, 17), 2
NTIE = NZERO = 8


def tie_inputs(nband):
    """(x0, weight): x0 in multiples of 1/8 on (24, 20), weights powers of two (and NZERO zeros).  With the dual starting at
    zero and sigma = 1/2, vtilde = x0 / 2 and its band sum are exact; at NTIE coefficients |sum| == lam w exactly (the
    update must leave them unscaled: the comparison is a strict >), at NTIE more |sum| is one step of 1/16 above lam w."""
    nx, ny = SMALL
    rng = np.random.default_rng(700 + nband)
    x0 = rng.integers(-24, 25, size=(nband, nx, ny)) / 8.0
    weight = 2.0 ** rng.integers(-2, 4, size=(nx, ny))
    flat = rng.permutation(nx * ny)[:2 * NTIE + NZERO]
    for j, f in enumerate(flat[:2 * NTIE]):
        i, k = divmod(int(f), ny)
        thr = TIE_LAM * weight[i, k]  # 1/16 .. 2
        want = (thr if j < NTIE else thr + 1.0 / 16.0) * (1.0 if j % 2 == 0 else -1.0)
        x0[0, i, k] = want / TIE_SIGMA - x0[1:, i, k].sum()
    for f in flat[2 * NTIE:]:
        i, k = divmod(int(f), ny)
        weight[i, k] = 0.0
        if not x0[:, i, k].sum():
            x0[0, i, k] += 0.125
    return x0, weight[None]


def tie_case(nband, pos=0):
    return Case(f"f-S-nb{nband}", "f", "pd", nband, SMALL, SMALL_PAD, "S", "nocopyt", "l21", pos, True, 1.0, TIE_LAM, 700 + nband,
                (1,))


def tie_expected(nband):
    """(vt, s, thr, v): the dual after one iteration, one division and one multiply per element."""
    x0, weight = tie_inputs(nband)
    vt = TIE_SIGMA * x0[:, None]
    s = np.abs(vt.sum(axis=0))
    thr = TIE_LAM * weight
    return vt, s, thr, vt * np.where(s > thr, thr / np.where(s > 0, s, 1.0), 1.0)[None]
