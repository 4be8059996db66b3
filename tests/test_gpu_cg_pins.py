"""The device-resident conjugate gradients (DevCG) and power iteration (DevPower) of csrc/devcg.hpp against reference runs
and at the edges of their reductions.

The solver runs through ``PsfConv.cg`` with every bound psfhat identically 1, so that the operator is the diagonal
``d = sum_parts beam_part**2 + eta`` whatever the padding, and the pinned runs of the reference's ``pcg_numba`` /
``power_method_numba`` on that diagonal (tests/golden/cg_pins.npz, read through tests/_cg_pins.py) apply as they are.

Tolerances and where they come from:

  * iterations and status: exact.  The generator asserts that no pinned eps lies within 1e-6 (relative) of tol and no stall
    decision within 1e-6 of its threshold, so the reference alone decides every branch.
  * x: relative l2 <= 1e-11, this project's tolerance for FFT-based operators (header of test_gpu_psf_hessian.py); the float64
    reference run itself is within 1e-13 of the longdouble run (``x_floor``).
  * eps, phi: relative <= max(100 floors, 1e-11); the floor is the float64 reference run's distance from the longdouble run
    (in the file), the factor covers another summation order and the FFT's rounding of the operator.
  * power method: beta 1e-11, b 1e-9 relative l2 (as test_power_method_on_device), ||b|| = 1 to 1e-12.

Padded sizes: 1024 / 2048 are row-FFT lengths (the three-pass pipeline), (96, 80) takes the rocFFT fallback."""

import numpy as np
import pytest

from tests import _cg_pins as cp

pytestmark = pytest.mark.gpu

X_TOL = 1e-11
# padded sizes per image size; the two special cases of (37, 29) go through the row-FFT pipeline, the other (37, 29) cases
# through the fallback
PADS = {(3, 21): (1024, 1024), (5, 13): (1024, 1024), (3, 85): (1024, 1024), (1, 257): (1024, 2048), (37, 29): (96, 80),
        (512, 512): (1024, 1024), (512, 513): (1024, 1024)}
SPECIAL_PAD = (1024, 1024)
ROWFFT = (1024, 2048)


class Plans:
    """One PsfConv per geometry for the whole module: psfhat == 1 in slots 0 and 1, beams bound per solve."""

    def __init__(self):
        self.plans = {}

    def get(self, nx, ny, pad):
        from pfb_imaging_amd.psfconv import PsfConv

        key = (nx, ny) + tuple(pad)
        if key not in self.plans:
            pc = PsfConv(*key)
            assert pc.uses_rowfft == (pad[0] in ROWFFT and pad[1] in ROWFFT), key
            ones = np.ones((pad[0], pad[1] // 2 + 1))
            pc.set_psfhat(0, ones)
            pc.set_psfhat(1, ones)
            self.plans[key] = pc
        return self.plans[key]

    def solve(self, beam, b, x0, tol, maxit, minit, pad):
        """(x, last_cg) of PsfConv.cg on the diagonal of ``beam`` (nparts, nx, ny)."""
        nparts, nx, ny = beam.shape
        pc = self.get(nx, ny, pad)
        for k in range(nparts):
            pc.set_beam(k, beam[k])
        slots = list(range(nparts))
        x = pc.cg(b, slots, slots, scale=1.0, eta=cp.ETA, x0=x0, tol=tol, maxit=maxit, minit=minit)
        return x, dict(pc.last_cg)

    def close(self):
        for pc in self.plans.values():
            pc.close()
        self.plans.clear()


@pytest.fixture(scope="module")
def plans(monkeypatch_module):
    monkeypatch_module.delenv("PFBHIP_PSF_ROWFFT", raising=False)
    p = Plans()
    yield p
    p.close()


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _pad(name):
    size, kind = name.split("_")
    return SPECIAL_PAD if kind in ("x0", "two") else PADS[tuple(int(v) for v in size.split("x"))]


def _rel(a, ref):
    return abs(float(a) - float(ref)) / abs(float(ref))


_WORST = {}


# ---- a. reference runs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cp.CG_CASES)
def test_reference_runs(golden_dir, plans, name):
    c = cp.cg_case(cp.load(golden_dir), name)
    x, last = plans.solve(c["beam"], c["b"], c["x0"], *c["params"], _pad(name))
    dx, de, dp = cp.rel_l2(x, c["x"]), _rel(last["eps"], c["eps"][-1]), _rel(last["phi"], c["phi"])
    fl = {k: max(c[k + "_floor"], 1e-17) for k in ("x", "eps", "phi")}
    print(f"{name}: iters {last['iters']} status {last['status']} | x {dx:.2e} = {dx / fl['x']:.1f} floors, eps {de:.2e} = "
          f"{de / fl['eps']:.2f} floors, phi {dp:.2e} = {dp / fl['phi']:.1f} floors")
    for k, v in (("x", dx / fl["x"]), ("eps", de / fl["eps"]), ("phi", dp / fl["phi"])):
        if v > _WORST.get(k, (0.0, ""))[0]:
            _WORST[k] = (v, name)
    if name == cp.CG_CASES[-1]:
        print("worst of the cases run (distance in floors, case):", _WORST)
    assert (last["iters"], last["status"]) == (c["iters"], c["status"]), (last, c["iters"], c["status"])
    assert dx <= X_TOL, f"x {dx:.3e}"
    assert de <= cp.bound(c["eps_floor"]), f"eps {de:.3e} > {cp.bound(c['eps_floor']):.3e}"
    assert dp <= cp.bound(c["phi_floor"]), f"phi {dp:.3e} > {cp.bound(c['phi_floor']):.3e}"


# ---- b. one trip of the grid stride, and one element more -------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_inputs():
    out = {}
    for size in ((512, 512), (512, 513)):
        raw = cp.draw(size, 1)
        beam = raw["beam_num"] / cp.BEAM_DEN
        out[size] = dict(beam=beam, d=cp.diagonal(beam), b=raw["b_num"] / cp.B_DEN)
    return out


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("size", [(512, 512), (512, 513)], ids=["262144", "262656"])
def test_grid_stride_fixed_iterations(plans, big_inputs, size, K):
    """n = CG_BLOCKS * CG_THREADS exactly, and 512 elements more (some threads take a second one): K iterations with tol = 0,
    so the iterates themselves are compared with the longdouble restatement."""
    c = big_inputs[size]
    want = cp.cg_ref(c["d"], c["b"], None, 0.0, K, K)
    x, last = plans.solve(c["beam"], c["b"], None, 0.0, K, K, PADS[size])
    dx, de, dp = cp.rel_l2(x, want["x"]), _rel(last["eps"], want["eps"][-1]), _rel(last["phi"], want["phi"])
    print(f"{size} K={K}: x {dx:.2e} eps {de:.2e} phi {dp:.2e}")
    assert (last["iters"], last["status"]) == (K, 1) == (want["iters"], want["status"])
    assert dx <= X_TOL and de <= 1e-11 and dp <= 1e-11, (dx, de, dp)


# ---- c. sentinels -------------------------------------------------------------------------------------------------------
def _sentinel(plans, beam, d, j, pad):
    b = np.zeros(d.shape)
    b.flat[j] = 1.5
    x, last = plans.solve(beam, b, None, 0.0, 1, 1, pad)
    xj = x.flat[j]
    rest = x.copy()
    rest.flat[j] = 0.0
    assert (last["iters"], last["status"]) == (1, 1), (j, last)       # (status 3 here: a reduction missed element j)
    assert abs(xj - 1.5 / d.flat[j]) <= 1e-12 * abs(1.5 / d.flat[j]), (j, xj, 1.5 / d.flat[j])
    assert np.abs(rest).max() <= 1e-11 * abs(xj), (j, np.abs(rest).max())
    assert abs(last["eps"] - 1.0) <= 1e-12 and 0.0 <= last["phi"] <= 1e-20, (j, last)


@pytest.mark.parametrize("j", [0, 63, 64, 255, 256, 1072])
def test_sentinel_small(golden_dir, plans, j):
    """b = 1.5 e_j: one iteration solves the diagonal system exactly in element j and leaves every other element alone."""
    c = cp.cg_case(cp.load(golden_dir), "37x29_conv")
    assert c["d"].size == 1073
    _sentinel(plans, c["beam"], c["d"], j, PADS[(37, 29)])


@pytest.mark.parametrize("j", [262143, 262144, 262655])
def test_sentinel_second_trip(plans, big_inputs, j):
    c = big_inputs[(512, 513)]
    assert c["d"].size == 262656
    _sentinel(plans, c["beam"], c["d"], j, PADS[(512, 513)])


# ---- d. zero residual ---------------------------------------------------------------------------------------------------
def test_zero_rhs(golden_dir, plans):
    c = cp.cg_case(cp.load(golden_dir), "37x29_conv")
    x, last = plans.solve(c["beam"], np.zeros_like(c["b"]), None, 1e-5, 500, 1, PADS[(37, 29)])
    assert (last["status"], last["iters"]) == (3, 0) and not x.any()


@pytest.mark.parametrize("pad", [PADS[(37, 29)], SPECIAL_PAD], ids=["fallback", "rowfft"])
def test_start_is_the_solution(golden_dir, plans, pad):
    """b is the device's own A x0: the start residual is exactly zero, x0 comes back bit for bit."""
    c = cp.cg_case(cp.load(golden_dir), "37x29_x0")
    pc = plans.get(c["nx"], c["ny"], pad)
    pc.set_beam(0, c["beam"][0])
    b = np.array(pc.apply(c["x0"], 0, beam_slot=0, eta=cp.ETA))
    assert cp.rel_l2(b, c["d"] * c["x0"]) <= 1e-13
    x, last = plans.solve(c["beam"], b, c["x0"], 1e-5, 500, 1, pad)
    assert (last["status"], last["iters"]) == (3, 0) and last["phi"] == 0.0
    assert np.array_equal(x, c["x0"])


# ---- e. contracts of the header -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["37x29_conv", "37x29_x0", "1x257_stall"])
def test_two_solves_are_bitwise_equal(golden_dir, plans, name):
    c = cp.cg_case(cp.load(golden_dir), name)
    x0 = None if c["x0"] is None else c["x0"].copy()
    runs = [plans.solve(c["beam"], c["b"], x0, *c["params"], _pad(name)) for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1], (runs[0][1], runs[1][1])
    if x0 is not None:
        assert np.array_equal(x0, c["x0"]) and runs[0][0] is not x0, "PsfConv.cg does not modify the caller's x0"


def test_pcg_psf_two_band_cube(golden_dir):
    """pcg_psf on a cube whose bands are two pinned cases (zero and non-zero start): each band's pinned x."""
    from pfb_imaging_amd import opt

    p = cp.load(golden_dir)
    cases = [cp.cg_case(p, "37x29_conv"), cp.cg_case(p, "37x29_x0")]
    nxp, nyp = SPECIAL_PAD
    b = np.stack([c["b"] for c in cases])
    x0 = np.stack([np.zeros_like(cases[0]["b"]), cases[1]["x0"]])
    beam = np.stack([c["beam"][0] for c in cases])
    tol, maxit, minit = cases[0]["params"]
    x = opt.pcg_psf(np.ones((2, nxp, nyp // 2 + 1)), b, x0, beam, nyp, 1, cp.ETA, dict(tol=tol, maxit=maxit, minit=minit))
    for k, c in enumerate(cases):
        dx = cp.rel_l2(x[k], c["x"])
        print(f"band {k} ({c['name']}): x {dx:.2e}")
        assert dx <= X_TOL, (k, dx)


# ---- f. power method ----------------------------------------------------------------------------------------------------
def _hess(c, pad):
    from pfb_imaging_amd.operators.hessian import HessPSF

    h = HessPSF(c["nx"], c["ny"], np.ones((2, pad[0], pad[1] // 2 + 1)), beam=np.array(c["beam"]), eta=np.array([cp.ETA, cp.ETA]),
                taper_width=1)
    assert h._plan.uses_rowfft == (pad[0] in ROWFFT and pad[1] in ROWFFT)
    return h


@pytest.fixture(scope="module")
def hessians(golden_dir, monkeypatch_module):
    monkeypatch_module.delenv("PFBHIP_PSF_ROWFFT", raising=False)
    p = cp.load(golden_dir)
    made = {}

    def get(size):
        if size not in made:
            c = cp.pm_case(p, size)
            made[size] = (c, _hess(c, PADS[size]))
        return made[size]

    yield get
    for _, h in made.values():
        h._plan.close()


@pytest.mark.parametrize("run", list(cp.PM_RUNS))
@pytest.mark.parametrize("size", cp.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_power_method_reference_runs(hessians, size, run):
    from pfb_imaging_amd import opt

    c, h = hessians(size)
    pin = c[run]
    tol, maxit = cp.PM_RUNS[run]
    b0 = c["b0"].copy()
    beta, b = opt.power_method(h.dot, c["d"].shape, b0=b0, tol=tol, maxit=maxit, verbosity=0)
    last = opt.power_method.last
    db = _rel(beta, pin["beta"])
    print(f"{size} {run}: iters {last['iters']} status {last['status']} beta {db:.2e}" + (f" b {cp.rel_l2(b, c['b']):.2e}" if run == "fixed" else ""))
    assert (last["iters"], last["status"]) == (pin["iters"], pin["status"]), (last, pin)
    assert db <= 1e-11 and abs(np.linalg.norm(b) - 1.0) <= 1e-12 and np.array_equal(b0, c["b0"])
    if run == "fixed":
        assert cp.rel_l2(b, c["b"]) <= 1e-9


@pytest.mark.parametrize("j", [0, 255, 256, 1073, 2145])
def test_power_method_sentinel(hessians, j):
    """b0 = e_j is an eigenvector: beta = d_j at once, and the second iteration changes nothing (eps == 0 ends the run even
    with tol = 0).  j: the first and last element of the (2, 37, 29) cube, 255 / 256, and the first and last element of band 1.

    eps is exactly zero because the normalisation is exact at these elements: d_j * fl(1 / d_j) == 1 (asserted), so the
    iterate stays e_j up to the transform's 1e-17 leakage, which enters beta squared.  Where that product rounds (element
    1072 of this cube) the second beta may differ in its last bit, and a run with tol = 0 legitimately goes on."""
    from pfb_imaging_amd import opt

    c, h = hessians((37, 29))
    assert c["d"].size == 2146 and c["d"].flat[j] * (1.0 / c["d"].flat[j]) == 1.0
    b0 = np.zeros(c["d"].shape)
    b0.flat[j] = 1.0
    beta, b = opt.power_method(h.dot, b0.shape, b0=b0, tol=0.0, maxit=5, verbosity=0)
    last = opt.power_method.last
    print(f"j={j}: beta - d_j {beta - c['d'].flat[j]:.2e} iters {last['iters']} status {last['status']} eps {last['eps']:.2e}")
    assert abs(beta - c["d"].flat[j]) <= 1e-12 * c["d"].flat[j]
    assert (last["iters"], last["status"], last["eps"]) == (2, 0, 0.0), last


def test_power_method_refuses_a_bad_start(hessians):
    from pfb_imaging_amd import opt

    c, h = hessians((37, 29))
    bad = np.array(c["b0"])
    bad[1, 3, 4] = np.nan
    for b0 in (np.zeros(c["d"].shape), bad):
        with pytest.raises(ValueError, match="non-zero, finite start vector"):
            opt.power_method(h.dot, b0.shape, b0=b0, tol=0.0, maxit=3, verbosity=0)
        beta, _ = opt.power_method(h.dot, b0.shape, b0=c["b0"].copy(), tol=0.0, maxit=8, verbosity=0)   # the operator still works
        assert _rel(beta, c["fixed"]["beta"]) <= 1e-11
