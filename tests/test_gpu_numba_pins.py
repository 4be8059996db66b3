"""The wavelet, imaging-weight and l21 dual-update kernels against the reference's own numba code, run as plain Python by
tests/golden/make_numba_pins.py (tests/golden/numba_pins.npz; nothing here reads the reference).

Psi: the pin is the reference run in 80-bit longdouble; ``*_floor`` is the float64 reference's own distance from it.  Bounds:
relative l2 < 1e-14 (as test_gpu_psi.py against the oracle) and max abs <= 4x the case's floor (the kernels do the same sums in
another order, with FMA contraction).  Multi-basis handles: every slice of dot to its own basis' floor; hdot, a sum over the
bases, to 4x the sum of the members' floors plus one rounding of the running sum per further basis.Weighting: cell indices, counts (exact dyadic sums) and uniform weights (one IEEE division) are
bit-equal; Briggs weights within 16 eps (one ratio of exact sums, a multiply, the multiply-add and the division: about 8
roundings, doubled).  Dual update: dyadic inputs, one multiply and one divide per element: bit-equal.  Each test prints its
figures before it asserts."""

import numpy as np
import pytest

from tests import _numba_pins as npn

pytestmark = pytest.mark.gpu

MULTI = (("db8", "db1"), ("db1", "db8"), ("self",), ("db3", "self"), ("self", "self", "db1"))
MULTI_SIZE, MULTI_LEVEL = (30, 32), 1


@pytest.fixture(scope="module")
def pins(golden_dir):
    return npn.load(golden_dir)


def _dev_dot(band, x, nrep=1):
    """pfbhip_psi_dot_dev into device cubes full of NaN"""
    from pfb_imaging_amd._lib import DeviceArray, check, lib

    xd = DeviceArray.from_host(x)
    outs = []
    for _ in range(nrep):
        ad = DeviceArray.from_host(np.full((band.nbasis, band.nxmax, band.nymax), np.nan))
        check(lib().pfbhip_psi_dot_dev(band._h, xd.ptr, ad.ptr))
        outs.append(ad.download())
        ad.free()
    xd.free()
    return outs


def _dev_hdot(band, cube):
    """pfbhip_psi_hdot_dev into an image full of NaN; returns (image, the input cube as it is afterwards)"""
    from pfb_imaging_amd._lib import DeviceArray, check, lib

    cd = DeviceArray.from_host(cube)
    xd = DeviceArray.from_host(np.full((band.nx, band.ny), np.nan))
    check(lib().pfbhip_psi_hdot_dev(band._h, cd.ptr, xd.ptr))
    res = xd.download(), cd.download()
    cd.free()
    xd.free()
    return res


def _check(what, got, pin, floor_max, extra=0.0):
    mx, l2 = npn.dist(got, pin)
    print(f"{what}: max-abs {mx:.2e} (bound {4 * floor_max + extra:.2e}) rel-l2 {l2:.2e} (bound 1e-14)")
    assert not np.isnan(got).any()
    assert l2 < 1e-14
    assert mx <= 4 * floor_max + extra


@pytest.mark.parametrize("tag", npn.PSI_TAGS)
def test_psi_single_wavelet_vs_reference(pins, tag):
    from pfb_imaging_amd.operators.psi import PsiBand

    c = npn.psi_case(pins, tag)
    g = PsiBand(c["nx"], c["ny"], (c["name"],), c["nlevel"])
    assert (g.nxmax, g.nymax) == (c["nxmax"], c["nymax"])
    ntx, nty = c["ntotx"], c["ntoty"]
    a, a2 = _dev_dot(g, c["x"], nrep=2)
    _check(f"{tag} dot", a[0, :ntx, :nty], c["alpha"], c["alpha_floor"][0])
    zero = np.ones(a.shape[1:], dtype=bool)           # the zero pattern of the packed layout, padding to nxmax / nymax included
    zero[:ntx, :nty] = npn.margins(c)
    assert not a[0][zero].any()
    assert np.array_equal(a2, a)                       # a second dot on the same handle
    cube = np.full((1, g.nxmax, g.nymax), 7.5)         # outside [:ntotx, :ntoty] the reference reads nothing (psi.py:516)
    cube[0, :ntx, :nty] = c["c"]
    img, after = _dev_hdot(g, cube)
    _check(f"{tag} hdot", img, c["img"], c["img_floor"][0])
    assert np.array_equal(after, cube)                 # hdot leaves its input bit-identical
    g.close()


@pytest.mark.parametrize("tag", npn.PSI_TAGS)
def test_psi_transposed_layout_vs_reference(pins, tag):
    """The older ``Psi`` (coefficients (nbasis, nymax, nxmax)) against the transposed pin; for the case the generator also ran
    through the reference's own transposed dwt2d / idwt2d, against that run too."""
    from pfb_imaging_amd.operators.psi import Psi

    c = npn.psi_case(pins, tag)
    p = Psi(1, c["nx"], c["ny"], (c["name"],), c["nlevel"])
    ntx, nty = c["ntotx"], c["ntoty"]
    at = np.full((1, 1, p.nymax, p.nxmax), np.nan)
    p.dot(c["x"][None], at)
    _check(f"{tag} Psi.dot", at[0, 0, :nty, :ntx], c["alpha"].T, c["alpha_floor"][0])
    ct = np.zeros((1, 1, p.nymax, p.nxmax))
    ct[0, 0, :nty, :ntx] = c["c"].T
    xo = np.full((1, c["nx"], c["ny"]), np.nan)
    p.hdot(ct, xo)
    _check(f"{tag} Psi.hdot", xo[0], c["img"], c["img_floor"][0])
    if tag == str(pins["copyt_case"]):
        _check(f"{tag} Psi.dot vs copyt run", at[0, 0, :nty, :ntx], pins["copyt_alpha"], c["alpha_floor"][0])
        _check(f"{tag} Psi.hdot vs copyt run", xo[0], pins["copyt_img"], c["img_floor"][0])


@pytest.mark.parametrize("bases", MULTI, ids="-".join)
def test_psi_multi_basis_vs_reference(pins, bases):
    """Handles of several bases assembled from the single-wavelet pins (PsiBandNocopyt.dot / hdot, psi.py:466-533): a short
    filter after a long one (stale scratch), the accumulating row pass, the identity slice riding on a row pass, and the
    zeroed rectangles when nxmax / nymax come from another basis."""
    from pfb_imaging_amd.operators.psi import PsiBand

    nx, ny = MULTI_SIZE
    cs = [None if b == "self" else npn.psi_case(pins, f"{b}_{MULTI_LEVEL}_{nx}_{ny}") for b in bases]
    x = next((c["x"] for c in cs if c is not None), npn.psi_case(pins, f"db1_{MULTI_LEVEL}_{nx}_{ny}")["x"])
    g = PsiBand(nx, ny, bases, MULTI_LEVEL)
    assert g.nxmax == max([nx] + [c["ntotx"] for c in cs if c]) and g.nymax == max([ny] + [c["ntoty"] for c in cs if c])
    ref = np.zeros((len(bases), g.nxmax, g.nymax))
    cube = np.full(ref.shape, 7.5)
    img_ref = np.zeros((nx, ny))
    floor_i = 0.0
    rng = np.random.default_rng(5)
    for i, c in enumerate(cs):
        if c is None:
            ref[i, :nx, :ny] = x
            cube[i, :nx, :ny] = rng.integers(-4, 5, size=(nx, ny)) / 4.0
            img_ref += cube[i, :nx, :ny]
        else:
            ref[i, :c["ntotx"], :c["ntoty"]] = c["alpha"]
            cube[i, :c["ntotx"], :c["ntoty"]] = c["c"]
            img_ref += c["img"]
            floor_i += c["img_floor"][0]
    a, a2 = _dev_dot(g, x, nrep=2)
    for i, c in enumerate(cs):
        if c is None:
            assert np.array_equal(a[i], ref[i])            # the identity slice: the image, zeros around it
        else:
            _check(f"{bases} dot, slice {i} ({c['name']})", a[i], ref[i], c["alpha_floor"][0])   # each basis to its own floor
            zero = np.ones(a.shape[1:], dtype=bool)        # the layout's margins and the padding up to the largest basis
            zero[:c["ntotx"], :c["ntoty"]] = npn.margins(c)
            assert not a[i][zero].any()
    assert np.array_equal(a2, a)
    img, after = _dev_hdot(g, cube)
    _check(f"{bases} hdot", img, img_ref, floor_i, extra=(len(bases) - 1) * npn.EPS * np.abs(img_ref).max())
    assert np.array_equal(after, cube)
    g.close()


@pytest.mark.parametrize("tag", npn.WGT_TAGS)
def test_weighting_vs_reference(pins, tag):
    from pfb_imaging_amd.utils.weighting import _compute_counts, counts_to_weights, uvcell_index

    c = npn.wgt_case(pins, tag)
    geo = (c["nx"], c["ny"], c["cell_size"], c["cell_size"])
    sg = dict(usign=c["usign"], vsign=c["vsign"])
    cell = uvcell_index(c["uvw"], c["freq"], c["mask"], *geo, c["usign"], c["vsign"])
    assert np.array_equal(cell, c["cell"])
    for ngrid in (1, 3):
        counts = _compute_counts(c["uvw"], c["freq"], c["mask"], c["wgt"], *geo, np.float64, ngrid=ngrid, **sg)
        assert np.array_equal(counts, c["counts"])
    on = npn.touched(c)
    zero = np.array([c["counts"][k].ravel()[c["cell"]] == 0 for k in range(c["ncorr"])]) & on
    assert zero.any() and (~on).sum() > 50
    for rb in npn.ROBUST:
        w = c["imw_in"].copy()
        with np.errstate(all="ignore"):
            res = counts_to_weights(c["counts"].copy(), c["uvw"], c["freq"], w, c["mask"], *geo, rb, **sg)
        assert res is w
        pin = c["imw"][rb]
        assert np.array_equal(w[:, ~on], c["imw_in"][:, ~on])       # masked or out of range: untouched
        # a count of zero: untouched (Briggs: the reference divides by 0 * ssq + 1, exactly 1)
        assert np.array_equal(pin[zero], c["imw_in"][zero]) and np.array_equal(w[zero], c["imw_in"][zero])
        if rb == -3:
            assert np.array_equal(w, pin)
        else:
            err = np.abs(w / pin - 1).max()
            print(f"{tag} robust {rb}: {err / npn.EPS:.2f} eps (bound 16)")
            assert err <= 16 * npn.EPS
    none = np.zeros_like(c["mask"])                                 # all-masked: counts.any() is false
    z = _compute_counts(c["uvw"], c["freq"], none, c["wgt"], *geo, np.float64, **sg)
    assert not z.any()
    assert np.array_equal(uvcell_index(c["uvw"], c["freq"], none, *geo, c["usign"], c["vsign"]), np.full(cell.shape, -1))
    w = c["imw_in"].copy()
    assert counts_to_weights(z, c["uvw"], c["freq"], w, c["mask"], *geo, 0.0, **sg) is w and np.array_equal(w, c["imw_in"])


@pytest.mark.parametrize("nband", npn.DUAL_NBAND)
def test_dual_update_vs_reference(pins, nband):
    """dual_update_numba_fast and the two-phase device pair: bit-equal (every vtilde and band sum is exact for these dyadic
    inputs, contraction or not; the scale is one division, the update one multiply).  Where |sum| == lam w the reference's
    strict > leaves vtilde unscaled."""
    from pfb_imaging_amd import prox

    c = npn.dual_case(pins, nband)
    vt = c["vp"] + c["sigma"] * c["v"]
    got = c["v"].copy()
    prox.dual_update_numba_fast(c["vp"], got, c["lam"], c["sigma"], c["w"])
    assert np.array_equal(got, c["out"])
    assert np.array_equal(got[:, c["eq"]], vt[:, c["eq"]]) and c["eq"].sum() >= 5
    two = c["v"].copy()
    s = prox._vtilde_sum_gpu(c["vp"].copy(), two, c["sigma"])      # pfbhip_l21_vtilde_sum_dev
    assert np.array_equal(two, vt) and np.array_equal(s, vt.sum(axis=0))
    prox._scale_gpu(two, c["lam"], np.ascontiguousarray(c["w"]), np.ascontiguousarray(s))   # pfbhip_l21_scale_dev
    assert np.array_equal(two, c["out"])
