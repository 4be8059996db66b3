"""The CPU oracles of the wavelet dictionary, the imaging weights and the l21 dual update against the reference's own numba
kernels, run as plain Python by tests/golden/make_numba_pins.py (tests/golden/numba_pins.npz).

Bookkeeping, cell indices and counts are integers or exact dyadic sums: ``array_equal``.  For the DWT the pin is the reference
run in 80-bit longdouble; the float64 reference's own distance from it is recorded per case, and the oracle -- the same sums
in another order -- may be at most 4x that far away.  Each test prints its figures before it asserts."""

import numpy as np
import pytest

from oracle import psi as opsi
from oracle import weighting as ow
from tests import _numba_pins as npn


@pytest.fixture(scope="module")
def pins(golden_dir):
    return npn.load(golden_dir)


@pytest.mark.parametrize("tag", npn.PSI_TAGS)
def test_bookkeeping_vs_reference(pins, tag):
    c = npn.psi_case(pins, tag)
    bk = opsi.Bookkeeping(c["nx"], c["ny"], (c["name"],), c["nlevel"])
    for k in ("ix", "iy", "sx", "sy", "spx", "spy"):
        assert np.array_equal(getattr(bk, k)[0], c[k]), k
    assert (bk.ntotx[0], bk.ntoty[0], bk.nxmax, bk.nymax) == (c["ntotx"], c["ntoty"], c["nxmax"], c["nymax"])


@pytest.mark.parametrize("tag", npn.PSI_TAGS)
def test_dwt_idwt_vs_longdouble_reference(pins, tag):
    c = npn.psi_case(pins, tag)
    bk = opsi.Bookkeeping(c["nx"], c["ny"], (c["name"],), c["nlevel"])
    alpha = opsi.dwt2d(c["x"], bk, 0)
    keep = c["c"].copy()
    img = opsi.idwt2d(keep, bk, 0)
    assert np.array_equal(keep, c["c"])
    for what, got, pin, floor in (("dwt", alpha, c["alpha"], c["alpha_floor"]), ("idwt", img, c["img"], c["img_floor"])):
        mx, l2 = npn.dist(got, pin)
        print(f"{tag} {what}: oracle max-abs {mx:.2e} (floor {floor[0]:.2e}) rel-l2 {l2:.2e} (floor {floor[1]:.2e})")
        assert mx <= 4 * floor[0] and l2 <= 4 * floor[1]
    m = npn.margins(c)
    assert not c["alpha"][m].any() and not alpha[m].any()    # the zero pattern of the packed layout


def test_transposed_layout_is_the_transpose(pins):
    """The reference's older dwt2d / idwt2d (copyt, coefficients (ntoty, ntotx)) against its nocopyt pair: both pins are
    longdouble runs rounded to float64, so they differ by roundings of the last place only."""
    tag = str(pins["copyt_case"])
    c = npn.psi_case(pins, tag)
    mx, _ = npn.dist(pins["copyt_alpha"].T, c["alpha"])
    mi, _ = npn.dist(pins["copyt_img"], c["img"])
    print(f"{tag}: copyt vs nocopyt pins, max-abs dwt {mx:.2e} idwt {mi:.2e}")
    assert mx <= 2 * npn.EPS * np.abs(c["alpha"]).max() and mi <= 2 * npn.EPS * np.abs(c["img"]).max()
    o = opsi.Psi(1, c["nx"], c["ny"], (c["name"],), c["nlevel"], transposed=True)
    at = np.zeros((1, 1, o.nymax, o.nxmax))
    o.dot(c["x"][None], at)
    assert npn.dist(at[0, 0, :c["ntoty"], :c["ntotx"]], pins["copyt_alpha"])[0] <= 4 * c["alpha_floor"][0]


@pytest.mark.parametrize("nband", npn.DUAL_NBAND)
def test_dual_update_vs_reference(pins, nband):
    c = npn.dual_case(pins, nband)
    got = opsi.dual_update(c["vp"], c["v"].copy(), c["lam"], c["sigma"], c["w"])
    assert np.array_equal(got, c["out"])
    vt = c["vp"] + c["sigma"] * c["v"]
    assert c["eq"].sum() >= 5 and np.array_equal(got[:, c["eq"]], vt[:, c["eq"]])  # |sum| == lam w: strict >, unscaled


@pytest.mark.parametrize("tag", npn.WGT_TAGS)
def test_weighting_oracle_vs_reference(pins, tag):
    c = npn.wgt_case(pins, tag)
    geo = (c["nx"], c["ny"], c["cell_size"], c["cell_size"])
    sg = dict(usign=c["usign"], vsign=c["vsign"])
    cell = ow.uvcell_index(c["uvw"], c["freq"], c["mask"], *geo, c["usign"], c["vsign"])   # oracle/pfb_oracle.c
    assert np.array_equal(cell, c["cell"])
    assert (cell < 0).sum() > 50 and (cell >= 0).sum() > 200
    counts = ow.compute_counts(c["uvw"], c["freq"], c["mask"], c["wgt"], *geo, **sg)
    assert np.array_equal(counts, c["counts"])
    on = npn.touched(c)
    for rb in npn.ROBUST:
        w = c["imw_in"].copy()
        with np.errstate(all="ignore"):
            ow.counts_to_weights(c["counts"].copy(), c["uvw"], c["freq"], w, c["mask"], *geo, rb, **sg)
        pin = c["imw"][rb]
        assert np.array_equal(w[:, ~on], c["imw_in"][:, ~on]) and np.array_equal(pin[:, ~on], c["imw_in"][:, ~on])
        zero = np.array([c["counts"][k].ravel()[c["cell"]] == 0 for k in range(c["ncorr"])]) & on
        # a count of zero leaves the weight alone (Briggs: the reference divides by 0 * ssq + 1, exactly 1)
        assert zero.any() and np.array_equal(pin[zero], c["imw_in"][zero]) and np.array_equal(w[zero], c["imw_in"][zero])
        if rb == -3:
            assert np.array_equal(w, pin)
        else:
            err = np.abs(w / pin - 1).max()
            print(f"{tag} robust {rb}: oracle vs reference {err / npn.EPS:.2f} eps")
            assert err <= 16 * npn.EPS
    # all-masked: counts.any() is false, the weights come back as they were
    none = np.zeros_like(c["mask"])
    z = ow.compute_counts(c["uvw"], c["freq"], none, c["wgt"], *geo, **sg)
    assert not z.any()
    w = c["imw_in"].copy()
    assert ow.counts_to_weights(z, c["uvw"], c["freq"], w, c["mask"], *geo, 0.0, **sg) is w and np.array_equal(w, c["imw_in"])
