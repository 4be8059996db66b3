"""The cases of tests/_weighting_cases.py hold what their names promise, and the oracle's C loops (oracle/weighting.py,
oracle/pfb_oracle.c) agree with that module's longdouble restatement of the imaging-weight chain: the cell index bit for bit
everywhere, every stage bit for bit on the exact cases and within ``bounds`` elsewhere.  No GPU."""

import warnings

import numpy as np
import pytest

from oracle import weighting as ow
from tests import _weighting_cases as wc

CHAIN = sorted(wc.CHAIN)
FILTER, BOX = wc.filter_cases(), wc.box_cases()


def geo(c):
    return c["nx"], c["ny"], c["cell_x"], c["cell_y"]


def sg(c):
    return dict(usign=c["usign"], vsign=c["vsign"])


@pytest.mark.parametrize("name", CHAIN)
def test_case_holds_what_its_name_promises(name):
    c = wc.chain_case(name)
    have = wc.census(c)
    print(name, have)
    for key, want in c["promises"].items():
        if key in wc.EXACT_PROMISES:
            assert have[key] == want, (key, have[key], want)
        else:
            assert have[key] >= want, (key, have[key], want)
    if c["exact"]:
        assert np.array_equal(c["wgt"] * 1024, np.round(c["wgt"] * 1024)) and (c["wgt"] < 64).all()
        assert c["level"] in (0.0, 4.0, 8.0)


def test_the_classes_of_cases_are_all_there():
    """every shape, sign pair, correlation count and robustness the chain is tested at, so that none can be dropped unnoticed"""
    cases = [wc.chain_case(n) for n in CHAIN]
    shapes = {c["mask"].shape for c in cases}
    assert {(0, 3), (1, 1), (51, 5), (64, 4), (257, 1), (67, 5), (300, 1)} <= shapes
    assert {c["wgt"].shape[0] for c in cases} == {1, 2, 3, 4}
    for signs in wc.DEFAULT_SIGNS:
        assert any(c["exact"] and (c["usign"], c["vsign"]) == signs for c in cases)
        assert any(not c["exact"] and (c["usign"], c["vsign"]) == signs for c in cases)
    assert {(c["nx"], c["ny"]) for c in cases} >= {(8, 16), (10, 14), (23, 18), (15, 12), (513, 512)}
    assert all(c["cell_x"] != c["cell_y"] for c in cases)
    assert {-3.0, -2.0, float(np.nextafter(-2.0, 0.0)), 0.0, 2.0} <= {c["robust"] for c in cases}
    assert {5.0, 10.0} <= {c["level"] for c in cases if not c["exact"]}
    assert 513 * 512 > 1024 * 256 >= 512 * 512   # the smallest grid past 1024 blocks of 256
    dead = {n: wc.census(wc.chain_case(n))["dead"] for n in CHAIN}
    assert dead["dead-1of3"] == 1 and dead["dead-1of2"] == 1 and dead["all-zero-weight"] == 2
    assert not wc.chain_case("dead-1of3")["wgt"][1].any() and wc.chain_case("dead-1of3")["wgt"][0].all()
    for n in ("exact-(1,-1)", "exact-(-1,1)"):   # a row whose samples straddle a workgroup: 256 is no multiple of 5
        assert wc.chain_case(n)["mask"].shape == (67, 5) and 256 % 5


@pytest.mark.parametrize("name", sorted(FILTER))
def test_filter_case_holds_what_its_name_promises(name):
    counts, level, npos, _ = FILTER[name]
    assert int((counts > 0).sum()) == npos
    ref = wc.ref_filter(counts, level)
    if name == "one-positive":
        assert np.array_equal(ref, counts)
    if name in ("odd", "even"):
        assert npos % 2 == (name == "odd") and not np.array_equal(ref, counts)
    if name == "all-equal":
        assert np.unique(counts[counts > 0]).size == 1
    if name == "tie-at-threshold":
        low = np.median(counts[counts > 0]) / level
        assert (counts == low).sum() == 1 and ((counts > 0) & (counts < low)).sum() == 1
    if name == "not-a-multiple-of-256":
        assert counts.size % 256 and counts.size > 256
    if name == "joint-median":
        per_plane = np.stack([wc.ref_filter(counts[k:k + 1], level)[0] for k in range(counts.shape[0])])
        assert int((per_plane != ref).sum()) == 2


def test_box_cases_hold_what_their_names_promise():
    shapes = {(a.shape[1:], s) for a, s, _ in BOX.values()}
    assert {((5, 9), 1), ((5, 9), 3), ((5, 9), 5), ((5, 9), 9), ((1, 11), 2)} <= shapes
    a, s, _ = BOX["plane-boundaries-s1"]
    assert a.shape[0] == 3 and not a[:, 1:-1].any() and a[:, -1].all() and a[1:, 0].all() and not a[0, 0].any()
    # a window that ran on into the next plane would change the last rows
    flat = wc.ref_box(a.reshape(1, -1, a.shape[2]), s).reshape(a.shape)
    assert not np.array_equal(flat, wc.ref_box(a, s))


@pytest.mark.parametrize("name", CHAIN)
def test_oracle_chain_against_the_restatement(name):
    c, r = wc.chain_case(name), wc.chain_reference(name)
    b = wc.bounds(r["h"], c["sup"], c["nx"] * c["ny"], c["robust"] > -2)
    cell = ow.uvcell_index(c["uvw"], c["freq"], c["mask"], *geo(c), c["usign"], c["vsign"])
    assert np.array_equal(cell, r["cell"])
    counts = ow.compute_counts(c["uvw"], c["freq"], c["mask"], c["wgt"], *geo(c), **sg(c))
    filtered = ow.filter_extreme_counts(counts.copy(), c["level"])
    boxed = np.array(ow.box_sum_counts(filtered, c["sup"]))
    final, wgt = boxed.copy(), np.array(c["wgt"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # the dead plane's 0 / 0 stays inside the oracle
        back = ow.counts_to_weights(final, c["uvw"], c["freq"], wgt, c["mask"], *geo(c), c["robust"], **sg(c))
    assert back is wgt
    stages = dict(counts=counts, filtered=filtered, boxed=boxed, final=final, weights=wgt)
    exact_to = ("counts", "filtered", "boxed") + (("final", "weights") if c["robust"] <= -2 else ())
    for stage, got in stages.items():
        exact = c["exact"] and stage in exact_to
        w = wc.worst(got, r[stage], 0 if exact else b[stage])
        print(f"{name} {stage}: worst error / bound {w:.3f}" + (" (exact)" if exact else f" (bound {b[stage]:.2e})"))
        if exact:
            assert np.array_equal(got, r[stage]), stage
        assert w <= 1.0, stage
        if stage != "weights":
            assert np.array_equal(got > 0, r[stage] > 0), stage
    if not r["changed"]:
        assert wgt.tobytes() == c["wgt"].tobytes() and not final.any()


@pytest.mark.parametrize("name", ["dead-1of3", "dead-1of2", "dead-general"])
def test_restatement_and_oracle_give_nan_on_exactly_the_dead_planes(name):
    c, r = wc.chain_case(name), wc.chain_reference(name)
    dead = ~c["wgt"].reshape(c["wgt"].shape[0], -1).any(axis=1)
    assert dead.any() and not dead.all() and c["robust"] > -2
    final = np.array(r["boxed"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        wgt = ow.counts_to_weights(final, c["uvw"], c["freq"], np.array(c["wgt"]), c["mask"], *geo(c), c["robust"], **sg(c))
    for got in (final, r["final"]):
        assert np.isnan(got[dead]).all() and np.isfinite(got[~dead]).all() and (got[~dead] >= 1).all()
    assert wgt[dead].tobytes() == c["wgt"][dead].tobytes() and r["weights"][dead].tobytes() == c["wgt"][dead].tobytes()
    assert not np.array_equal(wgt[~dead], c["wgt"][~dead])


def test_unscaled_dead_plane_stays_zero():
    c, r = wc.chain_case("dead-1of3-unscaled"), wc.chain_reference("dead-1of3-unscaled")
    assert c["robust"] <= -2 and not r["final"][1].any() and r["final"][0].any() and r["final"][2].any()
    assert r["weights"][1].tobytes() == c["wgt"][1].tobytes()


@pytest.mark.parametrize("name", sorted(FILTER))
def test_oracle_filter_against_the_restatement(name):
    counts, level, _, bound = FILTER[name]
    got = ow.filter_extreme_counts(np.array(counts), level)
    ref = wc.ref_filter(counts, level).astype(np.float64)
    w = wc.worst(got, ref, bound)
    print(f"{name}: worst error / bound {w:.3f}")
    assert w <= 1.0 and np.array_equal(got > 0, ref > 0)


@pytest.mark.parametrize("name", sorted(BOX))
def test_oracle_box_sum_against_the_restatement(name):
    counts, s, bound = BOX[name]
    got = ow.box_sum_counts(np.array(counts), s)
    ref = wc.ref_box(counts, s).astype(np.float64)
    w = wc.worst(got, ref, bound)
    print(f"{name}: worst error / bound {w:.3f}")
    assert w <= 1.0 and np.array_equal(got > 0, ref > 0)
