"""The imaging-weight kernels (csrc/weighting.hip) at their edges, against the longdouble restatement of
tests/_weighting_cases.py -- never against another device path.

Every chain case runs through (a) ``uvcell_index``, (b) ``_compute_counts``, (c) ``filter_extreme_counts`` and
``box_sum_counts``, (d) ``counts_to_weights`` -- each step fed with the step before it, as the callers chain them -- and (e) the
fused ``imaging_weights(return_counts=True)`` and, where there is a row, ``VisChunk.imaging_weights``.  The filter and the box
sum also get counts handed in directly (the filter and box cases).

The cell index is compared with ``np.array_equal``; so is every stage of an exact case through the box sum, and through the
final weights when ``robust <= -2`` (see the cases' module docstring for why they are exact).  Everything else is held,
element by element, to ``_weighting_cases.bounds``, and ``counts > 0`` must hold in the same places.  Each test prints the
worst observed error over its bound per stage before it asserts.

Not covered: float32 counts (the reference then computes in float32 while the device widens), negative or NaN input weights,
counts reduced over several ranks.
"""

import warnings

import numpy as np
import pytest

from tests import _weighting_cases as wc

pytestmark = pytest.mark.gpu

CHAIN = sorted(wc.CHAIN)
FILTER, BOX = wc.filter_cases(), wc.box_cases()
DEAD = ["dead-1of3", "dead-1of2", "dead-general"]


def geo(c):
    return c["nx"], c["ny"], c["cell_x"], c["cell_y"]


def sg(c):
    return dict(usign=c["usign"], vsign=c["vsign"])


def case_bounds(c, r):
    return wc.bounds(r["h"], c["sup"], c["nx"] * c["ny"], c["robust"] > -2)


def hold(name, c, r, stages):
    """print, then assert, every stage of ``stages`` (name -> array) against the restatement ``r``"""
    b = case_bounds(c, r)
    exact_to = ("counts", "filtered", "boxed") + (("final", "weights") if c["robust"] <= -2 else ())
    report = []
    for stage, got in stages.items():
        exact = c["exact"] and stage in exact_to
        w = wc.worst(got, r[stage], 0 if exact else b[stage])
        same_sign = stage == "weights" or np.array_equal(got > 0, r[stage] > 0)
        report.append((stage, exact, w, same_sign, got))
        print(f"{name} {stage}: worst error / bound {w:.3f}" + (" (exact)" if exact else f" (bound {b[stage]:.2e})"))
    for stage, exact, w, same_sign, got in report:
        assert got.shape == r[stage].shape and got.dtype == np.float64, stage
        if exact:
            assert np.array_equal(got, r[stage]), stage
        assert w <= 1.0, (stage, w)
        assert same_sign, stage


def step_chain(c):
    """(b) -> (c) -> (d) on the device, one entry after the other; no RuntimeWarning may escape"""
    from pfb_imaging_amd.utils.weighting import _compute_counts, box_sum_counts, counts_to_weights, filter_extreme_counts

    counts = _compute_counts(c["uvw"], c["freq"], c["mask"], c["wgt"], *geo(c), np.float64, **sg(c))
    filtered = filter_extreme_counts(counts.copy(), c["level"])
    boxed = np.array(box_sum_counts(filtered, c["sup"]))
    final, wgt = boxed.copy(), np.array(c["wgt"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        back = counts_to_weights(final, c["uvw"], c["freq"], wgt, c["mask"], *geo(c), c["robust"], **sg(c))
    assert back is wgt
    return dict(counts=counts, filtered=filtered, boxed=boxed, final=final, weights=wgt)


def fused(c):
    from pfb_imaging_amd.utils.weighting import imaging_weights

    wgt = np.array(c["wgt"])
    back, final = imaging_weights(c["uvw"], c["freq"], c["mask"], wgt, *geo(c), c["robust"], filter_level=c["level"],
                                  npix_super=c["sup"], return_counts=True, **sg(c))
    assert back is wgt
    return dict(final=np.array(final), weights=wgt)


def on_the_chunk(c, return_counts=True):
    from pfb_imaging_amd.vischunk import VisChunk

    with VisChunk(c["uvw"], c["freq"], np.zeros(c["wgt"].shape, dtype=np.complex128), c["wgt"], c["mask"]) as ch:
        final = ch.imaging_weights(*geo(c), c["robust"], filter_level=c["level"], npix_super=c["sup"], return_counts=return_counts,
                                   **sg(c))
        return dict(final=None if final is None else np.array(final), weights=ch.weights())


# ---- (a) the cell index ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CHAIN)
def test_cell_index_is_the_restatements(name):
    from pfb_imaging_amd.utils.weighting import uvcell_index

    c, r = wc.chain_case(name), wc.chain_reference(name)
    got = uvcell_index(c["uvw"], c["freq"], c["mask"], *geo(c), c["usign"], c["vsign"])
    assert got.shape == c["mask"].shape and got.dtype == np.int64
    wrong = np.flatnonzero(got.ravel() != r["cell"].ravel())
    print(f"{name}: {wrong.size} of {got.size} indices differ" + (f", first at sample {wrong[0]}" if wrong.size else ""))
    assert np.array_equal(got, r["cell"])


# ---- (b) - (d) the steps ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CHAIN)
def test_steps_against_the_restatement(name):
    c, r = wc.chain_case(name), wc.chain_reference(name)
    got = step_chain(c)
    hold(name, c, r, got)
    if not r["changed"]:
        assert got["weights"].tobytes() == c["wgt"].tobytes() and not got["final"].any()


@pytest.mark.parametrize("name", sorted(FILTER))
def test_filter_on_counts_handed_in(name):
    from pfb_imaging_amd.utils.weighting import filter_extreme_counts

    counts, level, _, bound = FILTER[name]
    got = np.array(counts)
    assert filter_extreme_counts(got, level) is got
    ref = wc.ref_filter(counts, level).astype(np.float64)
    w = wc.worst(got, ref, bound)
    print(f"{name}: worst error / bound {w:.3f}; {int((got != counts).sum())} cells raised, the restatement raises {int((ref != counts).sum())}")
    if bound == 0:
        assert np.array_equal(got, ref)
    assert w <= 1.0 and np.array_equal(got > 0, ref > 0)


@pytest.mark.parametrize("name", sorted(BOX))
def test_box_sum_on_counts_handed_in(name):
    from pfb_imaging_amd.utils.weighting import box_sum_counts

    counts, s, bound = BOX[name]
    got = box_sum_counts(np.array(counts), s)
    ref = wc.ref_box(counts, s).astype(np.float64)
    w = wc.worst(got, ref, bound)
    print(f"{name}: worst error / bound {w:.3f}")
    if bound == 0:
        assert np.array_equal(got, ref)
    assert got.shape == counts.shape and w <= 1.0 and np.array_equal(got > 0, ref > 0)


# ---- (e) the fused pipeline, uploading and on the chunk --------------------------------------------------------------------

@pytest.mark.parametrize("name", CHAIN)
def test_fused_pipeline_against_the_restatement(name):
    c, r = wc.chain_case(name), wc.chain_reference(name)
    got = fused(c)
    hold(name, c, r, got)
    if not r["changed"]:
        assert got["weights"].tobytes() == c["wgt"].tobytes() and not got["final"].any()


WITH_ROWS = [n for n in CHAIN if wc.chain_case(n)["mask"].shape[0] >= 1]


def ulps(a, b):
    """(number of entries that differ, largest difference in units of the last place of ``b``)"""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    d = (a != b) & ~(np.isnan(a) & np.isnan(b))
    return int(d.sum()), float((np.abs(a[d] - b[d]) / np.spacing(np.abs(b[d]))).max()) if d.any() else 0.0


@pytest.mark.parametrize("name", WITH_ROWS)
def test_chunk_entry_is_bit_identical_to_the_uploading_entry(name):
    """The resident entry and the uploading one run the same kernels on the same bytes and agree byte for byte: the counts are a
    sorted, segmented sum and the Briggs sums a two-stage reduction, neither with atomics, so the order of the additions
    depends on the input alone.  (With float64 atomics in both, the non-dyadic cases differed in up to 293 entries by 1 to 4
    ulp, changing from run to run.)"""
    c = wc.chain_case(name)
    got, up = on_the_chunk(c), fused(c)
    for what in ("final", "weights"):
        n, worst_ulp = ulps(got[what], up[what])
        print(f"{name} {what}: {n} of {got[what].size} entries differ between the chunk and the uploading entry, by up to {worst_ulp:.0f} ulp")
    assert got["final"].tobytes() == up["final"].tobytes() and got["weights"].tobytes() == up["weights"].tobytes()


@pytest.mark.parametrize("name", WITH_ROWS)
def test_chunk_entry_against_the_restatement(name):
    c, r = wc.chain_case(name), wc.chain_reference(name)
    got = on_the_chunk(c)
    hold(name + " (chunk)", c, r, got)
    if not r["changed"]:
        assert got["weights"].tobytes() == c["wgt"].tobytes() and not got["final"].any()
        quiet = on_the_chunk(c, return_counts=False)
        assert quiet["final"] is None and quiet["weights"].tobytes() == c["wgt"].tobytes()


def test_untouched_cases_are_there():
    untouched = [n for n in CHAIN if not wc.chain_reference(n)["changed"]]
    assert {"all-masked", "all-out-of-range", "all-zero-weight", "nrow0"} <= set(untouched)


def test_no_rows():
    """every entry takes an empty input: arrays of the right shape, zero counts"""
    from pfb_imaging_amd.utils.weighting import _compute_counts, counts_to_weights, imaging_weights, uvcell_index

    c = wc.chain_case("nrow0")
    assert c["mask"].shape == (0, 3)
    shape = (c["wgt"].shape[0], c["nx"], c["ny"])
    cell = uvcell_index(c["uvw"], c["freq"], c["mask"], *geo(c), c["usign"], c["vsign"])
    assert cell.shape == (0, 3) and cell.dtype == np.int64
    counts = _compute_counts(c["uvw"], c["freq"], c["mask"], c["wgt"], *geo(c), np.float64, **sg(c))
    assert counts.shape == shape and not counts.any()
    wgt = np.array(c["wgt"])
    assert counts_to_weights(counts, c["uvw"], c["freq"], wgt, c["mask"], *geo(c), 0.0, **sg(c)) is wgt
    ones = np.ones(shape)   # (counts that would divide, had there been a sample)
    assert counts_to_weights(ones, c["uvw"], c["freq"], wgt, c["mask"], *geo(c), -3.0, **sg(c)).shape == c["wgt"].shape
    for robust in (0.0, -3.0):
        back, final = imaging_weights(c["uvw"], c["freq"], c["mask"], wgt, *geo(c), robust, filter_level=4.0, npix_super=1,
                                      return_counts=True, **sg(c))
        assert back is wgt and back.shape == c["wgt"].shape and final.shape == shape and not np.asarray(final).any()


# ---- dead planes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", DEAD)
def test_dead_plane_counts_are_nan_and_its_weights_untouched(name):
    c, r = wc.chain_case(name), wc.chain_reference(name)
    dead = ~c["wgt"].reshape(c["wgt"].shape[0], -1).any(axis=1)
    assert dead.any() and not dead.all() and c["robust"] > -2
    b = case_bounds(c, r)
    paths = {"steps": step_chain(c), "fused": fused(c), "chunk": on_the_chunk(c)}
    for path, got in paths.items():
        final, wgt = got["final"], got["weights"]
        print(f"{name} {path}: dead planes {np.flatnonzero(dead)}, NaN planes {np.flatnonzero(np.isnan(final).all(axis=(1, 2)))}, "
              f"dead-plane counts {np.unique(final[dead])[:3]}; live weights worst error / bound "
              f"{wc.worst(wgt[~dead], r['weights'][~dead], b['weights']):.3f}")
    for path, got in paths.items():
        final, wgt = got["final"], got["weights"]
        assert np.isnan(final[dead]).all() and np.isfinite(final[~dead]).all(), path
        assert wgt[dead].tobytes() == c["wgt"][dead].tobytes(), path
        assert wc.worst(wgt[~dead], r["weights"][~dead], b["weights"]) <= 1.0, path
        assert wc.worst(final[~dead], r["final"][~dead], b["final"]) <= 1.0, path
        assert not np.array_equal(wgt[~dead], c["wgt"][~dead]), path
    assert np.array_equal(np.isnan(paths["fused"]["final"]), np.isnan(paths["steps"]["final"]))
    assert np.array_equal(np.isnan(paths["fused"]["final"]), np.isnan(r["final"]))


def test_dead_plane_stays_zero_without_the_scaling():
    name = "dead-1of3-unscaled"
    c, r = wc.chain_case(name), wc.chain_reference(name)
    for path, got in (("steps", step_chain(c)), ("fused", fused(c)), ("chunk", on_the_chunk(c))):
        assert not got["final"][1].any() and np.array_equal(got["final"], r["final"]), path
        assert got["weights"][1].tobytes() == c["wgt"][1].tobytes() and np.array_equal(got["weights"], r["weights"]), path
