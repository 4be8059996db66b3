"""``VisChunk.average`` (pfb_imaging_amd.vischunk, csrc/chunkavg.hip) against its numpy restatement in longdouble
(tests/_chunkavg_ref.py).

Bounds (u = 2^-53, n = |K| the unmasked input samples of an output sample).  A sum of n terms in any order is within
(n - 1) u sum|terms| of the exact sum; each product and the final quotient add one rounding each.  So
  * ``wgt_out`` is held to n u wgt_out (the weights are non-negative);
  * each part of ``vis_out`` to (n + 3) u sum_K wgt |vis| / wgt_out, element-wise -- in sum|terms|, not in |result|: the inputs
    have magnitude 1 and random phases, so cancellation inside a bin is real;
  * ``mask_out`` is compared exactly, and outputs of all-flagged and dead-weight bins are exact zeros.
Every case prints its largest error as a fraction of the bound.

Inputs: weights in [0.5, 2], 20 % of the samples masked -- with visibilities and weights that would show if they were read
--, row 3 (where there is one) fully flagged, the last correlation of row 2 with dead weights.

Block edges.  The kernels have one thread per output sample (chan_bin = 1 and chan_bin > 64) or one per input channel of an
output sample (2 <= chan_bin <= 64; a bin owns chan_bin rounded up to a power of two lanes), in 256-thread blocks, and NO
grid stride: no thread takes a second step, so there is no size "one past the second stride".  The edges are the thread
counts 255, 256 and 257 of either kernel (the nearest counts on either side where the second kernel's count is a multiple
of its lanes per bin), and 65 and 130 channels at chan_bin = 64, where a row takes two and three whole waves.
"""

import numpy as np
import pytest

from pfb_imaging_amd.utils import synth
from tests import _chunkavg_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


def inputs(ncorr, nrow, nchan, seed=0):
    rng = np.random.default_rng(1000 * nrow + 10 * nchan + ncorr + seed)
    vis = np.exp(2j * np.pi * rng.random((ncorr, nrow, nchan)))
    wgt = rng.uniform(0.5, 2.0, (ncorr, nrow, nchan))
    mask = (rng.random((nrow, nchan)) > 0.2).astype(np.uint8)
    if nrow > 3:
        mask[3] = 0
        wgt[-1, 2] = 0.0
        mask[2, 0] = 1
    for a in (vis, wgt, mask):
        a.setflags(write=False)
    return vis, wgt, mask


def device_average(vis, wgt, mask, chan_bin, row_map=None, nrow_out=None, twice=False):
    """``(vis_out, wgt_out, mask_out)`` of the device, after checking that the receiver is bit-unchanged (and, with ``twice``,
    that a second call gives the same bits)"""
    from pfb_imaging_amd.vischunk import VisChunk

    ncorr, nrow, nchan = vis.shape
    with VisChunk(np.zeros((nrow, 3)), 1.0 + np.arange(nchan), vis, wgt, mask) as ch:
        outs = []
        for _ in range(2 if twice else 1):
            with ch.average(chan_bin, row_map, nrow_out) as av:
                assert av is not ch and (av.ncorr, av.nchan) == (ncorr, -(-nchan // chan_bin))
                outs.append((av.vis.download(), av.wgt.download(), av.mask.download()))
                assert np.array_equal(outs[-1][2], av.mask_host)
        assert ch.vis.download().tobytes() == vis.tobytes() and ch.wgt.download().tobytes() == wgt.tobytes()
        assert ch.mask.download().tobytes() == mask.tobytes()
    if twice:
        for a, b in zip(*outs):
            assert a.tobytes() == b.tobytes()
    return outs[0]


def hold_to_bounds(got, want, label):
    gv, gw, gm = got
    rv, rw, rm, absum, n = want
    assert gv.shape == rv.shape[:-1] and gw.shape == rw.shape and gm.shape == rm.shape
    assert np.array_equal(gm, rm)
    zero = rw == 0                                  # all-flagged (n == 0) and dead-weight outputs
    assert not gv[zero].any() and not gw[zero].any()
    live = ~zero
    nn = np.broadcast_to(n[None], rw.shape)[live].astype(LD)
    ew = np.abs(LD(1) * gw[live] - rw[live])
    bw = nn * U * rw[live]
    bv = (nn + 3) * U * absum[live] / rw[live]
    ere = np.abs(LD(1) * gv.real[live] - rv[..., 0][live])
    eim = np.abs(LD(1) * gv.imag[live] - rv[..., 1][live])
    fw = float((ew / bw).max()) if live.any() else 0.0
    fv = float(np.maximum(ere / bv, eim / bv).max()) if live.any() else 0.0
    print(f"{label}: {int(live.sum())} live outputs, n up to {int(n.max(initial=0))}; wgt error {fw:.3f} of its bound, "
          f"vis error {fv:.3f} of its bound")
    assert (ew <= bw).all()
    assert (ere <= bv).all() and (eim <= bv).all()


# ---- channel bins, identity map -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ncorr", [1, 2, 4])
@pytest.mark.parametrize("nchan,chan_bin", [(8, 2), (8, 8), (8, 16), (10, 4), (65, 64), (130, 64), (9, 3), (11, 5), (67, 65)])
def test_channel_bins_with_the_identity_map(ncorr, nchan, chan_bin):
    vis, wgt, mask = inputs(ncorr, 7, nchan)
    got = device_average(vis, wgt, mask, chan_bin, twice=True)
    hold_to_bounds(got, ref.average(vis, wgt, mask, chan_bin), f"ncorr={ncorr} nchan={nchan} chan_bin={chan_bin}")


def gathered(vis, wgt, mask, rows):
    """rows ``rows`` of the inputs, masked samples as exact zeros: what chan_bin = 1 with one member per bin must give"""
    m = mask[rows]
    return np.where(m != 0, vis[:, rows], 0.0), np.where(m != 0, wgt[:, rows], 0.0), (m != 0).astype(np.uint8)


@pytest.mark.parametrize("ncorr", [1, 2, 4])
@pytest.mark.parametrize("nchan", [1, 5])
def test_chan_bin_one_with_a_dropping_map_is_a_pure_gather_bit_for_bit(ncorr, nchan):
    vis, wgt, mask = inputs(ncorr, 7, nchan)
    vis, mask = vis.copy(), mask.copy()
    vis[0, 0, 0], mask[0, 0] = complex(-0.0, 1.0), 1  # (a signed zero survives a gather)
    wgt = np.where(wgt == 0.0, 1.25, wgt)  # (a dead weight zeroes its output: not a gather)
    for row_map, rows in ((np.array([0, -1, 1, 2, -1, 3, 4]), [0, 2, 3, 5, 6]),       # drops rows
                          (np.array([6, 4, -1, 5, 0, 1, 2]), [4, 5, 6, 0, 1, 3, 0]),  # reorders; output 3 has no members
                          ):
        nrow_out = len(rows)
        got = device_average(vis, wgt, mask, 1, row_map, nrow_out)
        want = list(gathered(vis, wgt, mask, rows))
        empty = [R for R in range(nrow_out) if R not in row_map]
        for a in want[:2]:
            a[:, empty] = 0
        want[2][empty] = 0
        for g, w, name in zip(got, want, ("vis", "wgt", "mask")):
            assert g.tobytes() == np.ascontiguousarray(w).tobytes(), (name, row_map)
        hold_to_bounds(got, ref.average(vis, wgt, mask, 1, row_map, nrow_out), f"gather ncorr={ncorr} nchan={nchan}")


# ---- row bins ------------------------------------------------------------------------------------------------------------------

# 11 rows: output 0 <- {4}, output 1 <- nothing, output 2 <- {1, 9}, output 3 <- {0, 2, 3, 5, 7, 8, 10}, row 6 dropped, output 4 <- nothing
ROW_MAP = np.array([3, 2, 3, 3, 0, 3, -1, 3, 3, 2, 3])


@pytest.mark.parametrize("ncorr", [1, 2, 4])
@pytest.mark.parametrize("chan_bin", [1, 2])
def test_row_bins_of_one_two_and_seven_members_a_dropped_row_and_empty_outputs(ncorr, chan_bin):
    vis, wgt, mask = inputs(ncorr, 11, 5)
    mask = mask.copy()
    mask[[1, 9], 2:4] = 0      # every member of output 2 masked in channels 2 and 3 (one channel bin at chan_bin = 2) only
    mask[[1, 9], 0] = 1
    got = device_average(vis, wgt, mask, chan_bin, ROW_MAP, 5, twice=True)
    want = ref.average(vis, wgt, mask, chan_bin, ROW_MAP, 5)
    assert not want[2][[1, 4]].any() and want[2][2, 0] == 1 and want[2][2, 2 // chan_bin] == 0 and want[4].max() >= 4
    hold_to_bounds(got, want, f"rows ncorr={ncorr} chan_bin={chan_bin}")


@pytest.mark.parametrize("chan_bin", [1, 2])
def test_rows_with_data_drops_three_fully_flagged_rows_of_eleven(chan_bin):
    from pfb_imaging_amd.vischunk import VisChunk

    vis, wgt, mask = inputs(2, 11, 5)
    mask = mask.copy()
    mask[[0, 3, 10]] = 0
    mask[[1, 2, 4, 5, 6, 7, 8, 9], 1] = 1
    uvw = np.random.default_rng(1).standard_normal((11, 3))
    with VisChunk(uvw, 1.0 + np.arange(5), vis, wgt, mask) as ch:
        row_map = ch.rows_with_data()
        assert np.array_equal(row_map, [-1, 0, 1, -1, 2, 3, 4, 5, 6, 7, -1])
        with ch.average(chan_bin, row_map) as av:
            got = av.vis.download(), av.wgt.download(), av.mask.download()
            assert av.nrow == 8 and np.array_equal(av.uvw, uvw[row_map >= 0])
            assert np.array_equal(av.freq, ref.channel_bins(ch.freq, chan_bin)[0]) and av.chan_width is None
    hold_to_bounds(got, ref.average(vis, wgt, mask, chan_bin, row_map), f"rows_with_data chan_bin={chan_bin}")


def test_uvw_freq_and_chan_width_of_the_new_chunk():
    from pfb_imaging_amd.vischunk import VisChunk

    vis, wgt, mask = inputs(1, 11, 5)
    rng = np.random.default_rng(2)
    uvw, freq, width = rng.standard_normal((11, 3)), 1e9 + 1e6 * np.arange(5), np.full(5, 1e6)
    given = rng.standard_normal((5, 3))
    with VisChunk(uvw, freq, vis, wgt, mask) as ch:
        with ch.average(2, ROW_MAP, 5, chan_width=width) as av:
            np.testing.assert_allclose(av.uvw, ref.mean_uvw(uvw, ROW_MAP, 5), rtol=0, atol=1e-14)  # (7 terms of size 1, two orders)
            assert not av.uvw[[1, 4]].any()
            assert np.array_equal(av.freq, [1e9 + 0.5e6, 1e9 + 2.5e6, 1e9 + 4e6]) and np.array_equal(av.chan_width, [2e6, 2e6, 1e6])
        with ch.average(1, ROW_MAP, 5, uvw_out=given) as av:
            assert np.array_equal(av.uvw, given) and np.array_equal(av.freq, freq)


# ---- block edges ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nthreads", [255, 256, 257])
def test_block_edges_of_the_thread_per_output_kernel(nthreads):
    """``nthreads`` output samples, one thread each: at chan_bin = 66 > 64, and at chan_bin = 1 with a row map"""
    nrow = nthreads  # nchan = 66, chan_bin = 66: one output per row
    vis, wgt, mask = inputs(2, nrow, 66)
    hold_to_bounds(device_average(vis, wgt, mask, 66), ref.average(vis, wgt, mask, 66), f"per-output, {nthreads} threads")
    row_map = np.arange(nrow + 1) - 1  # chan_bin = 1: drops row 0, nrow outputs of one channel
    vis, wgt, mask = inputs(1, nrow + 1, 1)
    got = device_average(vis, wgt, mask, 1, row_map)
    hold_to_bounds(got, ref.average(vis, wgt, mask, 1, row_map), f"per-output gather, {nthreads} threads")
    assert got[2][-1] == mask[-1] and got[1][0, -1, 0] == wgt[0, -1, 0] * (mask[-1, 0] != 0)


@pytest.mark.parametrize("nthreads", [255, 256, 257])
def test_block_edges_of_the_thread_per_input_channel_kernel(nthreads):
    """Thread counts around ``nthreads``.  chan_bin = 2 (2 lanes a bin): 5 channels are 3 bins, 6 lanes a row, so 42 and 43 rows
    (252 and 258 threads) stand on either side of 255; 2 channels x 128 rows are 256 threads, x 129 rows 258; 1 channel x 129
    rows 258 with every second lane idle.  chan_bin = 3 (4 lanes a bin, one idle): 3 channels x 63, 64, 65 rows are 252, 256,
    260 threads."""
    shapes = {255: [(42, 5, 2), (43, 5, 2), (63, 3, 3)], 256: [(128, 2, 2), (64, 3, 3)], 257: [(129, 2, 2), (129, 1, 2), (65, 3, 3)]}[nthreads]
    for nrow, nchan, chan_bin in shapes:
        vis, wgt, mask = inputs(2, nrow, nchan)
        hold_to_bounds(device_average(vis, wgt, mask, chan_bin), ref.average(vis, wgt, mask, chan_bin),
                       f"per-input, {nrow} x {nchan}, chan_bin={chan_bin}")
        row_map = np.arange(nrow) // 2  # pairs of rows as well
        hold_to_bounds(device_average(vis, wgt, mask, chan_bin, row_map), ref.average(vis, wgt, mask, chan_bin, row_map),
                       f"per-input with row pairs, {nrow} x {nchan}, chan_bin={chan_bin}")


# ---- the C entry's refusals --------------------------------------------------------------------------------------------------

def test_the_entry_refuses_bad_arguments_and_writes_nothing():
    from pfb_imaging_amd._lib import DeviceArray, check, lib, ptr

    ncorr, nrow, nchan, nrow_out = 2, 4, 3, 2
    vis, wgt, mask = inputs(ncorr, nrow, nchan)
    made = [DeviceArray.from_host(a) for a in (vis, wgt, mask)]
    sentinels = [np.full((ncorr, nrow, nchan), 7.0 + 7.0j), np.full((ncorr, nrow, nchan), 7.0), np.full((nrow, nchan), 7, dtype=np.uint8)]
    made += [DeviceArray.from_host(a) for a in sentinels]  # (large enough for every output shape below)
    dv, dw, dm, ov, ow, om = made
    row_start, members = np.array([0, 2, 3]), np.array([0, 2, 1])
    good = dict(vis=dv.ptr, wgt=dw.ptr, mask=dm.ptr, ncorr=ncorr, nrow=nrow, nchan=nchan, chan_bin=2, row_start=row_start,
                members=members, nkept=3, nrow_out=nrow_out, vis_out=ov.ptr, wgt_out=ow.ptr, mask_out=om.ptr)
    bad = [
        dict(vis=None), dict(wgt=None), dict(mask=None), dict(vis_out=None), dict(wgt_out=None), dict(mask_out=None),
        dict(members=None),
        dict(ncorr=0), dict(ncorr=65536),
        dict(chan_bin=0), dict(chan_bin=-1),
        dict(row_start=np.array([1, 2, 3])),                    # row_start[0] != 0
        dict(row_start=np.array([0, 3, 2]), nkept=2),           # decreasing
        dict(row_start=np.array([0, 2, 2])),                    # row_start[nrow_out] != nkept
        dict(row_start=np.array([0, 2, 4]), nkept=4, members=np.array([0, 2, 1, 4])),    # member == nrow
        dict(members=np.array([0, 2, -1])),                     # member < 0
        dict(members=np.array([2, 0, 1])),                      # descending inside a bin
        dict(members=np.array([2, 2, 1])),                      # not STRICTLY ascending
        dict(row_start=None, members=None, nkept=nrow),         # identity with nrow_out != nrow
        dict(vis_out=dv.ptr), dict(wgt_out=dw.ptr), dict(mask_out=dm.ptr), dict(wgt_out=dv.ptr),   # outputs alias inputs
        dict(wgt_out=ov.ptr),                                   # two outputs overlap
    ]
    try:
        for change in bad:
            kw = dict(good, **change)
            rs, mem = (None if kw[k] is None else np.ascontiguousarray(kw[k], dtype=np.int64) for k in ("row_start", "members"))
            status = lib().pfbhip_chunk_average_dev(kw["vis"], kw["wgt"], kw["mask"], kw["ncorr"], kw["nrow"], kw["nchan"],
                                                    kw["chan_bin"], ptr(rs), ptr(mem), kw["nkept"], kw["nrow_out"], kw["vis_out"],
                                                    kw["wgt_out"], kw["mask_out"])
            assert status == 1, change  # PFBHIP_ERR_INVALID
            with pytest.raises(ValueError):
                check(status)
            for d, s in zip((ov, ow, om), sentinels):
                assert d.download().tobytes() == s.tobytes(), change
        for d, a in zip((dv, dw, dm), (vis, wgt, mask)):
            assert d.download().tobytes() == a.tobytes()
        # the unchanged arguments pass, and write the outputs' leading (ncorr, 2, 2) / (2, 2) elements
        rs, mem = row_start.astype(np.int64), members.astype(np.int64)
        check(lib().pfbhip_chunk_average_dev(dv.ptr, dw.ptr, dm.ptr, ncorr, nrow, nchan, 2, ptr(rs), ptr(mem), 3, nrow_out, ov.ptr,
                                             ow.ptr, om.ptr))
        want = ref.average(vis, wgt, mask, 2, np.array([0, 1, 0, -1]), 2)
        assert np.array_equal(om.download().reshape(-1)[:4].reshape(2, 2), want[2])
    finally:
        for d in made:
            d.free()


# ---- from raw correlations -------------------------------------------------------------------------------------------------

def raw_case(nrow=38, nchan=5, nc=4):
    """Raw correlations of the kind tests/test_gpu_stokes.py runs: time bins (9, 1, 27) from row 100 with a gap at row 10,
    diagonal Jones terms, 7 antennas, 30 % of the correlations flagged and rows 3, 20 and 37 flagged throughout."""
    from tests import _stokes_ref

    rng = np.random.default_rng(1000 * nrow + 10 * nchan + nc)
    tbin_idx, tbin_counts = np.array([100, 109, 100 + nrow - 27]), np.array([9, 1, 27])
    data = rng.standard_normal((nrow, nchan, nc)) + 1j * rng.standard_normal((nrow, nchan, nc))
    weight = rng.uniform(0.1, 2.0, (nrow, nchan, nc))
    flag = rng.random((nrow, nchan, nc)) < 0.3
    flag[[3, 20, 37]] = True
    jones = _stokes_ref.random_jones(rng, (3, 7, nchan, 1), False)
    ant1, ant2 = rng.integers(0, 7, nrow), rng.integers(0, 7, nrow)
    return data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2


def test_from_weight_data_with_averaging_equals_from_weight_data_then_average():
    from pfb_imaging_amd.vischunk import VisChunk

    raw = raw_case()
    nrow, nchan = raw[0].shape[:2]
    s = synth.make_case(nrow, nchan, 32, zscale=0.2, seed=3, with_vis=False)
    width = np.full(nchan, 2.5e5)
    tail = ("linear", "IQ", "4", "l2")
    with VisChunk.from_weight_data(s["uvw"], s["freq"], *raw, *tail, chan_average=2, drop_flagged_rows=True, chan_width=width) as one:
        got = one.vis.download(), one.wgt.download(), one.mask.download(), one.uvw, one.freq, one.chan_width
        assert one.nchan == 3 and one.nrow < nrow - 2
    with VisChunk.from_weight_data(s["uvw"], s["freq"], *raw, *tail) as first:
        assert first.nrow == nrow and first.chan_width is None and not first.mask_host[[3, 20, 37]].any()
        with first.average(2, first.rows_with_data(), chan_width=width) as two:
            want = two.vis.download(), two.wgt.download(), two.mask.download(), two.uvw, two.freq, two.chan_width
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    assert np.array_equal(got[5], [5e5, 5e5, 2.5e5]) and got[2].any()
    # the defaults change nothing, and so does dropping where no row is fully flagged
    with VisChunk.from_weight_data(s["uvw"], s["freq"], *raw, *tail, chan_average=1, drop_flagged_rows=False) as same:
        assert same.nrow == nrow and same.nchan == nchan


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def test_products_of_an_averaged_chunk_equal_the_products_of_host_averaged_arrays():
    """The case of tests/test_gpu_vischunk.py (3000 rows x 2 channels, 5 % flagged, several w-planes; ncorr = 2 with vis = [v,
    conj v] and wgt = [w, 1]) averaged over both channels, which lie close in uv, after dropping the rows without data.  The
    bounds are DESIGN §17.3's for another rounding in front of the same arithmetic."""
    from pfb_imaging_amd.operators.gridder import image_data_products_arrays, image_data_products_chunk
    from pfb_imaging_amd.vischunk import VisChunk

    c = synth.make_case(3000, 2, 40, zscale=0.2, seed=11)
    cell = c["cell"] * 30.0
    vis = np.stack([c["vis"], c["vis"].conj()])
    wgt = np.stack([c["wgt"], np.ones_like(c["wgt"])])
    mask = np.array(c["mask"], dtype=np.uint8)
    mask[[5, 1700]] = 0  # (two rows without data for certain)
    args = (40, 40, 80, 80, cell, cell)
    with VisChunk(c["uvw"], c["freq"], vis, wgt, mask) as ch:
        row_map = ch.rows_with_data()
        with ch.average(2, row_map) as av:
            assert av.nchan == 1 and av.nrow == int(mask.any(1).sum()) < 3000
            uvw_out, freq_out = av.uvw, av.freq
            got, _ = image_data_products_chunk(av, *args)
    rv, rw, rm, _, count = ref.average(vis, wgt, mask, 2, row_map)
    hv, hw = ref.to_double(rv, rw)
    assert np.array_equal(uvw_out, c["uvw"][row_map >= 0]) and freq_out[0] == c["freq"].mean()
    want, _ = image_data_products_arrays(uvw_out, freq_out, hv, hw, rm, *args)
    n = int((rm != 0).sum())
    for key in ("DIRTY", "PSF"):
        r = ref.rel(got[key], want[key])
        print(f"{key}: averaged chunk vs host-averaged arrays {r:.3e}")
        assert got[key].shape == want[key].shape and r < 1e-10
    live = rm != 0
    np.testing.assert_allclose(got["WEIGHT"][:, live], want["WEIGHT"][:, live], rtol=1e-11)
    assert np.array_equal(got["MASK"], rm)
    assert (np.abs(got["WSUM"] - want["WSUM"]) <= n * U * want["WSUM"]).all()
