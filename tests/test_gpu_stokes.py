"""Device ``weight_data`` (pfb_imaging_amd.utils.weighting, csrc/stokes.hip) against the numpy oracle (tests/_stokes_ref.py).

Tolerances.  Double precision: errors are measured per sample against the oracle's scales (``_stokes_ref.sample_scales``: the
norm of the sample's four Stokes visibilities, its largest Stokes weight) and must stay within 8 d, d the rounding scale
that test_stokes_cpu.py prints (the oracle through adjugates against the oracle through matrix inverses): the device
evaluates the same algebra in a third order, without contraction.  Single precision: the outputs are f64 results rounded
once, so each real and imaginary part lies within 1.2e-7 of the magnitude of the oracle's value on the same rounded inputs.
Flagged and uncovered samples are exactly zero.

Shapes are the smallest at which the kernel can go wrong: nchan = 5 (several rows in one wave), 1, 70 (a row crosses a
64-lane wave) and nrow = 3, nchan = 257 (a row crosses a 256-lane workgroup; 771 samples are no multiple of it).  Time bins
(9, 1, 27) count from 100.  They cover 37 rows exactly, so the shapes that must leave a row outside every bin have 38 rows
and a gap before the last bin (row 10); nrow = 37 is run too, fully covered.
"""

import functools

import numpy as np
import pytest

from tests import _stokes_ref as ref

pytestmark = pytest.mark.gpu

NANT = 7
SP_TOL = 1.2e-7
PRODUCTS4 = ("I", "Q", "U", "V", "IQ", "QU", "UV", "IQUV", "VQI")
COMBOS = [(4, full, pol, product) for full in (False, True) for pol in ("linear", "circular") for product in PRODUCTS4]
COMBOS += [(2, False, "linear", p) for p in ("I", "Q", "IQ")] + [(2, False, "circular", p) for p in ("I", "V", "VI")]
SHAPES = [(37, 5), (38, 5), (38, 1), (38, 70), (3, 257)]
FLAGS = ("none", "all", "random", "row", "channel")


def bins_of(nrow):
    if nrow >= 37:
        return np.array([100, 109, 100 + nrow - 27]), np.array([9, 1, 27])
    return np.array([100, 102]), np.array([1, 1])  # rows 0 and 2 of 3


def flags_of(rng, kind, shape):
    flag = np.zeros(shape, dtype=bool)
    if kind == "all":
        flag[:] = True
    elif kind == "random":
        flag = rng.random(shape) < 0.3  # per correlation: a sample with any of them set is dropped
    elif kind == "row":
        flag[shape[0] // 2] = True
    elif kind == "channel":
        flag[:, shape[1] // 2] = True
    return flag


@functools.lru_cache(maxsize=None)
def case(nrow, nchan, nc, full, flags, seed=0):
    rng = np.random.default_rng(1000 * nrow + 10 * nchan + nc + seed)
    tbin_idx, tbin_counts = bins_of(nrow)
    data = rng.standard_normal((nrow, nchan, nc)) + 1j * rng.standard_normal((nrow, nchan, nc))
    weight = rng.uniform(0.1, 2.0, (nrow, nchan, nc))
    jones = ref.random_jones(rng, (tbin_idx.size, NANT, nchan, 1), full)
    ant1, ant2 = rng.integers(0, NANT, nrow), rng.integers(0, NANT, nrow)
    ant2[::5] = ant1[::5]  # autocorrelations: p == q
    out = (data, weight, flags_of(rng, flags, data.shape), jones, tbin_idx, tbin_counts, ant1, ant2)
    for a in out:
        a.setflags(write=False)
    return out


def live_samples(args):
    flag, nrow = args[2], args[0].shape[0]
    return (ref.row_to_bin(args[4], args[5], nrow) >= 0)[:, None] & ~flag.any(axis=-1)


def check_double(args, pol, product, got_vis, got_wgt, label):
    want_vis, want_wgt, vscale, wscale = ref.weight_data(*args, pol, product, full_stokes=True)
    assert got_vis.shape == want_vis.shape and got_vis.dtype == np.complex128
    assert got_wgt.shape == want_wgt.shape and got_wgt.dtype == np.float64
    dead = ~live_samples(args)
    assert not got_vis[dead].any() and not got_wgt[dead].any(), f"{label}: flagged or uncovered samples are not zero"
    ev = (np.abs(got_vis - want_vis) / vscale[..., None]).max() if got_vis.size else 0.0
    ew = (np.abs(got_wgt - want_wgt) / wscale[..., None]).max() if got_wgt.size else 0.0
    d = ref.rounding_scale()
    print(f"{label}: vis {ev:.2e}, wgt {ew:.2e}, d = {d:.2e}, bound {8 * d:.2e}")
    assert ev <= 8 * d and ew <= 8 * d, label


def check_single(args, pol, product, got_vis, got_wgt, label):
    rounded = (args[0].astype(np.complex64), args[1].astype(np.float32)) + tuple(args[2:])
    want_vis, want_wgt = ref.weight_data(*rounded, pol, product)
    assert got_vis.shape == want_vis.shape and got_vis.dtype == np.complex64 and got_wgt.dtype == np.float32
    dead = ~live_samples(args)
    assert not got_vis[dead].any() and not got_wgt[dead].any(), f"{label}: flagged or uncovered samples are not zero"
    mag = np.abs(want_vis)
    er = (np.abs(got_vis.real - want_vis.real) - SP_TOL * mag).max() if mag.size else -1.0
    ei = (np.abs(got_vis.imag - want_vis.imag) - SP_TOL * mag).max() if mag.size else -1.0
    ew = (np.abs(got_wgt - want_wgt) - SP_TOL * np.abs(want_wgt)).max() if mag.size else -1.0
    rel = (np.abs(got_vis - want_vis)[mag > 0] / mag[mag > 0]).max() if (mag > 0).any() else 0.0
    print(f"{label}: single precision, largest |error| / |value| = {rel:.2e}")
    assert er <= 0.0 and ei <= 0.0 and ew <= 0.0, label


@pytest.mark.parametrize("nc,full,pol,product", COMBOS, ids=lambda v: str(v))
def test_every_admitted_combination(nc, full, pol, product):
    from pfb_imaging_amd.utils.weighting import weight_data

    args = list(case(38, 5, nc, full, "random"))
    ants32 = (len(product) + nc) % 2 == 0  # both index widths over the sweep
    args[6], args[7] = (a.astype(np.int32 if ants32 else np.int64) for a in args[6:8])
    label = f"nc={nc} {'full' if full else 'diag'} {pol} {product}"
    vis, wgt = weight_data(*args, pol, product, str(nc), "l2")
    assert vis.shape == (38, 5, len(product))
    check_double(args, pol, product, vis, wgt, label)
    vis, wgt = weight_data(args[0].astype(np.complex64), args[1].astype(np.float32), *args[2:], pol, product, str(nc), "l2")
    check_single(args, pol, product, vis, wgt, label)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_flag_patterns(shape, flags):
    from pfb_imaging_amd.utils.weighting import weight_data

    for nc, full, pol, product in ((4, True, "linear", "IQUV"), (4, False, "circular", "V"), (2, False, "linear", "IQ")):
        args = case(*shape, nc, full, flags)
        label = f"{shape} {flags} nc={nc} {'full' if full else 'diag'} {pol} {product}"
        live = live_samples(args)
        if flags == "all":
            assert not live.any()
        elif shape[0] != 37:
            assert not live[10 if shape[0] == 38 else 1].any()  # the row outside every bin
        vis, wgt = weight_data(*args, pol, product, str(nc), "l2")
        check_double(args, pol, product, vis, wgt, label)
        if shape in ((38, 70), (3, 257)):
            vis, wgt = weight_data(args[0].astype(np.complex64), args[1].astype(np.float32), *args[2:], pol, product, str(nc), "l2")
            check_single(args, pol, product, vis, wgt, label)


def test_readonly_noncontiguous_inputs_and_no_rows():
    from pfb_imaging_amd.utils.weighting import as_contiguous_readonly_view, weight_data

    args = case(38, 5, 4, True, "random")
    want = weight_data(*args, "linear", "IQUV", "4", "l2")  # (every array of `case` is read-only)
    # the same values behind strides: reversed rows of a padded buffer, Fortran order, every second element
    strided = []
    for a in args:
        big = np.zeros(tuple(2 * n for n in a.shape), dtype=a.dtype)
        big[tuple(slice(None, None, 2) for _ in a.shape)] = a
        view = big[tuple(slice(None, None, 2) for _ in a.shape)]
        assert not view.flags.c_contiguous or a.size <= 1
        view.setflags(write=False)
        strided.append(view)
    got = weight_data(*strided, "linear", "IQUV", "4", "l2")
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    got = weight_data(*(as_contiguous_readonly_view(np.asfortranarray(a)) for a in args), "linear", "IQUV", "4", "l2")
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    # more than one direction in jones: only direction 0 is read
    two = np.concatenate([args[3], np.full_like(args[3], np.nan)], axis=3)
    got = weight_data(*args[:3], two, *args[4:], "linear", "IQUV", "4", "l2")
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    # nothing to do
    zeros = np.zeros(3, dtype=np.int64)
    empty = weight_data(args[0][:0], args[1][:0], args[2][:0], args[3], zeros, zeros, args[6][:0], args[7][:0], "linear", "IQ", "4", "l2")
    assert empty[0].shape == (0, 5, 2) and empty[0].dtype == np.complex128 and empty[1].shape == (0, 5, 2)
    # no bins: everything is uncovered, and zero
    none = weight_data(*args[:4], np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), *args[6:], "linear", "I", "4", "l2")
    assert none[0].shape == (38, 5, 1) and not none[0].any() and not none[1].any()


@pytest.mark.parametrize("nc,full,pol,product", [(4, True, "circular", "IQUV"), (4, False, "linear", "QU"), (2, False, "circular", "V")])
def test_device_outputs_correlation_first_and_mask(nc, full, pol, product):
    from pfb_imaging_amd.utils.weighting import weight_data, weight_data_dev

    args = case(3, 257, nc, full, "random")
    vis, wgt = weight_data(*args, pol, product, str(nc), "l2")
    dvis, dwgt, dmask = weight_data_dev(*args, pol, product, str(nc), "l2")
    ns = len(product)
    assert dvis.shape == (ns, 3, 257) and dvis.dtype == np.complex128 and dwgt.shape == (ns, 3, 257) and dmask.shape == (3, 257)
    assert (dvis.download() == vis.transpose(2, 0, 1)).all() and (dwgt.download() == wgt.transpose(2, 0, 1)).all()
    mask = dmask.download()
    assert mask.dtype == np.uint8 and (mask == ~args[2].any(axis=-1)).all()
    assert mask[1].any()  # the mask speaks of flags only: row 1 is in no bin and still unflagged somewhere
    dvis, dwgt, none = weight_data_dev(*args, pol, product, str(nc), "l2", corr_first=False, with_mask=False)
    assert none is None and dvis.shape == (3, 257, ns)
    assert (dvis.download() == vis).all() and (dwgt.download() == wgt).all()


@pytest.mark.parametrize("full", [False, True], ids=["diagonal gains", "full jones"])
def test_polarised_point_source_end_to_end(full):
    """The reference's tests/test_polproducts.py at a test's size: predict a polarised point source, corrupt the coherencies
    with antenna gains, undo them in weight_data, grid, and read the flux back off the dirty image."""
    from pfb_imaging_amd.dft import DFT, lm_of_pixels
    from pfb_imaging_amd.utils import synth
    from pfb_imaging_amd.utils.stokes import stokes_to_corr
    from pfb_imaging_amd.utils.weighting import weight_data
    from pfb_imaging_amd.wgridder import Gridder

    flux = {"I": 1.0, "Q": 0.6, "U": 0.3, "V": 0.1}
    npix, nrow, nchan, nt = 64, 900, 2, 3
    locx, locy = 3 * npix // 4, npix // 4
    c = synth.make_case(nrow=nrow, nchan=nchan, npix=npix, zscale=0.05, seed=11, with_vis=False)
    rng = np.random.default_rng(420)
    conv = dict(flip_u=False, flip_v=True, flip_w=False)
    lm, su, sv, sw = lm_of_pixels([locx], [locy], npix, npix, c["cell"], c["cell"], **conv)
    with DFT(c["uvw"], c["freq"]) as d:
        unit = d.predict(lm, np.ones(1), signs=(su, sv, sw), sgn=-1.0, do_wgridding=True, divide_by_n=False)
    stokes_vis = np.stack([flux[s] * unit for s in "IQUV"], axis=-1)
    model = stokes_to_corr(stokes_vis, axis=2).reshape(nrow, nchan, 2, 2)
    tbin_idx, tbin_counts = np.arange(nt) * (nrow // nt), np.full(nt, nrow // nt)
    ant1, ant2 = rng.integers(0, NANT, nrow), rng.integers(0, NANT, nrow)
    jones = ref.random_jones(rng, (nt, NANT, nchan, 1), full)
    jm = jones[:, :, :, 0] if full else ref.full_of_diag(jones[:, :, :, 0])
    t = np.repeat(np.arange(nt), nrow // nt)
    gp, gq = jm[t, ant1], jm[t, ant2]  # (nrow, nchan, 2, 2)
    data = (gp @ model @ gq.conj().swapaxes(-1, -2)).reshape(nrow, nchan, 4)
    weight = rng.uniform(0.5, 1.5, (nrow, nchan, 4))
    flag = rng.random((nrow, nchan, 4)) < 0.02
    g = Gridder(c["uvw"], c["freq"], None, npix_x=npix, npix_y=npix, pixsize_x=c["cell"], pixsize_y=c["cell"], epsilon=1e-7,
                do_wgridding=True, divide_by_n=False, **conv)
    try:
        for product in ("I", "Q", "U", "V", "IQUV"):
            vis, wgt = weight_data(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, "linear", product, "4", "l2")
            for k, s in enumerate(product):
                dirty = g.vis2dirty(np.ascontiguousarray(vis[:, :, k]), np.ascontiguousarray(wgt[:, :, k]))
                got = dirty[locx, locy] / wgt[:, :, k].sum()
                print(f"{product}[{s}]: {got:.8f} for {flux[s]}")
                np.testing.assert_allclose(got, flux[s], rtol=1e-4, atol=1e-4)
    finally:
        g.close()
