"""GPU tests of the direct DFT (csrc/dft.hip, dft.py, comps2vis(method="dft"), utils/transients.py inject_transients).

The yardstick is oracle/dft.py, directly where it can be asked (images, the gridder's conventions) and through the numpy
restatement tests/_dft_ref.py -- tied to the oracle by tests/test_dft_cpu.py -- where it cannot (row / channel factors, the
offset, sgn = +1, free positions).

Bound, per visibility:  4 . 2 pi . 2^-52 . T_max . |wgt| sum_s |amp_s rowf chanf| / N_s  with T_max the largest phase of the
case in turns, computed from the case (``_dft_ref.predict`` returns it; the weights of ``_dft_ref.case`` lie in (0.1, 1), so
the factor |wgt| only tightens it).  For ``image`` the same with sum |wgt vis| / N_s.  The restatement forms its phases in
long double; the oracle itself sits at 0.1 - 0.3 of ONE of the four units (test_dft_cpu.py prints it).

Shapes: T = DFT_TILE sources per LDS tile, B = DFT_BLOCK threads (read from the source); nsrc in {1, T-1, T, T+1, 2T+3};
nrow x nchan in {1, B-1, B+1 (nchan = 1), 37 x 5} and, for the strips of ``image``, 301 x 5.
"""

import os
import re

import numpy as np
import pytest

from . import _dft_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "pfb-imaging_amd", "csrc", "dft.hip")).read()
T = int(re.search(r"constexpr int DFT_TILE = (\d+);", _SRC).group(1))
B = int(re.search(r"constexpr int DFT_BLOCK = (\d+);", _SRC).group(1))
assert B % 5 == 1 and T >= 8
NSRC = [1, T - 1, T, T + 1, 2 * T + 3]
SHAPES = [(1, 1), ((B - 1) // 5, 5), (B + 1, 1), (37, 5)]
OPTS = ("rowf", "chanf", "off", "wgt")


def _within(got, want, bound, what):
    err = np.abs(np.asarray(got) - want)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"{what}: max err / bound = {worst:.4f}")
    assert np.all(err <= bound), f"{what}: max err / bound = {worst:.4f}"


def _predict_both(c, use=(), mask=None, **conv):
    """device and restatement with the same options; ``use`` names the optional inputs that are present"""
    from pfb_imaging_amd.dft import DFT

    opts = {k: c[k] for k in use}
    with DFT(c["uvw"], c["freq"], mask) as d:
        got = d.predict(c["lm"], c["amp"], **opts, **conv)
    want, bound = ref.predict(c["uvw"], c["freq"], c["lm"], c["amp"], mask=mask, **opts, **conv)
    return got, want, bound


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("nsrc", NSRC)
def test_predict_at_every_tile_and_block_edge(nsrc, shape):
    c = ref.case(*shape, nsrc, seed=nsrc + shape[0])
    got, want, bound = _predict_both(c)
    assert got.shape == shape and got.dtype == np.complex128 and bound.min() > 0
    _within(got, want, bound, f"plain nsrc={nsrc} {shape}")
    got, want, bound = _predict_both(c, use=OPTS, sgn=+1.0, signs=(1.0, -1.0, 1.0))
    _within(got, want, bound, f"all options nsrc={nsrc} {shape}")


@pytest.mark.parametrize("use", [tuple(k for i, k in enumerate(OPTS[:3]) if n >> i & 1) for n in range(8)], ids=lambda u: "+".join(u) or "none")
def test_predict_with_each_optional_input(use):
    c = ref.case(37, 5, T + 1, seed=21)
    for extra in ((), ("wgt",)):
        got, want, bound = _predict_both(c, use=use + extra)
        _within(got, want, bound, "+".join(use + extra) or "none")


@pytest.mark.parametrize("sgn", [-1.0, 1.0])
def test_predict_under_every_convention(sgn):
    """each flip, do_wgridding / divide_by_n on and off, with a source at l = m = 0 and one at l^2 + m^2 = 0.9"""
    c = ref.case(37, 5, 7, seed=4)
    assert np.all(c["lm"][0] == 0.0) and abs(np.sum(c["lm"][1] ** 2) - 0.9) < 1e-15
    for signs in ((1.0, 1.0, 1.0), (-1.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, -1.0)):
        for do_w, div_n in ((True, True), (True, False), (False, True), (False, False)):
            got, want, bound = _predict_both(c, use=("off",), sgn=sgn, signs=signs, do_wgridding=do_w, divide_by_n=div_n)
            _within(got, want, bound, f"sgn={sgn} signs={signs} w={do_w} n={div_n}")
    # the centre source alone, no w term, no offset: every phase is exactly zero and so is the allowed error
    one = dict(c, lm=c["lm"][:1], amp=c["amp"][:1])
    got, want, bound = _predict_both(one, sgn=sgn)
    assert not bound.any() and np.array_equal(got, want) and np.all(got == c["amp"][0])


def _masks(nrow, nchan):
    rng = np.random.default_rng(8)
    some = (rng.uniform(size=(nrow, nchan)) > 0.2).astype(np.uint8)
    some[[0, nrow // 2, nrow - 1], :] = 0      # whole rows
    some[:, [1, nchan - 1]] = 0                # whole channels
    return dict(none=None, some=some, all=np.zeros((nrow, nchan), dtype=np.uint8))


@pytest.mark.parametrize("which", ["none", "some", "all"])
@pytest.mark.parametrize("device_out", [False, True], ids=["host", "device"])
def test_mask_weights_and_accumulate(which, device_out):
    """accumulate = 0 writes masked samples as 0 (whatever the target held); accumulate = 1 adds and leaves them untouched"""
    from pfb_imaging_amd._lib import DeviceArray
    from pfb_imaging_amd.dft import DFT

    c = ref.case(37, 5, 2 * T + 3, seed=31)
    mask = _masks(37, 5)[which]
    keep = np.ones((37, 5), bool) if mask is None else mask != 0
    base = c["vis"] * 3.0
    with DFT(c["uvw"], c["freq"], mask) as d:
        for use in ((), ("wgt",)):
            want, bound = ref.predict(c["uvw"], c["freq"], c["lm"], c["amp"], mask=mask, **{k: c[k] for k in use})
            for accumulate in (False, True):
                wgt = c["wgt"] if use else None
                if device_out:
                    out = DeviceArray.from_host(base)
                    d.predict(c["lm"], c["amp"], wgt=None if wgt is None else DeviceArray.from_host(wgt), accumulate=accumulate, out=out)
                    got = out.download()
                else:
                    got = d.predict(c["lm"], c["amp"], wgt=wgt, accumulate=accumulate, out=base.copy())
                if accumulate:
                    assert np.array_equal(got[~keep], base[~keep])
                    _within(got[keep], (base + want)[keep], bound[keep], f"accumulate mask={which} wgt={bool(use)}")
                else:
                    assert not got[~keep].any()
                    _within(got, want, bound, f"overwrite mask={which} wgt={bool(use)}")


def _image_case(seed):
    rng = np.random.default_rng(seed)
    c = ref.case(37, 5, seed=seed)
    nx, ny = 12, 10
    dirty = np.zeros((nx, ny))
    dirty[rng.integers(0, nx, T), rng.integers(0, ny, T)] = rng.uniform(0.2, 1.0, T)
    dirty[nx // 2, ny // 2] = 0.7
    return c, dirty, 2.0e-3, 2.5e-3


CONVS = [dict(flip_v=True), dict(flip_u=True), dict(flip_w=True), dict(), dict(flip_v=True, center_x=0.011, center_y=-0.007)]


@pytest.mark.parametrize("conv", CONVS, ids=lambda c: "-".join(sorted(c)) or "none")
def test_stateless_wrappers_against_the_oracle(conv):
    """dft_dirty2vis / dft_vis2dirty with the oracle's keywords against the oracle itself, subsets included"""
    from oracle import dft as odft
    from pfb_imaging_amd.dft import dft_dirty2vis, dft_vis2dirty, lm_of_pixels

    c, dirty, px, py = _image_case(13)
    ix, iy = np.nonzero(dirty)
    lm, su, sv, sw = lm_of_pixels(ix, iy, *dirty.shape, px, py, **conv)
    for do_w, div_n in ((True, True), (True, False), (False, False)):
        kw = dict(do_wgridding=do_w, divide_by_n=div_n, **conv)
        _, bound = ref.predict(c["uvw"], c["freq"], lm, dirty[ix, iy], signs=(su, sv, sw), do_wgridding=do_w, divide_by_n=div_n)
        want = odft.dft_dirty2vis(c["uvw"], c["freq"], dirty, px, py, **kw)
        _within(dft_dirty2vis(c["uvw"], c["freq"], dirty, px, py, **kw), want, bound, f"dirty2vis {kw}")
        rows, chans = np.array([36, 0, 5, 5, 20]), np.array([0, 4, 2, 3, 2])
        sub = dft_dirty2vis(c["uvw"], c["freq"], dirty, px, py, rows=rows, chans=chans, **kw)
        assert sub.shape == (5,)
        _within(sub, odft.dft_dirty2vis(c["uvw"], c["freq"], dirty, px, py, rows=rows, chans=chans, **kw), bound[rows, chans], "pairs")
        mask = _masks(37, 5)["some"]
        want = odft.dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], mask, *dirty.shape, px, py, **kw)
        all_lm = lm_of_pixels(*(a.ravel() for a in np.meshgrid(np.arange(12), np.arange(10), indexing="ij")), 12, 10, px, py, **conv)[0]
        _, bound = ref.image(c["uvw"], c["freq"], all_lm, c["vis"], mask=mask, wgt=c["wgt"], signs=(su, sv, sw), do_wgridding=do_w,
                             divide_by_n=div_n)
        got = dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], mask, *dirty.shape, px, py, **kw)
        assert got.shape == dirty.shape
        _within(got, want, bound.reshape(dirty.shape), f"vis2dirty {kw}")
        sel = dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], mask, *dirty.shape, px, py, pixels=(ix[:5], iy[:5]), **kw)
        assert np.array_equal(sel, got[ix[:5], iy[:5]])


@pytest.mark.parametrize("shape", SHAPES + [(301, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("nsrc", NSRC)
def test_image_at_every_edge_and_twice_the_same(nsrc, shape):
    from pfb_imaging_amd._lib import DeviceArray
    from pfb_imaging_amd.dft import DFT

    c = ref.case(*shape, nsrc, seed=nsrc + shape[0])
    mask = _masks(*shape)["some"] if shape[1] == 5 else None
    with DFT(c["uvw"], c["freq"], mask) as d:
        for kw, wgt in ((dict(), None), (dict(off=c["off"], sgn=+1.0, signs=(1.0, -1.0, -1.0), divide_by_n=False), c["wgt"])):
            got = d.image(c["lm"], c["vis"], wgt=wgt, **kw)
            want, bound = ref.image(c["uvw"], c["freq"], c["lm"], c["vis"], mask=mask, wgt=wgt, **kw)
            assert got.shape == (nsrc,)
            _within(got, want, bound, f"image nsrc={nsrc} {shape} {sorted(kw)}")
            assert np.array_equal(got, d.image(c["lm"], c["vis"], wgt=wgt, **kw))            # bit-identical
            dev = d.image(c["lm"], DeviceArray.from_host(c["vis"]), wgt=None if wgt is None else DeviceArray.from_host(wgt), **kw)
            assert np.array_equal(got, dev)
    if mask is not None:   # everything flagged: exactly nothing
        with DFT(c["uvw"], c["freq"], np.zeros(shape, np.uint8)) as d:
            assert not d.image(c["lm"], c["vis"]).any()


@pytest.mark.parametrize("sgn", [-1.0, 1.0])
def test_image_is_the_adjoint_of_predict(sgn):
    """<predict(a), v> = <a, image(v)> to 8 . 2^-52 . sum |terms|: both sides evaluate the same phases, only the order of the
    sums differs"""
    from pfb_imaging_amd.dft import DFT

    c = ref.case(301, 5, 2 * T + 3, seed=17)
    mask = _masks(301, 5)["some"]
    for div_n in (True, False):
        kw = dict(off=c["off"], sgn=sgn, signs=(1.0, -1.0, 1.0), divide_by_n=div_n)
        with DFT(c["uvw"], c["freq"], mask) as d:
            vis = d.predict(c["lm"], c["amp"], wgt=c["wgt"], **kw)
            img = d.image(c["lm"], c["vis"], wgt=c["wgt"], **kw)
        N = ref.nm1_of(c["lm"][:, 0], c["lm"][:, 1]) + 1.0 if div_n else np.ones(c["amp"].size)
        terms = np.abs(c["amp"] / N).sum() * np.abs(np.where(mask != 0, c["wgt"] * c["vis"], 0.0)).sum()
        lhs, rhs = float(np.sum(vis.conj() * c["vis"]).real), float(np.dot(c["amp"], img))
        print(f"adjointness: |lhs - rhs| / (8 eps sum|terms|) = {abs(lhs - rhs) / (8 * ref.EPS * terms):.4f}")
        assert abs(lhs - rhs) <= 8 * ref.EPS * terms


@pytest.mark.parametrize("region", [False, True], ids=["no-region", "region"])
def test_predict_comps_is_predict_of_the_same_sources(region):
    from pfb_imaging_amd.comps import Comps
    from pfb_imaging_amd.dft import DFT, lm_of_pixels

    rng = np.random.default_rng(5)
    nx, ny, ncomps, nparam = 40, 36, 2 * T + 3, 3
    flat = rng.choice(nx * ny, ncomps, replace=False)
    flat.sort()
    xi, yi = flat // ny, flat % ny
    coeffs, b = rng.normal(size=(nparam, ncomps)), rng.normal(size=nparam)
    keep = rng.uniform(size=(nx, ny)) > 0.4
    c = ref.case(37, 5, seed=6)
    geom = dict(cellx=1.5e-3, celly=1.1e-3, center_x=0.02, center_y=-0.013, flip_u=False, flip_v=True, flip_w=False)
    comps = Comps(nx, ny, xi, yi, coeffs)
    comps.set_region(keep)
    lm, su, sv, sw = lm_of_pixels(xi, yi, nx, ny, **geom)
    amp = b @ coeffs
    if region:
        amp = np.where(keep[xi, yi], amp, 0.0)
    with DFT(c["uvw"], c["freq"]) as d:
        for kw, chans in ((dict(divide_by_n=False), None), (dict(divide_by_n=True, off=c["off"], wgt=c["wgt"][:, 1:4]), slice(1, 4))):
            got = d.predict_comps(comps, b, region=region, chans=chans, **geom, **kw)
            same = d.predict(lm, amp, signs=(su, sv, sw), chans=chans, **kw)
            fs = slice(None) if chans is None else chans
            want, bound = ref.predict(c["uvw"], c["freq"][fs], lm, amp, signs=(su, sv, sw), **kw)
            assert got.shape == (37, c["freq"][fs].size)
            _within(got, same, bound, f"predict_comps vs predict region={region}")
            _within(got, want, bound, f"predict_comps vs restatement region={region}")
    comps.close()


def test_comps2vis_dft_method():
    """two time chunks, two bands in range and one outside it: against the oracle DFT of the rendered images within the
    bound, against method="grid" at the same epsilon within it (relative l2), no plan made; and the empty region mask"""
    from oracle import dft as odft
    from pfb_imaging_amd.dft import lm_of_pixels
    from pfb_imaging_amd.operators.gridder import comps2vis
    from pfb_imaging_amd.utils.modelspec import _parse

    from . import _modelspec_ref as mref
    from ._modelspec_pins import basis_of, c2v_fixture, fit_outputs

    args, region, mds, frange = c2v_fixture()
    coeffs, xi, yi = mds["coefficients"], mds["location_x"], mds["location_y"]
    a = mds["attrs"]
    nx, ny = a["npix_x"], a["npix_y"]
    _, _, _, expr, params, texpr, fexpr, _ = fit_outputs("c2v_fit")
    modelf, tfunc, ffunc = _parse(expr, params, texpr, fexpr)
    basis = basis_of("c2v_fit")
    conv = dict(center_x=a["center_x"], center_y=a["center_y"], flip_u=a["flip_u"], flip_v=a["flip_v"], flip_w=a["flip_w"])
    epsilon = 1e-7

    def oracle(uvw, freq, image):
        return odft.dft_dirty2vis(uvw, freq, image, a["cell_rad_x"], a["cell_rad_x"], do_wgridding=True, divide_by_n=False, **conv)

    def bound_of(uvw, freq, image):
        ix, iy = np.nonzero(image)
        lm, su, sv, sw = lm_of_pixels(ix, iy, nx, ny, a["cell_rad_x"], a["cell_rad_x"], **conv)
        return ref.predict(uvw, freq, lm, image[ix, iy], signs=(su, sv, sw), divide_by_n=False)[1].astype(np.complex128)

    def render(t, f):
        return mref.render(nx, ny, xi, yi, coeffs, basis(t, f))[0]

    want = mref.comps2vis(*args, region, coeffs, xi, yi, nx, ny, render, oracle, nproduct=2, **frange)
    bound = mref.comps2vis(*args, region, coeffs, xi, yi, nx, ny, render, bound_of, nproduct=2, **frange).real
    info = {}
    got = comps2vis(*args, region, mds, modelf, tfunc, ffunc, epsilon=epsilon, product="IQ", info=info, method="dft", **frange)
    assert got.shape == want.shape and got.dtype == np.complex128
    assert info == dict(device_renders=4, host_renders=0, plans=0, dft_predicts=4)         # 2 time chunks x 2 bands in range
    assert np.array_equal(got[..., 0], got[..., 1]) and not got[:, 4:].any() and got[:, :4].all()
    _within(got[:, :4], want[:, :4], bound[:, :4], "comps2vis(dft) vs oracle")
    grid = comps2vis(*args, region, mds, modelf, tfunc, ffunc, epsilon=epsilon, product="IQ", **frange)
    rel = np.linalg.norm(got - grid) / np.linalg.norm(got)
    print(f"comps2vis dft vs grid: rel l2 {rel:.3e} (epsilon {epsilon})")
    assert rel <= epsilon

    # a nonlinear modelf: values formed on the host, the same sum
    def render_nl(t, f):
        image = np.zeros((nx, ny))
        image[xi, yi] = mref.nonlinear_modelf(tfunc(t), ffunc(f), *coeffs)
        return image

    info = {}
    got_n = comps2vis(*args, region, mds, mref.nonlinear_modelf, tfunc, ffunc, product="IQ", info=info, method="dft", **frange)
    assert info == dict(device_renders=0, host_renders=4, plans=0, dft_predicts=4)
    want_n = mref.comps2vis(*args, region, coeffs, xi, yi, nx, ny, render_nl, oracle, nproduct=2, **frange)
    bound_n = mref.comps2vis(*args, region, coeffs, xi, yi, nx, ny, render_nl, bound_of, nproduct=2, **frange).real
    _within(got_n[:, :4], want_n[:, :4], bound_n[:, :4], "comps2vis(dft, nonlinear) vs oracle")

    info = {}
    none = comps2vis(*args, np.zeros_like(region), mds, modelf, tfunc, ffunc, product="IQ", info=info, method="dft", **frange)
    assert none.shape == want.shape and not none.any()
    assert info == dict(device_renders=0, host_renders=0, plans=0, dft_predicts=0)


@pytest.mark.parametrize("with_wdiff", [False, True], ids=["no-wdiff", "wdiff"])
@pytest.mark.parametrize("with_beam", [False, True], ids=["no-beam", "beam"])
def test_inject_transients(with_wdiff, with_beam):
    """against the literal restatement of the reference's step; allowed: the device's bound plus the restatement's own
    float64 phase error, which ``_dft_ref.inject`` derives, plus one rounding of the result for the additions into the data"""
    from pfb_imaging_amd.utils.transients import generate_transient_spectra, inject_transients

    rng = np.random.default_rng(12)
    c = ref.case(B + 45, 5, seed=40)
    nrow = B + 45
    cases = ref.transient_cases()
    all_times, all_freqs, _ = cases["gaussian"]
    sources = []
    for tag, (l, m) in (("gaussian", (0.03, -0.02)), ("step_periodic", (-0.11, 0.07)), ("exponential", (0.0, 0.0))):
        tprofile, fprofile = generate_transient_spectra(all_times, all_freqs, cases[tag][2])
        sources.append(dict(l=l, m=m, time_profile=tprofile, freq_profile=fprofile))
    time = np.sort(rng.uniform(all_times[0] - 5.0, all_times[-1] + 5.0, nrow))
    data = np.stack([c["vis"], 2 * c["vis"]], axis=-1)
    w_diff = c["off"][:, None] if with_wdiff else None
    beam = rng.uniform(0.3, 1.0, (3, 5)) if with_beam else None
    want, own = ref.inject(data, c["uvw"], c["freq"], time, sources, all_times, all_freqs, w_diff=w_diff, beam=beam)
    bound = own.copy()
    for k, s in enumerate(sources):
        chanf = np.interp(c["freq"], all_freqs, s["freq_profile"]) * (1.0 if beam is None else beam[k])
        bound += ref.predict(c["uvw"], c["freq"], np.array([[s["l"], s["m"]]]), np.ones(1), rowf=np.interp(time, all_times, s["time_profile"])[None],
                             chanf=chanf[None], off=None if w_diff is None else c["off"], divide_by_n=False)[1]
    w_before = None if w_diff is None else w_diff.copy()
    got = inject_transients(data.copy(), c["uvw"], c["freq"], time, sources, all_times, all_freqs, w_diff=w_diff, beam=beam)
    assert np.array_equal(got[:, :, 1], data[:, :, 1]) and (w_diff is None or np.array_equal(w_diff, w_before))
    assert np.abs(got[:, :, 0] - data[:, :, 0]).max() > 0.5
    _within(got[:, :, 0], want[:, :, 0], bound + ref.EPS * np.abs(want[:, :, 0]), f"inject wdiff={with_wdiff} beam={with_beam}")
