"""CPU tests of the direct-DFT layer: the pixel -> direction mapping and the numpy restatement against the oracle
(oracle/dft.py), the transient profiles against the reference-run pins (tests/golden/transient_pins.npz), and the shape checks
that must fire before any device call."""

import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

from . import _dft_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _image_case(nx=12, ny=10, seed=3):
    rng = np.random.default_rng(seed)
    c = ref.case(nrow=37, nchan=5, seed=seed)
    dirty = np.zeros((nx, ny))
    ix, iy = rng.integers(0, nx, 9), rng.integers(0, ny, 9)
    dirty[ix, iy] = rng.uniform(0.2, 1.0, 9)
    dirty[nx // 2, ny // 2] = 0.7          # the phase centre itself
    return c, dirty, 2.0e-3, 2.5e-3


FLIPS = [dict(flip_v=True), dict(flip_u=True), dict(flip_w=True), dict(), dict(flip_v=True, center_x=0.011, center_y=-0.007),
         dict(flip_u=True, flip_v=True, flip_w=True, center_x=-0.004, center_y=0.009)]


@pytest.mark.parametrize("conv", FLIPS, ids=lambda c: "-".join(sorted(c)) or "none")
@pytest.mark.parametrize("do_wgridding,divide_by_n", [(True, True), (True, False), (False, False)])
def test_lm_of_pixels_reproduces_the_oracle(conv, do_wgridding, divide_by_n):
    """lm_of_pixels + the restated sum == oracle.dft.dft_dirty2vis of the same image.  The oracle sits within 0.04 of
    2 pi 2^-52 T_max sum|amp| of a long-double evaluation; the restatement is that evaluation, so one such unit bounds them."""
    from oracle import dft as odft
    from pfb_imaging_amd.dft import lm_of_pixels

    c, dirty, px, py = _image_case()
    want = odft.dft_dirty2vis(c["uvw"], c["freq"], dirty, px, py, do_wgridding=do_wgridding, divide_by_n=divide_by_n, **conv)
    ix, iy = np.nonzero(dirty)
    lm, su, sv, sw = lm_of_pixels(ix, iy, *dirty.shape, px, py, **conv)
    assert (su, sv, sw) == tuple(-1.0 if conv.get(k) else 1.0 for k in ("flip_u", "flip_v", "flip_w"))
    got, bound = ref.predict(c["uvw"], c["freq"], lm, dirty[ix, iy], signs=(su, sv, sw), sgn=-1.0, do_wgridding=do_wgridding,
                             divide_by_n=divide_by_n)
    err = np.abs(got - want)
    print(f"max err / (2 pi eps T_max sum|amp|) = {np.max(err / (bound / 4)):.3f}")
    assert bound.min() > 0 and np.all(err <= bound / 4)


def test_restated_image_is_the_oracles_vis2dirty():
    from oracle import dft as odft
    from pfb_imaging_amd.dft import lm_of_pixels

    c, dirty, px, py = _image_case(seed=5)
    mask = (np.random.default_rng(1).uniform(size=c["vis"].shape) > 0.3).astype(np.uint8)
    ix, iy = np.nonzero(dirty)
    for conv in FLIPS[:2] + FLIPS[4:5]:
        want = odft.dft_vis2dirty(c["uvw"], c["freq"], c["vis"], c["wgt"], mask, *dirty.shape, px, py, pixels=(ix, iy), **conv)
        lm, su, sv, sw = lm_of_pixels(ix, iy, *dirty.shape, px, py, **conv)
        got, bound = ref.image(c["uvw"], c["freq"], lm, c["vis"], mask=mask, wgt=c["wgt"], signs=(su, sv, sw), sgn=-1.0)
        assert np.all(np.abs(got - want) <= bound / 4)


def test_restatement_is_self_adjoint_and_uses_every_option():
    """<predict(a), v> == <a, image(v)> for the restatement with off and sgn = +1 (what the oracle cannot be asked), and the
    row / channel factors act as an outer product."""
    c = ref.case(nsrc=5, seed=9)
    kw = dict(off=c["off"], signs=(1.0, -1.0, 1.0), sgn=+1.0, divide_by_n=True)
    vis, _ = ref.predict(c["uvw"], c["freq"], c["lm"], c["amp"], wgt=c["wgt"], **kw)
    img, _ = ref.image(c["uvw"], c["freq"], c["lm"], c["vis"], wgt=c["wgt"], **kw)
    lhs, rhs = np.sum(vis.conj() * c["vis"]).real, np.dot(c["amp"], img)
    assert abs(lhs - rhs) <= 1e-12 * np.abs(c["amp"]).sum() * np.abs(c["vis"]).sum()
    one, _ = ref.predict(c["uvw"], c["freq"], c["lm"][:1], c["amp"][:1], rowf=c["rowf"][:1], chanf=c["chanf"][:1], **kw)
    bare, _ = ref.predict(c["uvw"], c["freq"], c["lm"][:1], c["amp"][:1], **kw)
    assert np.allclose(one, bare * c["rowf"][0][:, None] * c["chanf"][0][None, :], rtol=1e-14, atol=0)


@pytest.mark.parametrize("tag", sorted(ref.transient_cases()))
def test_transient_profiles_match_the_reference_run(tag):
    """The mirror is the reference's numpy expressions: equal to the last bit."""
    from pfb_imaging_amd.utils import transients as tr

    p = np.load(os.path.join(HERE, "golden", "transient_pins.npz"))
    times, freqs, params = ref.transient_cases()[tag]
    tprofile, fprofile = tr.generate_transient_spectra(times, freqs, params)
    assert np.array_equal(tprofile, p[f"{tag}_time"]) and np.array_equal(fprofile, p[f"{tag}_freq"])
    t = params["time"]
    assert np.array_equal(tr.generate_time_profile(times - times[0], t["peak_time"], t["duration"], t["shape"]), p[f"{tag}_pulse"])
    if "periodic" in tag:
        assert tprofile.sum() > 2 * p[f"{tag}_pulse"].sum()       # (the pulse does repeat)
    f = params["frequency"]
    assert np.array_equal(tr.generate_frequency_profile(np.array([0.8e9, 1.2e9, 2.0e9]), f["peak_flux"], f["reference_freq"],
                                                        f["spectral_index"]), p["power_law"])
    with pytest.raises(ValueError):
        tr.generate_time_profile(times, 1.0, 1.0, "boxcar")


def _bare_handle(nrow, nchan):
    """A DFT object with its sizes and no device behind it: whatever reaches the library through it fails loudly"""
    from pfb_imaging_amd.dft import DFT

    d = object.__new__(DFT)
    d.nrow, d.nchan, d._h = nrow, nchan, None
    return d


def test_shape_errors_raise_before_any_device_call():
    from pfb_imaging_amd import dft
    from pfb_imaging_amd.operators.gridder import comps2vis
    from pfb_imaging_amd.utils.transients import inject_transients

    c = ref.case()
    with pytest.raises(ValueError):
        dft.DFT(c["uvw"][:, :2], c["freq"])
    with pytest.raises(ValueError):
        dft.DFT(c["uvw"], c["freq"][None, :])
    with pytest.raises(ValueError):
        dft.DFT(c["uvw"], c["freq"], mask=np.ones((37, 4)))
    with pytest.raises(ValueError):
        dft.lm_of_pixels(np.arange(3), np.arange(4), 8, 8, 1e-3, 1e-3)
    with pytest.raises(ValueError):
        dft.dft_dirty2vis(c["uvw"], c["freq"], np.ones(4), 1e-3, 1e-3)
    with pytest.raises(ValueError):
        dft.dft_dirty2vis(c["uvw"], c["freq"], np.ones((4, 4)), 1e-3, 1e-3, rows=np.arange(3))
    d = _bare_handle(37, 5)
    good = dict(lm=c["lm"], amp=c["amp"])
    for bad in (dict(good, amp=c["amp"][:-1]), dict(good, lm=c["lm"].T), dict(good, rowf=c["rowf"].T), dict(good, chanf=c["chanf"][:, :4]),
                dict(good, off=c["off"][:-1]), dict(good, wgt=c["wgt"][:, :4]), dict(good, signs=(1.0, 1.0)), dict(good, signs=(1.0, 0.5, 1.0)),
                dict(good, sgn=0.0), dict(good, accumulate=True), dict(good, out=np.zeros((37, 5))), dict(good, chans=slice(5, 5)),
                dict(good, chans=slice(0, 4, 2)), dict(good, chans=slice(1, 3), chanf=c["chanf"])):
        with pytest.raises(ValueError):
            d.predict(**bad)
    for bad in (dict(lm=c["lm"], vis=c["vis"][:, :4]), dict(lm=c["lm"][:, :1], vis=c["vis"]), dict(lm=c["lm"], vis=c["vis"], wgt=c["wgt"][:3])):
        with pytest.raises(ValueError):
            d.image(**bad)
    with pytest.raises(ValueError):
        comps2vis(*[None] * 14, method="auto")
    data = np.zeros((37, 5, 1), dtype=np.complex128)
    time = np.arange(37.0)
    src = [dict(l=0.01, m=0.0, time_profile=np.ones(3), freq_profile=np.ones(2))]
    for bad in (dict(data=data[:, :4]), dict(data=data.real), dict(time=time[:-1]), dict(beam=np.ones((2, 5)))):
        kw = dict(dict(data=data, uvw=c["uvw"], freq=c["freq"], time=time, sources=src, all_times=np.arange(3.0), all_freqs=c["freq"][:2]),
                  **bad)
        with pytest.raises(ValueError):
            inject_transients(**kw)


def test_conv_struct_layout_matches_header(tmp_path):
    from pfb_imaging_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pfbhip.h"\nint main(void){\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(pfbhip_dft_conv), offsetof(pfbhip_dft_conv, sgn),'
                   " offsetof(pfbhip_dft_conv, do_wgridding), offsetof(pfbhip_dft_conv, accumulate), offsetof(pfbhip_dft_conv, chan0));\n"
                   "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    C = _lib.DFTConv
    assert out == [ct.sizeof(C), C.sgn.offset, C.do_wgridding.offset, C.accumulate.offset, C.chan0.offset]


def test_cabi_refuses_bad_arguments_without_a_device():
    """argument errors come back through the status channel before anything touches the device"""
    from pfb_imaging_amd import _lib

    L = _lib.lib()
    h = ct.c_void_p()
    uvw, freq = np.zeros((2, 3)), np.ones(2)
    assert L.pfbhip_dft_create(ct.c_int64(0), ct.c_int64(2), _lib.ptr(uvw), _lib.ptr(freq), None, ct.byref(h)) == 1
    assert L.pfbhip_dft_create(ct.c_int64(2), ct.c_int64(2), None, _lib.ptr(freq), None, ct.byref(h)) == 1 and not h.value
    assert L.pfbhip_dft_predict(None, None, ct.c_int64(0), None, None, None, None, None, None, None) == 1
    assert L.pfbhip_dft_image(None, None, ct.c_int64(0), None, None, None, None, None) == 1
    assert L.pfbhip_dft_destroy(None) == 0
