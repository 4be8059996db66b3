"""CPU tests of Hogbom / Clark CLEAN: the yardstick's analytic cases, the argument checks of deconv.hogbom / deconv.clark
(raised before any GPU work), the C-ABI symbols and the info-struct layout."""

import ctypes as ct
import math
import os
import subprocess

import numpy as np
import pytest

from tests import _clean_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gauss_psf(nxp, nyp, sx, sy=None, peak=1.0):
    sy = sx if sy is None else sy
    x = np.arange(nxp)[:, None] - nxp // 2
    y = np.arange(nyp)[None, :] - nyp // 2
    return peak * np.exp(-0.5 * (x / sx) ** 2 - 0.5 * (y / sy) ** 2)


def test_yardstick_point_source_iteration_count():
    """One source of flux F under a peak-1 PSF: k = ceil(log pf / log(1 - gamma)) iterations, model F (1 - (1 - gamma)^k)."""
    nx, ny, F, gamma, pf = 24, 20, 3.0, 0.1, 0.1
    psf = _gauss_psf(2 * nx, 2 * ny, 2.0)[None]
    dirty = F * psf[:, nx - 7:2 * nx - 7, ny - 5:2 * ny - 5]  # source at (7, 5)
    model, _, k, status = ref.hogbom(dirty, psf, gamma=gamma, pf=pf, maxit=1000)
    kexp = math.ceil(math.log(pf) / math.log(1 - gamma))
    assert k == kexp and status == 0
    assert np.flatnonzero(model[0]).tolist() == [7 * ny + 5]
    assert model[0, 7, 5] == pytest.approx(F * (1 - (1 - gamma) ** k), rel=1e-12)


def test_yardstick_equal_peaks_in_row_major_order():
    nx, ny = 16, 12
    dirty = np.zeros((1, nx, ny))
    dirty[0, 9, 2] = dirty[0, 3, 8] = 1.0  # (3, 8) comes first in row-major order
    psf = np.zeros((1, 2 * nx, 2 * ny))
    psf[0, nx, ny] = 1.0
    model, _, k, status = ref.hogbom(dirty, psf, gamma=0.5, pf=0.1, maxit=1)
    assert (k, status) == (1, 1)
    assert np.flatnonzero(model[0]).tolist() == [3 * ny + 8]
    model, _, _, _ = ref.hogbom(dirty, psf, gamma=0.5, pf=0.1, maxit=2)
    assert np.flatnonzero(model[0]).tolist() == [3 * ny + 8, 9 * ny + 2]


def test_yardstick_clark_recovers_point_sources():
    """The major cycle of the yardstick with a symmetric PSF: components on the sources, residual below pf x peak."""
    rng = np.random.default_rng(1)
    nband, nx, ny = 2, 32, 28
    psf = np.stack([_gauss_psf(2 * nx, 2 * ny, s) for s in (1.5, 2.0)])
    psfhat = np.fft.rfft2(np.fft.ifftshift(psf, axes=(1, 2)), axes=(1, 2))
    sky = np.zeros((nband, nx, ny))
    for (i, j), f in zip([(8, 9), (20, 17)], [1.0, 0.6]):
        sky[:, i, j] = f * (1 + 0.1 * rng.standard_normal(nband))
    dirty = ref.psf_convolve_cube(sky, psfhat, 2 * ny)
    wsums = np.full(nband, 1.0 / nband)
    model, residual, k, status, nminor = ref.clark(dirty, psf, psfhat, wsums, np.ones((nx, ny)), pf=0.05, maxit=50)
    assert status == 0 and nminor > k > 0
    assert set(zip(*np.nonzero(model.any(axis=0)))) <= {(8, 9), (20, 17)}
    assert np.abs(ref.search_image(residual)).max() ** 0.5 <= 0.05 * ref.search_image(dirty).max() ** 0.5


def test_yardstick_aliased_xhat_differs_from_a_copy():
    """The view-aliasing of xhat changes the entries after the peak only."""
    rng = np.random.default_rng(3)
    nband, A = 2, 40
    psf = _gauss_psf(16, 16, 3.0)[None].repeat(nband, 0)
    pidx, qidx = np.divmod(np.arange(A), 8)
    a0 = 1 + 0.1 * rng.standard_normal((nband, A))
    a0[:, 17] = 3.0
    out = []
    for copy in (False, True):
        a, model = a0.copy(), np.zeros((nband, 8, 8))
        ref.subminor(a, psf, pidx, qidx, model, np.array([0.5, 0.5]), 0.1, 0.0, 1, copy_xhat=copy)
        out.append(a)
    assert np.array_equal(out[0][:, :18], out[1][:, :18])
    assert not np.allclose(out[0][:, 18:], out[1][:, 18:], rtol=1e-6, atol=0)


def _ok_clark():
    nband, nx, ny = 2, 8, 6
    psf = np.zeros((nband, 2 * nx, 2 * ny))
    psf[:, nx, ny] = 1.0
    psfhat = np.fft.rfft2(np.fft.ifftshift(psf, axes=(1, 2)), axes=(1, 2))
    return dict(dirty=np.ones((nband, nx, ny)), psf=psf, psfhat=psfhat, wsums=np.array([0.5, 0.5]), mask=np.ones((nx, ny)))


@pytest.mark.parametrize("change", [
    dict(dirty=np.ones((8, 6))),                       # not a cube
    dict(psf=np.ones((3, 16, 12))),                    # band count mismatch
    dict(psfhat=np.ones((2, 16, 6), complex)),         # wrong psfhat shape
    dict(subpf=0.0), dict(subpf=1.0), dict(subpf=1.5),
    dict(wsums=np.array([0.5, 0.4])),                  # does not sum to 1
    dict(wsums=np.array([0.0, 0.0])),                  # all zero
    dict(gamma=0.0),
    dict(mask=np.ones((5, 6))),
])
def test_clark_argument_checks(change):
    from pfb_imaging_amd import deconv

    kw = _ok_clark()
    kw.update(change)
    with pytest.raises(ValueError):
        deconv.clark(**kw)


@pytest.mark.parametrize("change", [
    dict(dirty=np.ones((8, 6))),
    dict(psf=np.ones((2, 16))),
    dict(psf=np.concatenate([np.ones((1, 16, 12)), -np.ones((1, 16, 12))])),  # band 1 PSF peak <= 0
    dict(psf=np.concatenate([np.ones((1, 16, 12)), np.zeros((1, 16, 12))])),
    dict(gamma=-0.1),
])
def test_hogbom_argument_checks(change):
    from pfb_imaging_amd import deconv

    kw = dict(dirty=np.ones((2, 8, 6)), psf=np.ones((2, 16, 12)))
    kw.update(change)
    with pytest.raises(ValueError):
        deconv.hogbom(**kw)


def test_valid_call_without_gpu_raises_runtime_error(monkeypatch):
    """With no device visible a valid call fails loudly (the device count is forced to 0 so this runs on any box)."""
    from pfb_imaging_amd import _lib, deconv

    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        deconv.hogbom(np.ones((2, 8, 6)), np.ones((2, 16, 12)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        deconv.clark(**_ok_clark())


def test_clean_symbols_exported():
    from pfb_imaging_amd import _lib

    names = ("pfbhip_clean_create", "pfbhip_clean_destroy", "pfbhip_clean_hogbom", "pfbhip_clean_clark")
    assert set(names) <= set(_lib.SYMBOLS)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)


def test_clean_info_layout_matches_header(tmp_path):
    from pfb_imaging_amd import _lib

    fields = [name for name, _ in _lib.CleanInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pfbhip.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(pfbhip_clean_info));\n'
                   + "".join(f'printf("%zu\\n", offsetof(pfbhip_clean_info, {f}));\n' for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    C = _lib.CleanInfo
    assert out == [ct.sizeof(C)] + [getattr(C, f).offset for f in fields]


# ---- the reference-run pins (tests/golden/clean_pins.npz, made by tests/golden/make_clean_pins.py) --------------------------
from tests import _clean_cases as cc  # noqa: E402

PINS = np.load(os.path.join(ROOT, "tests", "golden", "clean_pins.npz"))


def _pin_model(name, c, key="val"):
    return cc.dense(PINS[f"{name}_idx"], PINS[f"{name}_{key}"], c["dirty"].shape)


def _yardstick(c, clark=ref.clark):
    """(model, status, k, nminor)"""
    if c["kind"] == "hogbom":
        model, _, k, status = ref.hogbom(c["dirty"], c["psf"], **c["kw"])
        return model, status, k, k
    model, _, k, status, nminor = clark(c["dirty"], c["psf"], cc.psfhat(c["psf"]), c["wsums"], c["mask"], **c["kw"])
    return model, status, k, nminor


def test_pin_file_lists_every_case_and_holds_numbers_only():
    assert tuple(PINS["cases"]) == cc.ALL_CASES
    assert all(PINS[k].dtype.kind in "ifU" for k in PINS.files)
    assert all(":" in c or "=" in c for c in PINS["cites"])


@pytest.mark.parametrize("name", cc.E_CASES + cc.CLARK_T_CASES)
def test_yardstick_reproduces_reference_pin(name):
    """Class E and, over numpy.fft as the pin was made, class T: the reference's model bit for bit, its k and its status."""
    c = cc.case(name)
    model, status, k, nminor = _yardstick(c)
    assert (k, status) == (int(PINS[f"{name}_k"]), int(PINS[f"{name}_status"]))
    assert np.array_equal(model, _pin_model(name, c))
    if c["kind"] == "clark" and c["kw"]["maxit"] == 1:  # every class E Clark case is cut short by submaxit
        assert nminor == c["kw"]["submaxit"]


def test_yardstick_in_float64_is_within_ten_times_the_float32_pin_disagreement():
    """H6: the reference's float32 run against the yardstick in float64 on the same numbers (what the device computes)."""
    c = cc.case("H6")
    pin = _pin_model("H6", c)
    assert PINS["H6_val"].dtype == np.float32
    model, status, k, _ = _yardstick(dict(c, dirty=c["dirty"].astype(np.float64), psf=c["psf"].astype(np.float64)))
    assert (k, status) == (int(PINS["H6_k"]), int(PINS["H6_status"])) and np.array_equal(model != 0, pin != 0)
    err, bound = cc.rel_max(model.astype(np.float32), pin), cc.f_bound(PINS["H6_disagreement"])
    assert err <= bound < 1e-6, (err, bound)


def test_class_t_pins_are_conditioned():
    for name in cc.CLARK_T_CASES:
        c = cc.case(name)
        dis = float(PINS[f"{name}_disagreement"])
        assert dis == cc.rel_max(_pin_model(name, c, "sp_val"), _pin_model(name, c)) and dis < 1e-14
        assert cc.t_bound(dis) == max(10 * dis, 64 * 2.0 ** -52)


def _last_peak(search):
    flat = search.reshape(-1)
    pq = flat.size - 1 - int(np.argmax(flat[::-1]))
    return pq, np.sqrt(flat[pq])


def _clark_variant(**sw):
    """tests/_clean_ref.py's clark with one convention switched to a plausible wrong one"""
    peak = _last_peak if sw.get("last_max") else ref.peak

    def subminor(a, psf, pidx, qidx, model, wsums, gamma, th, maxit, mask):
        nband, nxp, nyp = psf.shape
        nxo2, nyo2 = nxp // 2, nyp // 2
        idx = np.arange(pidx.size)
        weight = mask[pidx, qidx] if sw.get("sub_mask") else 1.0
        pq, amax = peak(ref.search_image(a) * weight)
        p, q = pidx[pq], qidx[pq]
        k = 0
        while amax > th and k < maxit:
            sign = 1 if sw.get("unreflected") else -1
            pp, qq = nxo2 + sign * (pidx - p), nyo2 + sign * (qidx - q)
            if sw.get("wrap"):
                pp, qq = pp % nxp, qq % nyp
            inb = (pp >= 0) & (pp < nxp) & (qq >= 0) & (qq < nyp)
            after = idx[inb] >= pq if sw.get("strict_before") else idx[inb] > pq
            for b in range(nband):
                xb = a[b, pq]
                g = gamma * xb
                model[b, p, q] += g / wsums[b]
                g2 = g if sw.get("copy_xhat") else gamma * (xb - (g * psf[b, nxo2, nyo2]) / wsums[b])
                a[b, inb] = a[b, inb] - (np.where(after, g2, g) * psf[b, pp[inb], qq[inb]]) / wsums[b]
            pq, amax = peak(ref.search_image(a) * weight)
            p, q = pidx[pq], qidx[pq]
            k += 1
        return k

    def clark(dirty, psf, psfhat, wsums, mask, threshold, gamma, pf, maxit, subpf, submaxit):
        major_mask = np.ones_like(mask) if sw.get("no_major_mask") else mask
        model, residual = np.zeros_like(dirty), dirty.copy()
        search = ref.search_image(residual) * major_mask
        pq, rmax = peak(search)
        tol = max(pf * rmax, threshold)
        k = nminor = 0
        while rmax > tol and k < maxit:
            subth = subpf * rmax
            pidx, qidx = np.where(search > subth * subth)
            nminor += subminor(residual[:, pidx, qidx], psf, pidx, qidx, model, wsums, gamma, subth, submaxit, mask)
            residual = dirty - ref.psf_convolve_cube(model, psfhat, psf.shape[2])
            search = ref.search_image(residual) * major_mask
            pq, rmax = peak(search)
            k += 1
        return model, residual, k, int(k >= maxit), nminor

    return clark


def test_variant_scaffold_with_no_switch_is_the_yardstick():
    for name in ("C1_4096", "C4_6", "C5_half_mask", "T1"):
        c = cc.case(name)
        got, want = _yardstick(c, _clark_variant()), _yardstick(c)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]


# wrong variant -> the pins that must notice it
VARIANTS = {
    "unreflected": ("C4_6", "C4_5", "C4G_6", "C4G_5"),
    "copy_xhat": ("C4_6", "C4G_6", "C1_4096"),
    "last_max": ("H3", "H4_wave_1", "H4_sign_1", "H4_group_1", "H4_trip_1", "H4_trip_2", "C5_adjacent", "C5_far_lds", "C5_far_grid"),
    "wrap": ("C1_4096", "C1_4097", "C2_193"),
    "no_major_mask": ("C5_masked_peak", "T1"),
    "sub_mask": ("C5_half_mask",),
    "strict_before": ("C4_6", "C4_5", "C4G_6", "C4G_5"),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_pins_catch_wrong_variant(variant, monkeypatch):
    """Each plausible wrong reading of the reference changes the model of every pin named for it."""
    if variant == "last_max":
        monkeypatch.setattr(ref, "peak", _last_peak)  # Hogbom's search too
    for name in VARIANTS[variant]:
        c = cc.case(name)
        model = _yardstick(c, _clark_variant(**{variant: True}))[0]
        assert not np.array_equal(model, _pin_model(name, c)), f"{variant} passes {name}"


def test_c3_notices_a_compaction_that_forgets_its_running_base():
    """k_cl_compact walks its chunk of 257 pixels in two trips of 256 threads and must add the first trip's total to its base.
    Restated here without that: the second trip's pixel lands on the chunk's first slot, and the slots left over keep what
    fresh device memory holds (pixel (0, 0), value 0).  The sub-minor loop on that active set must not give C3's pin."""
    c = cc.case("C3")
    nband, nx, ny = c["dirty"].shape
    search = ref.search_image(c["dirty"]) * c["mask"]
    _, rmax = ref.peak(search)
    subth = c["kw"]["subpf"] * rmax
    flag = search.reshape(-1) > subth * subth
    A, nchunk = int(flag.sum()), -(-nx * ny // cc.C3_CHUNK)
    assert nchunk == 1024 and A > cc.TRIP

    def compact(forget):
        t_of = np.full(A, -1)
        base = 0
        for g in range(nchunk):
            t0, t1 = g * cc.C3_CHUNK, min((g + 1) * cc.C3_CHUNK, nx * ny)
            start = base
            for t00 in range(t0, t1, 256):
                ts = np.arange(t00, min(t00 + 256, t1))
                ts = ts[flag[ts]]
                t_of[start:start + ts.size] = ts
                if not forget:
                    start += ts.size
            base += int(flag[t0:t1].sum())
        return t_of

    good = compact(False)
    assert np.array_equal(good, np.flatnonzero(flag))
    t_of = compact(True)
    assert (t_of < 0).sum() > 1000
    pidx, qidx = np.divmod(np.where(t_of < 0, 0, t_of), ny)
    a = np.where(t_of < 0, 0.0, c["dirty"].reshape(nband, -1)[:, np.maximum(t_of, 0)])
    model = np.zeros_like(c["dirty"])
    ref.subminor(a, c["psf"], pidx, qidx, model, c["wsums"], c["kw"]["gamma"], subth, c["kw"]["submaxit"])
    assert not np.array_equal(model, _pin_model("C3", c))
