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
