"""CPU tests of the forward-backward solver's host surface: the legacy ``fista`` oracle (opt/fista.py:13-95 of the
reference) on a lasso, its backtracking branch, the ``ForwardBackward`` setup contract, and the C-ABI struct of the
device loop."""

import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lasso(b, lam, calls=None):
    def fprime(x):
        if calls is not None:
            calls.append(x.copy())
        r = x - b
        return 0.5 * float(np.vdot(r, r)), r

    def prox(x):
        return np.sign(x) * np.maximum(np.abs(x) - lam / 1.0, 0.0)

    return fprime, prox


@pytest.mark.parametrize("lam", [0.1, 1.0])
def test_fista_lasso_reaches_soft_threshold(lam):
    from pfb_imaging_amd.opt import fista

    b = np.random.default_rng(1).standard_normal((3, 16, 12))
    fprime, prox = _lasso(b, lam)
    x = fista(np.zeros_like(b), 1.0, fprime, prox, tol=1e-10, maxit=200, verbosity=0)
    expect = np.sign(b) * np.maximum(np.abs(b) - lam, 0.0)
    assert np.abs(x - expect).max() < 1e-6


def test_fista_backtracking_fires_when_hessnorm_is_underestimated():
    """With hessnorm = 0.3 the first step overshoots (f rises), so hessnorm doubles and the step is retried: fprime is
    called more than once per iteration, and the result is still the lasso solution."""
    from pfb_imaging_amd.opt import fista

    b = np.random.default_rng(2).standard_normal((2, 10, 10)) + 2.0
    lam = 0.05
    calls = []
    fprime_c, _ = _lasso(b, lam, calls)
    soft = lambda x: np.sign(x) * np.maximum(np.abs(x) - lam, 0.0)  # noqa: E731
    x = fista(np.zeros_like(b), 0.3, fprime_c, soft, tol=1e-12, maxit=3, verbosity=0)
    # 1 call before the loop + 1 per iteration without backtracking: more means the retry branch ran
    assert len(calls) > 1 + 3
    # the first retry is the step at hessnorm 0.6: y - grad / 0.6 from y = 0
    assert np.allclose(calls[2], soft(b / 0.6))
    assert np.all(np.isfinite(x))
    fb_calls = []
    fprime_n, _ = _lasso(b, lam, fb_calls)
    fista(np.zeros_like(b), 1.0, fprime_n, soft, tol=1e-12, maxit=3, verbosity=0)
    # exact hessnorm: one call per iteration, the first step accepted as it is
    assert len(fb_calls) <= 1 + 3 and np.allclose(fb_calls[1], soft(b))


def test_forward_backward_contract_without_gpu():
    from pfb_imaging_amd.operators.psi import IdentityPsi
    from pfb_imaging_amd.opt import L1, ForwardBackward

    fb = ForwardBackward(gamma=0.45, maxit=5, verbosity=0)
    x = np.zeros((2, 8, 6))
    with pytest.raises(RuntimeError, match="setup"):
        fb.solve(x, 1.0)
    reg = L1(IdentityPsi(2, 8, 6))
    fb.setup(reg, 1.7)
    assert fb.step == 2 * 0.45 / 1.7
    assert fb._alpha.shape == (2, 1, 8, 6) and fb._xout.shape == (2, 8, 6)
    with pytest.raises(RuntimeError, match="set_grad"):
        fb.solve(x, 1.0)
    with pytest.raises(TypeError):
        fb.setup(object(), 1.0)


def test_fb_info_layout_matches_header(tmp_path):
    from pfb_imaging_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "pfbhip.h"\n'
        "int main(void){\n"
        'printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(pfbhip_fb_info), offsetof(pfbhip_fb_info, status),'
        " offsetof(pfbhip_fb_info, eps), offsetof(pfbhip_fb_info, loop_ms), offsetof(pfbhip_fb_info, events),"
        " offsetof(pfbhip_fb_info, stage_ms), offsetof(pfbhip_fb_info, stage_calls), PFBHIP_FB_NSTAGES);\n"
        "return 0;}\n"
    )
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    F = _lib.FBInfo
    assert out == [ct.sizeof(F), F.status.offset, F.eps.offset, F.loop_ms.offset, F.events.offset, F.stage_ms.offset,
                   F.stage_calls.offset, _lib.FB_NSTAGES]
    assert len(_lib.FB_STAGE_NAMES) == _lib.FB_NSTAGES
