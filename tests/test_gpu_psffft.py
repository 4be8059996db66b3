"""The PSF row-FFT pipeline (csrc/psffft.hip) against numpy at every shape it instantiates.

A PsfConv plan runs the three-pass row-FFT pipeline when both padded sizes are plain row-FFT lengths (PsfFFT::init) and the
rocFFT 2-D r2c / c2r fallback otherwise; ``PsfConv.uses_rowfft`` reports which.  Every x-axis shape of PSF_FOR_SHAPES_X
(csrc/psffft.hip) and every y-axis shape of RF_FOR_SHAPES (csrc/rowfft.hpp) is checked here against a float64 numpy
reference in the psf_convolve_cube convention: pad at [0:nx, 0:ny], multiply by f(psfhat), crop, beam before and after.

The reference is numpy's rfft2 / irfft2 factorised the way numpy itself evaluates them (rfft along y, fft along x; ifft along
x, irfft along y), with the zero rows of the padded image and the cropped rows of the output left out of the transforms
along y; ``test_reference_is_rfft2_irfft2`` pins it to the literal rfft2 / irfft2.  Test spectra satisfy the pipeline's
precondition (psffft_api.hpp): the ky = 0 and ky = nyp / 2 columns are conjugate-symmetric in kx.

Bound: rel L2 <= 1e-13 and max|err| <= 1e-13 max|ref| (mode 2: times max|1/(psf+s)| / min|1/(psf+s)|).
"""

import itertools
import os
import re

import numpy as np
import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pfb-imaging_amd", "csrc")

# RF_FOR_SHAPES (csrc/rowfft.hpp): (LEAD, K), N = LEAD * 2^K
RF_SHAPES = [(1, 10), (1, 11), (1, 12), (1, 13), (1, 14), (3, 9), (3, 10), (3, 11), (3, 12), (5, 8), (5, 9), (5, 10), (5, 11),
             (7, 8), (7, 9), (7, 10), (7, 11), (9, 7), (9, 8), (9, 9), (9, 10), (15, 7), (15, 8), (15, 9), (15, 10)]
# PSF_FOR_SHAPES_X (csrc/psffft.hip): the x-axis shapes of pass 2
PSF_SHAPES_X = [(1, 10), (1, 11), (1, 12), (1, 13), (1, 14), (3, 9), (3, 10), (3, 11), (5, 8), (5, 9), (5, 10), (5, 11), (7, 8),
                (7, 9), (7, 10), (9, 7), (9, 8), (9, 9), (9, 10), (15, 7), (15, 8), (15, 9)]
# RF_FOR_SHAPES2 (csrc/rowfft.hpp): doubled lengths 2 * LEAD * 2^K, which the pipeline does not take
RF_DOUBLED = [(5, 11), (3, 12), (1, 14)]

BOUND = 1e-13


def _lead(n):
    for lead, k in RF_SHAPES:
        if lead << k == n:
            return lead
    return None


def admits(nx, ny, nxp, nyp):
    """PsfFFT::init (csrc/psffft.hip): both padded sizes plain row-FFT lengths (not doubled); on x, a radix-3/5/7/9/15 lead
    hands the row over through LDS, both components, so nxp * 16 bytes <= 160 KiB."""
    lx, ly = _lead(nxp), _lead(nyp)
    if lx is None or ly is None:
        return False
    if lx != 1 and nxp * 16 > 160 * 1024:
        return False
    return nx <= nxp and ny <= nyp


def herm_cols(p):
    """Project the ky = 0 and ky = nyp / 2 columns onto conjugate symmetry in kx (the pipeline's precondition).  numpy's
    irfft2 gives the same result before and after: it keeps only the real part of those two columns after the x inverse."""
    neg = (-np.arange(p.shape[0])) % p.shape[0]
    for c in (0, p.shape[1] - 1):
        col = p[:, c].copy()
        p[:, c] = 0.5 * (col + np.conj(col[neg]))
    return p


def real_psfhat(rng, nxp, nyo2):
    return herm_cols(1.0 + rng.random((nxp, nyo2)))


def complex_psfhat(rng, nxp, nyo2):
    return herm_cols((1.0 + rng.random((nxp, nyo2))) + 1j * (rng.random((nxp, nyo2)) - 0.5))


def spectrum(xb, nxp, nyp):
    """rfft2 of xb zero-padded to (nxp, nyp)."""
    return np.fft.fft(np.fft.rfft(xb, n=nyp, axis=1), n=nxp, axis=0)


def fpsf(ph, mode, shift):
    return ph if mode == 0 else (ph + shift if mode == 1 else 1.0 / (ph + shift))


def back(xh, f, nx, ny, nyp):
    """irfft2(xh * f, s=(nxp, nyp))[:nx, :ny]."""
    return np.fft.irfft(np.fft.ifft(xh * f, axis=0)[:nx], n=nyp, axis=1)[:, :ny]


def reference(x, ph, nxp, nyp, mode=0, shift=0.0, beam=None, scale=1.0, eta=0.0, prev=None, xh=None):
    nx, ny = x.shape
    if xh is None:
        xh = spectrum(x if beam is None else x * beam, nxp, nyp)
    r = back(xh, fpsf(ph, mode, shift), nx, ny, nyp)
    if beam is not None:
        r = r * beam
    r = r * scale + eta * x
    return r + prev if prev is not None else r


def bound(ph, mode, shift):
    if mode != 2:
        return BOUND
    a = np.abs(1.0 / (ph + shift))
    return BOUND * a.max() / a.min()


def agree(got, want, tol, what):
    err = np.asarray(got) - want
    r = np.linalg.norm(err) / np.linalg.norm(want)
    m = np.abs(err).max() / np.abs(want).max()
    print(f"{what}: rel L2 {r:.2e}  max {m:.2e}  (bound {tol:.1e})")
    assert r <= tol and m <= tol, f"{what}: rel L2 {r:.3e}, max|err| / max|ref| {m:.3e} > {tol:.1e}"


def _plan(nx, ny, nxp, nyp, monkeypatch):
    from pfb_imaging_amd.psfconv import PsfConv

    monkeypatch.delenv("PFBHIP_PSF_ROWFFT", raising=False)
    return PsfConv(nx, ny, nxp, nyp)


# ---- host-side checks of the test's own tables and reference ----------------------------------------------------------


def _macro_shapes(path, name):
    src = open(path).read()
    m = re.search(r"#define " + name + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", src)
    assert m, name
    return [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", m.group(1))]


def test_shape_tables_match_the_sources():
    """The parametrisations below cover exactly the kernel instantiations the sources define."""
    assert _macro_shapes(os.path.join(CSRC, "rowfft.hpp"), "RF_FOR_SHAPES") == RF_SHAPES
    assert _macro_shapes(os.path.join(CSRC, "rowfft.hpp"), "RF_FOR_SHAPES2") == RF_DOUBLED
    assert _macro_shapes(os.path.join(CSRC, "psffft.hip"), "PSF_FOR_SHAPES_X") == PSF_SHAPES_X
    # the x instantiations are exactly the lengths the admission rule takes on x
    assert [s for s in RF_SHAPES if admits(1, 1, s[0] << s[1], 1024)] == PSF_SHAPES_X


def test_reference_is_rfft2_irfft2():
    rng = np.random.default_rng(0)
    nx, ny, nxp, nyp = 37, 29, 64, 48
    x = rng.standard_normal((nx, ny))
    beam = 0.5 + rng.random((nx, ny))
    for ph in (real_psfhat(rng, nxp, nyp // 2 + 1), complex_psfhat(rng, nxp, nyp // 2 + 1)):
        for mode, shift in ((0, 0.0), (1, 0.5), (2, 0.5)):
            xp = np.zeros((nxp, nyp))
            xp[:nx, :ny] = x * beam
            want = np.fft.irfft2(np.fft.rfft2(xp) * fpsf(ph, mode, shift), s=(nxp, nyp))[:nx, :ny] * beam * 0.7 + 0.2 * x
            got = reference(x, ph, nxp, nyp, mode, shift, beam, 0.7, 0.2)
            assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-15
    # the precondition projection changes nothing numpy computes
    raw = rng.random((nxp, nyp // 2 + 1)) + 1j * rng.random((nxp, nyp // 2 + 1))
    proj = herm_cols(raw.copy())
    assert not np.allclose(raw, proj)
    assert np.linalg.norm(reference(x, raw, nxp, nyp) - reference(x, proj, nxp, nyp)) < 1e-15 * np.linalg.norm(
        reference(x, raw, nxp, nyp))


# ---- a. admission -----------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("axis", ["x", "y"])
def test_admission_table(axis, monkeypatch):
    """uses_rowfft follows PsfFFT::init for every family length on each axis (the other axis at 1024): 12288 / 14336 / 15360
    fall back on x only.  One small fallback geometry (padded sizes below 1024, as the small-size operator tests use) is
    checked against numpy as well."""
    rng = np.random.default_rng(1 if axis == "x" else 2)
    fallbacks = []
    for lead, k in RF_SHAPES:
        n = lead << k
        nxp, nyp = (n, 1024) if axis == "x" else (1024, n)
        pc = _plan(77, 91, nxp, nyp, monkeypatch)
        assert pc.uses_rowfft == admits(77, 91, nxp, nyp), (axis, n)
        if not pc.uses_rowfft:
            fallbacks.append(n)
        pc.close()
    assert fallbacks == ([12288, 14336, 15360] if axis == "x" else [])
    nx, ny, nxp, nyp = (45, 37, 96, 80) if axis == "x" else (37, 45, 80, 96)
    assert not admits(nx, ny, nxp, nyp)
    pc = _plan(nx, ny, nxp, nyp, monkeypatch)
    assert not pc.uses_rowfft
    ph = complex_psfhat(rng, nxp, nyp // 2 + 1)
    x = rng.standard_normal((nx, ny))
    pc.set_psfhat(0, ph)
    agree(pc.apply(x, 0), reference(x, ph, nxp, nyp), BOUND, f"fallback {nxp}x{nyp}")
    pc.close()


# The padded sizes next to the family that must fall back; good_size(2 * 1100) is added by the worker.
NEIGHBOURS = [2 * (lead << k) for lead, k in RF_DOUBLED] + [512, 1000, 2200, 12288, 14336, 15360]


@gpu
def test_admission_neighbours():
    """The neighbours of the family that must take the rocFFT fallback: the doubled lengths 20480 / 24576 / 32768 (which
    rowfft_make_plan accepts and PsfFFT::init must still refuse), 512, 1000, 2200 and good_size(2 * 1100) on each axis, and
    12288 / 14336 / 15360 on x (leads 3 / 7 / 15 above 10240; on y they are admitted).  uses_rowfft follows admits() for each,
    and each fallback matches numpy.

    The plans run in a child process (tests/_psffft_fallback_worker.py) that launches no row-FFT kernel.  rocFFT compiles,
    loads and, when a plan is destroyed, unloads one module per kernel of these plans (some 270 of each for these sizes).  When this
    list ran in the test process itself, the next launch from a code object loaded after it -- the PSF transpose, a plain
    load / LDS / store kernel -- was stopped with HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION; the same kernels pass at every shape in a
    process without that sequence.  Code memory is freed only by those module unloads, not by this library."""
    import json
    import subprocess
    import sys

    from pfb_imaging_amd.fft import good_size

    env = dict(os.environ)
    env.pop("PFBHIP_PSF_ROWFFT", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_psffft_fallback_worker.py"),
                        ",".join(str(n) for n in NEIGHBOURS)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    sizes = NEIGHBOURS + [good_size(2 * 1100)]
    assert [(r["axis"], r["n"]) for r in recs] == [(a, n) for a in ("x", "y") for n in sizes]
    for r in recs:
        print(r)
        assert r["uses_rowfft"] == admits(min(r["nxp"], 77), min(r["nyp"], 91), r["nxp"], r["nyp"]), r
        if r["axis"] == "x" or r["n"] not in (12288, 14336, 15360):
            assert not r["uses_rowfft"], r
        if not r["uses_rowfft"]:
            assert r["rel"] <= BOUND and r["max"] <= BOUND, r


# ---- b. shape sweep ---------------------------------------------------------------------------------------------------

SWEEP = [("x", lead << k) for lead, k in PSF_SHAPES_X] + [("y", lead << k) for lead, k in RF_SHAPES]


@gpu
@pytest.mark.parametrize("axis,n", SWEEP, ids=[f"{a}{n}" for a, n in SWEEP])
def test_shape_sweep(axis, n, monkeypatch):
    """One x-axis (pass 2) or y-axis (passes 1 and 3) instantiation at a time, the other axis at 1024: a real and a complex
    psfhat, modes 0 / 1 / 2, beam, scale, eta, accumulate.  nx is odd and not a multiple of 128 (the unpaired last row and
    the tail of the psf_xcd_row remap), ny < nyp."""
    nxp, nyp = (n, 1024) if axis == "x" else (1024, n)
    nyo2 = nyp // 2 + 1
    nx, ny = (5 * nxp) // 8 + 1, (3 * nyp) // 4 + 3
    assert nx % 2 == 1 and nx % 128 != 0 and ny < nyp
    rng = np.random.default_rng(n * 2 + (axis == "y"))
    x = rng.standard_normal((nx, ny))
    beam = 0.5 + rng.random((nx, ny))
    prev = rng.standard_normal((nx, ny))
    phs = (real_psfhat(rng, nxp, nyo2), complex_psfhat(rng, nxp, nyo2))
    pc = _plan(nx, ny, nxp, nyp, monkeypatch)
    assert pc.uses_rowfft
    pc.set_psfhat(0, phs[0])
    pc.set_psfhat(1, phs[1])
    pc.set_beam(0, beam)
    xh = {False: spectrum(x, nxp, nyp), True: spectrum(x * beam, nxp, nyp)}
    # (psf slot, mode, shift, beam, scale, eta, accumulate)
    cases = [(0, 0, 0.0, False, 1.0, 0.0, False), (1, 0, 0.0, True, 0.7, 0.2, False), (0, 1, 0.5, True, 1.0, 0.0, True),
             (1, 2, 0.5, False, 1.3, 0.1, False), (0, 2, 0.25, True, 1.0, 0.0, False)]
    for slot, mode, shift, bm, scale, eta, acc in cases:
        out = prev.copy() if acc else None
        got = pc.apply(x, slot, beam_slot=0 if bm else -1, mode=mode, shift=shift, scale=scale, eta=eta, out=out,
                       accumulate=acc)
        want = reference(x, phs[slot], nxp, nyp, mode, shift, beam if bm else None, scale, eta, prev if acc else None,
                         xh=xh[bm])
        agree(got, want, bound(phs[slot], mode, shift), f"{nxp}x{nyp} slot {slot} mode {mode} beam {bm} acc {acc}")
    pc.close()


# ---- c. geometry edges ------------------------------------------------------------------------------------------------

EDGE_OPTIONS = list(itertools.product((0, 1, 2), (False, True), (0.0, 0.3), (False, True)))  # mode, beam, eta, accumulate


@gpu
@pytest.mark.parametrize("nxp,nyp", [(1024, 2048), (10240, 1024)])
def test_geometry_edges(nxp, nyp, monkeypatch):
    """nx in {1, 2, 63, 64, 127, 128, 129, nxp - 1, nxp} x ny in {1, 2, nyp/2 + 1, nyp} (nx = nxp, ny = nyp: unpadded,
    circular), on a power-of-two shape and on 10240 along x (lead 5: the LDS hand-over of pass 2 is exactly 160 KiB).
    Every cell runs a real and a complex psfhat; the 24 combinations of mode, beam, eta and accumulate cycle over the
    cells, so each meets both psfhat kinds."""
    nyo2 = nyp // 2 + 1
    rng = np.random.default_rng(nxp + nyp)
    phs = (real_psfhat(rng, nxp, nyo2), complex_psfhat(rng, nxp, nyo2))
    cells = list(itertools.product((1, 2, 63, 64, 127, 128, 129, nxp - 1, nxp), (1, 2, nyp // 2 + 1, nyp)))
    for i, (nx, ny) in enumerate(cells):
        x = rng.standard_normal((nx, ny))
        beam = 0.5 + rng.random((nx, ny))
        prev = rng.standard_normal((nx, ny))
        pc = _plan(nx, ny, nxp, nyp, monkeypatch)
        assert pc.uses_rowfft
        pc.set_psfhat(0, phs[0])
        pc.set_psfhat(1, phs[1])
        pc.set_beam(0, beam)
        for slot, opt in ((0, EDGE_OPTIONS[i % 24]), (1, EDGE_OPTIONS[(i + 12) % 24])):
            mode, bm, eta, acc = opt
            shift = 0.5 if mode else 0.0
            out = prev.copy() if acc else None
            got = pc.apply(x, slot, beam_slot=0 if bm else -1, mode=mode, shift=shift, scale=0.9, eta=eta, out=out,
                           accumulate=acc)
            want = reference(x, phs[slot], nxp, nyp, mode, shift, beam if bm else None, 0.9, eta, prev if acc else None)
            agree(got, want, bound(phs[slot], mode, shift), f"{nxp}x{nyp} nx {nx} ny {ny} slot {slot} {opt}")
        pc.close()


# ---- d. slots on the transposed storage -------------------------------------------------------------------------------


@gpu
def test_slots_on_transposed_storage(monkeypatch):
    """Several slots on one plan (psfhat stored transposed, (nyo2, nxp)), a slot rebound real -> complex -> real, a beam
    unbound, and apply_dev on device buffers: every result equals a fresh plan's and numpy's."""
    from pfb_imaging_amd._lib import DeviceArray, check, cint, f64, i64, lib

    nx, ny, nxp, nyp = 601, 700, 1280, 1536
    nyo2 = nyp // 2 + 1
    rng = np.random.default_rng(5)
    x = rng.standard_normal((nx, ny))
    beams = [0.5 + rng.random((nx, ny)) for _ in range(2)]
    phs = [real_psfhat(rng, nxp, nyo2), complex_psfhat(rng, nxp, nyo2), real_psfhat(rng, nxp, nyo2)]
    pc = _plan(nx, ny, nxp, nyp, monkeypatch)
    assert pc.uses_rowfft
    for s, ph in enumerate(phs):
        pc.set_psfhat(s, ph)
    for s, b in enumerate(beams):
        pc.set_beam(s, b)

    def fresh(ph, beam, **kw):
        f = _plan(nx, ny, nxp, nyp, monkeypatch)
        f.set_psfhat(0, ph)
        if beam is not None:
            f.set_beam(0, beam)
        r = f.apply(x, 0, beam_slot=0 if beam is not None else -1, **kw)
        f.close()
        return r

    def same(slot, bslot, ph, **kw):
        beam = beams[bslot] if bslot >= 0 else None
        got = pc.apply(x, slot, beam_slot=bslot, **kw)
        assert np.array_equal(got, fresh(ph, beam, **kw)), (slot, bslot, kw)
        agree(got, reference(x, ph, nxp, nyp, kw.get("mode", 0), kw.get("shift", 0.0), beam), bound(ph, kw.get("mode", 0),
                                                                                                    kw.get("shift", 0.0)),
              f"slot {slot} beam {bslot} {kw}")
        return got

    for slot in range(3):
        for bslot in (-1, 0, 1):
            same(slot, bslot, phs[slot])
    same(1, 0, phs[1], mode=2, shift=0.5)
    # rebind slot 1: real -> complex -> real; the neighbours keep theirs
    for ph in (real_psfhat(rng, nxp, nyo2), complex_psfhat(rng, nxp, nyo2), real_psfhat(rng, nxp, nyo2)):
        pc.set_psfhat(1, ph)
        phs[1] = ph
        same(1, 1, ph)
        same(1, -1, ph, mode=1, shift=0.5)
        same(0, 1, phs[0])
        same(2, 0, phs[2])
    # unbind beam 1: applying with it is an error, the plan stays usable
    pc.set_beam(1, None)
    with pytest.raises(ValueError, match="not bound"):
        pc.apply(x, 0, beam_slot=1)
    same(0, 0, phs[0])
    same(2, -1, phs[2])
    # apply_dev on device buffers, plain and accumulating
    prev = rng.standard_normal((nx, ny))
    dx, dout = DeviceArray.from_host(x), DeviceArray.from_host(prev)
    check(lib().pfbhip_psfconv_apply_dev(pc._h, dx.ptr, i64(2), i64(0), cint(1), f64(0.5), f64(0.8), f64(0.1), cint(1),
                                         dout.ptr))
    acc = dout.download().copy()
    check(lib().pfbhip_psfconv_apply_dev(pc._h, dx.ptr, i64(2), i64(0), cint(1), f64(0.5), f64(0.8), f64(0.1), cint(0),
                                         dout.ptr))
    plain = dout.download().copy()
    kw = dict(mode=1, shift=0.5, scale=0.8, eta=0.1)
    assert np.array_equal(plain, fresh(phs[2], beams[0], **kw))
    assert np.array_equal(acc, prev + plain)
    agree(plain, reference(x, phs[2], nxp, nyp, beam=beams[0], **kw), BOUND, "apply_dev")
    dx.free()
    dout.free()
    pc.close()


# ---- 4. the precondition on psfhat ------------------------------------------------------------------------------------


@gpu
def test_psfhat_precondition(monkeypatch):
    """Pass 3 extends the half spectrum as it stands; numpy's irfft2 drops the imaginary part of the ky = 0 and ky = nyp / 2
    columns after the x inverse.  A psfhat whose two edge columns are not conjugate-symmetric in kx therefore gives a
    different result on the pipeline (the imaginary part leaks into the partner row), and its projection gives numpy's."""
    nx, ny, nxp, nyp = 9, 300, 1024, 1024
    nyo2 = nyp // 2 + 1
    rng = np.random.default_rng(9)
    raw = 1.0 + rng.random((nxp, nyo2))  # a random real psfhat: its edge columns are not even in kx
    x = rng.standard_normal((nx, ny))
    want = reference(x, raw, nxp, nyp)
    pc = _plan(nx, ny, nxp, nyp, monkeypatch)
    assert pc.uses_rowfft
    pc.set_psfhat(0, raw)
    pc.set_psfhat(1, herm_cols(raw.copy()))
    off = pc.apply(x, 0)
    agree(pc.apply(x, 1), want, BOUND, "projected psfhat")
    err = np.linalg.norm(off - want) / np.linalg.norm(want)
    print(f"unprojected psfhat: rel L2 {err:.2e}")
    # If this fails, the pipeline now handles such a psfhat and the precondition in psffft_api.hpp can go.
    assert err > 1e-6
    # the last row has no partner: its real part is exact either way
    agree(off[-1], want[-1], BOUND, "unpaired row")
    pc.close()


# ---- e. production sizes ----------------------------------------------------------------------------------------------


@gpu
def test_hesspsf_dot_c4_geometry(monkeypatch):
    """HessPSF.dot at the C4 geometry: a 4096^2 image on an 8192^2 PSF, with a beam."""
    from pfb_imaging_amd.operators.hessian import HessPSF

    monkeypatch.delenv("PFBHIP_PSF_ROWFFT", raising=False)
    nx = ny = 4096
    nxp = nyp = 8192
    rng = np.random.default_rng(4)
    abspsf = real_psfhat(rng, nxp, nyp // 2 + 1)[None]
    beam = 0.5 + rng.random((1, nx, ny))
    x = rng.standard_normal((1, nx, ny))
    h = HessPSF(nx, ny, abspsf, beam=beam, eta=0.1)
    assert h._plan.uses_rowfft
    got = np.array(h.dot(x))
    want = reference(x[0], abspsf[0], nxp, nyp, beam=beam[0], eta=0.1)
    agree(got[0], want, BOUND, "HessPSF.dot 4096^2 / 8192^2")


@gpu
def test_readme_headline_geometry(monkeypatch):
    """An 8192^2 image on a 16384^2 PSF with ~20 deltas: the reference is the sum of shifted copies of irfft2(psfhat), one
    numpy transform in all (its two axes run one after the other so the 2 GiB complex intermediate and the 2 GiB PSF
    overlap only with each other).  Peak host memory (RSS) of the numpy side, measured once: 5.0 GB."""
    nx = ny = 8192
    nxp = nyp = 16384
    rng = np.random.default_rng(16)
    ph = real_psfhat(rng, nxp, nyp // 2 + 1)
    pos = rng.integers(0, nx, size=(20, 2))
    amp = rng.standard_normal(20)
    x = np.zeros((nx, ny))
    np.add.at(x, (pos[:, 0], pos[:, 1]), amp)
    pc = _plan(nx, ny, nxp, nyp, monkeypatch)
    assert pc.uses_rowfft
    pc.set_psfhat(0, ph)
    got = pc.apply(x, 0).copy()
    pc.close()
    del x
    t = np.fft.ifft(ph, axis=0)
    del ph
    psf = np.fft.irfft(t, n=nyp, axis=1)
    del t
    want = np.zeros((nx, ny))
    for (i, j), a in zip(pos, amp):
        rows = (np.arange(nx) - i) % nxp
        cols = (np.arange(ny) - j) % nyp
        want += a * psf[np.ix_(rows, cols)]
    del psf
    agree(got, want, BOUND, "8192^2 / 16384^2 deltas")
