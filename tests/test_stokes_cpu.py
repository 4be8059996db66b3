"""The Stokes conventions without a device: ``stokes_products`` against every selection and refusal recorded from the reference
(tests/golden/stokes_pins.npz), the host coherency <-> Stokes maps, the numpy oracle of ``weight_data`` (tests/_stokes_ref.py)
against two independent statements of what it computes, and the library's refusals, which precede any device call.
"""

import ctypes as ct
import functools
import os

import numpy as np
import pytest

from tests import _stokes_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stokes_pins.npz")
NORMAL_EQ_TOL = 1e-9   # the weighted normal equations square the condition of A; measured 2e-13
FORMULA_TOL = 1e-13    # the written-out diagonal formulas differ from the oracle in rounding only; measured 9e-16


@functools.lru_cache(maxsize=None)
def pins():
    return dict(np.load(GOLDEN))


def test_stokes_products_agrees_with_every_recorded_selection():
    from pfb_imaging_amd.utils.stokes import stokes_products

    d = pins()
    assert d["sel_case"].size == 10 * 3 * 4 * 3 * 3
    gaps = 0
    for case, want in zip(d["sel_case"], d["sel_result"]):
        product, pol, nc, mode, ndim = str(case).split("|")
        ndim, want = int(ndim), str(want)
        try:
            got = stokes_products(product, pol, nc, mode, ndim)
        except Exception as e:  # noqa: BLE001  (the class is what is compared)
            got = "!" + type(e).__name__
        if not want.startswith("!") and mode == "minvar":
            # the one documented gap: the reference selects WEIGHT_MINVAR expressions for a diagonal Jones
            assert ndim == 5 and "WEIGHT_MINVAR" in want and got == "!NotImplementedError", case
            gaps += 1
            continue
        if want.startswith("!"):
            assert got == want, case
            continue
        vis_keys, wgt_keys = ([k.split("/") for k in part.split(",")] for part in want.split("#"))
        jmode = "JONES" if ndim == 6 else "DIAGJONES"
        assert [k[:3] for k in vis_keys] == [["VIS", pol.upper(), jmode]] * len(vis_keys), case
        assert [k[:3] for k in wgt_keys] == [["WEIGHT", pol.upper(), jmode]] * len(wgt_keys), case
        assert tuple(k[3] for k in vis_keys) == tuple(k[3] for k in wgt_keys) == got, case
    assert gaps > 0


def test_minvar_is_a_stated_gap_not_a_fallback():
    from pfb_imaging_amd.utils.stokes import stokes_products

    with pytest.raises(NotImplementedError, match="could not be read on the build machine"):
        stokes_products("I", "linear", "4", "minvar", 5)
    with pytest.raises(NotImplementedError, match="full-Stokes"):
        stokes_products("I", "linear", "4", "minvar", 6)
    assert stokes_products("VQI", "linear", "4", "l2", 6) == ("I", "Q", "V")


def test_coherency_matrices_and_host_maps_match_the_reference():
    from pfb_imaging_amd.utils import stokes

    d = pins()
    for pol in ("linear", "circular"):
        t = stokes.coherency_matrix(pol)
        assert (t == d[f"T_{pol}"]).all() and (ref.T[pol] == d[f"T_{pol}"]).all()
        assert np.abs(t.conj().T @ t / 2 - np.eye(4)).max() == 0.0  # inv(T) = T^H / 2, which the kernel uses
    s, c, wsum = d["cube_stokes"], d["cube_corr"], float(d["cube_wsum"])
    assert np.abs(stokes.stokes_to_corr(s, axis=0) - d["s2c_axis0"]).max() <= 1e-15
    assert np.abs(stokes.stokes_to_corr(np.moveaxis(s, 0, 1), axis=1) - d["s2c_axis1"]).max() <= 1e-15
    got = stokes.corr_to_stokes(c, wsum=wsum, axis=0)
    assert got.dtype == np.float64 and np.abs(got - d["c2s_axis0"]).max() <= 1e-15
    assert np.abs(stokes.corr_to_stokes(np.moveaxis(c, 0, 1), wsum=wsum, axis=1) - d["c2s_axis1"]).max() <= 1e-15
    for f in (stokes.stokes_to_corr, stokes.corr_to_stokes):
        with pytest.raises(NotImplementedError):
            f(s, poltype="circular")
        with pytest.raises(ValueError, match="Expected 4 polarisation products"):
            f(s, axis=1)


@pytest.mark.parametrize("full", [False, True], ids=["diag", "full"])
@pytest.mark.parametrize("pol", ["linear", "circular"])
def test_oracle_against_normal_equations_and_written_out_formulas(pol, full):
    rng = np.random.default_rng(7 + 2 * full + (pol == "circular"))
    n = 20000
    v = rng.standard_normal((n, 4)) + 1j * rng.standard_normal((n, 4))
    w = rng.uniform(0.1, 2.0, (n, 4))
    jp, jq = ref.random_jones(rng, (n,), full), ref.random_jones(rng, (n,), full)
    jpm, jqm = (jp, jq) if full else (ref.full_of_diag(jp), ref.full_of_diag(jq))
    s, ws = ref.stokes_of_samples(v, w, jpm, jqm, pol, not full)
    err = ref.rel_diff(*ref.normal_equations(v, w, jpm, jqm, pol), s, ws)
    print(f"{pol} {'full' if full else 'diag'}: normal equations {err:.2e}")
    assert err <= NORMAL_EQ_TOL
    if not full:
        # a diagonal Jones through the full-Jones branch of the oracle, and (linear feeds) the formulas as written out
        err = ref.rel_diff(*ref.stokes_of_samples(v, w, jpm, jqm, pol, False), s, ws)
        print(f"  diagonal terms through the adjugate branch {err:.2e}")
        assert err <= FORMULA_TOL
        if pol == "linear":
            err = ref.rel_diff(*ref.diagonal_formulas(v, w, jp, jq), s, ws)
            print(f"  written-out formulas {err:.2e}")
            assert err <= FORMULA_TOL


def test_rounding_scale_of_the_gpu_tests():
    d = ref.rounding_scale()
    print(f"d = {d:.3e}")
    assert 2.0**-53 < d < 1e-13  # a few roundings of well-conditioned 2x2 algebra: anything else means the oracle changed


def small_case(rng, nrow=6, nchan=3, nant=4, nt=2, nc=4, full=False):
    data = rng.standard_normal((nrow, nchan, nc)) + 1j * rng.standard_normal((nrow, nchan, nc))
    weight, flag = rng.uniform(0.5, 1.5, (nrow, nchan, nc)), np.zeros((nrow, nchan, nc), dtype=bool)
    jones = ref.random_jones(rng, (nt, nant, nchan, 1), full)
    tbin_idx, tbin_counts = np.array([0, nrow // 2]), np.array([nrow // 2, nrow - nrow // 2])
    ant1, ant2 = rng.integers(0, nant, nrow), rng.integers(0, nant, nrow)
    return [data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2]


def test_bad_indices_and_shapes_are_refused_on_the_host():
    """Every refusal comes before the first device call, so it is the same with and without a GPU."""
    from pfb_imaging_amd.utils.weighting import weight_data, weight_data_dev

    rng = np.random.default_rng(3)
    tail = ("linear", "I", "4", "l2")
    for entry in (weight_data, weight_data_dev):
        for dtype in (np.int32, np.int64):
            for which, value in ((6, 4), (7, -1), (6, 2**32 + 1)):
                if dtype == np.int32 and value > 2**31:
                    continue
                a = small_case(rng)
                a[which] = a[which].astype(dtype)
                a[which][4] = value
                with pytest.raises(ValueError, match="antenna"):
                    entry(*a, *tail)
        a = small_case(rng)
        a[5] = np.array([3, 4])  # the second bin ends at row 7 of 6
        with pytest.raises(ValueError, match="time bin 1 covers rows"):
            entry(*a, *tail)
        a = small_case(rng)
        a[5] = np.array([3, -1])
        with pytest.raises(ValueError, match="time bin"):
            entry(*a, *tail)
        a = small_case(rng)
        a[3] = a[3][:1]  # one Jones time slot for two bins
        with pytest.raises(ValueError, match="time slots"):
            entry(*a, *tail)
        for which, bad in ((1, lambda x: x[:-1]), (2, lambda x: x[:, :-1]), (3, lambda x: x[:, :, :-1]), (6, lambda x: x[:-1]),
                           (4, lambda x: x[:1]), (0, lambda x: x[:, :, :2])):
            a = small_case(rng)
            a[which] = bad(a[which])
            with pytest.raises(ValueError):
                entry(*a, *tail)
        with pytest.raises(ValueError, match="Full 2x2 jones mode requires 4 correlation data"):
            entry(*small_case(rng, nc=2, full=True), "linear", "I", "2", "l2")
        with pytest.raises(ValueError, match="V is not available in linear"):
            entry(*small_case(rng, nc=2), "linear", "IV", "2", "l2")
        with pytest.raises(NotImplementedError):
            entry(*small_case(rng), "linear", "I", "4", "minvar")
        with pytest.raises(TypeError):
            a = small_case(rng)
            a[0] = a[0].real
            entry(*a, *tail)


def test_the_library_refuses_them_too():
    from pfb_imaging_amd import _lib

    rng = np.random.default_rng(4)
    data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2 = small_case(rng)
    L = _lib.lib()
    vis, wgt = np.empty((6, 3, 1), dtype=np.complex128), np.empty((6, 3, 1))
    jones, flag = np.ascontiguousarray(jones[:, :, :, 0]), flag.astype(np.uint8)
    tbin_idx, tbin_counts = tbin_idx.astype(np.int64), tbin_counts.astype(np.int64)

    def call(spec, a1=ant1, counts=tbin_counts, ntime=2, data=data):
        a1, a2 = np.ascontiguousarray(a1, dtype=np.int32), np.ascontiguousarray(ant2, dtype=np.int32)
        return L.pfbhip_weight_data(ct.byref(spec), _lib.i64(6), _lib.i64(3), _lib.i64(4), _lib.i64(ntime), _lib.i64(2),
                                    _lib.ptr(data), _lib.ptr(weight), _lib.ptr(flag), _lib.ptr(jones), _lib.ptr(tbin_idx),
                                    _lib.ptr(counts), _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(vis), _lib.ptr(wgt), None, None)

    def spec(nc=4, full=0, circ=0, products=(0,)):
        return _lib.StokesSpec(nc, full, circ, len(products), (_lib.i32 * 4)(*products), 0, 0)

    bad_ant = ant1.copy()
    bad_ant[0] = 4
    for kw, needle in ((dict(spec=spec(), a1=bad_ant), "antennas"), (dict(spec=spec(), counts=np.array([3, 4])), "time bin 1"),
                       (dict(spec=spec(), ntime=1), "time slots"), (dict(spec=spec(nc=2, full=1)), "Full 2x2 jones"),
                       (dict(spec=spec(nc=3)), "nc must be 2 or 4"), (dict(spec=spec(products=(1, 0))), "ascending"),
                       (dict(spec=spec(nc=2, products=(0, 3))), "V is not available in linear"),
                       (dict(spec=spec(nc=2, circ=1, products=(1,))), "Q is not available in circular"),
                       (dict(spec=spec(products=())), "between one and four"), (dict(spec=spec(), data=None), "NULL")):
        assert call(**kw) == 1 and needle in _lib.last_error(), (needle, _lib.last_error())


def test_as_contiguous_readonly_view():
    from pfb_imaging_amd.utils.weighting import as_contiguous_readonly_view

    a = np.arange(12.0).reshape(3, 4)
    v = as_contiguous_readonly_view(a)
    assert not v.flags.writeable and v.flags.c_contiguous and np.shares_memory(v, a) and a.flags.writeable
    t = as_contiguous_readonly_view(a.T)
    assert not t.flags.writeable and t.flags.c_contiguous and (t == a.T).all() and not np.shares_memory(t, a)
