"""CPU tests of the drop-in boundary: the C-ABI library loads without a GPU, exports every symbol
include/pfbhip.h declares, the signatures the binding takes from that header are the compiler's, every call site passes what
they say, its structs match the ctypes mirror, and it fails loudly without a GPU."""

import ctypes as ct
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pfbhip.h")


def _declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pfbhip_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from pfb_imaging_amd import _lib

    L = _lib.lib()
    declared = _declared_symbols()
    assert len(declared) >= 45
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, missing
    assert sorted(_lib.SYMBOLS) == declared


def _gcc(tmp_path, source, *flags):
    src = tmp_path / "probe.c"
    src.write_text(source)
    return subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), *flags, str(src)], capture_output=True, text=True)


def test_parsed_prototypes_match_the_compiler(tmp_path):
    """The loader's parser against an independent reader of the header: for every prototype it found, a function pointer
    spelled from the PARSED return and parameter types must take the address of the function as pfbhip.h declares it."""
    from pfb_imaging_amd import _lib

    protos = _lib.parse_prototypes(open(HEADER).read())
    assert sorted(protos) == _declared_symbols() and len(protos) >= 45   # one prototype per name, none missed

    def pointer(name, ret, params):
        return f"{ret} (*const p_{name})({', '.join(params) or 'void'}) = &{name};\n"

    strict = ("-fsyntax-only", "-Wall", "-Werror", "-Werror=incompatible-pointer-types")
    head = '#include "pfbhip.h"\n'
    r = _gcc(tmp_path, head + "".join(pointer(n, *p) for n, p in protos.items()), *strict)
    assert r.returncode == 0, r.stderr
    # the same flags do refuse a wrong width, a wrong count and a dropped qualifier (so a pass above means agreement)
    for wrong in (("int64_t", ["int", "int"]), ("int64_t", ["int64_t"]), ("int64_t", ["int64_t", "int", "int"])):
        assert _gcc(tmp_path, head + pointer("pfbhip_good_size", *wrong), *strict).returncode != 0, wrong
    assert _gcc(tmp_path, head + pointer("pfbhip_hash64", "uint64_t", ["void *", "size_t"]), *strict).returncode != 0


def test_ctypes_signatures_by_example():
    """The C-to-ctypes mapping, pinned by hand on one entry point of each kind, as the loaded library carries it."""
    from pfb_imaging_amd import _lib

    L = _lib.lib()
    vp, i64, f64, cint, size_t = ct.c_void_p, ct.c_int64, ct.c_double, ct.c_int, ct.c_size_t
    expect = {
        "pfbhip_last_error": (ct.c_char_p, []),
        "pfbhip_thread_pool_size": (cint, []),
        "pfbhip_good_size": (i64, [i64, cint]),
        "pfbhip_hash64": (ct.c_uint64, [vp, size_t]),
        "pfbhip_gridder_create": (cint, [vp] * 5),
        "pfbhip_gridder_hessian_sp": (cint, [vp, vp, vp, f64, f64, vp]),
        "pfbhip_psfconv_power_method": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, f64, cint, vp, vp]),
        "pfbhip_pd_iterate_dev": (cint, [vp, vp]),
        "pfbhip_psi_create": (cint, [i64, i64, ct.c_int32, vp, ct.c_int32, vp]),
        "pfbhip_chunk_average_dev": (cint, [vp, vp, vp, i64, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp]),
    }
    for name, (restype, argtypes) in expect.items():
        f = getattr(L, name)
        assert (f.restype, list(f.argtypes)) == (restype, argtypes), name
    for name in _lib.SYMBOLS:   # every entry point got a signature of the right length, not only the examples
        assert getattr(L, name).argtypes is not None, name


def test_wrong_arguments_fail_before_the_call():
    """A float for an integer parameter and a wrong argument count are refused by ctypes, on entries that validate before they
    touch a device."""
    from pfb_imaging_amd import _lib

    L = _lib.lib()
    # (fetched by name: the audit of the call sites below reads every literal call, and these are wrong on purpose)
    good_size, get_info = getattr(L, "pfbhip_good_size"), getattr(L, "pfbhip_gridder_get_info")
    assert good_size(10, 0) == 10 and good_size(np.int64(127), True) == 128
    for bad in (10.5, ct.c_double(10.0), ct.c_int(10), "10", None):
        with pytest.raises(ct.ArgumentError):
            good_size(bad, 0)
    with pytest.raises(ct.ArgumentError):
        get_info(None, 1.5)
    # ctypes reports a wrong type as ArgumentError and a missing argument as TypeError.  It passes SURPLUS arguments of a
    # cdecl function on, as C does for a variadic one: those only the audit of the call sites below finds.
    with pytest.raises(TypeError, match="takes at least 2 arguments"):
        get_info(None)
    with pytest.raises(TypeError, match="takes at least 2 arguments"):
        good_size(10)


def test_unknown_c_type_fails_the_load():
    from pfb_imaging_amd import _lib

    header = "int pfbhip_fine(int64_t n, const double *x);\nint pfbhip_odd(float level, int n);\n"
    with pytest.raises(ImportError, match=r"unknown parameter type 'float' in `int pfbhip_odd\(float, int\)`"):
        _lib.signatures(header)
    with pytest.raises(ImportError, match=r"unknown return type 'void' in `void pfbhip_odd\(int\)`"):
        _lib.signatures("void pfbhip_odd(int n);\n")
    with pytest.raises(ImportError, match="pfbhip_odd"):     # an unnamed parameter is not guessed at either
        _lib.signatures("int pfbhip_odd(int);\n")
    assert _lib.signatures(header.splitlines()[0]) == {"pfbhip_fine": (ct.c_int, [ct.c_int64, ct.c_void_p])}


MIRRORS = {"gridder_params": "GridderParams", "gridder_info": "GridderInfo", "cg_info": "CGInfo", "pm_info": "PMInfo",
           "pd_info": "PDInfo", "pd_traffic": "PDTraffic", "clean_info": "CleanInfo", "fb_info": "FBInfo", "dft_conv": "DFTConv",
           "cleanbeam_info": "CleanbeamInfo", "stokes_spec": "StokesSpec"}
CONSTANTS = {"PFBHIP_NSTAGES": "NSTAGES", "PFBHIP_PD_NSTAGES": "PD_NSTAGES", "PFBHIP_FB_NSTAGES": "FB_NSTAGES",
             "PFBHIP_UNIQUE_ID_BYTES": "UNIQUE_ID_BYTES"}


def _declared_structs():
    """{struct name without the prefix: [field names in order]} of every struct body in the header."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*pfbhip_(\w+)\s*;", text):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            declarators = decl.split(None, 1)[1]            # "int64_t nu, nv" / "double f, p0[3]": a one-word type, then names
            fields += [re.sub(r"\[.*\]", "", d).strip() for d in declarators.split(",")]
        structs[name] = fields
    return structs


def test_struct_layout_matches_header(tmp_path):
    """Every field of every struct of the header: size and offset as gcc lays them out against the ctypes mirror, the mirror
    having the same field names in the same order; and the array-length constants the mirrors are built with."""
    from pfb_imaging_amd import _lib

    structs = _declared_structs()
    assert sorted(structs) == sorted(MIRRORS) and len(structs) == 11
    lines = ['#include <stdio.h>\n#include <stddef.h>\n#include "pfbhip.h"\nint main(void){\n']
    for c in CONSTANTS:
        lines.append(f'printf("%d\\n", (int){c});\n')
    for s, fields in structs.items():
        lines.append(f'printf("%zu\\n", sizeof(pfbhip_{s}));\n')
        for f in fields:
            lines.append(f'printf("%zu %zu\\n", offsetof(pfbhip_{s}, {f}), sizeof(((pfbhip_{s} *)0)->{f}));\n')
    exe = tmp_path / "layout"
    r = _gcc(tmp_path, "".join(lines) + "return 0;}\n", "-o", str(exe))
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    expect = [getattr(_lib, py) for py in CONSTANTS.values()]
    for s, fields in structs.items():
        mirror = getattr(_lib, MIRRORS[s])
        assert [n for n, _ in mirror._fields_] == fields, s
        expect.append(ct.sizeof(mirror))
        for f in fields:
            expect += [getattr(mirror, f).offset, getattr(mirror, f).size]
    assert got == expect
    assert len(_lib.STAGE_NAMES) == _lib.NSTAGES and len(_lib.PD_STAGE_NAMES) == _lib.PD_NSTAGES
    assert len(_lib.FB_STAGE_NAMES) == _lib.FB_NSTAGES


# calls that splat an argument tuple cannot be counted statically (argtypes check them when the GPU suite runs them); a new
# one has to be added here on purpose
SPLAT_CALLS = sorted([
    ("pfb-imaging_amd/comps.py", "pfbhip_comps_regrid"), ("pfb-imaging_amd/comps.py", "pfbhip_comps_regrid_dev"),
    ("pfb-imaging_amd/opt.py", "pfbhip_pd_create"), ("pfb-imaging_amd/opt.py", "pfbhip_primal_dual"),
    ("pfb-imaging_amd/opt.py", "pfbhip_fb_create"), ("pfb-imaging_amd/opt.py", "pfbhip_psfconv_power_method"),
    ("pfb-imaging_amd/gaussconv.py", "pfbhip_gaussconv_shape"),
    ("pfb-imaging_amd/gaussconv.py", "pfbhip_gaussconv_apply"), ("pfb-imaging_amd/gaussconv.py", "pfbhip_gaussconv_apply_dev"),
    ("pfb-imaging_amd/gaussconv.py", "pfbhip_gaussconv_restore"), ("pfb-imaging_amd/gaussconv.py", "pfbhip_gaussconv_restore_dev"),
    ("pfb-imaging_amd/utils/weighting.py", "pfbhip_weight_data_dev"),
    ("tests/test_gpu_beam.py", "pfbhip_beam_regrid"), ("tests/test_gpu_beam.py", "pfbhip_beam_regrid"),
    ("tests/test_gpu_restore.py", "pfbhip_gaussconv_apply_dev"), ("tests/test_gpu_restore.py", "pfbhip_gaussconv_restore_dev"),
])
# a ctypes constructor written in place as an argument, by its last name, and the C type it states
CONSTRUCTORS = {"cint": "int", "c_int": "int", "i32": "int32_t", "c_int32": "int32_t", "i64": "int64_t", "c_int64": "int64_t",
                "c_longlong": "int64_t", "c_long": "int64_t", "f64": "double", "c_double": "double", "c_size_t": "size_t",
                "c_uint64": "uint64_t", "c_ulong": "uint64_t", "c_float": "float", "c_uint32": "uint32_t", "c_uint": "uint32_t",
                "c_int16": "int16_t", "c_short": "int16_t", "c_int8": "int8_t", "c_uint8": "uint8_t", "c_bool": "bool"}
SAME = {"int32_t": "int", "uint64_t": "size_t"}


def test_call_sites_match_the_header():
    """Every literal ``.pfbhip_name(...)`` call in the product, the tests, the tools and the benchmark passes the declared
    number of positional arguments and no keywords, and a ctypes constructor written as an argument names the declared type."""
    import ast
    import glob

    from pfb_imaging_amd import _lib

    protos = _lib.parse_prototypes(open(HEADER).read())
    files = [os.path.join(ROOT, "bench.py")]
    for d in ("pfb-imaging_amd", "tests", "tools"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    splats, wrong, ncalls = [], [], 0
    for path in sorted(files):
        rel = os.path.relpath(path, ROOT)
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in protos):
                continue
            name, where = node.func.attr, f"{rel}:{node.lineno}"
            params = protos[name][1]
            ncalls += 1
            if node.keywords:
                wrong.append(f"{where} {name}: keyword arguments")
            if any(isinstance(a, ast.Starred) for a in node.args):
                splats.append((rel, name))
                continue
            if len(node.args) != len(params):
                wrong.append(f"{where} {name}: {len(node.args)} arguments, the header declares {len(params)}")
                continue
            for k, (a, declared) in enumerate(zip(node.args, params)):
                f = a.func if isinstance(a, ast.Call) else None
                stated = CONSTRUCTORS.get(getattr(f, "id", None) or getattr(f, "attr", None))
                if stated is not None and SAME.get(stated, stated) != SAME.get(declared, declared):
                    wrong.append(f"{where} {name}: argument {k} is written as {stated}, the header declares {declared}")
    assert not wrong, "\n".join(wrong)
    assert sorted(splats) == SPLAT_CALLS
    assert ncalls >= 150   # (the walk did find the call sites: about 200 in the product alone)


def test_no_gpu_paths_fail_loudly_or_work_on_host():
    from pfb_imaging_amd import _lib, fft, misc

    L = _lib.lib()
    assert fft.good_size(11468) == 11520
    assert fft.good_size(127, True) == 128
    misc.resize_thread_pool(7)
    assert misc.thread_pool_size() == 7
    assert misc.empty_noncritical((3, 4), "c16").shape == (3, 4)
    # invalid arguments are reported through the status / last-error channel (no exceptions cross the ABI)
    st = L.pfbhip_gridder_get_info(None, None)
    assert st == 1 and "NULL" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(st)
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _lib.require_gpu()
        from pfb_imaging_amd.wgridder import vis2dirty

        with pytest.raises(RuntimeError):
            vis2dirty(uvw=np.zeros((3, 3)), freq=np.ones(1), vis=np.zeros((3, 1), complex), npix_x=16, npix_y=16,
                      pixsize_x=1e-5, pixsize_y=1e-5, epsilon=1e-5, do_wgridding=True)


def test_unknown_scatter_switch_fails_plan_creation(monkeypatch):
    """PFBHIP_SCATTER is read before any device work: a value the plan does not know is refused, naming the valid ones."""
    from pfb_imaging_amd import _lib

    monkeypatch.setenv("PFBHIP_SCATTER", "records")
    p = _lib.GridderParams(nrow=1, nchan=1, nx=16, ny=16, pixsize_x=1e-5, pixsize_y=1e-5, epsilon=1e-5, sigma_min=1.1,
                           sigma_max=2.6, do_wgridding=1)
    uvw, freq, h = np.zeros((1, 3)), np.ones(1), ct.c_void_p()
    st = _lib.lib().pfbhip_gridder_create(ct.byref(p), uvw.ctypes.data_as(ct.c_void_p), freq.ctypes.data_as(ct.c_void_p),
                                          None, ct.byref(h))
    assert st != 0 and not h.value
    assert "PFBHIP_SCATTER=records: expected auto, walk, block, rec or rec_es" in _lib.last_error()


def test_product_never_imports_oracle():
    """The product path must not reach into the oracle (or any CPU fallback)."""
    pkg = os.path.join(ROOT, "pfb-imaging_amd")
    bad = []
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp")):
                text = open(os.path.join(dirpath, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M) or "libpfb_oracle" in text:
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad
    code = ("import sys; sys.path.insert(0, %r); import pfb_imaging_amd.operators.hessian, pfb_imaging_amd.operators.gridder, "
            "pfb_imaging_amd.operators.band_worker, pfb_imaging_amd.operators.psf, pfb_imaging_amd.utils.weighting; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_host_side_helpers():
    from pfb_imaging_amd.operators import LinearOperator, Preconditioner, require_protocol
    from pfb_imaging_amd.operators.gridder import psf_visibilities, wgridder_conventions
    from pfb_imaging_amd.operators.hessian import hessian_slice, taperf

    assert wgridder_conventions(0.1, -0.2) == (False, True, False, -0.1, 0.2)
    rng = np.random.default_rng(0)
    uvw = rng.standard_normal((10, 3)) * 100
    freq = np.array([1e9, 1.1e9])
    assert np.array_equal(psf_visibilities(uvw, freq, 0.0, 0.0), np.ones((10, 2)))
    x0, y0 = -0.1, 0.17
    n = np.sqrt(1 - x0**2 - y0**2)
    ref = np.exp(2j * np.pi * freq[None] / 299792458.0 * (uvw[:, 0:1] * x0 + uvw[:, 1:2] * y0 - uvw[:, 2:] * (n - 1)))
    np.testing.assert_allclose(psf_visibilities(uvw, freq, x0, y0), ref)
    t = taperf((64, 48), 8)
    assert t.shape == (64, 48) and t[32, 24] == 1.0 and t[0, 0] < 1e-2
    # zero-input shortcut never touches the device (hessian.py:47-48)
    assert not hessian_slice(np.zeros((8, 8))).any()

    class Bad:
        def dot(self, x):
            return x

    with pytest.raises(TypeError, match="hdot"):
        require_protocol(Bad(), LinearOperator, "hess")
    with pytest.raises(TypeError, match="Preconditioner"):
        require_protocol(Bad(), Preconditioner, "precond")


def test_content_hash_sees_every_byte():
    """The plan caches of the stateless calls are keyed on a hash of EVERY byte of uvw / freq / mask / weights / psfhat
    (the reference's ducc0 calls are stateless): a single flipped mask element, an in-place weight tweak, a swap of two
    elements and a reallocation with equal content must all be told apart / recognised."""
    from pfb_imaging_amd import _lib

    rng = np.random.default_rng(0)
    a = rng.standard_normal(1_000_003)
    k = _lib.content_key(a)
    assert k == _lib.content_key(a.copy())            # content, not address
    a[777_777] = np.nextafter(a[777_777], 10.0)       # one ulp, far from any "sample"
    k2 = _lib.content_key(a)
    assert k2 != k
    b = a.copy()
    b[[5, 6]] = b[[6, 5]]
    assert _lib.content_key(b) != k2                  # position-dependent
    m = np.ones((1001, 7), dtype=np.uint8)            # size not a multiple of 8: the tail bytes count too
    km = _lib.content_key(m)
    m[1000, 6] = 0
    assert _lib.content_key(m) != km
    assert _lib.content_key(m) != _lib.content_key(m.reshape(7, 1001))
    assert _lib.content_key(None) is None
    # read-only inputs are hashed once and remembered by address; anything writeable (also through a base) is not
    r = rng.standard_normal(4096)
    r.flags.writeable = False
    assert _lib._immutable(r) and not _lib._immutable(a)
    assert _lib.content_key(r) == _lib.content_key(r) and (r.ctypes.data, r.shape, r.dtype.str) in _lib._ro_memo
    base = rng.standard_normal(64)
    view = base[:32]
    view.flags.writeable = False
    assert not _lib._immutable(view)                  # still writeable through its base
    kv = _lib.content_key(view)
    base[3] += 1.0
    assert _lib.content_key(view) != kv
    # an owner that flips `writeable` on, edits in place and flips it off again: the memo's sampled fingerprint notices
    # (every word of a small array is sampled) and the entry is re-hashed
    own = rng.standard_normal(2048)
    own.flags.writeable = False
    ko = _lib.content_key(own)
    own.flags.writeable = True
    own[1234] += 1.0
    own.flags.writeable = False
    assert _lib.content_key(own) != ko
    # the memo is bounded by bytes as well as by entries
    assert _lib._ro_memo_bytes[0] == sum(v[0].nbytes for v in _lib._ro_memo.values()) <= _lib._RO_MEMO_BYTES


def test_pinned_results_are_capped(monkeypatch):
    """Live page-locked result bytes are bounded (PFBHIP_PINNED_MAX_MB): past the cap result arrays are ordinary numpy
    allocations.  (No GPU here: the allocator entry is replaced by one that records what it is asked for.)"""
    import ctypes as ct

    from pfb_imaging_amd import _lib

    bufs = []

    class FakeLib:
        def pfbhip_host_alloc(self, pp, nbytes):
            b = ct.create_string_buffer(nbytes)
            bufs.append(b)
            ct.cast(pp, ct.POINTER(ct.c_void_p))[0] = ct.addressof(b)
            return 0

        def pfbhip_host_free(self, p):
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: FakeLib())
    monkeypatch.setenv("PFBHIP_PINNED_RESULTS", "1")
    monkeypatch.setenv("PFBHIP_PINNED_MAX_MB", "5")
    monkeypatch.setattr(_lib, "_pinned_live", [0])
    monkeypatch.setattr(_lib, "_pinned_pool", [])
    monkeypatch.setattr(_lib, "_pinned_pooled", [0])
    a = _lib.result_empty((2 << 20,), np.uint8)    # 2 MiB: pinned
    b = _lib.result_empty((2 << 20,), np.uint8)    # 4 MiB live
    assert len(bufs) == 2 and _lib._pinned_live[0] == 4 << 20
    c = _lib.result_empty((2 << 20,), np.uint8)    # would be 6 MiB > 5: pageable
    assert len(bufs) == 2 and c.shape == a.shape
    del b                                           # back to the pool (still live), reused by the next request of that size
    import gc

    gc.collect()
    d = _lib.result_empty((2 << 20,), np.uint8)
    assert len(bufs) == 2 and _lib._pinned_live[0] == 4 << 20 and d.ctypes.data in (ct.addressof(x) for x in bufs)
    del a, c, d
    gc.collect()
