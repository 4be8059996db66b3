#!/usr/bin/env python3
"""Reference-RUN fixtures of Hogbom and Clark CLEAN: ``clean_pins.npz``.

Like make_numba_pins.py, this reads the reference's files AT GENERATION TIME and executes them AS THEY STAND:
``deconv/hogbom.py`` and ``deconv/clark.py`` are loaded WHOLE (importlib, unmodified) under their own dotted names, and
``hogbom``, ``clark`` and (through ``clark``) ``subminor`` are called.  No reference text is stored: only outputs and ``cites``
go into the ``.npz``; the inputs are rebuilt from tests/_clean_cases.py ``case()`` by whoever compares.

The stand-ins those two files import, exactly (all removed from ``sys.modules`` afterwards):

  * ``numba``: make_numba_pins.py's stand-in (``njit(**kw)`` is the identity decorator, every option ignored; ``prange = range``),
    so ``subminor`` is CPython evaluating the reference's statements one by one in IEEE double, bands and pixels in order;
  * ``numexpr``: a module with ``evaluate(expr, local_dict, out, casting)``, which is ``out[...] = eval(expr)`` over
    ``local_dict`` alone with numpy's operators (so "residual - gamma * xhat * psf" is residual - ((gamma * xhat) * psf));
    every value of ``local_dict`` goes through ``np.asarray`` first, which is how numexpr types its operands: a Python-float
    ``gamma`` is a double operand, so with float32 cubes the expression is evaluated in double and rounded to float32 on the
    store into ``out`` (numpy >= 2 promotes a 0-d float64 array like any array); with float64 cubes it changes nothing.
    ``casting`` is ignored (float64 -> float32 is "same_kind");
  * ``ducc0.misc.empty_noncritical(shape, dtype)`` is ``np.empty``;
  * ``pfb_imaging.operators.psf`` holds ``psf_convolve_cube`` taken from operators/psf.py by make_ref_pins.py's ``take()``
    (undecorated, unmodified); the ``r2c`` / ``c2r`` it calls are bound to stand-ins with ducc0's argument meaning (``axes``,
    ``forward``, ``inorm`` 0 / 2, ``lastsize``, ``out``) over an FFT module, numpy.fft (``_np``) or scipy.fft (``_sp``);
    ``psf_convolve_fscube`` is bound to None (fsclark is not run);
  * ``pfb_imaging.utils.logging.get_logger(name)`` returns a stub whose ``info`` appends the message to a list.

The reference returns ``(model, status)``.  The iteration count k is read from its own log line with ``verbosity=1``:
"converged after {k} iterations", or "Max iters reached" (then k = maxit).  The sub-minor count is not exposed; the tests
compare it with the yardstick, which this script shows to reproduce every pinned model bit for bit over numpy.fft.

Every run is under ``np.errstate(all="raise")``: a pinned case has no division by zero and no non-finite value.

Class E (every Hogbom case, Clark with maxit = 1: the model is complete before the first convolution): model, k, status.
Class T (Clark, several major cycles): the model over numpy.fft and over scipy.fft, their disagreement relative to the model's
max-abs, and a third run on ``dirty * (1 + 1e-9 h)``; the three runs must agree on support, k and status, or the case is
reshaped.  Models are stored sparsely: flat indices into the cube and the values there.

Class F (H6: float32 inputs; the reference computes in ``dirty.dtype``): the float32 model, k and status, after asserting that
the float64 run of the reference on the same numbers takes the same k, status and support.  It did (the two models differ by
7.9e-8 of the maximum), so the case is not chaotic and is pinned, with that disagreement stored beside it: the tests allow ten
times it, as class T does with its own.

Not pinned because the reference is undefined there, and shown below to be: a band with ``wsums == 0`` (division by zero in
``subminor``), a Hogbom PSF smaller than 2 nx - 1 (the slice comes out short and the subtraction raises).

Run from the repo root in the build container:  python tests/golden/make_clean_pins.py
"""

import importlib.util
import io
import os
import re
import sys
import types
import zipfile

import numpy as np
import scipy.fft

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_mrp, _mnp = _load("make_ref_pins"), _load("make_numba_pins")
take, REF, SRC = _mrp.take, _mrp.REF, _mnp.SRC

LOG = []


def fft_standins(fft):
    def r2c(a, axes, forward=True, nthreads=1, inorm=0, out=None):
        assert forward and inorm == 0
        out[...] = fft.rfftn(a, axes=axes)
        return out

    def c2r(a, axes, forward=False, lastsize=None, inorm=2, nthreads=1, out=None, allow_overwriting_input=False):
        assert not forward and inorm == 2 and lastsize is not None
        s = [a.shape[ax] for ax in axes]
        s[-1] = lastsize
        out[...] = fft.irfftn(a, s=s, axes=axes)  # carries the 1 / N of inorm = 2
        return out

    return r2c, c2r


def load_reference():
    """(hogbom module, clark module, namespace of psf_convolve_cube, cites)"""
    _mnp.install_standin()
    ne = types.ModuleType("numexpr")

    def evaluate(expr, local_dict=None, out=None, casting=None):
        out[...] = eval(expr, {"__builtins__": {}}, {k: np.asarray(v) for k, v in local_dict.items()})
        return out

    ne.evaluate = evaluate
    ducc0, misc = types.ModuleType("ducc0"), types.ModuleType("ducc0.misc")
    misc.empty_noncritical = lambda shape, dtype=None: np.empty(shape, dtype=dtype)
    ducc0.misc = misc
    rel_psf = f"{SRC}/operators/psf.py"
    psf_ns, found = take(rel_psf, ["psf_convolve_cube"])
    psf_mod = types.ModuleType("pfb_imaging.operators.psf")
    psf_mod.psf_convolve_cube, psf_mod.psf_convolve_fscube = psf_ns["psf_convolve_cube"], None
    log_mod = types.ModuleType("pfb_imaging.utils.logging")
    log_mod.get_logger = lambda name: types.SimpleNamespace(info=lambda msg, *a: LOG.append(msg % a if a else msg))
    stubs = {"numexpr": ne, "ducc0": ducc0, "ducc0.misc": misc, "pfb_imaging.operators.psf": psf_mod,
             "pfb_imaging.utils.logging": log_mod}
    for name in ("pfb_imaging", "pfb_imaging.operators", "pfb_imaging.utils", "pfb_imaging.deconv"):
        stubs[name] = types.ModuleType(name)
        stubs[name].__path__ = []
    stubs["pfb_imaging.utils"].logging = log_mod
    sys.modules.update(stubs)
    mods = {}
    try:
        for leaf in ("hogbom", "clark"):
            name = f"pfb_imaging.deconv.{leaf}"
            spec = importlib.util.spec_from_file_location(name, os.path.join(REF, SRC, "deconv", leaf + ".py"))
            mods[leaf] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[leaf])
    finally:
        for name in list(sys.modules):
            if name.split(".")[0] in ("pfb_imaging", "numexpr", "ducc0", "numba"):
                del sys.modules[name]
    cites = [f"{rel_psf}:{a}-{b} {k}" for k, (a, b) in found.items()]
    for leaf, names in (("hogbom", ["hogbom"]), ("clark", ["subminor", "clark"])):
        for n in names:
            code = getattr(mods[leaf], n).__code__
            last = max(ln for _, _, ln in code.co_lines() if ln)
            cites.append(f"{SRC}/deconv/{leaf}.py:{code.co_firstlineno}-{last} {n}")
    cites += ["numba: njit = identity, prange = range; numexpr.evaluate = eval over local_dict with numpy into out",
              "ducc0.misc.empty_noncritical = np.empty; ducc0.fft.r2c / c2r bound to numpy.fft (_np) and scipy.fft (_sp) stand-ins",
              "k from the reference's log line: 'converged after {k} iterations' / 'Max iters reached' (k = maxit)"]
    return mods["hogbom"], mods["clark"], psf_ns, cites


def run_reference(ref, c, fft=np.fft, dirty=None):
    """(model, status, k) of one reference run under errstate(all='raise')"""
    from tests import _clean_cases as cc

    hog, clk, psf_ns, _ = ref
    psf_ns["r2c"], psf_ns["c2r"] = fft_standins(fft)
    dirty = c["dirty"] if dirty is None else dirty
    del LOG[:]
    with np.errstate(all="raise"):
        if c["kind"] == "hogbom":
            model, status = hog.hogbom(dirty.copy(), np.array(c["psf"]), verbosity=1, **c["kw"])
        else:
            model, status = clk.clark(dirty.copy(), np.array(c["psf"]), cc.psfhat(c["psf"]), c["wsums"].copy(), c["mask"].copy(),
                                      verbosity=1, **c["kw"])
    assert len(LOG) == 1, LOG
    m = re.search(r"converged after (\d+) iterations", LOG[0])
    if m:
        k = int(m.group(1))
    else:
        assert LOG[0].startswith("Max iters reached"), LOG[0]
        k = int(c["kw"]["maxit"])
    assert np.isfinite(model).all()
    return model, int(status), k


def run_yardstick(c, dirty=None):
    """(model, status, k, nminor) of tests/_clean_ref.py"""
    from tests import _clean_cases as cc
    from tests import _clean_ref as yard

    dirty = c["dirty"] if dirty is None else dirty
    if c["kind"] == "hogbom":
        model, _, k, status = yard.hogbom(dirty, c["psf"], **c["kw"])
        return model, status, k, k
    model, _, k, status, nminor = yard.clark(dirty, c["psf"], cc.psfhat(c["psf"]), c["wsums"], c["mask"], **c["kw"])
    return model, status, k, nminor


def undefined_in_the_reference(ref):
    from tests import _clean_cases as cc

    c = cc.case("T1")
    c["wsums"] = np.array([0.5, 0.0, 0.5])
    try:
        run_reference(ref, c)
        raise AssertionError("wsums == 0 ran clean")
    except (FloatingPointError, ZeroDivisionError):
        pass
    c = cc.case("H1")
    c["psf"] = cc.tent_psf(2, 2 * cc.NX - 2, 2 * cc.NY - 2)
    try:
        run_reference(ref, c)
        raise AssertionError("a PSF smaller than 2 nx - 1 ran clean")
    except ValueError:
        pass


def compute():
    from tests import _clean_cases as cc

    ref = load_reference()
    out = {}
    for name in cc.E_CASES:
        c = cc.case(name)
        assert c["cls"] == "E" and (c["kind"] == "hogbom" or c["kw"]["maxit"] == 1)
        model, status, k = run_reference(ref, c)
        ym, ys, yk, yn = run_yardstick(c)
        idx, val = cc.sparse(model)
        out.update({f"{name}_idx": idx, f"{name}_val": val, f"{name}_k": np.int64(k), f"{name}_status": np.int64(status)})
        print(f"{name}: k {k} status {status} components {idx.size} sub-minor (yardstick) {yn}; yardstick bit-equal "
              f"{np.array_equal(ym, model) and (ys, yk) == (status, k)}")
    for name in cc.CLARK_T_CASES:
        c = cc.case(name)
        assert c["cls"] == "T" and c["kw"]["maxit"] > 1
        runs = {"np": run_reference(ref, c, np.fft), "sp": run_reference(ref, c, scipy.fft),
                "pert": run_reference(ref, c, np.fft, cc.perturbed(c["dirty"]))}
        (m_np, status, k), idx = runs["np"], cc.sparse(runs["np"][0])[0]
        for tag, (m, s, kk) in runs.items():
            assert (s, kk) == (status, k) and np.array_equal(cc.sparse(m)[0], idx), f"{name}: the {tag} run differs in support, k or status"
        ym, ys, yk, yn = run_yardstick(c)
        dis = cc.rel_max(runs["sp"][0], m_np)
        out.update({f"{name}_idx": idx, f"{name}_val": cc.sparse(m_np)[1], f"{name}_sp_val": runs["sp"][0].reshape(-1)[idx],
                    f"{name}_disagreement": np.float64(dis), f"{name}_k": np.int64(k), f"{name}_status": np.int64(status)})
        print(f"{name}: k {k} status {status} components {idx.size} sub-minor (yardstick) {yn}; numpy vs scipy {dis:.3e}, perturbed "
              f"input {cc.rel_max(runs['pert'][0], m_np):.3e}; yardstick bit-equal {np.array_equal(ym, m_np) and (ys, yk) == (status, k)}")
    for name in cc.F32_CASES:
        c = cc.case(name)
        assert c["cls"] == "F" and c["dirty"].dtype == c["psf"].dtype == np.float32
        model, status, k = run_reference(ref, c)
        wide = dict(c, dirty=c["dirty"].astype(np.float64), psf=c["psf"].astype(np.float64))
        m64, s64, k64 = run_reference(ref, wide)
        assert model.dtype == np.float32 and (s64, k64) == (status, k) and np.array_equal(m64 != 0, model != 0), f"{name} is chaotic"
        idx, val = cc.sparse(model)
        dis = cc.rel_max(model, m64)
        out.update({f"{name}_idx": idx, f"{name}_val": val, f"{name}_k": np.int64(k), f"{name}_status": np.int64(status),
                    f"{name}_disagreement": np.float64(dis)})
        print(f"{name}: k {k} status {status} components {idx.size}; float32 vs float64 reference run {dis:.3e}")
    undefined_in_the_reference(ref)
    out["cases"] = np.array(cc.ALL_CASES)
    out["cites"] = np.array(ref[3])
    return out


def save(path, out):
    """np.savez_compressed with fixed member times, so the file regenerates byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    out = compute()
    path = os.path.join(HERE, "clean_pins.npz")
    save(path, out)
    print("\n".join(out["cites"]))
    print("clean_pins.npz", os.path.getsize(path))
    assert os.path.getsize(path) < 500_000


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("make_clean_pins.py needs the reference checkout (build container only); the committed .npz travels instead")
    main()
