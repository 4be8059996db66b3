#!/usr/bin/env python3
"""Reference-RUN fixtures of the transient profiles: ``transient_pins.npz``.

Like make_restore_pins.py, this imports ``take()`` from make_ref_pins.py, takes the undecorated top-level functions
``generate_time_profile``, ``generate_frequency_profile`` and ``generate_transient_spectra`` out of the reference's parsed
``utils/transients.py`` and executes them AS THEY STAND on the cases of tests/_dft_ref.py ``transient_cases()``: the gaussian,
exponential and step pulses, alone and with periodicity (with and without ``total_duration``).  No reference source text is
stored: only outputs and ``cites`` go into the ``.npz``; the inputs are rebuilt by whoever compares.

Run from the repo root in the build container:  python tests/golden/make_transient_pins.py
"""

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("make_ref_pins", os.path.join(HERE, "make_ref_pins.py"))
_mrp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mrp)
take, REF = _mrp.take, _mrp.REF


def compute():
    from tests import _dft_ref as ref

    rel = "src/pfb_imaging/utils/transients.py"
    ns, found = take(rel, ["generate_time_profile", "generate_frequency_profile", "generate_transient_spectra"])
    out = {}
    for tag, (times, freqs, params) in ref.transient_cases().items():
        tprofile, fprofile = ns["generate_transient_spectra"](times, freqs, params)
        assert tprofile.shape == times.shape and fprofile.shape == freqs.shape and tprofile.any()
        out[f"{tag}_time"], out[f"{tag}_freq"] = tprofile, fprofile
        t = params["time"]
        out[f"{tag}_pulse"] = ns["generate_time_profile"](times - times[0], t["peak_time"], t["duration"], t["shape"])
        print(f"{tag}: time profile sum {tprofile.sum():.6f} max {tprofile.max():.6f}")
    f = next(iter(ref.transient_cases().values()))[2]["frequency"]
    out["power_law"] = ns["generate_frequency_profile"](np.array([0.8e9, 1.2e9, 2.0e9]), f["peak_flux"], f["reference_freq"],
                                                        f["spectral_index"])
    out["cites"] = np.array([f"{rel}:{a}-{b} {k}" for k, (a, b) in sorted(found.items())])
    return out


def main():
    out = compute()
    path = os.path.join(HERE, "transient_pins.npz")
    np.savez_compressed(path, **out)
    print("\n".join(out["cites"]))
    print("transient_pins.npz", os.path.getsize(path))
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("make_transient_pins.py needs the reference checkout (build container only); the committed .npz travels instead")
    main()
