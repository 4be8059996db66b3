#!/usr/bin/env python3
"""Reference-RUN fixtures for the primary-beam operations (csrc/beam.hip, utils/beam.py): beam_pins.npz.

Run from the repo root in the build container, where scipy and the reference checkout are present:
    python tests/golden/make_beam_pins.py

  * ``eval_beam`` (utils/beam.py:75-89 of the reference) is taken out of the parsed module at generation time and executed
    as it stands, the way make_ref_pins.py takes its functions; no source text is stored, only arrays and ``cites``.
  * the rotation mean calls ``scipy.ndimage.rotate`` exactly as utils/stokes2vis_msv4.py:405-409 does.

Regrid cases (keys ``rg_<case>_*``): node grids 5x4 (non-uniform) and 33x29, outputs 64x48 that straddle all four edges of
the node grid and hold points exactly on the first, the last and interior nodes, in the separable and in the 2-D form,
ncorr = 2; ``gp`` is the grid_partition case (33x29 beam, the second correlation identically 1.0, 64x48 image).
Rotation cases (keys ``rot_<n0>x<n1>_*``): a smooth elliptical beam plus 1 % noise at five shapes, three angle sets.
Inputs are rounded to float32 values (and stored as float32) to keep the file small; outputs are float64.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

ROT_SHAPES = ((33, 33), (40, 40), (48, 37), (64, 64), (96, 80))
ROT_ANGLES = {"lin25": np.linspace(0, 359, 25), "zero": np.array([0.0]), "q90_180": np.array([90.0, 180.0])}


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def smooth_beam(rng, nl, nm, ncorr=2):
    x, y = np.meshgrid(np.linspace(-1, 1, nl), np.linspace(-1, 1, nm), indexing="ij")
    out = []
    for c in range(ncorr):
        out.append(np.exp(-(x**2 / 0.5 + y**2 / (0.3 + 0.2 * c))) * (1.0 + 0.3 * c) + 0.01 * rng.standard_normal((nl, nm)))
    return f32(np.array(out))


def straddling_axis(rng, nodes, n):
    """``n`` ascending-ish output coordinates reaching a fifth of the span past both ends, some exactly on nodes."""
    span = nodes[-1] - nodes[0]
    x = np.linspace(nodes[0] - 0.2 * span, nodes[-1] + 0.2 * span, n) + 1e-3 * span * rng.standard_normal(n)
    x[n // 8 + 1] = nodes[0]
    x[n - n // 8 - 2] = nodes[-1]
    x[n // 2] = nodes[nodes.size // 2]
    x[n // 3] = nodes[1]
    return x


def main():
    from scipy import ndimage

    from make_ref_pins import take

    out, cites = {}, []
    rel = "src/pfb_imaging/utils/beam.py"
    ns, found = take(rel, ["eval_beam"])
    for k, (a, b) in sorted(found.items()):
        cites.append(f"{rel}:{a}-{b} {k}")
    eval_beam = ns["eval_beam"]
    rng = np.random.default_rng(20261020)

    grids = {
        "g5x4": (np.array([-1.0, -0.6, -0.1, 0.45, 1.3]), np.array([-0.9, -0.2, 0.1, 1.1])),
        "g33x29": (np.linspace(-2.0, 2.0, 33), np.linspace(-1.75, 1.75, 29)),
    }
    for name, (l_in, m_in) in grids.items():
        beam = smooth_beam(rng, l_in.size, m_in.size)
        l_out, m_out = straddling_axis(rng, l_in, 64), straddling_axis(rng, m_in, 48)
        ll, mm = np.meshgrid(l_out, m_out, indexing="ij")
        th = 0.3  # a rotated, sheared 2-D coordinate set: nothing separable about it
        ll2, mm2 = np.cos(th) * ll + np.sin(th) * mm, -np.sin(th) * ll + np.cos(th) * mm * 1.1
        for k, (i, j) in enumerate(((0, 0), (-1, -1), (0, -1), (-1, 0), (1, 2), (0, 1), (2, -1))):  # exactly on nodes
            ll2[5 + 7 * k, 3 + 5 * k], mm2[5 + 7 * k, 3 + 5 * k] = l_in[i], m_in[j]
        out.update({f"rg_{name}_beam": beam, f"rg_{name}_l_in": l_in, f"rg_{name}_m_in": m_in, f"rg_{name}_l_out": l_out,
                    f"rg_{name}_m_out": m_out, f"rg_{name}_ll": ll2, f"rg_{name}_mm": mm2})
        b64 = beam.astype(np.float64)
        out[f"rg_{name}_sep"] = np.array([eval_beam(b, l_in, m_in, l_out, m_out) for b in b64])
        out[f"rg_{name}_2d"] = np.array([eval_beam(b, l_in, m_in, ll2, mm2) for b in b64])
        # the statements of the issue, on scipy itself
        assert eval_beam(b64[0], l_in, m_in, l_in[-1:], m_in[-1:])[0, 0] == b64[0, -1, -1]
        assert eval_beam(b64[0], l_in, m_in, l_in[-1:] + 1e-7, m_in[-1:])[0, 0] == 1.0

    # grid_partition: image coordinates in degrees as operators/gridder.py forms them
    nx, ny, cell_rad = 64, 48, np.deg2rad(0.07)
    l_beam, m_beam = grids["g33x29"]
    gp_beam = smooth_beam(rng, 33, 29)
    gp_beam[1] = 1.0
    x = np.rad2deg((-nx / 2 + np.arange(nx)) * cell_rad)
    y = np.rad2deg((-ny / 2 + np.arange(ny)) * cell_rad)
    xx, yy = np.meshgrid(x, y, indexing="ij")
    out.update(gp_beam=gp_beam, gp_l_beam=l_beam, gp_m_beam=m_beam, gp_cell_rad=cell_rad, gp_nx=nx, gp_ny=ny)
    out["gp_out"] = np.array([eval_beam(b, l_beam, m_beam, xx, yy) for b in gp_beam.astype(np.float64)])
    assert (out["gp_out"][1] == 1.0).all() and (out["gp_out"][0] != 1.0).any() and (out["gp_out"][0, 0] == 1.0).all()

    cites.append("src/pfb_imaging/utils/stokes2vis_msv4.py:405-409 rotation mean (scipy.ndimage.rotate)")
    for n0, n1 in ROT_SHAPES:
        u, v = np.meshgrid(np.linspace(-1, 1, n0), np.linspace(-1, 1, n1), indexing="ij")
        beam0 = 1.3 * np.exp(-(u**2 / 0.35 + (v - 0.1) ** 2 / 0.6 + 0.4 * u * v)) + 0.01 * rng.standard_normal((n0, n1))
        beam0 = f32(beam0)
        out[f"rot_{n0}x{n1}_beam0"] = beam0
        b64 = beam0.astype(np.float64)
        for key, angles in ROT_ANGLES.items():
            acc = np.zeros((n0, n1))
            for angle in angles:
                acc += ndimage.rotate(b64, angle, reshape=False, mode="nearest")
            acc /= angles.size
            out[f"rot_{n0}x{n1}_{key}"] = acc
    for key, angles in ROT_ANGLES.items():
        out[f"rot_angles_{key}"] = angles

    out["cites"] = np.array(cites)
    path = os.path.join(HERE, "beam_pins.npz")
    np.savez_compressed(path, **out)
    print("\n".join(cites))
    print("beam_pins.npz", os.path.getsize(path))


if __name__ == "__main__":
    from make_ref_pins import REF

    if not os.path.isdir(REF):
        sys.exit("make_beam_pins.py needs the reference checkout (build container only); the committed .npz travels instead")
    main()
