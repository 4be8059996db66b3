"""Reader of tests/golden/numba_pins.npz (made by tests/golden/make_numba_pins.py: the reference's numba kernels, run as plain
Python).  Shared by test_numba_pins_cpu.py and test_gpu_numba_pins.py; loads once per directory and hands out read-only arrays."""

import functools
import os

import numpy as np

# the cases the generator writes (asserted against the file's own list in load())
PSI_TAGS = ("db1_1_2_2", "db2_2_12_20", "db3_1_12_10", "db4_1_14_16", "db5_1_20_18", "db6_1_22_24", "db7_1_28_26", "db8_2_60_62",
            "db1_5_32_96", "db1_1_2_514", "db1_1_514_2", "db2_1_6_1030", "db2_3_36_52", "db1_3_34_18", "db1_3_18_34",
            "db8_1_30_32", "db1_1_30_32", "db3_1_30_32")
WGT_TAGS = ("wgt_1_16_16_1_-1", "wgt_2_23_18_-1_1", "wgt_4_23_18_1_-1", "wgt_1_16_16_-1_1")
ROBUST = (-3, 0.0, 2.0)
DUAL_NBAND = (1, 3, 17)
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def load(golden_dir):
    with np.load(os.path.join(golden_dir, "numba_pins.npz")) as z:
        p = {k: z[k] for k in z.files}
    for a in p.values():
        a.setflags(write=False)
    assert tuple(p["psi_cases"]) == PSI_TAGS and tuple(p["wgt_cases"]) == WGT_TAGS
    return p


def psi_case(p, tag):
    """One wavelet case: image x, packed coefficients c (hdot's input), the pins alpha = dwt(x) and img = idwt(c), the
    bookkeeping of the reference and the float64 reference's own distance from the longdouble run."""
    name, nlevel, nx, ny = tag.split("_")
    i = PSI_TAGS.index(tag)
    bk = p[tag + "_bk"]
    x_den, c_den = p["psi_den"]
    fl = p["psi_floor"][i]
    return dict(name=name, nlevel=int(nlevel), nx=int(nx), ny=int(ny), x=p[tag + "_x_num"] / x_den, c=p[tag + "_c_num"] / c_den,
                alpha=p[tag + "_alpha"], img=p[tag + "_img"], ix=bk[:, 0:2], iy=bk[:, 2:4], sx=bk[:, 4], sy=bk[:, 5], spx=bk[:, 6],
                spy=bk[:, 7], ntotx=int(p["psi_tot"][i, 0]), ntoty=int(p["psi_tot"][i, 1]), nxmax=int(p["psi_tot"][i, 2]),
                nymax=int(p["psi_tot"][i, 3]), alpha_floor=(fl[0], fl[1]), img_floor=(fl[2], fl[3]))


def wgt_case(p, tag):
    _, ncorr, nx, ny, us, vs = tag.split("_")
    w_den, i_den, cell = p["wgt_den"]
    return dict(ncorr=int(ncorr), nx=int(nx), ny=int(ny), usign=float(us), vsign=float(vs), cell_size=float(cell),
                uvw=p[tag + "_uvw"], freq=p[tag + "_freq"], mask=p[tag + "_mask"], wgt=p[tag + "_w_num"] / w_den,
                imw_in=p[tag + "_i_num"] / i_den, counts=p[tag + "_counts"], cell=p[tag + "_cell"].astype(np.int64),
                imw={rb: p[f"{tag}_imw_{rb}"] for rb in ROBUST})


def dual_case(p, nband):
    lam, sigma, v_den, w_den = p["dual_par"]
    tag = f"dual_{nband}"
    return dict(lam=float(lam), sigma=float(sigma), vp=p[tag + "_vp_num"] / v_den, v=p[tag + "_v_num"] / v_den,
                w=p[tag + "_w_num"] / w_den, eq=p[tag + "_eq"], out=p[tag + "_out"])


def dist(a, ref):
    """(max abs, relative l2) of a - ref"""
    d = np.asarray(a, dtype=np.float64) - ref
    return float(np.abs(d).max()), float(np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-300))


def touched(c):
    """Visibilities counts_to_weights may change: in range and unmasked (the pinned cell index is -1 elsewhere)."""
    return c["cell"] >= 0


def margins(c):
    """The cells of the packed (ntotx, ntoty) layout that no level writes (pinned bookkeeping): exact zeros in the reference.
    Inside the blocks a zero is a value, and an exact cancellation there may round differently in another summation order."""
    m = np.ones((c["ntotx"], c["ntoty"]), dtype=bool)
    for k in range(c["nlevel"]):
        hx, hy = int(c["ix"][k, 1]), int(c["iy"][k, 1])
        m[hx - 2 * int(c["sx"][k]):hx, hy - 2 * int(c["sy"][k]):hy] = False
    return m
