"""numpy restatements for the direct-DFT tests: the predict sum and its adjoint with every option the device has, and the
transient injection step of the reference.

``predict`` / ``image`` restate ``vis = sum_pix dirty * exp(-2 pi i f/c (u l + v m - w (n - 1))) [/ n]`` of the reference
(tests/test_hessian_approx.py:44-67) -- the definition oracle/dft.py implements -- extended by the row / channel factors, the
per-row offset and the free exponent sign of src/pfb_imaging/utils/stokes2im.py:518-558.  The phase is formed in long double
and reduced to a fraction of a turn before it meets pi, so these carry no error worth counting against the device's bound.
``inject`` restates stokes2im.py:501-558 literally in float64 (``n0t - 1`` by subtraction and all).
"""

import numpy as np

C0 = 299792458.0
EPS = 2.0**-52


def nm1_of(l, m):
    """oracle/pfb_oracle.c ``nm1_of`` in float64"""
    r2 = l * l + m * m
    safe = np.where(r2 <= 1.0, r2, 0.0)
    return np.where(r2 <= 1.0, -safe / (1.0 + np.sqrt(1.0 - safe)), -np.sqrt(np.maximum(r2 - 1.0, 0.0)) - 1.0)


def phases(uvw, freq, lm, off=None, signs=(1.0, 1.0, 1.0), do_wgridding=True):
    """``(frac, turns, nm1)``: the phase of every (row, channel, source) in turns as a float64 fraction in [-1/2, 1/2] and as
    it stands (long double)"""
    ld = np.longdouble
    l, m = lm[:, 0], lm[:, 1]
    nm1 = nm1_of(l, m) if do_wgridding else np.zeros_like(l)
    u, v, w = (signs[0] * uvw[:, 0]).astype(ld), (signs[1] * uvw[:, 1]).astype(ld), (signs[2] * uvw[:, 2]).astype(ld)
    delay = u[:, None] * l.astype(ld)[None, :] + v[:, None] * m.astype(ld)[None, :] - w[:, None] * nm1.astype(ld)[None, :]
    if off is not None:
        delay = delay + np.asarray(off, dtype=np.float64).reshape(-1).astype(ld)[:, None]
    turns = (freq / C0).astype(ld)[None, :, None] * delay[:, None, :]
    return (turns - np.rint(turns)).astype(np.float64), turns, nm1


def predict(uvw, freq, lm, amp, mask=None, rowf=None, chanf=None, off=None, wgt=None, signs=(1.0, 1.0, 1.0), sgn=-1.0,
            do_wgridding=True, divide_by_n=True):
    """``(vis, bound)``: the visibilities (masked samples 0) and, per sample, the issue's bound
    ``4 . 2 pi . 2^-52 . T_max . |wgt| . sum_s |amp rowf chanf| / N_s`` with ``T_max`` the largest phase of the case in turns."""
    frac, turns, nm1 = phases(uvw, freq, lm, off, signs, do_wgridding)
    a = (amp / (nm1 + 1.0) if divide_by_n else amp)[None, None, :] * np.ones(frac.shape)
    if rowf is not None:
        a = a * rowf.T[:, None, :]
    if chanf is not None:
        a = a * chanf.T[None, :, :]
    vis = (a * np.exp(sgn * 2j * np.pi * frac)).sum(axis=-1)
    size = np.abs(a).sum(axis=-1)
    if wgt is not None:
        vis, size = vis * wgt, size * np.abs(wgt)
    if mask is not None:
        vis = np.where(mask != 0, vis, 0.0)
    tmax = float(np.abs(turns).max()) if turns.size else 0.0
    return vis, 4 * 2 * np.pi * EPS * tmax * size


def image(uvw, freq, lm, vis, mask=None, wgt=None, off=None, signs=(1.0, 1.0, 1.0), sgn=-1.0, do_wgridding=True, divide_by_n=True):
    """``(out, bound)``: ``out[s] = sum_{r, c} mask wgt Re(vis exp(-sgn 2 pi i t)) / N_s`` and the bound
    ``4 . 2 pi . 2^-52 . T_max . sum |wgt vis| / N_s``"""
    frac, turns, nm1 = phases(uvw, freq, lm, off, signs, do_wgridding)
    v = vis if wgt is None else vis * wgt
    if mask is not None:
        v = np.where(mask != 0, v, 0.0)
    out = (v[:, :, None] * np.exp(-sgn * 2j * np.pi * frac)).real.sum(axis=(0, 1))
    N = nm1 + 1.0 if divide_by_n else np.ones_like(nm1)
    tmax = float(np.abs(turns).max()) if turns.size else 0.0
    return out / N, 4 * 2 * np.pi * EPS * tmax * np.abs(v).sum() / np.abs(N)


def inject(data, uvw, freq, time, sources, all_times, all_freqs, w_diff=None, beam=None):
    """stokes2im.py:501-558 on arrays, per source independently (``w_diff`` is not carried from source to source); returns
    ``(data, bound)`` where ``bound`` (nrow, nchan) is what a phase-exact evaluation may differ from this one by: the
    float64 roundings of the phase here, 2 pi 2^-52 per turn of each of its four terms and of their sum, plus the
    cancellation of ``n0t - 1`` -- one ulp of 1 on ``n0t``, times ``w f / c`` turns."""
    data = data.copy()
    nrow = uvw.shape[0]
    freqfactor = -2j * np.pi * freq[None, :] / C0                                   # :354
    bound = np.zeros((nrow, freq.size))
    for k, src in enumerate(sources):
        x0t, y0t = src["l"], src["m"]
        n0t = np.sqrt(1 - x0t**2 - y0t**2)                                         # :512
        tprofile = np.interp(time, all_times, src["time_profile"])                  # :518
        fprofile = np.interp(freq, all_freqs, src["freq_profile"])                  # :519
        dspec = (tprofile[:, None]) * fprofile[None, :]                             # :523
        if beam is not None:
            dspec = dspec * beam[k][None, :]                                        # :540
        phase = np.zeros((nrow, 1)) if w_diff is None else np.array(w_diff, dtype=np.float64).reshape(nrow, 1)  # :548-551
        terms = np.abs(phase)
        phase += uvw[:, 0:1] * x0t                                                  # :552 (signu * signx == 1)
        phase += uvw[:, 1:2] * y0t                                                  # :553
        phase -= uvw[:, 2:] * (n0t - 1)                                             # :554
        terms = terms + np.abs(uvw[:, 0:1] * x0t) + np.abs(uvw[:, 1:2] * y0t) + np.abs(uvw[:, 2:] * (n0t - 1))
        data[:, :, 0] += dspec * np.exp(freqfactor * phase)                         # :555-558
        turns = (4 * terms + np.abs(uvw[:, 2:])) * freq[None, :] / C0
        bound += 2 * np.pi * EPS * turns * np.abs(dspec)
    return data, bound


def case(nrow=37, nchan=5, nsrc=7, seed=0, field=0.05, special=True):
    """A small problem: baselines of a few hundred metres (w a fifth of that), unevenly spaced channels around 1.2 GHz and
    sources within ``field`` of the centre.  With ``special`` (and room for them) source 0 sits at l = m = 0 exactly and
    source 1 at l^2 + m^2 = 0.9."""
    rng = np.random.default_rng(1000 + seed)
    uvw = rng.normal(0.0, 300.0, (nrow, 3))
    uvw[:, 2] *= 0.2
    freq = np.sort(1.0e9 + 4.0e8 * rng.uniform(0.0, 1.0, nchan) ** 2)
    lm = rng.uniform(-field, field, (nsrc, 2))
    if special and nsrc >= 3:
        lm[0] = 0.0
        lm[1] = np.sqrt(0.9) * np.array([np.cos(0.7), np.sin(0.7)])
    amp = rng.uniform(0.2, 1.0, nsrc) * rng.choice([-1.0, 1.0], nsrc)
    return dict(uvw=uvw, freq=freq, lm=lm, amp=amp,
                wgt=rng.uniform(0.1, 1.0, (nrow, nchan)),
                rowf=rng.uniform(0.0, 1.0, (nsrc, nrow)), chanf=rng.uniform(0.5, 1.0, (nsrc, nchan)),
                off=rng.normal(0.0, 5.0, nrow),
                vis=rng.normal(size=(nrow, nchan)) + 1j * rng.normal(size=(nrow, nchan)))


def transient_cases():
    """``{tag: (times, freqs, transient_params)}`` of tests/golden/transient_pins.npz: every pulse shape, alone and repeated"""
    times = 4.0e9 + np.cumsum(np.random.default_rng(77).uniform(1.0, 9.0, 61))     # seconds, unevenly sampled
    freqs = np.linspace(0.9e9, 1.7e9, 13) ** 1.0
    out = {}
    for shape, duration in (("gaussian", 11.5), ("exponential", 23.0), ("step", 40.0)):
        base = dict(time=dict(peak_time=37.25, duration=duration, shape=shape),
                    frequency=dict(peak_flux=2.5, reference_freq=1.2e9, spectral_index=-0.7))
        out[shape] = (times, freqs, base)
        out[shape + "_periodic"] = (times, freqs, dict(base, periodicity=dict(enabled=True, period=60.5, total_duration=230.0)))
        out[shape + "_periodic_default"] = (times, freqs, dict(base, periodicity=dict(enabled=True, period=83.0)))
    return out
