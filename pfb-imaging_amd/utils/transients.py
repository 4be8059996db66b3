"""Synthetic transients: their dynamic spectra and their injection into visibilities.

Mirrors ``src/pfb_imaging/utils/transients.py`` of the reference (the three profile functions, same signatures and the same
numpy expressions) and the array core of the injection step of ``utils/stokes2im.py:491-558``: per source the two profiles
are interpolated onto the rows' times and the channels' frequencies, optionally scaled by a per-channel beam, and
``tprofile[:, None] * fprofile[None, :] * exp(freqfactor * phase)`` is added into the Stokes-I data.  The profiles are
vectors and stay on the host; the outer product and the phase are one direct-DFT predict on the device
(:class:`pfb_imaging_amd.dft.DFT`), which never forms ``dspec`` in host memory.
"""

import numpy as np


def generate_time_profile(times, peak_time, duration, shape):
    """Time profile of a single pulse (transients.py:4-22): ``gaussian`` (``duration`` is sigma), ``exponential`` (decay
    time, zero before the peak) or ``step`` (on for ``duration`` from the peak)."""
    if shape == "gaussian":
        return np.exp(-((times - peak_time) ** 2) / (2 * duration**2))
    if shape == "exponential":
        return np.where(times >= peak_time, np.exp(-(times - peak_time) / duration), 0.0)
    if shape == "step":
        return np.where((times >= peak_time) & (times <= peak_time + duration), 1.0, 0.0)
    raise ValueError(f"Unknown time profile shape: {shape}")


def generate_frequency_profile(freqs, peak_flux, reference_freq, spectral_index):
    """Power-law spectrum (transients.py:25-27)."""
    return peak_flux * (freqs / reference_freq) ** spectral_index


def generate_transient_spectra(times, freqs, transient_params):
    """``(time_profile, freq_profile)`` of one transient (transients.py:30-86).  ``transient_params`` holds ``time``
    (``peak_time, duration, shape``), ``frequency`` (``peak_flux, reference_freq, spectral_index``) and optionally
    ``periodicity`` (``enabled, period, total_duration``).  ``peak_time`` counts from the first time; with periodicity the
    pulse repeats every ``period`` for as long as its peak lies within ``total_duration``."""
    tp, fp = transient_params["time"], transient_params["frequency"]
    periodicity = transient_params.get("periodicity", {"enabled": False})
    times = times - times[0]
    if periodicity.get("enabled", False):
        period = periodicity["period"]
        total = periodicity.get("total_duration", times[-1] - times[0])
        profile = np.zeros_like(times)
        for n in range(int((total - tp["peak_time"]) / period) + 1):
            if tp["peak_time"] + n * period <= total:
                profile += generate_time_profile(times, tp["peak_time"] + n * period, tp["duration"], tp["shape"])
    else:
        profile = generate_time_profile(times, tp["peak_time"], tp["duration"], tp["shape"])
    return profile, generate_frequency_profile(freqs, fp["peak_flux"], fp["reference_freq"], fp["spectral_index"])


def accumulate_sources(dft, out, time, freq, sources, all_times, all_freqs, w_diff=None, beam=None):
    """The per-source loop of stokes2im.py:501-558 on the device: each source's profiles are interpolated onto ``time`` / ``freq``,
    scaled by its row of ``beam``, and ``tprofile[:, None] * fprofile[None, :] * exp(freqfactor * phase)`` is added into ``out``
    (complex128 ``(nrow, nchan)``, a host array or a ``DeviceArray``) by one accumulating predict of ``dft`` (a
    :class:`~pfb_imaging_amd.dft.DFT` over the coordinates the sources are simulated at).  Shared by :func:`inject_transients`
    and ``VisChunk.inject_transients``; the arguments have been checked by the caller."""
    for k, src in enumerate(sources):
        tprofile = np.interp(time, all_times, src["time_profile"])
        fprofile = np.interp(freq, all_freqs, src["freq_profile"])
        if beam is not None:
            fprofile = fprofile * beam[k]
        dft.predict(np.array([[src["l"], src["m"]]]), np.ones(1), rowf=tprofile[None, :], chanf=fprofile[None, :], off=w_diff,
                    signs=(1.0, 1.0, 1.0), sgn=-1.0, do_wgridding=True, divide_by_n=False, accumulate=True, out=out)


def inject_transients(data, uvw, freq, time, sources, all_times, all_freqs, w_diff=None, beam=None):
    """Add point transients to ``data[:, :, 0]`` in place and return ``data`` (stokes2im.py:491-558, arrays only).

    ``data`` is ``(nrow, nchan, ncorr)`` complex, ``uvw (nrow, 3)`` the coordinates the sources are simulated at, ``time
    (nrow)`` the rows' times.  Each of ``sources`` is a dict with ``l`` and ``m`` (the direction cosines ``x0t, y0t`` towards
    the source, :509-511) and ``time_profile`` / ``freq_profile`` sampled on ``all_times`` / ``all_freqs`` (:515-519).
    ``w_diff (nrow)`` or ``(nrow, 1)`` [m] is the rephasing term of :548-549; ``beam (nsource, nchan)`` a per-channel power
    beam towards each source (:528-540).  Signs are the reference's: ``signu * signx == signv * signy == 1`` whatever the
    flips (:552-553), ``- w (n - 1)`` (:554) and ``freqfactor = -2 pi i f / c`` (:354).

    One difference: the reference adds each source's phase into ``w_diff`` itself (:549-554, ``phase = w_diff`` followed by
    ``+=``), so every source after the first inherits its predecessors' delays; here each source sees ``w_diff`` as given.
    """
    from .. import _lib
    from ..dft import DFT

    uvw, freq = np.asarray(uvw, dtype=np.float64), np.asarray(freq, dtype=np.float64)
    time = np.asarray(time, dtype=np.float64)
    if data.ndim != 3 or data.shape[:2] != (uvw.shape[0], freq.size) or not np.iscomplexobj(data):
        raise ValueError(f"data {data.shape} {data.dtype} must be complex (nrow, nchan, ncorr) = ({uvw.shape[0]}, {freq.size}, ...)")
    if time.shape != (uvw.shape[0],):
        raise ValueError(f"time {time.shape} != {(uvw.shape[0],)}")
    if beam is not None:
        beam = np.asarray(beam, dtype=np.float64)
        if beam.shape != (len(sources), freq.size):
            raise ValueError(f"beam {beam.shape} != {(len(sources), freq.size)}")
    if not len(sources):
        return data
    with DFT(uvw, freq) as d:
        acc = _lib.DeviceArray.from_host(np.ascontiguousarray(data[:, :, 0], dtype=np.complex128))
        try:
            accumulate_sources(d, acc, time, freq, sources, all_times, all_freqs, w_diff, beam)
            data[:, :, 0] = acc.download()
        finally:
            acc.free()
    return data
