"""Host-side refusals of the C ABI that come after the call has enqueued copies from or into the caller's arrays.

The psfconv and comps entry points run what they enqueue inside one stream scope (``synced`` of csrc/abi_scope.hpp) that
waits for the stream also when the body throws, so an error status is never returned while a copy is still in flight.
These tests walk error paths that scope owns: the refused call raises ``ValueError`` with the library's message, the
handle stays usable, and a valid call after the refusal returns bit for bit what the same handle returned before it.

They cannot show the early return itself: copies of this size (a 32 x 32 image, a 64 x 64 padded PSF) finish long
before Python looks at the arrays, so the tests would most likely pass without the scope too.  That defect is shown
from the code; what is checked here is that the rewritten paths still refuse, recover and compute the same.

The gridder is not covered: its entry points are not under the scope (csrc/gridder.hip is unchanged).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX = NY = 32
NXP = NYP = 64


@pytest.fixture()
def psfconv():
    from pfb_imaging_amd.psfconv import PsfConv

    rng = np.random.default_rng(11)
    psf = rng.standard_normal((NXP, NYP))
    p = PsfConv(NX, NY, NXP, NYP)
    p.set_psfhat(0, np.abs(np.fft.rfft2(np.fft.ifftshift(psf))) + 1.0)
    p.set_beam(0, 0.5 + rng.random((NX, NY)))  # the taper of direct()
    p.set_beam(1, 0.5 + rng.random((NX, NY)))
    yield p, rng.standard_normal((NX, NY))
    p.close()


def test_psfconv_direct_unbound_beam_slot(psfconv):
    p, x = psfconv
    raw0, raw1, raw2 = (np.full((NX, NY), np.nan) for _ in range(3))
    before = p.direct(x, 0, 0, 1.0, beam_slot=1, min_beam=0.6, raw=raw0).copy()
    with pytest.raises(ValueError, match="beam slot 3 is not bound"):
        p.direct(x, 0, 0, 1.0, beam_slot=3, min_beam=0.6, raw=raw1)  # raw is copied out before the slot is looked at
    after = p.direct(x, 0, 0, 1.0, beam_slot=1, min_beam=0.6, raw=raw2).copy()
    assert np.isfinite(before).all() and np.isfinite(raw0).all()
    assert np.array_equal(after, before) and np.array_equal(raw2, raw0)


def test_psfconv_apply_unbound_psf_slot(psfconv):
    p, x = psfconv
    before = p.apply(x, 0, beam_slot=1, scale=0.5, eta=0.1).copy()
    with pytest.raises(ValueError, match="psfhat slot 5 is not bound"):
        p.apply(x, 5, beam_slot=1, scale=0.5, eta=0.1)
    after = p.apply(x, 0, beam_slot=1, scale=0.5, eta=0.1).copy()
    assert np.isfinite(before).all() and np.abs(before).max() > 0.0
    assert np.array_equal(after, before)


def test_comps_render_region_not_bound():
    from pfb_imaging_amd.comps import Comps

    rng = np.random.default_rng(5)
    pix = rng.choice(NX * NY, size=40, replace=False)
    comps = Comps(NX, NY, pix // NY, pix % NY, rng.standard_normal((3, pix.size)))
    b = np.array([1.0, -0.5, 0.25])
    try:
        before = comps.render(b).copy()
        with pytest.raises(ValueError, match="no region mask bound: call pfbhip_comps_set_region first"):
            comps.render(b, region=True)
        after = comps.render(b).copy()
    finally:
        comps.close()
    assert np.count_nonzero(before) == pix.size
    assert np.array_equal(after, before)
