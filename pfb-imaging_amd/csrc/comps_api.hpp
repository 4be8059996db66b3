// comps_api.hpp -- the component-model handle, shared by comps.hip (which owns it) and dft.hip (which reads it).
#pragma once
#include "common.hpp"

struct pfbhip_comps {
    int64_t nx = 0, ny = 0, ncomps = 0;
    int nparam = 0;
    bool has_region = false;
    pfbhip::DevBuf<int64_t> xi, yi, pix;
    pfbhip::DevBuf<double> coeffs, basis, image;  // (nparam, ncomps); the basis vector of the last render; scratch of the host render
    pfbhip::DevBuf<uint8_t> region;
    hipStream_t stream() const { return hipStreamPerThread; }
};
