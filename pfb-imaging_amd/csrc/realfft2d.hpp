// realfft2d.hpp -- rocFFT 2-D r2c / c2r of one (n0, n1) plane, double precision: the transform of every padded size the
// hand-written row-FFT pipeline (psffft.hip) does not take.  Shared by psfconv.hip and restore.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <algorithm>

#include "common.hpp"

namespace pfbhip {

#define PFB_ROCFFT(expr)                                                                              \
    do {                                                                                              \
        rocfft_status _s = (expr);                                                                    \
        if (_s != rocfft_status_success)                                                              \
            throw std::runtime_error(pfbhip::strprintf("%s failed: rocfft status %d (%s:%d)", #expr, \
                                                       int(_s), __FILE__, __LINE__));                 \
    } while (0)

void rocfft_setup_once();

struct RealFFT2D {
    int64_t n0 = 0, n1 = 0;
    rocfft_plan fwd = nullptr, inv = nullptr;
    rocfft_execution_info info = nullptr;
    DevBuf<char> work;
    hipStream_t stream = nullptr;
    void create(int64_t n0_, int64_t n1_, hipStream_t st)
    {
        n0 = n0_;
        n1 = n1_;
        stream = st;
        rocfft_setup_once();
        size_t lengths[2] = {size_t(n1), size_t(n0)};
        rocfft_status rst = rocfft_status_success;
        // (rocFFT allocates inside plan creation: on failure the cache of released blocks gives way, once)
        if (!retry_after_cache_flush([&] {
                if (fwd == nullptr)
                    rst = rocfft_plan_create(&fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                                            rocfft_precision_double, 2, lengths, 1, nullptr);
                if (rst == rocfft_status_success && inv == nullptr)
                    rst = rocfft_plan_create(&inv, rocfft_placement_notinplace, rocfft_transform_type_real_inverse,
                                            rocfft_precision_double, 2, lengths, 1, nullptr);
                return rst == rocfft_status_success;
            }))
            PFB_ROCFFT(rst);
        size_t a = 0, b = 0;
        PFB_ROCFFT(rocfft_plan_get_work_buffer_size(fwd, &a));
        PFB_ROCFFT(rocfft_plan_get_work_buffer_size(inv, &b));
        PFB_ROCFFT(rocfft_execution_info_create(&info));
        if (std::max(a, b)) {
            work.alloc(std::max(a, b));
            PFB_ROCFFT(rocfft_execution_info_set_work_buffer(info, work.p, work.n));
        }
        PFB_ROCFFT(rocfft_execution_info_set_stream(info, st));
    }
    void r2c(double *in, double2 *out)
    {
        void *i[1] = {in}, *o[1] = {out};
        PFB_ROCFFT(rocfft_execute(fwd, i, o, info));
    }
    // destroys `in` (like ducc0's allow_overwriting_input=True, psf.py:31)
    void c2r(double2 *in, double *out)
    {
        void *i[1] = {in}, *o[1] = {out};
        PFB_ROCFFT(rocfft_execute(inv, i, o, info));
    }
    ~RealFFT2D()
    {
        if (fwd) rocfft_plan_destroy(fwd);
        if (inv) rocfft_plan_destroy(inv);
        if (info) rocfft_execution_info_destroy(info);
    }
};

}  // namespace pfbhip
