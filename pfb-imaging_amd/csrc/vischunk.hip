// vischunk.hip -- reductions and the l2 reweighting of a device-resident visibility chunk on MI355X.
//
// Replaces, for a chunk that stays in HBM (vischunk.py), the numpy passes of the reference's
// src/pfb_imaging/operators/gridder.py:584 (WSUM) and :509-532 (l2 reweighting), which the array path
// (operators/gridder.py::image_data_products_arrays) runs on the host over (ncorr, nrow, nchan).
// The imaging weights of a resident chunk are pfbhip_imaging_weights_dev in weighting.hip, next to the body they share with
// pfbhip_imaging_weights.
//
// Every sum is two-stage: each block of the first stage sums a grid-stride slice of one correlation and reduces it in LDS
// along a fixed tree, one block per correlation then sums the partials the same way.  No atomics: the order of every
// addition depends on the sizes alone, so a result is bit-identical from call to call.
#include <hip/hip_runtime.h>

#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"
#include "vischunk_api.hpp"

namespace pfbhip {

// part[c * gridDim.x + b] = sum over block b's samples of correlation c = blockIdx.y of wgt[c, i] where mask[i] != 0
__global__ void __launch_bounds__(CHUNK_THREADS) k_wsum_partial(const double *__restrict__ wgt, const uint8_t *__restrict__ mask,
                                                                int64_t nvis, double *__restrict__ part)
{
    __shared__ double s[CHUNK_THREADS];
    const int c = blockIdx.y;
    double t = 0.0;
    for (int64_t i = blockIdx.x * int64_t(CHUNK_THREADS) + threadIdx.x; i < nvis; i += int64_t(gridDim.x) * CHUNK_THREADS)
        if (mask[i]) t += wgt[size_t(c) * size_t(nvis) + size_t(i)];
    s[threadIdx.x] = t;
    block_tree_sum(s);
    if (threadIdx.x == 0) part[size_t(c) * gridDim.x + blockIdx.x] = s[0];
}

// part[c * gridDim.x + b] = the block's share of sum_{mask > 0} wgtp |r|^2 of correlation c; cnt[b] (c == 0 only) its share
// of sum(mask), the mask's VALUES as numpy's mask.sum() adds them.  ressq as numpy forms (r * wgtp * conj(r)).real.
__global__ void __launch_bounds__(CHUNK_THREADS) k_ressq_partial(const double2 *__restrict__ r, const double *__restrict__ wgtp,
                                                                 double wgtp_scalar, const uint8_t *__restrict__ mask, int64_t nvis,
                                                                 double *__restrict__ part, unsigned long long *__restrict__ cnt)
{
    __shared__ double s[CHUNK_THREADS];
    __shared__ unsigned long long sc[CHUNK_THREADS];
    const int c = blockIdx.y;
    double t = 0.0;
    unsigned long long n = 0;
    for (int64_t i = blockIdx.x * int64_t(CHUNK_THREADS) + threadIdx.x; i < nvis; i += int64_t(gridDim.x) * CHUNK_THREADS) {
        const uint8_t mk = mask[i];
        if (!mk) continue;
        const size_t k = size_t(c) * size_t(nvis) + size_t(i);
        const double2 v = r[k];
        const double wp = wgtp ? wgtp[k] : wgtp_scalar;
        t += (v.x * wp) * v.x + (v.y * wp) * v.y;
        n += mk;
    }
    s[threadIdx.x] = t;
    block_tree_sum(s);
    if (threadIdx.x == 0) part[size_t(c) * gridDim.x + blockIdx.x] = s[0];
    if (c == 0) {
        sc[threadIdx.x] = n;
        block_tree_sum(sc);
        if (threadIdx.x == 0) cnt[blockIdx.x] = sc[0];
    }
}

// out[c] = sum of part[c * nb, (c + 1) * nb): one block per correlation; cnt_out = sum of cnt[0, ncnt) by block 0 (cnt may be NULL)
__global__ void __launch_bounds__(CHUNK_THREADS) k_partial_final(const double *__restrict__ part, const unsigned long long *__restrict__ cnt,
                                                                 int nb, int ncnt, double *__restrict__ out,
                                                                 unsigned long long *__restrict__ cnt_out)
{
    __shared__ double s[CHUNK_THREADS];
    __shared__ unsigned long long sc[CHUNK_THREADS];
    const int c = blockIdx.x;
    double t = 0.0;
    for (int b = threadIdx.x; b < nb; b += CHUNK_THREADS) t += part[size_t(c) * nb + b];
    s[threadIdx.x] = t;
    block_tree_sum(s);
    if (threadIdx.x == 0) out[c] = s[0];
    if (c == 0 && cnt) {
        unsigned long long n = 0;
        for (int b = threadIdx.x; b < ncnt; b += CHUNK_THREADS) n += cnt[b];
        sc[threadIdx.x] = n;
        block_tree_sum(sc);
        if (threadIdx.x == 0) *cnt_out = sc[0];
    }
}

// wgt[c, i] *= (dof + 2) / (dof + ressq / ovar[c]) on every sample, masked ones included (gridder.py:527-530)
__global__ void __launch_bounds__(CHUNK_THREADS) k_l2_reweight(const double2 *__restrict__ r, const double *__restrict__ wgtp,
                                                               double wgtp_scalar, const double *__restrict__ ovar, double dof,
                                                               int64_t nvis, double *__restrict__ wgt)
{
    const int c = blockIdx.y;
    const int64_t i = blockIdx.x * int64_t(CHUNK_THREADS) + threadIdx.x;
    if (i >= nvis) return;
    const size_t k = size_t(c) * size_t(nvis) + size_t(i);
    const double2 v = r[k];
    const double wp = wgtp ? wgtp[k] : wgtp_scalar;
    const double ressq = (v.x * wp) * v.x + (v.y * wp) * v.y;
    wgt[k] *= (dof + 2.0) / (dof + ressq / ovar[c]);
}

int chunk_first_stage_blocks(int64_t nvis) { return int(std::min<int64_t>(std::max<int64_t>(ceil_div(nvis, CHUNK_THREADS), 1), CHUNK_MAX_BLOCKS)); }

void chunk_ressq_partial(hipStream_t st, const double2 *r, const double *wgtp_dev, double wgtp_scalar, const uint8_t *mask_dev,
                         int64_t ncorr, int64_t nvis, int nb, double *part, unsigned long long *cnt)
{
    hipLaunchKernelGGL(k_ressq_partial, dim3(uint32_t(nb), uint32_t(ncorr)), dim3(CHUNK_THREADS), 0, st, r, wgtp_dev, wgtp_scalar, mask_dev,
                       nvis, part, cnt);
}

void chunk_partial_final(hipStream_t st, const double *part, const unsigned long long *cnt, int nb, int ncnt, int nout, double *out,
                         unsigned long long *cnt_out)
{
    hipLaunchKernelGGL(k_partial_final, dim3(uint32_t(nout)), dim3(CHUNK_THREADS), 0, st, part, cnt, nb, ncnt, out, cnt_out);
}

}  // namespace pfbhip

using namespace pfbhip;

extern "C" {

int pfbhip_chunk_wsum_dev(const double *wgt_dev, const uint8_t *mask_dev, int64_t ncorr, int64_t nvis, double *wsum_host)
{
    return guarded([&] {
        PFB_REQUIRE(wsum_host && ncorr >= 1 && ncorr <= 65535 && nvis >= 0, "bad arguments");
        PFB_REQUIRE((wgt_dev && mask_dev) || nvis == 0, "NULL argument");
        const hipStream_t st = hipStreamPerThread;
        const int nb = chunk_first_stage_blocks(nvis);
        DevBuf<double> part(size_t(ncorr) * size_t(nb)), out{size_t(ncorr)};
        synced(st, [&] {  // (wsum_host is written until the wait; part and out are declared outside)
            hipLaunchKernelGGL(k_wsum_partial, dim3(uint32_t(nb), uint32_t(ncorr)), dim3(CHUNK_THREADS), 0, st, wgt_dev, mask_dev, nvis,
                               part.p);
            chunk_partial_final(st, part.p, nullptr, nb, 0, int(ncorr), out.p, nullptr);
            PFB_HIP(hipGetLastError());
            PFB_HIP(hipMemcpyAsync(wsum_host, out.p, size_t(ncorr) * sizeof(double), hipMemcpyDeviceToHost, st));
        });
    });
}

int pfbhip_chunk_l2_reweight_dev(const double *resvis_dev, const double *wgtp_dev, double wgtp_scalar, const uint8_t *mask_dev,
                                 double *wgt_dev, int64_t ncorr, int64_t nvis, double dof, double *ovar_host)
{
    return guarded([&] {
        PFB_REQUIRE(ncorr >= 1 && ncorr <= 65535 && nvis >= 0, "bad arguments");
        PFB_REQUIRE((resvis_dev && mask_dev && wgt_dev) || nvis == 0, "NULL argument");
        const hipStream_t st = hipStreamPerThread;
        const int nb = chunk_first_stage_blocks(nvis);
        DevBuf<double> part(size_t(ncorr) * size_t(nb)), ssq{size_t(ncorr)};
        DevBuf<unsigned long long> cnt(size_t(nb) + 1);
        std::vector<double> ovar(static_cast<size_t>(ncorr), 0.0);
        unsigned long long nmask = 0;
        const double2 *r = reinterpret_cast<const double2 *>(resvis_dev);
        synced(st, [&] {
            chunk_ressq_partial(st, r, wgtp_dev, wgtp_scalar, mask_dev, ncorr, nvis, nb, part.p, cnt.p);
            chunk_partial_final(st, part.p, cnt.p, nb, nb, int(ncorr), ssq.p, cnt.p + nb);
            PFB_HIP(hipGetLastError());
            PFB_HIP(hipMemcpyAsync(ovar.data(), ssq.p, size_t(ncorr) * sizeof(double), hipMemcpyDeviceToHost, st));
            PFB_HIP(hipMemcpyAsync(&nmask, cnt.p + nb, sizeof nmask, hipMemcpyDeviceToHost, st));
            PFB_HIP(hipStreamSynchronize(st));  // the sums decide whether anything is written at all
            bool ok = nmask > 0;
            for (auto &v : ovar) {
                v = v / double(nmask);  // (0 / 0 with an empty mask: refused below, like a zero variance)
                ok = ok && v != 0.0;
            }
            if (ovar_host)
                for (int64_t c = 0; c < ncorr; ++c) ovar_host[c] = ovar[size_t(c)];
            PFB_REQUIRE(ok, "l2 reweighting: zero residual variance");
            PFB_HIP(hipMemcpyAsync(ssq.p, ovar.data(), size_t(ncorr) * sizeof(double), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_l2_reweight, dim3(uint32_t(ceil_div(nvis, CHUNK_THREADS)), uint32_t(ncorr)), dim3(CHUNK_THREADS), 0, st, r,
                               wgtp_dev, wgtp_scalar, ssq.p, dof, nvis, wgt_dev);
            PFB_HIP(hipGetLastError());
        });
    });
}

}  // extern "C"
