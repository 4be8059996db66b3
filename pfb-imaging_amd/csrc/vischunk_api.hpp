// vischunk_api.hpp -- the two-stage partial-sum machinery of vischunk.hip, for the other files that reduce over a resident
// chunk or over image planes (snapshot.hip): the launch shape, the block tree, and host-callable launchers of the kernels
// that stay defined in vischunk.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pfbhip {

constexpr int CHUNK_THREADS = 256;
constexpr int CHUNK_MAX_BLOCKS = 1024;  // first-stage blocks per correlation: one sweep covers 262 144 samples

// first-stage blocks over nvis samples (at least one)
int chunk_first_stage_blocks(int64_t nvis);

// part[c * nb + b] = block b's share of sum_{mask > 0} wgtp |r|^2 of correlation c (wgtp_dev NULL: the scalar), cnt[b] its
// share of sum(mask): grid (nb, ncorr)
void chunk_ressq_partial(hipStream_t st, const double2 *r, const double *wgtp_dev, double wgtp_scalar, const uint8_t *mask_dev,
                         int64_t ncorr, int64_t nvis, int nb, double *part, unsigned long long *cnt);
// out[c] = sum of part[c * nb, (c + 1) * nb) for c < nout, one block each; cnt_out = sum of cnt[0, ncnt) (cnt may be NULL)
void chunk_partial_final(hipStream_t st, const double *part, const unsigned long long *cnt, int nb, int ncnt, int nout, double *out,
                         unsigned long long *cnt_out);

#if defined(__HIPCC__)
// sum of s[0, CHUNK_THREADS) into s[0] (every thread of a CHUNK_THREADS-wide block calls it)
template <class T>
__device__ __forceinline__ void block_tree_sum(T *s)
{
    __syncthreads();
    for (int h = CHUNK_THREADS / 2; h > 0; h >>= 1) {
        if (int(threadIdx.x) < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
}
#endif

}  // namespace pfbhip
