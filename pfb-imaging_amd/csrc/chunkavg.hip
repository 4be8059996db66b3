// chunkavg.hip -- weighted averaging of a device-resident visibility chunk over channel bins of fixed width and over
// caller-supplied row bins on MI355X: steps 2 to 4 of the reference's src/pfb_imaging/utils/stokes2vis.py:196-286 (drop
// the fully flagged rows, time_and_channel, bda with min_nchan = nchan) as one out-of-place pass over a chunk that stays
// in HBM (vischunk.py::VisChunk.average).  The row MAPPING is the caller's (host metadata); the O(ncorr nrow nchan) data
// work is here.
//
// For output sample (R, q) and correlation c, with K the unmasked input samples (r, k) of row bin R and channel bin q:
//   wgt_out = sum_K wgt,   vis_out = sum_K wgt vis / wgt_out,   mask_out = (K not empty);
// an empty K or a zero wgt_out gives exact zeros (no 0 / 0), and a K of one sample hands that sample's visibility on as
// it is (the weighted mean of one value is that value: chan_bin = 1 with a row map that only drops or reorders rows is
// a pure gather, bit for bit).
//
// No atomics: the order of every addition depends on the shapes and the map alone (members in ascending row order,
// channels in ascending order inside a member; the lane-per-channel kernel then adds across lanes along a fixed xor
// tree), so a result is bit-identical from call to call.
#include <hip/hip_runtime.h>

#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"

namespace pfbhip {

constexpr int AVG_THREADS = 256;

// what one correlation of one output sample has summed
struct AvgAcc {
    double sw = 0.0, sx = 0.0, sy = 0.0;  // sum w, sum w re(v), sum w im(v)
    double vx = -0.0, vy = -0.0;          // sum v: the sample itself, signed zeros included, when exactly one contributes
    __device__ __forceinline__ void add(double w, double2 v)
    {
        sw += w;
        sx += w * v.x;
        sy += w * v.y;
        vx += v.x;
        vy += v.y;
    }
};

// n: the unmasked samples of the bin (the same for every correlation)
__device__ __forceinline__ void avg_store(const AvgAcc &a, int64_t n, double2 *__restrict__ vis_out, double *__restrict__ wgt_out,
                                          size_t o)
{
    double2 v = make_double2(0.0, 0.0);
    double w = 0.0;
    if (n > 0 && a.sw != 0.0) {  // (a NaN weight passes: it propagates, as in numpy)
        w = a.sw;
        v = n == 1 ? make_double2(a.vx, a.vy) : make_double2(a.sx / a.sw, a.sy / a.sw);
    }
    vis_out[o] = v;
    wgt_out[o] = w;
}

// One lane per OUTPUT sample (R, q), all correlations: the lane walks its members' chan_bin contiguous channels.  Any
// chan_bin; IDENT: row bin R is input row R (no CSR).  Masked samples are skipped without reading vis or wgt.
template <bool IDENT>
__global__ void __launch_bounds__(AVG_THREADS)
k_avg_per_output(const double2 *__restrict__ vis, const double *__restrict__ wgt, const uint8_t *__restrict__ mask, int ncorr,
                 int64_t nrow, int64_t nchan, int64_t chan_bin, const int64_t *__restrict__ row_start,
                 const int64_t *__restrict__ members, int64_t nrow_out, int64_t nchan_out, double2 *__restrict__ vis_out,
                 double *__restrict__ wgt_out, uint8_t *__restrict__ mask_out)
{
    const int64_t i = blockIdx.x * int64_t(AVG_THREADS) + threadIdx.x;
    if (i >= nrow_out * nchan_out) return;
    const int64_t R = i / nchan_out, q = i - R * nchan_out;
    const int64_t k0 = q * chan_bin, k1 = min(k0 + chan_bin, nchan);
    const int64_t m0 = IDENT ? R : row_start[R], m1 = IDENT ? R + 1 : row_start[R + 1];
    int64_t n = 0;
    for (int64_t m = m0; m < m1; ++m) {
        const uint8_t *mk = mask + size_t(IDENT ? m : members[m]) * size_t(nchan);
        for (int64_t k = k0; k < k1; ++k) n += mk[k] != 0;
    }
    mask_out[i] = n > 0;
    const size_t plane_in = size_t(nrow) * size_t(nchan), plane_out = size_t(nrow_out) * size_t(nchan_out);
    for (int c = 0; c < ncorr; ++c) {
        AvgAcc a;
        if (n > 0)
            for (int64_t m = m0; m < m1; ++m) {
                const size_t row = size_t(IDENT ? m : members[m]) * size_t(nchan);
                const size_t base = size_t(c) * plane_in + row;
                for (int64_t k = k0; k < k1; ++k)
                    if (mask[row + k]) a.add(wgt[base + k], vis[base + k]);
            }
        avg_store(a, n, vis_out, wgt_out, size_t(c) * plane_out + size_t(i));
    }
}

// One lane per INPUT channel of an output sample, all correlations, for 2 <= chan_bin <= 64: a bin owns `lanes` adjacent
// lanes, chan_bin rounded up to a power of two (the lanes past chan_bin, and past nchan in the last bin, idle), so that
// loads run along the channel axis and a bin never crosses a wave.  The lane sums its channel over the bin's members, the
// bin's lanes add along an xor tree in registers, and the bin's first lane stores.
template <bool IDENT>
__global__ void __launch_bounds__(AVG_THREADS)
k_avg_per_input(const double2 *__restrict__ vis, const double *__restrict__ wgt, const uint8_t *__restrict__ mask, int ncorr,
                int64_t nrow, int64_t nchan, int chan_bin, int lanes, const int64_t *__restrict__ row_start,
                const int64_t *__restrict__ members, int64_t nrow_out, int64_t nchan_out, double2 *__restrict__ vis_out,
                double *__restrict__ wgt_out, uint8_t *__restrict__ mask_out)
{
    const int64_t i = blockIdx.x * int64_t(AVG_THREADS) + threadIdx.x;
    const int64_t o = i / lanes;  // the output sample (R, q), flat
    const int j = int(i - o * lanes);
    const bool bin_ok = o < nrow_out * nchan_out;  // (no early return: every lane of a wave takes part in the shuffles)
    const int64_t R = bin_ok ? o / nchan_out : 0, k = (o - R * nchan_out) * chan_bin + j;
    const bool live = bin_ok && j < chan_bin && k < nchan;
    const int64_t m0 = !live ? 0 : IDENT ? R : row_start[R], m1 = !live ? 0 : IDENT ? R + 1 : row_start[R + 1];
    long long nn = 0;  // the bin's unmasked samples: this lane's channel first, then the bin's lanes together
    for (int64_t m = m0; m < m1; ++m) nn += mask[size_t(IDENT ? m : members[m]) * size_t(nchan) + size_t(k)] != 0;
    const bool any_mine = nn > 0;
    for (int off = 1; off < lanes; off <<= 1) nn += __shfl_xor(nn, off);
    const bool lead = bin_ok && j == 0;
    if (lead) mask_out[o] = nn > 0;
    const size_t plane_in = size_t(nrow) * size_t(nchan), plane_out = size_t(nrow_out) * size_t(nchan_out);
    for (int c = 0; c < ncorr; ++c) {
        AvgAcc a;
        if (any_mine)
            for (int64_t m = m0; m < m1; ++m) {
                const size_t s = size_t(IDENT ? m : members[m]) * size_t(nchan) + size_t(k);
                if (mask[s]) a.add(wgt[size_t(c) * plane_in + s], vis[size_t(c) * plane_in + s]);
            }
        for (int off = 1; off < lanes; off <<= 1) {
            a.sw += __shfl_xor(a.sw, off);
            a.sx += __shfl_xor(a.sx, off);
            a.sy += __shfl_xor(a.sy, off);
            a.vx += __shfl_xor(a.vx, off);
            a.vy += __shfl_xor(a.vy, off);
        }
        if (lead) avg_store(a, nn, vis_out, wgt_out, size_t(c) * plane_out + size_t(o));
    }
}

static bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    const char *pa = static_cast<const char *>(a), *pb = static_cast<const char *>(b);
    return na && nb && pa < pb + nb && pb < pa + na;
}

}  // namespace pfbhip

using namespace pfbhip;

extern "C" {

int pfbhip_chunk_average_dev(const double *vis_dev, const double *wgt_dev, const uint8_t *mask_dev, int64_t ncorr, int64_t nrow,
                             int64_t nchan, int64_t chan_bin, const int64_t *row_start_host, const int64_t *members_host,
                             int64_t nkept, int64_t nrow_out, double *vis_out_dev, double *wgt_out_dev, uint8_t *mask_out_dev)
{
    return guarded([&] {
        PFB_REQUIRE(ncorr >= 1 && ncorr <= 65535, "ncorr = %lld is outside [1, 65535]", (long long)ncorr);
        PFB_REQUIRE(nrow >= 0 && nchan >= 0 && nrow_out >= 0 && nkept >= 0, "negative size");
        PFB_REQUIRE(chan_bin >= 1, "chan_bin = %lld must be at least 1", (long long)chan_bin);
        PFB_REQUIRE(nrow < (int64_t(1) << 40) && nchan < (int64_t(1) << 31) && nrow_out < (int64_t(1) << 40), "sizes too large");
        const bool ident = !row_start_host;
        if (ident) {
            PFB_REQUIRE(!members_host, "members without row_start");
            PFB_REQUIRE(nrow_out == nrow && nkept == nrow, "the identity map needs nrow_out == nkept == nrow");
        } else {
            PFB_REQUIRE(members_host || nkept == 0, "NULL members");
            PFB_REQUIRE(nkept <= nrow, "nkept = %lld exceeds nrow = %lld", (long long)nkept, (long long)nrow);
            PFB_REQUIRE(row_start_host[0] == 0, "row_start[0] must be 0");
            for (int64_t R = 0; R < nrow_out; ++R)
                PFB_REQUIRE(row_start_host[R + 1] >= row_start_host[R] && row_start_host[R + 1] <= nkept,
                            "row_start must be non-decreasing and end at nkept (bin %lld)", (long long)R);
            PFB_REQUIRE(row_start_host[nrow_out] == nkept, "row_start[nrow_out] must be nkept");
            for (int64_t R = 0; R < nrow_out; ++R)
                for (int64_t m = row_start_host[R]; m < row_start_host[R + 1]; ++m) {
                    PFB_REQUIRE(members_host[m] >= 0 && members_host[m] < nrow, "member %lld of bin %lld is outside [0, nrow)",
                                (long long)members_host[m], (long long)R);
                    PFB_REQUIRE(m == row_start_host[R] || members_host[m] > members_host[m - 1],
                                "the members of bin %lld must ascend strictly", (long long)R);
                }
        }
        const int64_t nchan_out = ceil_div(nchan, chan_bin);
        const size_t nin = size_t(nrow) * size_t(nchan), nout = size_t(nrow_out) * size_t(nchan_out);
        PFB_REQUIRE((vis_dev && wgt_dev && mask_dev) || nin == 0, "NULL input");
        PFB_REQUIRE((vis_out_dev && wgt_out_dev && mask_out_dev) || nout == 0, "NULL output");
        const struct {
            const void *p;
            size_t n;
        } in[3] = {{vis_dev, nin * size_t(ncorr) * 16}, {wgt_dev, nin * size_t(ncorr) * 8}, {mask_dev, nin}},
          out[3] = {{vis_out_dev, nout * size_t(ncorr) * 16}, {wgt_out_dev, nout * size_t(ncorr) * 8}, {mask_out_dev, nout}};
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) PFB_REQUIRE(!overlaps(out[a].p, out[a].n, in[b].p, in[b].n), "an output aliases an input");
            for (int b = a + 1; b < 3; ++b) PFB_REQUIRE(!overlaps(out[a].p, out[a].n, out[b].p, out[b].n), "two outputs overlap");
        }
        PFB_REQUIRE(nout <= (size_t(1) << 32), "too many output samples for one launch");  // (x 64 lanes / 256: 2^30 blocks)
        if (nout == 0) return;
        // -- every argument has passed: the device from here on
        const hipStream_t st = hipStreamPerThread;
        const double2 *vis = reinterpret_cast<const double2 *>(vis_dev);
        double2 *vis_out = reinterpret_cast<double2 *>(vis_out_dev);
        DevBuf<int64_t> rs_buf, mem_buf;
        synced(st, [&] {
            const int64_t *rs = ident ? nullptr : upload(rs_buf, row_start_host, size_t(nrow_out) + 1, st);
            const int64_t *mem = ident ? nullptr : upload(mem_buf, members_host, size_t(nkept), st);
            // lane per input channel wherever a bin fits a wave: 4.2 against 1.0 TB/s at chan_bin = 8
            const bool per_input = chan_bin >= 2 && chan_bin <= 64;
            int lanes = 1;
            while (lanes < chan_bin) lanes <<= 1;
            if (per_input) {
                const dim3 grid = blocks1d(nrow_out * nchan_out * lanes, AVG_THREADS);
                if (ident)
                    hipLaunchKernelGGL(k_avg_per_input<true>, grid, dim3(AVG_THREADS), 0, st, vis, wgt_dev, mask_dev, int(ncorr), nrow,
                                       nchan, int(chan_bin), lanes, rs, mem, nrow_out, nchan_out, vis_out, wgt_out_dev, mask_out_dev);
                else
                    hipLaunchKernelGGL(k_avg_per_input<false>, grid, dim3(AVG_THREADS), 0, st, vis, wgt_dev, mask_dev, int(ncorr), nrow,
                                       nchan, int(chan_bin), lanes, rs, mem, nrow_out, nchan_out, vis_out, wgt_out_dev, mask_out_dev);
            } else {
                const dim3 grid = blocks1d(nrow_out * nchan_out, AVG_THREADS);
                if (ident)
                    hipLaunchKernelGGL(k_avg_per_output<true>, grid, dim3(AVG_THREADS), 0, st, vis, wgt_dev, mask_dev, int(ncorr), nrow,
                                       nchan, chan_bin, rs, mem, nrow_out, nchan_out, vis_out, wgt_out_dev, mask_out_dev);
                else
                    hipLaunchKernelGGL(k_avg_per_output<false>, grid, dim3(AVG_THREADS), 0, st, vis, wgt_dev, mask_dev, int(ncorr), nrow,
                                       nchan, chan_bin, rs, mem, nrow_out, nchan_out, vis_out, wgt_out_dev, mask_out_dev);
            }
            PFB_HIP(hipGetLastError());
        });
    });
}

}  // extern "C"
