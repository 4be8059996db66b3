// reweight.hip -- l1 reweighting of the l21 regulariser with the coefficient cubes resident in HBM.
//
// Mirrors L21.init_reweighting / update_weights of pfb-imaging (src/pfb_imaging/prox/l21.py:52-88) and l1reweight_func
// (utils/misc.py:742-755):
//     s      = sum_band Psi^H x                                   (added in band order, as np.sum(axis=0) does)
//     weight = (1 + rmsfactor) / (1 + |s|^alpha / rms_basis^alpha)
//     rms_b  = population standard deviation of the NONZERO entries of s in basis b
// The analysis runs on the dictionary's stream into a caller-owned scratch cube (nband, nbasis, nxmax, nymax); the
// weight is ONE pass over it (nband planes read, one written), the rms two reducing passes.
#pragma clang fp contract(fast)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"
#include "pipeline_api.hpp"

namespace pfbhip {

constexpr int RW_MAXB = 16;    // bands held in registers by the one-pass kernel (LOOP_MAXB of devloop.hpp)
constexpr int RW_BLOCKS = 512;  // workgroups per basis of the rms passes (8 per CU at four bases; one f64 partial each per quantity)

// |s|^alpha: 0 -> alpha = 2, 1 -> alpha = 4 (the reference's two defaults: products), 2 -> pow
template <int MODE>
__device__ __forceinline__ double rw_pow(double a, double alpha)
{
    if (MODE == 0) return a * a;
    if (MODE == 1) return (a * a) * (a * a);
    return pow(a, alpha);
}
template <int MODE>
__device__ __forceinline__ double rw_weight(double s, double num, double inv_ra, double alpha)
{
    return num / (1.0 + rw_pow<MODE>(fabs(s), alpha) * inv_ra);
}

// One basis plane (m coefficients, m even) of a cube (NB, n): two coefficients per thread with 16-byte accesses, every
// band of a coefficient in the same thread.  coef / w point at the plane; num = 1 + rmsfactor, inv_ra = 1 / rms^alpha.
template <int NB, int MODE>
__global__ void __launch_bounds__(256) k_l21_reweight(const double *__restrict__ coef, int64_t n, int64_t m, double num, double inv_ra,
                                                       double alpha, double *__restrict__ w)
{
    const int64_t m2 = m / 2;
    for (int64_t i = blockIdx.x * int64_t(256) + threadIdx.x; i < m2; i += int64_t(gridDim.x) * 256) {
        double2 a[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) a[b] = reinterpret_cast<const double2 *>(coef + size_t(b) * size_t(n))[i];
        double2 s = a[0];
#pragma unroll
        for (int b = 1; b < NB; ++b) {
            s.x += a[b].x;
            s.y += a[b].y;
        }
        reinterpret_cast<double2 *>(w)[i] = double2{rw_weight<MODE>(s.x, num, inv_ra, alpha), rw_weight<MODE>(s.y, num, inv_ra, alpha)};
    }
}
// Any band count / odd plane sizes / unaligned pointers: one coefficient per thread, bands streamed
template <int MODE>
__global__ void __launch_bounds__(256) k_l21_reweight_gen(const double *__restrict__ coef, int nband, int64_t n, int64_t m, double num,
                                                           double inv_ra, double alpha, double *__restrict__ w)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i >= m) return;
    double s = coef[i];
    for (int b = 1; b < nband; ++b) s += coef[size_t(b) * size_t(n) + size_t(i)];
    w[i] = rw_weight<MODE>(s, num, inv_ra, alpha);
}

// sum of a wave, then of the block's four waves in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double rw_block_sum(double v, double *sm)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = sm[0] + sm[1] + sm[2] + sm[3];
    __syncthreads();
    return t;
}
// rms pass 1, grid (RW_BLOCKS, nbasis): the band sum of each coefficient is written over band 0 of the cube (the same
// thread read it), partials[(basis * RW_BLOCKS + block) * 2 + {0, 1}] = {number, sum} of the nonzero band sums
__global__ void __launch_bounds__(256) k_l21_rms_sum(double *__restrict__ coef, int nband, int64_t n, int64_t m,
                                                     double *__restrict__ partials)
{
    __shared__ double sm[4];
    double *plane = coef + size_t(blockIdx.y) * size_t(m);
    double cnt = 0.0, sum = 0.0;
    for (int64_t i = blockIdx.x * int64_t(256) + threadIdx.x; i < m; i += int64_t(RW_BLOCKS) * 256) {
        double s = plane[i];
        for (int b = 1; b < nband; ++b) s += plane[size_t(b) * size_t(n) + size_t(i)];
        plane[i] = s;
        cnt += s != 0.0 ? 1.0 : 0.0;
        sum += s;
    }
    const double c = rw_block_sum(cnt, sm), t = rw_block_sum(sum, sm);
    if (threadIdx.x == 0) {
        partials[(size_t(blockIdx.y) * RW_BLOCKS + blockIdx.x) * 2] = c;
        partials[(size_t(blockIdx.y) * RW_BLOCKS + blockIdx.x) * 2 + 1] = t;
    }
}
// rms pass 2, one basis plane of band sums: partials[block] = sum of (s - mean)^2 over the nonzero s
__global__ void __launch_bounds__(256) k_l21_rms_dev2(const double *__restrict__ plane, int64_t m, double mean,
                                                      double *__restrict__ partials)
{
    __shared__ double sm[4];
    double q = 0.0;
    for (int64_t i = blockIdx.x * int64_t(256) + threadIdx.x; i < m; i += int64_t(RW_BLOCKS) * 256) {
        const double s = plane[i], d = s - mean;
        q += s != 0.0 ? d * d : 0.0;
    }
    const double t = rw_block_sum(q, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

template <int NB, int MODE>
static void launch_reweight(hipStream_t st, const double *coef, int64_t n, int64_t m, double num, double inv_ra, double alpha, double *w)
{
    const int64_t blocks = std::min<int64_t>(ceil_div(m / 2, 256), 8192);
    hipLaunchKernelGGL((k_l21_reweight<NB, MODE>), dim3(uint32_t(blocks)), dim3(256), 0, st, coef, n, m, num, inv_ra, alpha, w);
}
template <int MODE, int NB = 1>
static void dispatch_reweight(int nband, hipStream_t st, const double *coef, int64_t n, int64_t m, double num, double inv_ra,
                              double alpha, double *w)
{
    if constexpr (NB <= RW_MAXB) {
        if (nband == NB) return launch_reweight<NB, MODE>(st, coef, n, m, num, inv_ra, alpha, w);
        dispatch_reweight<MODE, NB + 1>(nband, st, coef, n, m, num, inv_ra, alpha, w);
    }
}
template <int MODE>
static void reweight_plane(hipStream_t st, bool fast, int nband, const double *coef, int64_t n, int64_t m, double num, double inv_ra,
                           double alpha, double *w)
{
    if (fast)
        dispatch_reweight<MODE>(nband, st, coef, n, m, num, inv_ra, alpha, w);
    else
        hipLaunchKernelGGL(k_l21_reweight_gen<MODE>, dim3(uint32_t(ceil_div(m, 256))), dim3(256), 0, st, coef, nband, n, m, num,
                           inv_ra, alpha, w);
}

// weight (nbasis, m) from the coefficient cube coef (nband, nbasis, m), on `st`
static void reweight_async(hipStream_t st, const double *coef, int64_t nband, int nbasis, int64_t m, const double *rms,
                           double rmsfactor, double alpha, double *w)
{
    const int64_t n = int64_t(nbasis) * m;
    const bool aligned = reinterpret_cast<uintptr_t>(coef) % 16 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0;
    const bool fast = nband <= RW_MAXB && m % 2 == 0 && aligned;
    for (int b = 0; b < nbasis; ++b) {
        const double *cb = coef + size_t(b) * size_t(m);
        double *wb = w + size_t(b) * size_t(m);
        const double num = 1.0 + rmsfactor, inv_ra = 1.0 / std::pow(rms[b], alpha);
        if (alpha == 2.0)
            reweight_plane<0>(st, fast, int(nband), cb, n, m, num, inv_ra, alpha, wb);
        else if (alpha == 4.0)
            reweight_plane<1>(st, fast, int(nband), cb, n, m, num, inv_ra, alpha, wb);
        else
            reweight_plane<2>(st, fast, int(nband), cb, n, m, num, inv_ra, alpha, wb);
    }
    PFB_HIP(hipGetLastError());
}

// rms / count per basis of the band sum of coef (nband, nbasis, m); band 0 of coef is overwritten with the band sum
static void rms_sync(hipStream_t st, double *coef, int64_t nband, int nbasis, int64_t m, double *rms_out, int64_t *count_out)
{
    const int64_t n = int64_t(nbasis) * m;
    DevBuf<double> partials(size_t(nbasis) * RW_BLOCKS * 2);
    std::vector<double> host(size_t(nbasis) * RW_BLOCKS * 2), cnt(size_t(nbasis), 0.0);
    synced(st, [&] {  // (partials and host are declared outside: they outlive the wait on every path)
        hipLaunchKernelGGL(k_l21_rms_sum, dim3(RW_BLOCKS, uint32_t(nbasis)), dim3(256), 0, st, coef, int(nband), n, m, partials.p);
        PFB_HIP(hipGetLastError());
        PFB_HIP(hipMemcpyAsync(host.data(), partials.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        PFB_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < nbasis; ++b) {
            double c = 0.0, t = 0.0;
            for (int i = 0; i < RW_BLOCKS; ++i) {  // (fixed order: the result does not depend on the schedule)
                c += host[(size_t(b) * RW_BLOCKS + size_t(i)) * 2];
                t += host[(size_t(b) * RW_BLOCKS + size_t(i)) * 2 + 1];
            }
            cnt[size_t(b)] = c;
            if (c > 0.0)
                hipLaunchKernelGGL(k_l21_rms_dev2, dim3(RW_BLOCKS), dim3(256), 0, st, coef + size_t(b) * size_t(m), m, t / c,
                                   partials.p + size_t(b) * RW_BLOCKS);
        }
        PFB_HIP(hipGetLastError());
        PFB_HIP(hipMemcpyAsync(host.data(), partials.p, size_t(nbasis) * RW_BLOCKS * sizeof(double), hipMemcpyDeviceToHost, st));
    });
    for (int b = 0; b < nbasis; ++b) {
        double q = 0.0;
        for (int i = 0; i < RW_BLOCKS; ++i) q += host[size_t(b) * RW_BLOCKS + size_t(i)];
        count_out[b] = int64_t(cnt[size_t(b)]);
        rms_out[b] = cnt[size_t(b)] > 0.0 ? std::sqrt(q / cnt[size_t(b)]) : 0.0;
    }
}

}  // namespace pfbhip

using namespace pfbhip;

namespace {

struct Geometry {
    int64_t nx, ny, nxmax, nymax, m;
    int nbasis;
    size_t npix, cube;
};
Geometry geometry(const pfbhip_psi *psi)
{
    Geometry g;
    psi_geometry(psi, &g.nx, &g.ny, &g.nbasis, &g.nxmax, &g.nymax);
    g.m = g.nxmax * g.nymax;
    g.npix = size_t(g.nx) * size_t(g.ny);
    g.cube = size_t(g.nbasis) * size_t(g.m);
    return g;
}
void analyse(pfbhip_psi *psi, const Geometry &g, const double *x_dev, int64_t nband, double *coef_dev)
{
    for (int64_t b = 0; b < nband; ++b) psi_dot_async(psi, x_dev + size_t(b) * g.npix, coef_dev + size_t(b) * g.cube);
}
void check_rms(const double *rms, int nbasis, double alpha)
{
    for (int b = 0; b < nbasis; ++b)
        PFB_REQUIRE(rms[b] > 0.0 && std::isfinite(rms[b]), "rms[%d] = %g must be positive and finite", b, rms[b]);
    PFB_REQUIRE(std::isfinite(alpha), "alpha must be finite");
}

}  // namespace

extern "C" {

int pfbhip_l21_reweight_dev(pfbhip_psi *psi, const double *x_dev, int64_t nband, const double *rms, double rmsfactor, double alpha,
                            double *scratch_dev, double *weight_dev)
{
    return guarded([&] {
        PFB_REQUIRE(psi && x_dev && rms && scratch_dev && weight_dev && nband >= 1, "bad arguments");
        const Geometry g = geometry(psi);
        check_rms(rms, g.nbasis, alpha);
        const hipStream_t st = psi_stream(psi);
        synced(st, [&] {
            analyse(psi, g, x_dev, nband, scratch_dev);
            reweight_async(st, scratch_dev, nband, g.nbasis, g.m, rms, rmsfactor, alpha, weight_dev);
        });
    });
}

int pfbhip_l21_rms_dev(pfbhip_psi *psi, const double *update_dev, int64_t nband, double *scratch_dev, double *rms_out,
                       int64_t *count_out)
{
    return guarded([&] {
        PFB_REQUIRE(psi && update_dev && scratch_dev && rms_out && count_out && nband >= 1, "bad arguments");
        const Geometry g = geometry(psi);
        synced(psi_stream(psi), [&] { analyse(psi, g, update_dev, nband, scratch_dev); });
        rms_sync(psi_stream(psi), scratch_dev, nband, g.nbasis, g.m, rms_out, count_out);
    });
}

int pfbhip_l21_reweight(pfbhip_psi *psi, const double *x_host, int64_t nband, const double *rms, double rmsfactor, double alpha,
                        double *weight_host, double *bandsum_host)
{
    return guarded([&] {
        PFB_REQUIRE(psi && x_host && rms && weight_host && nband >= 1, "bad arguments");
        const Geometry g = geometry(psi);
        check_rms(rms, g.nbasis, alpha);
        const hipStream_t st = psi_stream(psi);
        DevBuf<double> x(size_t(nband) * g.npix), coef(size_t(nband) * g.cube), w(g.cube);
        DevBuf<double> partials(bandsum_host ? size_t(g.nbasis) * RW_BLOCKS * 2 : 0);
        synced(st, [&] {
            PFB_HIP(hipMemcpyAsync(x.p, x_host, x.n * sizeof(double), hipMemcpyHostToDevice, st));
            analyse(psi, g, x.p, nband, coef.p);
            reweight_async(st, coef.p, nband, g.nbasis, g.m, rms, rmsfactor, alpha, w.p);
            PFB_HIP(hipMemcpyAsync(weight_host, w.p, g.cube * sizeof(double), hipMemcpyDeviceToHost, st));
            if (bandsum_host) {  // the band sum itself, as the rms passes form it (tests: bit-identical to np.sum(axis=0))
                hipLaunchKernelGGL(k_l21_rms_sum, dim3(RW_BLOCKS, uint32_t(g.nbasis)), dim3(256), 0, st, coef.p, int(nband),
                                   int64_t(g.cube), g.m, partials.p);
                PFB_HIP(hipGetLastError());
                PFB_HIP(hipMemcpyAsync(bandsum_host, coef.p, g.cube * sizeof(double), hipMemcpyDeviceToHost, st));
            }
        });
    });
}

int pfbhip_l21_rms(pfbhip_psi *psi, const double *update_host, int64_t nband, double *rms_out, int64_t *count_out)
{
    return guarded([&] {
        PFB_REQUIRE(psi && update_host && rms_out && count_out && nband >= 1, "bad arguments");
        const Geometry g = geometry(psi);
        const hipStream_t st = psi_stream(psi);
        DevBuf<double> x(size_t(nband) * g.npix), coef(size_t(nband) * g.cube);
        synced(st, [&] {
            PFB_HIP(hipMemcpyAsync(x.p, update_host, x.n * sizeof(double), hipMemcpyHostToDevice, st));
            analyse(psi, g, x.p, nband, coef.p);
        });
        rms_sync(st, coef.p, nband, g.nbasis, g.m, rms_out, count_out);
    });
}

}  // extern "C"
