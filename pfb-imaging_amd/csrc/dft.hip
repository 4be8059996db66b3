// dft.hip -- the measurement equation summed directly, source by source: predict (sources -> visibilities) and its adjoint
// (visibilities -> flux at a list of positions).
//
// Replaces, for models that are a list of points: the explicit degridder the reference's tests define the gridder by
// (tests/test_hessian_approx.py:44-67), the transient injection of utils/stokes2im.py:491-558 (a dynamic spectrum
// tprofile x fprofile times the phase of one direction, added into the data) and the render + degrid of
// operators/gridder.py:345-351 when the image holds a few thousand isolated pixels.
//
// Phase of (row r, channel c, source s), in turns:  t = (f_c / c0) (su u_r l_s + sv v_r m_s - sw w_r nm1_s + off_r).
// The delay is one chain of three explicit fma()s (the Makefile's -ffp-contract=off leaves those alone), t is reduced to
// [-1/2, 1/2] with t - rint(t) -- exact -- and sincospi(2 t) takes it from there: no multiplication by pi of a large
// argument anywhere, so the error of a term is the rounding of the delay, 2 pi 2^-53 |t| per rounding.  The phase is
// evaluated afresh for every channel; nothing is rotated along the channel axis (freq need not be evenly spaced, and a
// recurrence compounds its rounding).
//
// predict: one thread per (r, c), c fastest.  A workgroup stages DFT_TILE sources at a time in LDS as (l, m, nm1, amp / N);
// every lane reads the same entry at the same time, which the LDS serves as a broadcast.  The inner loop is unrolled over
// DFT_UNROLL sources whose sincospi chains are independent.
// image: workgroup (g, k) holds the IM_SRC sources of group g in registers and walks strip k of the visibilities; a wave
// shuffle reduction and one LDS hop give the workgroup's partial sum, written to partial[k, s]; a second kernel adds the
// strips of every source in ascending k.  No atomics: the result does not depend on scheduling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"
#include "comps_api.hpp"

namespace pfbhip {

constexpr int DFT_BLOCK = 256;    // threads of a workgroup, both kernels
constexpr int DFT_TILE = 64;      // sources staged in LDS at a time (2 KiB)
constexpr int DFT_UNROLL = 4;     // sources in flight per thread
constexpr int IM_SRC = 4;         // sources a thread of the image kernel holds in registers
constexpr int IM_TARGET_BLOCKS = 2048;  // (8 workgroups for each of the 256 CUs)
constexpr double C0 = 299792458.0;
static_assert(DFT_TILE % DFT_UNROLL == 0 && DFT_TILE <= DFT_BLOCK, "tile staging is one entry per thread");

// n - 1 of a direction, oracle/pfb_oracle.c nm1_of: no cancellation for small (l, m); ducc0's branch beyond the horizon
__host__ __device__ inline double nm1_of(double l, double m)
{
    const double r2 = l * l + m * m;
    if (r2 <= 1.0) return -r2 / (1.0 + sqrt(1.0 - r2));
    return -sqrt(r2 - 1.0) - 1.0;
}

struct DftGeom {
    int64_t nrow, nchan, chan0, nsel;  // the handle's shape; the channels [chan0, chan0 + nsel) this call works on
    double u, v, w;                    // su, sv, -sw
    double sgn;
    int accumulate;
};

struct Sample {  // what a thread knows of its visibility
    double u, v, w, k, off;
    int64_t r, c;
};
__device__ __forceinline__ bool load_sample(const DftGeom &g, int64_t i, const double *__restrict__ uvw, const double *__restrict__ freq,
                                            const uint8_t *__restrict__ mask, const double *__restrict__ off, Sample &s)
{
    s.r = i / g.nsel;
    s.c = i - s.r * g.nsel;
    if (mask && !mask[s.r * g.nchan + g.chan0 + s.c]) return false;
    s.u = g.u * uvw[3 * s.r], s.v = g.v * uvw[3 * s.r + 1], s.w = g.w * uvw[3 * s.r + 2];
    s.k = freq[g.chan0 + s.c] / C0;
    s.off = off ? off[s.r] : 0.0;
    return true;
}
// cos and sin of 2 pi t for the phase t (turns) of sample s towards (l, m, nm1)
__device__ __forceinline__ void phase(const Sample &s, double l, double m, double nm1, double &cs, double &sn)
{
    const double delay = fma(s.u, l, fma(s.v, m, fma(s.w, nm1, s.off)));
    double t = s.k * delay;
    t -= rint(t);
    sincospi(2.0 * t, &sn, &cs);
}

// FACT: per-source row / channel factors are present (the transient's profiles)
template <bool FACT>
__global__ void __launch_bounds__(DFT_BLOCK) k_dft_predict(DftGeom g, const double *__restrict__ uvw, const double *__restrict__ freq,
                                                           const uint8_t *__restrict__ mask, const double4 *__restrict__ src, int64_t nsrc,
                                                           const double *__restrict__ rowf, const double *__restrict__ chanf,
                                                           const double *__restrict__ off, const double *__restrict__ wgt,
                                                           double2 *__restrict__ vis)
{
    __shared__ double4 tile[DFT_TILE];
    const int64_t i = int64_t(blockIdx.x) * DFT_BLOCK + threadIdx.x;
    const bool live = i < g.nrow * g.nsel;
    Sample s;
    const bool on = live && load_sample(g, i, uvw, freq, mask, off, s);
    double re = 0.0, im = 0.0;
    for (int64_t s0 = 0; s0 < nsrc; s0 += DFT_TILE) {
        const int n = nsrc - s0 < DFT_TILE ? int(nsrc - s0) : DFT_TILE;
        const int npad = (n + DFT_UNROLL - 1) / DFT_UNROLL * DFT_UNROLL;  // the tail of the last tile: sources of zero flux
        __syncthreads();  // (everyone is done with the previous tile)
        if (int(threadIdx.x) < npad) tile[threadIdx.x] = int(threadIdx.x) < n ? src[s0 + threadIdx.x] : make_double4(0.0, 0.0, 0.0, 0.0);
        __syncthreads();
        if (!on) continue;
        for (int j = 0; j < npad; j += DFT_UNROLL) {
#pragma unroll
            for (int q = 0; q < DFT_UNROLL; ++q) {
                const double4 p = tile[j + q];
                double cs, sn, a = p.w;
                phase(s, p.x, p.y, p.z, cs, sn);
                if (FACT && j + q < n) {
                    if (rowf) a *= rowf[(s0 + j + q) * g.nrow + s.r];
                    if (chanf) a *= chanf[(s0 + j + q) * g.nsel + s.c];
                }
                re = fma(a, cs, re);
                im = fma(a, sn, im);
            }
        }
    }
    if (!live) return;
    if (on) {
        const double wg = wgt ? wgt[i] : 1.0;
        const double2 val = make_double2(wg * re, wg * (g.sgn * im));
        if (g.accumulate) {
            const double2 old = vis[i];
            vis[i] = make_double2(old.x + val.x, old.y + val.y);
        } else {
            vis[i] = val;
        }
    } else if (!g.accumulate) {
        vis[i] = make_double2(0.0, 0.0);
    }
}

// partial[blockIdx.y, s] = sum over strip blockIdx.y of mask wgt Re(vis exp(-sgn 2 pi i t)), s in the group blockIdx.x
__global__ void __launch_bounds__(DFT_BLOCK) k_dft_image(DftGeom g, const double *__restrict__ uvw, const double *__restrict__ freq,
                                                         const uint8_t *__restrict__ mask, const double4 *__restrict__ src, int64_t nsrc,
                                                         const double *__restrict__ off, const double *__restrict__ wgt,
                                                         const double2 *__restrict__ vis, int64_t strip_len, double *__restrict__ partial)
{
    __shared__ double sm[DFT_BLOCK / 64][IM_SRC];
    const int64_t sbase = int64_t(blockIdx.x) * IM_SRC;
    double l[IM_SRC], m[IM_SRC], nm1[IM_SRC], acc[IM_SRC];
#pragma unroll
    for (int q = 0; q < IM_SRC; ++q) {
        const bool has = sbase + q < nsrc;
        const double4 p = has ? src[sbase + q] : make_double4(0.0, 0.0, 0.0, 1.0);
        l[q] = p.x, m[q] = p.y, nm1[q] = p.z, acc[q] = 0.0;
    }
    const int64_t nvis = g.nrow * g.nsel;
    const int64_t begin = int64_t(blockIdx.y) * strip_len, end = begin + strip_len < nvis ? begin + strip_len : nvis;
    for (int64_t i = begin + threadIdx.x; i < end; i += DFT_BLOCK) {
        Sample s;
        if (!load_sample(g, i, uvw, freq, mask, off, s)) continue;
        const double wg = wgt ? wgt[i] : 1.0;
        if (wg == 0.0) continue;
        const double2 v = vis[i];
        const double vr = wg * v.x, vi = wg * (g.sgn * v.y);
#pragma unroll
        for (int q = 0; q < IM_SRC; ++q) {
            double cs, sn;
            phase(s, l[q], m[q], nm1[q], cs, sn);
            acc[q] += fma(vr, cs, vi * sn);
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < IM_SRC; ++q) {
        double a = acc[q];
        for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d);
        if (lane == 0) sm[wave][q] = a;
    }
    __syncthreads();
    if (threadIdx.x < IM_SRC && sbase + threadIdx.x < nsrc) {
        double a = sm[0][threadIdx.x];
        for (int wv = 1; wv < DFT_BLOCK / 64; ++wv) a += sm[wv][threadIdx.x];
        partial[int64_t(blockIdx.y) * nsrc + sbase + threadIdx.x] = a;
    }
}

// out[s] = (sum_k partial[k, s]) / N_s, k ascending
__global__ void __launch_bounds__(DFT_BLOCK) k_dft_image_sum(const double *__restrict__ partial, int64_t nstrips, int64_t nsrc,
                                                             const double4 *__restrict__ src, double *__restrict__ out)
{
    const int64_t s = int64_t(blockIdx.x) * DFT_BLOCK + threadIdx.x;
    if (s >= nsrc) return;
    double a = 0.0;
    for (int64_t k = 0; k < nstrips; ++k) a += partial[k * nsrc + s];
    out[s] = a / src[s].w;
}

// the sources of a component model: (l, m, nm1, b . coeffs / N) per component
__global__ void __launch_bounds__(DFT_BLOCK) k_dft_src_comps(const int64_t *__restrict__ xi, const int64_t *__restrict__ yi,
                                                             const int64_t *__restrict__ pix, int64_t ncomps, int64_t nx, int64_t ny,
                                                             const double *__restrict__ coeffs, const double *__restrict__ b, int nparam,
                                                             const uint8_t *__restrict__ region, double cellx, double celly, double lshift,
                                                             double mshift, int do_w, int divide_by_n, double4 *__restrict__ src)
{
    const int64_t c = int64_t(blockIdx.x) * DFT_BLOCK + threadIdx.x;
    if (c >= ncomps) return;
    const double l = lshift + double(xi[c] - nx / 2) * cellx, m = mshift + double(yi[c] - ny / 2) * celly;
    const double nm1 = do_w ? nm1_of(l, m) : 0.0;
    double a = 0.0;
    for (int k = 0; k < nparam; ++k) a += b[k] * coeffs[size_t(k) * size_t(ncomps) + size_t(c)];
    if (region && !region[pix[c]]) a = 0.0;
    if (divide_by_n) a /= nm1 + 1.0;
    src[c] = make_double4(l, m, nm1, a);
}

}  // namespace pfbhip

using namespace pfbhip;

struct pfbhip_dft {
    int64_t nrow = 0, nchan = 0;
    bool has_mask = false;
    DevBuf<double> uvw, freq;
    DevBuf<uint8_t> mask;
    // per-call scratch, kept between calls
    DevBuf<double4> src;
    DevBuf<double> rowf, chanf, off, wgt, vis, partial, out;
    hipStream_t stream() const { return hipStreamPerThread; }
};

namespace {

bool unit(double s) { return s == 1.0 || s == -1.0; }

DftGeom geometry(const pfbhip_dft *h, const pfbhip_dft_conv *cv)
{
    PFB_REQUIRE(h && cv, "NULL argument");
    PFB_REQUIRE(unit(cv->su) && unit(cv->sv) && unit(cv->sw) && unit(cv->sgn), "su, sv, sw and sgn must each be +1 or -1");
    DftGeom g;
    g.nrow = h->nrow, g.nchan = h->nchan;
    g.chan0 = cv->chan0;
    g.nsel = cv->nchan ? cv->nchan : h->nchan - cv->chan0;
    PFB_REQUIRE(g.chan0 >= 0 && g.nsel >= 1 && g.chan0 + g.nsel <= h->nchan, "channels [%lld, %lld) are not inside the handle's %lld",
                (long long)g.chan0, (long long)(g.chan0 + g.nsel), (long long)h->nchan);
    PFB_REQUIRE(ceil_div(g.nrow * g.nsel, DFT_BLOCK) < (int64_t(1) << 31), "too many visibilities for one call");
    g.u = cv->su, g.v = cv->sv, g.w = -cv->sw;
    g.sgn = cv->sgn;
    g.accumulate = cv->accumulate ? 1 : 0;
    return g;
}

// (l, m, nm1, amp / N) of a host list; amp == NULL: (l, m, nm1, N) as the image kernels want it.  `keep` owns the staging
// array until the caller has synchronised.
void sources_from_host(pfbhip_dft *h, const pfbhip_dft_conv *cv, int64_t nsrc, const double *lm, const double *amp,
                       std::vector<double> &keep)
{
    PFB_REQUIRE(nsrc >= 0 && nsrc < (int64_t(1) << 40), "bad number of sources");
    PFB_REQUIRE(nsrc == 0 || lm, "NULL argument");
    keep.resize(size_t(nsrc) * 4);
    for (int64_t s = 0; s < nsrc; ++s) {
        const double l = lm[2 * s], m = lm[2 * s + 1];
        const double nm1 = cv->do_wgridding ? nm1_of(l, m) : 0.0;
        const double N = cv->divide_by_n ? nm1 + 1.0 : 1.0;
        keep[4 * s] = l, keep[4 * s + 1] = m, keep[4 * s + 2] = nm1;
        keep[4 * s + 3] = amp ? (cv->divide_by_n ? amp[s] / N : amp[s]) : N;
    }
    h->src.ensure(size_t(std::max<int64_t>(nsrc, 1)));
    if (nsrc) PFB_HIP(hipMemcpyAsync(h->src.p, keep.data(), keep.size() * sizeof(double), hipMemcpyHostToDevice, h->stream()));
}

void sources_from_comps(pfbhip_dft *h, const pfbhip_dft_conv *cv, pfbhip_comps *c, const double *basis_host, int use_region,
                        double cellx, double celly, double lshift, double mshift)
{
    PFB_REQUIRE(c && basis_host, "NULL argument");
    PFB_REQUIRE(!use_region || c->has_region, "no region mask bound: call pfbhip_comps_set_region first");
    PFB_REQUIRE(std::isfinite(cellx) && std::isfinite(celly) && std::isfinite(lshift) && std::isfinite(mshift), "geometry is not finite");
    for (int k = 0; k < c->nparam; ++k) PFB_REQUIRE(std::isfinite(basis_host[k]), "basis[%d] is not finite", k);
    const hipStream_t st = h->stream();
    h->src.ensure(size_t(std::max<int64_t>(c->ncomps, 1)));
    PFB_HIP(hipMemcpyAsync(c->basis.p, basis_host, size_t(c->nparam) * sizeof(double), hipMemcpyHostToDevice, st));
    if (c->ncomps)
        hipLaunchKernelGGL(k_dft_src_comps, dim3(uint32_t(ceil_div(c->ncomps, DFT_BLOCK))), dim3(DFT_BLOCK), 0, st, c->xi.p, c->yi.p, c->pix.p,
                           c->ncomps, c->nx, c->ny, c->coeffs.p, c->basis.p, c->nparam, use_region ? c->region.p : nullptr, cellx, celly,
                           lshift, mshift, cv->do_wgridding ? 1 : 0, cv->divide_by_n ? 1 : 0, h->src.p);
    PFB_HIP(hipGetLastError());
}

// launches predict on h->src; rowf / chanf / off are host arrays (uploaded here), wgt / vis device arrays
void predict_async(pfbhip_dft *h, const DftGeom &g, int64_t nsrc, const double *rowf, const double *chanf, const double *off,
                   const double *wgt_dev, double *vis_dev)
{
    PFB_REQUIRE(vis_dev, "NULL argument");
    const hipStream_t st = h->stream();
    const double *rowf_d = upload(h->rowf, rowf, size_t(nsrc) * size_t(g.nrow), st);
    const double *chanf_d = upload(h->chanf, chanf, size_t(nsrc) * size_t(g.nsel), st);
    const double *off_d = upload(h->off, off, size_t(g.nrow), st);
    const dim3 grid(uint32_t(ceil_div(g.nrow * g.nsel, DFT_BLOCK)));
    const uint8_t *mask = h->has_mask ? h->mask.p : nullptr;
    if (rowf_d || chanf_d)
        hipLaunchKernelGGL(k_dft_predict<true>, grid, dim3(DFT_BLOCK), 0, st, g, h->uvw.p, h->freq.p, mask, h->src.p, nsrc, rowf_d, chanf_d,
                           off_d, wgt_dev, reinterpret_cast<double2 *>(vis_dev));
    else
        hipLaunchKernelGGL(k_dft_predict<false>, grid, dim3(DFT_BLOCK), 0, st, g, h->uvw.p, h->freq.p, mask, h->src.p, nsrc, rowf_d, chanf_d,
                           off_d, wgt_dev, reinterpret_cast<double2 *>(vis_dev));
    PFB_HIP(hipGetLastError());
}

// host-array form of predict_async: vis goes up only when it is added to
void predict_host(pfbhip_dft *h, const DftGeom &g, int64_t nsrc, const double *rowf, const double *chanf, const double *off,
                  const double *wgt_host, double *vis_host)
{
    PFB_REQUIRE(vis_host, "NULL argument");
    const hipStream_t st = h->stream();
    const size_t nvis = size_t(g.nrow) * size_t(g.nsel);
    const double *wgt_d = upload(h->wgt, wgt_host, nvis, st);
    h->vis.ensure(2 * nvis);
    if (g.accumulate) PFB_HIP(hipMemcpyAsync(h->vis.p, vis_host, 2 * nvis * sizeof(double), hipMemcpyHostToDevice, st));
    predict_async(h, g, nsrc, rowf, chanf, off, wgt_d, h->vis.p);
    PFB_HIP(hipMemcpyAsync(vis_host, h->vis.p, 2 * nvis * sizeof(double), hipMemcpyDeviceToHost, st));
}

void image_async(pfbhip_dft *h, const DftGeom &g, int64_t nsrc, const double *off, const double *wgt_dev, const double *vis_dev,
                 double *out_host)
{
    PFB_REQUIRE(vis_dev && (out_host || nsrc == 0), "NULL argument");
    if (nsrc == 0) return;
    const hipStream_t st = h->stream();
    const double *off_d = upload(h->off, off, size_t(g.nrow), st);
    const int64_t nvis = g.nrow * g.nsel, ngroups = ceil_div(nsrc, IM_SRC);
    PFB_REQUIRE(ngroups < (int64_t(1) << 31), "too many sources for one call");
    // strips: enough workgroups to fill the device, whole workgroup passes each, at most 65535 (grid y)
    int64_t nstrips = std::min<int64_t>(std::max<int64_t>(ceil_div(IM_TARGET_BLOCKS, ngroups), 1), ceil_div(nvis, DFT_BLOCK));
    nstrips = std::min<int64_t>(nstrips, 65535);
    const int64_t strip_len = ceil_div(ceil_div(nvis, nstrips), DFT_BLOCK) * DFT_BLOCK;
    nstrips = ceil_div(nvis, strip_len);
    h->partial.ensure(size_t(nstrips) * size_t(nsrc));
    h->out.ensure(size_t(nsrc));
    hipLaunchKernelGGL(k_dft_image, dim3(uint32_t(ngroups), uint32_t(nstrips)), dim3(DFT_BLOCK), 0, st, g, h->uvw.p, h->freq.p,
                       h->has_mask ? h->mask.p : nullptr, h->src.p, nsrc, off_d, wgt_dev, reinterpret_cast<const double2 *>(vis_dev), strip_len,
                       h->partial.p);
    hipLaunchKernelGGL(k_dft_image_sum, dim3(uint32_t(ceil_div(nsrc, DFT_BLOCK))), dim3(DFT_BLOCK), 0, st, h->partial.p, nstrips, nsrc,
                       h->src.p, h->out.p);
    PFB_HIP(hipGetLastError());
    PFB_HIP(hipMemcpyAsync(out_host, h->out.p, size_t(nsrc) * sizeof(double), hipMemcpyDeviceToHost, st));
}

}  // namespace

extern "C" {

int pfbhip_dft_create(int64_t nrow, int64_t nchan, const double *uvw_host, const double *freq_host, const uint8_t *mask_host,
                      pfbhip_dft **out)
{
    return guarded([&] {
        PFB_REQUIRE(out, "NULL argument");
        *out = nullptr;
        PFB_REQUIRE(uvw_host && freq_host, "NULL argument");
        PFB_REQUIRE(nrow >= 1 && nchan >= 1 && nrow < (int64_t(1) << 40) && nchan < (int64_t(1) << 31), "bad sizes");
        auto h = std::make_unique<pfbhip_dft>();
        h->nrow = nrow, h->nchan = nchan;
        const hipStream_t st = h->stream();
        synced(st, [&] {
            h->uvw.alloc(size_t(nrow) * 3);
            h->freq.alloc(size_t(nchan));
            PFB_HIP(hipMemcpyAsync(h->uvw.p, uvw_host, h->uvw.bytes(), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(h->freq.p, freq_host, h->freq.bytes(), hipMemcpyHostToDevice, st));
            if (mask_host) {
                h->mask.alloc(size_t(nrow) * size_t(nchan));
                PFB_HIP(hipMemcpyAsync(h->mask.p, mask_host, h->mask.bytes(), hipMemcpyHostToDevice, st));
                h->has_mask = true;
            }
        });
        *out = h.release();
    });
}

int pfbhip_dft_destroy(pfbhip_dft *h)
{
    return guarded([&] {
        if (h) (void)hipStreamSynchronize(h->stream());
        delete h;
    });
}

int pfbhip_dft_predict(pfbhip_dft *h, const pfbhip_dft_conv *conv, int64_t nsrc, const double *lm, const double *amp,
                       const double *rowf, const double *chanf, const double *off, const double *wgt_host, double *vis_host)
{
    return guarded([&] {
        const DftGeom g = geometry(h, conv);
        PFB_REQUIRE(amp || nsrc == 0, "NULL argument");
        std::vector<double> keep;
        synced(h->stream(), [&] {
            sources_from_host(h, conv, nsrc, lm, amp, keep);
            predict_host(h, g, nsrc, rowf, chanf, off, wgt_host, vis_host);
        });
    });
}

int pfbhip_dft_predict_dev(pfbhip_dft *h, const pfbhip_dft_conv *conv, int64_t nsrc, const double *lm, const double *amp,
                           const double *rowf, const double *chanf, const double *off, const double *wgt_dev, double *vis_dev)
{
    return guarded([&] {
        const DftGeom g = geometry(h, conv);
        PFB_REQUIRE(amp || nsrc == 0, "NULL argument");
        std::vector<double> keep;
        synced(h->stream(), [&] {
            sources_from_host(h, conv, nsrc, lm, amp, keep);
            predict_async(h, g, nsrc, rowf, chanf, off, wgt_dev, vis_dev);
        });
    });
}

int pfbhip_dft_predict_comps(pfbhip_dft *h, const pfbhip_dft_conv *conv, pfbhip_comps *comps, const double *basis_host,
                             int use_region, double cellx, double celly, double lshift, double mshift, const double *off,
                             const double *wgt_host, double *vis_host)
{
    return guarded([&] {
        const DftGeom g = geometry(h, conv);
        synced(h->stream(), [&] {
            sources_from_comps(h, conv, comps, basis_host, use_region, cellx, celly, lshift, mshift);
            predict_host(h, g, comps->ncomps, nullptr, nullptr, off, wgt_host, vis_host);
        });
    });
}

int pfbhip_dft_predict_comps_dev(pfbhip_dft *h, const pfbhip_dft_conv *conv, pfbhip_comps *comps, const double *basis_host,
                                 int use_region, double cellx, double celly, double lshift, double mshift, const double *off,
                                 const double *wgt_dev, double *vis_dev)
{
    return guarded([&] {
        const DftGeom g = geometry(h, conv);
        synced(h->stream(), [&] {
            sources_from_comps(h, conv, comps, basis_host, use_region, cellx, celly, lshift, mshift);
            predict_async(h, g, comps->ncomps, nullptr, nullptr, off, wgt_dev, vis_dev);
        });
    });
}

int pfbhip_dft_image(pfbhip_dft *h, const pfbhip_dft_conv *conv, int64_t nsrc, const double *lm, const double *off,
                     const double *wgt_host, const double *vis_host, double *out_host)
{
    return guarded([&] {
        const DftGeom g = geometry(h, conv);
        PFB_REQUIRE(vis_host, "NULL argument");
        std::vector<double> keep;
        synced(h->stream(), [&] {
            const hipStream_t st = h->stream();
            const size_t nvis = size_t(g.nrow) * size_t(g.nsel);
            sources_from_host(h, conv, nsrc, lm, nullptr, keep);
            const double *wgt_d = upload(h->wgt, wgt_host, nvis, st);
            const double *vis_d = upload(h->vis, vis_host, 2 * nvis, st);
            image_async(h, g, nsrc, off, wgt_d, vis_d, out_host);
        });
    });
}

int pfbhip_dft_image_dev(pfbhip_dft *h, const pfbhip_dft_conv *conv, int64_t nsrc, const double *lm, const double *off,
                         const double *wgt_dev, const double *vis_dev, double *out_host)
{
    return guarded([&] {
        const DftGeom g = geometry(h, conv);
        std::vector<double> keep;
        synced(h->stream(), [&] {
            sources_from_host(h, conv, nsrc, lm, nullptr, keep);
            image_async(h, g, nsrc, off, wgt_dev, vis_dev, out_host);
        });
    });
}

}  // extern "C"
