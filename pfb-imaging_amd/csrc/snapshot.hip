// snapshot.hip -- the array steps of one `pfb hci` snapshot on a device-resident chunk (vischunk.py, utils/stokes2im.py) on
// MI355X: what src/pfb_imaging/utils/stokes2im.py::stokes_image of the reference does in numpy around its two vis2dirty
// calls per Stokes.
//
//   pfbhip_chunk_rephase_residual_dev   :364-373 (rephasing by w_diff) and :466-468 (model subtraction and mask)
//   pfbhip_chunk_l2_reweight_joint_dev  :470-481 (one residual variance over every correlation)
//   pfbhip_snapshot_finish_dev          :684-692 (PSF-peak normalisation, rms), :707-708 (beam), :731-737, :750-753 (float32,
//                                       transposed outputs)
//
// The sums are those of vischunk.hip (vischunk_api.hpp): block partials reduced along a fixed tree, one final block, no
// float atomics, so every result is bit-identical from call to call.  The PSF peak is a maximum reduced the same way.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"
#include "vischunk_api.hpp"

namespace pfbhip {

constexpr double SNAP_SPEED_OF_LIGHT = 299792458.0;
constexpr int SNAP_TILE = 32;  // the transposing kernels move SNAP_TILE x SNAP_TILE tiles with CHUNK_THREADS = 32 x 8 threads

// vis[k, i] = (vis[k, i] p - model[k, i] p) * mask[i], p = exp(-2 pi i fc[chan] w_diff[row]) (1 without w_diff), for every
// correlation k of sample i: the phase is formed once per sample, in cycles, and reduced before it meets pi (as
// k_permute_in_psf does).  The mask applies only with a model (:467-468); masked samples become exact zeros.
__global__ void __launch_bounds__(CHUNK_THREADS) k_rephase_residual(double2 *__restrict__ vis, const double2 *__restrict__ model,
                                                                    const uint8_t *__restrict__ mask, const double *__restrict__ w_diff,
                                                                    const double *__restrict__ fc, int ncorr, int64_t nvis, int nchan)
{
    const int64_t i = blockIdx.x * int64_t(CHUNK_THREADS) + threadIdx.x;
    if (i >= nvis) return;
    double c = 1.0, s = 0.0;
    if (w_diff) {
        const int64_t row = i / nchan;
        const int chan = int(i - row * nchan);
        double ph = w_diff[row] * fc[chan];
        ph -= rint(ph);
        sincospi(-2.0 * ph, &s, &c);
    }
    const bool keep = !model || mask[i];
    for (int k = 0; k < ncorr; ++k) {
        const size_t idx = size_t(k) * size_t(nvis) + size_t(i);
        double2 v = make_double2(0.0, 0.0);
        if (keep) {
            v = vis[idx];
            if (w_diff) v = make_double2(v.x * c - v.y * s, v.x * s + v.y * c);
            if (model) {
                double2 m = model[idx];
                if (w_diff) m = make_double2(m.x * c - m.y * s, m.x * s + m.y * c);
                v.x -= m.x;
                v.y -= m.y;
            }
        }
        vis[idx] = v;
    }
}

// wgt[c, i] = (dof + 1) / (dof + ressq / ovar) / ovar with ressq = |r|^2 * mask: replaces the weights (:477)
__global__ void __launch_bounds__(CHUNK_THREADS) k_l2_reweight_joint(const double2 *__restrict__ r, const uint8_t *__restrict__ mask,
                                                                     double ovar, double dof, int64_t nvis, double *__restrict__ wgt)
{
    const int c = blockIdx.y;
    const int64_t i = blockIdx.x * int64_t(CHUNK_THREADS) + threadIdx.x;
    if (i >= nvis) return;
    const size_t k = size_t(c) * size_t(nvis) + size_t(i);
    const double2 v = r[k];
    const double ressq = mask[i] ? v.x * v.x + v.y * v.y : 0.0;
    wgt[k] = (dof + 1.0) / (dof + ressq / ovar) / ovar;
}

// numpy's maximum: a NaN wins
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

// max of s[0, CHUNK_THREADS) into s[0]
__device__ __forceinline__ void block_tree_max(double *s)
{
    __syncthreads();
    for (int h = CHUNK_THREADS / 2; h > 0; h >>= 1) {
        if (int(threadIdx.x) < h) s[threadIdx.x] = nan_max(s[threadIdx.x], s[threadIdx.x + h]);
        __syncthreads();
    }
}

// part[c * gridDim.x + b] = max over block b's grid-stride slice of plane c = blockIdx.y (x[c, 0] where the slice is empty)
__global__ void __launch_bounds__(CHUNK_THREADS) k_max_partial(const double *__restrict__ x, int64_t n, double *__restrict__ part)
{
    __shared__ double s[CHUNK_THREADS];
    const double *plane = x + size_t(blockIdx.y) * size_t(n);
    double t = plane[0];
    for (int64_t i = blockIdx.x * int64_t(CHUNK_THREADS) + threadIdx.x; i < n; i += int64_t(gridDim.x) * CHUNK_THREADS)
        t = nan_max(plane[i], t);
    s[threadIdx.x] = t;
    block_tree_max(s);
    if (threadIdx.x == 0) part[size_t(blockIdx.y) * gridDim.x + blockIdx.x] = s[0];
}

__global__ void __launch_bounds__(CHUNK_THREADS) k_max_final(const double *__restrict__ part, int nb, double *__restrict__ out)
{
    __shared__ double s[CHUNK_THREADS];
    const double *p = part + size_t(blockIdx.x) * nb;
    double t = p[0];
    for (int b = threadIdx.x; b < nb; b += CHUNK_THREADS) t = nan_max(p[b], t);
    s[threadIdx.x] = t;
    block_tree_max(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

// One SNAP_TILE x SNAP_TILE tile of plane c = blockIdx.z of x (ns, nx, ny): rows blockIdx.y * SNAP_TILE.., columns
// blockIdx.x * SNAP_TILE...  Thread t handles column t & 31 of rows (t >> 5) + 8 j: loads and stores run along ny.  The
// transposed output (ns, ny, nx) leaves through an LDS tile padded by one element, along nx.
struct TilePos {
    int tx, ty, x0, y0;
    size_t plane, blk, nblk;
};
__device__ __forceinline__ TilePos tile_pos(int nx, int ny)
{
    TilePos p;
    p.tx = threadIdx.x & (SNAP_TILE - 1);
    p.ty = threadIdx.x / SNAP_TILE;
    p.x0 = blockIdx.y * SNAP_TILE;
    p.y0 = blockIdx.x * SNAP_TILE;
    p.plane = size_t(blockIdx.z) * size_t(nx) * size_t(ny);
    p.blk = size_t(blockIdx.y) * gridDim.x + blockIdx.x;
    p.nblk = size_t(gridDim.x) * gridDim.y;
    return p;
}
template <class TOut>
__device__ __forceinline__ void store_transposed(const double (*tile)[SNAP_TILE + 1], const TilePos &p, int nx, int ny, TOut *out_t)
{
    for (int j = 0; j < SNAP_TILE; j += CHUNK_THREADS / SNAP_TILE) {
        const int oy = p.y0 + p.ty + j, ox = p.x0 + p.tx;
        if (oy < ny && ox < nx) out_t[p.plane + size_t(oy) * size_t(nx) + size_t(ox)] = TOut(tile[p.tx][p.ty + j]);
    }
}

// x[c] /= pm[c] in place (:690-691; zeros where the Stokes is not active), out_t (may be NULL) its transpose as TOut, part (may
// be NULL) the block's sum of the normalised values at part[c * nblk + blk]
template <class TOut>
__global__ void __launch_bounds__(CHUNK_THREADS) k_norm_tile(double *__restrict__ x, const double *__restrict__ pm,
                                                             const uint8_t *__restrict__ active, int nx, int ny, TOut *__restrict__ out_t,
                                                             double *__restrict__ part)
{
    __shared__ double tile[SNAP_TILE][SNAP_TILE + 1];
    __shared__ double s[CHUNK_THREADS];
    const TilePos p = tile_pos(nx, ny);
    const bool act = active[blockIdx.z] != 0;
    const double d = pm[blockIdx.z];
    double t = 0.0;
    for (int j = 0; j < SNAP_TILE; j += CHUNK_THREADS / SNAP_TILE) {
        const int ix = p.x0 + p.ty + j, iy = p.y0 + p.tx;
        if (ix < nx && iy < ny) {
            const size_t k = p.plane + size_t(ix) * size_t(ny) + size_t(iy);
            const double y = act ? x[k] / d : 0.0;
            x[k] = y;
            tile[p.ty + j][p.tx] = y;
            t += y;
        }
    }
    if (out_t) {
        __syncthreads();
        store_transposed(tile, p, nx, ny, out_t);
    }
    if (part) {
        s[threadIdx.x] = t;
        block_tree_sum(s);
        if (threadIdx.x == 0) part[size_t(blockIdx.z) * p.nblk + p.blk] = s[0];
    }
}

// The second pass over the normalised residual: the block's share of sum (x - mean)^2 with mean = sum[c] / (nx ny) (np.std is
// two-pass, :692), then x *= pbeam / (pbeam^2 + eta) in place (:708; pbeam may be NULL) and the transposed outputs: the cube
// and, with a beam, pbeam^2 + eta (:751) -- the latter for EVERY Stokes, as the reference forms it from the beam alone.  A
// Stokes that is not active keeps its zeros whatever its beam holds (0 * NaN would not).
template <class TOut>
__global__ void __launch_bounds__(CHUNK_THREADS) k_rms_beam_tile(double *__restrict__ x, const double *__restrict__ sum,
                                                                 const uint8_t *__restrict__ active, const double *__restrict__ pbeam,
                                                                 double eta, int nx, int ny,
                                                                 TOut *__restrict__ cube_t, TOut *__restrict__ bw_t, double *__restrict__ part)
{
    __shared__ double tile[SNAP_TILE][SNAP_TILE + 1];
    __shared__ double btile[SNAP_TILE][SNAP_TILE + 1];
    __shared__ double s[CHUNK_THREADS];
    const TilePos p = tile_pos(nx, ny);
    const double mean = sum[blockIdx.z] / (double(nx) * double(ny));
    const bool act = active[blockIdx.z] != 0;
    double t = 0.0;
    for (int j = 0; j < SNAP_TILE; j += CHUNK_THREADS / SNAP_TILE) {
        const int ix = p.x0 + p.ty + j, iy = p.y0 + p.tx;
        if (ix < nx && iy < ny) {
            const size_t k = p.plane + size_t(ix) * size_t(ny) + size_t(iy);
            double y = x[k];
            const double dv = y - mean;
            t += dv * dv;
            if (pbeam) {
                const double pb = pbeam[k];
                const double den = pb * pb + eta;
                if (act) {
                    y *= pb / den;
                    x[k] = y;
                }
                btile[p.ty + j][p.tx] = den;
            }
            tile[p.ty + j][p.tx] = y;
        }
    }
    __syncthreads();
    store_transposed(tile, p, nx, ny, cube_t);
    if (bw_t) store_transposed(btile, p, nx, ny, bw_t);
    s[threadIdx.x] = t;
    block_tree_sum(s);
    if (threadIdx.x == 0) part[size_t(blockIdx.z) * p.nblk + p.blk] = s[0];
}

static dim3 tile_grid(int64_t ns, int64_t nx, int64_t ny)
{
    return dim3(uint32_t(ceil_div(ny, SNAP_TILE)), uint32_t(ceil_div(nx, SNAP_TILE)), uint32_t(ns));
}

template <class TOut>
static void finish_planes(hipStream_t st, double *residual, double *psf, const double *pbeam, const uint8_t *active, int64_t ns, int64_t nx,
                          int64_t ny, int64_t nxp, int64_t nyp, double eta, const double *pm, TOut *cube_t, TOut *psf_t, TOut *bw_t,
                          double *part, double *sum, double *ssq)
{
    const dim3 gi = tile_grid(ns, nx, ny), gp = tile_grid(ns, nxp, nyp);
    const int nblk = int(gi.x * gi.y);
    hipLaunchKernelGGL(k_norm_tile<TOut>, gp, dim3(CHUNK_THREADS), 0, st, psf, pm, active, int(nxp), int(nyp), psf_t, (double *)nullptr);
    hipLaunchKernelGGL(k_norm_tile<TOut>, gi, dim3(CHUNK_THREADS), 0, st, residual, pm, active, int(nx), int(ny), (TOut *)nullptr, part);
    chunk_partial_final(st, part, nullptr, nblk, 0, int(ns), sum, nullptr);
    hipLaunchKernelGGL(k_rms_beam_tile<TOut>, gi, dim3(CHUNK_THREADS), 0, st, residual, sum, active, pbeam, eta, int(nx), int(ny), cube_t, bw_t, part);
    chunk_partial_final(st, part, nullptr, nblk, 0, int(ns), ssq, nullptr);
    PFB_HIP(hipGetLastError());
}

}  // namespace pfbhip

using namespace pfbhip;

extern "C" {

int pfbhip_chunk_rephase_residual_dev(double *vis_dev, const double *model_dev, const uint8_t *mask_dev, const double *w_diff_dev,
                                      const double *freq_host, int64_t ncorr, int64_t nrow, int64_t nchan)
{
    return guarded([&] {
        PFB_REQUIRE(ncorr >= 1 && ncorr <= 65535 && nrow >= 0 && nchan >= 1 && nchan <= INT32_MAX, "bad arguments");
        PFB_REQUIRE(nrow <= INT64_MAX / nchan / ncorr / 16, "the chunk is too large");
        const int64_t nvis = nrow * nchan;
        PFB_REQUIRE(vis_dev || nvis == 0, "NULL argument");
        PFB_REQUIRE(!model_dev || mask_dev || nvis == 0, "a model needs the mask");
        PFB_REQUIRE(!w_diff_dev || freq_host, "rephasing needs the frequencies");
        if (nvis == 0 || (!w_diff_dev && !model_dev)) return;
        const hipStream_t st = hipStreamPerThread;
        std::vector<double> fc;
        if (w_diff_dev)
            for (int64_t k = 0; k < nchan; ++k) fc.push_back(freq_host[k] / SNAP_SPEED_OF_LIGHT);
        DevBuf<double> d_fc;
        synced(st, [&] {
            const double *fcp = upload(d_fc, w_diff_dev ? fc.data() : nullptr, fc.size(), st);
            hipLaunchKernelGGL(k_rephase_residual, blocks1d(nvis, CHUNK_THREADS), dim3(CHUNK_THREADS), 0, st,
                               reinterpret_cast<double2 *>(vis_dev), reinterpret_cast<const double2 *>(model_dev), mask_dev, w_diff_dev, fcp,
                               int(ncorr), nvis, int(nchan));
            PFB_HIP(hipGetLastError());
        });
    });
}

int pfbhip_chunk_l2_reweight_joint_dev(const double *resvis_dev, const uint8_t *mask_dev, double *wgt_dev, int64_t ncorr, int64_t nvis,
                                       double dof, double *ovar_host)
{
    return guarded([&] {
        PFB_REQUIRE(ncorr >= 1 && ncorr <= 65535 && nvis >= 0, "bad arguments");
        PFB_REQUIRE((resvis_dev && mask_dev && wgt_dev) || nvis == 0, "NULL argument");
        PFB_REQUIRE(dof > 0.0 && std::isfinite(dof), "l2 reweighting: dof = %g must be positive and finite", dof);
        const hipStream_t st = hipStreamPerThread;
        const int nb = chunk_first_stage_blocks(nvis);
        DevBuf<double> part(size_t(ncorr) * size_t(nb)), ssq{size_t(1)};
        DevBuf<unsigned long long> cnt(size_t(nb) + 1);
        double ovar = 0.0;
        unsigned long long nmask = 0;
        const double2 *r = reinterpret_cast<const double2 *>(resvis_dev);
        synced(st, [&] {
            // the per-correlation partials of vischunk.hip, summed by ONE final block: a joint variance
            chunk_ressq_partial(st, r, nullptr, 1.0, mask_dev, ncorr, nvis, nb, part.p, cnt.p);
            chunk_partial_final(st, part.p, cnt.p, int(ncorr) * nb, nb, 1, ssq.p, cnt.p + nb);
            PFB_HIP(hipGetLastError());
            PFB_HIP(hipMemcpyAsync(&ovar, ssq.p, sizeof ovar, hipMemcpyDeviceToHost, st));
            PFB_HIP(hipMemcpyAsync(&nmask, cnt.p + nb, sizeof nmask, hipMemcpyDeviceToHost, st));
            PFB_HIP(hipStreamSynchronize(st));  // the sums decide whether anything is written at all
            PFB_REQUIRE(nmask > 0, "l2 reweighting: the mask is empty");
            ovar /= double(nmask);
            if (ovar_host) *ovar_host = ovar;
            PFB_REQUIRE(ovar > 0.0, "l2 reweighting: residual visibilities are exactly zero");
            hipLaunchKernelGGL(k_l2_reweight_joint, dim3(uint32_t(ceil_div(nvis, CHUNK_THREADS)), uint32_t(ncorr)), dim3(CHUNK_THREADS), 0, st,
                               r, mask_dev, ovar, dof, nvis, wgt_dev);
            PFB_HIP(hipGetLastError());
        });
    });
}

int pfbhip_snapshot_finish_dev(double *residual_dev, double *psf_dev, const double *pbeam_dev, const double *wsum_host, int64_t ns,
                               int64_t nx, int64_t ny, int64_t nxp, int64_t nyp, double eta, int out_f64, void *cube_host, void *psf_host,
                               void *beam_weight_host, double *psf_max_host, double *rms_host, double *device_ms)
{
    return guarded([&] {
        PFB_REQUIRE(residual_dev && psf_dev && wsum_host && cube_host && psf_max_host && rms_host, "NULL argument");
        PFB_REQUIRE(ns >= 1 && ns <= 65535, "ns = %lld is outside [1, 65535]", (long long)ns);
        const int64_t lim = int64_t(65535) * SNAP_TILE;
        PFB_REQUIRE(nx >= 1 && ny >= 1 && nxp >= 1 && nyp >= 1 && nx <= lim && ny <= lim && nxp <= lim && nyp <= lim, "bad plane shape");
        PFB_REQUIRE(!beam_weight_host || pbeam_dev, "beam_weight needs a beam");
        PFB_REQUIRE(eta >= 0.0, "eta = %g must not be negative", eta);
        const hipStream_t st = hipStreamPerThread;
        const size_t n = size_t(nx) * size_t(ny), np = size_t(nxp) * size_t(nyp), esz = out_f64 ? 8 : 4;
        std::vector<uint8_t> active(static_cast<size_t>(ns));
        for (int64_t c = 0; c < ns; ++c) active[size_t(c)] = wsum_host[c] > 0.0;
        const int nbm = chunk_first_stage_blocks(int64_t(np));
        const size_t nblk = size_t(ceil_div(nx, SNAP_TILE)) * size_t(ceil_div(ny, SNAP_TILE));
        PFB_REQUIRE(nblk <= size_t(INT32_MAX), "bad plane shape");
        DevBuf<uint8_t> d_active;
        DevBuf<double> part(size_t(ns) * std::max(nblk, size_t(nbm))), red(size_t(ns) * 3);  // red: psf_max, sum, ssq
        DevBuf<char> cube_t(size_t(ns) * n * esz), psf_t(psf_host ? size_t(ns) * np * esz : 0), bw_t(beam_weight_host ? size_t(ns) * n * esz : 0);
        std::vector<double> pm(static_cast<size_t>(ns)), ssq(static_cast<size_t>(ns));
        EventTimer timer(device_ms != nullptr);  // the kernels alone: after the upload of `active`, before the downloads
        synced(st, [&] {
            const uint8_t *act = upload(d_active, active.data(), active.size(), st);
            double *pmd = red.p, *sumd = red.p + ns, *ssqd = red.p + 2 * ns;
            timer.start(st);
            hipLaunchKernelGGL(k_max_partial, dim3(uint32_t(nbm), uint32_t(ns)), dim3(CHUNK_THREADS), 0, st, psf_dev, int64_t(np), part.p);
            hipLaunchKernelGGL(k_max_final, dim3(uint32_t(ns)), dim3(CHUNK_THREADS), 0, st, part.p, nbm, pmd);
            if (out_f64)
                finish_planes<double>(st, residual_dev, psf_dev, pbeam_dev, act, ns, nx, ny, nxp, nyp, eta, pmd, (double *)cube_t.p,
                                      (double *)psf_t.p, (double *)bw_t.p, part.p, sumd, ssqd);
            else
                finish_planes<float>(st, residual_dev, psf_dev, pbeam_dev, act, ns, nx, ny, nxp, nyp, eta, pmd, (float *)cube_t.p,
                                     (float *)psf_t.p, (float *)bw_t.p, part.p, sumd, ssqd);
            timer.stop(st);
            PFB_HIP(hipMemcpyAsync(cube_host, cube_t.p, cube_t.bytes(), hipMemcpyDeviceToHost, st));
            if (psf_host) PFB_HIP(hipMemcpyAsync(psf_host, psf_t.p, psf_t.bytes(), hipMemcpyDeviceToHost, st));
            if (beam_weight_host) PFB_HIP(hipMemcpyAsync(beam_weight_host, bw_t.p, bw_t.bytes(), hipMemcpyDeviceToHost, st));
            PFB_HIP(hipMemcpyAsync(pm.data(), pmd, size_t(ns) * sizeof(double), hipMemcpyDeviceToHost, st));
            PFB_HIP(hipMemcpyAsync(ssq.data(), ssqd, size_t(ns) * sizeof(double), hipMemcpyDeviceToHost, st));
        });
        if (device_ms) *device_ms = timer.ms();
        for (int64_t c = 0; c < ns; ++c) {
            psf_max_host[c] = active[size_t(c)] ? pm[size_t(c)] : 0.0;
            rms_host[c] = active[size_t(c)] ? std::sqrt(ssq[size_t(c)] / double(n)) : 0.0;
        }
    });
}

}  // extern "C"
