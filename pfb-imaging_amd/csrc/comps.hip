// comps.hip -- the component model (pixel locations + coefficients of a time / frequency parametrisation) on the device.
//
// Mirrors utils/modelspec.py of pfb-imaging: fit_image_cube (:12-137: support mask, np.where compaction, the linear fit),
// the render of eval_coeffs_to_cube / eval_coeffs_to_slice (:223-275: image[x_index, y_index] = modelf(t, f, *coeffs), which
// for the parametrisations the reference writes is basis(t, f) . coeffs) and the bilinear regrid of eval_coeffs_to_slice
// (:277-332).  Everything is f64 and memory-bound; no product is contracted with a sum (the Makefile's -ffp-contract=off
// holds here: the regrid's grid coordinates have to round as numpy's do).
//
// Compaction order: component c is the c-th set pixel in ascending flat index x * ny + y, exactly np.where's order -- the
// coefficients are indexed by it.  Each workgroup owns CP_TILE consecutive pixels; it counts its set pixels, the host adds
// the counts up in workgroup order, and a second launch writes every set pixel at (workgroup offset + its rank inside the
// workgroup).  No atomic cursor anywhere.
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

constexpr int CP_THREADS = 256;
constexpr int CP_ITEMS = 4;                       // pixels per thread: pixel = tile base + item * 256 + thread
constexpr int CP_TILE = CP_THREADS * CP_ITEMS;    // pixels per workgroup
constexpr int CP_SLOTS = CP_ITEMS * (CP_THREADS / 64);  // (item, wave) pairs of a workgroup, in pixel order
constexpr int FIT_K = 8;                          // coefficients a thread accumulates per pass over the sample planes

// mask[p] = any_s(cube[s, p] != 0) (np.any: NaN counts, -0.0 does not), counts[workgroup] = set pixels of its tile
__global__ void __launch_bounds__(CP_THREADS) k_comps_mask(const double *__restrict__ cube, int ns, int64_t npix,
                                                           uint8_t *__restrict__ mask, int32_t *__restrict__ counts)
{
    __shared__ int32_t sm[CP_SLOTS];
    const int64_t base = int64_t(blockIdx.x) * CP_TILE;
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < CP_ITEMS; ++j) {
        const int64_t p = base + j * CP_THREADS + threadIdx.x;
        bool set = false;
        if (p < npix) {
            for (int s = 0; s < ns; ++s) set |= cube[size_t(s) * size_t(npix) + size_t(p)] != 0.0;
            mask[p] = set ? 1 : 0;
        }
        const unsigned long long b = __ballot(set);
        if ((threadIdx.x & 63) == 0) sm[j * (CP_THREADS / 64) + wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t n = 0;
        for (int i = 0; i < CP_SLOTS; ++i) n += sm[i];
        counts[blockIdx.x] = n;
    }
}

// ordered write: the set pixel p of workgroup w lands at offsets[w] + (set pixels of the tile below p)
__global__ void __launch_bounds__(CP_THREADS) k_comps_compact(const uint8_t *__restrict__ mask, int64_t npix, int64_t ny,
                                                              const int64_t *__restrict__ offsets, int64_t ncomps,
                                                              int64_t *__restrict__ xi, int64_t *__restrict__ yi,
                                                              int64_t *__restrict__ pix)
{
    __shared__ int32_t sm[CP_SLOTS];
    const int64_t base = int64_t(blockIdx.x) * CP_TILE;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long bal[CP_ITEMS];
#pragma unroll
    for (int j = 0; j < CP_ITEMS; ++j) {
        const int64_t p = base + j * CP_THREADS + threadIdx.x;
        bal[j] = __ballot(p < npix && mask[p] != 0);
        if (lane == 0) sm[j * (CP_THREADS / 64) + wave] = __popcll(bal[j]);
    }
    __syncthreads();
    const int64_t off = offsets[blockIdx.x];
#pragma unroll
    for (int j = 0; j < CP_ITEMS; ++j) {
        if (!((bal[j] >> lane) & 1ull)) continue;
        int32_t before = 0;
        for (int i = 0; i < j * (CP_THREADS / 64) + wave; ++i) before += sm[i];
        const int64_t r = off + before + __popcll(bal[j] & ((1ull << lane) - 1ull));
        if (r < ncomps) {  // (always: the offsets are the prefix sums of these very counts)
            const int64_t p = base + j * CP_THREADS + threadIdx.x;
            xi[r] = p / ny;
            yi[r] = p % ny;
            pix[r] = p;
        }
    }
}

// coeffs[k, c] = sum_s A[k, s] * cube[s, pix[c]], s ascending; one thread per component, FIT_K coefficients per pass (one
// pass, each plane gathered once, for nparam <= FIT_K)
__global__ void __launch_bounds__(CP_THREADS) k_comps_fit(const double *__restrict__ cube, int ns, int64_t npix,
                                                          const int64_t *__restrict__ pix, int64_t ncomps,
                                                          const double *__restrict__ A, int nparam, double *__restrict__ coeffs)
{
    const int64_t c = int64_t(blockIdx.x) * CP_THREADS + threadIdx.x;
    if (c >= ncomps) return;
    const size_t p = size_t(pix[c]);
    for (int k0 = 0; k0 < nparam; k0 += FIT_K) {
        double acc[FIT_K];
#pragma unroll
        for (int kk = 0; kk < FIT_K; ++kk) acc[kk] = 0.0;
        for (int s = 0; s < ns; ++s) {
            const double v = cube[size_t(s) * size_t(npix) + p];
#pragma unroll
            for (int kk = 0; kk < FIT_K; ++kk)
                if (k0 + kk < nparam) acc[kk] += A[size_t(k0 + kk) * size_t(ns) + size_t(s)] * v;
        }
#pragma unroll
        for (int kk = 0; kk < FIT_K; ++kk)
            if (k0 + kk < nparam) coeffs[size_t(k0 + kk) * size_t(ncomps) + size_t(c)] = acc[kk];
    }
}

// out[pix[c]] = sum_k b[k] * coeffs[k, c] (k ascending), or 0 where the region mask is unset; `out` was cleared on the stream
__global__ void __launch_bounds__(CP_THREADS) k_comps_scatter(const int64_t *__restrict__ pix, int64_t ncomps,
                                                              const double *__restrict__ coeffs, const double *__restrict__ b,
                                                              int nparam, const uint8_t *__restrict__ region,
                                                              double *__restrict__ out)
{
    const int64_t c = int64_t(blockIdx.x) * CP_THREADS + threadIdx.x;
    if (c >= ncomps) return;
    const int64_t p = pix[c];
    double v = 0.0;
    for (int k = 0; k < nparam; ++k) v += b[k] * coeffs[size_t(k) * size_t(ncomps) + size_t(c)];
    if (region && !region[p]) v = 0.0;
    out[p] = v;
}

// The regrid of eval_coeffs_to_slice (modelspec.py:277-332).  The input grid is the reference's zero-padded one: its node i
// (0 <= i < n + lo + hi) sits at (i - (n / 2 + lo)) * cell + x0 and holds in[i - lo], or 0 outside [0, n).
struct RegridAxis {
    int64_t n, lo, np;  // input size, pad below, padded size
    int64_t half_in, half_out;
    double cell_in, x0_in, cell_out, x0_out;
};
__device__ __forceinline__ double rg_node(const RegridAxis &a, int64_t i) { return double(i - a.half_in) * a.cell_in + a.x0_in; }
// scipy's find_indices: i with node(i) <= x < node(i + 1), clipped to [0, np - 2]; t = (x - node(i)) / (node(i + 1) - node(i))
__device__ __forceinline__ void rg_locate(const RegridAxis &a, int64_t o, int64_t &i, double &t)
{
    const double x = double(o - a.half_out) * a.cell_out + a.x0_out;
    double g = floor((x - rg_node(a, 0)) / a.cell_in);
    g = fmin(fmax(g, 0.0), double(a.np - 2));
    i = int64_t(g);
    for (int it = 0; it < 4 && i > 0 && x < rg_node(a, i); ++it) --i;             // (the estimate is off by one at most)
    for (int it = 0; it < 4 && i < a.np - 2 && x >= rg_node(a, i + 1); ++it) ++i;
    const double lo = rg_node(a, i);
    t = (x - lo) / (rg_node(a, i + 1) - lo);
}
__device__ __forceinline__ double rg_read(const double *__restrict__ in, const RegridAxis &ax, const RegridAxis &ay, int64_t i,
                                          int64_t j)
{
    i -= ax.lo;
    j -= ay.lo;
    return (i >= 0 && i < ax.n && j >= 0 && j < ay.n) ? in[size_t(i) * size_t(ay.n) + size_t(j)] : 0.0;
}
__global__ void __launch_bounds__(CP_THREADS) k_comps_regrid(const double *__restrict__ in, RegridAxis ax, RegridAxis ay, int64_t nxo,
                                                             int64_t nyo, int interp, double area_ratio, double *__restrict__ out)
{
    const int64_t o = int64_t(blockIdx.x) * CP_THREADS + threadIdx.x;
    if (o >= nxo * nyo) return;
    const int64_t ox = o / nyo, oy = o % nyo;
    if (!interp) {  // the reference returns its (padded) input as it stands: no area ratio
        out[o] = rg_read(in, ax, ay, ox, oy);
        return;
    }
    int64_t i, j;
    double tx, ty;
    rg_locate(ax, ox, i, tx);
    rg_locate(ay, oy, j, ty);
    double v = rg_read(in, ax, ay, i, j) * ((1.0 - tx) * (1.0 - ty));
    v += rg_read(in, ax, ay, i, j + 1) * ((1.0 - tx) * ty);
    v += rg_read(in, ax, ay, i + 1, j) * (tx * (1.0 - ty));
    v += rg_read(in, ax, ay, i + 1, j + 1) * (tx * ty);
    out[o] = v * area_ratio;
}

// one axis of the reference's padding arithmetic (modelspec.py:281-319), in the same order of operations
static RegridAxis regrid_axis(int64_t ni, double celli, double x0i, int64_t no, double cello, double x0o)
{
    const double in_min = double(-(ni / 2)) * celli + x0i, in_max = double(-(ni / 2) + ni - 1) * celli + x0i;
    const double out_min = double(-(no / 2)) * cello + x0o, out_max = double(-(no / 2) + no - 1) * cello + x0o;
    const double ldiff = in_min - out_min, udiff = out_max - in_max;
    const int64_t lo = ldiff > 0.0 ? int64_t(std::ceil(ldiff / celli)) : 0;
    const int64_t hi = udiff > 0.0 ? int64_t(std::ceil(udiff / celli)) : 0;
    RegridAxis a;
    a.n = ni;
    a.lo = lo;
    a.np = ni + lo + hi;
    a.half_in = ni / 2 + lo;
    a.half_out = no / 2;
    a.cell_in = celli;
    a.x0_in = x0i;
    a.cell_out = cello;
    a.x0_out = x0o;
    return a;
}

static void regrid_async(hipStream_t st, const double *in_dev, int64_t nxi, int64_t nyi, double cellxi, double cellyi, double x0i,
                         double y0i, int64_t nxo, int64_t nyo, double cellxo, double cellyo, double x0o, double y0o, double *out_dev,
                         int *interpolated)
{
    PFB_REQUIRE(nxi >= 1 && nyi >= 1 && nxo >= 1 && nyo >= 1, "image sizes must be positive");
    PFB_REQUIRE(cellxi > 0.0 && cellyi > 0.0 && cellxo > 0.0 && cellyo > 0.0, "cell sizes must be positive");
    PFB_REQUIRE(std::isfinite(x0i) && std::isfinite(y0i) && std::isfinite(x0o) && std::isfinite(y0o), "centres must be finite");
    const RegridAxis ax = regrid_axis(nxi, cellxi, x0i, nxo, cellxo, x0o), ay = regrid_axis(nyi, cellyi, y0i, nyo, cellyo, y0o);
    const bool interp = cellxi != cellxo || cellyi != cellyo || x0i != x0o || y0i != y0o || ax.np != nxo || ay.np != nyo;
    if (interp) {
        PFB_REQUIRE(ax.np >= 2 && ay.np >= 2, "interpolation needs at least two input pixels per axis");
        // RegularGridInterpolator(bounds_error=True): the padded grid has to cover the output grid
        auto outside = [](const RegridAxis &a, int64_t no) {
            const double lo = double(-a.half_in) * a.cell_in + a.x0_in, hi = double(a.np - 1 - a.half_in) * a.cell_in + a.x0_in;
            const double omin = double(-a.half_out) * a.cell_out + a.x0_out, omax = double(no - 1 - a.half_out) * a.cell_out + a.x0_out;
            return omin < lo || omax > hi;
        };
        PFB_REQUIRE(!outside(ax, nxo) && !outside(ay, nyo), "one of the requested output points is out of bounds of the padded input grid");
    }
    const double area_ratio = (cellxo * cellyo) / (cellxi * cellyi);
    hipLaunchKernelGGL(k_comps_regrid, blocks1d(nxo * nyo, CP_THREADS), dim3(CP_THREADS), 0, st, in_dev, ax, ay, nxo, nyo, int(interp), area_ratio,
                       out_dev);
    PFB_HIP(hipGetLastError());
    if (interpolated) *interpolated = interp ? 1 : 0;
}

}  // namespace pfbhip

using namespace pfbhip;

namespace {

void render_async(pfbhip_comps *h, const double *basis_host, int use_region, double *image_dev)
{
    PFB_REQUIRE(!use_region || h->has_region, "no region mask bound: call pfbhip_comps_set_region first");
    for (int k = 0; k < h->nparam; ++k) PFB_REQUIRE(std::isfinite(basis_host[k]), "basis[%d] is not finite", k);
    const hipStream_t st = h->stream();
    PFB_HIP(hipMemcpyAsync(h->basis.p, basis_host, size_t(h->nparam) * sizeof(double), hipMemcpyHostToDevice, st));
    PFB_HIP(hipMemsetAsync(image_dev, 0, size_t(h->nx) * size_t(h->ny) * sizeof(double), st));
    if (h->ncomps)
        hipLaunchKernelGGL(k_comps_scatter, blocks1d(h->ncomps, CP_THREADS), dim3(CP_THREADS), 0, st, h->pix.p, h->ncomps, h->coeffs.p, h->basis.p,
                           h->nparam, use_region ? h->region.p : nullptr, image_dev);
    PFB_HIP(hipGetLastError());
}

// a handle with its arrays allocated (one element where there are no components) and nothing in them
std::unique_ptr<pfbhip_comps> make_comps(int64_t nx, int64_t ny, int64_t ncomps, int32_t nparam)
{
    auto h = std::make_unique<pfbhip_comps>();
    h->nx = nx, h->ny = ny, h->ncomps = ncomps, h->nparam = nparam;
    const size_t n = size_t(std::max<int64_t>(ncomps, 1));
    h->xi.alloc(n), h->yi.alloc(n), h->pix.alloc(n);
    h->coeffs.alloc(n * size_t(nparam));
    h->basis.alloc(size_t(nparam));
    return h;
}

}  // namespace

extern "C" {

int pfbhip_comps_create(int64_t nx, int64_t ny, int64_t ncomps, int32_t nparam, const int64_t *x_index_host,
                        const int64_t *y_index_host, const double *coeffs_host, pfbhip_comps **out)
{
    return guarded([&] {
        PFB_REQUIRE(out, "NULL argument");
        *out = nullptr;
        PFB_REQUIRE(nx >= 1 && ny >= 1 && ncomps >= 0 && nparam >= 1, "bad sizes");
        PFB_REQUIRE(ncomps == 0 || (x_index_host && y_index_host && coeffs_host), "NULL argument");
        std::vector<int64_t> flat(size_t(ncomps), 0);
        for (int64_t c = 0; c < ncomps; ++c) {  // (the scatter writes where these say: nothing out of the image)
            const int64_t x = x_index_host[c], y = y_index_host[c];
            PFB_REQUIRE(x >= 0 && x < nx && y >= 0 && y < ny, "component %lld at (%lld, %lld) is outside the %lld x %lld image",
                        (long long)c, (long long)x, (long long)y, (long long)nx, (long long)ny);
            flat[size_t(c)] = x * ny + y;
        }
        {  // two components on one pixel would race in the scatter (numpy's assignment lets the last one win): refused
            std::vector<int64_t> sorted(flat);
            std::sort(sorted.begin(), sorted.end());
            const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
            PFB_REQUIRE(dup == sorted.end(), "two components share the pixel (%lld, %lld): locations must be distinct",
                        dup == sorted.end() ? 0LL : (long long)(*dup / ny), dup == sorted.end() ? 0LL : (long long)(*dup % ny));
        }
        auto h = make_comps(nx, ny, ncomps, nparam);
        const hipStream_t st = h->stream();
        synced(st, [&] {
            const size_t n = size_t(ncomps);
            upload(h->xi, x_index_host, n, st);
            upload(h->yi, y_index_host, n, st);
            upload(h->pix, flat.data(), n, st);
            upload(h->coeffs, coeffs_host, n * size_t(nparam), st);
        });
        *out = h.release();
    });
}

int pfbhip_comps_destroy(pfbhip_comps *h)
{
    return guarded([&] {
        if (h) (void)hipStreamSynchronize(h->stream());
        delete h;
    });
}

int pfbhip_comps_fit(const double *cube_host, const double *cube_dev, int64_t ns, int64_t nx, int64_t ny, const double *A_host,
                     int32_t nparam, pfbhip_comps **out, int64_t *ncomps_out)
{
    return guarded([&] {
        PFB_REQUIRE(out && ncomps_out && A_host, "NULL argument");
        *out = nullptr;
        PFB_REQUIRE((cube_host != nullptr) != (cube_dev != nullptr), "pass the cube either as a host or as a device array");
        PFB_REQUIRE(ns >= 1 && ns < (int64_t(1) << 31) && nx >= 1 && ny >= 1 && nparam >= 1, "bad sizes");
        for (int64_t i = 0; i < int64_t(nparam) * ns; ++i) PFB_REQUIRE(std::isfinite(A_host[i]), "the fit matrix is not finite");
        const int64_t npix = nx * ny, ntiles = ceil_div(npix, CP_TILE);
        PFB_REQUIRE(ntiles < (int64_t(1) << 31), "image too large");
        const hipStream_t st = hipStreamPerThread;
        DevBuf<double> cube, A;
        DevBuf<uint8_t> mask{size_t(npix)};
        DevBuf<int32_t> counts{size_t(ntiles)};
        DevBuf<int64_t> offsets{size_t(ntiles)};
        std::vector<int32_t> hc(static_cast<size_t>(ntiles));
        std::vector<int64_t> ho(static_cast<size_t>(ntiles));
        std::unique_ptr<pfbhip_comps> h;
        int64_t ncomps = 0;
        synced(st, [&] {  // (the temporaries above die after the kernels that use them)
            if (cube_host) cube_dev = upload(cube, cube_host, size_t(ns) * size_t(npix), st);
            upload(A, A_host, size_t(nparam) * size_t(ns), st);
            hipLaunchKernelGGL(k_comps_mask, dim3(uint32_t(ntiles)), dim3(CP_THREADS), 0, st, cube_dev, int(ns), npix, mask.p, counts.p);
            PFB_HIP(hipGetLastError());
            PFB_HIP(hipMemcpyAsync(hc.data(), counts.p, counts.bytes(), hipMemcpyDeviceToHost, st));
            PFB_HIP(hipStreamSynchronize(st));
            for (int64_t w = 0; w < ntiles; ++w) {  // the scan, in workgroup order
                ho[size_t(w)] = ncomps;
                ncomps += hc[size_t(w)];
            }
            h = make_comps(nx, ny, ncomps, nparam);
            if (ncomps) {
                PFB_HIP(hipMemcpyAsync(offsets.p, ho.data(), offsets.bytes(), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_comps_compact, dim3(uint32_t(ntiles)), dim3(CP_THREADS), 0, st, mask.p, npix, ny, offsets.p, ncomps,
                                   h->xi.p, h->yi.p, h->pix.p);
                hipLaunchKernelGGL(k_comps_fit, blocks1d(ncomps, CP_THREADS), dim3(CP_THREADS), 0, st, cube_dev, int(ns), npix, h->pix.p, ncomps, A.p,
                                   int(nparam), h->coeffs.p);
                PFB_HIP(hipGetLastError());
            }
        });
        *out = h.release();
        *ncomps_out = ncomps;
    });
}

int pfbhip_comps_shape(const pfbhip_comps *h, int64_t *nx, int64_t *ny, int64_t *ncomps, int32_t *nparam)
{
    return guarded([&] {
        PFB_REQUIRE(h, "NULL handle");
        if (nx) *nx = h->nx;
        if (ny) *ny = h->ny;
        if (ncomps) *ncomps = h->ncomps;
        if (nparam) *nparam = h->nparam;
    });
}

int pfbhip_comps_get(pfbhip_comps *h, int64_t *x_index_host, int64_t *y_index_host, double *coeffs_host)
{
    return guarded([&] {
        PFB_REQUIRE(h, "NULL handle");
        const hipStream_t st = h->stream();
        const size_t n = size_t(h->ncomps);
        synced(st, [&] {
            if (n && x_index_host) PFB_HIP(hipMemcpyAsync(x_index_host, h->xi.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            if (n && y_index_host) PFB_HIP(hipMemcpyAsync(y_index_host, h->yi.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            if (n && coeffs_host)
                PFB_HIP(hipMemcpyAsync(coeffs_host, h->coeffs.p, n * size_t(h->nparam) * sizeof(double), hipMemcpyDeviceToHost, st));
        });
    });
}

int pfbhip_comps_set_region(pfbhip_comps *h, const uint8_t *region_host)
{
    return guarded([&] {
        PFB_REQUIRE(h, "NULL handle");
        h->has_region = false;
        if (!region_host) return;
        const size_t npix = size_t(h->nx) * size_t(h->ny);
        synced(h->stream(), [&] { upload(h->region, region_host, npix, h->stream()); });
        h->has_region = true;
    });
}

int pfbhip_comps_render_dev(pfbhip_comps *h, const double *basis_host, int use_region, double *image_dev)
{
    return guarded([&] {
        PFB_REQUIRE(h && basis_host && image_dev, "NULL argument");
        synced(h->stream(), [&] { render_async(h, basis_host, use_region, image_dev); });
    });
}

int pfbhip_comps_render(pfbhip_comps *h, const double *basis_host, int use_region, double *image_host)
{
    return guarded([&] {
        PFB_REQUIRE(h && basis_host && image_host, "NULL argument");
        const size_t npix = size_t(h->nx) * size_t(h->ny);
        synced(h->stream(), [&] {
            h->image.ensure(npix);
            render_async(h, basis_host, use_region, h->image.p);
            PFB_HIP(hipMemcpyAsync(image_host, h->image.p, npix * sizeof(double), hipMemcpyDeviceToHost, h->stream()));
        });
    });
}

int pfbhip_comps_regrid_dev(const double *in_dev, int64_t nxi, int64_t nyi, double cellxi, double cellyi, double x0i, double y0i,
                            int64_t nxo, int64_t nyo, double cellxo, double cellyo, double x0o, double y0o, double *out_dev,
                            int *interpolated)
{
    return guarded([&] {
        PFB_REQUIRE(in_dev && out_dev && in_dev != out_dev, "NULL or aliased argument");
        synced(hipStreamPerThread, [&] {
            regrid_async(hipStreamPerThread, in_dev, nxi, nyi, cellxi, cellyi, x0i, y0i, nxo, nyo, cellxo, cellyo, x0o, y0o, out_dev,
                         interpolated);
        });
    });
}

int pfbhip_comps_regrid(const double *in_host, int64_t nxi, int64_t nyi, double cellxi, double cellyi, double x0i, double y0i,
                        int64_t nxo, int64_t nyo, double cellxo, double cellyo, double x0o, double y0o, double *out_host,
                        int *interpolated)
{
    return guarded([&] {
        PFB_REQUIRE(in_host && out_host, "NULL argument");
        PFB_REQUIRE(nxi >= 1 && nyi >= 1 && nxo >= 1 && nyo >= 1, "image sizes must be positive");
        const hipStream_t st = hipStreamPerThread;
        DevBuf<double> in{size_t(nxi) * size_t(nyi)}, out{size_t(nxo) * size_t(nyo)};
        synced(st, [&] {
            PFB_HIP(hipMemcpyAsync(in.p, in_host, in.bytes(), hipMemcpyHostToDevice, st));
            regrid_async(st, in.p, nxi, nyi, cellxi, cellyi, x0i, y0i, nxo, nyo, cellxo, cellyo, x0o, y0o, out.p, interpolated);
            PFB_HIP(hipMemcpyAsync(out_host, out.p, out.bytes(), hipMemcpyDeviceToHost, st));
        });
    });
}

}  // extern "C"
