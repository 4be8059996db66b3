// gridder.hip -- w-stacking gridder / degridder / exact Hessian on MI355X.
//
// Replaces ducc0.wgridder.experimental.vis2dirty / dirty2vis as called by the reference at
// /root/reference/src/pfb_imaging/operators/hessian.py:50-89 and
// /root/reference/src/pfb_imaging/operators/gridder.py:78,128,590-613,972-1016.
//
// Algorithm (published method: Arras et al. 2021, A&A 646 A58; ES kernel of Barnett et al. 2019):
//   vis2dirty: weight + phase-shift + Hermitian-fold the visibilities into tile-sorted order;
//              per w-plane: scatter with phi(u)phi(v)phi(w) (k_grid_mp) -> backward 2-D FFT as two pruned row
//              passes (rowfft.hpp; rocFFT row plans for sizes it does not take) -> crop, multiply by the
//              w-screen exp(-2 pi i w_p (n-1+nshift)), accumulate Re (fused into the second row pass);
//              finally multiply by the correction image 1/(psi_l psi_m psi_n) [/n].
//   dirty2vis: the exact adjoint, backwards.
//   hessian:   dirty2vis then vis2dirty with the model visibilities kept on the device in
//              tile-sorted order (no un-permute, no phase shift: they cancel).
//
// Compiled with -ffp-contract=off (see vismap.hpp: bit-exact index map).
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <string>
#include <cstring>
#include <memory>
#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"
#include "devcg.hpp"
#include "dispatch.hpp"
#include "eskernel.hpp"
#include "gridder_kernels_mp.hpp"
#include "gridder_wd_api.hpp"
#include "plan_layout.hpp"
#include "rowfft_api.hpp"
#include "vismap.hpp"

namespace pfbhip {

constexpr double SPEED_OF_LIGHT = 299792458.0;
constexpr double pi_const = 3.14159265358979323846;

#define PFB_ROCFFT(expr)                                                                              \
    do {                                                                                              \
        rocfft_status _s = (expr);                                                                    \
        if (_s != rocfft_status_success)                                                              \
            throw std::runtime_error(pfbhip::strprintf("%s failed: rocfft status %d (%s:%d)", #expr, \
                                                       int(_s), __FILE__, __LINE__));                 \
    } while (0)

void rocfft_setup_once();

// ---------------------------------------------------------------------------------------
// small kernels
// ---------------------------------------------------------------------------------------

__device__ __forceinline__ double nm1_of(double l, double m)
{
    double r2 = l * l + m * m;
    if (r2 <= 1.0) return -r2 / (1.0 + sqrt(1.0 - r2));
    return -sqrt(r2 - 1.0) - 1.0;
}

struct ImgGeom {
    int nx, ny, nu, nv;
    int bpitch;  // complex elements between consecutive rows of B
    int apitch;  // ... of the uv-plane buffer A
    double px, py, lshift, mshift, nshift;
};

__device__ __forceinline__ double pixel_t(const ImgGeom &g, int ix, int iy)
{
    double l = g.lshift + double(ix - g.nx / 2) * g.px;
    double m = g.mshift + double(iy - g.ny / 2) * g.py;
    return nm1_of(l, m) + g.nshift;
}

// min/max of w (>= 0 after the fold) over unmasked visibilities: one (min,max) pair per block
__global__ void k_wrange(MapArgs m, double *out)
{
    __shared__ double smin[256], smax[256];
    double lo = 1e300, hi = -1e300;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < m.nvis; i += int64_t(gridDim.x) * blockDim.x) {
        if (m.mask && !m.mask[i]) continue;
        int64_t row = i / m.nchan;
        int chan = int(i - row * m.nchan);
        double w = fabs(m.uvw[3 * row + 2] * m.sw * m.fc[chan]);
        lo = fmin(lo, w);
        hi = fmax(hi, w);
    }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + s]);
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = smin[0];
        out[2 * blockIdx.x + 1] = smax[0];
    }
}

__global__ void k_keys(MapArgs m, uint32_t *keys, uint32_t *idx)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i >= m.nvis) return;
    idx[i] = uint32_t(i);
    if (m.mask && !m.mask[i]) {
        keys[i] = 0xFFFFFFFFu;
        return;
    }
    VisPos p = vis_position(m, i);
    uint32_t key = tile_of(m, p.iu0, p.iv0);
    if (m.key_planes > 1) key = key * uint32_t(m.key_planes) + uint32_t(min(max(p.p0, 0), m.key_planes - 1));
    if (m.key_sub > 1) {
        const uint32_t lu = uint32_t(wrap_index(p.iu0, m.nu)) % TILE, lv = uint32_t(wrap_index(p.iv0, m.nv)) % TILE;
        key = key * 64u + (lu >> 2) * 8u + (lv >> 2);
        // 256: the 2 x 2-cell block inside the 4 x 4 one as well (4 x 4 runs stay contiguous: every block kernel can walk this order)
        if (m.key_sub == 256) key = key * 4u + ((lu >> 1) & 1u) * 2u + ((lv >> 1) & 1u);
    }
    keys[i] = key;
}

// tstart[t] = first sorted position whose key >= t * sub  (t = 0..ntiles); tstart[ntiles] = nactive
__global__ void k_tile_start(const uint32_t *keys, int64_t n, uint32_t ntiles, uint32_t sub, uint32_t *tstart)
{
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > ntiles) return;
    const uint64_t bound = uint64_t(t) * sub;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (uint64_t(keys[mid]) < bound) lo = mid + 1;
        else hi = mid;
    }
    tstart[t] = uint32_t(lo);
}

__global__ void k_records(MapArgs m, const uint32_t *sorted_idx, int64_t nactive, double *pu, double *pv, double *pw,
                          uint32_t *src)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (j >= nactive) return;
    uint32_t i = sorted_idx[j];
    VisPos p = vis_position(m, i);
    pu[j] = p.pu;
    pv[j] = p.pv;
    pw[j] = p.pw;
    src[j] = i | (uint32_t(p.flip) << 31);
}

__global__ void k_binmap(MapArgs m, int32_t *iu0, int32_t *iv0, int32_t *p0, uint8_t *flip)
{
    int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i >= m.nvis) return;
    VisPos p = vis_position(m, i);
    iu0[i] = p.iu0;
    iv0[i] = p.iv0;
    p0[i] = p.p0;
    flip[i] = uint8_t(p.flip);
}

// exp(sign * 2 pi i (u lshift + v mshift + w nshift)) for sorted visibility j
__device__ __forceinline__ void shift_phase(const MapArgs &m, uint32_t i, double ls, double ms, double ns, double *c,
                                            double *s)
{
    VisPos p = vis_position(m, i);
    double ph = p.u * ls + p.v * ms + p.w * ns;
    ph -= rint(ph);
    sincospi(2.0 * ph, s, c);
}

// sval[j] = vis[src] * wgt[src] (conj if folded) * exp(+2 pi i shift phase)
__global__ void k_permute_in(MapArgs m, const uint32_t *src, int64_t nactive, const double2 *vis, const double *wgt,
                             int shifting, double ls, double ms, double ns, double2 *sval)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (j >= nactive) return;
    uint32_t s = src[j];
    uint32_t i = s & 0x7FFFFFFFu;
    double2 v = vis[i];
    if (wgt) {
        double w = wgt[i];
        v.x *= w;
        v.y *= w;
    }
    if (s >> 31) v.y = -v.y;
    if (shifting) {
        double c, sn;
        shift_phase(m, i, ls, ms, ns, &c, &sn);
        double re = v.x * c - v.y * sn, im = v.x * sn + v.y * c;
        v.x = re;
        v.y = im;
    }
    sval[j] = v;
}

// vis[src] = sacc[j] * exp(-2 pi i shift phase) (conj if folded) * wgt[src]
__global__ void k_permute_out(MapArgs m, const uint32_t *src, int64_t nactive, const double2 *sacc, const double *wgt,
                              int shifting, double ls, double ms, double ns, double2 *vis)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (j >= nactive) return;
    uint32_t s = src[j];
    uint32_t i = s & 0x7FFFFFFFu;
    double2 v = sacc[j];
    if (shifting) {
        double c, sn;
        shift_phase(m, i, ls, ms, ns, &c, &sn);
        double re = v.x * c + v.y * sn, im = -v.x * sn + v.y * c;
        v.x = re;
        v.y = im;
    }
    if (s >> 31) v.y = -v.y;
    if (wgt) {
        double w = wgt[i];
        v.x *= w;
        v.y *= w;
    }
    vis[i] = v;
}

// k_permute_in whose visibilities are the PSF's, generated here: sval[j] = wgt[src] * exp(2 pi i (+-ramp + shift phase)), where
// ramp = (u x0 + v y0 - w (n0 - 1)) freq / c in the caller's unflipped uvw (operators/gridder.py::psf_visibilities; `ramp` is 0
// at the phase centre, where they are ones) and the sign is that of the Hermitian fold.  The ramp does NOT cancel against
// shift_phase: flip_u / flip_v enter shift_phase twice (u and lshift both carry the sign), so its u and v terms are
// +(u x0 + v y0) as well and the two add; the w terms, -w (n0 - 1) and +w nshift, have the same sign too.  Both phases
// go through one reduction and one sincospi.
__global__ void k_permute_in_psf(MapArgs m, const uint32_t *src, int64_t nactive, const double *wgt, int ramp, double x0, double y0,
                                 double nm1, int shifting, double ls, double ms, double ns, double2 *sval)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (j >= nactive) return;
    uint32_t s = src[j];
    uint32_t i = s & 0x7FFFFFFFu;
    double ph = 0.0;
    if (ramp) {
        int64_t row = i / uint32_t(m.nchan);
        int chan = int(i - row * m.nchan);
        ph = (m.uvw[3 * row] * x0 + m.uvw[3 * row + 1] * y0 - m.uvw[3 * row + 2] * nm1) * m.fc[chan];
        if (s >> 31) ph = -ph;
    }
    if (shifting) {
        VisPos p = vis_position(m, i);
        ph += p.u * ls + p.v * ms + p.w * ns;
    }
    double2 v = make_double2(wgt ? wgt[i] : 1.0, 0.0);
    if (ramp || shifting) {
        double c, sn;
        ph -= rint(ph);
        sincospi(2.0 * ph, &sn, &c);
        v.y = v.x * sn;
        v.x = v.x * c;
    }
    sval[j] = v;
}

// k_permute_out into a row-ordered device array that is written exactly once per sample, in one pass over
// max(nactive, nvis) threads: thread t < nactive un-sorts visibility t (vis[src] = R dirty, or minuend[src] - R dirty), thread
// t < nvis settles sample t when the mask drops it (0, or minuend[t]).  The two sets of samples are disjoint -- the sort
// keeps exactly the samples with mask != 0 -- and every sample is read and written by one thread, so vis may be minuend.
__global__ void k_permute_out_rows(MapArgs m, const uint32_t *src, int64_t nactive, const double2 *sacc, const double2 *minuend,
                                   int shifting, double ls, double ms, double ns, double2 *vis)
{
    int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (t < m.nvis && m.mask && !m.mask[t]) vis[t] = minuend ? minuend[t] : make_double2(0.0, 0.0);
    if (t >= nactive) return;
    uint32_t s = src[t];
    uint32_t i = s & 0x7FFFFFFFu;
    double2 v = sacc[t];
    if (shifting) {
        double c, sn;
        shift_phase(m, i, ls, ms, ns, &c, &sn);
        double re = v.x * c + v.y * sn, im = -v.x * sn + v.y * c;
        v.x = re;
        v.y = im;
    }
    if (s >> 31) v.y = -v.y;
    if (minuend) {
        double2 a = minuend[i];
        v.x = a.x - v.x;
        v.y = a.y - v.y;
    }
    vis[i] = v;
}

__global__ void k_gather_f64(const uint32_t *src, int64_t nactive, const double *in, double *out)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (j >= nactive) return;
    out[j] = in ? in[src[j] & 0x7FFFFFFFu] : 1.0;
}

// Zero rectangles {row0, nrows, col0, ncols} of the launch's planes (blockIdx.y): what the scatter of a Hessian apply can
// touch in its own plane buffer, see pfbhip_gridder::clear_rects.
__global__ void __launch_bounds__(256) k_clear_rects(const int4 *__restrict__ rects, double2 *__restrict__ grid, size_t plane_stride,
                                                      int apitch)
{
    const int4 r = rects[blockIdx.x];
    double2 *base = grid + size_t(blockIdx.y) * plane_stride + size_t(r.x) * size_t(apitch) + size_t(r.z);
    const double2 z = make_double2(0.0, 0.0);
    for (int row = 0; row < r.y; ++row) {
        double2 *p = base + size_t(row) * size_t(apitch);
        for (int c = threadIdx.x; c < r.w; c += 256) p[c] = z;
    }
}

__global__ void k_scale_sorted(int64_t nactive, const double2 *in, const double *swgt, double2 *out)
{
    int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (j >= nactive) return;
    double2 v = in[j];
    double w = swgt[j];
    v.x *= w;
    v.y *= w;
    out[j] = v;
}

// correction image: cfu[ix] cfv[iy] / psi_w(t dw) [/ n], in the layout of the accumulator accT (ny, nx)
__global__ void k_corr_image(ImgGeom g, const double *cfu, const double *cfv, const double *cheb, int ncheb, double dw,
                             double zmax, int do_w, int use_psiw, int divide_by_n, double *corr)
{
    int64_t p = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (p >= int64_t(g.nx) * g.ny) return;
    int ix = int(p / g.ny), iy = int(p - int64_t(ix) * g.ny);
    double c = cfu[ix] * cfv[iy];
    if (do_w) {
        double t = pixel_t(g, ix, iy);
        if (use_psiw) {
            double z = t * dw / zmax;
            double y = 2.0 * z * z - 1.0;
            // Clenshaw
            double b1 = 0.0, b2 = 0.0;
            for (int k = ncheb - 1; k >= 1; --k) {
                double b0 = 2.0 * y * b1 - b2 + cheb[k];
                b2 = b1;
                b1 = b0;
            }
            c *= y * b1 - b2 + cheb[0];
        }
        if (divide_by_n) c /= (t - g.nshift + 1.0);
    }
    corr[size_t(iy) * size_t(g.nx) + size_t(ix)] = c;  // stored transposed: (ny, nx) like the image accumulator
}

// ---------------------------------------------------------------------------------------
// pruned two-pass plane transform
// ---------------------------------------------------------------------------------------
// The 2-D FFT of a w-plane is done as two batched ROW transforms (contiguous rows run at ~4 TB/s, strided
// columns at ~1 TB/s) with a transpose of our own in between, and every pass is pruned to what the
// algorithm needs (here in the plan's own -- transposed -- coordinates, see pfbhip_gridder_create):
//   A (nu, nv)  v contiguous : the uv-plane the scatter/gather kernels see.  Only the row blocks
//                              that hold visibilities ("occupied", from the tile sort) are ever
//                              cleared, transformed or transposed.
//   B (ny, nu)  u contiguous : after the v-transform only the ny image columns are kept (crop)
//                              and transposed; the u-transform then runs on ny rows.
// The image accumulator of the plane loop is kept transposed (ny, nx).
//   grid side  : clear occ(A) -> scatter -> FFT_v(occ rows) -> A2B (crop+transpose) -> FFT_u(ny rows)
//                -> crop+screen+accumulate (B -> accT)
//   degrid side: pad+screen (imgT -> B) -> FFT_u(ny rows) -> B2A (transpose+pad, occ rows) -> FFT_v(occ rows)
//                -> gather

// The plan works on the TRANSPOSED problem (pfbhip_gridder_create exchanges the two image axes, u <-> v), so its
// transposed accumulator accT (ny, nx) IS the caller's image layout: the image-side steps are element-wise.
// accT = x * corr [* beam]   (degrid input)
__global__ void __launch_bounds__(256) k_prepare_img(const double *x, const double *corr, const double *beam, int64_t n,
                                                      double *out)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i >= n) return;
    double v = x[i] * corr[i];
    if (beam) v *= beam[i];
    out[i] = v;
}
// out = accT * corr [* beam] * scale + eta * x
__global__ void __launch_bounds__(256) k_finalize_img(const double *accT, const double *corr, const double *beam, double scale,
                                                       double eta, const double *x, int64_t n, double *out)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i >= n) return;
    double v = accT[i] * corr[i];
    if (beam) v *= beam[i];
    v *= scale;
    if (x) v += eta * x[i];
    out[i] = v;
}

constexpr int TRANSPOSE_ROWS = 8;  // blockDim.y of the plane transposes (compile-time: the four loads of a thread are then in flight together)

// B (ny, nu) <- A (nu, nv): B[y][u] = A[u][wrap(y - ny/2, nv)] for occupied 32-row blocks of u, 0 elsewhere
__global__ void __launch_bounds__(TP * TRANSPOSE_ROWS) k_a2b(ImgGeom g, const uint8_t *occ, const double2 *A, double2 *B, int write_zeros)
{
    __shared__ double2 t[TP][TP + 1];
    const int u0 = blockIdx.x * TP, y0 = blockIdx.y * TP;
    const int hy = g.ny / 2;
    const bool on = occ[blockIdx.x] != 0;
    if (!on && !write_zeros) return;  // the fused second pass treats unoccupied blocks as zero without reading them
    if (on) {
#pragma unroll
        for (int kk = 0; kk < TP / TRANSPOSE_ROWS; ++kk) {
            const int k = int(threadIdx.y) + kk * TRANSPOSE_ROWS;
            int u = u0 + k, y = y0 + threadIdx.x;
            if (u < g.nu && y < g.ny) {
                int v = y - hy;
                if (v < 0) v += g.nv;
                t[k][threadIdx.x] = A[size_t(u) * size_t(g.apitch) + v];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int kk = 0; kk < TP / TRANSPOSE_ROWS; ++kk) {
        const int k = int(threadIdx.y) + kk * TRANSPOSE_ROWS;
        int y = y0 + k, u = u0 + threadIdx.x;
        if (u < g.nu && y < g.ny) B[size_t(y) * size_t(g.bpitch) + u] = on ? t[threadIdx.x][k] : make_double2(0.0, 0.0);
    }
}

// A (nu, nv) <- B (ny, nu) for occupied 32-row blocks of u: A[u][v] = B[y(v)][u], 0 where v is outside the image
__global__ void __launch_bounds__(TP * TRANSPOSE_ROWS) k_b2a(ImgGeom g, const uint8_t *occ, const double2 *B, double2 *A)
{
    __shared__ double2 t[TP][TP + 1];
    if (!occ[blockIdx.x]) return;
    const int u0 = blockIdx.x * TP, v0 = blockIdx.y * TP;
    const int hy = g.ny / 2;
#pragma unroll
    for (int kk = 0; kk < TP / TRANSPOSE_ROWS; ++kk) {
        const int k = int(threadIdx.y) + kk * TRANSPOSE_ROWS;
        int v = v0 + k, u = u0 + threadIdx.x;
        int y = -1;
        if (v < g.ny - hy) y = v + hy;
        else if (v >= g.nv - hy) y = v - (g.nv - hy);
        double2 val = make_double2(0.0, 0.0);
        if (y >= 0 && u < g.nu && v < g.nv) val = B[size_t(y) * size_t(g.bpitch) + u];
        t[k][threadIdx.x] = val;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TP / TRANSPOSE_ROWS; ++kk) {
        const int k = int(threadIdx.y) + kk * TRANSPOSE_ROWS;
        int u = u0 + k, v = v0 + threadIdx.x;
        if (u < g.nu && v < g.nv) A[size_t(u) * size_t(g.apitch) + v] = t[threadIdx.x][k];
    }
}

// degrid side: B[y][wrap(x - nx/2, nu)] = dcT[y][x] * exp(+2 pi i w_p t), 0 elsewhere (whole B written once)
__global__ void k_pad_screen_T(ImgGeom g, FusedGeom fg, const double *dcT, int do_w, double wplane, double2 *B)
{
    int u = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    if (u >= g.nu) return;
    const int hx = g.nx / 2;
    int ix = -1;
    if (u < g.nx - hx) ix = u + hx;
    else if (u >= g.nu - hx) ix = u - (g.nu - hx);
    double2 out = make_double2(0.0, 0.0);
    if (ix >= 0) {
        double val = dcT[size_t(y) * g.nx + ix];
        if (do_w) {
            double ph = wplane * fg_t(fg, ix, y);  // the fused kernels' screen: polynomial n-1, folded Taylor sincos
            ph -= rint(ph);
            double s, c;
            fg_sincos2pi(ph, s, c);
            out.x = val * c;
            out.y = val * s;
        } else {
            out.x = val;
        }
    }
    B[size_t(y) * size_t(g.bpitch) + u] = out;
}

// grid side: accT[y][x] (+)= Re( B[y][wrap(x - nx/2, nu)] * exp(-2 pi i w_p t) )
__global__ void k_crop_screen_T(ImgGeom g, FusedGeom fg, const double2 *B, int do_w, double wplane, int first, double *accT)
{
    int ix = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    if (ix >= g.nx) return;
    int u = ix - g.nx / 2;
    if (u < 0) u += g.nu;
    double2 v = B[size_t(y) * size_t(g.bpitch) + u];
    double r;
    if (do_w) {
        double ph = wplane * fg_t(fg, ix, y);
        ph -= rint(ph);
        double s, c;
        fg_sincos2pi(ph, s, c);
        r = v.x * c + v.y * s;
    } else {
        r = v.x;
    }
    size_t o = size_t(y) * g.nx + ix;
    accT[o] = first ? r : accT[o] + r;
}

// ---------------------------------------------------------------------------------------
// the handle
// ---------------------------------------------------------------------------------------

// single-precision I/O (the reference's precision="single" with double_precision_accumulation: values cross PCIe as
// float / complex64, every sum is formed in double): element-wise widening / narrowing on the device
__global__ void k_widen_f32(int64_t n, const float *__restrict__ in, double *__restrict__ out)
{
    const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i < n) out[i] = double(in[i]);
}
__global__ void k_narrow_f64(int64_t n, const double *__restrict__ in, float *__restrict__ out)
{
    const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i < n) out[i] = float(in[i]);
}

// stage indices of the profile, in the order of _lib.STAGE_NAMES
enum Stage { ST_GRID, ST_DEGRID, ST_FFT_ROWS, ST_PAD, ST_CROP, ST_OTHER, ST_FFT_CROP, ST_PAD_FFT, ST_COUNT };
static_assert(ST_COUNT == PFBHIP_NSTAGES, "stage list");

// Which kernels and transforms a plan runs.  Decided in three steps of plan creation (sort_key_sub in sort_by_tile,
// choose_kernels once build_work_lists has the work lists, choose_transforms in setup_transforms once the row-FFT plans
// exist; PlanBuild::path until then), read-only afterwards, and reported as info.scatter_mode / scatter_launches /
// scatter_block / gather_mode / fft_mode (report_path).
enum class Scatter { Walk, Block, Rec, OnePlane };   // k_grid_mp, k_grid_blk, k_grid_rec, k_grid_wd
enum class Gather { Walk, RowWalk, OnePlane };       // k_degrid_mp, k_degrid_rw, k_degrid_wd
enum class FirstAxis { RocFFT, Rows, Transposing };  // rocFFT rows of A; rowfft_plain + k_a2b / k_b2a; rowfft_a2b / rowfft_b2a
enum class SecondAxis { RocFFT, Rows, Fused };       // rocFFT rows of B; rowfft_plain + k_crop_screen_T / k_pad_screen_T; fused_*
struct PlanPath {
    Scatter scatter = Scatter::Walk;
    Gather gather = Gather::Walk;
    int bc = BLK_CELLS;          // block edge of the register-footprint scatters' frame (2: the sort key carries 2 x 2-cell blocks)
    bool coloured = false;       // four launches per pass, one per tile colour (plain read-add-write tile flush); else one launch
    bool gather_values = false;  // Hessian applies: the gather's epilogue writes the scatter's values (k_grid_rec, one-plane scatter)
    bool hess_fused = false;     // one-plane Hessian applies: k_hess_wd per colour instead of the gather and the scatter
    bool side_clear = false;     // Hessian applies clear the scatter's planes (d_grid2) on a side stream
    FirstAxis axis1 = FirstAxis::RocFFT;
    SecondAxis axis2 = SecondAxis::RocFFT;
};

// What one call runs beyond its plan's path: built by every entry point, passed down the pipeline.  Only Hessian applies
// (apply_op) set more than the output buffer.
enum class SideClear { None, Pending, Done };  // Pending: to be issued during the degrid half; Done: issued (ev_clear)
struct ApplyState {
    double2 *out;                    // plane buffer the scatter writes: d_grid, or d_grid2 once the side-stream clear is waited for
    bool gather_values = false;      // the gather writes the scatter's values into d_pval (no sacc, no scaling pass)
    bool hess_fused = false;         // no gather launch: the scatter half's launches gather from d_grid themselves (k_hess_wd)
    SideClear side = SideClear::None;
};

}  // namespace pfbhip

using namespace pfbhip;

struct pfbhip_gridder {
    pfbhip_gridder_params prm{};   // the TRANSPOSED problem the plan works on (image axes, pixel sizes, centres and u/v flips exchanged)
    pfbhip_gridder_params uprm{};  // the caller's parameters
    pfbhip_gridder_info info{};
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t nvis = 0;
    bool shifting = false;
    MapArgs map{};
    ImgGeom geom{};
    // plan-lifetime device data
    DevBuf<double> d_uvw, d_fc, d_pu, d_pv, d_pw, d_corr, d_cfu, d_cfv, d_cheb, d_ktab;
    DevBuf<uint8_t> d_mask;
    DevBuf<uint32_t> d_src;
    DevBuf<WorkItem> d_work;
    std::vector<size_t> work_off, work_cnt;  // per group of kp_max planes: slice of d_work
    // the same work split by tile colour (parity of the tile row / column) for the register-footprint scatter, whose tile
    // flush is a plain read-add-write when no other tile of the launch overlaps: 4 slices per group (empty when the tile
    // counts are odd -- the periodic wrap would put two tiles of one colour next to each other -- then one slice, all shared)
    DevBuf<WorkItem> d_work_col;
    std::vector<size_t> col_off, col_cnt;  // [group * 4 + colour]
    PlanPath path;
    int kp_max = 1;                            // planes scattered / gathered per pass (LDS holds kp_max tiles)
    size_t plane_stride = 0;                   // complex elements per plane of d_grid
    std::vector<double> wplanes;               // w of every plane (wavelengths)
    std::vector<double> nodes, lagr_coef;      // wmode 1: Chebyshev nodes and Lagrange denominators
    float wshare[3] = {1.3f / 3, 1.f / 3, 0.7f / 3};  // see GroupArgs::wshare: measured optimum on C2 (equal shares: +7 % scatter time)
    bool weights_bound = false;

    // scratch
    DevBuf<double2> d_grid, d_sval, d_sacc, d_vis;
    // Hessian applies clear the scatter's planes on a side stream while the degrid half runs: a second plane buffer
    // (d_grid2) is zeroed there, the scatter waits for it (single-pass plans only)
    DevBuf<double2> d_grid2;
    // The second buffer only ever holds what the scatter flushed into it: the (TILE + W - 1)^2 regions of the tiles that have
    // work.  Clearing those -- per tile row the runs of touched tile columns, 8-row slices -- instead of every occupied row
    // moves a third of the bytes when the uv coverage is a disc (C2: 0.9 of 2.4 GB).
    DevBuf<int4> d_clear_rects;
    int n_clear_rects = 0;  // (> 0 only with the transposing first-axis transform)
    hipStream_t clear_stream = nullptr;
    hipEvent_t ev_clear = nullptr, ev_start = nullptr;
    DevBuf<double> d_wgt, d_swgt, d_img, d_img2, d_beam;
    DevBuf<double2> d_gridB;  // (ny, nu) transposed / cropped plane
    DevBuf<double> d_accT;    // (ny, nx) transposed image accumulator / transposed degrid input
    // host <-> device transfers of single-precision I/O go through this staging buffer (upload / download below); it is
    // reused by the next transfer: in-order on this stream
    DevBuf<float> d_stage32;

    // per-scheme tables
    // record-driven register-footprint scatter (k_grid_rec) and one-plane scatter: d_rec, static per-visibility records; d_pval,
    // the plane-weighted values of the current apply (kp_max, or wd.K, per visibility), written by the gather inside a Hessian
    // apply (ApplyState::gather_values) or by k_plane_values* in front of the scatter
    DevBuf<VisRec> d_rec;
    DevBuf<double2> d_pval;
    // row-walk gather (k_degrid_rw): d_kw, plane weights of every visibility (plan time)
    DevBuf<double> d_kw;
    // one-plane w-scheme (info.wmode == 2, gridder_wd_api.hpp): K kernel functions per axis, their derivative tables, the K
    // complex coefficients of every sorted visibility
    WdArgs wd{};
    DevBuf<double> d_dtab;
    DevBuf<double2> d_cw;

    // transforms
    DevBuf<uint8_t> d_occ;  // occupancy of 32-row blocks of the uv-plane
    struct RowSpan {
        int64_t row0, nrows;                      // occupied rows [row0, row0 + nrows) of A
        rocfft_plan fwd = nullptr, bwd = nullptr;  // batched length-nv row transforms
    };
    std::vector<RowSpan> spans;
    int64_t occ_rows = 0;
    RowFFT rowfft_u;     // hand-written row FFT of length nu with fused pad / crop (if nu is supported)
    RowFFT rowfft_v;     // hand-written row FFT of length nv for the occupied rows of A (if nv is supported)
    size_t bstride = 0;  // complex elements per plane of d_gridB
    // first-axis row FFTs with the crop / pad + transpose folded in (rowfft_a2b / rowfft_b2a): row of every workgroup,
    // ordered so that the 8 rows of a 128-byte line of B run on one XCD at about the same time (PFBHIP_TFFT=0: the
    // separate k_a2b / k_b2a passes)
    DevBuf<int> d_rowmap;
    DevBuf<int4> d_colruns;  // per tile row: the column runs in use (transposing first-axis FFT: RunLoad / RunStore)
    FusedGeom fgeom;         // filled once by create_impl (fused path)
    std::vector<FusedPlanes> plane_groups;  // per pass of kp_max planes: w and the composite screen polynomials (plan time)
    DevBuf<double2> d_tau;                  // column tables of the separable screens (FusedPlanes::sep), nplanes x nx
    rocfft_plan fftB_fwd = nullptr, fftB_bwd = nullptr;  // ny rows of length nu
    rocfft_execution_info fft_info = nullptr;
    DevBuf<char> d_fftwork;

    // the profile: events around the stages (timer), what pfbhip_gridder_profile / _profile_get collected from them so far
    StageTimer timer;
    double stage_ms[PFBHIP_NSTAGES] = {0};
    int64_t stage_calls[PFBHIP_NSTAGES] = {0};

    size_t device_bytes() const  // every DevBuf above, in the order of its declaration
    {
        return d_uvw.bytes() + d_fc.bytes() + d_pu.bytes() + d_pv.bytes() + d_pw.bytes() + d_corr.bytes() + d_cfu.bytes() +
               d_cfv.bytes() + d_cheb.bytes() + d_ktab.bytes() + d_mask.bytes() + d_src.bytes() + d_work.bytes() + d_work_col.bytes() +
               d_grid.bytes() + d_sval.bytes() + d_sacc.bytes() + d_vis.bytes() + d_grid2.bytes() + d_clear_rects.bytes() +
               d_wgt.bytes() + d_swgt.bytes() + d_img.bytes() + d_img2.bytes() + d_beam.bytes() + d_gridB.bytes() + d_accT.bytes() +
               d_stage32.bytes() + d_rec.bytes() + d_pval.bytes() + d_kw.bytes() + d_dtab.bytes() + d_cw.bytes() + d_occ.bytes() +
               d_rowmap.bytes() + d_colruns.bytes() + d_tau.bytes() + d_fftwork.bytes();
    }

    ~pfbhip_gridder()
    {
        for (auto &sp : spans) {
            if (sp.fwd) rocfft_plan_destroy(sp.fwd);
            if (sp.bwd) rocfft_plan_destroy(sp.bwd);
        }
        if (fftB_fwd) rocfft_plan_destroy(fftB_fwd);
        if (fftB_bwd) rocfft_plan_destroy(fftB_bwd);
        if (fft_info) rocfft_execution_info_destroy(fft_info);
        if (stream) (void)hipStreamDestroy(stream);
        if (clear_stream) (void)hipStreamDestroy(clear_stream);
        if (ev_clear) (void)hipEventDestroy(ev_clear);
        if (ev_start) (void)hipEventDestroy(ev_start);
    }

    PlaneArgs plane_args(int plane) const
    {
        PlaneArgs a;
        a.nu = int(info.nu);
        a.nv = int(info.nv);
        a.ntv = map.ntv;
        a.apitch = geom.apitch;
        a.do_w = prm.do_wgridding;
        a.plane = plane;
        a.wmode = info.wmode;
        a.nplanes = int(info.nplanes);
        a.ktab = d_ktab.p;
        a.coef = info.wmode == 1 ? lagr_coef[size_t(plane)] : 1.0;
        for (int m = 0; m < MAX_POLY_PLANES; ++m) a.nodes[m] = (info.wmode == 1 && m < int(nodes.size())) ? nodes[size_t(m)] : 0.0;
        a.pu = d_pu.p;
        a.pv = d_pv.p;
        a.pw = d_pw.p;
        const size_t grp = work_off.size() > 1 ? size_t(plane / kp_max) : 0;
        a.work = d_work.p + work_off[grp];
        a.nwork = uint32_t(work_cnt[grp]);
        return a;
    }

    // batched row transforms of the occupied rows of plane k of `planes` (length nv)
    void fft_rows_A(double2 *planes, bool forward, int k = 0)
    {
        timer.begin(ST_FFT_ROWS);
        for (auto &sp : spans) {
            double2 *rows = planes + size_t(k) * plane_stride + size_t(sp.row0) * size_t(geom.apitch);
            if (path.axis1 == FirstAxis::Rows) {
                rowfft_plain(rowfft_v.pl, rows, int(sp.nrows), !forward, stream, size_t(geom.apitch));
            } else {
                void *buf[1] = {rows};
                PFB_ROCFFT(rocfft_execute(forward ? sp.fwd : sp.bwd, buf, nullptr, fft_info));
            }
        }
        timer.end();
    }
    // ny row transforms of B (length nu)
    void fft_rows_B(bool forward)
    {
        timer.begin(ST_FFT_ROWS);
        if (path.axis2 == SecondAxis::Rows) {  // unfused second axis on the hand-written FFT (doubled shapes, PFBHIP_FUSED_FFT=0 + PFBHIP_ROWFFT=1)
            rowfft_plain(rowfft_u.pl, d_gridB.p, int(prm.ny), !forward, stream);
        } else {
            void *buf[1] = {d_gridB.p};
            PFB_ROCFFT(rocfft_execute(forward ? fftB_fwd : fftB_bwd, buf, nullptr, fft_info));
        }
        timer.end();
    }

    GroupArgs group_args(int plane0, int kp) const
    {
        GroupArgs ga;
        ga.a = plane_args(plane0);
        ga.kp = kp;
        ga.kp_alloc = kp_max;
        for (int k = 0; k < KP_MAX; ++k)
            ga.coefk[k] = (info.wmode == 1 && k < kp) ? lagr_coef[size_t(plane0 + k)] : 1.0;
        ga.plane_stride = plane_stride;
        for (int q = 0; q < 3; ++q) ga.wshare[q] = wshare[q];
        return ga;
    }
    // dynamic LDS: kp_max tiles (re/im or interleaved complex) + the (W, D+1) kernel table
    template <int W>
    size_t lds_bytes_mp() const
    {
        constexpr int D = kernel_poly_degree_c(W);
        static_assert(kernel_poly_degree_c(W) == kernel_poly_degree(W), "degree mismatch");
        return (size_t(2) * size_t(kp_max) * tile_rows(W) * tile_stride(W) + size_t(W) * (D + 1)) * sizeof(double);
    }
    template <int W>
    static constexpr size_t lds_bytes_mp_max()
    {
        constexpr int D = kernel_poly_degree_c(W);
        return (size_t(2) * KP_MAX * tile_rows(W) * tile_stride(W) + size_t(W) * (D + 1)) * sizeof(double);
    }
    template <int W, int KP>
    size_t lds_bytes_blk() const
    {
        return (size_t(2) * KP * blk_tile_rows(W) * blk_stride(W, KP) + blk_fixed_doubles(W, blk_threads(kp_max) / 64)) * sizeof(double);
    }

    // the scatter of planes [plane0, plane0 + kp) of sval into a.out: one launch, or one per tile colour (see blk_tile_to_grid)
    void launch_grid(const ApplyState &a, int plane0, int kp, const double2 *sval)
    {
        GroupArgs ga = group_args(plane0, kp);
        if (ga.a.nwork == 0) return;
        with_W(int(info.W), [&](auto w) {
            constexpr int W = decltype(w)::value;
            if (path.scatter == Scatter::Walk) {
                timer.begin(ST_GRID);
                with_KP(kp, [&](auto k) {
                    constexpr int KP = decltype(k)::value;
                    allow_dynamic_lds(reinterpret_cast<const void *>(&k_grid_mp<W, KP>), int(lds_bytes_mp_max<W>()));
                    hipLaunchKernelGGL((k_grid_mp<W, KP>), dim3(ga.a.nwork), dim3(MP_THREADS), lds_bytes_mp<W>(), stream, ga, sval, a.out);
                });
                timer.end();
                return;
            }
            const bool from_values = path.scatter == Scatter::Rec || path.scatter == Scatter::OnePlane;
            if (from_values && !a.gather_values && !a.hess_fused) {
                timer.begin(ST_OTHER);
                if (info.wmode == 2)
                    wd_launch_plane_values(wd.K, info.nactive, d_cw.p, sval, d_pval.p, stream);
                else if (prm.do_wgridding && info.wmode == 0)
                    hipLaunchKernelGGL((k_plane_values_es<W>), dim3(ga.a.nwork), dim3(256), 0, stream, ga, sval, d_pval.p);
                else
                    hipLaunchKernelGGL((k_plane_values<W>), dim3(uint32_t(ceil_div(info.nactive, 256))), dim3(256), 0, stream, ga,
                                       info.nactive, sval, d_pval.p);
                timer.end();
            }
            const size_t grp = work_off.size() > 1 ? size_t(plane0 / kp_max) : 0;
            for (int col = 0; col < 4; ++col) {
                ga.a.work = d_work_col.p + col_off[grp * 4 + size_t(col)];
                ga.a.nwork = uint32_t(col_cnt[grp * 4 + size_t(col)]);
                if (ga.a.nwork == 0) continue;
                timer.begin(ST_GRID);
                if (path.scatter == Scatter::OnePlane) {
                    if (a.hess_fused)  // (the gather's plane is d_grid, the output a.out = d_grid2)
                        wd_launch_hessian(ga, wd, d_rec.p, d_swgt.p, d_grid.p, a.out, stream);
                    else
                        wd_launch_grid(ga, wd, d_rec.p, d_pval.p, a.out, stream);
                } else {
                    with_KP(kp, [&](auto k) {
                        with_BC<W>(path.bc, [&](auto bc) {
                            constexpr int KP = decltype(k)::value, BC = decltype(bc)::value;
                            const size_t lds = lds_bytes_blk<W, KP>();
                            const dim3 grid(ga.a.nwork), block(blk_threads(kp_max));
                            if (path.scatter == Scatter::Rec) {
                                allow_dynamic_lds(reinterpret_cast<const void *>(&k_grid_rec<W, KP, BC>), 160 * 1024);
                                PFB_REQUIRE(lds <= size_t(160) * 1024, "record scatter needs %zu bytes of LDS", lds);
                                hipLaunchKernelGGL((k_grid_rec<W, KP, BC>), grid, block, lds, stream, ga, d_rec.p, d_pval.p, a.out);
                            } else {
                                allow_dynamic_lds(reinterpret_cast<const void *>(&k_grid_blk<W, KP, BC>), 160 * 1024);
                                PFB_REQUIRE(lds <= size_t(160) * 1024, "block scatter needs %zu bytes of LDS", lds);
                                hipLaunchKernelGGL((k_grid_blk<W, KP, BC>), grid, block, lds, stream, ga, sval, a.out);
                            }
                        });
                    });
                }
                timer.end();
            }
        });
    }
    // the gather of planes [plane0, plane0 + kp) of d_grid into sacc (or, with a.gather_values, the scatter's values into d_pval)
    void launch_degrid(const ApplyState &a, int plane0, int kp, double2 *sacc)
    {
        GroupArgs ga = group_args(plane0, kp);
        if (ga.a.nwork == 0) return;
        const double *swgt = a.gather_values ? d_swgt.p : nullptr;
        double2 *pval = a.gather_values ? d_pval.p : nullptr;
        with_W(int(info.W), [&](auto w) {
            if (path.gather == Gather::OnePlane) return wd_launch_degrid(ga, wd, d_rec.p, d_grid.p, sacc, swgt, pval, stream);
            with_KP(kp, [&](auto k) {
                constexpr int W = decltype(w)::value, KP = decltype(k)::value;
                if (path.gather == Gather::RowWalk) {
                    allow_dynamic_lds(reinterpret_cast<const void *>(&k_degrid_rw<W, KP>), 160 * 1024);
                    const size_t lds = size_t(KP) * RW_LS * RW_LS * sizeof(double2);
                    hipLaunchKernelGGL((k_degrid_rw<W, KP>), dim3(ga.a.nwork), dim3(MP_THREADS), lds, stream, ga, d_rec.p, d_kw.p, d_grid.p,
                                       sacc, swgt, pval);
                } else {
                    allow_dynamic_lds(reinterpret_cast<const void *>(&k_degrid_mp<W, KP>), int(lds_bytes_mp_max<W>()));
                    hipLaunchKernelGGL((k_degrid_mp<W, KP>), dim3(ga.a.nwork), dim3(MP_THREADS), lds_bytes_mp<W>(), stream, ga, d_grid.p,
                                       sacc, swgt, pval);
                }
            });
        });
    }

    dim3 tgrid(int64_t ncols, int64_t nrows) const { return dim3(uint32_t(ceil_div(ncols, TP)), uint32_t(ceil_div(nrows, TP))); }

    // Clear the second plane buffer on the side stream, starting when this stream reaches the present point (which also
    // means the previous apply's scatter half, the buffer's last user, has finished).
    void side_clear(ApplyState &a)
    {
        PFB_HIP(hipEventRecord(ev_start, stream));
        PFB_HIP(hipStreamWaitEvent(clear_stream, ev_start, 0));
        clear_planes(d_grid2.p, int(info.nplanes), clear_stream);
        PFB_HIP(hipEventRecord(ev_clear, clear_stream));
        a.side = SideClear::Done;
    }

    // zero the occupied rows of the first kp planes of `planes` -- or, where the first-axis transform reads column runs only
    // (FirstAxis::Transposing: n_clear_rects > 0), just the rectangles the scatter can touch (multi-pass plans: every pass
    // clears its planes)
    void clear_planes(double2 *planes, int kp, hipStream_t st)
    {
        if (n_clear_rects > 0) {
            hipLaunchKernelGGL(k_clear_rects, dim3(uint32_t(n_clear_rects), uint32_t(kp)), dim3(256), 0, st, d_clear_rects.p, planes,
                               plane_stride, geom.apitch);
            PFB_HIP(hipGetLastError());
            return;
        }
        for (int k = 0; k < kp; ++k)
            for (auto &sp : spans)
                PFB_HIP(hipMemsetAsync(planes + size_t(k) * plane_stride + size_t(sp.row0) * size_t(geom.apitch), 0,
                                       size_t(sp.nrows) * size_t(geom.apitch) * sizeof(double2), st));
    }

    // sval (tile-sorted, weighted) -> accT, the TRANSPOSED (ny, nx) raw image (before correction)
    // `fin` (fused path only): the last launch writes the finalized image; returns true if it did
    bool grid_all_planes(const ApplyState &a, const double2 *sval, const FusedFinal *fin = nullptr)
    {
        const int64_t npix = int64_t(prm.nx) * prm.ny;
        if (info.nactive == 0 || info.nwork == 0) {
            PFB_HIP(hipMemsetAsync(d_accT.p, 0, npix * sizeof(double), stream));
            return false;
        }
        const bool fused = path.axis2 == SecondAxis::Fused, tfft = path.axis1 == FirstAxis::Transposing;
        bool finalized = false;
        for (int p0 = 0; p0 < info.nplanes; p0 += kp_max) {
            const int kp = int(std::min<int64_t>(kp_max, info.nplanes - p0));
            if (a.side != SideClear::Done) {  // (a Hessian apply has cleared them on the side stream)
                timer.begin(ST_OTHER);
                clear_planes(a.out, kp, stream);
                timer.end();
            }
            launch_grid(a, p0, kp, sval);  // ST_GRID, timed per kernel launch inside
            PFB_HIP(hipGetLastError());
            if (tfft) {  // every plane of the pass in one launch
                timer.begin(ST_FFT_ROWS);
                rowfft_a2b(rowfft_v.pl, a.out, d_gridB.p, d_rowmap.p, int(occ_rows), geom.bpitch, int(prm.ny), size_t(geom.apitch),
                           kp, plane_stride, bstride, d_colruns.p, stream);
                timer.end();
            }
            for (int k = 0; k < kp && !tfft; ++k) {
                const int p = p0 + k;
                fft_rows_A(a.out, false, k);
                timer.begin(ST_CROP);
                hipLaunchKernelGGL(k_a2b, tgrid(info.nu, prm.ny), dim3(TP, TRANSPOSE_ROWS), 0, stream, geom, d_occ.p,
                                   a.out + size_t(k) * plane_stride, d_gridB.p + (fused ? size_t(k) * bstride : 0),
                                   fused ? 0 : 1);
                PFB_HIP(hipGetLastError());
                timer.end();
                if (!fused) {
                    fft_rows_B(false);
                    timer.begin(ST_CROP);
                    hipLaunchKernelGGL(k_crop_screen_T, dim3(uint32_t(ceil_div(prm.nx, 256)), uint32_t(prm.ny)),
                                       dim3(256), 0, stream, geom, fgeom, d_gridB.p, prm.do_wgridding, wplanes[size_t(p)],
                                       p == 0 ? 1 : 0, d_accT.p);
                    PFB_HIP(hipGetLastError());
                    timer.end();
                }
            }
            if (fused) {
                timer.begin(ST_FFT_CROP);
                const bool last_group = p0 + kp >= info.nplanes;
                FusedFinal f = (fin != nullptr && last_group) ? *fin : FusedFinal{};
                if (f.corr != nullptr) finalized = true;
                fused_fft_crop(rowfft_u, fused_geom(), d_occ.p, d_gridB.p, bstride, fused_planes(p0, kp), prm.do_wgridding,
                               p0 == 0, d_accT.p, f, stream);
                timer.end();
            }
        }
        return finalized;
    }
    // grid + finalize, folding the finalize into the last fused launch where possible
    void grid_and_finalize(const ApplyState &a, const double2 *sval, const double *beam, double scale, double eta, const double *x,
                           double *out)
    {
        FusedFinal f;
        f.corr = d_corr.p;
        f.beam = beam;
        f.x = x;
        f.scale = scale;
        f.eta = eta;
        f.out = out;
        if (!grid_all_planes(a, sval, path.axis2 == SecondAxis::Fused ? &f : nullptr)) finalize(beam, scale, eta, x, out);
    }

    const FusedGeom &fused_geom() const { return fgeom; }
    FusedPlanes fused_planes(int p0, int kp) const
    {
        const size_t grp = size_t(p0 / kp_max);
        if (grp < plane_groups.size() && plane_groups[grp].kp == kp) return plane_groups[grp];
        FusedPlanes fp;
        fp.kp = kp;
        for (int k = 0; k < FUSED_MAXPLANES; ++k) fp.w[k] = k < kp ? wplanes[size_t(p0 + k)] : 0.0;
        return fp;
    }

    // out = accT * corr [* beam] * scale + eta * x   (all in the caller's image layout)
    void finalize(const double *beam, double scale, double eta, const double *x, double *out)
    {
        const int64_t npix = int64_t(prm.nx) * prm.ny;
        timer.begin(ST_OTHER);
        hipLaunchKernelGGL(k_finalize_img, dim3(uint32_t(ceil_div(npix, 256))), dim3(256), 0, stream, d_accT.p, d_corr.p, beam, scale,
                           eta, x, npix, out);
        PFB_HIP(hipGetLastError());
        timer.end();
    }

    // accT = x * corr [* beam] : the degrid input
    void prepare_degrid_input(const double *x, const double *beam)
    {
        const int64_t npix = int64_t(prm.nx) * prm.ny;
        timer.begin(ST_OTHER);
        hipLaunchKernelGGL(k_prepare_img, dim3(uint32_t(ceil_div(npix, 256))), dim3(256), 0, stream, x, d_corr.p, beam, npix,
                           d_accT.p);
        PFB_HIP(hipGetLastError());
        timer.end();
    }

    // x -> sacc, folding the x * corr * beam step into the fused pad kernel where possible
    void prepare_and_degrid(ApplyState &a, const double *x, const double *beam, double2 *sacc)
    {
        // The side-stream clear of the scatter's planes starts with the apply, under the degridding side's row transforms (round
        // 4b; before that: in front of the gather).  The gather's workgroups fill every CU's registers (three
        // waves of 168 VGPRs per SIMD), so a clear issued next to it only got onto the chip as the gather drained and ran into
        // the scatter; the fused row-FFT kernels leave room.  C2: degrid 1.647 -> 1.594 ms, pad_fft + 0.01, apply 5.91 -> 5.86 ms.
        // (one plane only: with the three planes of the polynomial scheme the clear's 0.9 GB cost pad_fft what they save the gather,
        // 9.73 against 9.77 ms)
        if (a.side == SideClear::Pending && info.nplanes == 1) side_clear(a);
        if (path.axis2 == SecondAxis::Fused && info.nactive != 0 && info.nwork != 0 && fused_pad_takes_prep(rowfft_u, fgeom)) {
            FusedPrep p;
            p.x = x;
            p.corr = d_corr.p;
            p.beam = beam;
            degrid_all_planes(a, sacc, &p);
        } else {
            prepare_degrid_input(x, beam);
            degrid_all_planes(a, sacc);
        }
    }

    // accT (transposed, corrected image) -> sacc (tile-sorted)
    // `prep` (fused path only): the fused pad kernel reads x * corr [* beam] itself instead of a prepared accT
    void degrid_all_planes(ApplyState &a, double2 *sacc, const FusedPrep *prep = nullptr)
    {
        if (!a.gather_values && !a.hess_fused) PFB_HIP(hipMemsetAsync(sacc, 0, size_t(std::max<int64_t>(info.nactive, 1)) * sizeof(double2), stream));
        if (info.nactive == 0 || info.nwork == 0) return;
        const bool fused = path.axis2 == SecondAxis::Fused, tfft = path.axis1 == FirstAxis::Transposing;
        for (int p0 = 0; p0 < info.nplanes; p0 += kp_max) {
            const int kp = int(std::min<int64_t>(kp_max, info.nplanes - p0));
            if (fused) {
                timer.begin(ST_PAD_FFT);
                fused_pad_fft(rowfft_u, fused_geom(), d_occ.p, d_accT.p, prep != nullptr ? *prep : FusedPrep{},
                              fused_planes(p0, kp), prm.do_wgridding, d_gridB.p, bstride, stream);
                timer.end();
            }
            if (tfft) {
                timer.begin(ST_FFT_ROWS);
                rowfft_b2a(rowfft_v.pl, d_gridB.p, d_grid.p, d_rowmap.p, int(occ_rows), geom.bpitch, int(prm.ny), size_t(geom.apitch),
                           fgeom.tpitch, kp, plane_stride, bstride, d_colruns.p, stream);
                timer.end();
            }
            for (int k = 0; k < kp && !tfft; ++k) {
                const int p = p0 + k;
                if (!fused) {
                    timer.begin(ST_PAD);
                    hipLaunchKernelGGL(k_pad_screen_T, dim3(uint32_t(ceil_div(info.nu, 256)), uint32_t(prm.ny)),
                                       dim3(256), 0, stream, geom, fgeom, d_accT.p, prm.do_wgridding, wplanes[size_t(p)],
                                       d_gridB.p);
                    PFB_HIP(hipGetLastError());
                    timer.end();
                    fft_rows_B(true);
                }
                timer.begin(ST_PAD);
                hipLaunchKernelGGL(k_b2a, tgrid(info.nu, info.nv), dim3(TP, TRANSPOSE_ROWS), 0, stream, geom, d_occ.p,
                                   d_gridB.p + (fused ? size_t(k) * bstride : 0), d_grid.p + size_t(k) * plane_stride);
                PFB_HIP(hipGetLastError());
                timer.end();
                fft_rows_A(d_grid.p, true, k);
            }
            if (a.side == SideClear::Pending) side_clear(a);
            if (a.hess_fused) continue;  // (the fused launches of the scatter half gather)
            timer.begin(ST_DEGRID);
            launch_degrid(a, p0, kp, sacc);
            PFB_HIP(hipGetLastError());
            timer.end();
        }
    }

    // host <-> device transfers of n values: double as they are; float (single-precision I/O) through the staging buffer
    // d_stage32, widened / narrowed on the device
    void upload(const double *host, size_t n, double *dst)
    {
        PFB_HIP(hipMemcpyAsync(dst, host, n * sizeof(double), hipMemcpyHostToDevice, stream));
    }
    void upload(const float *host, size_t n, double *dst)
    {
        d_stage32.ensure(n);
        PFB_HIP(hipMemcpyAsync(d_stage32.p, host, n * sizeof(float), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_widen_f32, dim3(uint32_t(ceil_div(int64_t(n), 256))), dim3(256), 0, stream, int64_t(n), d_stage32.p, dst);
        PFB_HIP(hipGetLastError());
    }
    void download(const double *src, size_t n, double *host)
    {
        PFB_HIP(hipMemcpyAsync(host, src, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    void download(const double *src, size_t n, float *host)
    {
        d_stage32.ensure(n);
        hipLaunchKernelGGL(k_narrow_f64, dim3(uint32_t(ceil_div(int64_t(n), 256))), dim3(256), 0, stream, int64_t(n), src, d_stage32.p);
        PFB_HIP(hipGetLastError());
        PFB_HIP(hipMemcpyAsync(host, d_stage32.p, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    template <class T>
    void upload_vis_wgt(const T *vis_host, const T *wgt_host)
    {
        if (vis_host) {
            d_vis.ensure(size_t(nvis));
            upload(vis_host, size_t(nvis) * 2, reinterpret_cast<double *>(d_vis.p));
        }
        if (wgt_host) {
            d_wgt.ensure(size_t(nvis));
            upload(wgt_host, size_t(nvis), d_wgt.p);
        }
    }
    // the optional beam image of a Hessian apply: d_beam <- beam_host; NULL stays NULL
    template <class T>
    const double *bind_beam(const T *beam_host)
    {
        if (!beam_host) return nullptr;
        const size_t npix = size_t(prm.nx * prm.ny);
        d_beam.ensure(npix);
        upload(beam_host, npix, d_beam.p);
        return d_beam.p;
    }
};

namespace pfbhip {

// Measured rocFFT 2-D complex128 in-place times (ms) on MI355X, ROCm 7.2 (profiles/r01a_rocfft_sizes.txt):
// lengths <= 10240 (160 KiB of LDS per row) run one kernel per axis; longer ones are decomposed.
static double fft2d_seconds(int64_t nu, int64_t nv)
{
    static const struct { int64_t n; double ms; } meas[] = {
        {8192, 1.80}, {9216, 2.47}, {10240, 2.94}, {10368, 6.33}, {10752, 4.13}, {11520, 8.20},
        {12288, 6.13}, {12800, 11.1}, {13824, 12.4}, {14336, 12.1}, {16384, 9.27}};
    auto per_point = [&](int64_t n) {
        for (auto &m : meas)
            if (m.n == n) return m.ms * 1e-3 / (double(n) * double(n));
        return n <= 10240 ? 2.9e-11 : 5.5e-11;
    };
    return 0.5 * (per_point(nu) + per_point(nv)) * double(nu) * double(nv);
}

// Smallest K with  omega^K / (2^(K-1) K!) <= eps : the error bound of interpolating exp(i omega s),
// |s| <= 1, at K Chebyshev nodes.  0 if K would exceed MAX_POLY_PLANES.
static int poly_planes_needed(double omega, double eps)
{
    if (omega <= 0.0) return 1;
    double bound = omega;
    int k = 1;
    while (bound > eps) {
        ++k;
        bound *= omega / (2.0 * k);
        if (k > MAX_POLY_PLANES) return 0;
    }
    return k;
}

// One-plane w-scheme (wmode 2): t_q = n(s_q) - 1 + nshift at the K Chebyshev nodes s_q of [0, smax], and M[k][q], the
// coefficient of (s / smax)^k in the Lagrange basis polynomial of node q.
static void wd_interp_nodes(int K, double smax, double nshift, double *tq, double (*M)[WD_MAX_K])
{
    double xq[WD_MAX_K];
    for (int q = 0; q < K; ++q) {
        xq[q] = 0.5 * (1.0 - std::cos(pi_const * (2.0 * double(q) + 1.0) / (2.0 * double(K))));  // nodes on [0, 1]
        const double sq = xq[q] * smax;
        tq[q] = -sq / (1.0 + std::sqrt(1.0 - sq)) + nshift;
    }
    for (int q = 0; q < K; ++q) {  // monomial coefficients of the Lagrange basis polynomial of node q
        long double c[WD_MAX_K + 1] = {1.0L, 0, 0, 0, 0};
        int deg = 0;
        long double den = 1.0L;
        for (int m2 = 0; m2 < K; ++m2) {
            if (m2 == q) continue;
            for (int d = deg + 1; d >= 1; --d) c[d] = c[d - 1] - (long double)xq[m2] * c[d];
            c[0] = -(long double)xq[m2] * c[0];
            ++deg;
            den *= (long double)xq[q] - (long double)xq[m2];
        }
        for (int k = 0; k < K; ++k) M[k][q] = double(c[k] / den);
    }
}

// Worst error of the one-plane scheme's interpolation in s = l^2 + m^2 of exp(-2 pi i dw (t(s) + nshift)), t(s) = sqrt(1 - s) - 1,
// K nodes, over WD_ERR_NW + 1 values of dw in [-whalf, whalf] and WD_ERR_NS + 1 values of s in [0, smax].  Measured, not
// bounded: poly_planes_needed bounds the interpolation in a variable linear in t, and t(s) is curved -- the curvature term grows
// like omega smax^K, not (omega smax)^K, and dominates for a wide field with a small w range.  Infinite once the image reaches
// the horizon (smax >= 1: the nodes past s = 1 have no real n) or a sample is not finite, so a test `!(err <= bound)` rejects.
// (oracle/wgridder.py: wd_interp_error takes the same samples)
constexpr int WD_ERR_NW = 16, WD_ERR_NS = 128;
static double wd_interp_error(int K, double smax, double whalf, double nshift)
{
    if (!(smax >= 0.0 && smax < 1.0)) return HUGE_VAL;
    double tq[WD_MAX_K], M[WD_MAX_K][WD_MAX_K];
    wd_interp_nodes(K, smax, nshift, tq, M);
    double worst = 0.0;
    for (int iw = 0; iw <= WD_ERR_NW; ++iw) {
        const double dwv = whalf * (double(iw) / (0.5 * WD_ERR_NW) - 1.0);
        double cr[WD_MAX_K], ci[WD_MAX_K];
        for (int k = 0; k < K; ++k) {
            cr[k] = ci[k] = 0.0;
            for (int q = 0; q < K; ++q) {
                cr[k] += M[k][q] * std::cos(2.0 * pi_const * dwv * tq[q]);
                ci[k] -= M[k][q] * std::sin(2.0 * pi_const * dwv * tq[q]);
            }
        }
        for (int is = 0; is <= WD_ERR_NS; ++is) {
            const double x = double(is) / double(WD_ERR_NS), sv = x * smax;
            const double tt = -sv / (1.0 + std::sqrt(1.0 - sv)) + nshift;
            double ar = 0.0, ai = 0.0, xp = 1.0;
            for (int k = 0; k < K; ++k) {
                ar += cr[k] * xp;
                ai += ci[k] * xp;
                xp *= x;
            }
            const double e = std::hypot(ar - std::cos(2.0 * pi_const * dwv * tt), ai + std::sin(2.0 * pi_const * dwv * tt));
            if (!std::isfinite(e)) return HUGE_VAL;
            worst = std::max(worst, e);
        }
    }
    return worst;
}

// largest l^2 + m^2 of the pixel lattice of an on-axis image (pixel 0 sits at -(n / 2) pixsize)
static double wd_smax(const pfbhip_gridder_params &p)
{
    const double xe = double(p.nx / 2) * p.pixsize_x, ye = double(p.ny / 2) * p.pixsize_y;
    return xe * xe + ye * ye;
}

// The share of epsilon the w-interpolation of the polynomial and one-plane schemes may take: 2 eps_w, eps_w = epsilon / 3, times
// the smallest n of the image (>= 0.25) with divide_by_n, which weights a pixel's error with 1 / n
static double w_interp_budget(const pfbhip_gridder_params &p, double nmin)
{
    return 2.0 * p.epsilon / 3.0 * (p.divide_by_n ? std::max(0.25, std::min(1.0, nmin)) : 1.0);
}

// The switches that override the plan's choices.  Read once at the start of every plan creation,
// never cached for the process: the tests set them between plans to keep the alternative kernels covered.
enum class ScatterForce { Auto, Walk, Block, Rec, RecEs };  // PFBHIP_SCATTER=auto / walk / block / rec / rec_es
struct PlanSwitches {
    ScatterForce scatter = ScatterForce::Auto;
    bool wmode2 = true;       // PFBHIP_WMODE2=0: keep the multi-plane w-schemes
    bool wd_block4 = false;   // PFBHIP_WD_BLOCK=4: 4 x 4-cell anchoring at W = 14, 15
    int wd_colours = -1;      // PFBHIP_WD_COLOURS: -1 plan decides, 0 one launch (atomic flush), 1 four colour launches
    bool rowfft = true;       // PFBHIP_ROWFFT=0: rocFFT row plans
    bool fused_fft = true;    // PFBHIP_FUSED_FFT=0: unfused second axis
    int fused_doubled = -1;   // PFBHIP_FUSED_DOUBLED: -1 plan decides, 0 / 1 forced
    bool sepscreen = true;    // PFBHIP_SEPSCREEN=0: no separable w-screen form
    bool tfft = true;         // PFBHIP_TFFT=0: plain first-axis row FFT + separate transpose kernels
    bool wd_fused = true;     // PFBHIP_WD_FUSED=0: one-plane Hessian applies keep the gather / scatter pair
};

static PlanSwitches read_plan_switches()
{
    PlanSwitches sw;
    auto first = [](const char *name) -> int {  // first character of the value, -1 when unset
        const char *e = std::getenv(name);
        return e == nullptr ? -1 : e[0];
    };
    if (const char *e = std::getenv("PFBHIP_SCATTER")) {
        const std::string v(e);
        if (v == "auto") sw.scatter = ScatterForce::Auto;
        else if (v == "walk") sw.scatter = ScatterForce::Walk;
        else if (v == "block") sw.scatter = ScatterForce::Block;
        else if (v == "rec") sw.scatter = ScatterForce::Rec;
        else if (v == "rec_es") sw.scatter = ScatterForce::RecEs;
        else PFB_REQUIRE(false, "PFBHIP_SCATTER=%s: expected auto, walk, block, rec or rec_es", e);
    }
    sw.wmode2 = first("PFBHIP_WMODE2") != '0';
    sw.wd_block4 = first("PFBHIP_WD_BLOCK") == '4';
    const int wc = first("PFBHIP_WD_COLOURS");
    sw.wd_colours = wc == '0' ? 0 : (wc == '1' ? 1 : -1);
    sw.rowfft = first("PFBHIP_ROWFFT") != '0';
    sw.fused_fft = first("PFBHIP_FUSED_FFT") != '0';
    const int fd = first("PFBHIP_FUSED_DOUBLED");
    sw.fused_doubled = fd < 0 ? -1 : (fd == '1' ? 1 : 0);
    sw.sepscreen = first("PFBHIP_SEPSCREEN") != '0';
    sw.tfft = first("PFBHIP_TFFT") != '0';
    sw.wd_fused = first("PFBHIP_WD_FUSED") != '0';
    return sw;
}

// ---- the plan's path (PlanPath), step 1: sort key layout ----
// The register-footprint scatters walk runs of visibilities whose footprint origins share a 4 x 4-cell block: the sort key carries
// that block (key_sub 64) unless PFBHIP_SCATTER=walk or the key would not fit 32 bits.  At W = 14 / 15 the scatters' 16 x 16-cell
// register frame is anchored on 2 x 2-cell blocks (k_grid_blk, k_grid_rec, k_grid_wd), and the key carries those as well (256);
// PFBHIP_WD_BLOCK=4 keeps the 4 x 4 anchoring (17 / 18-cell frame on 3 x 20 lanes).  ES-plane plans whose (tile, plane, block)
// key would not fit 32 bits (C5: 409 600 tiles x 64 planes) stay on 4 x 4 blocks.
static int sort_key_sub(const PlanSwitches &sw, int W, int64_t nkeys)
{
    if (sw.scatter == ScatterForce::Walk || nkeys * 64 >= (int64_t(1) << 32) - 2) return 1;
    const bool fine = (W == 14 || W == 15) && !sw.wd_block4 && nkeys * 256 < (int64_t(1) << 32) - 2;
    return fine ? 256 : 64;
}

// ---- step 2: the scatter and gather kernels, once the work lists exist ----
struct WorkShape {
    int key_sub;           // sort_key_sub
    size_t nwork;          // work items of all passes
    size_t per_pass;       // mean work items per pass
    size_t coarse_per_pass;  // mean work items per pass at CHUNK visibilities each
    size_t grid_bytes;     // the plane buffer of one pass
};
static PlanPath choose_kernels(const PlanSwitches &sw, const pfbhip_gridder_params &prm, const pfbhip_gridder_info &info, int kp_max,
                               const WorkShape &ws)
{
    PlanPath p;
    p.bc = wd_block_edge(int(info.W), ws.key_sub == 256);
    bool blk = ws.key_sub > 1;  // without the block order in the 32-bit key the runs are ~1 long: the walk kernel is cheaper
    // Small plans (C1: ~300 work items) run faster on the single-launch walk kernel: four colour launches of a few dozen
    // workgroups each leave most of the 256 CUs idle.  (One-plane scheme, round 4 size sweep: one launch with the atomic flush
    // wins up to 4096^2 / 4e6 visibilities = 5 000 tiles in use, ties at 6144^2 = 11 000, loses at C2 = 20 000: 2.44 vs 2.31 ms.)
    // The block order of the sort is kept either way (any order is valid).  (Mean over the passes: the first and last pass of an
    // ES-plane plan hold the few visibilities at the ends of the w range -- their launches are short whichever kernel runs them.)
    bool one_launch = false;
    if (info.wmode == 2) {
        PFB_REQUIRE(blk, "the one-plane w-scheme needs the block-ordered sort");
        // (PFBHIP_WD_COLOURS=1: the four colour launches whatever the size -- tests; 0: one launch with the atomic flush)
        one_launch = sw.wd_colours < 0 ? ws.coarse_per_pass < size_t(8192) : sw.wd_colours == 0;
    } else if (blk && sw.scatter == ScatterForce::Auto && ws.per_pass < size_t(2048)) {
        blk = false;
    }
    // colour launches need whole tile pairs on both axes: with odd tile counts the periodic wrap puts two tiles of one colour
    // next to each other
    p.coloured = blk && !one_launch && ceil_div(info.nu, TILE) % 2 == 0 && ceil_div(info.nv, TILE) % 2 == 0 && info.nu % TILE == 0 &&
                 info.nv % TILE == 0;
    const bool has_work = info.nactive > 0 && ws.nwork > 0;
    // single-pass plans without ES-kernel w-planes: the record scatter and the row-walk gather
    const bool rec_mode = info.nplanes <= kp_max && (!prm.do_wgridding || info.wmode >= 1) && has_work;
    // ES-kernel plane stacks (round 3): the record scatter with the values of each pass written by k_plane_values_es in front of
    // it, ONLY with PFBHIP_SCATTER=rec_es.  Measured (gpurun_out/r03w, r03x): 8192^2 image, 19 planes, 9.5e6 visibilities: scatter
    // 21.2 -> 17.8 ms, + 1.4 ms of plane values (88 bytes per visibility and pass), apply 73.2 -> 70.9 ms; C5: 195 -> 190 ms,
    // + 13 ms of plane values, apply 1035 -> 1044 ms -- there the scatter waits on the records / values of 1e8 visibilities
    // (6 GB per pass set) whichever kernel runs.  Round 4b: with the 16 x 16-cell frame (W <= 13, or W = 14 / 15 on the finer sort key) and
    // its paired kernel evaluation the record form is 16 % ahead of k_grid_blk at 8192^2 / 19 planes (17.2 + 1.5 against 20.4 ms, apply
    // 69.9 against 72.2); at C5 (4 x 4 blocks: the key does not fit) it is 6.5 % ahead and the plane values eat that (1038.6 against
    // 1033.3 ms).  Default: the record form where the 16 x 16 frame applies and the plan is not C5's size; k_grid_blk otherwise.
    const bool rec_es_auto = sw.scatter == ScatterForce::Auto && blk_frame16(int(info.W), p.bc) && info.nactive <= int64_t(30000000);
    // (polynomial planes in several passes -- 5 to 10 planes, moderate omega -- can take the same route, k_plane_values in front of each
    // pass's scatter, on request only: 4096^2 / 10 planes, grid 3.70 + 0.37 ms of plane values against 4.20 for k_grid_blk, apply 13.05
    // against 13.02 ms -- every visibility is in every pass there, so the values pass costs what the kernel gains)
    const bool multi_poly = info.wmode == 1 && info.nplanes > kp_max;
    const bool rec_es = prm.do_wgridding && has_work &&
                        ((info.wmode == 0 && (sw.scatter == ScatterForce::RecEs || rec_es_auto)) ||
                         (multi_poly && sw.scatter == ScatterForce::RecEs));
    const bool rec = (rec_mode || rec_es) && blk && sw.scatter != ScatterForce::Block;
    p.scatter = !blk ? Scatter::Walk : info.wmode == 2 ? Scatter::OnePlane : rec ? Scatter::Rec : Scatter::Block;
    p.gather = info.wmode == 2 ? Gather::OnePlane : rec_mode ? Gather::RowWalk : Gather::Walk;
    // one pass over the planes (otherwise the buffer is reused inside the apply) and a second buffer of <= 40 GB
    p.side_clear = info.nplanes <= kp_max && has_work && ws.grid_bytes <= (size_t(40) << 30);
    // one-plane coloured plans (wd_hessian_supported): a Hessian apply runs k_hess_wd per colour instead of the gather and the
    // four scatter launches
    p.hess_fused = sw.wd_fused && info.wmode == 2 && p.coloured && p.side_clear && info.nplanes == 1 &&
                   wd_hessian_supported(int(info.W), p.bc);
    p.gather_values = rec_mode && rec && !p.hess_fused;
    return p;
}

// ---- step 3: the plane transforms, once the row-FFT plans exist ----
// (doubled first-axis shapes transpose only where the waiting half transform is parked in LDS -- 20480 points)
static bool transposing_possible(bool fused, const RowFFT &rv) { return fused && rv.ok && (!rv.pl.doubled || fused_doubled_stashes(rv)); }
static PlanPath choose_transforms(PlanPath p, const PlanSwitches &sw, const pfbhip_gridder_params &prm, const RowFFT &ru,
                                  const RowFFT &rv, int npoly, bool has_work)
{
    // Doubled shapes (20480, 24576, 32768 points) run the plain row kernel on both axes and keep the separate pad / crop
    // kernels.  Their dedicated fused kernels (k_fused_fft_crop2 / k_fused_pad_fft2: even / odd half transforms combined
    // pair by pair) hold one half's 16 outputs across the other half's transform and still spill ~100 registers at the
    // 170-VGPR budget of a 640..1024-thread workgroup: measured 36.8 ms against 35.6 ms unfused for the second axis of
    // a 16384^2 image / 20480^2 grid with 4 planes, so they stay behind PFBHIP_FUSED_DOUBLED=1 (tests keep them alive).
    // Round 3: at 20480 points the waiting half is parked in LDS (k_fused_fft_crop2 / k_fused_pad_fft2, STASH) and the fused
    // kernels are the default; PFBHIP_FUSED_DOUBLED=0 / 1 forces the choice for every doubled shape.
    const bool fuse_doubled = sw.fused_doubled >= 0 ? sw.fused_doubled == 1 : fused_doubled_stashes(ru);
    // (the fused kernels evaluate n - 1 by the polynomial only: fields reaching 45 degrees off axis, npoly = 0, keep the
    // separate pad / crop kernels with the closed form)
    const bool fused = sw.fused_fft && ru.ok && (!ru.pl.doubled || fuse_doubled) && (!prm.do_wgridding || npoly > 0);
    p.axis2 = fused ? SecondAxis::Fused : (sw.rowfft && ru.ok) ? SecondAxis::Rows : SecondAxis::RocFFT;
    p.axis1 = (sw.tfft && has_work && transposing_possible(fused, rv)) ? FirstAxis::Transposing
              : rv.ok                                                   ? FirstAxis::Rows
                                                                        : FirstAxis::RocFFT;
    return p;
}

// the plan's path as pfbhip_gridder_info reports it
static void report_path(const PlanPath &p, pfbhip_gridder_info &info)
{
    info.scatter_mode = p.scatter == Scatter::Walk ? 0 : (p.scatter == Scatter::Block ? 1 : 2);
    info.scatter_launches = p.coloured ? 4 : 1;
    info.scatter_block = p.bc;
    info.gather_mode = p.gather == Gather::Walk ? 0 : (p.gather == Gather::RowWalk ? 1 : 2);
    info.fft_mode = (p.axis1 != FirstAxis::RocFFT ? 1 : 0) | (p.axis2 == SecondAxis::Fused ? 2 : 0) |
                    (p.axis2 == SecondAxis::Rows ? 4 : 0) | (p.axis1 == FirstAxis::Transposing ? 8 : 0);
}

// what choose_kernel decides: the kernel row, the grid, the w-scheme and its planes
struct KernelChoice {
    const KernelRow *row = nullptr;  // W, beta, sigma, eps_max of the ES kernel
    int64_t nu = 0, nv = 0, npl = 1;
    double dw = 1.0;
    int mode = 0, nder = 0;  // w-scheme (info.wmode); kernel functions per axis of the one-plane scheme
};

// ONE plane, K kernel functions per axis (gridder_kernels_wd.hpp): K = wd_K, the interpolation in
// s = l^2 + m^2 measured in choose_kernel; the aliases of the k-th derivative term carry ((1 + 2 sigma) l_max)^(2k)
// where the wanted term has <= l_max^(2k) at weight omega^k / k!: the row's worst-position error times
// that sum must still pass
static double wd_alias_amplification(double omega, int K, int64_t nu, int64_t nv, int64_t nx, int64_t ny)
{
    const double gg = std::pow(std::max(1.0 + 2.0 * double(nu) / double(nx), 1.0 + 2.0 * double(nv) / double(ny)), 2);
    double amp = 0.0, term = 1.0;
    for (int k = 0; k < K; ++k) {
        amp += term;
        term *= omega * gg / double(k + 1);
    }
    return amp;
}

// Cost of one Hessian apply (both directions), from the C2 / C5 profiles (profiles/r01g_*):
//  plane transform, per plane: hand-written row FFTs + fused second axis 2.7e-11 s per grid
//  point; rocFFT rows + separate pad / crop kernels = measured 2-D transform time + three
//  streaming passes at 5 TB/s;
//  scatter + gather: 0.30 ns per visibility and touched plane, independent of W <= 16 (the
//  diagonal walk always takes 16 steps of LDS atomics / reads).
// (x 1.2 on the rocFFT path: its measured table is for the large sizes only, and every distinct size
// costs 1-3 s of rocFFT plan building that the hand-written path does not have)
// (doubled row-FFT shapes, > 16384 points: unfused second axis, measured 3.7e-11 s per point on C5)
static double apply_cost(int W, int64_t nu, int64_t nv, bool own, double nvis, int64_t npl, int64_t touched, int nder, bool wgrid)
{
    const double own_pt = (nu > 16384 || nv > 16384) ? 3.7e-11 : 2.7e-11;
    const double plane_cost = own ? own_pt * double(nu) * double(nv)
                                  : 1.2 * (fft2d_seconds(nu, nv) + 3.0 * 16.0 * double(nu) * double(nv) / 5.0e12);
    double gridcost = nvis * double(nder > 0 ? touched : std::min<int64_t>(touched, npl)) * 0.30e-9;
    // (one-plane scatter: the cells a lane holds of the block frame -- 7 rows of 3 x 20 lanes at W = 16, 4 rows of 4 x 16 lanes
    // up to W = 15 (2 x 2-cell anchoring at 14 / 15, the sort's 4 x 4 blocks below: fewer flushes) -- and the gather's W
    // steps: measured at C2, grid + degrid W = 16: 2.38 + 1.66 ms, W = 15: 1.88 + 1.63, relative to the 3.9 ms the
    // constant above was last checked against)
    if (nder > 0) gridcost *= W >= 16 ? 1.03 : (W >= 14 ? 0.90 : 0.87);
    // (the multi-plane register-footprint scatters hold the same frames: 4 cells per lane up to W = 15 against 7 at W = 16 --
    // k_grid_rec at C2 on three polynomial planes, W = 16: grid 2.31 of 4.05 ms of scatter + gather; the gathers walk 16
    // steps whatever W)
    else if (wgrid) gridcost *= W >= 16 ? 1.0 : 0.92;
    return double(npl) * plane_cost + gridcost;
}

static KernelChoice choose_kernel(const pfbhip_gridder_params &prm, const PlanSwitches &sw, int64_t nvis_all, double lshift, double mshift,
                                  double nshift, double wlo, double whi, double tmax, double nmin)
{
    size_t nrows = 0;
    const KernelRow *tab = kernel_table(&nrows);
    // admissible rows: worst-position (image-edge) 1-D error <= epsilon / ndim.  The L2 error over
    // the image is then ~4-5x smaller than requested; the stricter rule is what keeps max-norm
    // identities of the reference's tests (test_hessian_approx.py:188-231, |err|_inf <= epsilon) true.
    // divide_by_n weights a pixel's error with 1 / n: the budget shrinks by the smallest n of the image (a field reaching
    // 45 degrees off axis: 0.7; found by the fuzz sweep: 1.17e-7 at epsilon = 1e-7 for a centre at (-0.2, 0.35))
    //
    // Round 3: the test is made on eps_sup, the aliasing error at the worst SUB-CELL position of a visibility (1.2-1.5 x the
    // position-averaged eps_max), times 1.25 for the polynomial form of the kernel (admitted up to 0.25 x the row's error), and
    // against 0.8 x the share: a data set of a few dozen visibilities averages neither over positions nor over pixels, and
    // the relative L2 error of its image scatters around the per-visibility bound (the fuzz sweep's 1.2 epsilon case: 63
    // visibilities on a row admitted on eps_max with 42 % to spare).  Rows with margin -- every benchmark configuration --
    // are unaffected.
    const double eps1 = 0.8 / 1.25 * prm.epsilon / (prm.do_wgridding ? 3.0 : 2.0) *
                        ((prm.do_wgridding && prm.divide_by_n) ? std::max(0.25, std::min(1.0, nmin)) : 1.0);
    // (the interpolation bound of the polynomial w-planes is a true maximum already: it keeps its 2/3 epsilon)
    const double eps_w = 0.5 * w_interp_budget(prm, nmin);
    const double nvis = double(nvis_all);
    const bool wgrid = prm.do_wgridding && tmax > 0.0;
    const double pi = 3.14159265358979323846;
    double best_cost = 1e300;
    KernelChoice best;
    // one-plane scheme (wmode 2): phase centre on axis, the record kernels available, not switched off
    const bool wd_allowed = sw.wmode2 && lshift == 0.0 && mshift == 0.0 &&
                            (sw.scatter == ScatterForce::Auto || sw.scatter == ScatterForce::Rec);
    // its K depends on the geometry alone: the smallest K from the estimate of the polynomial scheme (at least 2) up to
    // WD_MAX_K whose measured interpolation error in s passes 2 eps_w.  0: none does, or the image reaches the horizon
    const double wd_omega = 2.0 * pi * 0.5 * (whi - wlo) * tmax;
    int wd_K = 0;
    if (wgrid && wd_allowed) {
        const int K0 = poly_planes_needed(wd_omega, 2.0 * eps_w);
        for (int K = K0; K >= 2 && K <= WD_MAX_K; ++K)
            if (wd_interp_error(K, wd_smax(prm), 0.5 * (whi - wlo), nshift) <= 2.0 * eps_w) {  // (NaN: not admitted)
                wd_K = K;
                break;
            }
    }
    for (size_t i = 0; i < nrows; ++i) {
        const KernelRow &r = tab[i];
        if (prm.force_W > 0) {
            if (r.W != prm.force_W || std::fabs(r.sigma - prm.force_sigma) > 1e-9) continue;
        } else {
            if (r.sigma < prm.sigma_min - 1e-9 || r.sigma > prm.sigma_max + 1e-9 || r.eps_sup > eps1) continue;
        }
        // Candidate grids: the smallest 2-3-5-7-smooth size >= sigma n, and the smallest size the
        // hand-written row FFT supports ({1,3,5} x 2^a) if that stays within sigma_max -- a larger grid
        // with the same (W, beta) only lowers the aliasing error.
        double rounding_es = 0.0, rounding_poly = 0.0;
        int64_t cand_u[2] = {grid_size(prm.nx, r.sigma), rowfft_size_at_least(double(prm.nx) * r.sigma)};
        int64_t cand_v[2] = {grid_size(prm.ny, r.sigma), rowfft_size_at_least(double(prm.ny) * r.sigma)};
        for (int cand = 0; cand < 2; ++cand) {
            const int64_t nu = cand_u[cand], nv = cand_v[cand];
            if (nu <= 0 || nv <= 0) continue;
            if (cand == 1 && (nu == cand_u[0] && nv == cand_v[0])) continue;
            if (cand == 1 && prm.force_W <= 0 &&
                (double(nu) > prm.sigma_max * double(prm.nx) || double(nv) > prm.sigma_max * double(prm.ny)))
                continue;
            // Rounding, the third term of the error budget (round 3; found by tools/soak_midsize.py 5, case 13): the image-side
            // correction 1 / psi amplifies the rounding errors of the grid and of the FFT, at the image corner by
            // psi(0)^2 / (psi(x_edge) psi(y_edge)), times psi(0) / psi(0.5 / sigma) of the w-kernel for ES-kernel planes.  A W = 16
            // row at sigma = 1.15 under an image that fills its grid (n / nu = 0.86) reaches 1.6e12 there, and the relative L2
            // error of the image was 4e-7 of pure rounding at epsilon = 1e-6 (2.5e-19 x the corner amplification, measured).
            // Rows whose rounding share would pass 0.2 epsilon are not admissible; the wider grids (sigma >= 1.25) every
            // epsilon <= 3e-7 needs stay below 1e-8.
            if (prm.force_W <= 0) {
                const KernelFT ft(r.W, r.beta);
                const double f0 = ft(0.0);
                double amp = (f0 / ft(0.5 * double(prm.nx) / double(nu))) * (f0 / ft(0.5 * double(prm.ny) / double(nv)));
                if (wgrid) amp = std::max(amp, amp * f0 / ft(0.5 / r.sigma));  // (ES-kernel planes; the polynomial scheme has none)
                rounding_es = 2.5e-19 * amp;
                rounding_poly = rounding_es * ft(0.5 / r.sigma) / f0;
            } else {
                rounding_es = rounding_poly = 0.0;
            }
            RowFFTPlan tmp;
            const bool own = rowfft_make_plan(nu, &tmp) && rowfft_make_plan(nv, &tmp);
            for (int mode = 0; mode < (wgrid ? 3 : 1); ++mode) {
                if (wgrid && prm.force_wmode != 0 && prm.force_wmode != mode + 1) continue;
                if ((wgrid && mode == 0 ? rounding_es : (wgrid ? rounding_poly : rounding_es)) > 0.2 * prm.epsilon) continue;
                double dw = 1.0;
                int64_t npl = 1, touched = 1;
                int nder = 0;
                if (wgrid) {
                    if (mode == 2) {
                        if (wd_K == 0) continue;
                        if (prm.force_W <= 0 && r.eps_sup * wd_alias_amplification(wd_omega, wd_K, nu, nv, prm.nx, prm.ny) > eps1) continue;
                        nder = wd_K;
                        npl = 1;
                        touched = wd_K;
                    } else if (mode == 0) {
                        dw = 0.5 / r.sigma / tmax;  // the w axis keeps the oversampling the kernel row was designed for
                        npl = int64_t((whi - wlo) / dw + r.W);
                        touched = r.W;
                    } else {
                        // The interpolation bound is a max-norm bound attained only at the extreme pixel and
                        // extreme w; its L2 average over the image and the w distribution is ~0.3x.  It gets
                        // 2/3 of epsilon: max-norm identities at the phase centre (kernel error ~0 there) still
                        // hold to epsilon, and the L2 total (2 kernels at ~eps/13 each + ~0.2 eps) stays << epsilon.
                        npl = poly_planes_needed(2.0 * pi * 0.5 * (whi - wlo) * tmax, 2.0 * eps_w);
                        if (npl == 0) continue;
                        touched = npl;
                    }
                }
                const double cost = apply_cost(r.W, nu, nv, own, nvis, npl, touched, nder, wgrid);
                // cheapest wins; within 1 % the more accurate row does (W is free up to 16, so the best row
                // that maps to the same grid and plane count usually beats the requested epsilon)
                const bool better = best.row == nullptr || cost < 0.99 * best_cost ||
                                    (cost <= 1.01 * best_cost && r.eps_sup < best.row->eps_sup);
                if (better) {
                    best_cost = std::min(cost, best_cost);
                    best = KernelChoice{&r, nu, nv, npl, dw, mode, nder};
                }
            }
        }
    }
    PFB_REQUIRE(best.row != nullptr || !(wgrid && prm.force_wmode == 3),
                "force_wmode=2: the one-plane w-scheme needs the phase centre on axis, a field of view inside the horizon "
                "(max l^2 + m^2 = %g, must be < 1) and 2..%d kernel functions for this field of view and w range (epsilon=%g); "
                "leave the scheme to the plan", wd_smax(prm), WD_MAX_K, prm.epsilon);
    PFB_REQUIRE(best.row != nullptr || !(wgrid && prm.force_wmode == 2),  // (C-ABI encoding: 0 = plan decides, wmode + 1 otherwise)
                "force_wmode=1: the polynomial w-plane scheme needs more than %d planes for this field of view and w range "
                "(epsilon=%g); leave the scheme to the plan", MAX_POLY_PLANES, prm.epsilon);
    // (the table's best row has a worst-position error of 2.3e-12; with the margins above the tightest epsilon a plan accepts is
    // ~1.1e-11 with w-gridding, ~7e-12 without, and 1 / n_min times that with divide_by_n)
    PFB_REQUIRE(best.row != nullptr, "no ES kernel reaches epsilon=%g with sigma in [%g, %g]: the tightest epsilon this kernel table admits "
                "is ~1.1e-11 with w-gridding (~7e-12 without; times 1 / min(n) with divide_by_n) at sigma_max >= 2.5",
                prm.epsilon, prm.sigma_min, prm.sigma_max);
    return best;
}

// the choice as the handle keeps it: info, the planes' w, and the Chebyshev nodes / Lagrange denominators of wmode 1
static void apply_choice(pfbhip_gridder *g, const KernelChoice &c, double wlo, double whi)
{
    const double pi = 3.14159265358979323846;
    auto &info = g->info;
    info.W = c.row->W;
    info.beta = c.row->beta;
    info.sigma = c.row->sigma;
    info.kernel_eps = c.row->eps_max;
    info.nu = c.nu;
    info.nv = c.nv;
    info.nplanes = c.npl;
    info.dw = c.dw;
    info.wmode = c.mode;
    info.nderiv = c.nder;
    info.occ_rows = 0;
    info.wcenter = 0.5 * (wlo + whi);
    info.whalf = 0.5 * (whi - wlo);
    info.wmin = (g->prm.do_wgridding && c.mode == 0) ? 0.5 * (wlo + whi) - 0.5 * double(c.npl - 1) * c.dw : 0.0;
    info.tile = TILE;
    g->wplanes.assign(size_t(c.npl), 0.0);
    if (c.mode == 0) {
        for (int64_t p = 0; p < c.npl; ++p) g->wplanes[size_t(p)] = info.wmin + double(p) * c.dw;
    } else if (c.mode == 2) {
        g->wplanes[0] = info.wcenter;
    } else {
        for (int64_t p = 0; p < c.npl; ++p) g->nodes.push_back(-std::cos(pi * (2.0 * double(p) + 1.0) / (2.0 * double(c.npl))));
        for (int64_t p = 0; p < c.npl; ++p) {
            double d = 1.0;
            for (int64_t m = 0; m < c.npl; ++m)
                if (m != p) d /= (g->nodes[size_t(p)] - g->nodes[size_t(m)]);
            g->lagr_coef.push_back(d);
            g->wplanes[size_t(p)] = info.wcenter + info.whalf * g->nodes[size_t(p)];
        }
    }
}

static void nm1_range(const pfbhip_gridder_params &p, double lshift, double mshift, double *lo, double *hi)
{
    // corners of the pixel-centre lattice plus axis crossings (cf. oracle/wgridder.py: nm1_range)
    // pixel i sits at (i - n / 2) * pixsize with INTEGER n / 2: for odd sizes the lattice runs from -(n-1)/2 to +(n-1)/2 (0.5 * n
    // put it half a pixel low: the last pixel's |n - 1| then exceeded the bound the plane spacing and the psi_w fit are built on)
    double x0 = lshift - double(p.nx / 2) * p.pixsize_x, y0 = mshift - double(p.ny / 2) * p.pixsize_y;
    std::vector<double> xs{x0, x0 + double(p.nx - 1) * p.pixsize_x}, ys{y0, y0 + double(p.ny - 1) * p.pixsize_y};
    if (xs[0] * xs[1] < 0) xs.push_back(0.0);
    if (ys[0] * ys[1] < 0) ys.push_back(0.0);
    *lo = 1e300;
    *hi = -1e300;
    for (double xc : xs)
        for (double yc : ys) {
            double t = xc * xc + yc * yc;
            double v = t <= 1.0 ? -t / (1.0 + std::sqrt(1.0 - t)) : -std::sqrt(t - 1.0) - 1.0;
            *lo = std::min(*lo, v);
            *hi = std::max(*hi, v);
        }
}

// ---------------------------------------------------------------------------------------
// plan creation, step by step (create_impl at the end): every step reads the handle and the scratch below and fills in its
// part of both.  The host combinatorics are in plan_layout.hpp.
// ---------------------------------------------------------------------------------------

// What one step of plan creation hands to a later one.  It is destroyed when creation ends: nothing of it stays in the handle.
struct PlanBuild {
    const PlanSwitches sw = read_plan_switches();
    PlanPath path;  // (g->path once complete)
    double tmax = 0.0, nm1min = 0.0;  // largest |n - 1 + nshift| and smallest n - 1 of the image
    double wlo = 0.0, whi = 0.0;      // w range of the unmasked visibilities
    bool plane_sorted = false;        // sort key (tile, first plane): a work list per pass
    // the tile sort's device buffers; the values of k_out / v_out are the sorted keys / visibility indices
    struct SortScratch {
        DevBuf<uint32_t> k_in, k_out, v_in, v_out;
        DevBuf<char> tmp;
        DevBuf<uint32_t> d_tstart;
        explicit SortScratch(size_t nvis) : k_in(nvis), k_out(nvis), v_in(nvis), v_out(nvis) {}
    };
    std::unique_ptr<SortScratch> sort;  // (sort_by_tile .. sorted_coordinates)
    std::vector<uint32_t> tstart;       // first sorted visibility of every key, nactive at the end; empty without visibilities
    WorkLists lists;                    // work items of every pass (d_work), their count at CHUNK visibilities each
    uint32_t chunk_used = CHUNK;        // visibilities per work item
    std::vector<uint8_t> occ;           // occupied 32-row blocks of the uv-plane (d_occ)
    // uploaded without a synchronisation of their own: they live until creation's last one
    std::vector<double> fc, cfu, cfv, cheb;
    size_t fft_work = 0;      // largest work buffer a rocFFT plan asks for
    bool any_rocfft = false;  // some transform runs on rocFFT
    int verbosity = 0;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();

    void lap(const char *what)  // verbosity >= 1: wall-clock of the plan-creation phases
    {
        if (verbosity < 1) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[pfbhip] plan: %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
};

// (also sets g->nvis, between the checks that bound its factors and the check of the product)
static void validate_params(pfbhip_gridder *g, const double *uvw, const double *freq)
{
    const auto &prm = g->prm;
    PFB_REQUIRE(prm.nrow >= 0 && prm.nchan >= 1, "bad visibility shape (%lld, %lld)", (long long)prm.nrow,
                (long long)prm.nchan);
    PFB_REQUIRE(prm.nx >= 2 && prm.ny >= 2 && prm.nx <= 65536 && prm.ny <= 65536, "bad image shape (%lld, %lld)",
                (long long)prm.nx, (long long)prm.ny);
    PFB_REQUIRE(prm.pixsize_x > 0 && prm.pixsize_y > 0, "pixel sizes must be positive");
    PFB_REQUIRE(prm.epsilon > 0 && prm.epsilon < 1, "epsilon must be in (0,1)");
    PFB_REQUIRE(prm.nchan < (1 << 16), "too many channels");
    g->nvis = prm.nrow * prm.nchan;
    PFB_REQUIRE(g->nvis < (int64_t(1) << 31), "too many visibilities per handle (%lld >= 2^31)", (long long)g->nvis);
    PFB_REQUIRE(uvw != nullptr || prm.nrow == 0, "uvw is NULL");
    PFB_REQUIRE(freq != nullptr, "freq is NULL");
}

// the device and the plan's stream: everything after this step is enqueued on it, inside create_impl's scope
static void open_stream(pfbhip_gridder *g)
{
    PFB_HIP(hipGetDevice(&g->device));
    PFB_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    g->timer.stream = g->stream;
}

// phase-centre geometry, the uploads of uvw / fc / mask and what of MapArgs does not depend on the kernel choice
static void setup_geometry_and_upload(pfbhip_gridder *g, PlanBuild &pb, const double *uvw, const double *freq, const uint8_t *mask)
{
    const auto &prm = g->prm;
    hipStream_t st = g->stream;
    auto &info = g->info;

    // geometry
    info.lshift = prm.flip_u ? -prm.center_x : prm.center_x;
    info.mshift = prm.flip_v ? -prm.center_y : prm.center_y;
    double nm1max;
    nm1_range(prm, info.lshift, info.mshift, &pb.nm1min, &nm1max);
    info.nshift = prm.do_wgridding ? -0.5 * (nm1max + pb.nm1min) : 0.0;
    pb.tmax = std::max(std::fabs(nm1max + info.nshift), std::fabs(pb.nm1min + info.nshift));
    g->shifting = (info.lshift != 0.0) || (info.mshift != 0.0) || (info.nshift != 0.0);

    // upload uvw / fc / mask
    const size_t nrow1 = size_t(std::max<int64_t>(prm.nrow, 1));
    g->d_uvw.alloc(nrow1 * 3);
    if (prm.nrow) PFB_HIP(hipMemcpyAsync(g->d_uvw.p, uvw, size_t(prm.nrow) * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    pb.fc.resize(size_t(prm.nchan));
    for (int64_t c = 0; c < prm.nchan; ++c) pb.fc[size_t(c)] = freq[c] / SPEED_OF_LIGHT;
    g->d_fc.alloc(size_t(prm.nchan));
    PFB_HIP(hipMemcpyAsync(g->d_fc.p, pb.fc.data(), pb.fc.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (mask && g->nvis) {
        g->d_mask.alloc(size_t(g->nvis));
        PFB_HIP(hipMemcpyAsync(g->d_mask.p, mask, size_t(g->nvis), hipMemcpyHostToDevice, st));
    }

    MapArgs &m = g->map;
    m.uvw = g->d_uvw.p;
    m.fc = g->d_fc.p;
    m.mask = g->d_mask.p;
    m.nvis = g->nvis;
    m.nchan = int(prm.nchan);
    m.su = prm.flip_u ? -1.0 : 1.0;
    m.sv = prm.flip_v ? -1.0 : 1.0;
    m.sw = prm.flip_w ? -1.0 : 1.0;
    m.px = prm.pixsize_x;
    m.py = prm.pixsize_y;
    m.do_w = prm.do_wgridding;
    m.swap_uv = 1;
}

// w range over unmasked visibilities
static void w_range(pfbhip_gridder *g, PlanBuild &pb)
{
    hipStream_t st = g->stream;
    if (g->prm.do_wgridding && g->nvis > 0) {
        const int nb = 512;
        DevBuf<double> d_mm(2 * nb);
        hipLaunchKernelGGL(k_wrange, dim3(nb), dim3(256), 0, st, g->map, d_mm.p);
        PFB_HIP(hipGetLastError());
        std::vector<double> mm(2 * nb);
        PFB_HIP(hipMemcpyAsync(mm.data(), d_mm.p, mm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        PFB_HIP(hipStreamSynchronize(st));  // mm is read here, d_mm is a local
        pb.wlo = 1e300;
        pb.whi = -1e300;
        for (int b = 0; b < nb; ++b) {
            pb.wlo = std::min(pb.wlo, mm[2 * b]);
            pb.whi = std::max(pb.whi, mm[2 * b + 1]);
        }
        if (pb.wlo > pb.whi) pb.wlo = pb.whi = 0.0;  // everything masked
    }
}

// the rest of MapArgs, the tile counts and the image / grid geometry, once the kernel and the grid are chosen
static void finish_map_args(pfbhip_gridder *g, const PlanBuild &pb)
{
    const auto &prm = g->prm;
    auto &info = g->info;
    MapArgs &m = g->map;
    m.nu = int(info.nu);
    m.nv = int(info.nv);
    m.dnu = double(info.nu);
    m.dnv = double(info.nv);
    m.ntv = int(ceil_div(info.nv, TILE));
    m.W = info.W;
    m.shift = 1.0 - 0.5 * double(info.W);
    if (info.wmode == 0) {
        m.wmin = info.wmin;
        m.xdw = 1.0 / info.dw;
    } else {  // pw = s = (w - wcenter) / whalf in [-1, 1]
        m.wmin = info.wcenter;
        m.xdw = info.whalf > 0.0 ? 1.0 / info.whalf : 0.0;
    }
    const int64_t ntu = ceil_div(info.nu, TILE);
    info.ntiles = ntu * m.ntv;

    g->geom = ImgGeom{int(prm.nx), int(prm.ny), int(info.nu), int(info.nv), int(info.nu), int(info.nv), prm.pixsize_x, prm.pixsize_y,
                      info.lshift, info.mshift, info.nshift};
    // (row pitch of the uv-plane buffer: see the B pitch in setup_transforms; rocFFT row plans on A need the dense pitch)
    RowFFTPlan probe;
    const bool own_v = pb.sw.rowfft && rowfft_make_plan(info.nv, &probe);
    g->geom.apitch = int(info.nv) + (own_v ? 8 : 0);
    g->plane_stride = size_t(info.nu) * size_t(g->geom.apitch);
}

// ---- tile sort of the unmasked visibilities: keys, radix sort, the start of every key ----
static void sort_by_tile(pfbhip_gridder *g, PlanBuild &pb)
{
    const auto &prm = g->prm;
    auto &info = g->info;
    MapArgs &m = g->map;
    hipStream_t st = g->stream;
    g->kp_max = int(std::min<int64_t>(KP_MAX, info.nplanes));
    // Wide fields (ES-kernel planes, P > W + planes per pass): a visibility touches only W of the P
    // planes.  Sorting by (tile, first plane) makes the visibilities that touch a pass's planes a
    // contiguous range per tile, so every pass gets its own, shorter work list.
    pb.plane_sorted = prm.do_wgridding && info.wmode == 0 && info.nplanes > info.W + g->kp_max - 1 &&
                      info.ntiles * info.nplanes < (int64_t(1) << 32) - 2;
    m.key_planes = pb.plane_sorted ? int(info.nplanes) : 1;
    const int64_t nkeys = info.ntiles * m.key_planes;
    m.key_sub = sort_key_sub(pb.sw, int(info.W), nkeys);
    info.nactive = 0;
    if (g->nvis == 0) return;
    pb.sort = std::make_unique<PlanBuild::SortScratch>(size_t(g->nvis));
    auto &s = *pb.sort;
    hipLaunchKernelGGL(k_keys, blocks1d(g->nvis), dim3(256), 0, st, m, s.k_in.p, s.v_in.p);
    PFB_HIP(hipGetLastError());
    size_t tmp_bytes = 0;
    PFB_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, s.k_in.p, s.k_out.p, s.v_in.p, s.v_out.p, int(g->nvis), 0,
                                               32, st));
    s.tmp.alloc(tmp_bytes);
    PFB_HIP(hipcub::DeviceRadixSort::SortPairs(s.tmp.p, tmp_bytes, s.k_in.p, s.k_out.p, s.v_in.p, s.v_out.p, int(g->nvis), 0,
                                               32, st));
    s.d_tstart.alloc(size_t(nkeys) + 1);
    hipLaunchKernelGGL(k_tile_start, blocks1d(nkeys + 1), dim3(256), 0, st, s.k_out.p, g->nvis, uint32_t(nkeys), uint32_t(m.key_sub),
                       s.d_tstart.p);
    PFB_HIP(hipGetLastError());
    pb.lap("keys + radix sort");
    pb.tstart.resize(size_t(nkeys) + 1);
    PFB_HIP(hipMemcpyAsync(pb.tstart.data(), s.d_tstart.p, pb.tstart.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PFB_HIP(hipStreamSynchronize(st));  // tstart is read from here on
    info.nactive = pb.tstart[size_t(nkeys)];
    pb.lap("tile starts");
}

// the work items of every pass
static void build_work_lists(pfbhip_gridder *g, PlanBuild &pb)
{
    const auto &info = g->info;
    if (g->nvis > 0) pb.chunk_used = gather_chunk(info.wmode, info.nactive);
    pb.lists = split_work(pb.tstart, info.ntiles, g->map.key_planes, info.nplanes, info.W, g->kp_max, pb.plane_sorted, pb.chunk_used);
    g->work_off = pb.lists.work_off;
    g->work_cnt = pb.lists.work_cnt;
    if (g->nvis > 0) pb.lap("work lists");
}

// grid coordinates and source index of the active visibilities in sorted order; the sort's buffers go
static void sorted_coordinates(pfbhip_gridder *g, PlanBuild &pb)
{
    if (g->nvis == 0) return;
    const auto &info = g->info;
    hipStream_t st = g->stream;
    const size_t na1 = size_t(std::max<int64_t>(info.nactive, 1));
    g->d_pu.alloc(na1);
    g->d_pv.alloc(na1);
    g->d_pw.alloc(na1);
    g->d_src.alloc(na1);
    if (info.nactive) {
        hipLaunchKernelGGL(k_records, blocks1d(info.nactive), dim3(256), 0, st, g->map, pb.sort->v_out.p, info.nactive, g->d_pu.p,
                           g->d_pv.p, g->d_pw.p, g->d_src.p);
        PFB_HIP(hipGetLastError());
    }
    PFB_HIP(hipStreamSynchronize(st));  // the sort's buffers are released
    pb.sort.reset();
}

// the colour slices of the work lists (d_work_col), cut to the scatter's item size
static void upload_colour_slices(pfbhip_gridder *g, const PlanBuild &pb)
{
    const auto &info = g->info;
    hipStream_t st = g->stream;
    const uint32_t schunk = scatter_chunk(info.wmode, info.nactive, pb.path.coloured, pb.chunk_used);
    ColourSlices cs = colour_slices(pb.lists.work, g->work_off, g->work_cnt, info.ntiles, g->map.ntv, pb.path.coloured, schunk, pb.chunk_used);
    g->col_off = std::move(cs.col_off);
    g->col_cnt = std::move(cs.col_cnt);
    g->d_work_col.alloc(std::max<size_t>(cs.wcol.size(), 1));
    if (!cs.wcol.empty())
        PFB_HIP(hipMemcpyAsync(g->d_work_col.p, cs.wcol.data(), cs.wcol.size() * sizeof(WorkItem), hipMemcpyHostToDevice, st));
    PFB_HIP(hipStreamSynchronize(st));  // cs.wcol is a local
}

// per-visibility records of the record scatter, the row-walk gather and the one-plane kernels; the work items (d_work)
static void build_records(pfbhip_gridder *g, const PlanBuild &pb)
{
    auto &info = g->info;
    const PlanPath &path = pb.path;
    const auto &work = pb.lists.work;
    hipStream_t st = g->stream;
    if (path.scatter == Scatter::Rec || path.scatter == Scatter::OnePlane || path.gather != Gather::Walk) {
        g->d_rec.alloc(size_t(info.nactive) + REC_PAD);
        g->d_pval.alloc((size_t(info.nactive) + REC_PAD) * size_t(info.wmode == 2 ? info.nderiv : g->kp_max));
        PFB_HIP(hipMemsetAsync(g->d_pval.p, 0, g->d_pval.bytes(), st));
        with_W(int(info.W), [&](auto w) {
            constexpr int W = decltype(w)::value;
            hipLaunchKernelGGL((k_vis_records<W>), blocks1d(info.nactive + REC_PAD), dim3(256), 0, st, int(info.nu), int(info.nv),
                               info.nactive, g->d_pu.p, g->d_pv.p, g->d_rec.p);
            PFB_HIP(hipGetLastError());
            if (path.gather == Gather::RowWalk) {
                g->d_kw.alloc((size_t(info.nactive) + REC_PAD) * size_t(g->kp_max));
                // (the planes / polynomial nodes are set by apply_choice; the work list is not needed here)
                GroupArgs ga = g->group_args(0, int(info.nplanes));
                hipLaunchKernelGGL((k_plane_weights<W>), blocks1d(info.nactive + REC_PAD), dim3(256), 0, st, ga, info.nactive, g->d_kw.p);
                PFB_HIP(hipGetLastError());
            }
        });
        PFB_HIP(hipStreamSynchronize(st));
    }
    info.nwork = int64_t(work.size());
    g->d_work.alloc(std::max<size_t>(work.size(), 1));
    if (!work.empty())  // (pb.lists.work outlives creation's last synchronisation)
        PFB_HIP(hipMemcpyAsync(g->d_work.p, work.data(), work.size() * sizeof(WorkItem), hipMemcpyHostToDevice, st));
}

// one-plane scheme: derivative tables of the kernel polynomial, interpolation nodes in s, per-visibility coefficients.
// Returns the derivative table, which the caller keeps until its upload is synchronised.
static std::vector<double> setup_one_plane(pfbhip_gridder *g, const PlanBuild &pb, const std::vector<double> &ktab)
{
    const auto &prm = g->prm;
    auto &info = g->info;
    hipStream_t st = g->stream;
    const int K = info.nderiv, W = info.W, D1 = kernel_poly_degree(W) + 1;
    WdArgs &wa = g->wd;
    wa = WdArgs{};
    wa.K = K;
    wa.W = W;
    wa.bc = pb.path.bc;
    wa.whalf = info.whalf;
    wa.nshift = info.nshift;
    std::vector<double> dtab = wd_derivative_table(ktab, K, W, D1);
    g->d_dtab.alloc(dtab.size());
    PFB_HIP(hipMemcpyAsync(g->d_dtab.p, dtab.data(), dtab.size() * sizeof(double), hipMemcpyHostToDevice, st));
    wa.dtab = g->d_dtab.p;
    const double smax = wd_smax(prm);
    info.smax = smax;
    const double au = std::pow(double(info.nu) * prm.pixsize_x / (pi_const * double(W)), 2) / smax;
    const double av = std::pow(double(info.nv) * prm.pixsize_y / (pi_const * double(W)), 2) / smax;
    for (int q = 0; q < K; ++q) {
        wa.su[q] = std::pow(-au, q);
        wa.sv[q] = std::pow(-av, q);
    }
    wd_interp_nodes(K, smax, info.nshift, wa.tq, wa.M);
    g->d_cw.alloc((size_t(info.nactive) + REC_PAD) * size_t(K));
    wa.cw = g->d_cw.p;
    wd_launch_coeffs(wa, info.nactive, g->d_pw.p, g->d_cw.p, st);
    // the interpolation in s on a dense grid of (dw, s) against the closed form: what choose_kernel admitted the plan on
    const double worst = wd_interp_error(K, smax, info.whalf, info.nshift), bound = w_interp_budget(prm, 1.0 + pb.nm1min);
    if (prm.verbosity > 0) fprintf(stderr, "[pfbhip] one-plane w-scheme: K = %d, interpolation error %.3g\n", K, worst);
    PFB_REQUIRE(worst <= bound, "one-plane w-scheme: interpolation error %g exceeds its share %g of epsilon %g", worst, bound,
                prm.epsilon);
    return dtab;
}

// ---- kernel polynomial table ----
static void upload_kernel_tables(pfbhip_gridder *g, const PlanBuild &pb)
{
    const auto &info = g->info;
    hipStream_t st = g->stream;
    double perr = 0.0;
    std::vector<double> ktab = kernel_poly_table(info.W, info.beta, &perr);
    PFB_REQUIRE(perr <= 0.25 * info.kernel_eps, "kernel polynomial too coarse (err %g vs kernel eps %g)", perr,
                info.kernel_eps);
    g->d_ktab.alloc(ktab.size());
    PFB_HIP(hipMemcpyAsync(g->d_ktab.p, ktab.data(), ktab.size() * sizeof(double), hipMemcpyHostToDevice, st));
    std::vector<double> dtab;
    if (info.wmode == 2) dtab = setup_one_plane(g, pb, ktab);
    PFB_HIP(hipStreamSynchronize(st));  // ktab and dtab are locals
}

// ---- correction image ----
static void build_correction_image(pfbhip_gridder *g, PlanBuild &pb)
{
    const auto &prm = g->prm;
    const auto &info = g->info;
    hipStream_t st = g->stream;
    const int64_t npix = prm.nx * prm.ny;
    KernelFT ft(info.W, info.beta);
    pb.cfu = ft.correction_1d(prm.nx, info.nu);
    pb.cfv = (prm.ny == prm.nx && info.nv == info.nu) ? pb.cfu : ft.correction_1d(prm.ny, info.nv);
    g->d_cfu.alloc(pb.cfu.size());
    g->d_cfv.alloc(pb.cfv.size());
    PFB_HIP(hipMemcpyAsync(g->d_cfu.p, pb.cfu.data(), pb.cfu.size() * sizeof(double), hipMemcpyHostToDevice, st));
    PFB_HIP(hipMemcpyAsync(g->d_cfv.p, pb.cfv.data(), pb.cfv.size() * sizeof(double), hipMemcpyHostToDevice, st));
    pb.cheb.assign(1, 1.0);
    double zmax = 1.0;
    const bool use_psiw = prm.do_wgridding && pb.tmax > 0.0 && info.wmode == 0;
    if (use_psiw) {
        zmax = pb.tmax * info.dw * (1.0 + 1e-12);
        pb.cheb = ft.inverse_cheb(zmax);
    }
    g->d_cheb.alloc(pb.cheb.size());
    PFB_HIP(hipMemcpyAsync(g->d_cheb.p, pb.cheb.data(), pb.cheb.size() * sizeof(double), hipMemcpyHostToDevice, st));
    g->d_corr.alloc(size_t(npix));
    hipLaunchKernelGGL(k_corr_image, blocks1d(npix), dim3(256), 0, st, g->geom, g->d_cfu.p, g->d_cfv.p, g->d_cheb.p,
                       int(pb.cheb.size()), info.dw, zmax, prm.do_wgridding ? 1 : 0, use_psiw ? 1 : 0, prm.divide_by_n,
                       g->d_corr.p);
    PFB_HIP(hipGetLastError());
}

// ---- scratch: the uv-plane buffers (and what the side-stream clear needs), image and sorted-visibility buffers ----
static void alloc_plane_buffers(pfbhip_gridder *g, PlanBuild &pb)
{
    const auto &info = g->info;
    hipStream_t st = g->stream;
    g->d_grid.alloc(g->plane_stride * size_t(g->kp_max));
    if (pb.path.side_clear) {
        g->d_grid2.alloc(g->plane_stride * size_t(g->kp_max));
        PFB_HIP(hipStreamCreateWithFlags(&g->clear_stream, hipStreamNonBlocking));
        PFB_HIP(hipEventCreateWithFlags(&g->ev_clear, hipEventDisableTiming));
        PFB_HIP(hipEventCreateWithFlags(&g->ev_start, hipEventDisableTiming));
        PFB_HIP(hipMemsetAsync(g->d_grid2.p, 0, g->d_grid2.bytes(), st));
    }
    pb.lap("uv-plane buffers");
    g->d_img.alloc(size_t(g->prm.nx * g->prm.ny));
    g->d_sval.alloc(size_t(std::max<int64_t>(info.nactive, 1)));
    g->d_sacc.alloc(size_t(std::max<int64_t>(info.nactive, 1)));
}

// screen form per pass of a fused second axis: composite polynomials of the whole phase where it is small, else the separable
// form (column table x row factor x residual polynomials; PFBHIP_SEPSCREEN=0 disables), else n - 1 and sincos per pixel and plane
static void fit_screens(pfbhip_gridder *g, const PlanBuild &pb)
{
    const auto &prm = g->prm;
    auto &info = g->info;
    hipStream_t st = g->stream;
    if (pb.path.axis2 == SecondAxis::Fused) {
        bool any_sep = false;
        for (int p0 = 0; p0 < info.nplanes; p0 += g->kp_max) {
            FusedPlanes fp;
            fp.kp = int(std::min<int64_t>(g->kp_max, info.nplanes - p0));
            for (int k = 0; k < FUSED_MAXPLANES; ++k) fp.w[k] = k < fp.kp ? g->wplanes[size_t(p0 + k)] : 0.0;
            // (the doubled shapes' kernels have the separable and the general form only)
            if (prm.do_wgridding && !g->rowfft_u.pl.doubled) fused_planes_fit(g->fgeom, fp);
            if (fp.nsc == 0 && pb.sw.sepscreen && prm.do_wgridding) fused_planes_fit(g->fgeom, fp, true);
            any_sep = any_sep || fp.sep != 0;
            g->plane_groups.push_back(fp);
        }
        if (any_sep) {
            g->d_tau.alloc(size_t(info.nplanes) * size_t(prm.nx));
            DevBuf<double> d_w(size_t(info.nplanes));
            PFB_HIP(hipMemcpyAsync(d_w.p, g->wplanes.data(), size_t(info.nplanes) * sizeof(double), hipMemcpyHostToDevice, st));
            fused_screen_table(g->fgeom, d_w.p, int(info.nplanes), g->d_tau.p, st);
            PFB_HIP(hipStreamSynchronize(st));  // d_w is a local
            for (size_t grp = 0; grp < g->plane_groups.size(); ++grp)
                g->plane_groups[grp].tau = g->d_tau.p + grp * size_t(g->kp_max) * size_t(prm.nx);
        }
        if (prm.verbosity > 0 && !g->plane_groups.empty()) {
            int n_sc = 0, n_sep = 0, nsc_max = 0;
            for (const FusedPlanes &fp : g->plane_groups) {
                n_sc += fp.nsc > 0 && !fp.sep;
                n_sep += fp.sep != 0;
                nsc_max = std::max(nsc_max, fp.nsc);
            }
            fprintf(stderr, "[pfbhip] w-screen of %zu passes: %d composite cos/sin polynomials, %d separable form, %zu general; <= %d "
                            "coefficients; n - 1 polynomial %d\n",
                    g->plane_groups.size(), n_sc, n_sep, g->plane_groups.size() - size_t(n_sc + n_sep), nsc_max, g->fgeom.npoly);
        }
    }
    info.screen_poly = g->fgeom.npoly;
    info.screen_composite = info.screen_separable = 0;
    for (const FusedPlanes &fp : g->plane_groups) {
        info.screen_composite += (fp.nsc > 0 && !fp.sep) ? 1 : 0;
        info.screen_separable += fp.sep ? 1 : 0;
    }
}

// Plane transforms: hand-written row FFT (rowfft.hpp) where the padded sizes are of the form
// {1,3,5} x 2^a (every size grid_size() prefers), with the pad / crop / w-screen of the second axis
// fused into its load / store; rocFFT row plans otherwise.  PFBHIP_FUSED_FFT=0 / PFBHIP_ROWFFT=0
// force the rocFFT paths (used by the tests to keep both alive).
static void setup_transforms(pfbhip_gridder *g, PlanBuild &pb)
{
    const auto &prm = g->prm;
    auto &info = g->info;
    const PlanSwitches &sw = pb.sw;
    if (sw.rowfft || sw.fused_fft) (void)g->rowfft_u.init(info.nu);
    if (sw.rowfft) (void)g->rowfft_v.init(info.nv);
    {  // the screen geometry serves the fused kernels and the separate pad / crop kernels alike
        FusedGeom &fg = g->fgeom;
        fg.nx = int(prm.nx);
        fg.ny = int(prm.ny);
        fg.nu = int(info.nu);
        fg.px = prm.pixsize_x;
        fg.py = prm.pixsize_y;
        fg.lshift = info.lshift;
        fg.mshift = info.mshift;
        fg.nshift = info.nshift;
        if (prm.do_wgridding) fused_geom_fit(fg);
        if (prm.verbosity > 0) fprintf(stderr, "[pfbhip] w-screen: n-1 polynomial with %d coefficients\n", fg.npoly);
    }
    pb.path = choose_transforms(pb.path, sw, prm, g->rowfft_u, g->rowfft_v, g->fgeom.npoly, !pb.lists.work.empty());
    g->path = pb.path;
    report_path(pb.path, info);
    const bool fused = pb.path.axis2 == SecondAxis::Fused;
    if (pb.path.axis2 == SecondAxis::RocFFT) g->rowfft_u.release();
    fit_screens(g, pb);
    // Row pitch of B.  A workgroup of the transposing first-axis FFT touches B[y][u] for one u and every y: with a pitch of
    // nu * 16 bytes (a multiple of 2^15 for every size the plan picks) all of a row's 16-byte pieces fall on one L2 /
    // memory channel.  8 more elements (128 bytes) per row walk the channels instead (the rocFFT second axis needs the dense
    // pitch).
    g->geom.bpitch = int(info.nu) + (fused ? 8 : 0);
    g->fgeom.bpitch = g->geom.bpitch;
    g->bstride = size_t(prm.ny) * size_t(g->geom.bpitch);
    // Degridding side of the transposing first-axis FFT: the fused pad kernel stores Bt[u][y] (scattered 16-byte stores that
    // meet in L2, as on the gridding side) and the first-axis transform of row u reads its row of Bt contiguously -- a
    // 16-byte GATHER in that transform's load phase cost 0.3 ms per plane at C2, scattered stores cost 0.1.  The pitch is
    // kept off the power of two for the same reason as bpitch (40 more elements: whole 128-byte lines).  (B is sized for that
    // layout wherever the transposing first axis could run, whether or not the plan takes it.)
    g->fgeom.tpitch = pb.path.axis1 == FirstAxis::Transposing ? int(prm.ny) + 40 : 0;  // (0: the tile-transpose kernels read B[y][u])
    if (transposing_possible(fused, g->rowfft_v)) g->bstride = std::max(g->bstride, size_t(info.nu) * size_t(prm.ny + 40));
    pb.lap("row-FFT tables + w-screens");
    g->d_gridB.alloc(g->bstride * size_t(fused ? g->kp_max : 1));
    g->d_accT.alloc(size_t(prm.nx * prm.ny));
    pb.lap("intermediate plane + image buffers");
}

// Which parts of the uv-plane the work items' footprints reach: 32-row blocks (d_occ) and their spans, and per tile row the
// column runs of touched tiles.  The transposing first-axis transforms load / store only these (d_colruns: RunLoad /
// RunStore), so they are also what has to be cleared of the scatter's planes (d_clear_rects: side-stream clear of
// single-pass plans, clear_planes()).
static void setup_occupancy(pfbhip_gridder *g, PlanBuild &pb)
{
    const auto &prm = g->prm;
    auto &info = g->info;
    const auto &work = pb.lists.work;
    hipStream_t st = g->stream;
    pb.occ = row_block_occupancy(work, g->map.ntv, info.nu, info.W);
    std::vector<uint8_t> touched;
    try {
        touched = touched_tiles(work, info.ntiles, g->map.ntv, info.nu, info.nv, info.W);
    } catch (const LayoutError &e) {
        PFB_REQUIRE(false, "%s", e.what());
    }
    const ColumnRuns cr = column_runs(touched, info.nu, info.nv, g->map.ntv);
    static_assert(sizeof(Int4) == sizeof(int4) && alignof(Int4) == alignof(int4), "Int4 is uploaded as int4");
    if (!work.empty()) {
        info.used_cells = cr.cells;
        if (!cr.rects.empty() && cr.cells * 10 < cr.full * 8) {  // (fragmented or nearly full coverage: plain memsets of whole rows)
            g->d_clear_rects.alloc(cr.rects.size());
            PFB_HIP(hipMemcpyAsync(g->d_clear_rects.p, cr.rects.data(), cr.rects.size() * sizeof(int4), hipMemcpyHostToDevice, st));
            PFB_HIP(hipStreamSynchronize(st));  // (as before the split; cr.rects lives to the end of this step)
            // (the plain first-axis transform runs IN PLACE on the scatter's planes: whole rows to clear)
            if (pb.path.axis1 == FirstAxis::Transposing) g->n_clear_rects = int(cr.rects.size());
        }
        if (prm.verbosity > 0)
            fprintf(stderr, "[pfbhip] scatter-plane clear: %lld of %lld cells in %zu rectangles\n", (long long)cr.cells,
                    (long long)cr.full, cr.rects.size());
    }
    g->d_colruns.alloc(cr.runs_t.size());
    PFB_HIP(hipMemcpyAsync(g->d_colruns.p, cr.runs_t.data(), cr.runs_t.size() * sizeof(int4), hipMemcpyHostToDevice, st));
    PFB_HIP(hipStreamSynchronize(st));  // cr is a local
    // spans of consecutive occupied blocks (at most a handful for a centrally concentrated uv coverage)
    for (auto &r : occupied_spans(pb.occ, info.nu)) {
        pfbhip_gridder::RowSpan sp;
        sp.row0 = r.first;
        sp.nrows = r.second;
        g->occ_rows += sp.nrows;
        g->spans.push_back(sp);
    }
    info.occ_rows = int32_t(g->occ_rows);
    g->d_occ.alloc(pb.occ.size());  // (pb.occ outlives creation's last synchronisation)
    PFB_HIP(hipMemcpyAsync(g->d_occ.p, pb.occ.data(), pb.occ.size(), hipMemcpyHostToDevice, st));
}

static rocfft_plan make_row_plan(PlanBuild &pb, int64_t len, int64_t batch, bool forward)
{
    rocfft_setup_once();
    pb.any_rocfft = true;
    rocfft_plan pl = nullptr;
    size_t lengths[1] = {size_t(len)};
    rocfft_status status = rocfft_status_success;
    // (rocFFT allocates inside plan creation: on failure the cache of released blocks gives way, once)
    if (!retry_after_cache_flush([&] {
            status = rocfft_plan_create(&pl, rocfft_placement_inplace,
                                        forward ? rocfft_transform_type_complex_forward : rocfft_transform_type_complex_inverse,
                                        rocfft_precision_double, 1, lengths, size_t(batch), nullptr);
            return status == rocfft_status_success;
        }))
        PFB_ROCFFT(status);
    size_t w = 0;
    PFB_ROCFFT(rocfft_plan_get_work_buffer_size(pl, &w));
    pb.fft_work = std::max(pb.fft_work, w);
    return pl;
}

// rocFFT row plans where the hand-written row FFT does not take the axis: per span of occupied rows, and for the rows of B
static void make_rocfft_plans(pfbhip_gridder *g, PlanBuild &pb)
{
    const auto &info = g->info;
    if (pb.path.axis1 == FirstAxis::RocFFT)
        for (auto &sp : g->spans) {
            sp.fwd = make_row_plan(pb, info.nv, sp.nrows, true);
            sp.bwd = make_row_plan(pb, info.nv, sp.nrows, false);
        }
    if (pb.path.axis2 == SecondAxis::RocFFT) {  // second axis on rocFFT only if the hand-written FFT does not take nu
        g->fftB_fwd = make_row_plan(pb, info.nu, g->prm.ny, true);
        g->fftB_bwd = make_row_plan(pb, info.nu, g->prm.ny, false);
    }
}

// the row every workgroup of the transposing first-axis transforms takes (d_rowmap)
static void upload_row_map(pfbhip_gridder *g, const PlanBuild &pb)
{
    if (pb.path.axis1 != FirstAxis::Transposing) return;
    std::vector<std::pair<int64_t, int64_t>> spans;
    for (auto &sp : g->spans) spans.emplace_back(sp.row0, sp.nrows);
    const std::vector<int> map = xcd_row_map(spans);
    g->d_rowmap.alloc(map.size());
    PFB_HIP(hipMemcpyAsync(g->d_rowmap.p, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice, g->stream));
    PFB_HIP(hipStreamSynchronize(g->stream));  // map is a local
}

// rocFFT's execution info, and the one clear of the scatter's planes
static void finish_rocfft_and_clear(pfbhip_gridder *g, const PlanBuild &pb)
{
    hipStream_t st = g->stream;
    if (pb.any_rocfft) {
        PFB_ROCFFT(rocfft_execution_info_create(&g->fft_info));
        if (pb.fft_work) {
            g->d_fftwork.alloc(pb.fft_work);
            PFB_ROCFFT(rocfft_execution_info_set_work_buffer(g->fft_info, g->d_fftwork.p, pb.fft_work));
        }
        PFB_ROCFFT(rocfft_execution_info_set_stream(g->fft_info, st));
    }
    // rows of A outside the occupied spans are never written: clear the plane once
    PFB_HIP(hipMemsetAsync(g->d_grid.p, 0, g->d_grid.bytes(), st));
}

// Runs once per handle (pfbhip_gridder_create), on a freshly constructed one that the caller owns.  Several steps upload
// vectors of pb, or the caller's arrays, without a wait of their own: pb is declared in front of the scope, whose wait is
// the one they rely on -- also when a later step throws.
static void create_impl(pfbhip_gridder *g, const double *uvw, const double *freq, const uint8_t *mask)
{
    const auto &prm = g->prm;
    auto &info = g->info;
    PlanBuild pb;
    pb.verbosity = prm.verbosity;
    validate_params(g, uvw, freq);
    open_stream(g);
    synced(g->stream, [&] {
        setup_geometry_and_upload(g, pb, uvw, freq, mask);
        w_range(g, pb);
        pb.lap("upload + w range");
        const KernelChoice choice = choose_kernel(prm, pb.sw, g->nvis, info.lshift, info.mshift, info.nshift, pb.wlo, pb.whi, pb.tmax,
                                                  1.0 + pb.nm1min);
        apply_choice(g, choice, pb.wlo, pb.whi);
        PFB_REQUIRE(info.nplanes >= 1 && info.nplanes < 100000, "unreasonable number of w-planes (%lld)",
                    (long long)info.nplanes);
        finish_map_args(g, pb);
        sort_by_tile(g, pb);
        build_work_lists(g, pb);
        sorted_coordinates(g, pb);
        {  // step 2 of the plan's path: the scatter and gather kernels
            const size_t nwork = pb.lists.work.size(), npass = std::max<size_t>(g->work_cnt.size(), 1);
            const WorkShape ws{g->map.key_sub, nwork, nwork / npass, pb.lists.coarse_items / npass,
                               g->plane_stride * size_t(g->kp_max) * sizeof(double2)};
            pb.path = choose_kernels(pb.sw, prm, info, g->kp_max, ws);
        }
        upload_colour_slices(g, pb);
        build_records(g, pb);
        pb.lap("records");
        upload_kernel_tables(g, pb);
        build_correction_image(g, pb);
        pb.lap("kernel table + correction");
        alloc_plane_buffers(g, pb);
        setup_transforms(g, pb);
        setup_occupancy(g, pb);
        make_rocfft_plans(g, pb);
        upload_row_map(g, pb);
        pb.lap("occupancy, column runs, row map");
        finish_rocfft_and_clear(g, pb);
    });
    pb.lap("rocFFT plans + plane clear");
    info.device_bytes = g->device_bytes();
}

}  // namespace pfbhip

// ---------------------------------------------------------------------------------------
// bodies of the C-ABI entries.  The *_host templates are the double and single-precision host entries themselves (T = double,
// float: only pfbhip_gridder::upload / download differ): they check their arguments, then run everything they enqueue inside
// one synced().  The other functions here run inside an entry's scope and leave the final wait to it.
// ---------------------------------------------------------------------------------------

// sval = the caller's row-ordered (nrow, nchan) device arrays in tile-sorted order, weighted with wgt_dev unless it is NULL,
// phase-shifted
static void permute_in_rows(pfbhip_gridder *g, const double2 *vis_dev, const double *wgt_dev)
{
    if (g->info.nactive)
        hipLaunchKernelGGL(k_permute_in, blocks1d(g->info.nactive), dim3(256), 0, g->stream, g->map, g->d_src.p, g->info.nactive,
                           vis_dev, wgt_dev, int(g->shifting), g->info.lshift, g->info.mshift, g->info.nshift, g->d_sval.p);
    PFB_HIP(hipGetLastError());
}

// the same of the uploaded visibilities (d_vis), weighted with d_wgt if `weighted`
static void permute_in(pfbhip_gridder *g, bool weighted)
{
    permute_in_rows(g, g->d_vis.p, weighted ? g->d_wgt.p : nullptr);
}

// the caller's host visibilities (weighted with wgt_host unless it is NULL) -> the dirty image at dirty_dev, resident in HBM
template <class T>
static void vis2dirty_upload(pfbhip_gridder *g, const T *vis_host, const T *wgt_host, double *dirty_dev)
{
    g->upload_vis_wgt(vis_host, wgt_host);
    permute_in(g, wgt_host != nullptr);
    g->grid_and_finalize(ApplyState{g->d_grid.p}, g->d_sval.p, nullptr, 1.0, 0.0, nullptr, dirty_dev);
}

template <class T>
static void vis2dirty_host(pfbhip_gridder *g, const T *vis_host, const T *wgt_host, T *dirty_host)
{
    PFB_REQUIRE(g && dirty_host && (vis_host || g->nvis == 0), "NULL argument");
    synced(g->stream, [&] {
        vis2dirty_upload(g, vis_host, wgt_host, g->d_img.p);
        g->download(g->d_img.p, size_t(g->prm.nx * g->prm.ny), dirty_host);
    });
}

// the degrid of an image resident in HBM and the un-sort of its visibilities into the caller's (nrow, nchan) order
template <class T>
static void degrid_to_host(pfbhip_gridder *g, const double *img_dev, const T *wgt_host, T *vis_host)
{
    hipStream_t st = g->stream;
    g->upload_vis_wgt<T>(nullptr, wgt_host);
    ApplyState a{g->d_grid.p};
    g->prepare_and_degrid(a, img_dev, nullptr, g->d_sacc.p);
    if (g->nvis) {
        g->d_vis.ensure(size_t(g->nvis));
        PFB_HIP(hipMemsetAsync(g->d_vis.p, 0, size_t(g->nvis) * sizeof(double2), st));
        if (g->info.nactive)
            hipLaunchKernelGGL(k_permute_out, blocks1d(g->info.nactive), dim3(256), 0, st, g->map, g->d_src.p, g->info.nactive,
                               g->d_sacc.p, wgt_host ? g->d_wgt.p : nullptr, int(g->shifting), g->info.lshift, g->info.mshift,
                               g->info.nshift, g->d_vis.p);
        PFB_HIP(hipGetLastError());
        g->download(reinterpret_cast<const double *>(g->d_vis.p), size_t(g->nvis) * 2, vis_host);
    }
}

template <class T>
static void dirty2vis_host(pfbhip_gridder *g, const T *dirty_host, const T *wgt_host, T *vis_host)
{
    PFB_REQUIRE(g && dirty_host && (vis_host || g->nvis == 0), "NULL argument");
    synced(g->stream, [&] {
        g->upload(dirty_host, size_t(g->prm.nx * g->prm.ny), g->d_img.p);
        degrid_to_host(g, g->d_img.p, wgt_host, vis_host);
    });
}

// d_swgt = the weights of the Hessian applies in tile-sorted order (ones where wgt_dev is NULL)
static void bind_weights(pfbhip_gridder *g, const double *wgt_dev)
{
    g->d_swgt.ensure(size_t(std::max<int64_t>(g->info.nactive, 1)));
    if (g->info.nactive)
        hipLaunchKernelGGL(k_gather_f64, blocks1d(g->info.nactive), dim3(256), 0, g->stream, g->d_src.p, g->info.nactive, wgt_dev,
                           g->d_swgt.p);
    PFB_HIP(hipGetLastError());
}

template <class T>
static void set_weights_host(pfbhip_gridder *g, const T *wgt_host)
{
    PFB_REQUIRE(g, "NULL handle");
    synced(g->stream, [&] {
        g->upload_vis_wgt<T>(nullptr, wgt_host);
        bind_weights(g, wgt_host ? g->d_wgt.p : nullptr);
    });
    g->weights_bound = true;
}

// out = beam_out * R^H W R (beam_in * x) * scale + eta * addend   (every image resident in HBM; beams and addend may be NULL)
static void apply_op(pfbhip_gridder *g, const double *x_dev, const double *beam_dev, const double *beam_out_dev, double scale,
                     double eta, const double *addend_dev, double *out_dev)
{
    PFB_REQUIRE(g->weights_bound, "call pfbhip_gridder_set_weights before the Hessian");
    const PlanPath &path = g->path;
    ApplyState a{g->d_grid.p};
    // the scatter's planes (second buffer) are cleared on the side stream while the degrid half runs (the gather is LDS /
    // VALU-bound: the clear's HBM traffic is free there): see side_clear()
    a.side = path.side_clear ? SideClear::Pending : SideClear::None;
    // record scatter: the gather's epilogue writes the weighted, plane-weighted model visibilities (no sacc, no scaling pass)
    a.gather_values = path.gather_values;
    // one-plane coloured plans: no gather launch; the scatter half's launches gather from d_grid themselves (k_hess_wd)
    a.hess_fused = path.hess_fused;
    g->prepare_and_degrid(a, x_dev, beam_dev, g->d_sacc.p);
    PFB_REQUIRE(!a.hess_fused || a.side == SideClear::Done, "fused Hessian: the output plane was not cleared");
    if (!a.gather_values && !a.hess_fused) {
        g->timer.begin(ST_OTHER);
        if (g->info.nactive)
            hipLaunchKernelGGL(k_scale_sorted, blocks1d(g->info.nactive), dim3(256), 0, g->stream, g->info.nactive, g->d_sacc.p,
                               g->d_swgt.p, g->d_sval.p);
        PFB_HIP(hipGetLastError());
        g->timer.end();
    }
    if (a.side == SideClear::Done) {
        PFB_HIP(hipStreamWaitEvent(g->stream, g->ev_clear, 0));
        a.out = g->d_grid2.p;
    }
    g->grid_and_finalize(a, g->d_sval.p, beam_out_dev, scale, eta, (eta != 0.0) ? addend_dev : nullptr, out_dev);
}

static void hessian_dev_impl(pfbhip_gridder *g, const double *x_dev, const double *beam_dev, double eta, double wsum,
                             double *out_dev)
{
    apply_op(g, x_dev, beam_dev, beam_dev, wsum > 0.0 ? 1.0 / wsum : 1.0, eta, eta != 0.0 ? x_dev : nullptr, out_dev);
}

template <class T>
static void hessian_host(pfbhip_gridder *g, const T *x_host, const T *beam_host, double eta, double wsum, T *out_host)
{
    PFB_REQUIRE(g && x_host && out_host, "NULL argument");
    const size_t npix = size_t(g->prm.nx * g->prm.ny);
    synced(g->stream, [&] {
        g->d_img.ensure(npix);
        g->d_img2.ensure(npix);
        g->upload(x_host, npix, g->d_img.p);
        hessian_dev_impl(g, g->d_img.p, g->bind_beam(beam_host), eta, wsum, g->d_img2.p);
        g->download(g->d_img2.p, npix, out_host);
    });
}

// the operator of the device solvers: out = Hessian(in) with the beam (resident, or NULL), eta and wsum of the call
static auto hessian_op(pfbhip_gridder *g, const double *beam_dev, double eta, double wsum)
{
    return [=](const double *in, double *out) { hessian_dev_impl(g, in, beam_dev, eta, wsum, out); };
}

// The CG solve on images resident in HBM: x_dev holds x0 on entry (zeros unless has_x0), the solution on exit.  cg comes from
// the caller, which declares it in front of its scope.
static void cg_solve(pfbhip_gridder *g, DevCG &cg, const double *beam_dev, double eta, double wsum, const double *rhs_dev,
                     double *x_dev, int has_x0, double tol, int maxit, int minit, pfbhip_cg_info *info)
{
    PFB_REQUIRE(g->weights_bound, "call pfbhip_gridder_set_weights before the CG solve");
    if (!has_x0) PFB_HIP(hipMemsetAsync(x_dev, 0, size_t(cg.n) * sizeof(double), g->stream));
    cg.solve(hessian_op(g, beam_dev, eta, wsum), rhs_dev, x_dev, tol, maxit, minit, info);
}

// ---------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------

extern "C" {

int pfbhip_gridder_create(const pfbhip_gridder_params *params, const double *uvw_host, const double *freq_host,
                          const uint8_t *mask_host, pfbhip_gridder **out)
{
    return guarded([&] {
        PFB_REQUIRE(params && out, "NULL argument");
        std::unique_ptr<pfbhip_gridder> g(new pfbhip_gridder);
        // The plan runs the transposed problem: with u <-> v exchanged the pipeline's transposed accumulator
        // (ny', nx') is the caller's (nx, ny) layout, so no image transposes are needed on either side.
        g->uprm = *params;
        g->prm = *params;
        std::swap(g->prm.nx, g->prm.ny);
        std::swap(g->prm.pixsize_x, g->prm.pixsize_y);
        std::swap(g->prm.center_x, g->prm.center_y);
        std::swap(g->prm.flip_u, g->prm.flip_v);
        create_impl(g.get(), uvw_host, freq_host, mask_host);
        *out = g.release();
    });
}

int pfbhip_gridder_destroy(pfbhip_gridder *g)
{
    return guarded([&] { delete g; });
}

int pfbhip_gridder_get_info(const pfbhip_gridder *g, pfbhip_gridder_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(g && info, "NULL argument");
        *info = g->info;
        std::swap(info->nu, info->nv);          // report the caller's orientation (the plan holds the transposed problem)
        std::swap(info->lshift, info->mshift);
        info->device_bytes = g->device_bytes();
        info->reserved0 = info->reserved1 = 0;
    });
}

int pfbhip_gridder_get_planes(const pfbhip_gridder *g, double *w_host)
{
    return guarded([&] {
        PFB_REQUIRE(g && w_host, "NULL argument");
        for (size_t p = 0; p < g->wplanes.size(); ++p) w_host[p] = g->wplanes[p];
    });
}

int pfbhip_gridder_get_binmap(pfbhip_gridder *g, int32_t *iu0, int32_t *iv0, int32_t *p0, uint8_t *flip, int64_t *order)
{
    return guarded([&] {
        PFB_REQUIRE(g, "NULL handle");
        hipStream_t st = g->stream;
        const int64_t n = (iu0 || iv0 || p0 || flip) ? g->nvis : 0;  // the index arrays are computed if one of them is asked for
        DevBuf<int32_t> a(n), b(n), c(n);
        DevBuf<uint8_t> f(n);
        std::vector<uint32_t> src(order ? size_t(g->info.nactive) : 0);
        synced(st, [&] {
            if (n) {
                hipLaunchKernelGGL(k_binmap, blocks1d(n), dim3(256), 0, st, g->map, a.p, b.p, c.p, f.p);
                PFB_HIP(hipGetLastError());
                // the plan's u is the caller's v
                if (iu0) PFB_HIP(hipMemcpyAsync(iu0, b.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                if (iv0) PFB_HIP(hipMemcpyAsync(iv0, a.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                if (p0) PFB_HIP(hipMemcpyAsync(p0, c.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                if (flip) PFB_HIP(hipMemcpyAsync(flip, f.p, n, hipMemcpyDeviceToHost, st));
            }
            if (!src.empty()) PFB_HIP(hipMemcpyAsync(src.data(), g->d_src.p, src.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        });
        for (size_t j = 0; j < src.size(); ++j) order[j] = int64_t(src[j] & 0x7FFFFFFFu);
    });
}

int pfbhip_gridder_vis2dirty(pfbhip_gridder *g, const double *vis_host, const double *wgt_host, double *dirty_host)
{
    return guarded([&] { vis2dirty_host(g, vis_host, wgt_host, dirty_host); });
}

int pfbhip_gridder_vis2dirty_dev(pfbhip_gridder *g, const double *vis_host, const double *wgt_host, double *dirty_dev)
{
    return guarded([&] {
        PFB_REQUIRE(g && dirty_dev && (vis_host || g->nvis == 0), "NULL argument");
        synced(g->stream, [&] { vis2dirty_upload(g, vis_host, wgt_host, dirty_dev); });
    });
}

int pfbhip_gridder_grid_plane(pfbhip_gridder *g, const double *vis_host, const double *wgt_host, int64_t plane,
                              double *grid_host)
{
    return guarded([&] {
        PFB_REQUIRE(g && grid_host && vis_host, "NULL argument");
        PFB_REQUIRE(plane >= 0 && plane < g->info.nplanes, "plane %lld out of range", (long long)plane);
        hipStream_t st = g->stream;
        std::vector<double2> tmp(g->plane_stride);
        synced(st, [&] {
            g->upload_vis_wgt(vis_host, wgt_host);
            PFB_HIP(hipMemsetAsync(g->d_grid.p, 0, g->plane_stride * sizeof(double2), st));
            if (g->info.nactive && g->info.nwork) {
                permute_in(g, wgt_host != nullptr);
                g->launch_grid(ApplyState{g->d_grid.p}, int(plane), 1, g->d_sval.p);
                PFB_HIP(hipGetLastError());
            }
            PFB_HIP(hipMemcpyAsync(tmp.data(), g->d_grid.p, g->plane_stride * sizeof(double2), hipMemcpyDeviceToHost, st));
        });
        // the plan's plane is (nv, nu) in the caller's terms: transpose on the host (debug entry)
        const int64_t pu = g->info.nu, pv = g->info.nv;  // plan rows / columns = caller's nv / nu
        double2 *out = reinterpret_cast<double2 *>(grid_host);
        for (int64_t a0 = 0; a0 < pu; a0 += 32)
            for (int64_t b0 = 0; b0 < pv; b0 += 32)
                for (int64_t a = a0; a < std::min(a0 + 32, pu); ++a)
                    for (int64_t b = b0; b < std::min(b0 + 32, pv); ++b) out[b * pu + a] = tmp[a * int64_t(g->geom.apitch) + b];
    });
}

int pfbhip_gridder_dirty2vis(pfbhip_gridder *g, const double *dirty_host, const double *wgt_host, double *vis_host)
{
    return guarded([&] { dirty2vis_host(g, dirty_host, wgt_host, vis_host); });
}

// dirty2vis of an image that is already in HBM (a rendered component model): the same degrid and un-sort, no image upload
int pfbhip_gridder_dirty2vis_dev(pfbhip_gridder *g, const double *dirty_dev, const double *wgt_host, double *vis_host)
{
    return guarded([&] {
        PFB_REQUIRE(g && dirty_dev && (vis_host || g->nvis == 0), "NULL argument");
        synced(g->stream, [&] { degrid_to_host<double>(g, dirty_dev, wgt_host, vis_host); });
    });
}

int pfbhip_gridder_set_weights(pfbhip_gridder *g, const double *wgt_host)
{
    return guarded([&] { set_weights_host(g, wgt_host); });
}

// ---- row-ordered DEVICE arrays: one correlation of a resident (ncorr, nrow, nchan) chunk (vischunk.hip).  Each entry checks
// its arguments, then enqueues everything inside one synced(), like every entry of this file. ----

// vis2dirty of gridder.py:587-614 of the reference: vis2dirty_upload without the upload
int pfbhip_gridder_vis2dirty_rows_dev(pfbhip_gridder *g, const double *vis_dev, const double *wgt_dev, double *dirty_dev)
{
    return guarded([&] {
        PFB_REQUIRE(g && dirty_dev && (vis_dev || g->nvis == 0), "NULL argument");
        synced(g->stream, [&] {
            permute_in_rows(g, reinterpret_cast<const double2 *>(vis_dev), wgt_dev);
            g->grid_and_finalize(ApplyState{g->d_grid.p}, g->d_sval.p, nullptr, 1.0, 0.0, nullptr, dirty_dev);
        });
    });
}

// The PSF of gridder.py:616-655 for the plan's own centre: the visibilities (ones, or the phase ramp of :617-622) are formed
// inside the permute kernel, see k_permute_in_psf.  ramp_sign = -1 conjugates the ramp: the snapshot imager's PSF
// visibilities (utils/stokes2im.py:354, :483-486 of the reference: freqfactor = -2 pi i f / c where grid has +2 pi i).
int pfbhip_gridder_psf_rows_signed_dev(pfbhip_gridder *g, const double *wgt_dev, double ramp_sign, double *psf_dev)
{
    return guarded([&] {
        PFB_REQUIRE(g && psf_dev, "NULL argument");
        PFB_REQUIRE(ramp_sign == 1.0 || ramp_sign == -1.0, "ramp_sign must be +1 or -1, not %g", ramp_sign);
        const double x0 = g->uprm.center_x, y0 = g->uprm.center_y;
        PFB_REQUIRE(x0 * x0 + y0 * y0 < 1.0, "phase centre (%g, %g) is not on the sphere", x0, y0);
        const double nm1 = std::sqrt(1.0 - x0 * x0 - y0 * y0) - 1.0;
        synced(g->stream, [&] {
            if (g->info.nactive)
                hipLaunchKernelGGL(k_permute_in_psf, blocks1d(g->info.nactive), dim3(256), 0, g->stream, g->map, g->d_src.p,
                                   g->info.nactive, wgt_dev, int(x0 != 0.0 || y0 != 0.0), ramp_sign * x0, ramp_sign * y0, ramp_sign * nm1,
                                   int(g->shifting), g->info.lshift, g->info.mshift, g->info.nshift, g->d_sval.p);
            PFB_HIP(hipGetLastError());
            g->grid_and_finalize(ApplyState{g->d_grid.p}, g->d_sval.p, nullptr, 1.0, 0.0, nullptr, psf_dev);
        });
    });
}

int pfbhip_gridder_psf_rows_dev(pfbhip_gridder *g, const double *wgt_dev, double *psf_dev)
{
    return pfbhip_gridder_psf_rows_signed_dev(g, wgt_dev, 1.0, psf_dev);
}

// set_weights (the weights of hessian.py:50-89) from a resident array
int pfbhip_gridder_set_weights_dev(pfbhip_gridder *g, const double *wgt_dev)
{
    return guarded([&] {
        PFB_REQUIRE(g, "NULL handle");
        synced(g->stream, [&] { bind_weights(g, wgt_dev); });
        g->weights_bound = true;
    });
}

// The un-weighted model visibilities of gridder.py:480-507 and their subtraction from the data (:506-507) in the un-sort:
// vis = R dirty (0 on masked samples), or vis = minuend - R dirty (minuend on masked samples); vis may be minuend.
int pfbhip_gridder_dirty2vis_rows_dev(pfbhip_gridder *g, const double *dirty_dev, const double *minuend_dev, double *vis_dev)
{
    return guarded([&] {
        PFB_REQUIRE(g && dirty_dev && (vis_dev || g->nvis == 0), "NULL argument");
        synced(g->stream, [&] {
            ApplyState a{g->d_grid.p};
            g->prepare_and_degrid(a, dirty_dev, nullptr, g->d_sacc.p);
            if (g->nvis)
                hipLaunchKernelGGL(k_permute_out_rows, blocks1d(std::max(g->info.nactive, g->nvis)), dim3(256), 0, g->stream, g->map,
                                   g->d_src.p, g->info.nactive, g->d_sacc.p, reinterpret_cast<const double2 *>(minuend_dev),
                                   int(g->shifting), g->info.lshift, g->info.mshift, g->info.nshift, reinterpret_cast<double2 *>(vis_dev));
            PFB_HIP(hipGetLastError());
        });
    });
}

// The exact residual of one partition (gridder.py:962-1016 of the reference: dirty2vis of beam * model, vis2dirty with the
// imaging weights, subtracted from the dirty image): out = acc - R^H W R (beam * model), every image resident in HBM -- the
// subtraction is the eta * addend term of the fused second-axis kernel's epilogue (scale -1, eta 1), not another pass.
int pfbhip_gridder_residual_dev(pfbhip_gridder *g, const double *model_dev, const double *beam_dev, const double *acc_dev,
                                double *out_dev)
{
    return guarded([&] {
        PFB_REQUIRE(g && model_dev && acc_dev && out_dev, "NULL argument");
        PFB_REQUIRE(model_dev != out_dev, "the residual cannot overwrite the model image");
        synced(g->stream, [&] { apply_op(g, model_dev, beam_dev, nullptr, -1.0, 1.0, acc_dev, out_dev); });
    });
}

int pfbhip_gridder_hessian_dev(pfbhip_gridder *g, const double *x_dev, const double *beam_dev, double eta, double wsum,
                               double *out_dev)
{
    return guarded([&] {
        PFB_REQUIRE(g && x_dev && out_dev, "NULL argument");
        PFB_REQUIRE(x_dev != out_dev, "in-place Hessian is not supported");
        synced(g->stream, [&] { hessian_dev_impl(g, x_dev, beam_dev, eta, wsum, out_dev); });
    });
}

int pfbhip_gridder_hessian(pfbhip_gridder *g, const double *x_host, const double *beam_host, double eta, double wsum,
                           double *out_host)
{
    return guarded([&] { hessian_host(g, x_host, beam_host, eta, wsum, out_host); });
}

// ---- single-precision host arrays (precision = "single" of the reference's vis2im / im2vis, operators/gridder.py:58-100, with
// double-precision accumulation: complex64 / float32 cross PCIe, every device buffer and sum stays double) ----
int pfbhip_gridder_vis2dirty_sp(pfbhip_gridder *g, const float *vis_host, const float *wgt_host, float *dirty_host)
{
    return guarded([&] { vis2dirty_host(g, vis_host, wgt_host, dirty_host); });
}

int pfbhip_gridder_dirty2vis_sp(pfbhip_gridder *g, const float *dirty_host, const float *wgt_host, float *vis_host)
{
    return guarded([&] { dirty2vis_host(g, dirty_host, wgt_host, vis_host); });
}

int pfbhip_gridder_set_weights_sp(pfbhip_gridder *g, const float *wgt_host)
{
    return guarded([&] { set_weights_host(g, wgt_host); });
}

int pfbhip_gridder_hessian_sp(pfbhip_gridder *g, const float *x_host, const float *beam_host, double eta, double wsum,
                              float *out_host)
{
    return guarded([&] { hessian_host(g, x_host, beam_host, eta, wsum, out_host); });
}

int pfbhip_gridder_cg(pfbhip_gridder *g, const double *beam_host, double eta, double wsum, const double *rhs_host,
                      double *x_host, int has_x0, double tol, int maxit, int minit, pfbhip_cg_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(g && rhs_host && x_host, "NULL argument");
        hipStream_t st = g->stream;
        const size_t npix = size_t(g->prm.nx * g->prm.ny);
        DevBuf<double> b{npix}, x{npix};
        DevCG cg(int64_t(npix), st);
        synced(st, [&] {
            g->upload(rhs_host, npix, b.p);
            if (has_x0) g->upload(x_host, npix, x.p);
            cg_solve(g, cg, g->bind_beam(beam_host), eta, wsum, b.p, x.p, has_x0, tol, maxit, minit, info);
            g->download(x.p, npix, x_host);
        });
    });
}

int pfbhip_gridder_cg_dev(pfbhip_gridder *g, const double *beam_dev, double eta, double wsum, const double *rhs_dev, double *x_dev,
                          int has_x0, double tol, int maxit, int minit, pfbhip_cg_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(g && rhs_dev && x_dev, "NULL argument");
        DevCG cg(g->prm.nx * g->prm.ny, g->stream);
        synced(g->stream, [&] { cg_solve(g, cg, beam_dev, eta, wsum, rhs_dev, x_dev, has_x0, tol, maxit, minit, info); });
    });
}

int pfbhip_gridder_power_method(pfbhip_gridder *g, const double *beam_host, double eta, double wsum, double *b_host, double tol,
                                int maxit, pfbhip_pm_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(g && b_host && maxit >= 0, "bad arguments");
        PFB_REQUIRE(g->weights_bound, "call pfbhip_gridder_set_weights before the power method");
        hipStream_t st = g->stream;
        const size_t npix = size_t(g->prm.nx * g->prm.ny);
        DevBuf<double> bp{npix};
        DevPower pm(int64_t(npix), st);
        synced(st, [&] {
            g->upload(b_host, npix, bp.p);
            pm.run(hessian_op(g, g->bind_beam(beam_host), eta, wsum), [](double *) {}, bp.p, tol, maxit, info);
            g->download(bp.p, npix, b_host);
        });
    });
}

int pfbhip_gridder_degrid_dev(pfbhip_gridder *g, const double *dirty_dev, double *vis_sorted_dev)
{
    return guarded([&] {
        PFB_REQUIRE(g && dirty_dev && vis_sorted_dev, "NULL argument");
        synced(g->stream, [&] {
            ApplyState a{g->d_grid.p};
            g->prepare_and_degrid(a, dirty_dev, nullptr, reinterpret_cast<double2 *>(vis_sorted_dev));
        });
    });
}

int pfbhip_gridder_grid_dev(pfbhip_gridder *g, const double *vis_sorted_dev, double *dirty_dev)
{
    return guarded([&] {
        PFB_REQUIRE(g && dirty_dev && vis_sorted_dev, "NULL argument");
        synced(g->stream, [&] {
            g->grid_and_finalize(ApplyState{g->d_grid.p}, reinterpret_cast<const double2 *>(vis_sorted_dev), nullptr, 1.0, 0.0, nullptr,
                                 dirty_dev);
        });
    });
}

int pfbhip_gridder_profile(pfbhip_gridder *g, int enable)
{
    return guarded([&] {
        PFB_REQUIRE(g, "NULL handle");
        g->timer.collect(g->stage_ms, g->stage_calls);
        g->timer.enabled = enable != 0;
    });
}

int pfbhip_gridder_profile_get(pfbhip_gridder *g, double *ms, int64_t *calls, int reset)
{
    return guarded([&] {
        PFB_REQUIRE(g, "NULL handle");
        g->timer.collect(g->stage_ms, g->stage_calls);
        for (int s = 0; s < PFBHIP_NSTAGES; ++s) {
            if (ms) ms[s] = g->stage_ms[s];
            if (calls) calls[s] = g->stage_calls[s];
            if (reset) {
                g->stage_ms[s] = 0;
                g->stage_calls[s] = 0;
            }
        }
    });
}

}  // extern "C"
