// cleanbeam.hip -- the Gaussian that approximates the main lobe of a PSF, per band, on MI355X.
//
// Replaces, of the reference,
//   src/pfb_imaging/utils/misc.py:529-613   fitcleanbeam up to the solver's result
//   src/pfb_imaging/utils/misc.py:505-526   psf_errorsq, the objective
// (the swap of the axes and the pixel-size scaling of :615-625 stay in Python: utils/misc.py::_finish_cleanbeam).
//
// Two launches per call, for any number of bands:
//   k_cb_peak  the only pass over the cube: per band, partial maxima and "any non-zero" flags
//   k_cb_fit   one workgroup per band: the second stage of the peak, the main lobe by a flood fill in LDS, its moments and
//              the start point, and a projected Levenberg-Marquardt fit over the pixels of the fit disc.
// The reference labels every island of the image (scipy.ndimage.label) and keeps the centre's; here only the centre's
// component is grown, inside a window that doubles (64, 128, 256) while the lobe touches its edge.  The fit is defined as
// the minimiser of the reference's objective under its bounds, not as the point where L-BFGS-B's factr = 1e7 stops.
// Every loop has a hard cap, no workgroup waits on another, and all arithmetic is f64 in a fixed order: two calls on the
// same cube give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"

namespace pfbhip {

constexpr int CB_THREADS = 256;
constexpr int CB_WAVES = CB_THREADS / 64;
constexpr int CB_PEAK_MAX_BLOCKS = 1024;  // per band
constexpr int CB_PEAK_PER_THREAD = 16;    // elements a thread takes before another block is worth starting
constexpr int CB_WINDOW0 = 64;
constexpr int CB_NACC = 11;               // f, J^T r (3), J^T J (6, upper triangle by rows), pixel count
constexpr double CB_AXIS_FLOOR = 1e-12;
constexpr double CB_STEP_TOL = 1e-12;
constexpr double CB_PI = 3.141592653589793238462643383279502884;

// pmax[b * gridDim.x + blockIdx.x] = max over this block's share of band b (-inf when it has none), pnz = any element != 0.
__global__ __launch_bounds__(CB_THREADS) void k_cb_peak(const double *__restrict__ psf, int64_t n, double *__restrict__ pmax,
                                                         int *__restrict__ pnz)
{
    const double *src = psf + size_t(blockIdx.y) * size_t(n);
    const int64_t stride = int64_t(gridDim.x) * CB_THREADS;
    int64_t i = int64_t(blockIdx.x) * CB_THREADS + threadIdx.x;
    double m = -INFINITY;
    int nz = 0;
    for (; i + 3 * stride < n; i += 4 * stride) {  // four independent loads in flight
        const double v0 = src[i], v1 = src[i + stride], v2 = src[i + 2 * stride], v3 = src[i + 3 * stride];
        m = fmax(fmax(fmax(v0, v1), fmax(v2, v3)), m);
        nz |= (v0 != 0.0) | (v1 != 0.0) | (v2 != 0.0) | (v3 != 0.0);
    }
    for (; i < n; i += stride) {
        const double v = src[i];
        m = fmax(m, v);
        nz |= v != 0.0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        m = fmax(m, __shfl_down(m, off, 64));
        nz |= __shfl_down(nz, off, 64);
    }
    __shared__ double s_m[CB_WAVES];
    __shared__ int s_z[CB_WAVES];
    if ((threadIdx.x & 63) == 0) {
        s_m[threadIdx.x >> 6] = m;
        s_z[threadIdx.x >> 6] = nz;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CB_WAVES; ++w) {
            m = fmax(m, s_m[w]);
            nz |= s_z[w];
        }
        const size_t o = size_t(blockIdx.y) * gridDim.x + blockIdx.x;
        pmax[o] = m;
        pnz[o] = nz;
    }
}

// Block reductions whose result every thread holds, in a fixed order.  sh: CB_WAVES * K doubles.
template <int K, bool MAX>
__device__ __forceinline__ void cb_block_reduce(double (&v)[K], double *sh)
{
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_down(v[k], off, 64);
            v[k] = MAX ? fmax(v[k], o) : v[k] + o;
        }
    __syncthreads();  // sh may still be read from the reduction before
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh[(threadIdx.x >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double a = sh[k];
        for (int w = 1; w < CB_WAVES; ++w) a = MAX ? fmax(a, sh[w * K + k]) : a + sh[w * K + k];
        v[k] = a;
    }
}

// One line of the flood fill, forwards then backwards: a pixel above the level (bit 0) next to a lobe pixel (bit 1) on
// this line joins the lobe.  Returns whether anything changed.
__device__ __forceinline__ int cb_sweep(unsigned char *p, int len, int stride)
{
    int changed = 0, carry = 0;
    for (int k = 0; k < len; ++k) {
        const unsigned char v = p[k * stride];
        if (v & 1) {
            if (v & 2) carry = 1;
            else if (carry) {
                p[k * stride] = 3;
                changed = 1;
            }
        } else carry = 0;
    }
    carry = 0;
    for (int k = len - 1; k >= 0; --k) {
        const unsigned char v = p[k * stride];
        if (v & 1) {
            if (v & 2) carry = 1;
            else if (carry) {
                p[k * stride] = 3;
                changed = 1;
            }
        } else carry = 0;
    }
    return changed;
}

struct CbBox {
    int x0, y0, nx, ny;  // first pixel and extent of a rectangle of the image
};

// acc = (f, J^T r, J^T J, count) of r = psfv - exp(-k q) at p over the pixels of box with xx^2 + yy^2 < r2 (psf_errorsq,
// misc.py:505-526, and its Jacobian), reduced over the block.
__device__ void cb_eval(const double *__restrict__ src, double mx, int ny, int cx, int cy, CbBox box, double r2, double k,
                        const double (&p)[3], double (&acc)[CB_NACC], double *sh)
{
    const double em = fmax(p[0], CB_AXIS_FLOOR), en = fmax(p[1], CB_AXIS_FLOOR);
    const double s = sin(p[2]), c = cos(p[2]);
    const double a = 1.0 / (em * em), b = 1.0 / (en * en);
#pragma unroll
    for (int q = 0; q < CB_NACC; ++q) acc[q] = 0.0;
    // (i, j) walks the box in row-major order, CB_THREADS pixels at a time; the inner while is bounded by CB_THREADS
    int i = int(threadIdx.x) / box.ny, j = int(threadIdx.x) % box.ny;
    while (i < box.nx) {
        const double x = double(box.x0 + i - cx), y = double(box.y0 + j - cy);
        if (x * x + y * y < r2) {
            const double d = src[size_t(box.x0 + i) * size_t(ny) + size_t(box.y0 + j)] / mx;
            const double u0 = -s * x + c * y, u1 = -c * x - s * y;  // R^T [x y]^T
            const double m = exp(-k * (a * u0 * u0 + b * u1 * u1));
            const double r = d - m, km = k * m;
            const double j0 = km * (-2.0 * u0 * u0 * a / em), j1 = km * (-2.0 * u1 * u1 * b / en), j2 = km * (2.0 * u0 * u1 * (a - b));
            acc[0] += r * r;
            acc[1] += j0 * r;
            acc[2] += j1 * r;
            acc[3] += j2 * r;
            acc[4] += j0 * j0;
            acc[5] += j0 * j1;
            acc[6] += j0 * j2;
            acc[7] += j1 * j1;
            acc[8] += j1 * j2;
            acc[9] += j2 * j2;
            acc[10] += 1.0;
        }
        j += CB_THREADS;
        while (j >= box.ny) {
            j -= box.ny;
            ++i;
        }
    }
    cb_block_reduce<CB_NACC, false>(acc, sh);
}

// d = -(H + lambda diag H)^-1 g on the variables that are not fixed (Cholesky of the damped 3 x 3 matrix); false when the
// matrix is not positive definite.
__device__ bool cb_solve(const double (&acc)[CB_NACC], const bool (&fixed)[3], double lambda, double (&d)[3])
{
    double m[3][3] = {{acc[4], acc[5], acc[6]}, {acc[5], acc[7], acc[8]}, {acc[6], acc[8], acc[9]}};
    double rhs[3] = {-acc[1], -acc[2], -acc[3]};
    for (int i = 0; i < 3; ++i) {
        m[i][i] *= 1.0 + lambda;
        if (fixed[i]) {
            for (int q = 0; q < 3; ++q) m[i][q] = m[q][i] = 0.0;
            m[i][i] = 1.0;
            rhs[i] = 0.0;
        }
    }
    if (!(m[0][0] > 0.0)) return false;
    const double l00 = sqrt(m[0][0]), l10 = m[1][0] / l00, l20 = m[2][0] / l00;
    const double t11 = m[1][1] - l10 * l10;
    if (!(t11 > 0.0)) return false;
    const double l11 = sqrt(t11), l21 = (m[2][1] - l20 * l10) / l11;
    const double t22 = m[2][2] - l20 * l20 - l21 * l21;
    if (!(t22 > 0.0)) return false;
    const double l22 = sqrt(t22);
    const double y0 = rhs[0] / l00, y1 = (rhs[1] - l10 * y0) / l11, y2 = (rhs[2] - l20 * y0 - l21 * y1) / l22;
    d[2] = y2 / l22;
    d[1] = (y1 - l21 * d[2]) / l11;
    d[0] = (y0 - l10 * d[1] - l20 * d[2]) / l00;
    return isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
}

struct CbArgs {
    const double *psf;
    int nx, ny, npeak;
    double level, nsigma, fwhm;  // fwhm = 2 sqrt(2 ln 2), from the host's libm as numpy has it
    const double *pmax;
    const int *pnz;
    double *pars;
    pfbhip_cleanbeam_info *info;
};

// One workgroup per band.  Every branch below is taken by the whole workgroup: its conditions come out of block reductions.
__global__ __launch_bounds__(CB_THREADS) void k_cb_fit(CbArgs A)
{
    extern __shared__ unsigned char win[];  // PFBHIP_CB_MAX_WINDOW^2 bytes: bit 0 above the level, bit 1 in the lobe
    __shared__ double sh[CB_WAVES * CB_NACC];
    const int band = blockIdx.x, tid = threadIdx.x;
    const double *src = A.psf + size_t(band) * size_t(A.nx) * size_t(A.ny);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    pfbhip_cleanbeam_info rec;
    rec.status = PFBHIP_CB_ALL_ZERO;
    rec.window = rec.nit = rec.nlobe = 0;
    rec.nfit = 0;
    rec.f = rec.p0[0] = rec.p0[1] = rec.p0[2] = nan;
    double p[3] = {nan, nan, nan};
    auto finish = [&](int status) {
        if (tid == 0) {
            rec.status = status;
            A.info[band] = rec;
            for (int q = 0; q < 3; ++q) A.pars[3 * band + q] = p[q];
        }
    };

    // (a) second stage of the peak
    double mxv[1] = {-INFINITY};
    int nz = 0;
    for (int q = tid; q < A.npeak; q += CB_THREADS) {
        mxv[0] = fmax(mxv[0], A.pmax[size_t(band) * A.npeak + q]);
        nz |= A.pnz[size_t(band) * A.npeak + q];
    }
    cb_block_reduce<1, true>(mxv, sh);
    const double mx = mxv[0];
    if (!__syncthreads_or(nz)) return finish(PFBHIP_CB_ALL_ZERO);
    if (!(mx > 0.0) || !isfinite(mx)) return finish(PFBHIP_CB_BAD_PEAK);
    const int cx = A.nx / 2, cy = A.ny / 2;
    if (!(src[size_t(cx) * A.ny + cy] / mx > A.level)) return finish(PFBHIP_CB_CENTRE_LOW);

    // (b) main lobe: the 4-connected component of {psfv > level} that holds the centre
    int W = CB_WINDOW0;
    CbBox w;
    for (;; W *= 2) {
        w.x0 = max(cx - W / 2, 0);
        w.y0 = max(cy - W / 2, 0);
        w.nx = min(cx + W / 2, A.nx) - w.x0;
        w.ny = min(cy + W / 2, A.ny) - w.y0;
        rec.window = W;
        for (int q = tid; q < w.nx * w.ny; q += CB_THREADS) {
            const int i = q / w.ny, j = q % w.ny;
            win[i * W + j] = src[size_t(w.x0 + i) * A.ny + (w.y0 + j)] / mx > A.level ? 1 : 0;
        }
        __syncthreads();
        if (tid == 0) win[(cx - w.x0) * W + (cy - w.y0)] = 3;
        __syncthreads();
        const int cap = W * W / 2;
        bool settled = false;
        for (int round = 0; round < cap; ++round) {
            int changed = 0;
            for (int i = tid; i < w.nx; i += CB_THREADS) changed |= cb_sweep(win + i * W, w.ny, 1);
            __syncthreads();
            for (int j = tid; j < w.ny; j += CB_THREADS) changed |= cb_sweep(win + j, w.nx, W);
            if (!__syncthreads_or(changed)) {
                settled = true;
                break;
            }
        }
        if (!settled) return finish(PFBHIP_CB_SWEEP_CAP);
        // a lobe pixel on a window edge that is not an image edge: the lobe may go on outside
        int touch = 0;
        for (int j = tid; j < w.ny; j += CB_THREADS) {
            if (w.x0 > 0) touch |= win[j] & 2;
            if (w.x0 + w.nx < A.nx) touch |= win[(w.nx - 1) * W + j] & 2;
        }
        for (int i = tid; i < w.nx; i += CB_THREADS) {
            if (w.y0 > 0) touch |= win[i * W] & 2;
            if (w.y0 + w.ny < A.ny) touch |= win[i * W + w.ny - 1] & 2;
        }
        if (!__syncthreads_or(touch)) break;
        if (W >= PFBHIP_CB_MAX_WINDOW) return finish(PFBHIP_CB_LOBE_TOO_WIDE);
    }

    // (c) start point from the lobe's weighted moments (misc.py:569-591)
    const int nwin = w.nx * w.ny;
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = tid; q < nwin; q += CB_THREADS) {
        const int i = q / w.ny, j = q % w.ny;
        if (win[i * W + j] & 2) {
            const double v = src[size_t(w.x0 + i) * A.ny + (w.y0 + j)] / mx;
            s4[0] += 1.0;
            s4[1] += v;
            s4[2] += v * double(w.x0 + i - cx);
            s4[3] += v * double(w.y0 + j - cy);
        }
    }
    cb_block_reduce<4, false>(s4, sh);
    rec.nlobe = int(s4[0]);
    const double wsum = s4[1], xbar = s4[2] / wsum, ybar = s4[3] / wsum;
    double s3[3] = {0.0, 0.0, 0.0};
    for (int q = tid; q < nwin; q += CB_THREADS) {
        const int i = q / w.ny, j = q % w.ny;
        if (win[i * W + j] & 2) {
            const double v = src[size_t(w.x0 + i) * A.ny + (w.y0 + j)] / mx;
            const double dx = double(w.x0 + i - cx) - xbar, dy = double(w.y0 + j - cy) - ybar;
            s3[0] += v * (dx * dx);
            s3[1] += v * (dy * dy);
            s3[2] += v * dx * dy;
        }
    }
    cb_block_reduce<3, false>(s3, sh);
    const double mxx = s3[0] / wsum, myy = s3[1] / wsum, mxy = s3[2] / wsum;
    const double pa0 = fmin(fmax(CB_PI / 2 + 0.5 * atan2(2.0 * mxy, mxx - myy), 0.0), CB_PI);
    const double ct = cos(CB_PI / 2 + pa0), st = sin(CB_PI / 2 + pa0);
    double e4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};  // max and -min of the rotated offsets
    for (int q = tid; q < nwin; q += CB_THREADS) {
        const int i = q / w.ny, j = q % w.ny;
        if (win[i * W + j] & 2) {
            const double dx = double(w.x0 + i - cx) - xbar, dy = double(w.y0 + j - cy) - ybar;
            const double xr = ct * dx + st * dy, yr = -st * dx + ct * dy;
            e4[0] = fmax(e4[0], xr);
            e4[1] = fmax(e4[1], -xr);
            e4[2] = fmax(e4[2], yr);
            e4[3] = fmax(e4[3], -yr);
        }
    }
    cb_block_reduce<4, true>(e4, sh);
    p[0] = rec.p0[0] = fmax(e4[0] + e4[1], 1.0);
    p[1] = rec.p0[1] = fmax(e4[2] + e4[3], 1.0);
    p[2] = rec.p0[2] = pa0;

    // (d) fit region: the disc of nsigma standard deviations of the start's major axis, as its bounding box in the image
    const double rsig = A.nsigma * (p[0] / A.fwhm), r2 = rsig * rsig;
    const int rad = int(fmin(fabs(rsig), 1073741824.0)) + 1;
    CbBox box;
    box.x0 = max(cx - rad, 0);
    box.y0 = max(cy - rad, 0);
    box.nx = int(min(int64_t(cx) + rad, int64_t(A.nx) - 1)) - box.x0 + 1;
    box.ny = int(min(int64_t(cy) + rad, int64_t(A.ny) - 1)) - box.y0 + 1;

    // (e) Levenberg-Marquardt with projection onto emaj >= 0, emin >= 0, 0 <= pa <= pi.  A variable that sits on a bound
    // with the gradient pushing outwards is held there and the step is solved for the others, so the fixed point is the
    // constrained minimiser.  Every thread holds the reduced sums and solves the same 3 x 3 system: nothing to broadcast.
    const double kq = 0.5 * A.fwhm * A.fwhm;
    const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {INFINITY, INFINITY, CB_PI};
    double acc[CB_NACC], tacc[CB_NACC];
    cb_eval(src, mx, A.ny, cx, cy, box, r2, kq, p, acc, sh);
    rec.nfit = int64_t(acc[10]);
    double lambda = 1e-3;
    int status = PFBHIP_CB_ITER_CAP;
    for (int it = 0; it < PFBHIP_CB_MAX_ITER; ++it) {
        rec.nit = it + 1;
        const double diag[3] = {acc[4], acc[7], acc[9]};
        bool fixed[3];
        for (int q = 0; q < 3; ++q)
            fixed[q] = (p[q] <= lo[q] && acc[1 + q] > 0.0) || (p[q] >= hi[q] && acc[1 + q] < 0.0) || !(diag[q] > 0.0);
        bool moved = false, small = false;
        for (int raise = 0; raise < PFBHIP_CB_MAX_RAISE; ++raise) {
            double d[3], t[3];
            if (cb_solve(acc, fixed, lambda, d)) {
                small = true;
                for (int q = 0; q < 3; ++q) {
                    t[q] = fmin(fmax(p[q] + d[q], lo[q]), hi[q]);
                    small = small && fabs(t[q] - p[q]) <= CB_STEP_TOL * (1.0 + fabs(p[q]));
                }
                if (small) break;
                cb_eval(src, mx, A.ny, cx, cy, box, r2, kq, t, tacc, sh);
                if (tacc[0] <= acc[0]) {
                    for (int q = 0; q < 3; ++q) p[q] = t[q];
                    for (int q = 0; q < CB_NACC; ++q) acc[q] = tacc[q];
                    lambda = fmax(lambda * 0.1, 1e-12);
                    moved = true;
                    break;
                }
            }
            lambda *= 10.0;
        }
        if (small) {
            status = PFBHIP_CB_CONVERGED;
            break;
        }
        if (!moved) {
            status = PFBHIP_CB_RAISE_CAP;
            break;
        }
    }
    rec.f = acc[0];
    finish(status);
}

static void cleanbeam_run(const double *psf_dev, int64_t nband, int64_t nx, int64_t ny, double level, double nsigma, double *pars,
                          pfbhip_cleanbeam_info *info)
{
    const int64_t n = nx * ny;
    const int npeak = int(std::min<int64_t>(std::max<int64_t>(ceil_div(n, int64_t(CB_THREADS) * CB_PEAK_PER_THREAD), 1), CB_PEAK_MAX_BLOCKS));
    DevBuf<double> d_pmax(size_t(nband) * npeak), d_pars(size_t(nband) * 3);
    DevBuf<int> d_pnz(size_t(nband) * npeak);
    DevBuf<pfbhip_cleanbeam_info> d_info(size_t(nband) + 0);
    const bool timing = std::getenv("PFBHIP_CLEANBEAM_TIMING") != nullptr;  // hipEvent times of the two kernels on stderr
    EventTimer t_peak(timing), t_fit(timing);
    std::vector<pfbhip_cleanbeam_info> h_info(static_cast<size_t>(nband));
    synced(nullptr, [&] {
        t_peak.start(nullptr);
        hipLaunchKernelGGL(k_cb_peak, dim3(npeak, uint32_t(nband)), dim3(CB_THREADS), 0, nullptr, psf_dev, n, d_pmax.p, d_pnz.p);
        PFB_HIP(hipGetLastError());
        t_peak.stop(nullptr);
        t_fit.start(nullptr);
        const int lds = PFBHIP_CB_MAX_WINDOW * PFBHIP_CB_MAX_WINDOW;
        allow_dynamic_lds(reinterpret_cast<const void *>(&k_cb_fit), lds);  // 64 KiB of window on top of the static scratch
        const CbArgs a{psf_dev, int(nx), int(ny), npeak, level, nsigma, 2.0 * std::sqrt(2.0 * std::log(2.0)),
                       d_pmax.p, d_pnz.p, d_pars.p, d_info.p};
        hipLaunchKernelGGL(k_cb_fit, dim3(uint32_t(nband)), dim3(CB_THREADS), lds, nullptr, a);
        PFB_HIP(hipGetLastError());
        t_fit.stop(nullptr);
        PFB_HIP(hipMemcpy(pars, d_pars.p, d_pars.bytes(), hipMemcpyDeviceToHost));
        PFB_HIP(hipMemcpy(h_info.data(), d_info.p, d_info.bytes(), hipMemcpyDeviceToHost));
    });
    if (timing)
        fprintf(stderr, "pfbhip_cleanbeam (%lld, %lld, %lld): k_cb_peak %.4f ms (%.1f GB/s), k_cb_fit %.4f ms\n", (long long)nband,
                (long long)nx, (long long)ny, t_peak.ms(), double(nband) * double(n) * 8.0 / (t_peak.ms() * 1e6), t_fit.ms());
    if (info)
        for (int64_t b = 0; b < nband; ++b) info[b] = h_info[size_t(b)];
    for (int64_t b = 0; b < nband; ++b) {
        const pfbhip_cleanbeam_info &r = h_info[size_t(b)];
        PFB_REQUIRE(r.status != PFBHIP_CB_BAD_PEAK, "cleanbeam: band %lld has non-zero data but no positive finite maximum", (long long)b);
        PFB_REQUIRE(r.status != PFBHIP_CB_CENTRE_LOW,
                    "cleanbeam: band %lld: the centre pixel (%lld, %lld) is not above level = %g of the peak, so no main lobe holds it "
                    "(the reference would fit the background there)",
                    (long long)b, (long long)(nx / 2), (long long)(ny / 2), level);
        PFB_REQUIRE(r.status != PFBHIP_CB_LOBE_TOO_WIDE,
                    "cleanbeam: band %lld: the main lobe above level = %g still touches a window of %d pixels around the centre: "
                    "beams wider than the limit of %d pixels are not fitted",
                    (long long)b, level, PFBHIP_CB_MAX_WINDOW, PFBHIP_CB_MAX_WINDOW);
        if (r.status == PFBHIP_CB_SWEEP_CAP)
            throw std::runtime_error(strprintf("cleanbeam: band %lld: the flood fill of the main lobe hit its cap of %d rounds",
                                               (long long)b, r.window * r.window / 2));
    }
}

static void cleanbeam_check(const void *psf, int64_t nband, int64_t nx, int64_t ny, double level, double nsigma, const double *pars)
{
    PFB_REQUIRE(psf && pars, "NULL argument");
    PFB_REQUIRE(nband >= 1 && nband <= 65535 && nx >= 1 && ny >= 1 && nx <= (int64_t(1) << 30) && ny <= (int64_t(1) << 30),
                "bad cube shape (%lld, %lld, %lld)", (long long)nband, (long long)nx, (long long)ny);
    PFB_REQUIRE(std::isfinite(level) && std::isfinite(nsigma) && nsigma > 0.0, "bad level %g or nsigma %g", level, nsigma);
}

}  // namespace pfbhip

using namespace pfbhip;

extern "C" {

int pfbhip_cleanbeam_fit_dev(const double *psf_dev, int64_t nband, int64_t nx, int64_t ny, double level, double nsigma, double *pars,
                             pfbhip_cleanbeam_info *info)
{
    return guarded([&] {
        cleanbeam_check(psf_dev, nband, nx, ny, level, nsigma, pars);
        cleanbeam_run(psf_dev, nband, nx, ny, level, nsigma, pars, info);
    });
}

int pfbhip_cleanbeam_fit(const double *psf_host, int64_t nband, int64_t nx, int64_t ny, double level, double nsigma, double *pars,
                         pfbhip_cleanbeam_info *info)
{
    return guarded([&] {
        cleanbeam_check(psf_host, nband, nx, ny, level, nsigma, pars);
        DevBuf<double> d_psf(size_t(nband) * size_t(nx) * size_t(ny));
        PFB_HIP(hipMemcpy(d_psf.p, psf_host, d_psf.bytes(), hipMemcpyHostToDevice));
        cleanbeam_run(d_psf.p, nband, nx, ny, level, nsigma, pars, info);
    });
}

}  // extern "C"
