// fb.hip -- the forward-backward (ISTA / FISTA) backward step of the minor cycle with every cube resident in HBM.
//
// Mirrors ForwardBackward.solve of pfb-imaging (src/pfb_imaging/opt/forward_backward.py:95-133) with the tight-frame
// prox of an l21 (prox/l21.py) or l1 (prox/l1.py) regulariser over a wavelet dictionary or the identity, and the
// gradient of the forward-backward splitting grad(y) = -H (xtilde - y) / g (deconv/pfb.py:158-161):
//     xg    <- y + (step / g) H (xtilde - y)                 (forward step, psfconv accumulating into y)
//     alpha <- Psi^H xg ;  alpha <- prox(alpha) - alpha       (k_fb_shrink, in place)
//     x     <- positivity(xg + Psi alpha / nu)               (k_fb_step, with the norms, y_next and d = xtilde - y_next)
//     eps   =  ||x - xp|| / max(||x||^2, 1e-12)^1/2 (1 if x == 0) ;  y <- x + beta_k (x - xp) ;  xp <- x
// One host round trip per iteration (the three scalars of eps).  The state survives a convergence event: the host hands
// x to on_converge and, if asked to go on, calls pfbhip_fb_run again with the state still in HBM.
#pragma clang fp contract(fast)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <memory>
#include <utility>
#include <vector>

#include "common.hpp"
#include "devcg.hpp"
#include "devloop.hpp"
#include "pipeline_api.hpp"

namespace pfbhip {

// ratio of the l21 prox: prox(alpha)_b = alpha_b * ratio(sum_b alpha_b) (prox_21m.py:5-26; 0 where the band sum is 0)
__device__ __forceinline__ double l21_ratio(double s, double thr)
{
    const double a = fabs(s);
    return a > 0.0 ? fmax(a - thr, 0.0) / a : 0.0;
}
// prox(a) - a of the soft threshold (prox/l1.py)
__device__ __forceinline__ double l1_delta(double a, double thr) { return copysign(fmax(fabs(a) - thr, 0.0), a) - a; }

// alpha <- prox(alpha) - alpha over a coefficient cube (NB, n), two coefficients per thread (n even), every band of a
// coefficient in the same thread.  l1 = 0: l21 over the band axis; l1 = 1: per-band soft threshold.
template <int NB>
__global__ void __launch_bounds__(256) k_fb_shrink(double *__restrict__ alpha, int64_t n, double tau, const double *__restrict__ w,
                                                   int l1)
{
    const int64_t n2 = n / 2;
    for (int64_t i = blockIdx.x * int64_t(256) + threadIdx.x; i < n2; i += int64_t(gridDim.x) * 256) {
        const double2 wt = reinterpret_cast<const double2 *>(w)[i];
        double2 a[NB];
        double2 s = {0.0, 0.0};
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            a[b] = reinterpret_cast<const double2 *>(alpha + size_t(b) * size_t(n))[i];
            s.x += a[b].x;
            s.y += a[b].y;
        }
        const double rx = l21_ratio(s.x, tau * wt.x), ry = l21_ratio(s.y, tau * wt.y);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            double2 o;
            if (l1) {
                o.x = l1_delta(a[b].x, tau * wt.x);
                o.y = l1_delta(a[b].y, tau * wt.y);
            } else {
                o.x = a[b].x * rx - a[b].x;
                o.y = a[b].y * ry - a[b].y;
            }
            reinterpret_cast<double2 *>(alpha + size_t(b) * size_t(n))[i] = o;
        }
    }
}

// Fallback for any band count / odd sizes, pass 1 of 2: s = sum_b alpha_b (l21 only)
__global__ void __launch_bounds__(256) k_fb_bandsum(const double *__restrict__ alpha, int nband, int64_t n, double *__restrict__ s)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i >= n) return;
    double t = 0.0;
    for (int b = 0; b < nband; ++b) t += alpha[size_t(b) * size_t(n) + size_t(i)];
    s[i] = t;
}
// pass 2: one element per thread over the whole cube (s == nullptr: l1)
__global__ void __launch_bounds__(256) k_fb_shrink_gen(double *__restrict__ alpha, int64_t n, int64_t total, double tau,
                                                       const double *__restrict__ w, const double *__restrict__ s)
{
    const int64_t j = blockIdx.x * int64_t(256) + threadIdx.x;
    if (j >= total) return;
    const int64_t i = j % n;
    const double a = alpha[j], thr = tau * w[i];
    alpha[j] = s != nullptr ? a * l21_ratio(s[i], thr) - a : l1_delta(a, thr);
}

// The image-domain pass, two pixels per thread (npix even), every band of a pixel in the same thread:
//   ID = false: x = xg + xout / nu ;  ID = true (IdentityPsi): x = xg + (prox(xg) - xg) / nu, prox l21 (l1 = 0) or l1
//   positivity 1: clamp negatives, 2: zero the pixel in every band if any band is <= 0 (positivity.py:12-33)
//   partials [0] = |x - xp|^2, [1] = |x|^2, [2] = #nonzero(x)
//   x out ; y <- x + beta (x - xp) (y holds xg on entry: same element, same thread) ; d = xtilde - y
template <int NB, bool ID>
__global__ void __launch_bounds__(CG_THREADS) k_fb_step(int64_t npix, double *__restrict__ y, const double *__restrict__ xout,
                                                        const double *__restrict__ xp, const double *__restrict__ xt,
                                                        double *__restrict__ x, double *__restrict__ d, double inv_nu, double beta,
                                                        int mode, double tau, const double *__restrict__ w, int l1,
                                                        double *partials)
{
    double v[3] = {0.0, 0.0, 0.0};
    const int64_t n2 = npix / 2;
    for (int64_t i = blockIdx.x * int64_t(CG_THREADS) + threadIdx.x; i < n2; i += int64_t(CG_BLOCKS) * CG_THREADS) {
        double2 xs[NB];
        if (ID) {
            const double2 wt = reinterpret_cast<const double2 *>(w)[i];
            double2 s = {0.0, 0.0};
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                xs[b] = reinterpret_cast<const double2 *>(y + size_t(b) * size_t(npix))[i];
                s.x += xs[b].x;
                s.y += xs[b].y;
            }
            const double rx = l21_ratio(s.x, tau * wt.x), ry = l21_ratio(s.y, tau * wt.y);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const double2 g = xs[b];
                if (l1) {
                    xs[b].x = g.x + l1_delta(g.x, tau * wt.x) * inv_nu;
                    xs[b].y = g.y + l1_delta(g.y, tau * wt.y) * inv_nu;
                } else {
                    xs[b].x = g.x + (g.x * rx - g.x) * inv_nu;
                    xs[b].y = g.y + (g.y * ry - g.y) * inv_nu;
                }
            }
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const double2 g = reinterpret_cast<const double2 *>(y + size_t(b) * size_t(npix))[i];
                const double2 o = reinterpret_cast<const double2 *>(xout + size_t(b) * size_t(npix))[i];
                xs[b].x = g.x + o.x * inv_nu;
                xs[b].y = g.y + o.y * inv_nu;
            }
        }
        bool badx = false, bady = false;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            badx = badx || xs[b].x <= 0.0;
            bady = bady || xs[b].y <= 0.0;
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const size_t o = size_t(b) * size_t(npix);
            double2 xi = xs[b];
            if (mode == 1) {
                xi.x = xi.x < 0.0 ? 0.0 : xi.x;
                xi.y = xi.y < 0.0 ? 0.0 : xi.y;
            } else if (mode == 2) {
                xi.x = badx ? 0.0 : xi.x;
                xi.y = bady ? 0.0 : xi.y;
            }
            const double2 p = reinterpret_cast<const double2 *>(xp + o)[i];
            const double2 t = reinterpret_cast<const double2 *>(xt + o)[i];
            const double dx = xi.x - p.x, dy = xi.y - p.y;
            v[0] += dx * dx + dy * dy;
            v[1] += xi.x * xi.x + xi.y * xi.y;
            v[2] += (xi.x != 0.0 ? 1.0 : 0.0) + (xi.y != 0.0 ? 1.0 : 0.0);
            const double2 yn = {xi.x + beta * dx, xi.y + beta * dy};
            reinterpret_cast<double2 *>(x + o)[i] = xi;
            reinterpret_cast<double2 *>(y + o)[i] = yn;
            reinterpret_cast<double2 *>(d + o)[i] = double2{t.x - yn.x, t.y - yn.y};
        }
    }
    block_reduce_store<3>(v, partials);
}

// Fallback for any band count / odd sizes: positivity 2 first flags the pixels with a non-positive band (x computed
// on the fly from xg, xout), then k_fb_step_gen streams band by band (no band held in registers).
__global__ void __launch_bounds__(256) k_fb_flag(int64_t npix, int nband, const double *__restrict__ y, const double *__restrict__ xout,
                                                 double inv_nu, double *__restrict__ bad)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i >= npix) return;
    bool f = false;
    for (int b = 0; b < nband; ++b) {
        const size_t o = size_t(b) * size_t(npix) + size_t(i);
        f = f || y[o] + xout[o] * inv_nu <= 0.0;
    }
    bad[i] = f ? 1.0 : 0.0;
}
static __global__ void __launch_bounds__(CG_THREADS) k_fb_step_gen(int64_t npix, int nband, double *__restrict__ y,
                                                                    const double *__restrict__ xout, const double *__restrict__ xp,
                                                                    const double *__restrict__ xt, double *__restrict__ x,
                                                                    double *__restrict__ d, double inv_nu, double beta, int mode,
                                                                    const double *__restrict__ bad, double *partials)
{
    double v[3] = {0.0, 0.0, 0.0};
    const int64_t n = int64_t(nband) * npix;
    for (int64_t j = blockIdx.x * int64_t(CG_THREADS) + threadIdx.x; j < n; j += int64_t(CG_BLOCKS) * CG_THREADS) {
        double xi = y[j] + xout[j] * inv_nu;
        if (mode == 1 && xi < 0.0) xi = 0.0;
        if (mode == 2 && bad[j % npix] > 0.0) xi = 0.0;
        const double dx = xi - xp[j];
        v[0] += dx * dx;
        v[1] += xi * xi;
        v[2] += (xi != 0.0) ? 1.0 : 0.0;
        const double yn = xi + beta * dx;
        x[j] = xi;
        y[j] = yn;
        d[j] = xt[j] - yn;
    }
    block_reduce_store<3>(v, partials);
}

template <int NB>
static void launch_shrink(hipStream_t st, double *alpha, int64_t n, double tau, const double *w, int l1)
{
    const int64_t blocks = std::min<int64_t>(ceil_div(n / 2, 256), 8192);
    hipLaunchKernelGGL(k_fb_shrink<NB>, dim3(uint32_t(blocks)), dim3(256), 0, st, alpha, n, tau, w, l1);
}
template <int NB, bool ID>
static void launch_step(hipStream_t st, int64_t npix, double *y, const double *xout, const double *xp, const double *xt, double *x,
                        double *d, double inv_nu, double beta, int mode, double tau, const double *w, int l1, double *partials)
{
    hipLaunchKernelGGL((k_fb_step<NB, ID>), dim3(CG_BLOCKS), dim3(CG_THREADS), 0, st, npix, y, xout, xp, xt, x, d, inv_nu, beta, mode,
                       tau, w, l1, partials);
}

// compile-time band count 1..LOOP_MAXB from a runtime one
template <template <int> class F, int NB = 1, class... A>
static void dispatch_nb(int nband, A &&...args)
{
    if constexpr (NB <= LOOP_MAXB) {
        if (nband == NB) return F<NB>::run(std::forward<A>(args)...);
        dispatch_nb<F, NB + 1>(nband, std::forward<A>(args)...);
    }
}
template <int NB>
struct ShrinkNB {
    template <class... A>
    static void run(A &&...a) { launch_shrink<NB>(std::forward<A>(a)...); }
};
template <int NB>
struct StepNB {
    template <class... A>
    static void run(A &&...a) { launch_step<NB, false>(std::forward<A>(a)...); }
};
template <int NB>
struct StepIdNB {
    template <class... A>
    static void run(A &&...a) { launch_step<NB, true>(std::forward<A>(a)...); }
};

}  // namespace pfbhip

using namespace pfbhip;

// The resumable state of one forward-backward solve.
struct pfbhip_fb {
    pfbhip_psi *psi = nullptr;  // nullptr: IdentityPsi
    PsfHessBands bands;
    int64_t nband = 0, nx = 0, ny = 0, nxmax = 0, nymax = 0;
    int nbasis = 1;
    size_t npix = 0, nimg = 0, cube = 0, ncoef = 0;
    double g = 1.0, nu = 1.0, step = 1.0;
    int reg_kind = 0, positivity = 0, acceleration = 1;
    hipStream_t st = nullptr;  // the first plan's: every launch of the solve goes there
    DevBuf<double> xt, y, xa, xb, d, xout, alpha, w, scratch, partials;
    double *x = nullptr, *xp = nullptr;
    std::vector<double> hpart;
    Resume run;
    double t = 1.0;  // the FISTA sequence
    int64_t events = 0;
};

extern "C" {

int pfbhip_fb_create(pfbhip_psi *psi, pfbhip_psfconv *const *pcs, int64_t nband, const int64_t *nparts, const int64_t *psf_slots,
                     const int64_t *beam_slots, const double *scale, const double *eta, const double *xtilde_host, double g,
                     const double *x0_host, const double *weight_host, int reg_kind, double nu, double step, int positivity,
                     int acceleration, pfbhip_fb **out)
{
    return guarded([&] {
        PFB_REQUIRE(out && xtilde_host && x0_host, "bad arguments");
        PFB_REQUIRE(reg_kind == 0 || reg_kind == 1, "reg_kind %d (0 l21, 1 l1)", reg_kind);
        PFB_REQUIRE(positivity >= 0 && positivity <= 2, "positivity mode %d", positivity);
        PFB_REQUIRE(g != 0.0 && nu != 0.0, "g and nu must be non-zero");
        std::unique_ptr<pfbhip_fb> h(new pfbhip_fb);
        h->psi = psi;
        h->nband = nband;
        h->g = g;
        h->nu = nu;
        h->step = step;
        h->reg_kind = reg_kind;
        h->positivity = positivity;
        h->acceleration = acceleration ? 1 : 0;
        if (psi) psi_geometry(psi, &h->nx, &h->ny, &h->nbasis, &h->nxmax, &h->nymax);
        h->bands = PsfHessBands(pcs, nband, nparts, psf_slots, beam_slots, scale, eta, psi ? h->nx : -1, psi ? h->ny : -1);
        if (!psi) {  // the identity: the coefficients are the image
            h->nx = h->nxmax = h->bands.nx;
            h->ny = h->nymax = h->bands.ny;
            h->nbasis = 1;
        }
        h->npix = size_t(h->nx) * size_t(h->ny);
        h->nimg = size_t(nband) * h->npix;
        h->cube = psi ? size_t(h->nbasis) * size_t(h->nxmax) * size_t(h->nymax) : h->npix;
        h->ncoef = size_t(nband) * h->cube;
        // IdentityPsi: the one-pass step folds the prox in when the bands fit in registers; otherwise alpha is a copy of xg
        const bool fused_id = !psi && nband <= LOOP_MAXB && h->npix % 2 == 0;
        h->st = h->bands.stream();
        h->xt.alloc(h->nimg);
        h->y.alloc(h->nimg);
        h->xa.alloc(h->nimg);
        h->xb.alloc(h->nimg);
        h->d.alloc(h->nimg);
        if (psi) h->xout.alloc(h->nimg);
        if (!fused_id) h->alpha.alloc(h->ncoef);
        h->w.alloc(h->cube);
        h->scratch.alloc(std::max(h->cube, h->npix));
        h->partials.alloc(3 * size_t(CG_BLOCKS));
        h->hpart.resize(3 * size_t(CG_BLOCKS));
        h->xp = h->xa.p;
        h->x = h->xb.p;
        const hipStream_t st = h->st;
        h->run.has_weight = weight_host != nullptr;  // (NULL: the caller sets the weight before the first run)
        synced(st, [&] {
            PFB_HIP(hipMemcpyAsync(h->xt.p, xtilde_host, h->nimg * sizeof(double), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(h->xp, x0_host, h->nimg * sizeof(double), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(h->y.p, h->xp, h->nimg * sizeof(double), hipMemcpyDeviceToDevice, st));
            if (weight_host) PFB_HIP(hipMemcpyAsync(h->w.p, weight_host, h->cube * sizeof(double), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_diff, blocks1d(int64_t(h->nimg)), dim3(256), 0, st, h->xt.p, h->y.p, h->d.p, int64_t(h->nimg));
            PFB_HIP(hipGetLastError());
        });
        *out = h.release();
    });
}

int pfbhip_fb_set_weight(pfbhip_fb *h, const double *weight_host)
{
    return guarded([&] {
        PFB_REQUIRE(h && weight_host, "NULL argument");
        h->run.set_weight(h->w.p, weight_host, h->cube, hipMemcpyHostToDevice, h->st);
    });
}

int pfbhip_fb_set_weight_dev(pfbhip_fb *h, const double *weight_dev)
{
    return guarded([&] {
        PFB_REQUIRE(h && weight_dev, "NULL argument");
        h->run.set_weight(h->w.p, weight_dev, h->cube, hipMemcpyDeviceToDevice, h->st);
    });
}

int pfbhip_fb_iterate_dev(pfbhip_fb *h, const double **x_dev)
{
    return guarded([&] {
        PFB_REQUIRE(h && x_dev, "NULL argument");
        *x_dev = h->run.iterate(h->x, h->xp);
    });
}

int pfbhip_fb_run(pfbhip_fb *h, double lam, double tol, int maxit, double *x_host, pfbhip_fb_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(h && x_host && maxit >= 1, "bad arguments");
        h->run.require_runnable(maxit);
        StreamScope scope(h->psi, h->bands, h->st);
        const hipStream_t st = h->st;
        const int64_t nband = h->nband;
        const size_t npix = h->npix, cube = h->cube;
        const double tau = h->step * lam, inv_nu = 1.0 / h->nu;
        const int l1 = h->reg_kind;
        const bool fast = nband <= LOOP_MAXB && npix % 2 == 0;
        const bool fused_id = !h->psi && fast;
        StageTimer clk(st, info != nullptr && maxit <= 64);
        int status = 1;
        synced(st, [&] {
            PFB_HIP(hipStreamSynchronize(st));
            const auto t0 = std::chrono::steady_clock::now();
            for (;;) {
                (void)h->run.complete(h->x, h->xp);  // xp <- x (y and d were written by the previous step kernel)
                double beta = 0.0;
                if (h->acceleration) {  // FISTA momentum: data-independent, advanced once per iteration
                    const double tp = h->t;
                    h->t = (1.0 + std::sqrt(1.0 + 4.0 * tp * tp)) / 2.0;
                    beta = (tp - 1.0) / h->t;
                }
                // 1. forward step: y <- y + (step / g) H d, d = xtilde - y
                for (int64_t b = 0; b < nband; ++b)
                    h->bands.apply(b, h->d.p + size_t(b) * npix, h->y.p + size_t(b) * npix, h->step / h->g, 1.0, true, &clk, 0);
                const double *xo = h->xout.p;
                if (!fused_id) {
                    // 2. analysis (a copy of xg for the identity)
                    clk.begin(1);
                    if (h->psi) {
                        for (int64_t b = 0; b < nband; ++b) psi_dot_async(h->psi, h->y.p + size_t(b) * npix, h->alpha.p + size_t(b) * cube);
                    } else {
                        PFB_HIP(hipMemcpyAsync(h->alpha.p, h->y.p, h->nimg * sizeof(double), hipMemcpyDeviceToDevice, st));
                    }
                    clk.end();
                    // 3. alpha <- prox(alpha) - alpha
                    clk.begin(2);
                    if (nband <= LOOP_MAXB && cube % 2 == 0) {
                        dispatch_nb<ShrinkNB>(int(nband), st, h->alpha.p, int64_t(cube), tau, (const double *)h->w.p, l1);
                    } else {
                        if (!l1) hipLaunchKernelGGL(k_fb_bandsum, blocks1d(int64_t(cube)), dim3(256), 0, st, h->alpha.p, int(nband), int64_t(cube),
                                                    h->scratch.p);
                        hipLaunchKernelGGL(k_fb_shrink_gen, blocks1d(int64_t(h->ncoef)), dim3(256), 0, st, h->alpha.p, int64_t(cube),
                                           int64_t(h->ncoef), tau, h->w.p, l1 ? nullptr : h->scratch.p);
                    }
                    clk.end();
                    // 4. synthesis (the identity's alpha is the image-domain difference already)
                    clk.begin(3);
                    if (h->psi) {
                        for (int64_t b = 0; b < nband; ++b) psi_hdot_async(h->psi, h->alpha.p + size_t(b) * cube, h->xout.p + size_t(b) * npix);
                    } else {
                        xo = h->alpha.p;
                    }
                    clk.end();
                }
                // 5. x, positivity, norms, y_next, d
                clk.begin(4);
                if (fused_id) {
                    dispatch_nb<StepIdNB>(int(nband), st, int64_t(npix), h->y.p, (const double *)nullptr, (const double *)h->xp,
                                          (const double *)h->xt.p, h->x, h->d.p, inv_nu, beta, h->positivity, tau,
                                          (const double *)h->w.p, l1, h->partials.p);
                } else if (fast) {
                    dispatch_nb<StepNB>(int(nband), st, int64_t(npix), h->y.p, xo, (const double *)h->xp, (const double *)h->xt.p, h->x,
                                        h->d.p, inv_nu, beta, h->positivity, tau, (const double *)h->w.p, l1, h->partials.p);
                } else {
                    if (h->positivity == 2)
                        hipLaunchKernelGGL(k_fb_flag, blocks1d(int64_t(npix)), dim3(256), 0, st, int64_t(npix), int(nband), h->y.p, xo, inv_nu,
                                           h->scratch.p);
                    hipLaunchKernelGGL(k_fb_step_gen, dim3(CG_BLOCKS), dim3(CG_THREADS), 0, st, int64_t(npix), int(nband), h->y.p, xo, h->xp,
                                       h->xt.p, h->x, h->d.p, inv_nu, beta, h->positivity, h->scratch.p, h->partials.p);
                }
                clk.end();
                PFB_HIP(hipGetLastError());
                double s[3];  // |x - xp|^2, |x|^2, #nonzero(x)
                fetch_partials<3>(h->partials.p, h->hpart, st, s);
                h->run.eps = rel_change_eps(s[0], s[1], s[2]);
                h->run.pending = true;
                if (h->run.eps < tol) {
                    status = 0;
                    ++h->events;
                    break;
                }
                if (h->run.k + 1 >= maxit) break;
            }
            h->run.loop_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            PFB_HIP(hipMemcpyAsync(x_host, h->x, h->nimg * sizeof(double), hipMemcpyDeviceToHost, st));
        });
        clk.collect(h->run.stage_ms, h->run.stage_calls);
        if (info) {
            info->iters = h->run.k;
            info->status = status;
            info->eps = h->run.eps;
            info->loop_ms = h->run.loop_ms;
            info->events = h->events;
            h->run.stages_to(info->stage_ms, info->stage_calls);
        }
    });
}

int pfbhip_fb_destroy(pfbhip_fb *h)
{
    return guarded([&] { delete h; });
}

}  // extern "C"
