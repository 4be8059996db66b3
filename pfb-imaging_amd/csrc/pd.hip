// pd.hip -- the primal-dual (backward) step of the SARA minor cycle with every cube resident in HBM.
//
// Mirrors PrimalDual.solve (/root/reference/src/pfb_imaging/opt/primal_dual.py:406-448; legacy loop :230-262)
// with the l21 regulariser over the wavelet dictionary (prox/l21.py:15-50, fused dual update
// prox/prox_21m.py:105-135) and the gradient of the forward-backward splitting,
// grad(x) = -H (xtilde - x) / gamma (deconv/pfb.py:158-161, core/sara.py:288-289), H the PSF-approximate
// Hessian of HessianTree / HessPSF (operators/hessian.py:326-348, 439-522):
//     v     <- Psi^H xp ;  v <- dual update(vp, v) ;  vp <- 2 v - vp
//     xout  <- Psi vp + grad(xp) ;  x <- xp - tau xout ;  x <- positivity(x)
//     eps   =  ||x - xp|| / max(||x||, 1e-6) (1 if x == 0) ;  stop if eps < tol ;  xp <- x, vp <- v
// One host round trip per iteration (the three scalars of eps) instead of ~10 cubes.
#pragma clang fp contract(fast)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "common.hpp"
#include "devcg.hpp"
#include "devloop.hpp"
#include "pipeline_api.hpp"

// a failed C-ABI call inside the driver (its message is already in pfbhip_last_error())
#define PFB_CHECK_STATUS(call)                                                    \
    do {                                                                          \
        if ((call) != 0) throw std::runtime_error(std::string(pfbhip_last_error())); \
    } while (0)

namespace pfbhip {

__global__ void __launch_bounds__(256) k_pd_primal(double *__restrict__ x, const double *__restrict__ xp,
                                                   const double *__restrict__ xout, double tau, int64_t n)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i < n) x[i] = xp[i] - tau * xout[i];
}
// Primal step, positivity and the three norms in ONE pass over the images (all bands of a pixel in the same thread):
// x = xp - tau xout ; mode 1: clamp negatives, mode 2: zero the pixel in every band where any band is <= 0
// (positivity.py:12-33) ; partials [0] = |x - xp|^2, [1] = |x|^2, [2] = #nonzero(x).  nband <= LOOP_MAXB.
static __global__ void __launch_bounds__(CG_THREADS) k_pd_step(int64_t npix, int nband, double *__restrict__ x,
                                                                const double *__restrict__ xp, const double *__restrict__ xout,
                                                                double tau, int mode, double *partials)
{
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = blockIdx.x * int64_t(CG_THREADS) + threadIdx.x; i < npix; i += int64_t(CG_BLOCKS) * CG_THREADS) {
        double xs[LOOP_MAXB], ps[LOOP_MAXB];
        bool bad = false;
        for (int b = 0; b < nband; ++b) {
            const size_t o = size_t(b) * size_t(npix) + size_t(i);
            ps[b] = xp[o];
            xs[b] = ps[b] - tau * xout[o];
            bad = bad || xs[b] <= 0.0;
        }
        for (int b = 0; b < nband; ++b) {
            double xi = xs[b];
            if (mode == 1 && xi < 0.0) xi = 0.0;
            if (mode == 2 && bad) xi = 0.0;
            x[size_t(b) * size_t(npix) + size_t(i)] = xi;
            const double d = xi - ps[b];
            v[0] += d * d;
            v[1] += xi * xi;
            v[2] += (xi != 0.0) ? 1.0 : 0.0;
        }
    }
    block_reduce_store<3>(v, partials);
}

// partials [0] = |x - xp|^2, [1] = |x|^2, [2] = #nonzero(x)
static __global__ void __launch_bounds__(CG_THREADS) k_pd_norms(int64_t n, const double *x, const double *xp, double *partials)
{
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = blockIdx.x * int64_t(CG_THREADS) + threadIdx.x; i < n; i += int64_t(CG_BLOCKS) * CG_THREADS) {
        const double xi = x[i], d = xi - xp[i];
        v[0] += d * d;
        v[1] += xi * xi;
        v[2] += (xi != 0.0) ? 1.0 : 0.0;
    }
    block_reduce_store<3>(v, partials);
}

}  // namespace pfbhip

using namespace pfbhip;

// The state of one primal-dual solve in HBM: the problem, the buffers and where the loop stands.  comm == NULL: all bands
// are on this device.  comm != NULL: this rank's local bands; the band sum of the dual update, the "any band <= 0" test
// of positivity mode 2 and the norms are completed with all-reduces (pfbhip_primal_dual only).
struct pfbhip_pd {
    pfbhip_psi *psi = nullptr;
    PsfHessBands bands;
    pfbhip_comm *comm = nullptr;
    size_t npix = 0, nimg = 0, cube = 0, ncoef = 0;
    double gamma = 1.0, sigma = 1.0, tau = 1.0;
    int positivity = 0;
    hipStream_t st = nullptr;  // the first plan's: every launch of the solve goes there
    // Buffer rotation instead of copies: xa / xb alternate as (x, xp); va / vb alternate as (dual, previous dual); vext
    // holds the extrapolated dual 2 v - vp of the current iteration; sum only with a communicator.
    DevBuf<double> xa, xb, xout, xt, d, va, vb, vext, w, sum, partials;
    double *x = nullptr, *xp = nullptr, *v = nullptr, *vp = nullptr;
    std::vector<double> hpart;
    Resume run;
    pfbhip_pd_traffic traffic = {};

    // uploads the start values (weight_host may be NULL: set before the first run)
    pfbhip_pd(pfbhip_psi *psi_, pfbhip_psfconv *const *pcs, int64_t nband, const int64_t *nparts, const int64_t *psf_slots,
              const int64_t *beam_slots, const double *scale, const double *eta, const double *xtilde_host, double gamma_,
              const double *x_host, const double *v_host, const double *weight_host, double sigma_, double tau_, int positivity_,
              pfbhip_comm *comm_)
        : psi(psi_), comm(comm_), gamma(gamma_), sigma(sigma_), tau(tau_), positivity(positivity_)
    {
        PFB_REQUIRE(psi && xtilde_host && x_host && v_host, "bad arguments");
        PFB_REQUIRE(positivity >= 0 && positivity <= 2, "positivity mode %d", positivity);
        PFB_REQUIRE(gamma != 0.0, "gamma must be non-zero");
        int64_t nx, ny, nxmax, nymax;
        int nbasis;
        psi_geometry(psi, &nx, &ny, &nbasis, &nxmax, &nymax);
        bands = PsfHessBands(pcs, nband, nparts, psf_slots, beam_slots, scale, eta, nx, ny);
        npix = bands.npix();
        cube = size_t(nbasis) * size_t(nxmax) * size_t(nymax);
        nimg = size_t(nband) * npix;
        ncoef = size_t(nband) * cube;
        st = bands.stream();
        xa.alloc(nimg);
        xb.alloc(nimg);
        xout.alloc(nimg);
        xt.alloc(nimg);
        d.alloc(npix);
        va.alloc(ncoef);
        vb.alloc(ncoef);
        vext.alloc(ncoef);
        w.alloc(cube);
        if (comm) sum.alloc(cube);
        partials.alloc(3 * size_t(CG_BLOCKS));
        hpart.resize(3 * size_t(CG_BLOCKS));
        xp = xa.p;
        x = xb.p;
        vp = va.p;
        v = vb.p;
        run.has_weight = weight_host != nullptr;
        synced(st, [&] {
            PFB_HIP(hipMemcpyAsync(xp, x_host, nimg * sizeof(double), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(xt.p, xtilde_host, nimg * sizeof(double), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(vp, v_host, ncoef * sizeof(double), hipMemcpyHostToDevice, st));
            if (weight_host) PFB_HIP(hipMemcpyAsync(w.p, weight_host, cube * sizeof(double), hipMemcpyHostToDevice, st));
        });
    }
};

namespace {

// One iteration enqueued on h->st: v <- Psi^H xp ; dual update and extrapolation ; xout_b <- Psi vext_b + grad(xp)_b ;
// primal step, positivity and the norm partials.  Stage clocks: Psi^H analysis, dual update, Psi synthesis, the
// PSF-approximate Hessian applies, primal step + norms -- what bench.py's C4 roofline is computed from.
void pd_iteration(pfbhip_pd *h, double lam, StageTimer &clk)
{
    const hipStream_t st = h->st;
    const int64_t nband = h->bands.nband();
    const size_t npix = h->npix, cube = h->cube;
    clk.begin(0);
    for (int64_t b = 0; b < nband; ++b) psi_dot_async(h->psi, h->xp + size_t(b) * npix, h->v + size_t(b) * cube);
    clk.end();
    clk.begin(1);
    if (h->comm == nullptr) {
        l21_fused_async(h->vp, h->v, h->vext.p, nband, int64_t(cube), lam, h->sigma, h->w.p, st);  // one pass over the cubes
    } else {  // the bands of this rank only: the band sum of vtilde is completed with ONE all-reduce per iteration
        l21_localsum_async(h->vp, h->v, nband, int64_t(cube), h->sigma, h->sum.p, st);
        PFB_HIP(hipStreamSynchronize(st));
        PFB_CHECK_STATUS(pfbhip_comm_allreduce_sum(h->comm, h->sum.p, h->sum.p, int64_t(cube)));
        l21_apply_async(h->vp, h->v, h->vext.p, nband, int64_t(cube), lam, h->sigma, h->w.p, h->sum.p, st);
    }
    clk.end();
    for (int64_t b = 0; b < nband; ++b) {  // synthesis, d = xtilde - xp, the partition applies accumulating
        double *xo = h->xout.p + size_t(b) * npix;
        clk.begin(2);
        psi_hdot_async(h->psi, h->vext.p + size_t(b) * cube, xo);
        clk.end();
        hipLaunchKernelGGL(k_diff, blocks1d(int64_t(npix)), dim3(256), 0, st, h->xt.p + size_t(b) * npix, h->xp + size_t(b) * npix, h->d.p,
                           int64_t(npix));
        h->bands.apply(b, h->d.p, xo, -1.0, h->gamma, true, &clk, 3);
    }
    clk.begin(4);
    const bool flag_spans_ranks = h->comm != nullptr && h->positivity == 2;  // "any band <= 0" needs the other ranks' bands
    if (nband <= LOOP_MAXB && !flag_spans_ranks) {
        hipLaunchKernelGGL(k_pd_step, dim3(CG_BLOCKS), dim3(CG_THREADS), 0, st, int64_t(npix), int(nband), h->x, h->xp, h->xout.p, h->tau,
                           h->positivity, h->partials.p);
    } else {
        hipLaunchKernelGGL(k_pd_primal, blocks1d(int64_t(h->nimg)), dim3(256), 0, st, h->x, h->xp, h->xout.p, h->tau, int64_t(h->nimg));
        if (flag_spans_ranks) {
            positivity_flag_async(h->x, nband, int64_t(npix), h->d.p, st);
            PFB_HIP(hipStreamSynchronize(st));
            PFB_CHECK_STATUS(pfbhip_comm_allreduce_sum(h->comm, h->d.p, h->d.p, int64_t(npix)));
            positivity_zero_async(h->x, nband, int64_t(npix), h->d.p, st);
        } else if (h->positivity) {
            positivity_async(h->x, nband, int64_t(npix), h->positivity, st);
        }
        hipLaunchKernelGGL(k_pd_norms, dim3(CG_BLOCKS), dim3(CG_THREADS), 0, st, int64_t(h->nimg), h->x, h->xp, h->partials.p);
    }
    clk.end();
    PFB_HIP(hipGetLastError());
}

// Iterates from where the handle stands until eps < tol (returns 0) or iteration maxit - 1 ran (returns 1).  One host
// round trip per iteration: the norm partials, summed over the ranks when there is a communicator.
int pd_loop(pfbhip_pd *h, double lam, double tol, int maxit, StageTimer &clk)
{
    for (;;) {
        // complete the previous iteration: xp <- x, vp <- v (primal_dual.py:434-435)
        if (h->run.complete(h->x, h->xp)) std::swap(h->v, h->vp);
        pd_iteration(h, lam, clk);
        double s[3];  // |x - xp|^2, |x|^2, #nonzero(x)
        fetch_partials<3>(h->partials.p, h->hpart, h->st, s);
        h->traffic.norm_bytes += int64_t(h->hpart.size() * sizeof(double));
        if (h->comm != nullptr) {  // the norms are over ALL bands
            PFB_HIP(hipMemcpyAsync(h->partials.p, s, sizeof s, hipMemcpyHostToDevice, h->st));
            PFB_HIP(hipStreamSynchronize(h->st));
            PFB_CHECK_STATUS(pfbhip_comm_allreduce_sum(h->comm, h->partials.p, h->partials.p, 3));
            PFB_HIP(hipMemcpy(s, h->partials.p, sizeof s, hipMemcpyDeviceToHost));
        }
        h->run.eps = rel_change_eps(s[0], s[1], s[2]);
        h->run.pending = true;
        if (h->run.eps < tol) {
            ++h->traffic.events;
            return 0;
        }
        if (h->run.k + 1 >= maxit) return 1;
    }
}

// One run of the loop with Psi and the plans on the handle's stream; the wall clock brackets the loop alone (every
// iteration ends with a stream synchronisation).  Leaves the iterate in h->x and the dual in h->v.
void pd_solve(pfbhip_pd *h, double lam, double tol, int maxit, bool clock_on, pfbhip_pd_info *info)
{
    StreamScope scope(h->psi, h->bands, h->st);
    StageTimer clk(h->st, clock_on);
    PFB_HIP(hipStreamSynchronize(h->st));
    const auto t0 = std::chrono::steady_clock::now();
    const int status = pd_loop(h, lam, tol, maxit, clk);
    h->run.loop_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    clk.collect(h->run.stage_ms, h->run.stage_calls);
    if (info) {
        info->iters = h->run.k;  // the reference reports the loop index of the last iteration
        info->status = status;
        info->eps = h->run.eps;
        info->loop_ms = h->run.loop_ms;
        h->run.stages_to(info->stage_ms, info->stage_calls);
    }
}

}  // namespace

extern "C" {

int pfbhip_primal_dual(pfbhip_psi *psi, pfbhip_psfconv *const *pcs, int64_t nband, const int64_t *nparts, const int64_t *psf_slots,
                       const int64_t *beam_slots, const double *scale, const double *eta, const double *xtilde_host, double gamma,
                       double *x_host, double *v_host, const double *weight_host, double lam, double sigma, double tau,
                       int positivity, double tol, int maxit, pfbhip_comm *comm, pfbhip_pd_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(weight_host && maxit >= 1, "bad arguments");
        pfbhip_pd h(psi, pcs, nband, nparts, psf_slots, beam_slots, scale, eta, xtilde_host, gamma, x_host, v_host, weight_host, sigma,
                    tau, positivity, comm);
        synced(h.st, [&] {
            pd_solve(&h, lam, tol, maxit, info != nullptr && maxit <= 64, info);
            PFB_HIP(hipMemcpyAsync(x_host, h.x, h.nimg * sizeof(double), hipMemcpyDeviceToHost, h.st));
            PFB_HIP(hipMemcpyAsync(v_host, h.v, h.ncoef * sizeof(double), hipMemcpyDeviceToHost, h.st));
        });
    });
}

// ---- the resumable form: the state of one solve kept in HBM between runs (convergence events), single process -------

int pfbhip_pd_create(pfbhip_psi *psi, pfbhip_psfconv *const *pcs, int64_t nband, const int64_t *nparts, const int64_t *psf_slots,
                     const int64_t *beam_slots, const double *scale, const double *eta, const double *xtilde_host, double gamma,
                     const double *x_host, const double *v_host, const double *weight_host, double sigma, double tau, int positivity,
                     pfbhip_pd **out)
{
    return guarded([&] {
        PFB_REQUIRE(out, "bad arguments");
        std::unique_ptr<pfbhip_pd> h(new pfbhip_pd(psi, pcs, nband, nparts, psf_slots, beam_slots, scale, eta, xtilde_host, gamma, x_host,
                                                   v_host, weight_host, sigma, tau, positivity, nullptr));
        *out = h.release();
    });
}

int pfbhip_pd_set_weight(pfbhip_pd *h, const double *weight_host)
{
    return guarded([&] {
        PFB_REQUIRE(h && weight_host, "NULL argument");
        h->run.set_weight(h->w.p, weight_host, h->cube, hipMemcpyHostToDevice, h->st);
        h->traffic.h2d_bytes += int64_t(h->cube * sizeof(double));
    });
}

int pfbhip_pd_set_weight_dev(pfbhip_pd *h, const double *weight_dev)
{
    return guarded([&] {
        PFB_REQUIRE(h && weight_dev, "NULL argument");
        h->run.set_weight(h->w.p, weight_dev, h->cube, hipMemcpyDeviceToDevice, h->st);
    });
}

int pfbhip_pd_iterate_dev(pfbhip_pd *h, const double **x_dev)
{
    return guarded([&] {
        PFB_REQUIRE(h && x_dev, "NULL argument");
        *x_dev = h->run.iterate(h->x, h->xp);
    });
}

int pfbhip_pd_run(pfbhip_pd *h, double lam, double tol, int maxit, double *x_host, pfbhip_pd_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(h && x_host && maxit >= 1, "bad arguments");
        h->run.require_runnable(maxit);
        synced(h->st, [&] {
            pd_solve(h, lam, tol, maxit, maxit <= 64, info);
            PFB_HIP(hipMemcpyAsync(x_host, h->x, h->nimg * sizeof(double), hipMemcpyDeviceToHost, h->st));
        });
        h->traffic.d2h_bytes += int64_t(h->nimg * sizeof(double));
    });
}

int pfbhip_pd_get_dual(pfbhip_pd *h, double *v_host)
{
    return guarded([&] {
        PFB_REQUIRE(h && v_host, "NULL argument");
        synced(h->st, [&] {  // the dual of the last iteration run (the start value before the first)
            PFB_HIP(hipMemcpyAsync(v_host, h->run.iterate(h->v, h->vp), h->ncoef * sizeof(double), hipMemcpyDeviceToHost, h->st));
        });
        h->traffic.d2h_bytes += int64_t(h->ncoef * sizeof(double));
    });
}

int pfbhip_pd_get_traffic(const pfbhip_pd *h, pfbhip_pd_traffic *out)
{
    return guarded([&] {
        PFB_REQUIRE(h && out, "NULL argument");
        *out = h->traffic;
    });
}

int pfbhip_pd_destroy(pfbhip_pd *h)
{
    return guarded([&] { delete h; });
}

int pfbhip_psfconv_power_method(pfbhip_psfconv *const *pcs, int64_t nband, const int64_t *nparts, const int64_t *psf_slots,
                                const int64_t *beam_slots, const double *scale, const double *eta, double *b_host, double tol,
                                int maxit, pfbhip_comm *comm, pfbhip_pm_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(b_host && maxit >= 0, "bad arguments");
        const PsfHessBands bands(pcs, nband, nparts, psf_slots, beam_slots, scale, eta);
        const size_t npix = bands.npix(), nimg = size_t(nband) * npix;
        hipStream_t st = bands.stream();
        StreamScope scope(nullptr, bands, st);
        DevBuf<double> bp(nimg), red(comm != nullptr ? 3 : 0);
        DevPower pm(int64_t(nimg), st);
        auto aop = [&](const double *in, double *out) {
            for (int64_t b = 0; b < nband; ++b) bands.apply(b, in + size_t(b) * npix, out + size_t(b) * npix, 1.0, 1.0, false);
        };
        auto allreduce = [&](double *s) {
            if (comm == nullptr) return;
            PFB_HIP(hipMemcpyAsync(red.p, s, 3 * sizeof(double), hipMemcpyHostToDevice, st));
            PFB_HIP(hipStreamSynchronize(st));
            PFB_CHECK_STATUS(pfbhip_comm_allreduce_sum(comm, red.p, red.p, 3));
            PFB_HIP(hipMemcpy(s, red.p, 3 * sizeof(double), hipMemcpyDeviceToHost));
        };
        synced(st, [&] {
            PFB_HIP(hipMemcpyAsync(bp.p, b_host, nimg * sizeof(double), hipMemcpyHostToDevice, st));
            pm.run(aop, allreduce, bp.p, tol, maxit, info);
            PFB_HIP(hipMemcpyAsync(b_host, bp.p, nimg * sizeof(double), hipMemcpyDeviceToHost, st));
        });
    });
}

}  // extern "C"
