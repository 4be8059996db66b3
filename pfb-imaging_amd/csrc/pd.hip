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

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <chrono>

#include "common.hpp"
#include "devcg.hpp"
#include "pipeline_api.hpp"

// a failed C-ABI call inside the driver (its message is already in pfbhip_last_error())
#define PFB_CHECK_STATUS(call)                                                    \
    do {                                                                          \
        if ((call) != 0) throw std::runtime_error(std::string(pfbhip_last_error())); \
    } while (0)

namespace pfbhip {

__global__ void __launch_bounds__(256) k_pd_diff(const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ d,
                                                 int64_t n)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i < n) d[i] = a[i] - b[i];
}
__global__ void __launch_bounds__(256) k_pd_primal(double *__restrict__ x, const double *__restrict__ xp,
                                                   const double *__restrict__ xout, double tau, int64_t n)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i < n) x[i] = xp[i] - tau * xout[i];
}
// Primal step, positivity and the three norms in ONE pass over the images (all bands of a pixel in the same thread):
// x = xp - tau xout ; mode 1: clamp negatives, mode 2: zero the pixel in every band where any band is <= 0
// (positivity.py:12-33) ; partials [0] = |x - xp|^2, [1] = |x|^2, [2] = #nonzero(x).  nband <= PD_MAXB.
constexpr int PD_MAXB = 16;
static __global__ void __launch_bounds__(CG_THREADS) k_pd_step(int64_t npix, int nband, double *__restrict__ x,
                                                                const double *__restrict__ xp, const double *__restrict__ xout,
                                                                double tau, int mode, double *partials)
{
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = blockIdx.x * int64_t(CG_THREADS) + threadIdx.x; i < npix; i += int64_t(CG_BLOCKS) * CG_THREADS) {
        double xs[PD_MAXB], ps[PD_MAXB];
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


// Swaps Psi's and the plans' streams to the solve's stream and restores them on exit.
struct PdStreamScope {
    pfbhip_psi *psi;
    hipStream_t psi_prev;
    std::vector<std::pair<pfbhip_psfconv *, hipStream_t>> plans;
    PdStreamScope(pfbhip_psi *p, pfbhip_psfconv *const *pcs, int64_t nband, hipStream_t st) : psi(p), psi_prev(psi_swap_stream(p, st))
    {
        for (int64_t b = 1; b < nband; ++b) {
            bool seen = pcs[b] == pcs[0];
            for (auto &pr : plans) seen = seen || pr.first == pcs[b];
            if (!seen) plans.emplace_back(pcs[b], psfconv_swap_stream(pcs[b], st));
        }
    }
    ~PdStreamScope()
    {
        (void)psi_swap_stream(psi, psi_prev);
        for (auto it = plans.rbegin(); it != plans.rend(); ++it) {
            try {
                (void)psfconv_swap_stream(it->first, it->second);
            } catch (...) {
            }
        }
    }
};

// Stage clocks (HIP events on the loop's stream, read back after the loop): Psi^H analysis, dual update, Psi synthesis, the
// PSF-approximate Hessian applies, primal step + norms -- what bench.py's C4 roofline is computed from.  `on` only for a
// bounded number of events (maxit <= 64: short, benchmark-style runs).
struct PdStageClock {
    hipStream_t st;
    bool on;
    std::vector<hipEvent_t> ev;
    std::vector<int> stage;
    void begin(int s)
    {
        if (!on) return;
        hipEvent_t a, b;
        PFB_HIP(hipEventCreate(&a));
        PFB_HIP(hipEventCreate(&b));
        PFB_HIP(hipEventRecord(a, st));
        ev.push_back(a);
        ev.push_back(b);
        stage.push_back(s);
    }
    void end()
    {
        if (on) PFB_HIP(hipEventRecord(ev.back(), st));
    }
    // adds the bracketed times to ms / calls (after the stream was synchronised)
    void read(double *ms, int64_t *calls) const
    {
        for (size_t i = 0; i < stage.size(); ++i) {
            float e = 0.f;
            PFB_HIP(hipEventElapsedTime(&e, ev[2 * i], ev[2 * i + 1]));
            ms[stage[i]] += double(e);
            calls[stage[i]] += 1;
        }
    }
    ~PdStageClock()
    {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
};

// What one iteration works on: the problem (borrowed pointers) and the buffers.  (x, xp) and (v, vp) rotate outside.
struct PdProblem {
    pfbhip_psi *psi;
    pfbhip_psfconv *const *pcs;
    int64_t nband;
    const int64_t *off, *psf_slots, *beam_slots;
    const double *scale, *eta;
    double gamma, sigma, tau;
    int positivity;
    size_t npix, cube;
    hipStream_t st;
    double *xt, *d, *xout, *vext, *w, *partials;
};
static dim3 pd_blocks(size_t n) { return dim3(uint32_t(ceil_div(int64_t(n), 256))); }

// xout_b <- Psi vext_b + grad(xp)_b for every band: synthesis, d = xtilde - xp, the partition applies accumulating
static void pd_gradient(const PdProblem &p, const double *xp, PdStageClock &clk)
{
    for (int64_t b = 0; b < p.nband; ++b) {
        double *xo = p.xout + size_t(b) * p.npix;
        clk.begin(2);
        psi_hdot_async(p.psi, p.vext + size_t(b) * p.cube, xo);
        clk.end();
        hipLaunchKernelGGL(k_pd_diff, pd_blocks(p.npix), dim3(256), 0, p.st, p.xt + size_t(b) * p.npix, xp + size_t(b) * p.npix, p.d,
                           int64_t(p.npix));
        for (int64_t q = p.off[b]; q < p.off[b + 1]; ++q) {
            clk.begin(3);
            psfconv_apply_async(p.pcs[b], p.d, p.psf_slots[q], p.beam_slots[q], 0, 0.0, -p.scale[b] / p.gamma,
                                q == p.off[b] ? -p.eta[b] / p.gamma : 0.0, 1, xo);
            clk.end();
        }
    }
}

// One iteration with all bands on this device, enqueued on p.st: v <- Psi^H xp ; dual update and extrapolation in one pass ;
// xout ; primal step, positivity and the norm partials.  The single-process body of pfbhip_primal_dual and pfbhip_pd_run.
static void pd_iteration_local(const PdProblem &p, double lam, double *x, const double *xp, double *v, const double *vp,
                               PdStageClock &clk)
{
    const size_t nimg = size_t(p.nband) * p.npix;
    clk.begin(0);
    for (int64_t b = 0; b < p.nband; ++b) psi_dot_async(p.psi, xp + size_t(b) * p.npix, v + size_t(b) * p.cube);
    clk.end();
    clk.begin(1);
    l21_fused_async(vp, v, p.vext, p.nband, int64_t(p.cube), lam, p.sigma, p.w, p.st);  // one pass over the cubes
    clk.end();
    pd_gradient(p, xp, clk);
    clk.begin(4);
    if (p.nband <= PD_MAXB) {
        hipLaunchKernelGGL(k_pd_step, dim3(CG_BLOCKS), dim3(CG_THREADS), 0, p.st, int64_t(p.npix), int(p.nband), x, xp, p.xout, p.tau,
                           p.positivity, p.partials);
    } else {
        hipLaunchKernelGGL(k_pd_primal, pd_blocks(nimg), dim3(256), 0, p.st, x, xp, p.xout, p.tau, int64_t(nimg));
        if (p.positivity) positivity_async(x, p.nband, int64_t(p.npix), p.positivity, p.st);
        hipLaunchKernelGGL(k_pd_norms, dim3(CG_BLOCKS), dim3(CG_THREADS), 0, p.st, int64_t(nimg), x, xp, p.partials);
    }
    clk.end();
    PFB_HIP(hipGetLastError());
}

// Downloads the norm partials (synchronises the stream) and adds them in block order: |x - xp|^2, |x|^2, #nonzero(x)
static void pd_fetch_norms(const PdProblem &p, std::vector<double> &hpart, double *num, double *den, double *nnz)
{
    PFB_HIP(hipMemcpyAsync(hpart.data(), p.partials, hpart.size() * sizeof(double), hipMemcpyDeviceToHost, p.st));
    PFB_HIP(hipStreamSynchronize(p.st));
    *num = *den = *nnz = 0.0;
    for (int i = 0; i < CG_BLOCKS; ++i) {
        *num += hpart[size_t(i)];
        *den += hpart[size_t(CG_BLOCKS) + size_t(i)];
        *nnz += hpart[2 * size_t(CG_BLOCKS) + size_t(i)];
    }
}
// _nb_norm_diff, primal_dual.py:40-52, 429
static double pd_eps(double num, double den, double nnz) { return nnz > 0.0 ? std::sqrt(num / std::max(den, 1e-12)) : 1.0; }

}  // namespace pfbhip

using namespace pfbhip;

extern "C" {

int pfbhip_primal_dual(pfbhip_psi *psi, pfbhip_psfconv *const *pcs, int64_t nband, const int64_t *nparts, const int64_t *psf_slots,
                       const int64_t *beam_slots, const double *scale, const double *eta, const double *xtilde_host, double gamma,
                       double *x_host, double *v_host, const double *weight_host, double lam, double sigma, double tau,
                       int positivity, double tol, int maxit, pfbhip_comm *comm, pfbhip_pd_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(psi && pcs && nparts && psf_slots && beam_slots && scale && eta && xtilde_host && x_host && v_host &&
                        weight_host && nband >= 1 && maxit >= 1,
                    "bad arguments");
        PFB_REQUIRE(positivity >= 0 && positivity <= 2, "positivity mode %d", positivity);
        PFB_REQUIRE(gamma != 0.0, "gamma must be non-zero");
        int64_t nx, ny, nxmax, nymax, px, py;
        int nbasis;
        psi_geometry(psi, &nx, &ny, &nbasis, &nxmax, &nymax);
        for (int64_t b = 0; b < nband; ++b) {
            PFB_REQUIRE(pcs[b] != nullptr, "band %lld has no PSF plan", (long long)b);
            psfconv_geometry(pcs[b], &px, &py);
            PFB_REQUIRE(px == nx && py == ny, "Psi is (%lld, %lld) but the PSF plan of band %lld is (%lld, %lld)", (long long)nx,
                        (long long)ny, (long long)b, (long long)px, (long long)py);
        }
        const size_t npix = size_t(nx) * size_t(ny), cube = size_t(nbasis) * size_t(nxmax) * size_t(nymax);
        const size_t nimg = size_t(nband) * npix, ncoef = size_t(nband) * cube;
        // one stream for everything: the first plan's; Psi and the other plans are switched to it for the call
        hipStream_t st = psfconv_stream(pcs[0]);
        PdStreamScope scope(psi, pcs, nband, st);

        // Buffer rotation instead of copies: xa / xb alternate as (x, xp); va / vb alternate as (dual, previous
        // dual); vext holds the extrapolated dual 2 v - vp of the current iteration.
        DevBuf<double> xa(nimg), xb(nimg), xout(nimg), xt(nimg), d(npix), va(ncoef), vb(ncoef), vext(ncoef), w(cube);
        DevBuf<double> sum(comm != nullptr ? cube : 0);
        DevBuf<double> partials(3 * size_t(CG_BLOCKS));
        std::vector<double> hpart(3 * size_t(CG_BLOCKS));
        double *xp = xa.p, *x = xb.p, *vp = va.p, *v = vb.p;
        PFB_HIP(hipMemcpyAsync(xp, x_host, nimg * sizeof(double), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(xt.p, xtilde_host, nimg * sizeof(double), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(vp, v_host, ncoef * sizeof(double), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(w.p, weight_host, cube * sizeof(double), hipMemcpyHostToDevice, st));
        std::vector<int64_t> off(size_t(nband) + 1, 0);
        for (int64_t b = 0; b < nband; ++b) {
            PFB_REQUIRE(nparts[b] >= 1, "band %lld has no partitions", (long long)b);
            off[size_t(b) + 1] = off[size_t(b)] + nparts[b];
        }
        PdStageClock clk{st, info != nullptr && maxit <= 64, {}, {}};
        const PdProblem prob{psi, pcs, nband, off.data(), psf_slots, beam_slots, scale, eta, gamma, sigma, tau, positivity, npix, cube, st,
                             xt.p, d.p, xout.p, vext.p, w.p, partials.p};
        double eps = 1.0;
        int k = 0, status = 1;
        const auto t_loop0 = std::chrono::steady_clock::now();  // (the stream is idle here: the uploads above were synchronised)
        PFB_HIP(hipStreamSynchronize(st));
        for (; k < maxit; ++k) {
            double num, den, nnz;
            if (comm == nullptr) {
                pd_iteration_local(prob, lam, x, xp, v, vp, clk);
            } else {
                clk.begin(0);
                for (int64_t b = 0; b < nband; ++b) psi_dot_async(psi, xp + size_t(b) * npix, v + size_t(b) * cube);
                clk.end();
                // the bands of this rank only: the band sum of vtilde is completed with ONE all-reduce per iteration
                clk.begin(1);
                l21_localsum_async(vp, v, nband, int64_t(cube), sigma, sum.p, st);
                PFB_HIP(hipStreamSynchronize(st));
                PFB_CHECK_STATUS(pfbhip_comm_allreduce_sum(comm, sum.p, sum.p, int64_t(cube)));
                l21_apply_async(vp, v, vext.p, nband, int64_t(cube), lam, sigma, w.p, sum.p, st);
                clk.end();
                pd_gradient(prob, xp, clk);
                clk.begin(4);
                if (positivity != 2 && nband <= PD_MAXB) {
                    hipLaunchKernelGGL(k_pd_step, dim3(CG_BLOCKS), dim3(CG_THREADS), 0, st, int64_t(npix), int(nband), x, xp, xout.p, tau,
                                       positivity, partials.p);
                } else {
                    hipLaunchKernelGGL(k_pd_primal, pd_blocks(nimg), dim3(256), 0, st, x, xp, xout.p, tau, int64_t(nimg));
                    if (positivity == 2) {  // "any band <= 0" spans the ranks
                        positivity_flag_async(x, nband, int64_t(npix), d.p, st);
                        PFB_HIP(hipStreamSynchronize(st));
                        PFB_CHECK_STATUS(pfbhip_comm_allreduce_sum(comm, d.p, d.p, int64_t(npix)));
                        positivity_zero_async(x, nband, int64_t(npix), d.p, st);
                    } else if (positivity) {
                        positivity_async(x, nband, int64_t(npix), positivity, st);
                    }
                    hipLaunchKernelGGL(k_pd_norms, dim3(CG_BLOCKS), dim3(CG_THREADS), 0, st, int64_t(nimg), x, xp, partials.p);
                }
                clk.end();
                PFB_HIP(hipGetLastError());
            }
            pd_fetch_norms(prob, hpart, &num, &den, &nnz);
            if (comm != nullptr) {  // the norms are over ALL bands
                const double loc[3] = {num, den, nnz};
                double tot[3];
                PFB_HIP(hipMemcpyAsync(partials.p, loc, sizeof loc, hipMemcpyHostToDevice, st));
                PFB_HIP(hipStreamSynchronize(st));
                PFB_CHECK_STATUS(pfbhip_comm_allreduce_sum(comm, partials.p, partials.p, 3));
                PFB_HIP(hipMemcpy(tot, partials.p, sizeof tot, hipMemcpyDeviceToHost));
                num = tot[0];
                den = tot[1];
                nnz = tot[2];
            }
            eps = pd_eps(num, den, nnz);
            if (eps < tol) {
                status = 0;
                break;
            }
            std::swap(x, xp);  // xp <- x
            std::swap(v, vp);  // vp <- v
        }
        // (every iteration ends with a stream synchronisation: the wall clock brackets exactly the device work of the loop)
        const double loop_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_loop0).count();
        // after a break x / v hold the last iterate; after maxit the final swap moved them to xp / vp
        if (status != 0) {
            std::swap(x, xp);
            std::swap(v, vp);
        }
        PFB_HIP(hipMemcpyAsync(x_host, x, nimg * sizeof(double), hipMemcpyDeviceToHost, st));
        PFB_HIP(hipMemcpyAsync(v_host, v, ncoef * sizeof(double), hipMemcpyDeviceToHost, st));
        PFB_HIP(hipStreamSynchronize(st));
        if (info) {
            info->iters = status == 0 ? k : maxit - 1;  // the reference reports the loop index k
            info->status = status;
            info->eps = eps;
            info->loop_ms = loop_ms;
            for (int q = 0; q < PFBHIP_PD_NSTAGES; ++q) {
                info->stage_ms[q] = 0.0;
                info->stage_calls[q] = 0;
            }
            clk.read(info->stage_ms, info->stage_calls);
        }
    });
}

// ---- the resumable form: the state of one solve kept in HBM between runs (convergence events) -------------------
}  // extern "C"

// Single process only (all bands on this device): the kernels of pfbhip_primal_dual's comm == NULL branch, in its order.
struct pfbhip_pd {
    pfbhip_psi *psi = nullptr;
    std::vector<pfbhip_psfconv *> pcs;
    std::vector<int64_t> off, psf_slots, beam_slots;
    std::vector<double> scale, eta;
    int64_t nband = 0;
    size_t npix = 0, nimg = 0, cube = 0, ncoef = 0;
    double gamma = 1.0, sigma = 1.0, tau = 1.0;
    int positivity = 0;
    hipStream_t st = nullptr;  // the first plan's: every launch of the solve goes there
    DevBuf<double> xa, xb, xout, xt, d, va, vb, vext, w, partials;
    double *x = nullptr, *xp = nullptr, *v = nullptr, *vp = nullptr;
    std::vector<double> hpart;
    int k = 0;             // index of the next iteration
    bool pending = false;  // iteration k - 1 ran: (x, xp) and (v, vp) are rotated and k advanced before the next one
    bool has_weight = false;
    double eps = 1.0, loop_ms = 0.0;
    pfbhip_pd_traffic traffic = {};
    double stage_ms[PFBHIP_PD_NSTAGES] = {};
    int64_t stage_calls[PFBHIP_PD_NSTAGES] = {};
};

extern "C" {

int pfbhip_pd_create(pfbhip_psi *psi, pfbhip_psfconv *const *pcs, int64_t nband, const int64_t *nparts, const int64_t *psf_slots,
                     const int64_t *beam_slots, const double *scale, const double *eta, const double *xtilde_host, double gamma,
                     const double *x_host, const double *v_host, const double *weight_host, double sigma, double tau, int positivity,
                     pfbhip_pd **out)
{
    return guarded([&] {
        PFB_REQUIRE(out && psi && pcs && nparts && psf_slots && beam_slots && scale && eta && xtilde_host && x_host && v_host &&
                        nband >= 1,
                    "bad arguments");
        PFB_REQUIRE(positivity >= 0 && positivity <= 2, "positivity mode %d", positivity);
        PFB_REQUIRE(gamma != 0.0, "gamma must be non-zero");
        std::unique_ptr<pfbhip_pd> h(new pfbhip_pd);
        h->psi = psi;
        h->nband = nband;
        h->gamma = gamma;
        h->sigma = sigma;
        h->tau = tau;
        h->positivity = positivity;
        int64_t nx, ny, nxmax, nymax, px, py;
        int nbasis;
        psi_geometry(psi, &nx, &ny, &nbasis, &nxmax, &nymax);
        h->off.assign(size_t(nband) + 1, 0);
        for (int64_t b = 0; b < nband; ++b) {
            PFB_REQUIRE(pcs[b] != nullptr, "band %lld has no PSF plan", (long long)b);
            psfconv_geometry(pcs[b], &px, &py);
            PFB_REQUIRE(px == nx && py == ny, "Psi is (%lld, %lld) but the PSF plan of band %lld is (%lld, %lld)", (long long)nx,
                        (long long)ny, (long long)b, (long long)px, (long long)py);
            PFB_REQUIRE(nparts[b] >= 1, "band %lld has no partitions", (long long)b);
            h->off[size_t(b) + 1] = h->off[size_t(b)] + nparts[b];
            h->pcs.push_back(pcs[b]);
            h->scale.push_back(scale[b]);
            h->eta.push_back(eta[b]);
        }
        h->psf_slots.assign(psf_slots, psf_slots + h->off.back());
        h->beam_slots.assign(beam_slots, beam_slots + h->off.back());
        h->npix = size_t(nx) * size_t(ny);
        h->cube = size_t(nbasis) * size_t(nxmax) * size_t(nymax);
        h->nimg = size_t(nband) * h->npix;
        h->ncoef = size_t(nband) * h->cube;
        h->st = psfconv_stream(pcs[0]);
        h->xa.alloc(h->nimg);
        h->xb.alloc(h->nimg);
        h->xout.alloc(h->nimg);
        h->xt.alloc(h->nimg);
        h->d.alloc(h->npix);
        h->va.alloc(h->ncoef);
        h->vb.alloc(h->ncoef);
        h->vext.alloc(h->ncoef);
        h->w.alloc(h->cube);
        h->partials.alloc(3 * size_t(CG_BLOCKS));
        h->hpart.resize(3 * size_t(CG_BLOCKS));
        h->xp = h->xa.p;
        h->x = h->xb.p;
        h->vp = h->va.p;
        h->v = h->vb.p;
        const hipStream_t st = h->st;
        PFB_HIP(hipMemcpyAsync(h->xp, x_host, h->nimg * sizeof(double), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(h->xt.p, xtilde_host, h->nimg * sizeof(double), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(h->vp, v_host, h->ncoef * sizeof(double), hipMemcpyHostToDevice, st));
        h->has_weight = weight_host != nullptr;  // (NULL: the caller sets the weight before the first run)
        if (weight_host) PFB_HIP(hipMemcpyAsync(h->w.p, weight_host, h->cube * sizeof(double), hipMemcpyHostToDevice, st));
        PFB_HIP(hipStreamSynchronize(st));
        *out = h.release();
    });
}

int pfbhip_pd_set_weight(pfbhip_pd *h, const double *weight_host)
{
    return guarded([&] {
        PFB_REQUIRE(h && weight_host, "NULL argument");
        PFB_HIP(hipMemcpyAsync(h->w.p, weight_host, h->cube * sizeof(double), hipMemcpyHostToDevice, h->st));
        PFB_HIP(hipStreamSynchronize(h->st));
        h->has_weight = true;
        h->traffic.h2d_bytes += int64_t(h->cube * sizeof(double));
    });
}

int pfbhip_pd_set_weight_dev(pfbhip_pd *h, const double *weight_dev)
{
    return guarded([&] {
        PFB_REQUIRE(h && weight_dev, "NULL argument");
        PFB_HIP(hipMemcpyAsync(h->w.p, weight_dev, h->cube * sizeof(double), hipMemcpyDeviceToDevice, h->st));
        PFB_HIP(hipStreamSynchronize(h->st));
        h->has_weight = true;
    });
}

int pfbhip_pd_iterate_dev(pfbhip_pd *h, const double **x_dev)
{
    return guarded([&] {
        PFB_REQUIRE(h && x_dev, "NULL argument");
        *x_dev = h->pending ? h->x : h->xp;  // (before the first iteration the iterate is the start value)
    });
}

int pfbhip_pd_run(pfbhip_pd *h, double lam, double tol, int maxit, double *x_host, pfbhip_pd_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(h && x_host && maxit >= 1, "bad arguments");
        PFB_REQUIRE(h->k + (h->pending ? 1 : 0) < maxit, "iteration %d is past maxit %d", h->k + (h->pending ? 1 : 0), maxit);
        PFB_REQUIRE(h->has_weight, "no weight: created with weight_host == NULL and none set since");
        const hipStream_t st = h->st;
        PdStreamScope scope(h->psi, h->pcs.data(), h->nband, st);
        const PdProblem prob{h->psi, h->pcs.data(), h->nband, h->off.data(), h->psf_slots.data(), h->beam_slots.data(),
                             h->scale.data(), h->eta.data(), h->gamma, h->sigma, h->tau, h->positivity, h->npix, h->cube, st,
                             h->xt.p, h->d.p, h->xout.p, h->vext.p, h->w.p, h->partials.p};
        PdStageClock clk{st, maxit <= 64, {}, {}};
        int status = 1;
        PFB_HIP(hipStreamSynchronize(st));
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            if (h->pending) {  // complete the previous iteration: xp <- x, vp <- v (primal_dual.py:434-435)
                std::swap(h->x, h->xp);
                std::swap(h->v, h->vp);
                ++h->k;
                h->pending = false;
            }
            pd_iteration_local(prob, lam, h->x, h->xp, h->v, h->vp, clk);
            double num, den, nnz;
            pd_fetch_norms(prob, h->hpart, &num, &den, &nnz);
            h->traffic.norm_bytes += int64_t(h->hpart.size() * sizeof(double));
            h->eps = pd_eps(num, den, nnz);
            h->pending = true;
            if (h->eps < tol) {
                status = 0;
                ++h->traffic.events;
                break;
            }
            if (h->k + 1 >= maxit) break;
        }
        h->loop_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        PFB_HIP(hipMemcpyAsync(x_host, h->x, h->nimg * sizeof(double), hipMemcpyDeviceToHost, st));
        PFB_HIP(hipStreamSynchronize(st));
        h->traffic.d2h_bytes += int64_t(h->nimg * sizeof(double));
        clk.read(h->stage_ms, h->stage_calls);
        if (info) {
            info->iters = h->k;
            info->status = status;
            info->eps = h->eps;
            info->loop_ms = h->loop_ms;
            for (int q = 0; q < PFBHIP_PD_NSTAGES; ++q) {
                info->stage_ms[q] = h->stage_ms[q];
                info->stage_calls[q] = h->stage_calls[q];
            }
        }
    });
}

int pfbhip_pd_get_dual(pfbhip_pd *h, double *v_host)
{
    return guarded([&] {
        PFB_REQUIRE(h && v_host, "NULL argument");
        // the dual of the last iteration run (the start value before the first)
        PFB_HIP(hipMemcpyAsync(v_host, h->pending ? h->v : h->vp, h->ncoef * sizeof(double), hipMemcpyDeviceToHost, h->st));
        PFB_HIP(hipStreamSynchronize(h->st));
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
        PFB_REQUIRE(pcs && nparts && psf_slots && beam_slots && scale && eta && b_host && nband >= 1 && maxit >= 0, "bad arguments");
        int64_t nx = 0, ny = 0, px, py;
        for (int64_t b = 0; b < nband; ++b) {
            PFB_REQUIRE(pcs[b] != nullptr, "band %lld has no PSF plan", (long long)b);
            psfconv_geometry(pcs[b], &px, &py);
            if (b == 0) nx = px, ny = py;
            PFB_REQUIRE(px == nx && py == ny, "band %lld is (%lld, %lld), band 0 is (%lld, %lld)", (long long)b, (long long)px,
                        (long long)py, (long long)nx, (long long)ny);
        }
        const size_t npix = size_t(nx) * size_t(ny), nimg = size_t(nband) * npix;
        hipStream_t st = psfconv_stream(pcs[0]);
        struct Restore {
            std::vector<std::pair<pfbhip_psfconv *, hipStream_t>> plans;
            ~Restore()
            {
                for (auto it = plans.rbegin(); it != plans.rend(); ++it) {
                    try {
                        (void)psfconv_swap_stream(it->first, it->second);
                    } catch (...) {
                    }
                }
            }
        } restore;
        for (int64_t b = 1; b < nband; ++b) {
            bool seen = pcs[b] == pcs[0];
            for (auto &pr : restore.plans) seen = seen || pr.first == pcs[b];
            if (!seen) restore.plans.emplace_back(pcs[b], psfconv_swap_stream(pcs[b], st));
        }
        std::vector<int64_t> off(size_t(nband) + 1, 0);
        for (int64_t b = 0; b < nband; ++b) {
            PFB_REQUIRE(nparts[b] >= 1, "band %lld has no partitions", (long long)b);
            off[size_t(b) + 1] = off[size_t(b)] + nparts[b];
        }
        DevBuf<double> bp(nimg), red(comm != nullptr ? 3 : 0);
        PFB_HIP(hipMemcpyAsync(bp.p, b_host, nimg * sizeof(double), hipMemcpyHostToDevice, st));
        DevPower pm(int64_t(nimg), st);
        auto aop = [&](const double *in, double *out) {
            for (int64_t b = 0; b < nband; ++b)
                for (int64_t q = off[size_t(b)]; q < off[size_t(b) + 1]; ++q)
                    psfconv_apply_async(pcs[b], in + size_t(b) * npix, psf_slots[q], beam_slots[q], 0, 0.0, scale[b],
                                        q == off[size_t(b)] ? eta[b] : 0.0, q > off[size_t(b)], out + size_t(b) * npix);
        };
        auto allreduce = [&](double *s) {
            if (comm == nullptr) return;
            PFB_HIP(hipMemcpyAsync(red.p, s, 3 * sizeof(double), hipMemcpyHostToDevice, st));
            PFB_HIP(hipStreamSynchronize(st));
            PFB_CHECK_STATUS(pfbhip_comm_allreduce_sum(comm, red.p, red.p, 3));
            PFB_HIP(hipMemcpy(s, red.p, 3 * sizeof(double), hipMemcpyDeviceToHost));
        };
        pm.run(aop, allreduce, bp.p, tol, maxit, info);
        PFB_HIP(hipMemcpyAsync(b_host, bp.p, nimg * sizeof(double), hipMemcpyDeviceToHost, st));
        PFB_HIP(hipStreamSynchronize(st));
    });
}


}  // extern "C"
