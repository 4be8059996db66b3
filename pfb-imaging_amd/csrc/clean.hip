// clean.hip -- Hogbom and Clark CLEAN with every cube resident in HBM (the kclean minor cycle).
//
// Semantics (deconv/hogbom.py:9-63 and deconv/clark.py:11-143 of pfb-imaging; DESIGN.md "Device-resident CLEAN"):
//   search  = (sum_b r_b)^2 (bands summed in order b = 0, 1, ...), times the mask in Clark's major search only;
//   peak    = the FIRST maximum in row-major order; rmax = sqrt(search[peak]) (IEEE sqrt);
//   loop    while rmax > tol and k < maxit, tol = max(pf * rmax_0, threshold); no stall stop (the reference's never fires).
//   Hogbom  xhat_b = r_b[p,q] / max(psf_b); model_b[p,q] += gamma xhat_b;
//           r_b[i,j] -= (gamma xhat_b) psf_b[nx0 - p + i, ny0 - q + j]  (entries outside the PSF count as 0).
//   Clark   residual = dirty - psfconv(model) after every sub-minor loop; active set = pixels with search > (subpf rmax)^2 in
//           row-major order; sub-minor: model_b[p,q] += (gamma xhat_b) / w_b and
//           a_b[i] -= ((gamma xhat_b) psf_b[nxo2 - (p_i - p), nyo2 - (q_i - q)]) / w_b   (the REFLECTED PSF), where xhat_b is the
//           peak's value before its own update for i <= pq and after it for i > pq (the reference's xhat is a view into a_set).
//           Bands with w_b == 0 are left alone (neither model nor active set changes).
// Every step is two launches (a streaming kernel over the pixels / the active set, then one workgroup that finishes the argmax
// and prepares the next step); the host enqueues steps in growing batches and reads {k, done} back once per batch.  Launches
// after `done` return at once.  Small active sets run their whole sub-minor loop in ONE workgroup with the active set in LDS.
// No FP contraction (Makefile: -ffp-contract=off): float64 results follow the reference's order of operations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"
#include "pipeline_api.hpp"

namespace pfbhip {

constexpr int CL_MAXB = 64;       // bands per plan
constexpr int CL_THREADS = 256;   // streaming kernels
constexpr int CL_MAXBLK = 1024;   // streaming grid cap (4 workgroups per CU): partial slots
constexpr int CL_FIN = 1024;      // the finishing workgroup
constexpr int CL_LDS_THREADS = 1024;
constexpr int64_t CL_LDS_BYTES = 96 * 1024;  // the one-workgroup sub-minor loop keeps nband * A doubles in LDS up to this
constexpr int64_t CL_NONE = INT64_MAX;

// Device state of one loop.  gx / gx2: gamma * xhat_b for the next subtraction (Clark sub-minor: gx for i <= pq, gx2 after).
struct CleanState {
    int64_t p, q, pq;
    int64_t k;       // Hogbom iterations / Clark major iterations
    int64_t ksub;    // iterations of the current sub-minor loop
    int64_t A;       // active-set size
    double r2;       // search value at the peak
    double rmax, tol, subth;
    int32_t done, sdone;
    double gx[CL_MAXB], gx2[CL_MAXB];
};

struct CleanParams {  // by value into the finishing kernels
    double threshold, gamma, pf, subpf;
    int64_t maxit, submaxit;
};

// (value, index) argmax that keeps the first maximum: larger value wins, equal values go to the lower index
__device__ inline void am_merge(double &v, int64_t &i, double v2, int64_t i2)
{
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}
__device__ inline void am_wave(double &v, int64_t &i)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_xor(v, o);
        const int64_t i2 = __shfl_xor(i, o);
        am_merge(v, i, v2, i2);
    }
}
// block argmax; every thread gets the result.  sv / si hold NT / 64 entries.
template <int NT>
__device__ inline void am_block(double &v, int64_t &i, double *sv, int64_t *si)
{
    am_wave(v, i);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sv[w] = v;
        si[w] = i;
    }
    __syncthreads();
    v = sv[0];
    i = si[0];
    for (int k = 1; k < NT / 64; ++k) am_merge(v, i, sv[k], si[k]);
}

// Streaming search over the image: optionally subtract the shifted PSF (Hogbom step), form (sum_b r_b)^2 [* mask], keep it
// in `srch` when asked (Clark major search), and leave the per-workgroup first maximum in pv / pi.
template <bool SUB, bool MASK>
__global__ void __launch_bounds__(CL_THREADS) k_cl_image(const CleanState *__restrict__ st, int nband, int64_t nx, int64_t ny,
                                                       double *__restrict__ r, const double *__restrict__ psf, int64_t nxp,
                                                       int64_t nyp, const double *__restrict__ mask, double *__restrict__ srch,
                                                       double *__restrict__ pv, int64_t *__restrict__ pi)
{
    __shared__ double sv[CL_THREADS / 64];
    __shared__ int64_t si[CL_THREADS / 64];
    if (st->done) return;
    const int64_t npix = nx * ny;
    int64_t p = 0, q = 0;
    if (SUB) {
        p = st->p;
        q = st->q;
    }
    const int64_t x0 = nxp / 2 - p, y0 = nyp / 2 - q;  // psf row / column of pixel (0, 0)
    double bv = -1.0;
    int64_t bi = CL_NONE;
    for (int64_t t = blockIdx.x * int64_t(CL_THREADS) + threadIdx.x; t < npix; t += int64_t(gridDim.x) * CL_THREADS) {
        const int64_t i = t / ny, j = t - i * ny;
        double s = 0.0;
        if (SUB) {
            const int64_t pr = x0 + i, pc = y0 + j;
            const bool in = pr >= 0 && pr < nxp && pc >= 0 && pc < nyp;
            for (int b = 0; b < nband; ++b) {
                double v = r[size_t(b) * size_t(npix) + size_t(t)];
                if (in) {
                    v = v - st->gx[b] * psf[(size_t(b) * size_t(nxp) + size_t(pr)) * size_t(nyp) + size_t(pc)];
                    r[size_t(b) * size_t(npix) + size_t(t)] = v;
                }
                s = s + v;
            }
        } else {
            for (int b = 0; b < nband; ++b) s = s + r[size_t(b) * size_t(npix) + size_t(t)];
        }
        s = s * s;
        if (MASK) s = s * mask[t];
        if (srch) srch[t] = s;
        if (s > bv) {  // increasing t per thread: strict > keeps the first
            bv = s;
            bi = t;
        }
    }
    am_block<CL_THREADS>(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        pv[blockIdx.x] = bv;
        pi[blockIdx.x] = bi;
    }
}

// Sub-minor step over the active set (nband, A): subtract with the reflected PSF, form (sum_b a_b)^2, per-workgroup maximum.
template <bool SUB>
__global__ void __launch_bounds__(CL_THREADS) k_cl_active(const CleanState *__restrict__ st, int nband, double *__restrict__ a,
                                                        const int32_t *__restrict__ pidx, const int32_t *__restrict__ qidx,
                                                        const double *__restrict__ psf, int64_t nxp, int64_t nyp,
                                                        const double *__restrict__ w, double *__restrict__ pv,
                                                        int64_t *__restrict__ pi)
{
    __shared__ double sv[CL_THREADS / 64];
    __shared__ int64_t si[CL_THREADS / 64];
    if (st->done || st->sdone) return;
    const int64_t A = st->A;
    int64_t p = 0, q = 0, pq = 0;
    if (SUB) {
        p = st->p;
        q = st->q;
        pq = st->pq;
    }
    double bv = -1.0;
    int64_t bi = CL_NONE;
    for (int64_t i = blockIdx.x * int64_t(CL_THREADS) + threadIdx.x; i < A; i += int64_t(gridDim.x) * CL_THREADS) {
        double s = 0.0;
        if (SUB) {
            const int64_t pp = nxp / 2 - (pidx[i] - p), qq = nyp / 2 - (qidx[i] - q);
            const bool in = pp >= 0 && pp < nxp && qq >= 0 && qq < nyp;
            for (int b = 0; b < nband; ++b) {
                double v = a[size_t(b) * size_t(A) + size_t(i)];
                const double wb = w[b];
                if (in && wb != 0.0) {
                    const double g = i <= pq ? st->gx[b] : st->gx2[b];
                    v = v - (g * psf[(size_t(b) * size_t(nxp) + size_t(pp)) * size_t(nyp) + size_t(qq)]) / wb;
                    a[size_t(b) * size_t(A) + size_t(i)] = v;
                }
                s = s + v;
            }
        } else {
            for (int b = 0; b < nband; ++b) s = s + a[size_t(b) * size_t(A) + size_t(i)];
        }
        s = s * s;
        if (s > bv) {
            bv = s;
            bi = i;
        }
    }
    am_block<CL_THREADS>(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        pv[blockIdx.x] = bv;
        pi[blockIdx.x] = bi;
    }
}

enum { FIN_HOGBOM = 0, FIN_MAJOR = 1, FIN_SUB = 2 };

// Sub-minor bookkeeping of thread 0 once the peak pq of the active set is known: stop test, then the model update and both
// values of gamma * xhat_b (before / after the peak's own update).  `a` is the active set (global or LDS), stride A.
__device__ inline void sub_finish(CleanState *st, const CleanParams &cp, double v, int64_t pq, bool first, int nband,
                                  const double *a, int64_t A, const int32_t *pidx, const int32_t *qidx,
                                  const double *psf, int64_t nxp, int64_t nyp, const double *w, double *model, int64_t nx,
                                  int64_t ny, int64_t *nminor)
{
    if (pq == CL_NONE) {
        st->sdone = 1;
        return;
    }
    const int64_t p = pidx[pq], q = qidx[pq];
    const double amax = sqrt(v);
    if (!first) {
        st->ksub += 1;
        *nminor += 1;
    }
    if (!(amax > st->subth && st->ksub < cp.submaxit)) {
        st->sdone = 1;
        return;
    }
    st->p = p;
    st->q = q;
    st->pq = pq;
    const size_t c = (size_t(nxp / 2) * size_t(nyp) + size_t(nyp / 2));
    for (int b = 0; b < nband; ++b) {
        const double wb = w[b];
        if (wb == 0.0) {
            st->gx[b] = st->gx2[b] = 0.0;
            continue;
        }
        const double xb = a[size_t(b) * size_t(A) + size_t(pq)];
        const double g = cp.gamma * xb;
        model[(size_t(b) * size_t(nx) + size_t(p)) * size_t(ny) + size_t(q)] += g / wb;
        const double xb2 = xb - (g * psf[size_t(b) * size_t(nxp) * size_t(nyp) + c]) / wb;
        st->gx[b] = g;
        st->gx2[b] = cp.gamma * xb2;
    }
}

__global__ void __launch_bounds__(CL_FIN) k_cl_finish(CleanState *__restrict__ st, CleanParams cp, int mode, int first, int nparts,
                                                    const double *__restrict__ pv, const int64_t *__restrict__ pi, int nband,
                                                    int64_t nx, int64_t ny, const double *__restrict__ r,
                                                    const double *__restrict__ wsum, double *__restrict__ model,
                                                    const double *__restrict__ a, const int32_t *__restrict__ pidx,
                                                    const int32_t *__restrict__ qidx, const double *__restrict__ psf,
                                                    int64_t nxp, int64_t nyp, int64_t *__restrict__ nminor)
{
    __shared__ double sv[CL_FIN / 64];
    __shared__ int64_t si[CL_FIN / 64];
    if (st->done || (mode == FIN_SUB && st->sdone)) return;
    double v = -1.0;
    int64_t idx = CL_NONE;
    for (int k = threadIdx.x; k < nparts; k += CL_FIN) am_merge(v, idx, pv[k], pi[k]);
    am_block<CL_FIN>(v, idx, sv, si);
    if (threadIdx.x != 0) return;
    if (mode == FIN_SUB) {
        sub_finish(st, cp, v, idx, first != 0, nband, a, st->A, pidx, qidx, psf, nxp, nyp, wsum, model, nx, ny, nminor);
        return;
    }
    if (idx == CL_NONE) {  // no comparable value (NaN everywhere): nothing to clean
        st->done = 1;
        return;
    }
    const int64_t p = idx / ny, q = idx - (idx / ny) * ny;
    const double rmax = sqrt(v);
    st->p = p;
    st->q = q;
    st->r2 = v;
    st->rmax = rmax;
    if (first)
        st->tol = fmax(cp.pf * rmax, cp.threshold);
    else
        st->k += 1;
    if (!(rmax > st->tol && st->k < cp.maxit)) {
        st->done = 1;
        return;
    }
    if (mode == FIN_MAJOR) {
        st->subth = cp.subpf * rmax;
        return;
    }
    const size_t o = size_t(p) * size_t(ny) + size_t(q), npix = size_t(nx) * size_t(ny);
    for (int b = 0; b < nband; ++b) {
        const double xh = r[size_t(b) * npix + o] / wsum[b];
        const double g = cp.gamma * xh;
        model[size_t(b) * npix + o] += g;
        st->gx[b] = g;
    }
}

// Order-preserving compaction of {t : srch[t] > subth^2}.  Workgroup g owns the contiguous pixel range [g*chunk, (g+1)*chunk).
__global__ void __launch_bounds__(CL_THREADS) k_cl_count(const CleanState *__restrict__ st, const double *__restrict__ srch,
                                                       int64_t npix, int64_t chunk, int64_t *__restrict__ cnt)
{
    __shared__ int64_t sc[CL_THREADS / 64];
    if (st->done) return;
    const double th2 = st->subth * st->subth;
    const int64_t t0 = blockIdx.x * chunk, t1 = t0 + chunk < npix ? t0 + chunk : npix;
    int64_t c = 0;
    for (int64_t t = t0 + threadIdx.x; t < t1; t += CL_THREADS) c += srch[t] > th2 ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t s = 0;
        for (int k = 0; k < CL_THREADS / 64; ++k) s += sc[k];
        cnt[blockIdx.x] = s;
    }
}

// exclusive prefix sum of the workgroup counts (in place) and A
__global__ void __launch_bounds__(CL_FIN) k_cl_scan(CleanState *__restrict__ st, int64_t *__restrict__ cnt, int n)
{
    __shared__ int64_t s[CL_MAXBLK];
    if (st->done) return;
    for (int k = threadIdx.x; k < CL_MAXBLK; k += CL_FIN) s[k] = k < n ? cnt[k] : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int k = 0; k < n; ++k) {
            const int64_t c = s[k];
            s[k] = run;
            run += c;
        }
        st->A = run;
        st->ksub = 0;
        st->sdone = 0;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += CL_FIN) cnt[k] = s[k];
}

__global__ void __launch_bounds__(CL_THREADS) k_cl_compact(const CleanState *__restrict__ st, const double *__restrict__ srch,
                                                         const double *__restrict__ r, int nband, int64_t nx, int64_t ny,
                                                         int64_t chunk, const int64_t *__restrict__ off,
                                                         int32_t *__restrict__ pidx, int32_t *__restrict__ qidx,
                                                         double *__restrict__ a)
{
    __shared__ int64_t sw[CL_THREADS / 64];
    if (st->done) return;
    const double th2 = st->subth * st->subth;
    const int64_t npix = nx * ny, A = st->A;
    const int64_t t0 = blockIdx.x * chunk, t1 = t0 + chunk < npix ? t0 + chunk : npix;
    int64_t base = off[blockIdx.x];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t t00 = t0; t00 < t1; t00 += CL_THREADS) {
        const int64_t t = t00 + threadIdx.x;
        const bool f = t < t1 && srch[t] > th2;
        const uint64_t m = __ballot(f);
        const int64_t below = __popcll(m & ((uint64_t(1) << lane) - 1));
        if (lane == 0) sw[wv] = __popcll(m);
        __syncthreads();
        int64_t wbase = 0, tot = 0;
        for (int k = 0; k < CL_THREADS / 64; ++k) {
            if (k < wv) wbase += sw[k];
            tot += sw[k];
        }
        if (f) {
            const int64_t o = base + wbase + below;
            const int64_t i = t / ny;
            pidx[o] = int32_t(i);
            qidx[o] = int32_t(t - i * ny);
            for (int b = 0; b < nband; ++b) a[size_t(b) * size_t(A) + size_t(o)] = r[size_t(b) * size_t(npix) + size_t(t)];
        }
        base += tot;
        __syncthreads();
    }
}

// The whole sub-minor loop in one workgroup, active set in LDS (nband * A * 8 <= CL_LDS_BYTES).  Same arithmetic and argmax
// order as k_cl_active + k_cl_finish, no launches between steps.  The loop state lives in LDS too (thread 0 updates it between
// barriers) and goes back to global memory at the end.
__global__ void __launch_bounds__(CL_LDS_THREADS) k_cl_sub_lds(CleanState *__restrict__ st, CleanParams cp, int nband,
                                                             const double *__restrict__ ag, const int32_t *__restrict__ pidx,
                                                             const int32_t *__restrict__ qidx, const double *__restrict__ psf,
                                                             int64_t nxp, int64_t nyp, const double *__restrict__ w,
                                                             double *__restrict__ model, int64_t nx, int64_t ny,
                                                             int64_t *__restrict__ nminor)
{
    extern __shared__ double a[];
    __shared__ double sv[CL_LDS_THREADS / 64];
    __shared__ int64_t si[CL_LDS_THREADS / 64];
    __shared__ CleanState ls;
    __shared__ double lw[CL_MAXB];
    if (st->done) return;
    if (threadIdx.x == 0) ls = *st;
    if (threadIdx.x < nband) lw[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const int64_t A = ls.A, n = int64_t(nband) * A;
    for (int64_t k = threadIdx.x; k < n; k += CL_LDS_THREADS) a[k] = ag[k];
    __syncthreads();
    bool first = true;
    for (;;) {
        const int64_t p = ls.p, q = ls.q, pq = ls.pq;
        double bv = -1.0;
        int64_t bi = CL_NONE;
        for (int64_t i = threadIdx.x; i < A; i += CL_LDS_THREADS) {  // thread-owned entries: no barrier between subtract and search
            double s = 0.0;
            if (!first) {
                const int64_t pp = nxp / 2 - (pidx[i] - p), qq = nyp / 2 - (qidx[i] - q);
                const bool in = pp >= 0 && pp < nxp && qq >= 0 && qq < nyp;
                for (int b = 0; b < nband; ++b) {
                    double v = a[b * A + i];
                    const double wb = lw[b];
                    if (in && wb != 0.0) {
                        const double g = i <= pq ? ls.gx[b] : ls.gx2[b];
                        v = v - (g * psf[(size_t(b) * size_t(nxp) + size_t(pp)) * size_t(nyp) + size_t(qq)]) / wb;
                        a[b * A + i] = v;
                    }
                    s = s + v;
                }
            } else {
                for (int b = 0; b < nband; ++b) s = s + a[b * A + i];
            }
            s = s * s;
            if (s > bv) {
                bv = s;
                bi = i;
            }
        }
        am_block<CL_LDS_THREADS>(bv, bi, sv, si);  // its barriers order every thread's LDS updates before the peak is read
        if (threadIdx.x == 0)
            sub_finish(&ls, cp, bv, bi, first, nband, a, A, pidx, qidx, psf, nxp, nyp, lw, model, nx, ny, nminor);
        __syncthreads();
        if (ls.sdone) break;
        first = false;
    }
    if (threadIdx.x == 0) *st = ls;
}

// what the host reads back once per batch (pinned memory)
struct CleanHostState {
    int64_t k, A, nminor;
    int32_t done, sdone;
    double rmax;
};
__global__ void k_cl_readback(const CleanState *__restrict__ s, const int64_t *__restrict__ nm, CleanHostState *__restrict__ h)
{
    if (threadIdx.x == 0) {
        h->k = s->k;
        h->A = s->A;
        h->nminor = *nm;
        h->done = s->done;
        h->sdone = s->sdone;
        h->rmax = s->rmax;
    }
}

}  // namespace pfbhip

using namespace pfbhip;

struct pfbhip_clean {
    int64_t nband = 0, nx = 0, ny = 0, nxp = 0, nyp = 0;
    hipStream_t stream = nullptr;  // the psfconv plan's stream when there is one
    hipStream_t own_stream = nullptr;
    pfbhip_psfconv *pc = nullptr;  // Clark's major-cycle convolution: psfhat of band b in slot b
    DevBuf<double> psf, dirty, resid, model, srch, aset, wsum, mask, pv;
    DevBuf<int64_t> pi, cnt, nminor;
    DevBuf<int32_t> pidx, qidx;
    DevBuf<CleanState> st;
    std::vector<double> psf_peak;
    CleanHostState *hs = nullptr;  // pinned read-back
    hipEvent_t ev_sync = nullptr;
    ~pfbhip_clean()
    {
        if (hs) (void)hipHostFree(hs);
        if (ev_sync) (void)hipEventDestroy(ev_sync);
        if (pc) (void)pfbhip_psfconv_destroy(pc);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
    int64_t npix() const { return nx * ny; }
    int grid(int64_t n) const { return int(std::max<int64_t>(1, std::min<int64_t>(CL_MAXBLK, ceil_div(n, CL_THREADS)))); }

    // {k, done, A, ...} back to the host through the pinned block: the only synchronisation of a batch
    void read_state()
    {
        hipLaunchKernelGGL(k_cl_readback, dim3(1), dim3(64), 0, stream, st.p, nminor.p, hs);
        PFB_HIP(hipGetLastError());
        PFB_HIP(hipEventRecord(ev_sync, stream));
        PFB_HIP(hipEventSynchronize(ev_sync));
    }
    void reset_state()
    {
        PFB_HIP(hipMemsetAsync(st.p, 0, sizeof(CleanState), stream));
        PFB_HIP(hipMemsetAsync(nminor.p, 0, sizeof(int64_t), stream));
    }
    void image_search(bool sub, bool masked, bool keep)
    {
        const int g = grid(npix());
        auto kern = sub ? k_cl_image<true, false> : (masked ? k_cl_image<false, true> : k_cl_image<false, false>);
        hipLaunchKernelGGL(kern, dim3(g), dim3(CL_THREADS), 0, stream, st.p, int(nband), nx, ny, resid.p, psf.p, nxp, nyp,
                           mask.p, keep ? srch.p : nullptr, pv.p, pi.p);
        PFB_HIP(hipGetLastError());
        last_parts = g;
    }
    void finish(const CleanParams &cp, int mode, bool first)
    {
        hipLaunchKernelGGL(k_cl_finish, dim3(1), dim3(CL_FIN), 0, stream, st.p, cp, mode, int(first), last_parts, pv.p, pi.p,
                           int(nband), nx, ny, resid.p, wsum.p, model.p, aset.p, pidx.p, qidx.p, psf.p, nxp, nyp, nminor.p);
        PFB_HIP(hipGetLastError());
    }
    int last_parts = 1;
};

namespace {

void check_params(double gamma, double pf, int64_t maxit)
{
    PFB_REQUIRE(gamma > 0.0 && std::isfinite(gamma), "gamma must be > 0 (got %g)", gamma);
    PFB_REQUIRE(std::isfinite(pf), "pf must be finite");
    PFB_REQUIRE(maxit >= 0, "maxit must be >= 0");
}

// Launch `step` (one iteration: returns nothing, enqueues its kernels) in batches of 8, 16, ... 256 until the device says
// done, never more than `budget` in all.  Returns the launches made.
template <class F>
int64_t run_batched(pfbhip_clean *c, int64_t budget, bool sub, F &&step)
{
    int64_t launched = 0, batch = 8;
    c->read_state();
    while ((sub ? c->hs->sdone : c->hs->done) == 0 && launched < budget) {
        const int64_t n = std::min(batch, budget - launched);
        for (int64_t i = 0; i < n; ++i) step();
        launched += n;
        batch = std::min<int64_t>(batch * 2, 256);
        c->read_state();
    }
    return launched;
}

enum ClarkStage { T_CONV, T_SEARCH, T_COMPACT, T_LDS, T_GRID, T_COUNT };  // stage times of pfbhip_clean_info

}  // namespace

extern "C" {

int pfbhip_clean_create(int64_t nband, int64_t nx, int64_t ny, int64_t nx_psf, int64_t ny_psf, const double *psf_host,
                        const double *psfhat_host, pfbhip_clean **out)
{
    return guarded([&] {
        PFB_REQUIRE(out && psf_host, "NULL argument");
        PFB_REQUIRE(nband >= 1 && nband <= CL_MAXB, "nband must be in [1, %d] (got %lld)", CL_MAXB, (long long)nband);
        PFB_REQUIRE(nx >= 1 && ny >= 1 && nx_psf >= 1 && ny_psf >= 1, "bad geometry");
        PFB_REQUIRE(nx * ny < (int64_t(1) << 31), "image too large for 32-bit active-set indices");
        std::unique_ptr<pfbhip_clean> c(new pfbhip_clean);
        c->nband = nband;
        c->nx = nx;
        c->ny = ny;
        c->nxp = nx_psf;
        c->nyp = ny_psf;
        const size_t np = size_t(nx_psf) * size_t(ny_psf);
        c->psf_peak.resize(size_t(nband));
        for (int64_t b = 0; b < nband; ++b) {
            const double *s = psf_host + size_t(b) * np;
            double m = s[0];
            for (size_t k = 1; k < np; ++k) m = std::max(m, s[k]);
            c->psf_peak[size_t(b)] = m;
        }
        if (psfhat_host) {
            PFB_REQUIRE(nx_psf >= nx && ny_psf >= ny, "the PSF must be at least the image size for the convolution");
            if (pfbhip_psfconv_create(nx, ny, nx_psf, ny_psf, &c->pc) != 0) throw std::runtime_error(pfbhip_last_error());
            const size_t nh = size_t(nx_psf) * size_t(ny_psf / 2 + 1) * 2;
            for (int64_t b = 0; b < nband; ++b)
                if (pfbhip_psfconv_set_psfhat(c->pc, b, psfhat_host + size_t(b) * nh, 1) != 0)
                    throw std::runtime_error(pfbhip_last_error());
            c->stream = psfconv_stream(c->pc);
        } else {
            PFB_HIP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
            c->stream = c->own_stream;
        }
        const size_t cube = size_t(nband) * size_t(nx) * size_t(ny);
        c->psf.alloc(size_t(nband) * np);
        c->dirty.alloc(cube);
        c->resid.alloc(cube);
        c->model.alloc(cube);
        c->wsum.alloc(CL_MAXB);
        c->pv.alloc(CL_MAXBLK);
        c->pi.alloc(CL_MAXBLK);
        c->nminor.alloc(1);
        c->st.alloc(1);
        if (psfhat_host) {
            c->srch.alloc(size_t(nx) * size_t(ny));
            c->mask.alloc(size_t(nx) * size_t(ny));
            c->aset.alloc(cube);
            c->pidx.alloc(size_t(nx) * size_t(ny));
            c->qidx.alloc(size_t(nx) * size_t(ny));
            c->cnt.alloc(CL_MAXBLK);
        }
        synced(c->stream, [&] {
            PFB_HIP(hipMemcpyAsync(c->psf.p, psf_host, size_t(nband) * np * sizeof(double), hipMemcpyHostToDevice, c->stream));
            PFB_HIP(hipHostMalloc((void **)&c->hs, sizeof(CleanHostState), hipHostMallocDefault));
            PFB_HIP(hipEventCreateWithFlags(&c->ev_sync, hipEventDisableTiming));
        });
        *out = c.release();
    });
}

int pfbhip_clean_destroy(pfbhip_clean *c)
{
    return guarded([&] { delete c; });
}

int pfbhip_clean_hogbom(pfbhip_clean *c, const double *dirty_host, double threshold, double gamma, double pf, int64_t maxit,
                        double *model_host, double *residual_host, pfbhip_clean_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(c && dirty_host && model_host, "NULL argument");
        check_params(gamma, pf, maxit);
        for (int64_t b = 0; b < c->nband; ++b)
            PFB_REQUIRE(c->psf_peak[size_t(b)] > 0.0, "the PSF of band %lld has no positive peak", (long long)b);
        const size_t cube = size_t(c->nband) * size_t(c->npix());
        hipStream_t s = c->stream;
        int64_t launched = 0;
        double ms = 0.0;
        synced(s, [&] {
            PFB_HIP(hipMemcpyAsync(c->wsum.p, c->psf_peak.data(), size_t(c->nband) * sizeof(double), hipMemcpyHostToDevice, s));
            PFB_HIP(hipMemcpyAsync(c->resid.p, dirty_host, cube * sizeof(double), hipMemcpyHostToDevice, s));
            PFB_HIP(hipMemsetAsync(c->model.p, 0, cube * sizeof(double), s));
            c->reset_state();
            const CleanParams cp{threshold, gamma, pf, 0.0, maxit, 0};
            PFB_HIP(hipStreamSynchronize(s));
            const auto t0 = std::chrono::steady_clock::now();
            c->image_search(false, false, false);
            c->finish(cp, FIN_HOGBOM, true);
            launched = run_batched(c, maxit, false, [&] {
                c->image_search(true, false, false);
                c->finish(cp, FIN_HOGBOM, false);
            });
            ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            PFB_HIP(hipMemcpyAsync(model_host, c->model.p, cube * sizeof(double), hipMemcpyDeviceToHost, s));
            if (residual_host) PFB_HIP(hipMemcpyAsync(residual_host, c->resid.p, cube * sizeof(double), hipMemcpyDeviceToHost, s));
        });
        if (info) {
            *info = pfbhip_clean_info{};
            info->iters = int32_t(c->hs->k);
            info->status = c->hs->k >= maxit ? 1 : 0;
            info->minor_iters = c->hs->k;
            info->idle_launches = launched - c->hs->k;
            info->rmax = c->hs->rmax;
            info->loop_ms = ms;
        }
    });
}

int pfbhip_clean_clark(pfbhip_clean *c, const double *dirty_host, const double *wsums, const double *mask_host, double threshold,
                       double gamma, double pf, int64_t maxit, double subpf, int64_t submaxit, double *model_host,
                       double *residual_host, pfbhip_clean_info *info)
{
    return guarded([&] {
        PFB_REQUIRE(c && dirty_host && wsums && mask_host && model_host, "NULL argument");
        PFB_REQUIRE(c->pc, "this CLEAN plan was made without psfhat: Hogbom only");
        check_params(gamma, pf, maxit);
        PFB_REQUIRE(subpf > 0.0 && subpf < 1.0, "subpf must be in (0, 1) (got %g)", subpf);
        PFB_REQUIRE(submaxit >= 0, "submaxit must be >= 0");
        bool any = false;
        for (int64_t b = 0; b < c->nband; ++b) {
            PFB_REQUIRE(wsums[b] >= 0.0, "wsums must be non-negative");
            any = any || wsums[b] > 0.0;
        }
        PFB_REQUIRE(any, "wsums are all zero");
        const int64_t npix = c->npix();
        const size_t cube = size_t(c->nband) * size_t(npix);
        hipStream_t s = c->stream;
        double t_ms[T_COUNT] = {}, ms = 0.0;
        int64_t t_calls[T_COUNT] = {}, idle = 0;
        StageTimer tm(s, true);
        synced(s, [&] {
            PFB_HIP(hipMemcpyAsync(c->wsum.p, wsums, size_t(c->nband) * sizeof(double), hipMemcpyHostToDevice, s));
            PFB_HIP(hipMemcpyAsync(c->dirty.p, dirty_host, cube * sizeof(double), hipMemcpyHostToDevice, s));
            PFB_HIP(hipMemcpyAsync(c->mask.p, mask_host, size_t(npix) * sizeof(double), hipMemcpyHostToDevice, s));
            PFB_HIP(hipMemcpyAsync(c->resid.p, c->dirty.p, cube * sizeof(double), hipMemcpyDeviceToDevice, s));
            PFB_HIP(hipMemsetAsync(c->model.p, 0, cube * sizeof(double), s));
            c->reset_state();
            const CleanParams cp{threshold, gamma, pf, subpf, maxit, submaxit};
            const int g = c->grid(npix);
            const int64_t chunk = ceil_div(npix, g);
            const int64_t lds_max = CL_LDS_BYTES / (8 * c->nband);
            allow_dynamic_lds(reinterpret_cast<const void *>(&k_cl_sub_lds), int(CL_LDS_BYTES));
            PFB_HIP(hipStreamSynchronize(s));
            const auto t0 = std::chrono::steady_clock::now();
            bool first = true;
            for (;;) {
                // residual = dirty - conv(model) (skipped before the first sub-minor loop), masked search, stop test, active set
                tm.begin(T_CONV);
                if (!first) {
                    PFB_HIP(hipMemcpyAsync(c->resid.p, c->dirty.p, cube * sizeof(double), hipMemcpyDeviceToDevice, s));
                    for (int64_t b = 0; b < c->nband; ++b)
                        psfconv_apply_async(c->pc, c->model.p + size_t(b) * size_t(npix), b, -1, 0, 0.0, -1.0, 0.0, 1,
                                            c->resid.p + size_t(b) * size_t(npix));
                }
                tm.end();
                tm.begin(T_SEARCH);
                c->image_search(false, true, true);
                c->finish(cp, FIN_MAJOR, first);
                tm.end();
                tm.begin(T_COMPACT);
                hipLaunchKernelGGL(k_cl_count, dim3(g), dim3(CL_THREADS), 0, s, c->st.p, c->srch.p, npix, chunk, c->cnt.p);
                PFB_HIP(hipGetLastError());
                hipLaunchKernelGGL(k_cl_scan, dim3(1), dim3(CL_FIN), 0, s, c->st.p, c->cnt.p, g);
                PFB_HIP(hipGetLastError());
                hipLaunchKernelGGL(k_cl_compact, dim3(g), dim3(CL_THREADS), 0, s, c->st.p, c->srch.p, c->resid.p, int(c->nband),
                                   c->nx, c->ny, chunk, c->cnt.p, c->pidx.p, c->qidx.p, c->aset.p);
                PFB_HIP(hipGetLastError());
                tm.end();
                c->read_state();
                tm.collect(t_ms, t_calls);
                first = false;
                if (c->hs->done) break;
                // sub-minor loop over the active set
                const int64_t A = c->hs->A;
                tm.begin(A <= lds_max ? T_LDS : T_GRID);
                if (A <= lds_max) {
                    hipLaunchKernelGGL(k_cl_sub_lds, dim3(1), dim3(CL_LDS_THREADS), size_t(c->nband * A) * sizeof(double), s, c->st.p,
                                       cp, int(c->nband), c->aset.p, c->pidx.p, c->qidx.p, c->psf.p, c->nxp, c->nyp, c->wsum.p,
                                       c->model.p, c->nx, c->ny, c->nminor.p);
                    PFB_HIP(hipGetLastError());
                } else {
                    const int ga = c->grid(A);
                    c->last_parts = ga;
                    hipLaunchKernelGGL(k_cl_active<false>, dim3(ga), dim3(CL_THREADS), 0, s, c->st.p, int(c->nband), c->aset.p,
                                       c->pidx.p, c->qidx.p, c->psf.p, c->nxp, c->nyp, c->wsum.p, c->pv.p, c->pi.p);
                    PFB_HIP(hipGetLastError());
                    c->finish(cp, FIN_SUB, true);
                    const int64_t before = c->hs->nminor;
                    const int64_t launched = run_batched(c, submaxit, true, [&] {
                        hipLaunchKernelGGL(k_cl_active<true>, dim3(ga), dim3(CL_THREADS), 0, s, c->st.p, int(c->nband), c->aset.p,
                                           c->pidx.p, c->qidx.p, c->psf.p, c->nxp, c->nyp, c->wsum.p, c->pv.p, c->pi.p);
                        PFB_HIP(hipGetLastError());
                        c->finish(cp, FIN_SUB, false);
                    });
                    idle += launched - (c->hs->nminor - before);
                    c->last_parts = g;
                }
                tm.end();
                tm.collect(t_ms, t_calls);
            }
            ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            PFB_HIP(hipMemcpyAsync(model_host, c->model.p, cube * sizeof(double), hipMemcpyDeviceToHost, s));
            if (residual_host) PFB_HIP(hipMemcpyAsync(residual_host, c->resid.p, cube * sizeof(double), hipMemcpyDeviceToHost, s));
        });
        if (info) {
            *info = pfbhip_clean_info{};
            info->iters = int32_t(c->hs->k);
            info->status = c->hs->k >= maxit ? 1 : 0;
            info->minor_iters = c->hs->nminor;
            info->idle_launches = idle;
            info->nsub_lds = t_calls[T_LDS];
            info->nsub_grid = t_calls[T_GRID];
            info->rmax = c->hs->rmax;
            info->loop_ms = ms;
            info->conv_ms = t_ms[T_CONV];
            info->search_ms = t_ms[T_SEARCH];
            info->compact_ms = t_ms[T_COMPACT];
            info->sub_lds_ms = t_ms[T_LDS];
            info->sub_grid_ms = t_ms[T_GRID];
        }
    });
}

}  // extern "C"
