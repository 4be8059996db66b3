// devloop.hpp -- the host-side scaffold of the device-resident backward solvers (pd.hip, fb.hip): the PSF-Hessian band
// description, the stream scope, the stopping measure and the resume protocol of a handle.  Host code
// only, apart from k_diff (a pure subtraction): kernels with a multiply-add stay in their .hip file, whose
// floating-point contraction they were built under.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"
#include "devcg.hpp"
#include "pipeline_api.hpp"

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#pragma clang diagnostic ignored "-Wunused-function"

namespace pfbhip {

constexpr int LOOP_MAXB = 16;  // bands held in registers by the one-pass kernels of the solvers

// d = a - b
static __global__ void __launch_bounds__(256) k_diff(const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ d,
                                                     int64_t n)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i < n) d[i] = a[i] - b[i];
}

// _nb_norm_diff / _nb_any_nonzero of the reference: ||x - xp|| / max(||x||^2, 1e-12)^1/2, 1 when x is all zero
inline double rel_change_eps(double num, double den, double nnz) { return nnz > 0.0 ? std::sqrt(num / std::max(den, 1e-12)) : 1.0; }

// The PSF-approximate Hessian of a cube, band by band (an owned copy of the C-ABI description): H_b = scale_b * sum over
// the band's partitions q in [off[b], off[b + 1]) of beam_q PSF_q beam_q, + eta_b.
struct PsfHessBands {
    std::vector<pfbhip_psfconv *> pcs;
    std::vector<int64_t> off, psf_slots, beam_slots;
    std::vector<double> scale, eta;
    int64_t nx = 0, ny = 0;

    PsfHessBands() = default;
    // every plan must be (nx_, ny_); nx_ < 0: band 0's geometry
    PsfHessBands(pfbhip_psfconv *const *pcs_, int64_t nband, const int64_t *nparts, const int64_t *psf_slots_, const int64_t *beam_slots_,
                 const double *scale_, const double *eta_, int64_t nx_ = -1, int64_t ny_ = -1)
        : nx(nx_), ny(ny_)
    {
        PFB_REQUIRE(pcs_ && nparts && psf_slots_ && beam_slots_ && scale_ && eta_ && nband >= 1, "bad band description");
        off.assign(1, 0);
        for (int64_t b = 0; b < nband; ++b) {
            PFB_REQUIRE(pcs_[b] != nullptr, "band %lld has no PSF plan", (long long)b);
            int64_t px, py;
            psfconv_geometry(pcs_[b], &px, &py);
            if (nx < 0) nx = px, ny = py;
            PFB_REQUIRE(px == nx && py == ny, "the PSF plan of band %lld is (%lld, %lld), expected (%lld, %lld)", (long long)b,
                        (long long)px, (long long)py, (long long)nx, (long long)ny);
            PFB_REQUIRE(nparts[b] >= 1, "band %lld has no partitions", (long long)b);
            off.push_back(off.back() + nparts[b]);
        }
        pcs.assign(pcs_, pcs_ + nband);
        scale.assign(scale_, scale_ + nband);
        eta.assign(eta_, eta_ + nband);
        psf_slots.assign(psf_slots_, psf_slots_ + off.back());
        beam_slots.assign(beam_slots_, beam_slots_ + off.back());
    }
    int64_t nband() const { return int64_t(pcs.size()); }
    size_t npix() const { return size_t(nx) * size_t(ny); }
    hipStream_t stream() const { return psfconv_stream(pcs[0]); }  // the first plan's: where a solve enqueues everything

    // Enqueues out (+)= (mul / div) H_b in for band b, one apply per partition, eta with the first; the first apply
    // accumulates into out only if `accumulate_first`.  The plan is handed mul * scale_b / div and mul * eta_b / div (so
    // -1, gamma gives the -scale_b / gamma of the primal-dual gradient to the bit).  clk brackets every apply as `stage`.
    void apply(int64_t b, const double *in, double *out, double mul, double div, bool accumulate_first, StageTimer *clk = nullptr,
               int stage = 0) const
    {
        const size_t ub = size_t(b);
        for (int64_t q = off[ub]; q < off[ub + 1]; ++q) {
            const bool first = q == off[ub];
            if (clk) clk->begin(stage);
            psfconv_apply_async(pcs[ub], in, psf_slots[size_t(q)], beam_slots[size_t(q)], 0, 0.0, mul * scale[ub] / div,
                                first ? mul * eta[ub] / div : 0.0, !first || accumulate_first, out);
            if (clk) clk->end();
        }
    }
};

// Swaps Psi's (if any) and the plans' streams to the solve's stream and restores them, in reverse order, on exit.  The
// first plan owns `st`; a plan that serves several bands is swapped once.
struct StreamScope {
    pfbhip_psi *psi;
    hipStream_t psi_prev = nullptr;
    std::vector<std::pair<pfbhip_psfconv *, hipStream_t>> plans;
    StreamScope(pfbhip_psi *psi_or_null, const PsfHessBands &bands, hipStream_t st) : psi(psi_or_null)
    {
        if (psi) psi_prev = psi_swap_stream(psi, st);
        for (pfbhip_psfconv *pc : bands.pcs) {
            bool seen = pc == bands.pcs[0];
            for (auto &pr : plans) seen = seen || pr.first == pc;
            if (!seen) plans.emplace_back(pc, psfconv_swap_stream(pc, st));
        }
    }
    StreamScope(const StreamScope &) = delete;
    StreamScope &operator=(const StreamScope &) = delete;
    ~StreamScope()
    {
        if (psi) (void)psi_swap_stream(psi, psi_prev);
        for (auto it = plans.rbegin(); it != plans.rend(); ++it) {
            try {
                (void)psfconv_swap_stream(it->first, it->second);
            } catch (...) {
            }
        }
    }
};

// The resume protocol of a solver handle.  An iteration is completed lazily: after iteration k ran, `pending` is set and
// the rotation xp <- x (whatever else the solver rotates) and k += 1 happen at the start of the next one, so a run that
// resumes after a convergence event continues as the reference's loop does when on_converge returns False.
constexpr int LOOP_NSTAGES = 5;
static_assert(LOOP_NSTAGES == PFBHIP_PD_NSTAGES && LOOP_NSTAGES == PFBHIP_FB_NSTAGES, "stage arrays of the info structs");
struct Resume {
    int k = 0;             // index of the next iteration (of the last one while `pending`)
    bool pending = false;  // iteration k ran and is not completed yet
    bool has_weight = false;
    double eps = 1.0, loop_ms = 0.0;
    double stage_ms[LOOP_NSTAGES] = {};
    int64_t stage_calls[LOOP_NSTAGES] = {};

    // what a run needs before its first iteration
    void require_runnable(int maxit) const
    {
        PFB_REQUIRE(k + (pending ? 1 : 0) < maxit, "iteration %d is past maxit %d", k + (pending ? 1 : 0), maxit);
        PFB_REQUIRE(has_weight, "no weight: created with weight_host == NULL and none set since");
    }
    // completes the previous iteration, if any: xp <- x by rotation; true when the caller has more to rotate
    bool complete(double *&x, double *&xp)
    {
        if (!pending) return false;
        std::swap(x, xp);
        ++k;
        pending = false;
        return true;
    }
    // the iterate of the last iteration run (before the first: the start value)
    const double *iterate(const double *x, const double *xp) const { return pending ? x : xp; }
    // w_dev <- src (n doubles, from the host or the device), synchronised
    void set_weight(double *w_dev, const double *src, size_t n, hipMemcpyKind kind, hipStream_t st)
    {
        synced(st, [&] { PFB_HIP(hipMemcpyAsync(w_dev, src, n * sizeof(double), kind, st)); });
        has_weight = true;
    }
    void stages_to(double *ms, int64_t *calls) const
    {
        std::copy(stage_ms, stage_ms + LOOP_NSTAGES, ms);
        std::copy(stage_calls, stage_calls + LOOP_NSTAGES, calls);
    }
};

}  // namespace pfbhip

#pragma clang diagnostic pop
