// gridder_wd.hip -- the one-plane w-scheme's scatter / gather (gridder_kernels_wd.hpp) in a translation unit of its own:
// 13 kernel supports x 3 term counts x 3 kernels (scatter, gather, fused Hessian) compile next to gridder.hip, not behind it.
#include "gridder_kernels_wd.hpp"

#include <algorithm>
#include <stdexcept>

#include "common.hpp"
#include "dispatch.hpp"

namespace pfbhip {

// Threads per workgroup: 256 -- one wave per SIMD, three workgroups per CU (see gridder_kernels_wd.hpp; measured on C2, ms per
// apply: scatter 768 x 1: 2.76, 384 x 2: 3.3, 256 x 3: 2.31; gather 768 x 1: 1.90, 384 x 2: 2.33, 256 x 3: 1.64).  Launches of
// fewer work items than three per CU (C1: ~300) cannot fill the chip with 256-thread workgroups: those take one 768-thread
// workgroup per item.
static int scatter_threads_for(uint32_t nwork) { return nwork < 768u ? wd_threads() : 256; }
static int wd_gather_threads_rt(int NJ, uint32_t nwork) { return std::min(nwork < 768u ? 768 : 256, wd_gather_threads(NJ)); }
size_t wd_gather_lds_bytes() { return size_t(RW_LS) * RW_LS * sizeof(double2); }

void wd_launch_coeffs(const WdArgs &wa, int64_t nactive, const double *pw, double2 *cw, hipStream_t st)
{
    const int64_t n = nactive + REC_PAD;
    hipLaunchKernelGGL(k_wd_coeffs, dim3(uint32_t(ceil_div(n, 256))), dim3(256), 0, st, wa, nactive, pw, cw);
    PFB_HIP(hipGetLastError());
}

void wd_launch_plane_values(int K, int64_t nactive, const double2 *cw, const double2 *sval, double2 *pval, hipStream_t st)
{
    if (nactive <= 0) return;
    hipLaunchKernelGGL(k_plane_values_wd, dim3(uint32_t(ceil_div(nactive, 256))), dim3(256), 0, st, K, nactive, cw, sval, pval);
    PFB_HIP(hipGetLastError());
}

void wd_launch_grid(const GroupArgs &ga, const WdArgs &wa, const VisRec *rec, const double2 *pval, double2 *grid, hipStream_t st)
{
    if (ga.a.nwork == 0) return;
    with_W(wa.W, [&](auto w) {
        constexpr int W = decltype(w)::value;
        with_K(wa.K, [&](auto nj) {
            with_BC<W>(wa.bc, [&](auto bc) {
                constexpr int NJ = decltype(nj)::value, BC = decltype(bc)::value;
                allow_dynamic_lds(reinterpret_cast<const void *>(&k_grid_wd<W, NJ, BC>), 160 * 1024);
                const int threads = scatter_threads_for(ga.a.nwork);
                const size_t lds = wd_lds_doubles(W, threads / 64) * sizeof(double);
                hipLaunchKernelGGL((k_grid_wd<W, NJ, BC>), dim3(ga.a.nwork), dim3(threads), lds, st, ga, wa, rec, pval, grid);
            });
        });
    });
    PFB_HIP(hipGetLastError());
}

void wd_launch_degrid(const GroupArgs &ga, const WdArgs &wa, const VisRec *rec, const double2 *grid, double2 *sacc,
                      const double *swgt, double2 *pval_out, hipStream_t st)
{
    if (ga.a.nwork == 0) return;
    with_W(wa.W, [&](auto w) {
        with_K(wa.K, [&](auto nj) {
            constexpr int W = decltype(w)::value, NJ = decltype(nj)::value;
            allow_dynamic_lds(reinterpret_cast<const void *>(&k_degrid_wd<W, NJ>), 160 * 1024);
            hipLaunchKernelGGL((k_degrid_wd<W, NJ>), dim3(ga.a.nwork), dim3(wd_gather_threads_rt(NJ, ga.a.nwork)), wd_gather_lds_bytes(),
                               st, ga, wa, rec, grid, sacc, swgt, pval_out);
        });
    });
    PFB_HIP(hipGetLastError());
}

bool wd_hessian_supported(int W, int bc) { return W >= 4 && W <= 16 && (bc == 2 || bc == 4) && wd_hess_fits(W, bc) && (bc == 4 || W >= 14); }
void wd_launch_hessian(const GroupArgs &ga, const WdArgs &wa, const VisRec *rec, const double *swgt, const double2 *gin, double2 *gout,
                       hipStream_t st)
{
    if (ga.a.nwork == 0) return;
    if (!wd_hessian_supported(wa.W, wa.bc)) throw std::runtime_error("fused Hessian: W + block edge - 1 must be <= 16");
    with_W(wa.W, [&](auto w) {
        constexpr int W = decltype(w)::value;
        if constexpr (W <= 15) {  // (built as supported: BC = 4 up to W = 13, BC = 2 at W = 14, 15)
            constexpr int BC = W >= 14 ? 2 : 4;
            with_K(wa.K, [&](auto nj) {
                constexpr int NJ = decltype(nj)::value;
                allow_dynamic_lds(reinterpret_cast<const void *>(&k_hess_wd<W, NJ, BC>), 160 * 1024);
                hipLaunchKernelGGL((k_hess_wd<W, NJ, BC>), dim3(ga.a.nwork), dim3(256), wd_hess_lds_bytes(W), st, ga, wa, rec, swgt, gin,
                                   gout);
            });
        } else {
            throw std::runtime_error("unsupported kernel support");
        }
    });
    PFB_HIP(hipGetLastError());
}

}  // namespace pfbhip
