// beam.hip -- primary beams on the device: the regrid onto the image grid and the azimuthal average.
//
// Mirrors two scipy call sites of pfb-imaging:
//   eval_beam (utils/beam.py:75-89): RegularGridInterpolator((l_in, m_in), beam, method="linear", bounds_error=False,
//     fill_value=1.0), with the reference's short-circuit for a beam that is identically 1.0;
//   the BEAM product of utils/stokes2vis_msv4.py:399-409: the mean of ndimage.rotate(beam0, angle, reshape=False,
//     mode="nearest") over an angle table, restated as edge pad by 12 -> cubic B-spline prefilter -> one pass that evaluates
//     the 4x4 B-spline at every angle's rotated coordinate.
// Everything is f64; no product is contracted with a sum (the Makefile's -ffp-contract=off), so the regrid rounds as its
// numpy restatement (tests/_beam_ref.py) does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"

namespace pfbhip {

constexpr int BM_THREADS = 256;
constexpr int BM_WORKGROUPS = 8192;  // of the separable regrid: 32 per CU, each writes many rows

// ---- regrid ------------------------------------------------------------------------------------------------------

// scipy's find_indices on strictly ascending nodes (n >= 2): i with node[i] <= x < node[i + 1], clipped to [0, n - 2], and
// t = (x - node[i]) / (node[i + 1] - node[i]).  Returns true when x lies outside [node[0], node[n - 1]] (the last node is
// inside).  A NaN coordinate is not outside and gives a NaN weight, as in scipy.
__device__ __forceinline__ bool bm_locate(const double *__restrict__ node, int n, double x, int &i, double &t)
{
    int lo = 0, hi = n - 1;  // node[lo] <= x or lo == 0; node[hi] > x or hi == n - 1
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (node[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    i = lo;
    const double a = node[lo];
    t = (x - a) / (node[lo + 1] - a);
    return x < node[0] || x > node[n - 1];
}

// four loads, three lerps; (1 - t) a + t b returns a at t = 0 and b at t = 1 exactly
__device__ __forceinline__ double bm_bilinear(const double *__restrict__ plane, int nm, int i, double tx, int j, double ty)
{
    const double *r0 = plane + size_t(i) * size_t(nm) + size_t(j), *r1 = r0 + nm;
    const double lo = (1.0 - ty) * r0[0] + ty * r0[1];
    const double hi = (1.0 - ty) * r1[0] + ty * r1[1];
    return (1.0 - tx) * lo + tx * hi;
}

// notones[c] = any(beam[c] != 1.0) (NaN counts), the reference's (beam_image == 1.0).all() negated; notones was cleared on
// the stream.  Every thread that finds such a value stores the same 1.
__global__ void __launch_bounds__(BM_THREADS) k_beam_notones(const double *__restrict__ beam, int64_t plane, int32_t *__restrict__ notones)
{
    const double *b = beam + size_t(blockIdx.y) * size_t(plane);
    bool any = false;
    for (int64_t p = int64_t(blockIdx.x) * BM_THREADS + threadIdx.x; p < plane; p += int64_t(gridDim.x) * BM_THREADS) any |= b[p] != 1.0;
    if (any) notones[blockIdx.y] = 1;
}

// index (-1: outside) and weight of every separable output coordinate: nx + ny searches in total
__global__ void __launch_bounds__(BM_THREADS) k_beam_axes(const double *__restrict__ l_in, int nl, const double *__restrict__ m_in, int nm,
                                                          const double *__restrict__ l_out, int64_t nx, const double *__restrict__ m_out,
                                                          int64_t ny, int32_t *__restrict__ ix, double *__restrict__ tx,
                                                          int32_t *__restrict__ jy, double *__restrict__ ty)
{
    const int64_t e = int64_t(blockIdx.x) * BM_THREADS + threadIdx.x;
    if (e >= nx + ny) return;
    int i;
    double t;
    if (e < nx) {
        const bool out = bm_locate(l_in, nl, l_out[e], i, t);
        ix[e] = out ? -1 : i;
        tx[e] = t;
    } else {
        const bool out = bm_locate(m_in, nm, m_out[e - nx], i, t);
        jy[e - nx] = out ? -1 : i;
        ty[e - nx] = t;
    }
}

// One output row (c, x) per blockIdx.y step, two adjacent y per thread.  The pair starts on an even element of `out`, so
// that it leaves in one 16-byte store: when ny is odd every other row begins one element late.
template <bool GENERAL>
__global__ void __launch_bounds__(BM_THREADS) k_beam_regrid(const double *__restrict__ beam, int nl, int nm, const double *__restrict__ l_in,
                                                            const double *__restrict__ m_in, const double *__restrict__ ll,
                                                            const double *__restrict__ mm, const int32_t *__restrict__ ix,
                                                            const double *__restrict__ tx, const int32_t *__restrict__ jy,
                                                            const double *__restrict__ ty, const int32_t *__restrict__ notones,
                                                            int64_t nrows, int64_t nx, int64_t ny, double *__restrict__ out)
{
    const int64_t k = int64_t(blockIdx.x) * BM_THREADS + threadIdx.x;
    // The separable form keeps its two y entries over the rows of the walk: they change only with the parity of the row's
    // first element, which an even row stride (the host's choice) leaves alone.
    int64_t held = -1;
    int jh[2] = {-1, -1};
    double wh[2] = {0.0, 0.0};
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const int64_t c = row / nx, x = row - c * nx, base = row * ny;
        const int64_t y0 = 2 * k - (base & 1);
        if (y0 >= ny) continue;
        if (!GENERAL && held != (base & 1)) {
            held = base & 1;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int64_t y = y0 + s;
                const bool in = y >= 0 && y < ny;
                jh[s] = in ? jy[y] : -1;
                wh[s] = in ? ty[y] : 0.0;
            }
        }
        const double *plane = beam + size_t(c) * size_t(nl) * size_t(nm);
        const bool ones = notones[c] == 0;
        double v[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int64_t y = y0 + s;
            v[s] = 1.0;
            if (y < 0 || y >= ny || ones) continue;
            int i, j;
            double wx, wy;
            bool outside;
            if (GENERAL) {
                const size_t o = size_t(x) * size_t(ny) + size_t(y);
                outside = bm_locate(l_in, nl, ll[o], i, wx);
                outside |= bm_locate(m_in, nm, mm[o], j, wy);
            } else {
                i = ix[x], j = jh[s], wx = tx[x], wy = wh[s];
                outside = i < 0 || j < 0;
            }
            if (!outside) v[s] = bm_bilinear(plane, nm, i, wx, j, wy);
        }
        if (y0 >= 0 && y0 + 1 < ny)
            *reinterpret_cast<double2 *>(out + base + y0) = make_double2(v[0], v[1]);
        else if (y0 >= 0)
            out[base + y0] = v[0];
        else
            out[base + y0 + 1] = v[1];  // (y0 == -1: ny >= 1 makes y = 0 valid)
    }
}

// ---- cubic B-spline prefilter --------------------------------------------------------------------------------------

constexpr int SP_PAD = 12;        // scipy's _prepad_for_spline_filter for mode "nearest"
constexpr int SP_SEG = 64;        // samples of a line a workgroup finishes
constexpr int SP_WARM = 32;       // samples either side that only warm the recursions up: |z|^32 = 5e-19
constexpr int SP_T = SP_SEG + 2 * SP_WARM;
constexpr int SP_LINES = 32;      // lines per workgroup
constexpr int SP_THREADS = 128;
constexpr int SP_HORIZON = 48;    // terms of the causal initialisation sum: |z|^48 = 3.5e-28
constexpr double SP_POLE = -0.26794919243112270647;  // sqrt(3) - 2

// One axis of spline_filter(mode="nearest") (scipy's reflect initialisation) on an array that is the edge-padded source:
// dst (N0, N1) = filter_AXIS(gain * src[clamp(i0 - pad), clamp(i1 - pad)]).  pad = 12 reads the beam itself, pad = 0 an
// array already padded.  A workgroup takes SP_LINES lines x one segment through an LDS tile, so global reads and writes
// are coalesced on either axis; a segment that does not start (end) the line warms its causal (anticausal) recursion
// up over SP_WARM samples instead of scanning the whole line.  blockIdx = (line tile, segment, plane).
template <int AXIS>
__global__ void __launch_bounds__(SP_THREADS) k_spline_axis(const double *__restrict__ src, int64_t s0, int64_t s1, int pad, int64_t N0,
                                                            int64_t N1, double zn, double *__restrict__ dst)
{
    __shared__ double tile[SP_LINES][SP_T + 1];
    const int64_t n = AXIS == 0 ? N0 : N1, nlines = AXIS == 0 ? N1 : N0;
    const int64_t line0 = int64_t(blockIdx.x) * SP_LINES;
    const int64_t s = int64_t(blockIdx.y) * SP_SEG, e = std::min<int64_t>(s + SP_SEG, n);
    const int64_t a = std::max<int64_t>(s - SP_WARM, 0), b = std::min<int64_t>(e + SP_WARM, n);
    const int len = int(b - a);
    const double *sp = src + size_t(blockIdx.z) * size_t(s0) * size_t(s1);
    double *dp = dst + size_t(blockIdx.z) * size_t(N0) * size_t(N1);
    const double z = SP_POLE, gain = (1.0 - z) * (1.0 - 1.0 / z);
    auto load = [&](int64_t line, int64_t smp) {
        const int64_t i0 = (AXIS == 0 ? smp : line) - pad, i1 = (AXIS == 0 ? line : smp) - pad;
        const int64_t c0 = std::min<int64_t>(std::max<int64_t>(i0, 0), s0 - 1), c1 = std::min<int64_t>(std::max<int64_t>(i1, 0), s1 - 1);
        return sp[size_t(c0) * size_t(s1) + size_t(c1)] * gain;
    };
    // the index that is contiguous in memory goes to adjacent threads
    for (int q = threadIdx.x; q < SP_LINES * SP_T; q += SP_THREADS) {
        const int L = AXIS == 0 ? q % SP_LINES : q / SP_T, S = AXIS == 0 ? q / SP_LINES : q % SP_T;
        if (S < len && line0 + L < nlines) tile[L][S] = load(line0 + L, a + S);
    }
    __syncthreads();
    if (threadIdx.x < SP_LINES && line0 + threadIdx.x < nlines) {
        double *c = tile[threadIdx.x];
        if (a == 0) {  // the line starts here: c[0] += z / (1 - z^2n) sum_i z^i (c[i] + z^n c[n - 1 - i])
            const int h = int(std::min<int64_t>(n, SP_HORIZON));  // (h <= len: the first tile holds min(n, 96) samples)
            double acc = 0.0, zi = 1.0;
            for (int i = 0; i < h; ++i) {
                const int64_t far = n - 1 - i;  // beyond the tile only when n > 96, where z^n < 1e-54
                acc += zi * (c[i] + (far < len ? zn * c[far] : 0.0));
                zi *= z;
            }
            c[0] += z / (1.0 - zn * zn) * acc;
        }
        for (int i = 1; i < len; ++i) c[i] += z * c[i - 1];
        c[len - 1] *= z / (z - 1.0);  // exact at the end of the line, a start that decays elsewhere
        for (int i = len - 2; i >= 0; --i) c[i] = z * (c[i + 1] - c[i]);
    }
    __syncthreads();
    const int first = int(s - a), count = int(e - s);
    for (int q = threadIdx.x; q < SP_LINES * SP_SEG; q += SP_THREADS) {
        const int L = AXIS == 0 ? q % SP_LINES : q / SP_SEG, S = AXIS == 0 ? q / SP_LINES : q % SP_SEG;
        if (S >= count || line0 + L >= nlines) continue;
        const int64_t i0 = AXIS == 0 ? s + S : line0 + L, i1 = AXIS == 0 ? line0 + L : s + S;
        dp[size_t(i0) * size_t(N1) + size_t(i1)] = tile[L][first + S];
    }
}

// ---- rotation mean -------------------------------------------------------------------------------------------------

constexpr int RM_TX = 32, RM_TY = 8;  // output tile of a workgroup (columns x rows)
constexpr int RM_TABLE = 64;          // angles staged in LDS at a time

// scipy's get_spline_interpolation_weights for order 3 at fractional part y
__device__ __forceinline__ void rm_weights(double y, double w[4])
{
    const double z = 1.0 - y;
    w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = z * z * z / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}

// out[c, i, j] = mean_a spline(coef[c]; rotated (i, j)).  Samples outside the padded array follow scipy's rule for mode
// "nearest" after the prepad: the coordinate is NOT clamped (weights from its own fractional part, support from
// floor(x) - 1), each of the four support indices is clamped to [0, N - 1].
__global__ void __launch_bounds__(RM_TX *RM_TY) k_beam_rotmean(const double *__restrict__ coef, int64_t n0, int64_t n1,
                                                               const double2 *__restrict__ cs, int na, double *__restrict__ out)
{
    __shared__ double2 tab[RM_TABLE];
    const int64_t N0 = n0 + 2 * SP_PAD, N1 = n1 + 2 * SP_PAD;
    const int tid = threadIdx.y * RM_TX + threadIdx.x;
    const int64_t i = int64_t(blockIdx.y) * RM_TY + threadIdx.y, j = int64_t(blockIdx.x) * RM_TX + threadIdx.x;
    const bool valid = i < n0 && j < n1;
    const double *cp = coef + size_t(blockIdx.z) * size_t(N0) * size_t(N1);
    const double c0 = double(n0 - 1) / 2.0, c1 = double(n1 - 1) / 2.0;
    const double di = double(i) - c0, dj = double(j) - c1;
    double acc = 0.0;
    for (int a0 = 0; a0 < na; a0 += RM_TABLE) {
        const int m = std::min(na - a0, RM_TABLE);
        __syncthreads();
        if (tid < m) tab[tid] = cs[a0 + tid];
        __syncthreads();
        if (!valid) continue;
        for (int a = 0; a < m; ++a) {
            const double c = tab[a].x, s = tab[a].y;
            const double ii = c * di + s * dj + c0 + double(SP_PAD);
            const double jj = -s * di + c * dj + c1 + double(SP_PAD);
            const double fi = floor(ii), fj = floor(jj);
            double wi[4], wj[4];
            rm_weights(ii - fi, wi);
            rm_weights(jj - fj, wj);
            const int64_t si = int64_t(fi) - 1, sj = int64_t(fj) - 1;
            size_t col[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) col[q] = size_t(std::min<int64_t>(std::max<int64_t>(sj + q, 0), N1 - 1));
            double val = 0.0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const double *r = cp + size_t(std::min<int64_t>(std::max<int64_t>(si + p, 0), N0 - 1)) * size_t(N1);
                double rowsum = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) rowsum += wj[q] * r[col[q]];
                val += wi[p] * rowsum;
            }
            acc += val;
        }
    }
    if (valid) out[(size_t(blockIdx.z) * size_t(n0) + size_t(i)) * size_t(n1) + size_t(j)] = acc / double(na);
}

// cos and sin of an angle in degrees, exact at the multiples of 90 (as scipy.special.cosdg / sindg are)
static double2 cos_sin_deg(double deg)
{
    double r = std::fmod(deg, 360.0);
    if (r < 0.0) r += 360.0;
    if (r == 0.0 || r == 360.0) return make_double2(1.0, 0.0);
    if (r == 90.0) return make_double2(0.0, 1.0);
    if (r == 180.0) return make_double2(-1.0, 0.0);
    if (r == 270.0) return make_double2(0.0, -1.0);
    const double rad = r * (3.14159265358979323846 / 180.0);
    return make_double2(std::cos(rad), std::sin(rad));
}

static void require_ascending(const double *node, int64_t n, const char *name)
{
    for (int64_t i = 0; i < n; ++i) PFB_REQUIRE(std::isfinite(node[i]), "%s[%lld] is not finite", name, (long long)i);
    for (int64_t i = 1; i < n; ++i)
        PFB_REQUIRE(node[i] > node[i - 1], "The points in dimension %s must be strictly ascending (%s[%lld] = %.17g, %s[%lld] = %.17g)", name,
                    name, (long long)(i - 1), node[i - 1], name, (long long)i, node[i]);
}

}  // namespace pfbhip

using namespace pfbhip;

extern "C" {

int pfbhip_beam_regrid(const double *beam_host, int32_t ncorr, int64_t nl, int64_t nm, const double *l_in, const double *m_in,
                       const double *l_out, const double *m_out, int general, int64_t nx, int64_t ny, double *out_host,
                       double *device_ms)
{
    return guarded([&] {
        PFB_REQUIRE(beam_host && l_in && m_in && l_out && m_out && out_host, "NULL argument");
        PFB_REQUIRE(ncorr >= 1 && ncorr <= 65535 && nx >= 1 && ny >= 1, "bad sizes");
        PFB_REQUIRE(nl >= 2 && nm >= 2 && nl < (int64_t(1) << 30) && nm < (int64_t(1) << 30), "the beam needs at least two nodes per axis");
        PFB_REQUIRE(nx + ny < (int64_t(1) << 31) && ny / 2 + 1 <= int64_t(BM_THREADS) * 0x7fffffff, "output too large");
        require_ascending(l_in, nl, "l_in");
        require_ascending(m_in, nm, "m_in");
        const hipStream_t st = hipStreamPerThread;
        const size_t plane = size_t(nl) * size_t(nm), nout = size_t(nx) * size_t(ny);
        const size_t ncoord_l = general ? nout : size_t(nx), ncoord_m = general ? nout : size_t(ny);
        DevBuf<double> beam{size_t(ncorr) * plane}, dl{size_t(nl)}, dm{size_t(nm)}, lo{ncoord_l}, mo{ncoord_m}, out{size_t(ncorr) * nout};
        DevBuf<double> tx, ty;
        DevBuf<int32_t> ix, jy, notones{size_t(ncorr)};
        if (!general) tx.alloc(size_t(nx)), ty.alloc(size_t(ny)), ix.alloc(size_t(nx)), jy.alloc(size_t(ny));
        EventTimer timer(device_ms != nullptr);
        synced(st, [&] {
            PFB_HIP(hipMemcpyAsync(beam.p, beam_host, beam.bytes(), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(dl.p, l_in, dl.bytes(), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(dm.p, m_in, dm.bytes(), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(lo.p, l_out, lo.bytes(), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(mo.p, m_out, mo.bytes(), hipMemcpyHostToDevice, st));
            timer.start(st);
            PFB_HIP(hipMemsetAsync(notones.p, 0, notones.bytes(), st));
            const uint32_t nb = uint32_t(std::min<int64_t>(ceil_div(int64_t(plane), BM_THREADS), 256));
            hipLaunchKernelGGL(k_beam_notones, dim3(nb, uint32_t(ncorr)), dim3(BM_THREADS), 0, st, beam.p, int64_t(plane), notones.p);
            const int64_t nrows = int64_t(ncorr) * nx;
            // Separable form: about BM_WORKGROUPS workgroups walk the rows with an even stride (k_beam_regrid keeps its y
            // entries then); measured at 8192^2, 0.151 ms against 0.205 ms with a workgroup per row segment.  The general form
            // spends its time in the searches and wants the workgroups: 0.98 ms per row segment against 1.15 ms walking.
            const int64_t gx = ceil_div(ny / 2 + 1, BM_THREADS);
            int64_t gy = std::min<int64_t>(nrows, general ? 65534 : std::max<int64_t>(BM_WORKGROUPS / gx, 1));
            if (gy > 1) gy &= ~int64_t(1);
            const dim3 grid{uint32_t(gx), uint32_t(gy)};
            if (general) {
                hipLaunchKernelGGL(k_beam_regrid<true>, grid, dim3(BM_THREADS), 0, st, beam.p, int(nl), int(nm), dl.p, dm.p, lo.p, mo.p,
                                   nullptr, nullptr, nullptr, nullptr, notones.p, nrows, nx, ny, out.p);
            } else {
                hipLaunchKernelGGL(k_beam_axes, dim3(uint32_t(ceil_div(nx + ny, BM_THREADS))), dim3(BM_THREADS), 0, st, dl.p, int(nl), dm.p,
                                   int(nm), lo.p, nx, mo.p, ny, ix.p, tx.p, jy.p, ty.p);
                hipLaunchKernelGGL(k_beam_regrid<false>, grid, dim3(BM_THREADS), 0, st, beam.p, int(nl), int(nm), dl.p, dm.p, nullptr,
                                   nullptr, ix.p, tx.p, jy.p, ty.p, notones.p, nrows, nx, ny, out.p);
            }
            PFB_HIP(hipGetLastError());
            timer.stop(st);
            PFB_HIP(hipMemcpyAsync(out_host, out.p, out.bytes(), hipMemcpyDeviceToHost, st));
        });
        if (device_ms) *device_ms = timer.ms();
    });
}

int pfbhip_beam_rotate_mean(const double *beam0_host, int32_t ncorr, int64_t n0, int64_t n1, const double *angles_deg, int32_t nangles,
                            double *out_host, double *device_ms)
{
    return guarded([&] {
        PFB_REQUIRE(beam0_host && angles_deg && out_host, "NULL argument");
        PFB_REQUIRE(ncorr >= 1 && ncorr <= 65535 && n0 >= 1 && n1 >= 1 && nangles >= 1, "bad sizes");
        PFB_REQUIRE(n0 < (int64_t(1) << 18) && n1 < (int64_t(1) << 18), "beam too large");
        std::vector<double2> table(static_cast<size_t>(nangles));
        for (int32_t a = 0; a < nangles; ++a) {
            PFB_REQUIRE(std::isfinite(angles_deg[a]), "angles[%d] is not finite", int(a));
            table[size_t(a)] = cos_sin_deg(angles_deg[a]);
        }
        const int64_t N0 = n0 + 2 * SP_PAD, N1 = n1 + 2 * SP_PAD;
        const hipStream_t st = hipStreamPerThread;
        const size_t nin = size_t(ncorr) * size_t(n0) * size_t(n1), npad = size_t(ncorr) * size_t(N0) * size_t(N1);
        DevBuf<double> in{nin}, half{npad}, coef{npad}, out{nin};
        DevBuf<double2> cs{size_t(nangles)};
        EventTimer timer(device_ms != nullptr);
        synced(st, [&] {
            PFB_HIP(hipMemcpyAsync(in.p, beam0_host, in.bytes(), hipMemcpyHostToDevice, st));
            PFB_HIP(hipMemcpyAsync(cs.p, table.data(), cs.bytes(), hipMemcpyHostToDevice, st));
            timer.start(st);
            // scipy's spline_filter runs axis 0 first
            hipLaunchKernelGGL(k_spline_axis<0>, dim3(uint32_t(ceil_div(N1, SP_LINES)), uint32_t(ceil_div(N0, SP_SEG)), uint32_t(ncorr)),
                               dim3(SP_THREADS), 0, st, in.p, n0, n1, SP_PAD, N0, N1, std::pow(SP_POLE, double(N0)), half.p);
            hipLaunchKernelGGL(k_spline_axis<1>, dim3(uint32_t(ceil_div(N0, SP_LINES)), uint32_t(ceil_div(N1, SP_SEG)), uint32_t(ncorr)),
                               dim3(SP_THREADS), 0, st, half.p, N0, N1, 0, N0, N1, std::pow(SP_POLE, double(N1)), coef.p);
            hipLaunchKernelGGL(k_beam_rotmean, dim3(uint32_t(ceil_div(n1, RM_TX)), uint32_t(ceil_div(n0, RM_TY)), uint32_t(ncorr)),
                               dim3(RM_TX, RM_TY), 0, st, coef.p, n0, n1, cs.p, int(nangles), out.p);
            PFB_HIP(hipGetLastError());
            timer.stop(st);
            PFB_HIP(hipMemcpyAsync(out_host, out.p, out.bytes(), hipMemcpyDeviceToHost, st));
        });
        if (device_ms) *device_ms = timer.ms();
    });
}

}  // extern "C"
