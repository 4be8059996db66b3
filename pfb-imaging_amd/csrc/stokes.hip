// stokes.hip -- Stokes visibilities and weights from raw correlations, with the Jones correction: weight_data on the device.
//
// Mirrors weight_data of pfb-imaging (src/pfb_imaging/utils/weighting.py:274-468).  For an unflagged
// sample of baseline (p, q) in time bin t, with V = [[v00, v01], [v10, v11]], weights w and the coherency-from-Stokes
// matrix T of the feed type:
//     X   = Jp^-1 V Jq^-H                         (adjugates over the determinants; plain quotients for a diagonal Jones)
//     s_k = sum_c Tinv[k][c] vec(X)[c]            Tinv = T^H / 2
//     W_k = sum_c w_c |A_ck|^2                    A = (Jp (x) conj(Jq)) T, the diagonal of A^H diag(w) A
// A sample with any correlation flagged, and every row that no time bin covers, is written as zero.  Two-correlation data is
// widened to (v0, 0, 0, v1) with weights (w0, 1, 1, w1) (weighting.py:257-266).
//
// One pass, one sample per lane, adjacent lanes on adjacent channels of a row: the Jones terms (contiguous in channel for a
// fixed time and antenna) and every output coalesce; a sample's correlations leave memory in 16-byte loads and its flags as
// one word.  All arithmetic is f64 and nothing is contracted (the Makefile's -ffp-contract=off), so the kernel rounds as
// tests/_stokes_ref.py does up to the complex quotient.  The _sp entries keep single precision across PCIe only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "abi_scope.hpp"
#include "common.hpp"

namespace pfbhip {

namespace {

constexpr int SK_THREADS = 256;
constexpr int SK_MAX_WORKGROUPS = 2048;  // 8 per CU; the rest of the samples by grid stride

// what the kernel needs of T for the selected products, by output slot k (ascending I, Q, U, V)
struct StokesTable {
    double2 tinv[4][4];  // [k][c]: Tinv[product k][c]
    double2 t[4][4];     // [c][k]: T[c][product k]
    int32_t ns;
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// a conj(b)
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double cabs2(double2 a) { return a.x * a.x + a.y * a.y; }
// a / b as a conj(b) / |b|^2: a zero b gives what IEEE division gives
__device__ __forceinline__ double2 cdiv(double2 a, double2 b, double b2)
{
    const double2 n = cmulc(a, b);
    return make_double2(n.x / b2, n.y / b2);
}

// the NC correlations of sample e, widened to four; 16 bytes per load where a sample has them
template <int NC>
__device__ __forceinline__ void load_corr(const double2 *__restrict__ data, int64_t e, double2 v[4])
{
    const double2 *p = data + size_t(e) * NC;
    const double2 zero = make_double2(0.0, 0.0);
    if (NC == 4)
        v[0] = p[0], v[1] = p[1], v[2] = p[2], v[3] = p[3];
    else
        v[0] = p[0], v[1] = zero, v[2] = zero, v[3] = p[1];
}
template <int NC>
__device__ __forceinline__ void load_corr(const float2 *__restrict__ data, int64_t e, double2 v[4])
{
    const float4 *p = reinterpret_cast<const float4 *>(data + size_t(e) * NC);
    const double2 zero = make_double2(0.0, 0.0);
    const float4 a = p[0];
    if (NC == 4) {
        const float4 b = p[1];
        v[0] = make_double2(a.x, a.y), v[1] = make_double2(a.z, a.w), v[2] = make_double2(b.x, b.y), v[3] = make_double2(b.z, b.w);
    } else {
        v[0] = make_double2(a.x, a.y), v[1] = zero, v[2] = zero, v[3] = make_double2(a.z, a.w);
    }
}
template <int NC>
__device__ __forceinline__ void load_wgt(const double *__restrict__ weight, int64_t e, double w[4])
{
    const double2 *p = reinterpret_cast<const double2 *>(weight + size_t(e) * NC);
    const double2 a = p[0];
    if (NC == 4) {
        const double2 b = p[1];
        w[0] = a.x, w[1] = a.y, w[2] = b.x, w[3] = b.y;
    } else {
        w[0] = a.x, w[1] = 1.0, w[2] = 1.0, w[3] = a.y;
    }
}
template <int NC>
__device__ __forceinline__ void load_wgt(const float *__restrict__ weight, int64_t e, double w[4])
{
    if (NC == 4) {
        const float4 a = *reinterpret_cast<const float4 *>(weight + size_t(e) * 4);
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
    } else {
        const float2 a = *reinterpret_cast<const float2 *>(weight + size_t(e) * 2);
        w[0] = a.x, w[1] = 1.0, w[2] = 1.0, w[3] = a.y;
    }
}
template <int NC>
__device__ __forceinline__ bool any_flag(const uint8_t *__restrict__ flag, int64_t e)
{
    if (NC == 4) return *reinterpret_cast<const uint32_t *>(flag + size_t(e) * 4) != 0u;
    return *reinterpret_cast<const uint16_t *>(flag + size_t(e) * 2) != 0u;
}

__device__ __forceinline__ void store_c(double2 *p, double2 s) { *p = s; }
__device__ __forceinline__ void store_c(float2 *p, double2 s) { *p = make_float2(float(s.x), float(s.y)); }

template <typename R>
struct Cplx;
template <>
struct Cplx<double> {
    using type = double2;
};
template <>
struct Cplx<float> {
    using type = float2;
};

// jones: (ntime, nant, nchan, 2) complex for the diagonal form, (ntime, nant, nchan, 2, 2) for the full one, direction 0
// only.  Output element (e, k) of vis / wgt sits at e * out_se + k * out_sk: (nrow, nchan, ns) or (ns, nrow, nchan).
// mask (may be NULL) = ~flag.any(-1), whatever the bins say.
template <typename R, int NC, bool FULL>
__global__ void __launch_bounds__(SK_THREADS) k_weight_data(const typename Cplx<R>::type *__restrict__ data, const R *__restrict__ weight,
                                                            const uint8_t *__restrict__ flag, const double2 *__restrict__ jones,
                                                            const int32_t *__restrict__ row2bin, const int32_t *__restrict__ ant1,
                                                            const int32_t *__restrict__ ant2, int64_t nsamp, int64_t nchan, int64_t nant,
                                                            StokesTable tab, int64_t out_se, int64_t out_sk,
                                                            typename Cplx<R>::type *__restrict__ vis, R *__restrict__ wgt,
                                                            uint8_t *__restrict__ mask)
{
    constexpr int NJ = FULL ? 4 : 2;  // complex values of one Jones term
    const int64_t step = int64_t(gridDim.x) * SK_THREADS;
    for (int64_t e = int64_t(blockIdx.x) * SK_THREADS + threadIdx.x; e < nsamp; e += step) {
        const int64_t row = e / nchan, chan = e - row * nchan;
        const int32_t bin = row2bin[row];
        const bool flagged = any_flag<NC>(flag, e);
        if (mask) mask[e] = flagged ? 0 : 1;
        double2 s[4];
        double ws[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = make_double2(0.0, 0.0), ws[k] = 0.0;
        if (bin >= 0 && !flagged) {
            const int64_t p = ant1[row], q = ant2[row];
            const double2 *jp = jones + ((size_t(bin) * size_t(nant) + size_t(p)) * size_t(nchan) + size_t(chan)) * NJ;
            const double2 *jq = jones + ((size_t(bin) * size_t(nant) + size_t(q)) * size_t(nchan) + size_t(chan)) * NJ;
            double2 v[4], x[4];
            double w[4];
            load_corr<NC>(data, e, v);
            load_wgt<NC>(weight, e, w);
            if (!FULL) {
                const double2 p0 = jp[0], p1 = jp[1], q0 = jq[0], q1 = jq[1];
                // g[c] = Jp[i][i] conj(Jq[j][j]) for c = (i, j): the diagonal of Jp (x) conj(Jq)
                const double2 g[4] = {cmulc(p0, q0), cmulc(p0, q1), cmulc(p1, q0), cmulc(p1, q1)};
#pragma unroll
                for (int c = 0; c < 4; ++c) x[c] = cdiv(v[c], g[c], cabs2(g[c]));
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= tab.ns) break;
#pragma unroll
                    for (int c = 0; c < 4; ++c) ws[k] += w[c] * cabs2(cmul(g[c], tab.t[c][k]));
                }
            } else {
                const double2 p00 = jp[0], p01 = jp[1], p10 = jp[2], p11 = jp[3];
                const double2 q00 = jq[0], q01 = jq[1], q10 = jq[2], q11 = jq[3];
                // Y = adj(Jp) V
                const double2 y00 = csub(cmul(p11, v[0]), cmul(p01, v[2])), y01 = csub(cmul(p11, v[1]), cmul(p01, v[3]));
                const double2 y10 = csub(cmul(p00, v[2]), cmul(p10, v[0])), y11 = csub(cmul(p00, v[3]), cmul(p10, v[1]));
                // Z = Y adj(Jq)^H, adj(Jq)^H = [[conj q11, -conj q10], [-conj q01, conj q00]]
                const double2 z[4] = {csub(cmulc(y00, q11), cmulc(y01, q01)), csub(cmulc(y01, q00), cmulc(y00, q10)),
                                      csub(cmulc(y10, q11), cmulc(y11, q01)), csub(cmulc(y11, q00), cmulc(y10, q10))};
                const double2 detp = csub(cmul(p00, p11), cmul(p01, p10)), detq = csub(cmul(q00, q11), cmul(q01, q10));
                const double2 det = cmulc(detp, detq);
                const double det2 = cabs2(det);
#pragma unroll
                for (int c = 0; c < 4; ++c) x[c] = cdiv(z[c], det, det2);
                // row c = (i, j) of Jp (x) conj(Jq): Jp[i][k] conj(Jq[j][l]) at column (k, l)
                const double2 jpm[2][2] = {{p00, p01}, {p10, p11}}, jqm[2][2] = {{q00, q01}, {q10, q11}};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int i = c >> 1, j = c & 1;
                    const double2 m[4] = {cmulc(jpm[i][0], jqm[j][0]), cmulc(jpm[i][0], jqm[j][1]), cmulc(jpm[i][1], jqm[j][0]),
                                          cmulc(jpm[i][1], jqm[j][1])};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (k >= tab.ns) break;
                        double2 a = make_double2(0.0, 0.0);
#pragma unroll
                        for (int l = 0; l < 4; ++l) a = cadd(a, cmul(m[l], tab.t[l][k]));
                        ws[k] += w[c] * cabs2(a);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= tab.ns) break;
#pragma unroll
                for (int c = 0; c < 4; ++c) s[k] = cadd(s[k], cmul(tab.tinv[k][c], x[c]));
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= tab.ns) break;
            const size_t o = size_t(e) * size_t(out_se) + size_t(k) * size_t(out_sk);
            store_c(vis + o, s[k]);
            wgt[o] = R(ws[k]);
        }
    }
}

// 16 bytes per lane, grid stride: the copy the kernel's rate is set against (tools/bench_weight_data.py)
__global__ void __launch_bounds__(SK_THREADS) k_copy16(const float4 *__restrict__ src, float4 *__restrict__ dst, int64_t n)
{
    const int64_t step = int64_t(gridDim.x) * SK_THREADS;
    for (int64_t i = int64_t(blockIdx.x) * SK_THREADS + threadIdx.x; i < n; i += step) dst[i] = src[i];
}

struct Shape {
    int64_t nrow, nchan, nant, ntime, nbin;
};

// T of utils/stokes.py:33 (linear) and :35 (circular), rows = correlations, columns = I, Q, U, V
void coherency_matrix(bool circular, double2 t[4][4])
{
    const double2 O = make_double2(0, 0), I = make_double2(1, 0), N = make_double2(-1, 0), J = make_double2(0, 1), K = make_double2(0, -1);
    const double2 lin[4][4] = {{I, I, O, O}, {O, O, I, J}, {O, O, I, K}, {I, N, O, O}};
    const double2 circ[4][4] = {{I, O, O, I}, {O, I, J, O}, {O, I, K, O}, {I, O, O, N}};
    for (int c = 0; c < 4; ++c)
        for (int s = 0; s < 4; ++s) t[c][s] = circular ? circ[c][s] : lin[c][s];
}

StokesTable make_table(const pfbhip_stokes_spec &sp)
{
    PFB_REQUIRE(sp.nc == 2 || sp.nc == 4, "nc must be 2 or 4, not %d", int(sp.nc));
    PFB_REQUIRE(!(sp.full_jones && sp.nc != 4), "Full 2x2 jones mode requires 4 correlation data");
    PFB_REQUIRE(sp.ns >= 1 && sp.ns <= 4, "between one and four Stokes products, not %d", int(sp.ns));
    static const char names[] = "IQUV";
    for (int k = 0; k < sp.ns; ++k) {
        const int s = sp.product[k];
        PFB_REQUIRE(s >= 0 && s < 4 && (k == 0 || s > sp.product[k - 1]), "products must be ascending indices into IQUV");
        // two correlations are the parallel hands: I and Q of linear feeds, I and V of circular ones
        PFB_REQUIRE(sp.nc == 4 || s == 0 || s == (sp.circular ? 3 : 1), "%c is not available in %s polarisation with 2 correlations",
                    names[s], sp.circular ? "circular" : "linear");
    }
    double2 t[4][4];
    coherency_matrix(sp.circular != 0, t);
    StokesTable tab{};
    tab.ns = sp.ns;
    for (int k = 0; k < sp.ns; ++k)
        for (int c = 0; c < 4; ++c) {
            const double2 e = t[c][sp.product[k]];
            tab.t[c][k] = e;
            tab.tinv[k][c] = make_double2(0.5 * e.x, -0.5 * e.y);  // Tinv = T^H / 2: the columns of T are orthogonal, of norm^2 2
        }
    return tab;
}

// Everything an index could do wrong, before any launch.  Returns the row -> bin table (-1: in no bin); bins count from
// the smallest tbin_idx (weighting.py:380), and where two bins overlap the later one holds the row.
std::vector<int32_t> validate(const Shape &sh, const int64_t *tbin_idx, const int64_t *tbin_counts, const int32_t *ant1,
                              const int32_t *ant2)
{
    PFB_REQUIRE(sh.nrow >= 0 && sh.nchan >= 0 && sh.nant >= 1 && sh.ntime >= 0 && sh.nbin >= 0, "negative sizes");
    PFB_REQUIRE(sh.nchan < (int64_t(1) << 31) && sh.nant < (int64_t(1) << 31) && sh.nbin < (int64_t(1) << 31), "sizes too large");
    PFB_REQUIRE(sh.nrow == 0 || sh.nchan == 0 || sh.nrow < (int64_t(1) << 58) / sh.nchan, "too many samples");
    PFB_REQUIRE(sh.nbin <= sh.ntime, "jones has %lld time slots for %lld time bins", (long long)sh.ntime, (long long)sh.nbin);
    PFB_REQUIRE(sh.nbin == 0 || (tbin_idx && tbin_counts), "NULL argument");
    PFB_REQUIRE(sh.nrow == 0 || (ant1 && ant2), "NULL argument");
    std::vector<int32_t> row2bin(size_t(sh.nrow), -1);
    int64_t first = 0;
    for (int64_t t = 0; t < sh.nbin; ++t) first = t == 0 ? tbin_idx[0] : std::min(first, tbin_idx[t]);
    for (int64_t t = 0; t < sh.nbin; ++t) {
        const int64_t r0 = tbin_idx[t] - first, n = tbin_counts[t];
        PFB_REQUIRE(n >= 0 && r0 <= sh.nrow && n <= sh.nrow - r0, "time bin %lld covers rows [%lld, %lld) of %lld", (long long)t,
                    (long long)r0, (long long)(r0 + n), (long long)sh.nrow);
        for (int64_t r = r0; r < r0 + n; ++r) row2bin[size_t(r)] = int32_t(t);
    }
    for (int64_t r = 0; r < sh.nrow; ++r) {
        if (row2bin[size_t(r)] < 0) continue;
        PFB_REQUIRE(ant1[r] >= 0 && ant1[r] < sh.nant && ant2[r] >= 0 && ant2[r] < sh.nant,
                    "row %lld: antennas (%d, %d) outside [0, %lld)", (long long)r, int(ant1[r]), int(ant2[r]), (long long)sh.nant);
    }
    return row2bin;
}

template <typename R, int NC, bool FULL>
void launch(hipStream_t st, int64_t nsamp, const void *data, const void *weight, const uint8_t *flag, const double *jones,
            const int32_t *row2bin, const int32_t *ant1, const int32_t *ant2, const Shape &sh, const StokesTable &tab, int64_t se,
            int64_t sk, void *vis, void *wgt, uint8_t *mask)
{
    using C = typename Cplx<R>::type;
    const uint32_t grid = uint32_t(std::min<int64_t>(ceil_div(nsamp, SK_THREADS), SK_MAX_WORKGROUPS));
    hipLaunchKernelGGL((k_weight_data<R, NC, FULL>), dim3(grid), dim3(SK_THREADS), 0, st, static_cast<const C *>(data),
                       static_cast<const R *>(weight), flag, reinterpret_cast<const double2 *>(jones), row2bin, ant1, ant2, nsamp, sh.nchan,
                       sh.nant, tab, se, sk, static_cast<C *>(vis), static_cast<R *>(wgt), mask);
}

// out_dev: vis / wgt / mask are device arrays the kernel writes in place; otherwise host arrays filled by a copy
template <typename R>
void weight_data_impl(const pfbhip_stokes_spec *spec, const Shape &sh, const void *data, const void *weight, const uint8_t *flag,
                      const double *jones, const int64_t *tbin_idx, const int64_t *tbin_counts, const int32_t *ant1, const int32_t *ant2,
                      void *vis, void *wgt, uint8_t *mask, bool out_dev, double *device_ms)
{
    PFB_REQUIRE(spec, "NULL argument");
    const StokesTable tab = make_table(*spec);
    const std::vector<int32_t> row2bin = validate(sh, tbin_idx, tbin_counts, ant1, ant2);
    if (device_ms) *device_ms = 0.0;
    const int64_t nsamp = sh.nrow * sh.nchan;
    if (nsamp == 0) return;
    PFB_REQUIRE(data && weight && flag && vis && wgt, "NULL argument");
    const bool covered = std::any_of(row2bin.begin(), row2bin.end(), [](int32_t b) { return b >= 0; });
    PFB_REQUIRE(jones || !covered, "NULL argument");
    const int nc = spec->nc, ns = spec->ns, nj = spec->full_jones ? 4 : 2;
    const size_t n = size_t(nsamp), njones = size_t(sh.ntime) * size_t(sh.nant) * size_t(sh.nchan) * size_t(nj) * 2;
    const hipStream_t st = hipStreamPerThread;
    DevBuf<R> d_data{n * size_t(nc) * 2}, d_wgt_in{n * size_t(nc)}, d_vis, d_wgt;
    DevBuf<uint8_t> d_flag{n * size_t(nc)}, d_mask;
    DevBuf<double> d_jones{std::max<size_t>(njones, 1)};
    DevBuf<int32_t> d_bin{size_t(sh.nrow)}, d_a1{size_t(sh.nrow)}, d_a2{size_t(sh.nrow)};
    if (!out_dev) {
        d_vis.alloc(n * size_t(ns) * 2), d_wgt.alloc(n * size_t(ns));
        if (mask) d_mask.alloc(n);
    }
    void *o_vis = out_dev ? vis : d_vis.p, *o_wgt = out_dev ? wgt : d_wgt.p;
    uint8_t *o_mask = out_dev ? mask : d_mask.p;
    const int64_t se = spec->corr_first ? 1 : ns, sk = spec->corr_first ? nsamp : 1;
    const auto run = spec->full_jones ? launch<R, 4, true> : nc == 4 ? launch<R, 4, false> : launch<R, 2, false>;
    EventTimer timer(device_ms != nullptr);
    synced(st, [&] {  // the inputs are read from the caller's memory until it returns
        PFB_HIP(hipMemcpyAsync(d_data.p, data, d_data.bytes(), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(d_wgt_in.p, weight, d_wgt_in.bytes(), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(d_flag.p, flag, d_flag.bytes(), hipMemcpyHostToDevice, st));
        if (njones && jones) PFB_HIP(hipMemcpyAsync(d_jones.p, jones, njones * sizeof(double), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(d_bin.p, row2bin.data(), d_bin.bytes(), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(d_a1.p, ant1, d_a1.bytes(), hipMemcpyHostToDevice, st));
        PFB_HIP(hipMemcpyAsync(d_a2.p, ant2, d_a2.bytes(), hipMemcpyHostToDevice, st));
        // a caller that asks for the kernel's time gets that of a second, warm launch
        for (int pass = device_ms ? 0 : 1; pass < 2; ++pass) {
            if (pass == 1) timer.start(st);
            run(st, nsamp, d_data.p, d_wgt_in.p, d_flag.p, d_jones.p, d_bin.p, d_a1.p, d_a2.p, sh, tab, se, sk, o_vis, o_wgt, o_mask);
            PFB_HIP(hipGetLastError());
        }
        timer.stop(st);
        if (!out_dev) {
            PFB_HIP(hipMemcpyAsync(vis, d_vis.p, d_vis.bytes(), hipMemcpyDeviceToHost, st));
            PFB_HIP(hipMemcpyAsync(wgt, d_wgt.p, d_wgt.bytes(), hipMemcpyDeviceToHost, st));
            if (mask) PFB_HIP(hipMemcpyAsync(mask, d_mask.p, d_mask.bytes(), hipMemcpyDeviceToHost, st));
        }
    });
    if (device_ms) *device_ms = timer.ms();
}

}  // namespace

}  // namespace pfbhip

using namespace pfbhip;

extern "C" {

int pfbhip_weight_data(const pfbhip_stokes_spec *spec, int64_t nrow, int64_t nchan, int64_t nant, int64_t ntime, int64_t nbin,
                       const double *data_host, const double *weight_host, const uint8_t *flag_host, const double *jones_host,
                       const int64_t *tbin_idx, const int64_t *tbin_counts, const int32_t *ant1, const int32_t *ant2, double *vis_host,
                       double *wgt_host, uint8_t *mask_host, double *device_ms)
{
    return guarded([&] {
        weight_data_impl<double>(spec, Shape{nrow, nchan, nant, ntime, nbin}, data_host, weight_host, flag_host, jones_host, tbin_idx,
                                 tbin_counts, ant1, ant2, vis_host, wgt_host, mask_host, false, device_ms);
    });
}

int pfbhip_weight_data_sp(const pfbhip_stokes_spec *spec, int64_t nrow, int64_t nchan, int64_t nant, int64_t ntime, int64_t nbin,
                          const float *data_host, const float *weight_host, const uint8_t *flag_host, const double *jones_host,
                          const int64_t *tbin_idx, const int64_t *tbin_counts, const int32_t *ant1, const int32_t *ant2, float *vis_host,
                          float *wgt_host, uint8_t *mask_host, double *device_ms)
{
    return guarded([&] {
        weight_data_impl<float>(spec, Shape{nrow, nchan, nant, ntime, nbin}, data_host, weight_host, flag_host, jones_host, tbin_idx,
                                tbin_counts, ant1, ant2, vis_host, wgt_host, mask_host, false, device_ms);
    });
}

int pfbhip_weight_data_dev(const pfbhip_stokes_spec *spec, int64_t nrow, int64_t nchan, int64_t nant, int64_t ntime, int64_t nbin,
                           const double *data_host, const double *weight_host, const uint8_t *flag_host, const double *jones_host,
                           const int64_t *tbin_idx, const int64_t *tbin_counts, const int32_t *ant1, const int32_t *ant2, double *vis_dev,
                           double *wgt_dev, uint8_t *mask_dev, double *device_ms)
{
    return guarded([&] {
        weight_data_impl<double>(spec, Shape{nrow, nchan, nant, ntime, nbin}, data_host, weight_host, flag_host, jones_host, tbin_idx,
                                 tbin_counts, ant1, ant2, vis_dev, wgt_dev, mask_dev, true, device_ms);
    });
}

int pfbhip_debug_copy16(int64_t nbytes, int32_t reps, double *ms)
{
    return guarded([&] {
        PFB_REQUIRE(ms && nbytes >= 16 && nbytes % 16 == 0 && reps >= 1 && reps <= 1000, "bad arguments");
        const hipStream_t st = hipStreamPerThread;
        DevBuf<float4> src{size_t(nbytes / 16)}, dst{size_t(nbytes / 16)};
        const int64_t n = nbytes / 16;
        const uint32_t grid = uint32_t(std::min<int64_t>(ceil_div(n, SK_THREADS), SK_MAX_WORKGROUPS));
        EventTimer timer(true);
        synced(st, [&] {
            PFB_HIP(hipMemsetAsync(src.p, 0, src.bytes(), st));
            hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(SK_THREADS), 0, st, src.p, dst.p, n);  // warm-up
            timer.start(st);
            for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(SK_THREADS), 0, st, src.p, dst.p, n);
            PFB_HIP(hipGetLastError());
            timer.stop(st);
        });
        *ms = timer.ms() / double(reps);
    });
}

}  // extern "C"
