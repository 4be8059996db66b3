// restore.hip -- convolution of an image cube to a Gaussian resolution, and the restore step, on MI355X.
//
// Replaces, of the reference,
//   /root/reference/src/pfb_imaging/utils/misc.py:123-192      convolve2gaussres
//   /root/reference/src/pfb_imaging/utils/misc.py:468-502      gaussian2d (as convolve2gaussres calls it: nsigma = 5)
//   /root/reference/src/pfb_imaging/utils/misc.py:107-120      get_padding_info
//   /root/reference/src/pfb_imaging/utils/restoration.py:71-88 restore_image's arithmetic (IMAGE = conv(model) + rconv)
//
// Per band:  out = fftshift(c2r(r2c(ifftshift(pad(image))) * K))[unpad] / N  with  K = gausshat, or, given the intrinsic
// resolution, K = where(|thishat| > 0, gausshat / thishat, 0).  The transforms are realfft2d.hpp's (the padded sizes
// good_size(n + int(pfrac n), real) are mostly odd or carry factors the row-FFT pipeline of psffft.hip does not take); the
// passes around them are the kernels below, each one streaming pass.  The centred pad and the two shifts are index maps
// on load and on store; the Gaussian is rendered straight into its padded, shifted place; its normalisation is a
// two-stage sum in a fixed order whose result the spectral pass reads from device memory (r2c(g / s) = r2c(g) / s).
// The plan holds one padded plane, one image spectrum and two kernel spectra: bands go through them one after another.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>

#include "abi_scope.hpp"
#include "common.hpp"
#include "realfft2d.hpp"

namespace pfbhip {

// numpy's shifts on an axis of any length n, as source indices:
//   ifftshift(a)[i] = a[(i + n / 2) % n]           fftshift(a)[i] = a[(i + (n + 1) / 2) % n]
// (np.roll by -(n // 2) and by +(n // 2)).  They coincide for even n only.
__device__ __forceinline__ int ifftshift_src(int i, int n)
{
    const int p = i + n / 2;
    return p >= n ? p - n : p;
}
__device__ __forceinline__ int fftshift_src(int i, int n)
{
    const int p = i + (n + 1) / 2;
    return p >= n ? p - n : p;
}

struct Geom {
    int nx, ny, nfx, nfy, plx, ply;
};

template <int V>
__device__ __forceinline__ void store_v(double *p, const double (&v)[V])
{
    if constexpr (V == 2) *reinterpret_cast<double2 *>(p) = make_double2(v[0], v[1]);
    else p[0] = v[0];
}

// pad (nfx, nfy) = ifftshift(pad_centred(img * in_scale)).  One workgroup per padded row; V = 2 (nfy even): 16-byte stores.
template <int V>
__global__ __launch_bounds__(256) void k_pad_shift(const double *__restrict__ img, Geom g, double in_scale,
                                                   double *__restrict__ pad)
{
    const int i = blockIdx.x;
    const int ix = ifftshift_src(i, g.nfx) - g.plx;
    const bool row_in = ix >= 0 && ix < g.nx;
    const double *src = img + size_t(row_in ? ix : 0) * g.ny;
    double *dst = pad + size_t(i) * g.nfy;
    for (int j0 = threadIdx.x * V; j0 < g.nfy; j0 += blockDim.x * V) {
        double v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int iy = ifftshift_src(j0 + k, g.nfy) - g.ply;
            v[k] = (row_in && iy >= 0 && iy < g.ny) ? src[iy] * in_scale : 0.0;
        }
        store_v<V>(dst + j0, v);
    }
}

// gaussian2d of the reference on the grids x = (-(nx // 2) + ix) * sx, y = (-(ny // 2) + iy) * sy:
// exp(-c * [x y] A [x y]^T) where x^2 + y^2 <= extent, exactly 0 elsewhere.
struct GaussPar {
    double a00, a01, a10, a11, c, extent, sx, sy;
};

// pad = ifftshift(pad_centred(gaussian)), unnormalised; partial[4 * row + wave] = that wave's share of the row's sum.
template <int V>
__global__ __launch_bounds__(256) void k_gauss_render(GaussPar q, Geom g, double *__restrict__ pad, double *__restrict__ partial)
{
    const int i = blockIdx.x;
    const int ix = ifftshift_src(i, g.nfx) - g.plx;
    const bool row_in = ix >= 0 && ix < g.nx;
    const double x = double(ix - g.nx / 2) * q.sx;
    double *dst = pad + size_t(i) * g.nfy;
    double acc = 0.0;
    for (int j0 = threadIdx.x * V; j0 < g.nfy; j0 += blockDim.x * V) {
        double v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int iy = ifftshift_src(j0 + k, g.nfy) - g.ply;
            v[k] = 0.0;
            if (row_in && iy >= 0 && iy < g.ny) {
                const double y = double(iy - g.ny / 2) * q.sy;
                if (x * x + y * y <= q.extent) v[k] = exp(-q.c * (x * (q.a00 * x + q.a01 * y) + y * (q.a10 * x + q.a11 * y)));
            }
            acc += v[k];
        }
        store_v<V>(dst + j0, v);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) partial[size_t(i) * 4 + (threadIdx.x >> 6)] = acc;
}

// out[0] = sum of partial[0:n], one wave, fixed order: two calls agree bit for bit.
__global__ __launch_bounds__(64) void k_sum_partials(const double *__restrict__ partial, int64_t n, double *__restrict__ out)
{
    double acc = 0.0;
    for (int64_t k = threadIdx.x; k < n; k += 64) acc += partial[k];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x == 0) out[0] = acc;
}

// imhat *= K in place.  ghat and thishat are the spectra of the unnormalised kernels; sums (NULL without norm_kernel) holds
// their two sums.  Complex division as numpy's (Smith).
__global__ __launch_bounds__(256) void k_spec_combine(double2 *__restrict__ imhat, const double2 *__restrict__ ghat,
                                                      const double2 *__restrict__ thishat, const double *__restrict__ sums,
                                                      int64_t n)
{
    const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    double2 k = ghat[i];
    if (sums) {
        const double s = sums[0];
        k.x /= s;
        k.y /= s;
    }
    if (thishat) {
        double2 t = thishat[i];
        if (sums) {
            const double s = sums[1];
            t.x /= s;
            t.y /= s;
        }
        if (t.x == 0.0 && t.y == 0.0) {
            k = make_double2(0.0, 0.0);
        } else if (fabs(t.x) >= fabs(t.y)) {
            const double r = t.y / t.x, d = t.x + t.y * r;
            k = make_double2((k.x + k.y * r) / d, (k.y - k.x * r) / d);
        } else {
            const double r = t.x / t.y, d = t.x * r + t.y;
            k = make_double2((k.x * r + k.y) / d, (k.y * r - k.x) / d);
        }
    }
    const double2 v = imhat[i];
    imhat[i] = make_double2(v.x * k.x - v.y * k.y, v.x * k.y + v.y * k.x);
}

// out (nx, ny) = [out +] fftshift(pad)[plx : plx + nx, ply : ply + ny] * scale [+ add_scale * add].  V = 2 (ny even): 16-byte
// accesses to out and add.
template <int V>
__global__ __launch_bounds__(256) void k_crop_shift(const double *__restrict__ pad, Geom g, double scale,
                                                    const double *__restrict__ add, double add_scale, int accumulate,
                                                    double *__restrict__ out)
{
    const int ix = blockIdx.x;
    const double *src = pad + size_t(fftshift_src(g.plx + ix, g.nfx)) * g.nfy;
    const size_t o = size_t(ix) * g.ny;
    for (int j0 = threadIdx.x * V; j0 < g.ny; j0 += blockDim.x * V) {
        double v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = src[fftshift_src(g.ply + j0 + k, g.nfy)] * scale;
        if (add) {
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] += add_scale * add[o + j0 + k];
        }
        if (accumulate) {
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] += out[o + j0 + k];
        }
        store_v<V>(out + o + j0, v);
    }
}

// the three numbers of one (emaj, emin, pa) as gaussian2d turns them into a quadratic form (misc.py:476-489)
static GaussPar gauss_par(const double *p, double sx, double sy)
{
    const double smaj = p[0], smin = p[1], pa = p[2];
    const double fwhm = 2.0 * std::sqrt(2.0 * std::log(2.0));
    const double r[2][2] = {{-std::sin(pa), -std::cos(pa)}, {std::cos(pa), -std::sin(pa)}};
    const double d[2] = {1.0 / (smaj * smaj), 1.0 / (smin * smin)};
    double a[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) a[i][j] = r[i][0] * d[0] * r[j][0] + r[i][1] * d[1] * r[j][1];
    const double sig = 5.0 * (smaj / fwhm);
    return GaussPar{a[0][0], a[0][1], a[1][0], a[1][1], 0.5 * fwhm * fwhm, sig * sig, sx, sy};
}

static void check_pars(const double *p, int64_t n, const char *name)
{
    for (int64_t b = 0; b < n; ++b) {
        const double *q = p + 3 * b;
        PFB_REQUIRE(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]), "%s[%lld] = (%g, %g, %g) is not finite", name,
                    (long long)b, q[0], q[1], q[2]);
        PFB_REQUIRE(q[0] > 0.0 && q[1] > 0.0, "%s[%lld]: emaj = %g and emin = %g must be positive", name, (long long)b, q[0], q[1]);
        PFB_REQUIRE(q[1] <= q[0], "%s[%lld]: emin = %g > emaj = %g", name, (long long)b, q[1], q[0]);
    }
}

// np.allclose(f, i) on one band's three numbers (rtol 1e-5, atol 1e-8, relative to the second argument)
static bool allclose3(const double *f, const double *i)
{
    for (int k = 0; k < 3; ++k)
        if (!(std::fabs(f[k] - i[k]) <= 1e-8 + 1e-5 * std::fabs(i[k]))) return false;
    return true;
}

}  // namespace pfbhip

using namespace pfbhip;

struct pfbhip_gaussconv {
    int64_t nband = 0, nx = 0, ny = 0;
    Geom g{};
    int64_t nyo2 = 0;
    hipStream_t stream = nullptr;
    RealFFT2D fft;
    DevBuf<double> pad;              // (nfx, nfy): the padded image, then the kernel being rendered, then c2r's output
    DevBuf<double2> imhat, ghat, that;  // (nfx, nyo2) each
    DevBuf<double> partial, sums;    // (4 nfx) wave sums of a render; [sum of g, sum of thiskern]
    DevBuf<double> d_a, d_b, d_o, d_kf, d_ki;  // staging of the host-array entry points
    ~pfbhip_gaussconv()
    {
        if (stream) (void)hipStreamDestroy(stream);
    }
    size_t npix() const { return size_t(nx) * size_t(ny); }

    void pad_shift(const double *img, double in_scale)
    {
        if (g.nfy % 2 == 0) hipLaunchKernelGGL(k_pad_shift<2>, dim3(g.nfx), dim3(256), 0, stream, img, g, in_scale, pad.p);
        else hipLaunchKernelGGL(k_pad_shift<1>, dim3(g.nfx), dim3(256), 0, stream, img, g, in_scale, pad.p);
        PFB_HIP(hipGetLastError());
    }
    // spectrum of one kernel -> hat; its sum -> sums[slot] (rendered kernels only: an image comes normalised as it should be)
    void kernel_hat(const double *par, const double *kern_img, double sx, double sy, DevBuf<double2> &hat, int slot)
    {
        if (kern_img) {
            pad_shift(kern_img, 1.0);
        } else {
            const GaussPar q = gauss_par(par, sx, sy);
            if (g.nfy % 2 == 0) hipLaunchKernelGGL(k_gauss_render<2>, dim3(g.nfx), dim3(256), 0, stream, q, g, pad.p, partial.p);
            else hipLaunchKernelGGL(k_gauss_render<1>, dim3(g.nfx), dim3(256), 0, stream, q, g, pad.p, partial.p);
            PFB_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(64), 0, stream, partial.p, int64_t(partial.n), sums.p + slot);
            PFB_HIP(hipGetLastError());
        }
        fft.r2c(pad.p, hat.p);
    }
    // out = [out +] crop(conv(img * in_scale, K)) [+ add_scale * add], K from ghat (and that when ratio)
    void convolve(const double *img, double in_scale, bool ratio, bool normalised, const double *add, double add_scale,
                  int accumulate, double *out)
    {
        pad_shift(img, in_scale);
        fft.r2c(pad.p, imhat.p);
        const int64_t nh = int64_t(g.nfx) * nyo2;
        hipLaunchKernelGGL(k_spec_combine, dim3(uint32_t(ceil_div(nh, 256))), dim3(256), 0, stream, imhat.p, ghat.p,
                           ratio ? that.p : nullptr, normalised ? sums.p : nullptr, nh);
        PFB_HIP(hipGetLastError());
        fft.c2r(imhat.p, pad.p);
        const double scale = 1.0 / (double(g.nfx) * double(g.nfy));
        // 16-byte accesses need ny even (every row then starts on an even element) and 16-byte-aligned cubes
        const bool vec = g.ny % 2 == 0 && (reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(add)) % 16 == 0;
        if (vec)
            hipLaunchKernelGGL(k_crop_shift<2>, dim3(g.nx), dim3(256), 0, stream, pad.p, g, scale, add, add_scale, accumulate, out);
        else
            hipLaunchKernelGGL(k_crop_shift<1>, dim3(g.nx), dim3(256), 0, stream, pad.p, g, scale, add, add_scale, accumulate, out);
        PFB_HIP(hipGetLastError());
    }

    void check_args(const double *parf, int64_t nparf, const double *pari, int64_t npari, bool need_pari) const
    {
        PFB_REQUIRE(parf, "NULL gaussparf");
        PFB_REQUIRE(nparf == 1 || nparf == nband, "gaussparf holds %lld parameter sets: expected 1 or nband = %lld", (long long)nparf,
                    (long long)nband);
        check_pars(parf, nparf, "gaussparf");
        PFB_REQUIRE(!need_pari || pari, "NULL gausspari");
        if (pari) {
            PFB_REQUIRE(npari == nband, "gausspari must be of length nband = %lld, not %lld", (long long)nband, (long long)npari);
            check_pars(pari, npari, "gausspari");
        }
    }

    // all pointers on the device; kernf (nparf, nx, ny) / kerni (nband, nx, ny): kernels rendered by the caller, or NULL
    void apply(const double *image, const double *parf, int64_t nparf, const double *pari, int norm_kernel, double sx, double sy,
               const double *kernf, const double *kerni, double *out)
    {
        const bool normalised = norm_kernel != 0 && !kernf;
        for (int64_t b = 0; b < nband; ++b) {
            if (b == 0 || nparf > 1) {
                const int64_t k = nparf > 1 ? b : 0;
                kernel_hat(parf + 3 * k, kernf ? kernf + size_t(k) * npix() : nullptr, sx, sy, ghat, 0);
            }
            if (pari) kernel_hat(pari + 3 * b, kerni ? kerni + size_t(b) * npix() : nullptr, sx, sy, that, 1);
            convolve(image + size_t(b) * npix(), 1.0, pari != nullptr, normalised, nullptr, 0.0, 0, out + size_t(b) * npix());
        }
    }

    // restoration.py:71-88 with the allclose test per band: image = conv(model, gf) + (close ? residual / wsum
    //                                                                                   : conv(residual / wsum, gf / gi))
    void restore(const double *model, const double *residual, const double *wsum, const double *pari, const double *parf,
                 int64_t nparf, double *image)
    {
        for (int64_t b = 0; b < nband; ++b) {
            const double *pf = parf + 3 * (nparf > 1 ? b : 0), *pi = pari + 3 * b;
            const bool close = allclose3(pf, pi);
            const double rw = 1.0 / wsum[b];
            const size_t o = size_t(b) * npix();
            if (b == 0 || nparf > 1) kernel_hat(pf, nullptr, 1.0, 1.0, ghat, 0);
            convolve(model + o, 1.0, false, false, close ? residual + o : nullptr, rw, 0, image + o);
            if (!close) {
                kernel_hat(pi, nullptr, 1.0, 1.0, that, 1);
                convolve(residual + o, rw, true, false, nullptr, 0.0, 1, image + o);
            }
        }
    }
};

extern "C" {

int pfbhip_gaussconv_create(int64_t nband, int64_t nx, int64_t ny, double pfrac, pfbhip_gaussconv **out)
{
    return guarded([&] {
        PFB_REQUIRE(out, "NULL argument");
        *out = nullptr;
        PFB_REQUIRE(nband >= 1 && nx >= 1 && ny >= 1, "bad cube shape (%lld, %lld, %lld)", (long long)nband, (long long)nx, (long long)ny);
        PFB_REQUIRE(std::isfinite(pfrac) && pfrac >= 0.0 && pfrac <= 16.0, "bad padding fraction %g", pfrac);
        const int64_t nfx = good_size(nx + int64_t(pfrac * double(nx)), true), nfy = good_size(ny + int64_t(pfrac * double(ny)), true);
        PFB_REQUIRE(nfx <= (int64_t(1) << 20) && nfy <= (int64_t(1) << 20), "padded size (%lld, %lld) is out of range", (long long)nfx,
                    (long long)nfy);
        // the reference unpads with slice(l, -r): r == 0 makes that an empty array (misc.py:118-119); refused here
        PFB_REQUIRE(nfx > nx && nfy > ny,
                    "padding fraction %g leaves no right pad on (%lld, %lld) -> (%lld, %lld): the reference's unpad slice is empty there",
                    pfrac, (long long)nx, (long long)ny, (long long)nfx, (long long)nfy);
        std::unique_ptr<pfbhip_gaussconv> p(new pfbhip_gaussconv);
        p->nband = nband;
        p->nx = nx;
        p->ny = ny;
        p->g = Geom{int(nx), int(ny), int(nfx), int(nfy), int((nfx - nx) / 2), int((nfy - ny) / 2)};
        p->nyo2 = nfy / 2 + 1;
        PFB_HIP(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
        p->fft.create(nfx, nfy, p->stream);
        p->pad.alloc(size_t(nfx) * size_t(nfy));
        const size_t nh = size_t(nfx) * size_t(p->nyo2);
        p->imhat.alloc(nh);
        p->ghat.alloc(nh);
        p->that.alloc(nh);
        p->partial.alloc(size_t(nfx) * 4);
        p->sums.alloc(2);
        *out = p.release();
    });
}

int pfbhip_gaussconv_destroy(pfbhip_gaussconv *h)
{
    return guarded([&] { delete h; });
}

int pfbhip_gaussconv_shape(const pfbhip_gaussconv *h, int64_t *nfft_x, int64_t *nfft_y, int64_t *padl_x, int64_t *padl_y)
{
    return guarded([&] {
        PFB_REQUIRE(h && nfft_x && nfft_y && padl_x && padl_y, "NULL argument");
        *nfft_x = h->g.nfx;
        *nfft_y = h->g.nfy;
        *padl_x = h->g.plx;
        *padl_y = h->g.ply;
    });
}

static void check_scales(double sx, double sy)
{
    PFB_REQUIRE(std::isfinite(sx) && std::isfinite(sy) && sx != 0.0 && sy != 0.0, "bad axis scales (%g, %g)", sx, sy);
}

int pfbhip_gaussconv_apply_dev(pfbhip_gaussconv *h, const double *image_dev, const double *gaussparf, int64_t nparf,
                               const double *gausspari, int64_t npari, int norm_kernel, double scale_x, double scale_y,
                               const double *kernf_dev, const double *kerni_dev, double *out_dev)
{
    return guarded([&] {
        PFB_REQUIRE(h && image_dev && out_dev, "NULL argument");
        h->check_args(gaussparf, nparf, gausspari, npari, false);
        check_scales(scale_x, scale_y);
        PFB_REQUIRE(!kerni_dev || gausspari, "kerni without gausspari");
        PFB_REQUIRE(!gausspari || (kernf_dev == nullptr) == (kerni_dev == nullptr), "kernf and kerni must be given together");
        synced(h->stream, [&] {
            h->apply(image_dev, gaussparf, nparf, gausspari, norm_kernel, scale_x, scale_y, kernf_dev, kerni_dev, out_dev);
        });
    });
}

int pfbhip_gaussconv_apply(pfbhip_gaussconv *h, const double *image_host, const double *gaussparf, int64_t nparf,
                           const double *gausspari, int64_t npari, int norm_kernel, double scale_x, double scale_y,
                           const double *kernf_host, const double *kerni_host, double *out_host)
{
    return guarded([&] {
        PFB_REQUIRE(h && image_host && out_host, "NULL argument");
        h->check_args(gaussparf, nparf, gausspari, npari, false);
        check_scales(scale_x, scale_y);
        PFB_REQUIRE(!kerni_host || gausspari, "kerni without gausspari");
        PFB_REQUIRE(!gausspari || (kernf_host == nullptr) == (kerni_host == nullptr), "kernf and kerni must be given together");
        const size_t n = size_t(h->nband) * h->npix(), bytes = n * sizeof(double);
        hipStream_t st = h->stream;
        synced(st, [&] {
            const double *image = upload(h->d_a, image_host, n, st);
            const double *kernf = upload(h->d_kf, kernf_host, size_t(nparf) * h->npix(), st);
            const double *kerni = upload(h->d_ki, kerni_host, n, st);
            h->d_o.ensure(n);
            h->apply(image, gaussparf, nparf, gausspari, norm_kernel, scale_x, scale_y, kernf, kerni, h->d_o.p);
            PFB_HIP(hipMemcpyAsync(out_host, h->d_o.p, bytes, hipMemcpyDeviceToHost, st));
        });
    });
}

static void check_wsum(const pfbhip_gaussconv *h, const double *wsum)
{
    PFB_REQUIRE(wsum, "NULL wsum");
    for (int64_t b = 0; b < h->nband; ++b)
        PFB_REQUIRE(std::isfinite(wsum[b]) && wsum[b] != 0.0, "wsum[%lld] = %g: the residual is divided by it", (long long)b, wsum[b]);
}

int pfbhip_gaussconv_restore_dev(pfbhip_gaussconv *h, const double *model_dev, const double *residual_dev, const double *wsum,
                                 const double *gausspari, int64_t npari, const double *gaussparf, int64_t nparf,
                                 double *image_dev)
{
    return guarded([&] {
        PFB_REQUIRE(h && model_dev && residual_dev && image_dev, "NULL argument");
        h->check_args(gaussparf, nparf, gausspari, npari, true);
        check_wsum(h, wsum);
        synced(h->stream, [&] { h->restore(model_dev, residual_dev, wsum, gausspari, gaussparf, nparf, image_dev); });
    });
}

int pfbhip_gaussconv_restore(pfbhip_gaussconv *h, const double *model_host, const double *residual_host, const double *wsum,
                             const double *gausspari, int64_t npari, const double *gaussparf, int64_t nparf, double *image_host)
{
    return guarded([&] {
        PFB_REQUIRE(h && model_host && residual_host && image_host, "NULL argument");
        h->check_args(gaussparf, nparf, gausspari, npari, true);
        check_wsum(h, wsum);
        const size_t n = size_t(h->nband) * h->npix(), bytes = n * sizeof(double);
        hipStream_t st = h->stream;
        synced(st, [&] {
            const double *model = upload(h->d_a, model_host, n, st);
            const double *residual = upload(h->d_b, residual_host, n, st);
            h->d_o.ensure(n);
            h->restore(model, residual, wsum, gausspari, gaussparf, nparf, h->d_o.p);
            PFB_HIP(hipMemcpyAsync(image_host, h->d_o.p, bytes, hipMemcpyDeviceToHost, st));
        });
    });
}

// Test hook: fills every buffer the plan owns with `byte` (0xFF: NaNs), so that a test can show that an apply reads nothing an
// earlier one left behind.
int pfbhip_gaussconv_debug_fill(pfbhip_gaussconv *h, int byte)
{
    return guarded([&] {
        PFB_REQUIRE(h, "NULL argument");
        hipStream_t st = h->stream;
        auto fill = [&](void *p, size_t bytes) {
            if (p && bytes) PFB_HIP(hipMemsetAsync(p, byte, bytes, st));
        };
        fill(h->pad.p, h->pad.bytes());
        fill(h->imhat.p, h->imhat.bytes());
        fill(h->ghat.p, h->ghat.bytes());
        fill(h->that.p, h->that.bytes());
        fill(h->partial.p, h->partial.bytes());
        fill(h->sums.p, h->sums.bytes());
        fill(h->d_a.p, h->d_a.bytes());
        fill(h->d_b.p, h->d_b.bytes());
        fill(h->d_o.p, h->d_o.bytes());
        fill(h->d_kf.p, h->d_kf.bytes());
        fill(h->d_ki.p, h->d_ki.bytes());
        PFB_HIP(hipStreamSynchronize(st));
    });
}

}  // extern "C"
