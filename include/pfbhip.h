/*
 * pfbhip.h -- C-ABI of libpfbhip.so, the MI355X (gfx950) measurement operator
 * for pfb-imaging.
 *
 * Every entry point replaces one of the third-party native calls the reference
 * makes on its hot path (the reference is 100 % Python; its FFI for this path
 * is the ducc0 / numba call boundary).  Citations are file:line under
 * /root/reference.  All functions return 0 on success and a non-zero status
 * on failure; pfbhip_last_error() then returns a thread-local message.  No
 * C++ exception crosses this boundary.  Pointers named *_host are caller-owned
 * host memory (numpy arrays, possibly read-only); pointers named *_dev are
 * device memory obtained from pfbhip_malloc.  Complex arrays are interleaved
 * (re, im) doubles.  All arrays are C-contiguous.
 *
 * Threading: a handle is single-caller (like the reference's operators, which
 * share scratch: src/pfb_imaging/operators/hessian.py:481-485); different
 * handles may be used from different host threads.  Each handle owns a HIP
 * stream; calls are synchronous with respect to the host unless stated.  That
 * holds on failure too: a call does not return, whatever its status, while the
 * device still reads or writes memory the caller passed.
 */
#ifndef PFBHIP_H
#define PFBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFBHIP_OK 0
#define PFBHIP_ERR_INVALID 1  /* bad argument / shape (-> ValueError)   */
#define PFBHIP_ERR_RUNTIME 2  /* HIP / rocFFT / RCCL failure (-> RuntimeError) */

/* ---- runtime ------------------------------------------------------- */
const char *pfbhip_last_error(void);
int pfbhip_device_count(int *count);
int pfbhip_set_device(int device);
int pfbhip_get_device(int *device);
int pfbhip_device_name(char *buf, size_t buflen);
int pfbhip_mem_info(size_t *free_bytes, size_t *total_bytes);
/* Device blocks released by destroyed handles are kept for the next handle of the same sizes (hipMalloc costs ~45 ms per GB
 * here; a plan is created per band and major cycle, as the reference creates its ducc0 plans per call,
 * src/pfb_imaging/operators/gridder.py:590-613).  Reports the bytes currently cached (before the flush) and, with flush != 0,
 * returns them to the driver.  PFBHIP_DEVCACHE_MB bounds the cache (default 131072, 0 = off); it empties itself when an
 * allocation fails. */
int pfbhip_device_cache(size_t *cached_bytes, int flush);
/* replaces ducc0.misc.resize_thread_pool / thread_pool_size (src/pfb_imaging/operators/band_worker.py:50-52):
 * the "pool" is the GPU; kept so callers need no change. */
int pfbhip_resize_thread_pool(int nthreads);
int pfbhip_thread_pool_size(void);
/* replaces ducc0.fft.good_size (src/pfb_imaging/utils/misc.py:921-951):
 * smallest 2-3-5-7-11-smooth (real=0) or 2-3-5-smooth (real=1) integer >= n. */
int64_t pfbhip_good_size(int64_t n, int real);

/* ---- device memory (for device-resident callers: on-device CG, bench) ---- */
/* 64-bit content hash of a whole host buffer (multi-threaded, memory-bandwidth bound).  The Python layer keys its
 * plan caches on it: the reference's ducc0 calls are stateless (operators/gridder.py:590-613), so a cached plan is
 * reused only for byte-identical uvw / freq / mask / weights / psfhat. */
uint64_t pfbhip_hash64(const void *data_host, size_t nbytes);
/* Page-locked host buffers for result arrays (device-to-host copies into pinned memory run at the PCIe rate; into
 * pageable memory the runtime stages them at a fraction of it). */
int pfbhip_host_alloc(void **ptr_host, size_t bytes);
int pfbhip_host_free(void *ptr_host);
int pfbhip_malloc(void **ptr_dev, size_t bytes);
int pfbhip_free(void *ptr_dev);
int pfbhip_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int pfbhip_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
int pfbhip_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes);
int pfbhip_memset(void *dst_dev, int value, size_t bytes);
int pfbhip_synchronize(void);

/* ---- w-stacking gridder / degridder --------------------------------- */
/*
 * Replaces ducc0.wgridder.experimental.vis2dirty / dirty2vis as called at
 *   src/pfb_imaging/operators/hessian.py:50-89      (hessian_slice)
 *   src/pfb_imaging/operators/gridder.py:78,128,590-613,633-656,852-910,972-1016,1067-1117
 * A handle binds what is constant over a run -- geometry, uvw, freq, mask --
 * (the reference pins exactly these per band: operators/band_worker.py:61-106)
 * and holds the tile-sorted visibility index, kernel choice, correction image,
 * rocFFT plans and device scratch.
 */
typedef struct pfbhip_gridder pfbhip_gridder;

typedef struct pfbhip_gridder_params {
    int64_t nrow, nchan;
    int64_t nx, ny;               /* npix_x, npix_y                          */
    double pixsize_x, pixsize_y;  /* radians                                 */
    double center_x, center_y;    /* as ducc0: x0 = -l0, y0 = -m0 on the pfb path (gridder.py:23-34) */
    double epsilon;
    double sigma_min, sigma_max;  /* oversampling bounds (gridder.py:609-610) */
    int32_t flip_u, flip_v, flip_w;
    int32_t do_wgridding;
    int32_t divide_by_n;
    int32_t verbosity;
    /* 0 / 0.0 = automatic.  Tests pin the kernel row / w-plane scheme with these. */
    int32_t force_W;
    int32_t force_wmode; /* 0 auto, 1 ES-kernel w-planes, 2 polynomial (Chebyshev-node) w-planes, 3 one plane (differentiated kernels) */
    double force_sigma;
} pfbhip_gridder_params;

typedef struct pfbhip_gridder_info {
    int64_t nu, nv;        /* oversampled uv-grid                             */
    int64_t nplanes;       /* w-planes                                        */
    int64_t nactive;       /* unmasked visibilities                           */
    int64_t ntiles, nwork; /* uv tiles, (tile, chunk) work items              */
    int32_t W, tile;       /* kernel support, tile edge (cells)               */
    double beta, sigma;    /* ES kernel exp(beta (sqrt(1-x^2) - 1)), design oversampling */
    double wmin, dw;       /* plane p sits at w = wmin + p dw (wavelengths)   */
    double nshift, lshift, mshift;
    double kernel_eps;     /* tabulated 1-D image-edge error of the chosen row  */
    /* w-plane scheme.  wmode 0: W-wide ES kernel over equispaced planes wmin + p dw (classic
     * w-stacking; each visibility touches W planes).  wmode 1: the w range [wcenter - whalf,
     * wcenter + whalf] is interpolated by a degree-(nplanes-1) polynomial through Chebyshev
     * nodes (each visibility touches all planes with Lagrange weights; no w-correction in the
     * image).  wmode 2: see nderiv below.  The cheapest admissible scheme is chosen per plan. */
    int32_t wmode;
    int32_t occ_rows;      /* rows of the uv-plane that hold visibilities (only these are cleared / transformed) */
    double wcenter, whalf;
    size_t device_bytes;   /* device memory held by the handle                */
    /* plane transform: bit 0 = hand-written row FFT on the first axis (else rocFFT); bit 1 = second axis fused
     * with pad / crop / w-screen (sizes {1,3,5,7,9,15} x 2^a in 1024..16384); bit 2 = second axis on the hand-written
     * FFT with separate pad / crop kernels (the doubled sizes 20480, 24576); neither bit 1 nor 2: rocFFT; bit 3 = first
     * axis with the crop / pad + transpose folded into the transform (no separate transpose kernels) */
    int32_t fft_mode;
    int32_t screen_poly;   /* coefficients of the n-1 polynomial of the fused w-screen (0: closed form) */
    /* scatter kernel: 2 = record-driven register-footprint form (k_grid_rec), 1 = register-footprint form (k_grid_blk:
     * visibilities sorted by tile and 4 x 4-cell block, LDS atomics only when the block changes), 0 = diagonal-walk form
     * (k_grid_mp: LDS atomics per tap) */
    int32_t scatter_mode;
    /* launches of the scatter per pass over the planes: 4 = one per tile colour (tile-row / tile-column parity), whose
     * tile flush is a plain read-add-write because no two tiles of a colour overlap; 1 = one launch, atomic flush */
    int32_t scatter_launches;
    /* cells of one uv-plane the scatter / gather can touch (tiles with visibilities + halo); the first-axis transforms and
     * the Hessian's plane clear move only these of the occupied rows (0: not computed, every cell of the occupied rows) */
    int64_t used_cells;
    /* w-screen of the fused second axis, passes (launches of <= 4 planes) per form: composite cos / sin polynomials of the whole
     * phase (small w x field), separable form (per-plane column table x row factor x residual polynomials), and the rest
     * (n - 1 polynomial + sincos per pixel and plane) */
    int32_t screen_composite, screen_separable;
    /* wmode 2 (round 4): ONE uv-plane at wcenter; the rest of the w-term, exp(-2 pi i (w - wcenter)(n - 1 + nshift)), is
     * interpolated in s = l^2 + m^2 through nderiv Chebyshev nodes of [0, smax] and carried by the gridding kernel of each
     * visibility: multiplication by s^k in the image = the 2k-th derivatives of the kernel on the uv-plane (nderiv kernel
     * functions per axis; phase centre on axis only).  Replaces the nderiv planes wmode 1 would use. */
    int32_t nderiv;
    double smax;
    /* edge (cells) of the blocks the register-footprint scatters anchor their frame on: 4 (the tile sort's 4 x 4-cell blocks), or 2
     * for the one-plane scatter at W = 14, 15 (16 x 16-cell frame on 4 x 16 lanes; the sort key then carries the 2 x 2 block) */
    int32_t scatter_block;
    int32_t reserved0;
    /* gather kernel: 0 = diagonal-walk form (k_degrid_mp), 1 = row-walk form (k_degrid_rw: single-pass plans without ES-kernel
     * w-planes), 2 = one-plane form (k_degrid_wd; Hessian applies of fused plans run k_hess_wd and launch no gather) */
    int32_t gather_mode;
    int32_t reserved1;
} pfbhip_gridder_info;

int pfbhip_gridder_create(const pfbhip_gridder_params *params, const double *uvw_host /* (nrow,3) */,
                          const double *freq_host /* (nchan) */, const uint8_t *mask_host /* (nrow,nchan) or NULL */,
                          pfbhip_gridder **out);
int pfbhip_gridder_destroy(pfbhip_gridder *g);
int pfbhip_gridder_get_info(const pfbhip_gridder *g, pfbhip_gridder_info *info);

/* w (wavelengths) of each of the nplanes planes. */
int pfbhip_gridder_get_planes(const pfbhip_gridder *g, double *w_host /* [nplanes] */);

/* The bit-exact uv-cell / tile / plane map, for parity tests: per visibility
 * (row-major (nrow,nchan)) first-tap indices iu0, iv0, first plane p0, the
 * Hermitian-fold flag, and `order`, the nactive visibility indices in tile-sorted
 * order.  Any output pointer may be NULL. */
int pfbhip_gridder_get_binmap(pfbhip_gridder *g, int32_t *iu0_host, int32_t *iv0_host, int32_t *p0_host,
                              uint8_t *flip_host, int64_t *order_host);

/* vis2dirty: dirty (nx,ny) = R^H (wgt * mask * vis).  wgt_host may be NULL (ones). */
int pfbhip_gridder_vis2dirty(pfbhip_gridder *g, const double *vis_host /* (nrow,nchan,2) */,
                             const double *wgt_host /* (nrow,nchan) or NULL */, double *dirty_host /* (nx,ny) */);
/* dirty2vis: vis (nrow,nchan) = wgt * mask * R dirty. */
int pfbhip_gridder_dirty2vis(pfbhip_gridder *g, const double *dirty_host, const double *wgt_host,
                             double *vis_host /* (nrow,nchan,2) */);
/* One pre-FFT w-plane of the uv-grid (nu,nv,2), for intermediate parity tests. */
int pfbhip_gridder_grid_plane(pfbhip_gridder *g, const double *vis_host, const double *wgt_host, int64_t plane,
                              double *grid_host);

/*
 * Fused exact Hessian  out = beam * R^H W R (beam * x) / wsum + eta * x
 * (src/pfb_imaging/operators/hessian.py:15-100).  Weights are bound once with
 * set_weights (they are constant across CG iterations, opt/pcg.py:519-538);
 * model visibilities never leave the device.  beam may be NULL; wsum <= 0
 * means "do not normalise"; eta == 0 skips the Tikhonov term.
 */
int pfbhip_gridder_set_weights(pfbhip_gridder *g, const double *wgt_host /* (nrow,nchan) or NULL */);
int pfbhip_gridder_hessian(pfbhip_gridder *g, const double *x_host, const double *beam_host, double eta, double wsum,
                           double *out_host);
int pfbhip_gridder_hessian_dev(pfbhip_gridder *g, const double *x_dev, const double *beam_dev, double eta,
                               double wsum, double *out_dev);
/* The exact residual of one partition with every image resident in HBM: out = acc - R^H W R (beam * model)
 * (src/pfb_imaging/operators/gridder.py:962-1016: dirty2vis of beam * model, vis2dirty with the imaging weights, subtracted
 * from the dirty image; band_worker.py:167-182 calls it per band).  Weights as bound by set_weights; beam may be NULL; out may
 * be acc (chains over the partitions of a band) but not model. */
int pfbhip_gridder_residual_dev(pfbhip_gridder *g, const double *model_dev, const double *beam_dev, const double *acc_dev,
                                double *out_dev);
/* Device-resident single directions (bench / on-device solvers).  vis_sorted_dev
 * holds nactive complex values in the handle's tile-sorted order. */
/* vis2dirty with the image left in HBM (row-sharded single band: the partial images are summed over xGMI before one download) */
int pfbhip_gridder_vis2dirty_dev(pfbhip_gridder *g, const double *vis_host, const double *wgt_host, double *dirty_dev);
int pfbhip_gridder_degrid_dev(pfbhip_gridder *g, const double *dirty_dev, double *vis_sorted_dev);
int pfbhip_gridder_grid_dev(pfbhip_gridder *g, const double *vis_sorted_dev, double *dirty_dev);
/* dirty2vis whose image is already in HBM (the rendered component model of comps2vis, operators/gridder.py:345-365): the
 * degrid and the un-sort of pfbhip_gridder_dirty2vis without the image upload; visibilities in (nrow, nchan) row order. */
int pfbhip_gridder_dirty2vis_dev(pfbhip_gridder *g, const double *dirty_dev, const double *wgt_host /* or NULL */,
                                 double *vis_host /* (nrow,nchan,2) */);

/* ---- one correlation of a device-resident chunk: row-ordered (nrow, nchan) DEVICE arrays in the caller's row order, e.g. a
 * contiguous slice of the correlation-first cube pfbhip_weight_data_dev leaves in HBM.  Nothing is uploaded; every call
 * returns with the plan's stream idle. */
/* vis2dirty (src/pfb_imaging/operators/gridder.py:587-614): pfbhip_gridder_vis2dirty_dev without the upload.  vis_dev complex128,
 * wgt_dev float64 or NULL (unit weights), dirty_dev (nx, ny). */
int pfbhip_gridder_vis2dirty_rows_dev(pfbhip_gridder *g, const double *vis_dev, const double *wgt_dev /* or NULL */,
                                      double *dirty_dev);
/* The PSF (operators/gridder.py:616-655; grid_partition :878-906): vis2dirty of the PSF visibilities for the plan's own centre --
 * ones at the phase centre, else the phase ramp of :617-622 -- formed inside the sort kernel: no (nrow, nchan) complex
 * array exists anywhere.  psf_dev has the plan's image shape. */
int pfbhip_gridder_psf_rows_dev(pfbhip_gridder *g, const double *wgt_dev /* or NULL */, double *psf_dev);
/* The same with the ramp's sign chosen: ramp_sign = +1 is pfbhip_gridder_psf_rows_dev, -1 the conjugate ramp of the snapshot
 * imager (src/pfb_imaging/utils/stokes2im.py:354, :483-486: freqfactor = -2 pi i f / c where operators/gridder.py:618 has
 * +2 pi i).  At the phase centre both are ones. */
int pfbhip_gridder_psf_rows_signed_dev(pfbhip_gridder *g, const double *wgt_dev /* or NULL */, double ramp_sign, double *psf_dev);
/* pfbhip_gridder_set_weights (operators/hessian.py:50-89) from a resident array. */
int pfbhip_gridder_set_weights_dev(pfbhip_gridder *g, const double *wgt_dev /* or NULL */);
/* Un-weighted model visibilities and the residual visibilities (operators/gridder.py:480-507).  minuend_dev NULL: vis = R dirty,
 * 0 on masked samples.  Else vis = minuend - R dirty on unmasked samples and vis = minuend on masked ones, in the one pass
 * that un-sorts; vis_dev may be minuend_dev. */
int pfbhip_gridder_dirty2vis_rows_dev(pfbhip_gridder *g, const double *dirty_dev, const double *minuend_dev /* or NULL */,
                                      double *vis_dev);

/* Per-stage device timing (HIP events on the handle's stream).  Stages:
 * 0 grid (scatter kernel)  1 degrid (gather kernel)  2 fft_rows (plain row-FFT passes: first axis, and the
 * second axis on the rocFFT fallback)  3 pad (B -> A transpose; + pad/w-screen kernel on the fallback)
 * 4 crop (A -> B transpose; + crop/w-screen kernel on the fallback)  5 other (clears, image transposes,
 * scaling)  6 fft_crop (fused second-axis inverse FFT + crop + w-screen)  7 pad_fft (fused pad + w-screen +
 * second-axis forward FFT).
 * ms[s] = accumulated milliseconds, calls[s] = timed regions, since the last reset. */
#define PFBHIP_NSTAGES 8
int pfbhip_gridder_profile(pfbhip_gridder *g, int enable);
int pfbhip_gridder_profile_get(pfbhip_gridder *g, double *ms /* [PFBHIP_NSTAGES] */, int64_t *calls, int reset);

/* ---- FFT (replaces ducc0.fft.r2c / c2r) ---------------------------- */
/* r2c(forward=True, inorm=0) and c2r(forward=False, inorm=2, lastsize) over the last two axes of a
 * (nbatch, n0, n1) real / (nbatch, n0, n1/2+1) complex array
 * (src/pfb_imaging/operators/psf.py:20-32, operators/fft.py:10,39, operators/gridder.py:659,912). */
int pfbhip_r2c_2d(const double *in_host, int64_t nbatch, int64_t n0, int64_t n1, double *out_host);
/* r2c of ifftshift(x) over both axes, EVEN lengths only: fft2d / fft_cube of the reference (operators/fft.py:9-40, PSF -> PSFHAT);
 * the shift is the checkerboard sign (-1)^(k0 + k1) on the spectrum, applied on the device. */
int pfbhip_r2c_2d_centred(const double *in_host, int64_t nbatch, int64_t n0, int64_t n1, double *out_host);
int pfbhip_c2r_2d(const double *in_host, int64_t nbatch, int64_t n0, int64_t n1 /* lastsize */, double *out_host);

/* Hand-written batched row FFT (the second-axis pass of the plane transform), exposed for tests and
 * benchmarks: in-place transform of (nrows, n) complex doubles, n = m 2^a (m in 1,3,5,7,9,15), 1024 <= n <= 16384, or 20480 / 24576 / 32768.
 * ms_out (may be NULL) receives the device time per transform when reps > 1. */
int pfbhip_debug_rowfft(double *data_host, int64_t n, int64_t nrows, int inverse, int reps, double *ms_out);
/* The same transform, once, on a chosen family of the per-length kernel shapes: family 0 is the one above (both components in
 * LDS where they fit), family 1 the one the fused second-axis kernels of the gridder are built on (one component at a time,
 * padded exchanges, one workgroup per CU).  Any other family, or an unsupported n, is an error.  ms_out (may be NULL): device time. */
int pfbhip_debug_rowfft_shape(double *data_host, int64_t n, int64_t nrows, int inverse, int family, double *ms_out);

/* ---- PSF-convolution operator family -------------------------------- */
/*
 * One plan serves psf_convolve_slice/cube/fscube (operators/psf.py:8-96),
 * hessian_psf_slice / hess_direct_slice (operators/hessian.py:103-248),
 * HessPSF.dot (:313-349) and HessianTree.dot (:487-518):
 *     out[b] = post[b] * crop( irfft2( rfft2( pad(pre[b] * x[b]) ) * f(psfhat[b]) ) ) * scale + eta[b] * x[b]
 * with real or complex psfhat resident on the device.
 */
typedef struct pfbhip_psfconv pfbhip_psfconv;
int pfbhip_psfconv_create(int64_t nx, int64_t ny, int64_t nx_psf, int64_t ny_psf, pfbhip_psfconv **out);
int pfbhip_psfconv_destroy(pfbhip_psfconv *p);
/* Bind slot `slot` (0 <= slot < nslots, grown on demand) to a Fourier-domain PSF:
 * is_complex = 0: (nx_psf, ny_psf/2+1) doubles; 1: interleaved complex. */
int pfbhip_psfconv_set_psfhat(pfbhip_psfconv *p, int64_t slot, const double *psfhat_host, int is_complex);
/* Bind slot `slot` to an image-plane multiplier (beam / taper), (nx,ny); NULL unbinds. */
int pfbhip_psfconv_set_beam(pfbhip_psfconv *p, int64_t slot, const double *beam_host);
/*
 * mode 0: multiply by psfhat[psf_slot]
 * mode 1: multiply by (psfhat + shift)          (hess_direct, forward)
 * mode 2: divide   by (psfhat + shift)          (hess_direct, backward)
 * beam_slot < 0: no image-plane multiplier.  accumulate != 0: out += result.
 */
int pfbhip_psfconv_apply(pfbhip_psfconv *p, const double *x_host, int64_t psf_slot, int64_t beam_slot, int mode,
                         double shift, double scale, double eta, int accumulate, double *out_host);
int pfbhip_psfconv_apply_dev(pfbhip_psfconv *p, const double *x_dev, int64_t psf_slot, int64_t beam_slot, int mode,
                             double shift, double scale, double eta, int accumulate, double *out_dev);
/* HessPSF.idot's direct estimate (operators/hessian.py:369-400): mode 2 with the taper in taper_slot, then -- beam_slot >= 0 --
 * x /= beam^2 where x > 0 and beam > min_beam, on the device (the reference divides on the host).  raw_host (may be NULL)
 * receives the estimate before the beam division, out_host after it. */
int pfbhip_psfconv_direct(pfbhip_psfconv *p, const double *x_host, int64_t psf_slot, int64_t taper_slot, double shift,
                          int64_t beam_slot, double min_beam, double *raw_host, double *out_host);
/* Diagnostic: *out = 1 when the plan runs the three-pass row-FFT pipeline (both padded sizes are plain row-FFT lengths), 0 when it
 * runs the rocFFT 2-D r2c / c2r fallback.  Fixed at create time. */
int pfbhip_psfconv_uses_rowfft(const pfbhip_psfconv *p, int *out);

/* Single-precision host arrays: the reference's precision="single" (vis2im / im2vis, operators/gridder.py:58-100:
 * complex64 visibilities, float32 weights and images) with double-precision accumulation (ducc0's
 * double_precision_accumulation=True, the reference's default, core/grid.py:50-52).  Values cross PCIe as float / complex64
 * -- half the bytes of the double entry points, which is what bounds the host-array surface -- and are widened / narrowed on
 * the device; every device buffer and every sum stays double. */
int pfbhip_gridder_vis2dirty_sp(pfbhip_gridder *g, const float *vis_host /* (nrow,nchan,2) */,
                                const float *wgt_host /* (nrow,nchan) or NULL */, float *dirty_host /* (nx,ny) */);
int pfbhip_gridder_dirty2vis_sp(pfbhip_gridder *g, const float *dirty_host, const float *wgt_host, float *vis_host);
int pfbhip_gridder_set_weights_sp(pfbhip_gridder *g, const float *wgt_host);
int pfbhip_gridder_hessian_sp(pfbhip_gridder *g, const float *x_host, const float *beam_host /* or NULL */, double eta,
                              double wsum, float *out_host);

/* ---- on-device conjugate gradients ------------------------------------- */
/*
 * Whole-solve entry points: every CG vector stays in HBM, one host call per solve
 * (replaces the per-iteration host loop of pcg_numba, src/pfb_imaging/opt/pcg.py:88-199,
 * as used by HessTreeRay.cg -> band_worker.py:124-140 and pcg_dds, opt/pcg.py:519-540).
 * Same stopping rule: eps = ||x - xp|| / ||x|| <= tol and k >= minit, or k == maxit, or 5 stalls.
 * x_host holds x0 on entry when has_x0 != 0 (else zeros are used) and the solution on exit.
 */
typedef struct pfbhip_cg_info {
    int32_t iters;
    int32_t status; /* 0 converged, 1 maxit, 2 stalled, 3 zero initial residual */
    double eps;     /* last ||x - xp|| / ||x|| */
    double phi;     /* (r.r) / (r0.r0) */
} pfbhip_cg_info;
/* A = (scale) * sum_k beam[beam_slots[k]] * PSF[psf_slots[k]] (*) (beam * .) + eta * I   (HessianTree / HessPSF band) */
int pfbhip_psfconv_cg(pfbhip_psfconv *p, int64_t nparts, const int64_t *psf_slots, const int64_t *beam_slots,
                      double scale, double eta, const double *rhs_host, double *x_host, int has_x0, double tol,
                      int maxit, int minit, pfbhip_cg_info *info);
/* A = beam * R^H W R (beam * .) / wsum + eta * I   (exact Hessian, weights bound by set_weights) */
int pfbhip_gridder_cg(pfbhip_gridder *g, const double *beam_host, double eta, double wsum, const double *rhs_host,
                      double *x_host, int has_x0, double tol, int maxit, int minit, pfbhip_cg_info *info);
/* The same solve with rhs / x / beam resident in HBM (bench, band workers that keep their images on the device). */
int pfbhip_gridder_cg_dev(pfbhip_gridder *g, const double *beam_dev, double eta, double wsum, const double *rhs_dev,
                          double *x_dev, int has_x0, double tol, int maxit, int minit, pfbhip_cg_info *info);

/* ---- power method on the device (spectral norm of a Hessian) ------------
 * Replaces power_method / power_method_numba (src/pfb_imaging/opt/power_method.py:40-148) as called on
 * precond.dot / hess.dot for `hess_norm` (core/sara.py:200-209, deconv/pfb.py:118-126) -- and the per-actor
 * form power_method_dist (:178-208) when a communicator is passed.  b_host: start vector in (any non-zero norm; the
 * reference draws randn), normalised last iterate out.  Stops when |beta - beta_prev| / beta_prev <= tol or after
 * maxit iterations (status 1). */
typedef struct pfbhip_pm_info {
    int32_t iters;
    int32_t status; /* 0 converged, 1 maxit reached */
    double eps;
    double beta; /* Rayleigh quotient (bp . A bp) / (bp . bp) of the last iteration */
} pfbhip_pm_info;
typedef struct pfbhip_comm pfbhip_comm; /* RCCL communicator, see below */
/* A = blockdiag_b( scale[b] sum_p beam_p (PSF_p * (beam_p .)) + eta[b] I ) on a cube (nband, nx, ny); band b owns
 * nparts[b] consecutive entries of psf_slots / beam_slots of its plan pcs[b] (as in pfbhip_primal_dual).
 * comm != NULL: the arrays hold this rank's LOCAL bands, the three dots are all-reduced. */
int pfbhip_psfconv_power_method(pfbhip_psfconv *const *pcs, int64_t nband, const int64_t *nparts, const int64_t *psf_slots,
                                const int64_t *beam_slots, const double *scale, const double *eta, double *b_host, double tol,
                                int maxit, pfbhip_comm *comm, pfbhip_pm_info *info);
/* A = beam * R^H W R (beam * .) / wsum + eta * I (exact Hessian, weights bound by set_weights), image (nx, ny) */
int pfbhip_gridder_power_method(pfbhip_gridder *g, const double *beam_host, double eta, double wsum, double *b_host,
                                double tol, int maxit, pfbhip_pm_info *info);

/* ---- uv-cell counts / Briggs weights (utils/weighting.py:81-208) ------ */
/* cell index (u_idx*ny+v_idx, -1 if masked / out of bounds): the bit-exact index map. */
int pfbhip_uvcell_index(const double *uvw_host, const double *freq_host, const uint8_t *mask_host, int64_t nrow,
                        int64_t nchan, int64_t nx, int64_t ny, double cell_x, double cell_y, double usign,
                        double vsign, int64_t *cell_host);
/* _compute_counts: counts (ncorr,nx,ny) += wgt (ncorr,nrow,nchan) scattered by the index map. */
int pfbhip_compute_counts(const double *uvw_host, const double *freq_host, const uint8_t *mask_host,
                          const double *wgt_host, int64_t ncorr, int64_t nrow, int64_t nchan, int64_t nx, int64_t ny,
                          double cell_x, double cell_y, double usign, double vsign, double *counts_host);
/* gather-divide half of counts_to_weights: wgt /= counts[cell] where counts > 0. */
int pfbhip_counts_divide(const double *uvw_host, const double *freq_host, const uint8_t *mask_host,
                         const double *counts_host, int64_t ncorr, int64_t nrow, int64_t nchan, int64_t nx,
                         int64_t ny, double cell_x, double cell_y, double usign, double vsign, double *wgt_host);

/* box_sum_counts (utils/weighting.py:229-254): (2 s + 1)^2 box sum with zero padding, per correlation plane. */
int pfbhip_box_sum_counts(const double *counts_host, int64_t ncorr, int64_t nx, int64_t ny, int64_t npix_super,
                          double *out_host);
/* filter_extreme_counts (utils/weighting.py:212-226): positive counts below median(positive)/level are
 * raised to that value, in place; the median is returned through median_out (may be NULL). */
int pfbhip_filter_extreme_counts(double *counts_host, int64_t n, double level, double *median_out);
/* The imaging-weight chain of image_data_products (operators/gridder.py:534-576) as ONE device pipeline:
 * _compute_counts on the (nx, ny) padded uv-grid -> filter_extreme_counts(level; <= 0 skips) -> box_sum_counts(npix_super)
 * -> Briggs scaling counts * (5 * 10^-robust)^2 * sum(c)/sum(c^2) + 1 (robust > -2) -> weight /= counts[cell].
 * wgt_host (ncorr, nrow, nchan) is updated in place (left untouched when every count is zero); the final counts
 * come back through counts_out_host (ncorr, nx, ny) when it is not NULL.  One upload of uvw / freq / mask / weights. */
int pfbhip_imaging_weights(const double *uvw_host, const double *freq_host, const uint8_t *mask_host, double *wgt_host,
                           int64_t ncorr, int64_t nrow, int64_t nchan, int64_t nx, int64_t ny, double cell_x, double cell_y,
                           double usign, double vsign, double robust, double filter_level, int64_t npix_super,
                           double *counts_out_host);

/* ---- a device-resident visibility chunk (csrc/vischunk.hip): wgt_dev (ncorr, nvis) float64, mask_dev (nvis) uint8, nvis = nrow *
 * nchan.  Reductions are two-stage (block partials, one final block, fixed trees, no float atomics): bit-reproducible. */
/* WSUM of operators/gridder.py:584: wsum_host[c] = wgt[c, mask != 0].sum(). */
int pfbhip_chunk_wsum_dev(const double *wgt_dev, const uint8_t *mask_dev, int64_t ncorr, int64_t nvis, double *wsum_host);
/* The l2 reweighting of operators/gridder.py:509-532 on resident residual visibilities resvis_dev (ncorr, nvis) complex128: per
 * correlation ressq = wgtp |r|^2 (wgtp_dev (ncorr, nvis), or the scalar when it is NULL), ovar_c = sum_{mask > 0} ressq /
 * sum(mask), wgt *= (dof + 2) / (dof + ressq / ovar_c) on every sample.  ovar_host (ncorr, may be NULL) receives ovar.  When
 * any ovar_c is zero (or the mask is empty) the call fails with PFBHIP_ERR_INVALID and the weights are untouched. */
int pfbhip_chunk_l2_reweight_dev(const double *resvis_dev, const double *wgtp_dev /* or NULL */, double wgtp_scalar,
                                 const uint8_t *mask_dev, double *wgt_dev, int64_t ncorr, int64_t nvis, double dof,
                                 double *ovar_host);
/* pfbhip_imaging_weights (operators/gridder.py:534-576) with the mask and the weights already resident: the same pipeline,
 * wgt_dev updated in place (untouched when every count is zero); uvw and freq come from the host. */
int pfbhip_imaging_weights_dev(const double *uvw_host, const double *freq_host, const uint8_t *mask_dev, double *wgt_dev,
                               int64_t ncorr, int64_t nrow, int64_t nchan, int64_t nx, int64_t ny, double cell_x, double cell_y,
                               double usign, double vsign, double robust, double filter_level, int64_t npix_super,
                               double *counts_out_host /* or NULL */);
/* Weighted averaging of a resident chunk over channel bins of fixed width and caller-supplied row bins (csrc/chunkavg.hip):
 * steps 2 to 4 of utils/stokes2vis.py:196-286 (drop flagged rows, time_and_channel, bda with min_nchan = nchan) in one
 * out-of-place pass.  vis_dev (ncorr, nrow, nchan) complex128, wgt_dev the same shape float64, mask_dev (nrow, nchan) uint8.
 * Output channel q covers input channels [q chan_bin, min((q + 1) chan_bin, nchan)), nchan_out = ceil(nchan / chan_bin).
 * Row bins are a CSR on the HOST: row_start_host (nrow_out + 1) and members_host (nkept) input rows, strictly ascending inside
 * a bin; both NULL: the identity (nrow_out == nkept == nrow).  With K the unmasked input samples of output sample (R, q):
 * wgt_out = sum_K wgt, vis_out = sum_K wgt vis / wgt_out, mask_out = (K not empty); an empty K or wgt_out == 0 gives exact
 * zeros, a K of one sample its visibility unchanged.  No atomics: bit-identical from call to call.  The outputs
 * (ncorr, nrow_out, nchan_out) / (nrow_out, nchan_out) are the caller's and may not overlap the inputs or each other.
 * Everything is validated on the host before anything is launched (PFBHIP_ERR_INVALID): ncorr in [1, 65535], chan_bin >= 1,
 * row_start[0] == 0, non-decreasing, row_start[nrow_out] == nkept, every member in [0, nrow), pointers non-NULL unless
 * their arrays are empty. */
int pfbhip_chunk_average_dev(const double *vis_dev, const double *wgt_dev, const uint8_t *mask_dev, int64_t ncorr, int64_t nrow,
                             int64_t nchan, int64_t chan_bin, const int64_t *row_start_host /* or NULL */,
                             const int64_t *members_host /* or NULL */, int64_t nkept, int64_t nrow_out, double *vis_out_dev,
                             double *wgt_out_dev, uint8_t *mask_out_dev);

/* ---- one `pfb hci` snapshot on a resident chunk (csrc/snapshot.hip): the array steps of
 * src/pfb_imaging/utils/stokes2im.py::stokes_image around its two vis2dirty calls per Stokes.  Every entry validates first and
 * returns with its stream idle; the sums are two-stage like the chunk's (bit-identical from call to call). */
/* Rephasing and model subtraction, stokes2im.py:364-373 and :466-468, one in-place pass over vis_dev (ncorr, nrow * nchan)
 * complex128:  vis = (vis p - model p) * mask,  p = exp(-2 pi i freq[chan] / c * w_diff[row]).  w_diff_dev (nrow) may be NULL
 * (p = 1), model_dev (ncorr, nrow * nchan) may be NULL; the mask (uint8) applies only with a model, as in the reference
 * (:467-468), and masked samples are then written as exact zeros.  The phase is formed in cycles, reduced to a fraction of
 * a turn, then sincospi.  The reference rephases the raw correlations before weight_data (:371, :447); weight_data's Jones
 * correction and Stokes combination are linear in the data and p is one complex scalar per (row, channel), so it commutes
 * with them and rephasing the Stokes chunk is the same operation. */
int pfbhip_chunk_rephase_residual_dev(double *vis_dev, const double *model_dev /* or NULL */, const uint8_t *mask_dev,
                                      const double *w_diff_dev /* or NULL */, const double *freq_host, int64_t ncorr, int64_t nrow,
                                      int64_t nchan);
/* The l2 reweighting in stokes_image's form, stokes2im.py:470-481: ressq = |r|^2 * mask (a 0 / 1 mask; the mask broadcast
 * over the correlations, the evident intent of :472), ovar = sum over EVERY correlation and sample of ressq / sum(mask) -- one
 * joint variance -- and wgt = (dof + 1) / (dof + ressq / ovar) / ovar on every sample: the weights are replaced, not
 * multiplied; a masked sample gets (dof + 1) / dof / ovar, so dof must be positive (and finite).  ovar_host (may be NULL) receives ovar.  A zero variance (the
 * reference's ValueError, :479) or an empty mask (:481 sets weight = None and fails later) is PFBHIP_ERR_INVALID before any
 * weight is written. */
int pfbhip_chunk_l2_reweight_joint_dev(const double *resvis_dev, const uint8_t *mask_dev, double *wgt_dev, int64_t ncorr, int64_t nvis,
                                       double dof, double *ovar_host);
/* The finish, stokes2im.py:684-692, :707-708, :731-737, :750-753, on the Stokes planes residual_dev (ns, nx, ny) and psf_dev
 * (ns, nxp, nyp) float64 in HBM.  Per Stokes c with wsum_host[c] > 0: psf_max = max(psf[c]) (exact); psf[c] /= psf_max and
 * residual[c] /= psf_max in place; rms[c] = np.std(residual[c]), two-pass; with pbeam_dev (ns, nx, ny; may be NULL)
 * residual[c] *= pbeam / (pbeam^2 + eta) in place and beam_weight = pbeam^2 + eta.  A Stokes with wsum <= 0 gets zero residual,
 * PSF, cube and psf planes (whatever its beam holds), psf_max 0 and rms 0; its beam_weight plane is pbeam^2 + eta all the
 * same, as the reference forms beam_weight from the beam alone (:751).  Host outputs, TRANSPOSED, float32 (out_f64 = 0) or float64: cube_host (ns, ny, nx), psf_host (ns, nyp,
 * nxp; may be NULL), beam_weight_host (ns, ny, nx; may be NULL, needs pbeam_dev); psf_max_host[ns], rms_host[ns].  Unlike the
 * reference, whose normalisation loop is nested inside the per-Stokes loop (:686), each Stokes is normalised once.
 * device_ms (may be NULL) receives the device time of the kernels alone, without the downloads. */
int pfbhip_snapshot_finish_dev(double *residual_dev, double *psf_dev, const double *pbeam_dev /* or NULL */, const double *wsum_host,
                               int64_t ns, int64_t nx, int64_t ny, int64_t nxp, int64_t nyp, double eta, int out_f64, void *cube_host,
                               void *psf_host /* or NULL */, void *beam_weight_host /* or NULL */, double *psf_max_host,
                               double *rms_host, double *device_ms /* or NULL */);

/* ---- wavelet dictionary Psi and the l21 / positivity proxes ---------------- */
/*
 * One band's dictionary: replaces PsiBandNocopyt (src/pfb_imaging/operators/psi.py:415-535; multi-level 2-D
 * DWT of wavelets/wavelets.py:216-343 on the 1-D kernels of wavelets/convolutions.py:5-327, zero-padding
 * mode, packed x-first layout of psi.py:23-142).  bases[i]: 0 = "self" (identity), N = "dbN" (1..8).
 * x is (nx, ny), alpha is (nbasis, nxmax, nymax) with (nxmax, nymax) from pfbhip_psi_shape; nx, ny even.
 * dot = image -> coefficients (every element of alpha is written), hdot = coefficients -> image, summed
 * over the bases.  transposed != 0 on the host entries: alpha is (nbasis, nymax, nxmax), the layout of the
 * reference's older Psi (psi.py:218-345).
 */
typedef struct pfbhip_psi pfbhip_psi;
int pfbhip_psi_create(int64_t nx, int64_t ny, int32_t nbasis, const int32_t *bases, int32_t nlevel, pfbhip_psi **out);
int pfbhip_psi_destroy(pfbhip_psi *p);
int pfbhip_psi_shape(const pfbhip_psi *p, int64_t *nxmax, int64_t *nymax);
int pfbhip_psi_dot(pfbhip_psi *p, const double *x_host, double *alpha_host, int transposed);
int pfbhip_psi_hdot(pfbhip_psi *p, const double *alpha_host, double *x_host, int transposed);
int pfbhip_psi_dot_dev(pfbhip_psi *p, const double *x_dev, double *alpha_dev);
int pfbhip_psi_hdot_dev(pfbhip_psi *p, const double *alpha_dev, double *x_dev);

/* dual_update_numba_fast (src/pfb_imaging/prox/prox_21m.py:105-135): v <- vtilde min(1, lam w / |sum_band vtilde|),
 * vtilde = vp + sigma v, arrays (nband, n), weight (n), in place on v.  With bands spread over ranks the
 * update is two device phases around one all-reduce of the band sum (pfbhip_comm_allreduce_sum):
 * vtilde_sum (v <- vtilde, sum over the LOCAL bands) and scale (given the sum over ALL bands). */
int pfbhip_dual_update(const double *vp_host, double *v_host, int64_t nband, int64_t n, double lam, double sigma,
                       const double *weight_host);
int pfbhip_l21_vtilde_sum_dev(const double *vp_dev, double *v_dev, int64_t nband, int64_t n, double sigma, double *sum_dev);
int pfbhip_l21_scale_dev(double *v_dev, int64_t nband, int64_t n, double lam, const double *weight_dev, const double *sum_dev);
/* prox_21m (prox_21m.py:5-26): out = v max(|s| - sigma w, 0) / |s|, s = band sum; weight may be NULL (= 1). */
int pfbhip_prox_21m(const double *v_host, int64_t nband, int64_t n, double sigma, const double *weight_host, double *out_host);
/* positivity (prox/positivity.py:12-33): mode 1 clamps negatives, mode 2 zeroes a pixel in all bands where any
 * band is <= 0; x is (nband, n), in place. */
int pfbhip_positivity(double *x_host, int64_t nband, int64_t n, int mode);
int pfbhip_positivity_dev(double *x_dev, int64_t nband, int64_t n, int mode);

/* Primal-dual backward step with every cube resident on the device: PrimalDual.solve
 * (src/pfb_imaging/opt/primal_dual.py:406-448) with the l21 regulariser over `psi` (prox/l21.py:15-50) and
 * grad(x) = -H (xtilde - x) / gamma (deconv/pfb.py:158-161), H_b(x) = scale[b] sum_p beam_p (PSF_p * (beam_p x)) +
 * eta[b] x from the slots of band b's plan pcs[b] (one plan for all bands -- HessPSF -- or one per band --
 * HessTreeRay; band b owns nparts[b] consecutive entries of psf_slots / beam_slots, as in pfbhip_psfconv_cg).  x (nband, nx, ny): initial iterate in, solution out; v (nband, nbasis, nxmax, nymax):
 * warm-started dual in / out; weight (nbasis, nxmax, nymax); positivity 0 | 1 | 2 (prox/positivity.py).
 * Stops when ||x - xp|| / ||x|| < tol or after maxit iterations; info->iters is the last loop index.
 * comm == NULL: all nband bands are on this device.  comm != NULL (one process per GPU, every rank calls
 * collectively): the arrays hold this rank's nband LOCAL bands; the band sum of the dual update, the
 * "any band <= 0" test of positivity mode 2 and the convergence norms are completed with all-reduces. */
#define PFBHIP_PD_NSTAGES 5
typedef struct pfbhip_pd_info {
    int32_t iters;
    int32_t status; /* 0 converged, 1 maxit reached */
    double eps;
    double loop_ms; /* wall time of the iteration loop alone (cubes resident in HBM: uploads / downloads excluded) */
    /* device time (HIP events on the loop's stream) and number of bracketed launches per stage, summed over the iterations of
     * runs with maxit <= 64 (zeros otherwise): 0 Psi^H analysis of all local bands, 1 l21 dual update, 2 Psi synthesis (one
     * band per launch), 3 PSF-approximate Hessian (one partition apply per launch), 4 primal step + positivity + norms */
    double stage_ms[PFBHIP_PD_NSTAGES];
    int64_t stage_calls[PFBHIP_PD_NSTAGES];
} pfbhip_pd_info;
int pfbhip_primal_dual(pfbhip_psi *psi, pfbhip_psfconv *const *pcs /* [nband] */, int64_t nband, const int64_t *nparts, const int64_t *psf_slots,
                       const int64_t *beam_slots, const double *scale, const double *eta, const double *xtilde_host, double gamma,
                       double *x_host, double *v_host, const double *weight_host, double lam, double sigma, double tau,
                       int positivity, double tol, int maxit, pfbhip_comm *comm, pfbhip_pd_info *info);

/* The same solve as a resumable handle, for PrimalDual.solve with an on_converge callback (primal_dual.py:430-435; the
 * callback the reference's PFBSolver installs is ReweightOnConverge, deconv/pfb.py:14-54, 132-136).  pfbhip_pd_create takes
 * the description of pfbhip_primal_dual (no communicator: all nband bands are on this device), uploads x, v, xtilde and the
 * weight once (weight_host == NULL: the caller sets it before the first run) and keeps x, xp, v, vp, the extrapolated dual, the weight and the loop index in HBM.  pfbhip_pd_run iterates
 * from where the previous run stopped until eps < tol (status 0, a convergence event) or the loop index reaches maxit - 1
 * (status 1) and writes x only to x_host; a run after an event continues as the reference's loop does when on_converge
 * returns False: xp <- x, vp <- v, the index goes on, maxit bounds the total.  Between runs the caller may replace the
 * weight from host (pfbhip_pd_set_weight) or device memory (pfbhip_pd_set_weight_dev: a copy, the handle keeps its own
 * buffer) and read the iterate in place (pfbhip_pd_iterate_dev: valid until the next run or the destroy).
 * pfbhip_pd_get_dual downloads the dual of the last iteration (PrimalDual._v, the warm start of the next solve).  It is the
 * same loop as pfbhip_primal_dual with comm == NULL: the iterates are identical.  Psi's and the
 * plans' streams are switched to the first plan's for the duration of each run; the handle must not outlive them. */
typedef struct pfbhip_pd pfbhip_pd;
typedef struct pfbhip_pd_traffic {
    int64_t events;     /* runs that ended with eps < tol */
    int64_t h2d_bytes;  /* host-to-device bytes after the create: the weights of pfbhip_pd_set_weight */
    int64_t d2h_bytes;  /* device-to-host bytes: the iterate of every run and the dual of pfbhip_pd_get_dual */
    int64_t norm_bytes; /* the per-iteration block of norm partials (3 x 1024 doubles), not part of d2h_bytes */
} pfbhip_pd_traffic;
int pfbhip_pd_create(pfbhip_psi *psi, pfbhip_psfconv *const *pcs /* [nband] */, int64_t nband, const int64_t *nparts,
                     const int64_t *psf_slots, const int64_t *beam_slots, const double *scale, const double *eta,
                     const double *xtilde_host, double gamma, const double *x_host, const double *v_host, const double *weight_host,
                     double sigma, double tau, int positivity, pfbhip_pd **out);
int pfbhip_pd_run(pfbhip_pd *h, double lam, double tol, int maxit, double *x_host, pfbhip_pd_info *info);
int pfbhip_pd_set_weight(pfbhip_pd *h, const double *weight_host);
int pfbhip_pd_set_weight_dev(pfbhip_pd *h, const double *weight_dev);
int pfbhip_pd_iterate_dev(pfbhip_pd *h, const double **x_dev);
int pfbhip_pd_get_dual(pfbhip_pd *h, double *v_host);
int pfbhip_pd_get_traffic(const pfbhip_pd *h, pfbhip_pd_traffic *out);
int pfbhip_pd_destroy(pfbhip_pd *h);

/* l1 reweighting of the l21 regulariser on the device: replaces the host arithmetic of L21.update_weights /
 * init_reweighting (src/pfb_imaging/prox/l21.py:52-88) and l1reweight_func (utils/misc.py:742-755).
 * pfbhip_l21_reweight_dev: x_dev (nband, nx, ny) is analysed band by band into scratch_dev (nband, nbasis, nxmax, nymax),
 * then ONE pass adds the bands of each coefficient in band order (np.sum(axis=0): bit-identical) and writes
 * weight_dev (nbasis, nxmax, nymax) = (1 + rmsfactor) / (1 + |s|^alpha / rms[basis]^alpha); alpha == 2 and alpha == 4 are
 * products.  Cells of the padded frame that hold no coefficient are zero and get 1 + rmsfactor.  rms is a HOST array.
 * pfbhip_l21_rms_dev: per basis, the number of NONZERO band sums of Psi^H update and their population standard deviation
 * (l21.py:56-65; two passes, f64 per-workgroup partials added on the host in a fixed order); a basis with no nonzero
 * entry reports count 0 and rms 0 (the caller keeps 1, l21.py:58).  scratch_dev is overwritten.
 * pfbhip_l21_reweight / pfbhip_l21_rms: the host-array forms ((nbasis, nxmax, nymax) layout; bandsum_host, may be NULL,
 * receives the band sum).  All run on the dictionary's stream and return when the result is complete. */
int pfbhip_l21_reweight_dev(pfbhip_psi *psi, const double *x_dev, int64_t nband, const double *rms /* [nbasis], host */,
                            double rmsfactor, double alpha, double *scratch_dev, double *weight_dev);
int pfbhip_l21_rms_dev(pfbhip_psi *psi, const double *update_dev, int64_t nband, double *scratch_dev,
                       double *rms_out /* [nbasis], host */, int64_t *count_out /* [nbasis], host */);
int pfbhip_l21_reweight(pfbhip_psi *psi, const double *x_host, int64_t nband, const double *rms, double rmsfactor, double alpha,
                        double *weight_host, double *bandsum_host);
int pfbhip_l21_rms(pfbhip_psi *psi, const double *update_host, int64_t nband, double *rms_out, int64_t *count_out);

/* ---- Hogbom and Clark CLEAN (the kclean minor cycle) ------------------- */
/*
 * deconv/hogbom.py:9-63 and deconv/clark.py:11-143 of pfb-imaging with every cube resident in HBM (clean.hip; the semantics,
 * quirks included, are listed in DESIGN.md "Device-resident CLEAN").  A plan holds psf (nband, nx_psf, ny_psf) and, for Clark,
 * psfhat (nband, nx_psf, ny_psf / 2 + 1) complex (NULL: Hogbom only).  Cubes are C-ordered float64 (nband, nx, ny); mask (nx, ny).
 * model_host receives the model, residual_host (may be NULL) the final residual.  nband <= 64.
 */
typedef struct pfbhip_clean pfbhip_clean;
typedef struct pfbhip_clean_info {
    int32_t iters;         /* Hogbom: iterations; Clark: major iterations */
    int32_t status;        /* 1 when iters >= maxit, else 0 */
    int64_t minor_iters;   /* Hogbom: iterations; Clark: sub-minor iterations over all major cycles */
    int64_t idle_launches; /* step launches enqueued after the loop had stopped (batched host control) */
    int64_t nsub_lds;      /* Clark sub-minor loops run by the one-workgroup LDS kernel */
    int64_t nsub_grid;     /* ... and by the two-kernel grid path */
    double rmax;           /* last peak residual */
    double loop_ms;        /* wall time of the loop (uploads / downloads excluded) */
    double conv_ms, search_ms, compact_ms, sub_lds_ms, sub_grid_ms; /* Clark: device time per phase (events), summed */
} pfbhip_clean_info;
int pfbhip_clean_create(int64_t nband, int64_t nx, int64_t ny, int64_t nx_psf, int64_t ny_psf, const double *psf_host,
                        const double *psfhat_host, pfbhip_clean **out);
int pfbhip_clean_destroy(pfbhip_clean *c);
int pfbhip_clean_hogbom(pfbhip_clean *c, const double *dirty_host, double threshold, double gamma, double pf, int64_t maxit,
                        double *model_host, double *residual_host, pfbhip_clean_info *info);
int pfbhip_clean_clark(pfbhip_clean *c, const double *dirty_host, const double *wsums, const double *mask_host, double threshold,
                       double gamma, double pf, int64_t maxit, double subpf, int64_t submaxit, double *model_host,
                       double *residual_host, pfbhip_clean_info *info);

/* ---- forward-backward (ISTA / FISTA) backward step ----------------------- */
/* ForwardBackward.solve (src/pfb_imaging/opt/forward_backward.py:95-133; replaces its host loop over
 * _apply_prox :83-93) with every cube resident on the device (fb.hip).  Per iteration: the forward step
 * xg = y + (step / g) H (xtilde - y) with H as in pfbhip_primal_dual (band b: nparts[b] consecutive slots of
 * its plan pcs[b], scale[b], eta[b]); the tight-frame prox x = xg + Psi(prox(Psi^H xg) - Psi^H xg) / nu with
 * the l21 (reg_kind 0, prox/l21.py) or l1 (reg_kind 1, prox/l1.py) prox at threshold step * lam * weight;
 * positivity 0 | 1 | 2; eps = ||x - xp|| / ||x|| (1 if x == 0); FISTA momentum when acceleration != 0.
 * psi == NULL is IdentityPsi.  x0 / xtilde (nband, nx, ny); weight (nbasis, nxmax, nymax) in the PsiNocopyt
 * layout ((nx, ny) for the identity).  weight_host == NULL: the caller sets the weight before the first
 * run.  All bands are on this device.
 *
 * The handle keeps the iterate, momentum and iteration count between runs: pfbhip_fb_run iterates from where
 * the previous run stopped until eps < tol (status 0, a convergence event) or the loop index reaches
 * maxit - 1 (status 1), then writes x to x_host.  The caller may replace the weight with pfbhip_fb_set_weight
 * and run again (the on_converge protocol of forward_backward.py:111-113).  Psi's and the plans' streams are
 * switched to the first plan's for the duration of each run; the handle must not outlive them. */
#define PFBHIP_FB_NSTAGES 5
typedef struct pfbhip_fb pfbhip_fb;
typedef struct pfbhip_fb_info {
    int32_t iters;  /* loop index of the last iteration run */
    int32_t status; /* 0 converged, 1 maxit reached */
    double eps;
    double loop_ms; /* wall time of the iteration loops of all runs of the handle (uploads / downloads excluded) */
    int64_t events; /* runs that ended with eps < tol */
    /* device time (HIP events) and bracketed launches per stage, summed over the iterations of runs with maxit <= 64:
     * 0 forward Hessian (one partition apply per launch), 1 Psi^H analysis, 2 shrink, 3 Psi synthesis, 4 step + norms */
    double stage_ms[PFBHIP_FB_NSTAGES];
    int64_t stage_calls[PFBHIP_FB_NSTAGES];
} pfbhip_fb_info;
int pfbhip_fb_create(pfbhip_psi *psi /* NULL: identity */, pfbhip_psfconv *const *pcs /* [nband] */, int64_t nband,
                     const int64_t *nparts, const int64_t *psf_slots, const int64_t *beam_slots, const double *scale,
                     const double *eta, const double *xtilde_host, double g, const double *x0_host, const double *weight_host,
                     int reg_kind, double nu, double step, int positivity, int acceleration, pfbhip_fb **out);
int pfbhip_fb_run(pfbhip_fb *h, double lam, double tol, int maxit, double *x_host, pfbhip_fb_info *info);
int pfbhip_fb_set_weight(pfbhip_fb *h, const double *weight_host);
/* Between runs: the weight from device memory (a copy; forward_backward.py:111-113 with the weights of
 * pfbhip_l21_reweight_dev) and the iterate in place (valid until the next run or the destroy). */
int pfbhip_fb_set_weight_dev(pfbhip_fb *h, const double *weight_dev);
int pfbhip_fb_iterate_dev(pfbhip_fb *h, const double **x_dev);
int pfbhip_fb_destroy(pfbhip_fb *h);

/* ---- component models: fit, render, regrid ------------------------------ */
/*
 * The component model of src/pfb_imaging/utils/modelspec.py on the device (comps.hip; DESIGN.md "Component models on the
 * device").  A handle holds the image geometry, the pixel locations x_index / y_index (int64, ncomps) and the coefficients
 * (nparam, ncomps) in HBM.  Component c is the c-th pixel in ascending flat index x * ny + y (np.where's order).
 *
 * pfbhip_comps_create: from host arrays (the `coefficients`, `location_x`, `location_y` of a model dataset as
 *   operators/gridder.py:318-320 reads them).  Locations must lie inside the image and be distinct.
 * pfbhip_comps_fit: modelspec.py:54-59 and :130-135 -- mask = any over the ns = ntime * nband planes of cube (ns, nx, ny)
 *   != 0, compaction of the set pixels in np.where's order, coeffs[k, c] = sum_s A[k, s] * cube[s, pix_c] with
 *   A = solve(hess_coeffs, xfit^T wgt) (nparam, ns) formed by the caller.  Exactly one of cube_host / cube_dev is non-NULL.
 *   *ncomps_out receives the number of components; pfbhip_comps_get downloads locations and coefficients (any pointer may
 *   be NULL), pfbhip_comps_shape the sizes.
 * pfbhip_comps_set_region: uploads a region mask (nx, ny) uint8 once per handle (NULL unbinds it).
 * pfbhip_comps_render / _render_dev: modelspec.py:227-238, :266-275 and operators/gridder.py:345-348 --
 *   image = 0; image[x_index, y_index] = sum_k basis[k] * coeffs[k] (k ascending); with use_region != 0,
 *   np.where(region_mask, image, 0).  Every pixel of the target is written: it need not be zero beforehand.
 * pfbhip_comps_regrid / _regrid_dev: modelspec.py:277-332 -- bilinear interpolation of an image on the grid
 *   (nxi, nyi, cellxi, cellyi, x0i, y0i), zero-extended by the reference's pad widths without forming a padded copy, at the
 *   points of (nxo, nyo, cellxo, cellyo, x0o, y0o), times cellxo * cellyo / (cellxi * cellyi).  When the reference's own test
 *   (:321-326) finds nothing to interpolate the (padded) input is returned as it stands, without the area ratio;
 *   *interpolated (may be NULL) tells which.  Output points outside the padded grid are an error (bounds_error=True).
 */
typedef struct pfbhip_comps pfbhip_comps;
int pfbhip_comps_create(int64_t nx, int64_t ny, int64_t ncomps, int32_t nparam, const int64_t *x_index_host,
                        const int64_t *y_index_host, const double *coeffs_host /* (nparam, ncomps) */, pfbhip_comps **out);
int pfbhip_comps_destroy(pfbhip_comps *h);
int pfbhip_comps_fit(const double *cube_host, const double *cube_dev, int64_t ns, int64_t nx, int64_t ny,
                     const double *A_host /* (nparam, ns) */, int32_t nparam, pfbhip_comps **out, int64_t *ncomps_out);
int pfbhip_comps_shape(const pfbhip_comps *h, int64_t *nx, int64_t *ny, int64_t *ncomps, int32_t *nparam);
int pfbhip_comps_get(pfbhip_comps *h, int64_t *x_index_host, int64_t *y_index_host, double *coeffs_host);
int pfbhip_comps_set_region(pfbhip_comps *h, const uint8_t *region_host /* (nx, ny) or NULL */);
int pfbhip_comps_render(pfbhip_comps *h, const double *basis_host /* [nparam] */, int use_region, double *image_host);
int pfbhip_comps_render_dev(pfbhip_comps *h, const double *basis_host /* [nparam] */, int use_region, double *image_dev);
int pfbhip_comps_regrid(const double *in_host, int64_t nxi, int64_t nyi, double cellxi, double cellyi, double x0i, double y0i,
                        int64_t nxo, int64_t nyo, double cellxo, double cellyo, double x0o, double y0o, double *out_host,
                        int *interpolated);
int pfbhip_comps_regrid_dev(const double *in_dev, int64_t nxi, int64_t nyi, double cellxi, double cellyi, double x0i, double y0i,
                            int64_t nxo, int64_t nyo, double cellxo, double cellyo, double x0o, double y0o, double *out_dev,
                            int *interpolated);

/* ---- direct DFT of point components ---------------------------------------- */
/*
 * The exact measurement equation summed source by source (dft.hip; DESIGN.md "Direct DFT of point components"): the
 * definition the gridder approximates (tests/test_hessian_approx.py:44-67 of the reference, its explicit_wdegridder), the
 * transient injection of src/pfb_imaging/utils/stokes2im.py:491-558, and the degrid of operators/gridder.py:345-351 for a
 * model of isolated pixels.  No image, no plan, no FFT, no epsilon.
 *
 * pfbhip_dft_create: a handle keeps uvw (nrow, 3) [m], freq (nchan) [Hz] and an optional mask (nrow, nchan) uint8 in HBM.
 * pfbhip_dft_conv: the caller's conventions.  su, sv, sw multiply u, v, w (the gridder's flips: -1 when flipped); sgn is the
 *   sign of the exponent (-1: the gridder's dirty2vis, stokes2im.py:354 freqfactor); do_wgridding = 0 sets n - 1 to 0;
 *   divide_by_n divides every source by N = n; accumulate (predict only) adds into vis and leaves masked samples
 *   untouched instead of writing them as 0.  The call works on the channels [chan0, chan0 + nchan) of the handle
 *   (nchan = 0: all of them); vis, wgt and chanf then have that many columns.
 * pfbhip_dft_predict / _dev: for every unmasked (r, c)
 *     vis[r, c] (+)= wgt[r, c] sum_s amp[s] rowf[s, r] chanf[s, c] / N_s
 *                    exp(sgn 2 pi i f_c / c0 (su u_r l_s + sv v_r m_s - sw w_r (n_s - 1) + off_r))
 *   (stokes2im.py:518-558 with rowf = tprofile, chanf = fprofile * beam, off = w_diff; test_hessian_approx.py:44-67 with
 *   all three absent).  lm (nsrc, 2), amp (nsrc), rowf (nsrc, nrow), chanf (nsrc, nchan) and off (nrow) [m] are host
 *   arrays; rowf, chanf, off and wgt may be NULL (ones, ones, zeros, ones).  n - 1 = -(l^2 + m^2) / (1 + sqrt(1 - l^2 - m^2)),
 *   and -sqrt(l^2 + m^2 - 1) - 1 beyond the horizon, as ducc0 has it.  vis is (nrow, nchan) complex128, wgt (nrow, nchan):
 *   host arrays for _predict, device arrays for _predict_dev.
 * pfbhip_dft_predict_comps / _dev: the same sum with the sources taken from a resident component model
 *   (operators/gridder.py:318-351): l = lshift + (x_index - nx / 2) cellx, m = mshift + (y_index - ny / 2) celly,
 *   amp_s = sum_k basis[k] coeffs[k, s] (k ascending), 0 outside the handle's region mask with use_region != 0.
 * pfbhip_dft_image / _dev: the adjoint, out[s] = sum_{r, c} mask wgt Re(vis[r, c] exp(-sgn 2 pi i ...)) / N_s, out (nsrc) a
 *   host array (the dirty image of the reference's explicit gridder at a list of positions).  Sums run in a fixed order:
 *   two calls on the same input give the same bits.
 */
typedef struct pfbhip_dft pfbhip_dft;
typedef struct pfbhip_dft_conv {
    double su, sv, sw, sgn;
    int32_t do_wgridding, divide_by_n, accumulate, reserved;
    int64_t chan0, nchan;
} pfbhip_dft_conv;
int pfbhip_dft_create(int64_t nrow, int64_t nchan, const double *uvw_host, const double *freq_host, const uint8_t *mask_host,
                      pfbhip_dft **out);
int pfbhip_dft_destroy(pfbhip_dft *h);
int pfbhip_dft_predict(pfbhip_dft *h, const pfbhip_dft_conv *conv, int64_t nsrc, const double *lm, const double *amp,
                       const double *rowf, const double *chanf, const double *off, const double *wgt_host, double *vis_host);
int pfbhip_dft_predict_dev(pfbhip_dft *h, const pfbhip_dft_conv *conv, int64_t nsrc, const double *lm, const double *amp,
                           const double *rowf, const double *chanf, const double *off, const double *wgt_dev, double *vis_dev);
int pfbhip_dft_predict_comps(pfbhip_dft *h, const pfbhip_dft_conv *conv, pfbhip_comps *comps, const double *basis_host,
                             int use_region, double cellx, double celly, double lshift, double mshift, const double *off,
                             const double *wgt_host, double *vis_host);
int pfbhip_dft_predict_comps_dev(pfbhip_dft *h, const pfbhip_dft_conv *conv, pfbhip_comps *comps, const double *basis_host,
                                 int use_region, double cellx, double celly, double lshift, double mshift, const double *off,
                                 const double *wgt_dev, double *vis_dev);
int pfbhip_dft_image(pfbhip_dft *h, const pfbhip_dft_conv *conv, int64_t nsrc, const double *lm, const double *off,
                     const double *wgt_host, const double *vis_host, double *out_host);
int pfbhip_dft_image_dev(pfbhip_dft *h, const pfbhip_dft_conv *conv, int64_t nsrc, const double *lm, const double *off,
                         const double *wgt_dev, const double *vis_dev, double *out_host);

/* ---- Gaussian-resolution convolution and restore --------------------------- */
/*
 * Replaces convolve2gaussres (src/pfb_imaging/utils/misc.py:123-192) with its gaussian2d (:468-502, nsigma = 5) and
 * get_padding_info (:107-120), and the arithmetic of restore_image (src/pfb_imaging/utils/restoration.py:71-88), on the
 * device (restore.hip; DESIGN.md "Gaussian-resolution convolution and restore").
 *
 * pfbhip_gaussconv_create: one plan per (nband, nx, ny, pfrac).  Padded sizes nfft = good_size(n + int(pfrac n), real),
 *   left pad (nfft - n) / 2, the rest on the right (pfbhip_gaussconv_shape returns them).  A geometry whose right pad is
 *   zero on either axis is refused: the reference's slice(l, -0) returns an empty array there.
 * pfbhip_gaussconv_apply / _apply_dev (misc.py:142-192): out[b] = fftshift(c2r(r2c(ifftshift(pad(image[b]))) * K_b))[unpad]
 *   with K_b = gausshat_b, or where(|thishat_b| > 0, gausshat_b / thishat_b, 0) when gausspari is given.  gaussparf is
 *   (nparf, 3) rows of (emaj, emin, pa), nparf 1 or nband; gausspari (npari, 3) with npari == nband, or NULL.  The kernels
 *   are gaussian2d on the grids (-(n // 2) + arange(n)) * scale of each axis, divided by their sum with norm_kernel != 0.
 *   kernf (nparf, nx, ny) / kerni (nband, nx, ny), when non-NULL, are kernels the caller rendered (grids that are no scaled
 *   pixel offsets): they replace the rendering and are taken as they are (norm_kernel is not applied to them).  With
 *   gausspari both or neither are given.  image / out / kernf / kerni are host arrays for _apply, device arrays for
 *   _apply_dev; the parameter arrays are always host arrays.
 * pfbhip_gaussconv_restore / _restore_dev (restoration.py:71-88): image[b] = conv(model[b]; gaussparf_b) + rconv_b with
 *   rconv_b = residual[b] / wsum[b] where allclose(gaussparf_b, gausspari_b) (numpy's defaults, decided on the host per
 *   band), else conv(residual[b] / wsum[b]; gaussparf_b / gausspari_b); pixel-offset grids, kernels not normalised.
 * Refused with PFBHIP_ERR_INVALID: non-positive axes, NaN or non-positive parameters, emin > emaj, gausspari of the wrong
 *   length, nparf not in {1, nband}, a zero or non-finite wsum.
 * pfbhip_gaussconv_debug_fill: test hook, fills every buffer the plan owns with a byte.
 */
typedef struct pfbhip_gaussconv pfbhip_gaussconv;
int pfbhip_gaussconv_create(int64_t nband, int64_t nx, int64_t ny, double pfrac, pfbhip_gaussconv **out);
int pfbhip_gaussconv_destroy(pfbhip_gaussconv *h);
int pfbhip_gaussconv_shape(const pfbhip_gaussconv *h, int64_t *nfft_x, int64_t *nfft_y, int64_t *padl_x, int64_t *padl_y);
int pfbhip_gaussconv_apply(pfbhip_gaussconv *h, const double *image_host, const double *gaussparf, int64_t nparf,
                           const double *gausspari, int64_t npari, int norm_kernel, double scale_x, double scale_y,
                           const double *kernf_host, const double *kerni_host, double *out_host);
int pfbhip_gaussconv_apply_dev(pfbhip_gaussconv *h, const double *image_dev, const double *gaussparf, int64_t nparf,
                               const double *gausspari, int64_t npari, int norm_kernel, double scale_x, double scale_y,
                               const double *kernf_dev, const double *kerni_dev, double *out_dev);
int pfbhip_gaussconv_restore(pfbhip_gaussconv *h, const double *model_host, const double *residual_host, const double *wsum,
                             const double *gausspari, int64_t npari, const double *gaussparf, int64_t nparf, double *image_host);
int pfbhip_gaussconv_restore_dev(pfbhip_gaussconv *h, const double *model_dev, const double *residual_dev, const double *wsum,
                                 const double *gausspari, int64_t npari, const double *gaussparf, int64_t nparf,
                                 double *image_dev);
int pfbhip_gaussconv_debug_fill(pfbhip_gaussconv *h, int byte);

/* ---- clean-beam fit -------------------------------------------------------- */
/*
 * Replaces fitcleanbeam (src/pfb_imaging/utils/misc.py:529-613) with its objective psf_errorsq (:505-526), on the device
 * (cleanbeam.hip; DESIGN.md "Clean-beam fit").  The swap rule and the pixel-size scaling of :615-625 stay with the caller.
 *
 * pfbhip_cleanbeam_fit / _fit_dev: per band of psf (nband, nx, ny; a host array for _fit, a device array for _fit_dev), with
 *   c = 2 sqrt(2 ln 2) and psfv = psf / max(psf):
 *     lobe   = the 4-connected component of {psfv > level} that holds (nx / 2, ny / 2)            (:559-567)
 *     p0     = (emaj0, emin0, pa0) from the lobe's weighted second moments and its rotated extents  (:569-591)
 *     region = {xx^2 + yy^2 < (nsigma emaj0 / c)^2} on pixel offsets from (nx / 2, ny / 2)         (:596-603)
 *     pars   = argmin sum_region (psfv - exp(-c^2 q / 2))^2 over emaj >= 0, emin >= 0, 0 <= pa <= pi,  (:604-611)
 *              q = [x y] R diag(1 / emaj^2, 1 / emin^2) R^T [x y]^T, R = [[-sin pa, -cos pa], [cos pa, -sin pa]]
 *   by a projected Levenberg-Marquardt iteration from p0 (the reference stops L-BFGS-B at factr = 1e7 instead).  pars is
 *   (nband, 3) in pixels, pixels, radians, unswapped: pars[b][0] < pars[b][1] is possible.  An all-zero band gives NaNs.
 *   info (nband records, may be NULL) is filled before any refusal is reported.
 * Refused with PFBHIP_ERR_INVALID: a band whose maximum is not positive although it has non-zero data; a centre pixel that
 *   is not above level (the reference then fits the background); a lobe that still touches a 256-pixel window away from
 *   the image's edge (its FWHM would exceed PFBHIP_CB_MAX_WINDOW pixels).
 */
#define PFBHIP_CB_MAX_WINDOW 256
#define PFBHIP_CB_MAX_ITER 200
#define PFBHIP_CB_MAX_RAISE 30
enum {
    PFBHIP_CB_CONVERGED = 0,   /* the projected step fell below 1e-12 (1 + |p|) */
    PFBHIP_CB_ALL_ZERO = 1,    /* NaN row */
    PFBHIP_CB_ITER_CAP = 2,    /* PFBHIP_CB_MAX_ITER iterations: pars is the last accepted point */
    PFBHIP_CB_RAISE_CAP = 3,   /* PFBHIP_CB_MAX_RAISE damping raises in one iteration: pars is the last accepted point */
    PFBHIP_CB_SWEEP_CAP = 4,   /* the flood fill ran window^2 / 2 rounds (PFBHIP_ERR_RUNTIME) */
    PFBHIP_CB_BAD_PEAK = 5,    /* refusals */
    PFBHIP_CB_CENTRE_LOW = 6,
    PFBHIP_CB_LOBE_TOO_WIDE = 7
};
typedef struct {
    int32_t status, window, nit, nlobe; /* PFBHIP_CB_*, final window width, LM iterations, lobe pixels */
    int64_t nfit;                       /* pixels in the fit region */
    double f, p0[3];                    /* objective at pars; the start point */
} pfbhip_cleanbeam_info;
int pfbhip_cleanbeam_fit(const double *psf_host, int64_t nband, int64_t nx, int64_t ny, double level, double nsigma,
                         double *pars /* nband*3, pixel units, unswapped */, pfbhip_cleanbeam_info *info /* nband, may be NULL */);
int pfbhip_cleanbeam_fit_dev(const double *psf_dev, int64_t nband, int64_t nx, int64_t ny, double level, double nsigma,
                             double *pars /* nband*3, pixel units, unswapped */, pfbhip_cleanbeam_info *info /* nband, may be NULL */);

/* ---- primary beams ----------------------------------------------------------- */
/*
 * Replaces the two scipy call sites of the primary beam (beam.hip).
 *
 * pfbhip_beam_regrid replaces eval_beam (src/pfb_imaging/utils/beam.py:75-89, called at operators/gridder.py:454 and :848):
 *   RegularGridInterpolator((l_in, m_in), beam[c], method="linear", bounds_error=False, fill_value=1.0) for every
 *   correlation of beam (ncorr, nl, nm) in one launch.  l_in (nl) and m_in (nm) are strictly ascending nodes, uniform or
 *   not.  general == 0: l_out (nx), m_out (ny) span the output grid; general != 0: l_out, m_out are (nx, ny) coordinate
 *   arrays.  out is (ncorr, nx, ny).  Index i with node[i] <= x < node[i + 1] clipped to [0, n - 2], weight
 *   t = (x - node[i]) / (node[i + 1] - node[i]); a point with either coordinate outside [node[0], node[n - 1]] is exactly
 *   1.0 (the last node is inside); a correlation whose beam is identically 1.0 gives exact ones (:85-86, decided by a
 *   device reduction).
 * pfbhip_beam_rotate_mean replaces the rotation loop of src/pfb_imaging/utils/stokes2vis_msv4.py:405-409:
 *   out[c] = mean over angles of ndimage.rotate(beam0[c], angle, reshape=False, mode="nearest") (cubic splines), beam0 and
 *   out (ncorr, n0, n1), angles in degrees.  Edge pad by 12, B-spline prefilter with scipy's reflect initialisation, then
 *   one pass over the output that evaluates the 4x4 B-spline at every angle.
 * All arrays are host arrays.  device_ms, when not NULL, receives the time of the kernels alone (device events; the
 *   copies are outside).
 * Refused with PFBHIP_ERR_INVALID: NULL arrays, fewer than two nodes on an axis, nodes that are not finite or not strictly
 *   ascending, non-positive sizes, no angle or an angle that is not finite.
 */
int pfbhip_beam_regrid(const double *beam_host, int32_t ncorr, int64_t nl, int64_t nm, const double *l_in, const double *m_in,
                       const double *l_out, const double *m_out, int general, int64_t nx, int64_t ny, double *out_host,
                       double *device_ms /* may be NULL */);
int pfbhip_beam_rotate_mean(const double *beam0_host, int32_t ncorr, int64_t n0, int64_t n1, const double *angles_deg,
                            int32_t nangles, double *out_host, double *device_ms /* may be NULL */);

/* ---- Stokes visibilities: weight_data --------------------------------------- */
/*
 * Replaces weight_data (src/pfb_imaging/utils/weighting.py:274-468, called at utils/stokes2vis.py:196-209,
 * utils/stokes2vis_msv4.py:294 and utils/stokes2im.py:447-460) on the device (stokes.hip).
 *
 * pfbhip_stokes_spec is what stokes_expr_funcs (src/pfb_imaging/utils/stokes.py:89-155) selects: nc correlations (2 or 4),
 *   a diagonal (full_jones == 0) or full 2x2 Jones term, linear or circular feeds, and ns products as ascending indices
 *   into IQUV.  corr_first != 0 writes vis / wgt as (ns, nrow, nchan) (the transpose of utils/stokes2im.py:561-562)
 *   instead of (nrow, nchan, ns).
 * pfbhip_weight_data: for every sample of a row that a time bin covers (rows tbin_idx[t] - min(tbin_idx) ... +
 *   tbin_counts[t], weighting.py:380-387) with no correlation flagged (:391, :442), p = ant1[row], q = ant2[row]:
 *     vis[k] = sum_c Tinv[k][c] vec(Jp^-1 V Jq^-H)[c],   wgt[k] = sum_c w_c |((Jp (x) conj(Jq)) T)[c][k]|^2
 *   with T of utils/stokes.py:33 / :35 and two-correlation data widened as weighting.py:257-266 does; every other sample
 *   is 0.  data (nrow, nchan, nc) complex, weight (nrow, nchan, nc), flag (nrow, nchan, nc) bytes, jones
 *   (ntime, nant, nchan, 2) or (ntime, nant, nchan, 2, 2) complex128 (direction 0 of the reference's array), tbin_idx and
 *   tbin_counts (nbin), ant1 and ant2 (nrow).  mask (nrow, nchan) uint8, when not NULL, receives ~flag.any(-1)
 *   (utils/stokes2im.py:463-464, utils/stokes2vis.py:285-286).  Arithmetic is f64; the _sp entry takes complex64 / float32
 *   data and weights and returns complex64 / float32, widened and narrowed on the device (jones stays complex128).
 * pfbhip_weight_data_dev: the same with vis, wgt and mask device arrays that stay in HBM; the inputs are host arrays.
 * device_ms, when not NULL, receives the time of a second, warm launch of the kernel (device events; copies outside).
 * Refused with PFBHIP_ERR_INVALID before anything reaches the device: a spec the reference refuses (full Jones with two
 *   correlations, a product two correlations do not give), a time bin outside [0, nrow], more bins than ntime, an antenna
 *   of a covered row outside [0, nant), NULL arrays.
 * pfbhip_debug_copy16: bench hook, the mean time of a 16-byte-per-lane device copy of nbytes.
 */
typedef struct pfbhip_stokes_spec {
    int32_t nc, full_jones, circular, ns;
    int32_t product[4];
    int32_t corr_first, reserved;
} pfbhip_stokes_spec;
int pfbhip_weight_data(const pfbhip_stokes_spec *spec, int64_t nrow, int64_t nchan, int64_t nant, int64_t ntime, int64_t nbin,
                       const double *data_host, const double *weight_host, const uint8_t *flag_host, const double *jones_host,
                       const int64_t *tbin_idx, const int64_t *tbin_counts, const int32_t *ant1, const int32_t *ant2,
                       double *vis_host, double *wgt_host, uint8_t *mask_host /* may be NULL */, double *device_ms /* may be NULL */);
int pfbhip_weight_data_sp(const pfbhip_stokes_spec *spec, int64_t nrow, int64_t nchan, int64_t nant, int64_t ntime, int64_t nbin,
                          const float *data_host, const float *weight_host, const uint8_t *flag_host, const double *jones_host,
                          const int64_t *tbin_idx, const int64_t *tbin_counts, const int32_t *ant1, const int32_t *ant2,
                          float *vis_host, float *wgt_host, uint8_t *mask_host /* may be NULL */, double *device_ms /* may be NULL */);
int pfbhip_weight_data_dev(const pfbhip_stokes_spec *spec, int64_t nrow, int64_t nchan, int64_t nant, int64_t ntime, int64_t nbin,
                           const double *data_host, const double *weight_host, const uint8_t *flag_host, const double *jones_host,
                           const int64_t *tbin_idx, const int64_t *tbin_counts, const int32_t *ant1, const int32_t *ant2,
                           double *vis_dev, double *wgt_dev, uint8_t *mask_dev /* may be NULL */, double *device_ms /* may be NULL */);
int pfbhip_debug_copy16(int64_t nbytes, int32_t reps, double *ms);

/* ---- band reduce over xGMI (RCCL) ------------------------------------ */
/*
 * Replaces the driver-side band sums of the reference
 * (src/pfb_imaging/core/grid.py:430-446, core/deconv.py:320-321): one process
 * per GPU, sum(dirty/residual) to root.  The 128-byte unique id is produced on
 * rank 0 and carried to the other ranks by the caller's launcher (torchrun /
 * any store).
 */
#define PFBHIP_UNIQUE_ID_BYTES 128
int pfbhip_comm_unique_id(uint8_t *id /* [PFBHIP_UNIQUE_ID_BYTES] */);
int pfbhip_comm_create(const uint8_t *id, int nranks, int rank, pfbhip_comm **out);
int pfbhip_comm_destroy(pfbhip_comm *c);
int pfbhip_comm_reduce_sum(pfbhip_comm *c, const double *send_dev, double *recv_dev, int64_t count, int root);
int pfbhip_comm_allreduce_sum(pfbhip_comm *c, const double *send_dev, double *recv_dev, int64_t count);
/* All-gather of equal blocks (recv = nranks blocks of `count` doubles, block r from rank r): the band pool's cube-level
 * methods when every rank owns the same number of bands (operators/band_worker.py:239-308). */
int pfbhip_comm_allgather(pfbhip_comm *c, const double *send_dev, double *recv_dev, int64_t count);
/* Host-array forms on the communicator's persistent device staging buffers (no allocation per call). */
int pfbhip_comm_allreduce_sum_host(pfbhip_comm *c, double *inout_host, int64_t count);
int pfbhip_comm_reduce_sum_host(pfbhip_comm *c, const double *send_host, double *recv_host, int64_t count, int root);
int pfbhip_comm_allgather_host(pfbhip_comm *c, const double *send_host, double *recv_host, int64_t count);
int pfbhip_comm_barrier(pfbhip_comm *c);

#ifdef __cplusplus
}
#endif
#endif /* PFBHIP_H */
