/*
 * lpc.h -- C ABI of the MI355X-native iterative deconvolution engine
 *          ("lpc" = LenslessPiCam hot path).
 *
 * The reference (LCAV/LenslessPiCam) is pure Python and has NO FFI for this path: its
 * "plugin API" is the Python class interface ReconstructionAlgorithm.set_data()/apply()
 * (lensless/recon/recon.py:179-605) implemented by ADMM (lensless/recon/admm.py:24-338),
 * GradientDescent / NesterovGradientDescent / FISTA (lensless/recon/gd.py:62-241) on top
 * of RealFFTConvolve2D (lensless/recon/rfft_convolve.py:26-223).  This header is the
 * boundary a maintainer would bind (ctypes stub in INTEGRATION.md); every entry point names
 * the reference method whose arithmetic it replaces.
 *
 * Conventions
 *  - plain C, no torch types.  Every pointer named dev_* is a DEVICE pointer (HBM) that the
 *    library only borrows for the duration of the call; images are lpc_real, channels-last,
 *    exactly the reference's layouts: psf (D,H,W,C), data (B,H,W,C), image estimate
 *    (B,D,H,W,C) for the gradient-descent family and (B,D,Hp,Wp,C) for ADMM (which iterates
 *    on the padded frame, admm.py:101 pad=False).
 *  - every function returns 0 on success, non-zero on failure; lpc_last_error() then holds
 *    a message (thread-local).  Nothing throws across the boundary.
 *  - one handle <-> one stream at a time; a handle is not thread-safe, distinct handles are
 *    independent.  stream is a hipStream_t passed as void* (NULL = default stream).
 *  - the library REQUIRES a HIP device; there is no CPU fallback.
 */
#ifndef LPC_H_
#define LPC_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lpc_engine* lpc_handle;

/* The library is built twice from the same sources: liblpc.so computes in float32 (the reference's
 * default dtype), liblpc_f64.so (-DLPC_DOUBLE) in float64 (dtype="float64", lensless/utils/io.py:645-674).
 * Every image / state buffer of a library is an array of its lpc_real. */
#ifdef LPC_DOUBLE
typedef double lpc_real;
#else
typedef float lpc_real;
#endif

enum lpc_algo {
  LPC_ALGO_CONV = 0,     /* operator only: RealFFTConvolve2D            rfft_convolve.py:26  */
  LPC_ALGO_ADMM = 1,     /* ADMM, TV prior + non-negativity             admm.py:24           */
  LPC_ALGO_GD = 2,       /* projected gradient descent                  gd.py:62             */
  LPC_ALGO_NESTEROV = 3, /* + Nesterov momentum                         gd.py:143            */
  LPC_ALGO_FISTA = 4     /* + FISTA momentum                            gd.py:191            */
};

enum lpc_norm { LPC_NORM_BACKWARD = 0, LPC_NORM_ORTHO = 1, LPC_NORM_FORWARD = 2 };

typedef struct lpc_config {
  int algo;                /* enum lpc_algo                                                   */
  int height, width;       /* un-padded H, W of PSF and data                                  */
  int channels;            /* C: 1 or 3                          recon.py:255-256             */
  int depth;               /* D >= 1.  ADMM with D > 1 = D independent planes sharing the     */
                           /* measurement (the reference refuses)  */
  int batch;               /* B >= 1 measurements sharing the PSF (additive to the reference) */
  int norm;                /* enum lpc_norm of the PSF spectrum  rfft_convolve.py:27,121      */
  int pad;                 /* LPC_ALGO_CONV only: operator pads/crops (1) or works on the     */
                           /* padded frame (0)                   rfft_convolve.py:133-176     */
  double mu1, mu2, mu3, tau; /* ADMM                              admm.py:39-42                */
  double lip_fact;         /* GD family step factor              gd.py:67,107-112             */
  double nesterov_mu, nesterov_p; /* gd.py:153,178-181                                         */
  double fista_tk;         /* gd.py:200,227-233                                               */
  const char* options;     /* NULL, or "key=value,key=value": launch-plan choices (below).  Read  */
                           /* by lpc_create only; the string is not kept.                         */
} lpc_config;

/* Launch-plan options (lpc_config.options; the environment variable LPC_OPTIONS, same syntax, supplies process-wide
 * defaults that a handle's own string overrides).  None changes a result beyond float round-off; none is needed in
 * production -- they exist so that tests and A/B measurements can select a launch plan without touching the process
 * environment.  lpc_plan_info() reports the plan a handle ended up with.
 * Which kernels a handle gets
 *   no_static=1        run-time FFT plans only (no plan module is looked for)
 *   jit=0              never compile a plan module: use what is on disk (default 1: a frame shape whose module is
 *                      missing is compiled with hipcc on first use, ~3 s, and kept in <libdir>/modules or ~/.cache)
 *   jit_min_points=N   padded frames with fewer than N points keep the run-time plans (default 65536)
 *   module_dir=PATH    first place modules are looked for / written;  compiler=PATH  the hipcc to use
 *   module_max=N module_loaded_max=N    plan-module files kept per directory this library writes to (256, least
 *                      recently used removed first); modules kept loaded once no handle uses them (64)
 * Forcing a plan the chooser takes at other sizes (how the tests run every kernel family on small frames)
 *   rows_half=0|1      paired rows / one real row per half-length transform (default: by width)
 *   col_t=N tile_budget=N split_n2=N passa_t=N     column tiling: image columns per tile, LDS points per tile, forced
 *                      length of the fused middle transform, columns per pass-A tile
 *   mid_seq=0|1        ADMM single-pass middle one spectrum at a time / side by side (default: by batch size);
 *   mid_pre=0          ... one at a time: the second tile's loads behind the first transform (default: both up front)
 *   prow_nt128=0|1     short paired rows on 256 / 128 threads (default: by batch size)
 *   g_plane=0|1        ADMM middles read |PsiT Psi| as a row term + a column term when it separates (0) / from its plane
 *                      (1); default: the terms when the plane exceeds 8 MB
 *   mid_swz=0|1        side-by-side middle: adjacent half-line column tiles on one XCD (default: when a tile row is < 128
 *                      bytes and the spectra are not in pair lines)
 *   spec_lay=0         ADMM work spectra as plain rows (default: paired rows + a single-pass middle of 8-column tiles keep
 *                      them in PAIR LINES -- rows 2p, 2p + 1 x 8 columns share one 128-byte line, lpc_args.h: spec_col)
 *   row_rad=16.16.8    radices of the compile-time row plan instead of the chooser's (one module)
 * The structure of an ADMM iteration (each setting is an older, complete form of the same arithmetic)
 *   xi_full=1 hv_full=1   without the sensor-window structure of xi / of the H V row transforms
 *   mid_pc=0           sequential middle on pair-line spectra: H, |G| and the phase factors loaded and combined per element
 *                      (default 1: precombined once per PSF and step sizes into one 16-byte + one 4-byte load per element)
 *   k1_half=0          duals stored plain between the iterations of one call (default 1: half-applied, the tiled kernel
 *                      then does not read V_old: 9R -> 8R)
 *   rho_rsp=0          ... rho~ stored and read between the iterations of one call (default 1: the tiled kernel recovers it
 *                      from the r_sp it overwrites and the eta~ it loads anyway: 8R -> 7R; not on the three-launch plan)
 *   xi_half=0          ... xi stored plain between the iterations of one call (default 1: half-applied, xi~ = -a, the X
 *                      half of the forward rows then does not read H V_old inside the sensor window: 3 Rw -> 2 Rw)
 *                      (k1_half=0 switches both off)
 *   k1_rows=0          keep the tiled TV / W kernel (default 1: paired rows of one or two quads per lane -- padded widths up
 *                      to 2048 -- take that half of the image-domain work as well: three launches per iteration, r_sp never
 *                      stored; rows of up to 1024 points then run on 256 lanes at every batch size)
 *   k1_group=N         ... on launches of more than 8192 row blocks: runs of N consecutive blocks per XCD (default 16;
 *                      0: launch order)
 *   admm_rows_v2=BITS  the second form of the half-length row kernels (lpc_admm_v2_kernels.h; wherever the row plan has one
 *                      radix and the window offset / width are even; float32; same bits as the first form): 1 the forward
 *                      rows with the X half (default), 2 the inverse rows (slower at 12 MP), 3 both; 0: first form
 *   hv_fuse=0          H V written and read back between the iterations of one call (default 1: where bit 0 of admm_rows_v2,
 *                      the H V row skipping and xi_half are on and the row plan is 16.16.16, every iteration but the last
 *                      three of a call keeps the sensor window's rows of H V in registers -- inverse row, the next X half
 *                      and forward row in one kernel, k_hv_rows_v2 -- same bits; 2: that launch behind the rows of V)
 * Block orders (permutations)
 *   rev_order=BITS     which ADMM kernels walk their grids backwards (1 tiled kernel, 2 / 4 forward / inverse pass A,
 *                      8 LDS middle; default 9);  gd_rev=BITS (gradient-descent family / operator: 1 residual rows, 2
 *                      update rows, 4 register middle; default: all three when a work spectrum exceeds the 256-MB
 *                      memory-side cache)
 * Gradient-descent family
 *   gd_v2=0            the first form of the two fused row kernels (default 1: the second form, lpc_gd_v2_kernels.h,
 *                      wherever the row plan has one radix and the window offset / width are even)
 *   gd_no_fuse_fwd=1   update without the next iteration's forward rows
 * (Variants that were built, measured and not adopted -- persistent row workgroups with LDS-DMA prefetch, whole-column
 * single-launch transforms, the xor / i + i/16 LDS layouts, staggered first generations, padded row pitches, the half-line
 * tile pairing of the sequential middle -- left the sources in round 6; their measurements are in profiles/HISTORY.md.)
 * Path-valued options (module_dir, compiler) are unescaped before use: %XX (two hex digits) stands for the byte XX, so the
 * separators of this string can appear in a path -- "%2C" is ',', "%3B" ';', "%20" ' ' -- and a literal '%' that is
 * followed by two hex digits must itself be written "%25".
 * An unknown key makes lpc_create fail. */

/* ---- life cycle ------------------------------------------------------------------ */
/* replaces the constructors (recon.py:203-329, admm.py:35-135, gd.py:67-92) minus the PSF */
int lpc_create(const lpc_config* cfg, lpc_handle* out);
int lpc_destroy(lpc_handle h);
/* Plan modules.  The compile-time-plan kernels of one frame shape live in a small shared object next to the library
 * (lenslesspicam_amd/csrc/lpc_plan.h); lpc_create loads it, compiling it first when missing.  lpc_plan_module reports
 * the key of the module lpc_create(cfg) would use ("" = none: run-time plans) and, with build != 0, compiles it now if
 * it is not on disk -- no device needed, so a build step can pre-build the shapes it knows (build.py does, for
 * BASELINE.json's).  key_buf may be NULL. */
int lpc_plan_module(const lpc_config* cfg, int build, char* key_buf, size_t n);
const char* lpc_last_error(void);
const char* lpc_backend(void);        /* "hip-gfx950" for the product library */
const char* lpc_real_name(void);      /* "float32" or "float64": the arithmetic type of this build */

/* padded frame chosen by the engine: next 5-smooth length >= 2*dim-1 (rfft_convolve.py:110-117) */
int lpc_padded_shape(lpc_handle h, int* Hp, int* Wp, int* start_h, int* start_w);

/* ---- operator: RealFFTConvolve2D.set_psf / convolve / deconvolve ------------------- */
/* dev_psf: (D,H,W,C).  Computes the PSF spectrum (and for ADMM R_divmat, for the GD family
 * the step alpha and the default initial estimate).  rfft_convolve.py:102-131,
 * admm.py:186-193, gd.py:94-126.  Implies lpc_reset(). */
int lpc_set_psf(lpc_handle h, const lpc_real* dev_psf, void* stream);
/* One PSF per frame: dev_psfs is (cfg.batch, D, H, W, C), and frame b of every later call is convolved with PSF b
 * (trainable_recon.py:346-350 rebuilds its convolver from a 5-D `psfs`, rfft_convolve.py:55-58,84-117).  The handle then
 * holds batch*D*C PSF spectra instead of D*C -- state plane q reads plane q where it read q % (D*C) -- until the next
 * lpc_set_psf, which returns to one PSF for the batch.  Like lpc_set_psf it implies lpc_reset(), and ADMM's precombined
 * middle constants are remade at the next iteration; unlike lpc_set_psf it leaves a caller's gram (lpc_set_psi_gram) in
 * place -- the gram of the prior does not depend on the PSF.  One launch sequence for all the PSFs (layout, forward transform of
 * batch*D*C planes, norm scale, pair-line copy); it does not wait for the stream, except at the first call of a handle,
 * which gives the D*C-plane buffers back and allocates them for batch*D*C planes:
 *     workspace_bytes grows by (batch - 1) * D*C * (spectrum plane + frame), for ADMM handles whose plan keeps pair-line
 *     copies by another spectrum plane, and with the sequential middle's precombined constants by 1.5 (real phases) or 2.5
 *     (complex phases) more.  (Spectrum plane: 2 * sizeof(real) * ((Hp + 1) & ~1) * cpitch bytes, cpitch = Wp/2 + 1 rounded
 *     up to 16; frame: sizeof(real) * H * W.)  The buffers keep that size for the life of the handle.
 * lpc_iterate, lpc_form_image, lpc_get_state, the plug-and-play and custom-psi steps, lpc_convolve,
 * lpc_convolve_spectrum (n == cfg.batch: plane q of the input meets PSF plane q) and lpc_reconstruction_error work as
 * before.  Refused, with a message that says "per-frame":
 *     lpc_fista_record / lpc_admm_record with a non-zero argument, the four backward entries, and this call on a handle
 *     that records: gradients with per-frame PSFs are not implemented (unless lpc_per_frame_grad, below, switched them on);
 *     a gradient-descent handle without a pinned start value (lpc_set_start_value) and a schedule
 *     (lpc_set_fista_schedule): plain GD / Nesterov / FISTA take their step and start value from ONE PSF. */
int lpc_set_psf_batch(lpc_handle h, const lpc_real* dev_psfs, void* stream);
/* Gradients with one PSF per frame: a switch of the handle, off by default -- then every refusal above answers as written.
 * lpc_per_frame_grad(h, 1): lpc_fista_record / lpc_admm_record work on a handle that holds per-frame PSFs,
 * lpc_set_psf_batch works on a handle that records (it invalidates what was recorded, like lpc_set_psf, and the reset it
 * implies starts the tape over), and the four backward entries run: frame b's state planes meet PSF b's spectrum in the
 * replay, in every spectral step of the reverse sweeps and in the PSF-gradient terms, as in the forward.  The parameter
 * gradients are summed over the frames as before; dev_grad_psf of the two _psf entries is then (B,D,H,W,C), PSF b's own
 * gradient in slice b, nothing summed over the batch (on a handle with one PSF it stays (D,H,W,C)).  Every other refusal
 * of the backward entries (odd padded lengths, depth > 1, the norm, ...) is unchanged.  Workspace of the PSF gradient on a
 * per-frame handle:
 *   ADMM   (4 * P + P) * Hp * cpitch * 2 * sizeof(lpc_real) bytes: the accumulator grows from C to P = B * C spectrum planes
 *          (a handle whose workspace was allocated by a one-PSF backward gives it back and allocates this; it does not
 *          shrink again before lpc_admm_record(h, 0));
 *   FISTA  unchanged (lpc_fista_backward_psf): its accumulator is P planes already.
 * lpc_per_frame_grad(h, 0) returns to the refusals; it frees nothing. */
int lpc_per_frame_grad(lpc_handle h, int on);

/* out = ifftshift(irfft2(rfft2(pad?(x)) * H or conj(H))) cropped if cfg.pad.
 * x: (n, D, Hx, Wx, x_channels), out: (n, D, Hx, Wx, C) with (Hx,Wx) = (H,W) if cfg.pad else (Hp,Wp);
 * n <= cfg.batch.  x_channels is C, or 1 (a grayscale input against an RGB PSF broadcasts over the channels like
 * the reference's `vpad[...] = v`, rfft_convolve.py:96-99); anything else is refused (it would be read out of bounds).
 * adjoint = 0: convolve (rfft_convolve.py:133-176); 1: deconvolve (:178-223). */
int lpc_convolve(lpc_handle h, const lpc_real* dev_x, lpc_real* dev_out, int n, int x_channels, int adjoint,
                 void* stream);

/* convolve / deconvolve with return_fft=True (rfft_convolve.py:148-150,161-163,193-195,206-208): the spectrum
 * rfft2(pad?(x)) * H (adjoint: * conj(H)) the reference returns instead of transforming back.  dev_out: complex values
 * as (re, im) pairs of lpc_real, (n, D, Hp, Wp/2+1, C), natural frequency order like rfft2's.  LPC_ALGO_CONV handles. */
int lpc_convolve_spectrum(lpc_handle h, const lpc_real* dev_x, lpc_real* dev_out, int n, int x_channels, int adjoint,
                          void* stream);

/* ---- solver state: set_data / _set_initial_estimate / reset ------------------------ */
/* dev_data: (B,H,W,data_channels) with B == cfg.batch; data_channels is C, or 1 (broadcast over the PSF's channels,
 * as `self._convolver._pad(self._data)` does, admm.py:253 / `- self._data`, gd.py:129).  recon.py:352-381 */
int lpc_set_data(lpc_handle h, const lpc_real* dev_data, int data_channels, void* stream);
/* dev_est: image-estimate shape (see top) or NULL to clear.  Takes effect at the next
 * lpc_reset(), like recon.py:383-413. */
int lpc_set_initial_estimate(lpc_handle h, const lpc_real* dev_est, void* stream);
/* admm.py:150-230 / gd.py:94-126,178-181,227-233 */
int lpc_reset(lpc_handle h, void* stream);
/* Nesterov: overrides (p, mu) like NesterovGradientDescent.reset(p, mu) gd.py:178-181;
 * FISTA: overrides tk like FISTA.reset(tk) gd.py:227-233.  Call after lpc_reset. */
int lpc_set_momentum(lpc_handle h, double p, double mu, double tk);
/* GD family: pins the default start value, dev_start: C values on the device (what lpc_get_state "start_value" wrote).
 * From then on lpc_set_psf leaves it alone -- the reference's UnrolledFISTA computes `_image_init` once, from the
 * constructor's PSF (unrolled_fista.py:55-59), and forward(batch, psfs=...) / _set_psf() restart from it whatever PSF is
 * current.  NULL: the start value follows the PSF again from the next lpc_set_psf on (gd.py:100-105).  Takes effect at the
 * next lpc_reset(); allocates nothing; an initial estimate (lpc_set_initial_estimate) still wins. */
int lpc_set_start_value(lpc_handle h, const lpc_real* dev_start, void* stream);

/* Unrolled ADMM (lensless/recon/unrolled_admm.py:133-234): iteration i (counted from the last reset)
 * uses mu1[i], mu2[i], mu3[i], tau[i]; the last entry is held beyond n.  n <= 0 clears the schedule and
 * returns to the constructor's constants. */
int lpc_set_admm_schedule(lpc_handle h, int n, const double* mu1, const double* mu2, const double* mu3,
                          const double* tau);

/* Unrolled FISTA (lensless/recon/unrolled_fista.py:60-106): iteration i uses the step alpha[i*C + c] and
 * the momentum factor coef[i] = (t_i - 1) / t_{i+1}; x_k starts as the initial image.  alpha, coef are
 * HOST arrays of n*C and n floats.  n <= 0 returns to the plain FISTA recursion. */
int lpc_set_fista_schedule(lpc_handle h, int n, const lpc_real* alpha, const lpc_real* coef, void* stream);

/* Reverse mode of the unrolled FISTA iterations (unrolled_fista.py:102-106 differentiated; what torch.autograd does
 * in the reference's training loop).  FISTA handles with a schedule (lpc_set_fista_schedule) only.
 * lpc_fista_record(h, 1): from the next lpc_reset on, lpc_iterate keeps the tape -- the iterate and x_k of every
 * iteration, (2 n + 1) un-padded state arrays, plus three work arrays and the partial sums of the reductions
 * (n * B * D * C * H * 2 doubles), allocated for the schedule's n iterations and counted in lpc_workspace_bytes; the
 * recorded forward launches the same kernels as the unrecorded one.  lpc_fista_record(h, 0) frees it (this waits for the
 * stream); lpc_fista_record(h, -1) pauses: nothing is recorded from the next lpc_reset on, the tape stays allocated (no
 * wait, no allocation: what a training loop that alternates with evaluation wants).  lpc_set_fista_schedule and
 * lpc_set_data invalidate what was recorded.
 * lpc_fista_backward: given dL/d(lpc_form_image) it writes the gradients w.r.t. the measurement, the schedule's alpha[]
 * and coef[] and the initial estimate.  Asynchronous on `stream`, device memory only, no synchronisation; the tape and
 * the solver state stay intact (it may be called again: the same bits come out).  It fails, with a message, when: the
 * handle is not a FISTA handle / has no schedule / does not record; the iterations since the reset are not exactly the
 * schedule's; the padded height or width is odd (the recursion uses convolve and deconvolve as each other's adjoints,
 * which they are for even padded lengths only); depth > 1; a split iteration is pending; an alpha of the schedule is 0. */
int lpc_fista_record(lpc_handle h, int on);
int lpc_fista_backward(lpc_handle h, const lpc_real* dev_grad_out,   /* (B,D,H,W,C): dL/d(lpc_form_image)        */
                       lpc_real* dev_grad_data,    /* (B,H,W,data_channels) or NULL                            */
                       lpc_real* dev_grad_alpha,   /* n*C, gradient w.r.t. the alpha[] given to the schedule   */
                       lpc_real* dev_grad_coef,    /* n,   gradient w.r.t. coef[]                               */
                       lpc_real* dev_grad_init,    /* (B,D,H,W,C) or NULL: w.r.t. the initial estimate          */
                       void* stream);
/* lpc_fista_backward_psf: lpc_fista_backward plus the gradient w.r.t. the PSF given to lpc_set_psf, summed over the batch
 * (the start value and the schedule count as constants, as in the reference's forward(batch, psfs=...)).  With the
 * tape's y_i, the sweep's gz_i and Hg_i = Cv(gz_i), the residual r_i = Cv(y_i) - b recomputed, P = zero-padding,
 * F = rfft2, K = crop . ifftshift . irfft2 and s the norm factor of the PSF spectrum, iteration i adds
 *   -alpha[i][c] * s * sum over the batch of  K(conj(F(P gz_i)) . F(P r_i)) + K(conj(F(P y_i)) . F(P Hg_i)).
 * Same refusals (and messages) as lpc_fista_backward; deterministic (no atomics).  Its workspace is allocated at the first
 * call, counted in lpc_workspace_bytes, kept across a pause and freed with the tape by lpc_fista_record(h, 0):
 *   3 * P * Hp * cpitch * 2 * sizeof(lpc_real)  +  P * H * W * sizeof(lpc_real)      bytes,
 * P = B * C planes, cpitch = Wp / 2 + 1 rounded up to a multiple of 16 (Hp, Wp: lpc_padded_shape).  lpc_fista_backward
 * itself allocates and launches nothing of this.  dev_grad_psf NULL: lpc_fista_backward.  On a handle that holds one PSF
 * per frame (lpc_set_psf_batch with lpc_per_frame_grad) nothing is summed over the batch: dev_grad_psf is (B,D,H,W,C). */
int lpc_fista_backward_psf(lpc_handle h, const lpc_real* dev_grad_out, lpc_real* dev_grad_data, lpc_real* dev_grad_alpha,
                           lpc_real* dev_grad_coef, lpc_real* dev_grad_init,
                           lpc_real* dev_grad_psf,    /* (D,H,W,C): w.r.t. the PSF; per-frame PSFs: (B,D,H,W,C)  */
                           void* stream);

/* Reverse mode of the unrolled ADMM iterations (unrolled_admm.py:181-234 differentiated; what torch.autograd does in the
 * reference's training loop).  ADMM handles with a schedule (lpc_set_admm_schedule) only.
 * lpc_admm_record(h, 1): from the next lpc_reset on, lpc_iterate keeps the iterates V_0 .. V_n -- the launch plan's own
 * kernels plus one device copy per iteration, so the recorded forward has the bits of the unrecorded one.  Nothing a launch
 * plan keeps in its own form (H V outside the window, xi, half-applied duals) is taped: lpc_admm_backward first replays
 * H V_i and the duals of every iteration from the iterates, so the tape is the same for every plan.  For a schedule of n
 * iterations the tape is ONE allocation, counted in lpc_workspace_bytes,
 *   (6 n + 11) * P * Hp * rpitch * sizeof(lpc_real)  +  n * P * ceil(Hp / 8) * ceil(Wp / 128) * 4 * sizeof(double)   bytes,
 * P = B * C planes, rpitch = Wp rounded up to a multiple of 4 (Hp, Wp: lpc_padded_shape): V_i and H V_i (2 n + 2 arrays),
 * xi, eta (two components) and rho of every iteration (4 n), 8 work arrays of the sweep, the data gradient, and the partial
 * sums of the four reductions.  lpc_admm_record(h, 0) frees it (this waits for the stream); lpc_admm_record(h, -1) pauses:
 * nothing is recorded from the next lpc_reset on, the tape stays allocated.  lpc_set_admm_schedule, lpc_set_data and
 * lpc_set_psf invalidate what was recorded.
 * lpc_admm_backward: given dL/d(clip(crop(V_n), 0)) -- the (B,D,H,W,C) image UnrolledADMM returns, unrolled_admm.py:236-240
 * -- it writes the gradients w.r.t. the measurement and the mu1[], mu2[], mu3[], tau[] given to lpc_set_admm_schedule (n
 * values each).  Per iteration: one spectral step of the forward's own (on every plan the form lpc_admm_pnp_end uses) and
 * one fused image-domain kernel; all four parameter gradients are image-domain dot products.  Asynchronous on `stream`,
 * device memory only, no atomics: a second call gives the same bits; the tape and the solver state stay intact.  It
 * fails, with a message, when: the handle is not an ADMM handle / has no schedule / has nothing recorded; the iterations
 * since the reset are not exactly the schedule's; depth > 1; the padded height or width is odd (the spectral step and the
 * convolve / deconvolve pair are self-adjoint for even padded lengths only); lpc_set_psi_gram replaced the prior or the
 * handle runs plug-and-play iterations; an initial estimate is set. */
int lpc_admm_record(lpc_handle h, int on);
int lpc_admm_backward(lpc_handle h, const lpc_real* dev_grad_out,   /* (B,D,H,W,C)                                   */
                      lpc_real* dev_grad_data,    /* (B,H,W,data_channels) or NULL                             */
                      lpc_real* dev_grad_mu1, lpc_real* dev_grad_mu2, lpc_real* dev_grad_mu3,
                      lpc_real* dev_grad_tau,     /* n values each                                             */
                      void* stream);
/* lpc_admm_backward_psf: lpc_admm_backward plus the gradient w.r.t. the PSF given to lpc_set_psf, summed over the batch.
 * The PSF spectrum Hs enters iteration i three times: in H V_{i+1}, in HT a_i inside r_k (a_i = mu1[i] X_i - xi_i) and
 * in R_i = 1 / (mu1[i] |Hs|^2 + mu2[i] |G| + mu3[i]).  With F = rfft2, phi the +-1 phase of the convolver's ifftshift,
 * ab the adjoint of H V_{i+1} and rb the adjoint of r_k -- what the sweep holds in front of and behind the spectral step
 * of iteration i -- and a_i recomputed from the tape, iteration i adds, summed over the frames of the batch,
 *   g^ += phi conj(F V_{i+1}) F ab  +  phi conj(F rb) F a_i  -  2 mu1[i] Re(conj(F rb) F V_{i+1}) Hs
 * in ONE complex accumulator of C spectrum planes kept across all iterations; after the sweep
 *   g_psf = s * crop_to_the_PSF_window(irfft2(g^)),      s the norm factor of the PSF spectrum (1 for "backward"):
 * one inverse transform.  Per iteration: one image-domain kernel (a_i), four forward transforms of P planes and one
 * point-wise kernel over the spectra.  Same refusals (and messages) as lpc_admm_backward, and one more: a handle whose
 * norm is not LPC_NORM_BACKWARD.  Deterministic, no atomics: a second call gives the same bits in all six outputs, and
 * the other five are those of lpc_admm_backward.  Its workspace is allocated at the first call, counted in
 * lpc_workspace_bytes, kept across a pause and freed with the tape by lpc_admm_record(h, 0):
 *   (4 * P + C) * Hp * cpitch * 2 * sizeof(lpc_real)      bytes,
 * P = B * C planes, cpitch = Wp / 2 + 1 rounded up to a multiple of 16 (Hp, Wp: lpc_padded_shape): the work spectra
 * F V_{i+1}, F rb, F a_i, F ab and the accumulator.  lpc_admm_backward itself allocates and launches nothing of this.
 * dev_grad_psf NULL: lpc_admm_backward.  On a handle that holds one PSF per frame (lpc_set_psf_batch with
 * lpc_per_frame_grad) nothing is summed over the batch: the accumulator is P planes, one thread per spectral point and
 * state plane adds its frame's term with that frame's Hs, dev_grad_psf is (B,D,H,W,C), and the workspace is
 * (4 * P + P) * Hp * cpitch * 2 * sizeof(lpc_real) bytes. */
int lpc_admm_backward_psf(lpc_handle h, const lpc_real* dev_grad_out, lpc_real* dev_grad_data, lpc_real* dev_grad_mu1,
                          lpc_real* dev_grad_mu2, lpc_real* dev_grad_mu3, lpc_real* dev_grad_tau,
                          lpc_real* dev_grad_psf,    /* (D,H,W,C): w.r.t. the PSF; per-frame PSFs: (B,D,H,W,C)   */
                          void* stream);

/* ---- the hot loop: `for i in range(n_iter): self._update(i)`  recon.py:575-576 ------ */
/* exactly n_iter iterations, asynchronous on `stream`; no early exit exists on this path */
int lpc_iterate(lpc_handle h, int n_iter, void* stream);

/* Plug-and-play hook (gradient-descent family): ONE iteration split where the reference calls
 * `self._form_image()` = `self._proj(self._image_est[, noise_level])` inside `_update` (gd.py:132-140,183-188,
 * 235-241; `proj=` argument gd.py:67, external denoiser gd.py:89-92).  lpc_iterate_begin runs the fused gradient /
 * momentum half and leaves the UNPROJECTED estimate readable as lpc_get_state("image_est"); the caller applies its
 * projection or denoiser to that (B,D,H,W,C) array and passes the result to lpc_iterate_end, which completes the
 * iteration (FISTA: the extrapolation and the t_k recursion).  Mixing with lpc_iterate between the two is an error;
 * whole iterations of either kind may follow one another.  On a handle with an unrolled schedule
 * (lpc_set_fista_schedule) a split iteration takes its step and its momentum factor from the schedule's entry of that
 * iteration, like a fused one; a handle that records a tape (lpc_fista_record) refuses lpc_iterate_begin: only the fused
 * projection is differentiated. */
int lpc_iterate_begin(lpc_handle h, void* stream);
int lpc_iterate_end(lpc_handle h, const lpc_real* dev_projected, void* stream);

/* Plug-and-play ADMM (admm.py:126-133,235-243,266-275,300-311): ONE iteration split at the U-update, where the
 * reference calls the external denoiser.  lpc_admm_pnp_begin writes the denoiser's input as (B,D,Hp,Wp,C):
 * U + eta/mu2 if use_dual, else the image estimate; the caller runs its denoiser and hands U (same shape) to
 * lpc_admm_pnp_end, which does the X / W updates, the spectral image update and the dual updates exactly as the
 * reference's branch is written (U and eta image-shaped, Psi^T = identity; use_dual: r_k = (mu3 W - rho) + mu2 U - eta,
 * else r_k = mu2 U + H^T(mu1 X - xi)).  A handle runs either these or lpc_iterate between two resets, not both.
 * lpc_get_state then serves "U","eta","X","W","xi","rho","forward_out","image_est" as (B,D,Hp,Wp,C). */
int lpc_admm_pnp_begin(lpc_handle h, int use_dual, lpc_real* dev_denoiser_in, void* stream);
int lpc_admm_pnp_end(lpc_handle h, int use_dual, const lpc_real* dev_U, void* stream);

/* ADMM with a caller-supplied sparsifying operator `psi / psi_adj / psi_gram` (admm.py:44-46,104-120): the operator
 * cannot be fused, so the caller keeps U, eta and Psi(V) (their shape is the operator's) and runs Psi, Psi^T and the
 * soft-threshold itself; the engine does everything else of `_update` (admm.py:252-329) in one call:
 *   lpc_set_psi_gram   |psi_gram(padded_shape)| (real, (Hp, Wc), NATURAL frequency order, one plane shared by all
 *                      channels) replaces the finite-difference gram in R_divmat (admm.py:186-190).  Call after
 *                      lpc_set_psf (which restores the default gram).  Synchronises `stream` once: the engine checks
 *                      on the device whether the plane is a row term + a column term (the finite-difference gram is)
 *                      and, for planes above 8 MB, lets its fused middles read the two vectors instead (option g_plane).
 *   lpc_admm_psi_step  dev_psit = Psi^T(mu2 U - eta) as (B,D,Hp,Wp,C): X and W updates, r_k = (mu3 W - rho) + dev_psit +
 *                      H^T(mu1 X - xi), the spectral image update, the xi and rho updates.  The new estimate is
 *                      lpc_get_state("image_est"); the caller then updates Psi(V) and eta (admm.py:302-308).
 * A handle runs either these or lpc_iterate between two resets. */
int lpc_set_psi_gram(lpc_handle h, const lpc_real* dev_gabs, void* stream);
int lpc_admm_psi_step(lpc_handle h, const lpc_real* dev_psit, void* stream);

/* _form_image(): ADMM crop + clamp (admm.py:331-338), GD family projection (gd.py:136-140).
 * dev_out: (B,D,H,W,C).  Like the reference, the ADMM clamp is an in-place side effect on the image
 * estimate: it is visible to the W-update of the following iterations (and to "image_est"). */
int lpc_form_image(lpc_handle h, lpc_real* dev_out, void* stream);

/* inspection (tests, warm starts).  name: "image_est" (solver state shape), and for ADMM
 * "X","xi","rho","forward_out","W" as (B,D,Hp,Wp,C), "U","eta" as (B,D,Hp,Wp,C,2)
 * [values as the reference holds them after the same number of iterations].
 * GD family: "alpha" and "start_value" (the default start value per channel) write C floats. */
int lpc_get_state(lpc_handle h, const char* name, lpc_real* dev_out, void* stream);

/* ---- evaluation reductions on the device (no host synchronisation of the results) -------------- */
/* ReconstructionAlgorithm.reconstruction_error (recon.py:607-653):
 *   out[b] = sum_{d,h,w,c} (N(H x)[b,d] - y[b])^2 / (D*H*W*C),  N(z) = (z - min z) / max(z - min z) over (H,W,C)
 * (N = identity when normalize == 0).  dev_pred: (B,D,H,W,C), e.g. what lpc_form_image wrote; dev_data:
 * (B,H,W,C) or NULL = the frame given to lpc_set_data; dev_out: B values.  Works on every handle kind. */
int lpc_reconstruction_error(lpc_handle h, const lpc_real* dev_pred, const lpc_real* dev_data, int normalize,
                             lpc_real* dev_out, void* stream);
/* mse() and psnr() of lensless/eval/metric.py:119-172 for n_items image pairs of n values each:
 * dev_out[2*i] = mean((t/max t - e/max e)^2), dev_out[2*i+1] = 10 log10(R^2 / mse) with R = 1 if min t >= 0 else 2
 * (skimage's data-range rule for float images); normalize == 0 skips the division by the maxima.
 * Handle-free and asynchronous on `stream` (scratch comes from the device's stream-ordered memory pool). */
int lpc_image_metrics(const lpc_real* dev_true, const lpc_real* dev_est, long n, int n_items, int normalize,
                      lpc_real* dev_out, void* stream);

/* ---- raw-frame preparation on the device: the step in front of lpc_set_psf / lpc_set_data -------------
 * Restates lensless/utils/io.py load_image (:157-196), load_psf (:283-375) and their chaining in load_data
 * (:462-552), minus file decoding, Bayer demosaicing and resizing.  Handle-free, asynchronous on `stream` (scratch
 * comes from the device's stream-ordered memory pool); results stay on the device. */
enum lpc_raw_type { LPC_RAW_U8 = 0, LPC_RAW_U16 = 1, LPC_RAW_F32 = 2, LPC_RAW_F64 = 3 };
typedef struct lpc_prep_config {
  int raw_type;          /* enum lpc_raw_type of the raw buffer                                        */
  int height, width;     /* of the raw buffer == of the result (no resizing)                            */
  int channels;          /* of the raw buffer, channels-last: 1 or 3                                    */
  int flip_ud, flip_lr;  /* io.py:160-166 (load_image's flip = both)                                    */
  int bgr_input;         /* 3 channels arrive as BGR (io.py:153-154)                                    */
  int gray;              /* rgb2gray AFTER normalisation, weights 0.299/0.587/0.114 (io.py:550-552)      */
  int normalize;         /* frames: divide by the frame's maximum (io.py:196-197)                        */
  int single_psf;        /* PSF: sum the colour channels into one (io.py:355-364)                        */
  int out_channels;      /* PSF with single_psf: replicate it over 1 or 3 channels (io.py:553-559)       */
  int bg_pix0, bg_pix1;  /* PSF: background level = mean of [p0:p1, p0:p1] per channel (io.py:331-350);  */
                         /* p1 <= p0: no background estimation (bg_pix=None)                             */
} lpc_prep_config;
/* n raw frames (n,H,W,C) -> dev_out (n,H,W,C') lpc_real, C' = 1 if gray else C.  dev_bg: C background levels on the
 * device (what lpc_preprocess_psf wrote: fractions of full scale, re-scaled by get_max_val of each integer frame,
 * image.py:251-278; values > 1 are taken as pixel units) or NULL.  Background removal clips at 0 (io.py:175). */
int lpc_preprocess_frames(const lpc_prep_config* cfg, const void* dev_raw, int n, const lpc_real* dev_bg,
                          lpc_real* dev_out, void* stream);
/* raw PSF stack (D,H,W,C) -> dev_psf_out (D,H,W,C') with unit l2 norm; dev_bg_out (may be NULL): the C background
 * levels divided by the stack's full-scale value (io.py:368). */
int lpc_preprocess_psf(const lpc_prep_config* cfg, const void* dev_raw, int depth, lpc_real* dev_psf_out,
                       lpc_real* dev_bg_out, void* stream);

/* resize (lensless/utils/image.py:28-80, the torch branch): anti-aliased bilinear resampling of n channels-last images
 * (n,H,W,C) -> (n,Hout,Wout,C), last axis first, result clipped to the input's [min, max].  This is what
 * load_psf(downsample=...) / load_data's "resize the frame to the PSF" do through torchvision's
 * Resize(size, antialias=True) = torch.nn.functional.interpolate(mode="bilinear", antialias=True).  Handle-free,
 * asynchronous on `stream`. */
int lpc_resize_aa(const lpc_real* dev_in, int n, int H, int W, int C, int Hout, int Wout, lpc_real* dev_out,
                  void* stream);

/* ---- measurement support (bench.py roofline leg) ----------------------------------- */
enum lpc_kernel_id {
  LPC_K_SPATIAL = 0,   /* fused prox/update kernel (ADMM) / fused update (GD family)  */
  LPC_K_ROW_FWD = 1,
  LPC_K_COL_A_FWD = 2,
  LPC_K_COL_MID = 3,
  LPC_K_COL_A_INV = 4,
  LPC_K_ROW_INV = 5,
  LPC_K_COUNT = 6
};
/* on = 1: every launch of the hot loop is bracketed by hipEvents on its stream; on = 2 << k (or a sum of such terms):
 * only the launches of kernel id k -- two event records per launch cost a 12-MP iteration 1.4 % (ADMM, 6 launches) to
 * 3.4 % (FISTA, 8 launches), so a timed region brackets the one kernel it reports; on = 0: off.  Resets the counts. */
int lpc_profile_enable(lpc_handle h, int on);
/* average milliseconds per launch and launch counts since the last enable; arrays of LPC_K_COUNT */
int lpc_profile_read(lpc_handle h, double* avg_ms, long* launches);
/* algorithmic HBM bytes one launch of kernel k moves */
int lpc_kernel_bytes(lpc_handle h, int kernel_id, double* bytes);
/* SURVEY.md section 8(d)'s algorithmic bytes of ONE solver iteration of all frames of the handle (the yardstick the
 * whole iteration is scored against): ADMM 19R + R0 + 13.5S, Nesterov / FISTA 8R0 + 14S, vanilla GD 6R0 + 14S, with
 * R = padded real array, S = half spectrum, R0 = un-padded array (all planes).  Independent of how many passes the
 * engine really makes. */
int lpc_model_bytes(lpc_handle h, double* bytes);
/* one-line description of the launch plan the handle chose (row scheme, column split, which passes run on compile-time
 * plans, whether the ADMM image-domain kernel is fused into the rows) -- for logs and tests */
int lpc_plan_info(lpc_handle h, char* buf, size_t n);
/* bytes of HBM the handle owns */
int lpc_workspace_bytes(lpc_handle h, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* LPC_H_ */
