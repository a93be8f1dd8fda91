// lpc_abi.cpp -- the C ABI declared in include/lpc.h: argument checks, the call's stream, dispatch by algorithm, the
// life cycle of a handle and the profile read-out.  Nothing here launches a kernel or holds arithmetic of a method: that
// lives in the unit of the role (lpc_engine.h).  lpc_reconstruction_error, lpc_image_metrics, lpc_preprocess_* and
// lpc_resize_aa: lpc_eval.cpp.
#include "lpc_engine.h"

// --------------------------------------------------------------------------- errors --
static thread_local std::string g_last_error;
int fail(const std::string& msg) {
  g_last_error = msg;
  return 1;
}

// process-wide defaults from the environment first (the ONE launch-plan variable the library reads), then the handle's own
static std::string parse_all_opts(const char* handle_opts, EngineOpts& o) {
  std::string err = parse_engine_opts(std::getenv("LPC_OPTIONS"), o);
  return err.empty() ? parse_engine_opts(handle_opts, o) : err;
}

// =============================================================================== C ABI ==
extern "C" {

const char* lpc_last_error(void) { return g_last_error.c_str(); }
const char* lpc_backend(void) { return rt::backend_name(); }
const char* lpc_real_name(void) { return LPC_REAL_NAME; }

int lpc_create(const lpc_config* cfg, lpc_handle* out) {
  if (!cfg || !out) return fail("lpc_create: null argument");
  *out = nullptr;
  if (cfg->height < 1 || cfg->width < 1) return fail("lpc_create: bad spatial size");
  if (cfg->channels != 1 && cfg->channels != 3) return fail("PSF must either be rgb (3) or grayscale (1)");
  if (cfg->depth < 1 || cfg->batch < 1) return fail("lpc_create: depth and batch must be >= 1");
  if (cfg->algo < LPC_ALGO_CONV || cfg->algo > LPC_ALGO_FISTA) return fail("lpc_create: unknown algo");
  if (cfg->norm < 0 || cfg->norm > 2) return fail("lpc_create: unknown norm");
  int ndev = 0;
  if (rt::device_count(&ndev) != lpcSuccess || ndev < 1)
    return fail("no HIP device: the engine has no CPU path");
  Engine* e = new Engine();
  e->cfg = *cfg;
  e->cfg.options = nullptr;            // (the caller's string is not kept)
  {   // process-wide defaults from the environment first, then the handle's own
    std::string err = parse_all_opts(cfg->options, e->opt);
    if (!err.empty()) { delete e; return fail("lpc_create: " + err); }
  }
  e->gd.tk = cfg->fista_tk; e->gd.nest_mu = cfg->nesterov_mu; e->gd.nest_p = cfg->nesterov_p;
  int rc = setup_geometry(e);
  if (!rc) rc = alloc_common(e);
  if (!rc && cfg->algo == LPC_ALGO_ADMM) rc = admm_alloc(e);
  if (!rc && cfg->algo >= LPC_ALGO_GD) rc = gd_alloc(e);
  if (rc) {
    lpc_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

// the plan module lpc_create(cfg) would use: its key, and (build != 0) compile it now if it is not on disk.  No device
// needed: build.py pre-builds the modules of BASELINE.json's shapes with it in the GPU-less build container.
int lpc_plan_module(const lpc_config* cfg, int build, char* key_buf, size_t n) {
  if (!cfg) return fail("lpc_plan_module: null config");
  if (cfg->height < 1 || cfg->width < 1 || cfg->depth < 1 || cfg->batch < 1) return fail("lpc_plan_module: bad size");
  EngineOpts opt;
  std::string err = parse_all_opts(cfg->options, opt);
  if (!err.empty()) return fail("lpc_plan_module: " + err);
  ShapePlan sp;
  LPC_OK(setup_shape(*cfg, opt, plan_cu_count(), &sp));
  const bool any = sp.want_static && sp.plan.spec.any();
  if (key_buf && n) std::snprintf(key_buf, n, "%s", any ? plan_spec_key(sp.plan.spec).c_str() : "");
  if (!any || !build) return 0;
  std::string path;
  if (build_plan_module(sp.plan.spec, opt, &path) != 0) return fail(path);
  return 0;
}

int lpc_destroy(lpc_handle e) {
  if (!e) return 0;
  (void)rt::stream_sync(e->stream);
  for (auto& a : e->allocs) (void)rt::dev_free(a.first);
  release_plan_module(e->mod);
  e->mod = nullptr;
#if !defined(LPC_SIMT_EMU)
  for (auto& v : e->timer.ev)
    for (auto& pr : v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
#endif
  delete e;
  return 0;
}

int lpc_padded_shape(lpc_handle e, int* Hp, int* Wp, int* sh, int* sw) {
  if (!e) return fail("null handle");
  if (Hp) *Hp = e->g.Hp;
  if (Wp) *Wp = e->g.Wp;
  if (sh) *sh = e->g.sh;
  if (sw) *sw = e->g.sw;
  return 0;
}

int lpc_workspace_bytes(lpc_handle e, size_t* bytes) {
  if (!e || !bytes) return fail("null argument");
  *bytes = e->total_bytes;
  return 0;
}

int lpc_set_psf(lpc_handle e, const real* dev_psf, void* stream) {
  if (!e || !dev_psf) return fail("lpc_set_psf: null argument");
  e->stream = (lpcStream_t)stream;
  LPC_OK(set_psf(e, dev_psf));
  if (e->cfg.algo == LPC_ALGO_ADMM) LPC_OK(admm_setup_constants(e));
  if (e->cfg.algo >= LPC_ALGO_GD) LPC_OK(gd_setup_constants(e));
  if (e->cfg.algo != LPC_ALGO_CONV) return lpc_reset(e, stream);
  return 0;
}

// One PSF per frame (include/lpc.h).  What such a handle does not do names the reason with the word "per-frame"
// -- unless lpc_per_frame_grad switched their gradients on
static int per_frame_refusal(const Engine* e, const char* who) {
  if (!e->psf_per_frame || e->per_frame_grad) return 0;
  return fail(std::string(who) + ": not available with per-frame PSFs (lpc_set_psf_batch): their gradients are not implemented");
}
// the gradient-descent family takes its step and its default start value from ONE PSF (gd.py:100-112): with one PSF per
// frame both must come from the caller -- unrolled FISTA's schedule and pinned start value (unrolled_fista.py:57-72)
static int per_frame_gd_check(const Engine* e, const char* who) {
  if (e->cfg.algo < LPC_ALGO_GD || (e->gd.gx0_pinned && e->fista.sched_n > 0)) return 0;
  return fail(std::string(who) + ": per-frame PSFs need a pinned start value (lpc_set_start_value) and a schedule "
              "(lpc_set_fista_schedule) on a gradient-descent handle: plain iterations take their step and start value from one PSF");
}

int lpc_set_psf_batch(lpc_handle e, const real* dev_psfs, void* stream) {
  if (!e || !dev_psfs) return fail("lpc_set_psf_batch: null argument");
  LPC_OK(per_frame_gd_check(e, "lpc_set_psf_batch"));
  if ((e->fista_tape.rec_on || e->admm_tape.rec_on) && !e->per_frame_grad)
    return fail("lpc_set_psf_batch: the handle records a tape, and gradients with per-frame PSFs are not implemented");
  e->stream = (lpcStream_t)stream;
  // |PsiT Psi| does not depend on the PSF: the finite-difference gram is made by the first PSF a handle gets, and a
  // caller's gram (lpc_set_psi_gram) stays; otherwise nothing here waits for the stream
  const bool gram = e->cfg.algo == LPC_ALGO_ADMM && !e->psf_set;
  LPC_OK(set_psf_batch(e, dev_psfs));
  e->admm.midc_valid = false;
  e->fista_tape.invalidate();
  e->admm_tape.invalidate();
  if (gram) LPC_OK(admm_setup_constants(e));
  if (e->cfg.algo != LPC_ALGO_CONV) return lpc_reset(e, stream);
  return 0;
}

int lpc_per_frame_grad(lpc_handle e, int on) {
  if (!e) return fail("null handle");
  e->per_frame_grad = on != 0;
  return 0;
}

int lpc_convolve(lpc_handle e, const real* dev_x, real* dev_out, int n, int x_channels, int adjoint, void* stream) {
  if (!e || !dev_x || !dev_out) return fail("lpc_convolve: null argument");
  LPC_OK(check_channels(e, x_channels, "lpc_convolve"));
  if (!e->psf_set) return fail("lpc_convolve: PSF not set");
  if (n < 1 || n > e->cfg.batch) return fail("lpc_convolve: n exceeds the configured batch");
  if (e->cfg.algo != LPC_ALGO_CONV) return fail("lpc_convolve: handle was not created with LPC_ALGO_CONV");
  e->stream = (lpcStream_t)stream;
  return convolve_hwc(e, dev_x, dev_out, n, x_channels, adjoint != 0, false);
}

int lpc_convolve_spectrum(lpc_handle e, const real* dev_x, real* dev_out, int n, int x_channels, int adjoint,
                          void* stream) {
  if (!e || !dev_x || !dev_out) return fail("lpc_convolve_spectrum: null argument");
  LPC_OK(check_channels(e, x_channels, "lpc_convolve_spectrum"));
  if (!e->psf_set) return fail("lpc_convolve_spectrum: PSF not set");
  if (n < 1 || n > e->cfg.batch) return fail("lpc_convolve_spectrum: n exceeds the configured batch");
  if (e->cfg.algo != LPC_ALGO_CONV) return fail("lpc_convolve_spectrum: handle was not created with LPC_ALGO_CONV");
  e->stream = (lpcStream_t)stream;
  return convolve_hwc(e, dev_x, dev_out, n, x_channels, adjoint != 0, true);
}

int lpc_set_data(lpc_handle e, const real* dev_data, int data_channels, void* stream) {
  if (!e || !dev_data) return fail("lpc_set_data: null argument");
  if (e->cfg.algo == LPC_ALGO_CONV) return fail("lpc_set_data: operator-only handle");
  LPC_OK(check_channels(e, data_channels, "lpc_set_data"));
  e->stream = (lpcStream_t)stream;
  const PlaneGeom& g = e->g;
  LPC_OK(hwc_to_planar(e, dev_data, e->Y, e->cfg.batch, g.H, g.W, g.W, g.uplane, data_channels));
  e->data_set = true;
  e->data_channels = data_channels;
  e->fista_tape.invalidate();      // a tape recorded with other data no longer matches (lpc_fista_backward refuses)
  e->admm_tape.invalidate();       // ... and lpc_admm_backward
  return 0;
}

int lpc_set_initial_estimate(lpc_handle e, const real* dev_est, void* stream) {
  if (!e) return fail("null handle");
  if (e->cfg.algo == LPC_ALGO_CONV) return fail("lpc_set_initial_estimate: operator-only handle");
  e->stream = (lpcStream_t)stream;
  const PlaneGeom& g = e->g;
  if (!dev_est) { e->has_init = false; return 0; }
  const bool admm = e->cfg.algo == LPC_ALGO_ADMM;
  const size_t n = (size_t)(admm ? g.rplane : g.uplane) * e->P;
  if (!e->init_est) LPC_OK(dev_alloc(e, &e->init_est, n));
  const int nimg = e->cfg.batch * e->cfg.depth;
  if (admm) LPC_OK(hwc_to_planar(e, dev_est, e->init_est, nimg, g.Hp, g.Wp, g.rpitch, g.rplane));
  else LPC_OK(hwc_to_planar(e, dev_est, e->init_est, nimg, g.H, g.W, g.W, g.uplane));
  e->has_init = true;
  return 0;
}

int lpc_reset(lpc_handle e, void* stream) {
  if (!e) return fail("null handle");
  if (!e->psf_set) return fail("lpc_reset: PSF not set");
  e->stream = (lpcStream_t)stream;
  if (e->cfg.algo == LPC_ALGO_ADMM) return admm_reset(e);
  if (e->cfg.algo >= LPC_ALGO_GD) return gd_reset(e);
  return 0;
}

int lpc_set_momentum(lpc_handle e, double p, double mu, double tk) {
  if (!e) return fail("null handle");
  e->gd.nest_p = p; e->gd.nest_mu = mu;
  if (tk > 0) e->gd.tk = tk;
  return gd_apply_momentum_reset(e);
}

int lpc_set_start_value(lpc_handle e, const real* dev_start, void* stream) {
  if (!e) return fail("null handle");
  if (e->cfg.algo < LPC_ALGO_GD) return fail("lpc_set_start_value: gradient-descent family only");
  e->stream = (lpcStream_t)stream;
  e->gd.gx0_pinned = dev_start != nullptr;
  if (dev_start) LPC_RT(rt::copy_d2d_async(e->gd.gx0, dev_start, e->cfg.channels * sizeof(real), e->stream));
  return 0;
}

int lpc_set_admm_schedule(lpc_handle e, int n, const double* mu1, const double* mu2, const double* mu3,
                          const double* tau) {
  if (!e) return fail("null handle");
  if (e->cfg.algo != LPC_ALGO_ADMM) return fail("lpc_set_admm_schedule: not an ADMM handle");
  for (auto& v : e->admm.sched) v.clear();
  e->admm_tape.invalidate();      // a tape recorded with another schedule no longer matches (lpc_admm_backward refuses)
  if (n <= 0) return 0;
  if (!mu1 || !mu2 || !mu3 || !tau) return fail("lpc_set_admm_schedule: null array");
  for (int i = 0; i < n; ++i) {
    if (!(mu1[i] > 0) || !(mu2[i] > 0) || !(mu3[i] > 0)) return fail("lpc_set_admm_schedule: step sizes must be > 0");
    e->admm.sched[0].push_back(mu1[i]); e->admm.sched[1].push_back(mu2[i]);
    e->admm.sched[2].push_back(mu3[i]); e->admm.sched[3].push_back(tau[i]);
  }
  return 0;
}

int lpc_set_fista_schedule(lpc_handle e, int n, const real* alpha, const real* coef, void* stream) {
  if (!e) return fail("null handle");
  if (e->cfg.algo != LPC_ALGO_FISTA) return fail("lpc_set_fista_schedule: not a FISTA handle");
  e->stream = (lpcStream_t)stream;
  return gd_set_schedule(e, n, alpha, coef);
}

int lpc_fista_record(lpc_handle e, int on) {
  if (!e) return fail("null handle");
  if (e->cfg.algo != LPC_ALGO_FISTA) return fail("lpc_fista_record: not a FISTA handle");
  if (on) LPC_OK(per_frame_refusal(e, "lpc_fista_record"));
  return tape_record(e, e->fista_tape, on, gd_tape_alloc);
}

// the two refusals of a backward (`who`: fista / admm) whose tape does not hold the schedule's n iterations since the last
// reset: nothing recorded at all, or (counted) not exactly n.  Two calls, because lpc_fista_backward has a refusal between
static int tape_refusal(const Engine* e, const Tape& t, long n, const std::string& who, bool counted) {
  if (!counted && (!t.rec_on || !t.buf || t.iters < 0))
    return fail("lpc_" + who + "_backward: nothing recorded (lpc_" + who + "_record(h, 1), then lpc_reset and lpc_iterate)");
  if (counted && !t.complete(n, e->iters_done))
    return fail("lpc_" + who + "_backward: " + std::to_string(e->iters_done) + " iterations since the reset, the schedule has " +
                std::to_string(n));
  return 0;
}

static int fista_backward(lpc_handle e, const real* dev_grad_out, real* dev_grad_data, real* dev_grad_alpha,
                          real* dev_grad_coef, real* dev_grad_init, real* dev_grad_psf, void* stream) {
  if (!e || !dev_grad_out || !dev_grad_alpha || !dev_grad_coef) return fail("lpc_fista_backward: null argument");
  if (e->cfg.algo != LPC_ALGO_FISTA) return fail("lpc_fista_backward: not a FISTA handle");
  LPC_OK(per_frame_refusal(e, "lpc_fista_backward"));
  if (e->fista.sched_n <= 0) return fail("lpc_fista_backward: the handle has no schedule (lpc_set_fista_schedule)");
  LPC_OK(tape_refusal(e, e->fista_tape, e->fista.sched_n, "fista", false));
  if (e->gd.split_pending) return fail("lpc_fista_backward: a split iteration is in flight (lpc_iterate_end missing)");
  LPC_OK(tape_refusal(e, e->fista_tape, e->fista.sched_n, "fista", true));
  if ((e->g.Hp | e->g.Wp) & 1)
    return fail("lpc_fista_backward: padded frame " + std::to_string(e->g.Hp) + " x " + std::to_string(e->g.Wp) +
                " has an odd length: convolve and deconvolve are not each other's adjoints there (not implemented)");
  if (e->cfg.depth > 1) return fail("lpc_fista_backward: depth > 1 is not implemented");
  for (real a : e->fista.alpha)
    if (a == (real)0.) return fail("lpc_fista_backward: a step alpha of the schedule is 0");
  if (dev_grad_data && !e->data_set) return fail("lpc_fista_backward: no data set");
  e->stream = (lpcStream_t)stream;
  return gd_backward(e, dev_grad_out, dev_grad_data, dev_grad_alpha, dev_grad_coef, dev_grad_init, dev_grad_psf);
}
int lpc_fista_backward(lpc_handle e, const real* dev_grad_out, real* dev_grad_data, real* dev_grad_alpha,
                       real* dev_grad_coef, real* dev_grad_init, void* stream) {
  return fista_backward(e, dev_grad_out, dev_grad_data, dev_grad_alpha, dev_grad_coef, dev_grad_init, nullptr, stream);
}
// ... and the gradient w.r.t. the PSF (dev_grad_psf null: lpc_fista_backward); same refusals, same messages
int lpc_fista_backward_psf(lpc_handle e, const real* dev_grad_out, real* dev_grad_data, real* dev_grad_alpha,
                           real* dev_grad_coef, real* dev_grad_init, real* dev_grad_psf, void* stream) {
  return fista_backward(e, dev_grad_out, dev_grad_data, dev_grad_alpha, dev_grad_coef, dev_grad_init, dev_grad_psf, stream);
}

int lpc_admm_record(lpc_handle e, int on) {
  if (!e) return fail("null handle");
  if (e->cfg.algo != LPC_ALGO_ADMM) return fail("lpc_admm_record: not an ADMM handle");
  if (on) LPC_OK(per_frame_refusal(e, "lpc_admm_record"));
  return tape_record(e, e->admm_tape, on, admm_tape_alloc);
}

static int admm_backward_checked(lpc_handle e, const real* dev_grad_out, real* dev_grad_data, real* dev_grad_mu1,
                                 real* dev_grad_mu2, real* dev_grad_mu3, real* dev_grad_tau, real* dev_grad_psf, void* stream) {
  if (!e || !dev_grad_out || !dev_grad_mu1 || !dev_grad_mu2 || !dev_grad_mu3 || !dev_grad_tau)
    return fail("lpc_admm_backward: null argument");
  if (e->cfg.algo != LPC_ALGO_ADMM) return fail("lpc_admm_backward: not an ADMM handle");
  LPC_OK(per_frame_refusal(e, "lpc_admm_backward"));
  const long n = (long)e->admm.sched[0].size();
  if (n <= 0) return fail("lpc_admm_backward: the handle has no schedule (lpc_set_admm_schedule)");
  if (e->cfg.depth > 1) return fail("lpc_admm_backward: depth > 1 is not implemented");
  if ((e->g.Hp | e->g.Wp) & 1)
    return fail("lpc_admm_backward: padded frame " + std::to_string(e->g.Hp) + " x " + std::to_string(e->g.Wp) +
                " has an odd length: the spectral step and the convolve / deconvolve pair are not self-adjoint there "
                "(not implemented)");
  if (e->admm.custom_gram || e->admm.pnp_mode)
    return fail("lpc_admm_backward: a caller's psi and plug-and-play iterations are not differentiated");
  if (e->has_init) return fail("lpc_admm_backward: an initial estimate is set (its gradient is not implemented)");
  LPC_OK(tape_refusal(e, e->admm_tape, n, "admm", false));
  LPC_OK(tape_refusal(e, e->admm_tape, n, "admm", true));
  if (dev_grad_data && !e->data_set) return fail("lpc_admm_backward: no data set");
  if (dev_grad_psf && e->cfg.norm != LPC_NORM_BACKWARD)
    return fail("lpc_admm_backward_psf: the gradient with respect to the PSF is implemented for norm \"backward\" only");
  e->stream = (lpcStream_t)stream;
  return admm_backward(e, dev_grad_out, dev_grad_data, dev_grad_mu1, dev_grad_mu2, dev_grad_mu3, dev_grad_tau, dev_grad_psf);
}
int lpc_admm_backward(lpc_handle e, const real* dev_grad_out, real* dev_grad_data, real* dev_grad_mu1, real* dev_grad_mu2,
                      real* dev_grad_mu3, real* dev_grad_tau, void* stream) {
  return admm_backward_checked(e, dev_grad_out, dev_grad_data, dev_grad_mu1, dev_grad_mu2, dev_grad_mu3, dev_grad_tau, nullptr,
                               stream);
}
// ... and the gradient w.r.t. the PSF (dev_grad_psf null: lpc_admm_backward); same refusals, same messages, plus the norm's
int lpc_admm_backward_psf(lpc_handle e, const real* dev_grad_out, real* dev_grad_data, real* dev_grad_mu1, real* dev_grad_mu2,
                          real* dev_grad_mu3, real* dev_grad_tau, real* dev_grad_psf, void* stream) {
  return admm_backward_checked(e, dev_grad_out, dev_grad_data, dev_grad_mu1, dev_grad_mu2, dev_grad_mu3, dev_grad_tau,
                               dev_grad_psf, stream);
}

int lpc_iterate(lpc_handle e, int n_iter, void* stream) {
  if (!e) return fail("null handle");
  if (n_iter < 0) return fail("lpc_iterate: negative iteration count");
  if (!e->psf_set) return fail("lpc_iterate: PSF not set");
  if (!e->data_set) return fail("Must set data with `set_data()`");
  e->stream = (lpcStream_t)stream;
  if (e->gd.split_pending) return fail("lpc_iterate: a split iteration is in flight (lpc_iterate_end missing)");
  if (e->admm.pnp_mode) return fail("lpc_iterate: the handle runs plug-and-play iterations since the last reset");
  if (e->psf_per_frame) LPC_OK(per_frame_gd_check(e, "lpc_iterate"));
  if (e->cfg.algo == LPC_ALGO_ADMM) return admm_iterate(e, n_iter);
  if (e->cfg.algo >= LPC_ALGO_GD) return gd_iterate(e, n_iter);
  return fail("lpc_iterate: operator-only handle");
}

// ---- plug-and-play hook (section 8f row N4): one iteration split at the projection ----
int lpc_iterate_begin(lpc_handle e, void* stream) {
  if (!e) return fail("null handle");
  if (e->cfg.algo < LPC_ALGO_GD) return fail("lpc_iterate_begin: gradient-descent family only");
  if (!e->psf_set) return fail("lpc_iterate_begin: PSF not set");
  if (!e->data_set) return fail("Must set data with `set_data()`");
  if (e->gd.split_pending) return fail("lpc_iterate_begin: the previous split iteration was not finished");
  if (e->psf_per_frame) LPC_OK(per_frame_gd_check(e, "lpc_iterate_begin"));
  if (e->fista_tape.rec_on)   // (the reverse sweep differentiates the fused projection only)
    return fail("lpc_iterate_begin: not available while the handle records a tape (lpc_fista_record)");
  e->stream = (lpcStream_t)stream;
  return gd_iterate(e, 1, 1);
}

int lpc_iterate_end(lpc_handle e, const real* dev_projected, void* stream) {
  if (!e || !dev_projected) return fail("lpc_iterate_end: null argument");
  if (e->cfg.algo < LPC_ALGO_GD) return fail("lpc_iterate_end: gradient-descent family only");
  if (!e->gd.split_pending) return fail("lpc_iterate_end: no split iteration in flight");
  e->stream = (lpcStream_t)stream;
  return gd_finish_split(e, dev_projected);
}

// ---- plug-and-play ADMM (section 8f row N4): one iteration split at the U-update ----
static int pnp_check(lpc_handle e, const char* who) {
  if (!e) return fail("null handle");
  if (e->cfg.algo != LPC_ALGO_ADMM) return fail(std::string(who) + ": ADMM handles only");
  if (!e->psf_set) return fail(std::string(who) + ": PSF not set");
  if (!e->data_set) return fail("Must set data with `set_data()`");
  if (!e->admm.sched[0].empty()) return fail(std::string(who) + ": not available with an unrolled schedule");
  return 0;
}

int lpc_admm_pnp_begin(lpc_handle e, int use_dual, real* dev_denoiser_in, void* stream) {
  LPC_OK(pnp_check(e, "lpc_admm_pnp_begin"));
  if (!dev_denoiser_in) return fail("lpc_admm_pnp_begin: null argument");
  if (e->admm.pnp_pending) return fail("lpc_admm_pnp_begin: the previous split iteration was not finished");
  if (!e->admm.pnp_mode && e->iters_done != 0)
    return fail("lpc_admm_pnp_begin: fused iterations already ran since the last reset");
  e->stream = (lpcStream_t)stream;
  return admm_pnp_begin(e, use_dual, dev_denoiser_in);
}

int lpc_admm_pnp_end(lpc_handle e, int use_dual, const real* dev_U, void* stream) {
  LPC_OK(pnp_check(e, "lpc_admm_pnp_end"));
  if (!dev_U) return fail("lpc_admm_pnp_end: null argument");
  if (!e->admm.pnp_pending) return fail("lpc_admm_pnp_end: no split iteration in flight");
  e->stream = (lpcStream_t)stream;
  return admm_pnp_end(e, use_dual, dev_U);
}

// ---- ADMM with a caller-supplied sparsifying operator (admm.py:104-120): one iteration around the caller's Psi / Psi^T ----
int lpc_set_psi_gram(lpc_handle e, const real* dev_gabs, void* stream) {
  if (!e || !dev_gabs) return fail("lpc_set_psi_gram: null argument");
  if (e->cfg.algo != LPC_ALGO_ADMM) return fail("lpc_set_psi_gram: ADMM handles only");
  e->stream = (lpcStream_t)stream;
  return admm_set_psi_gram(e, dev_gabs);
}

int lpc_admm_psi_step(lpc_handle e, const real* dev_psit, void* stream) {
  LPC_OK(pnp_check(e, "lpc_admm_psi_step"));
  if (!dev_psit) return fail("lpc_admm_psi_step: null argument");
  if (e->admm.pnp_pending) return fail("lpc_admm_psi_step: a plug-and-play iteration is in flight");
  if (!e->admm.pnp_mode && e->iters_done != 0)
    return fail("lpc_admm_psi_step: fused iterations already ran since the last reset");
  e->stream = (lpcStream_t)stream;
  return admm_psi_step(e, dev_psit);
}

int lpc_form_image(lpc_handle e, real* dev_out, void* stream) {
  if (!e || !dev_out) return fail("lpc_form_image: null argument");
  e->stream = (lpcStream_t)stream;
  if (e->cfg.algo == LPC_ALGO_ADMM) return admm_form_image(e, dev_out);
  if (e->cfg.algo >= LPC_ALGO_GD) return gd_form_image(e, dev_out);
  return fail("lpc_form_image: operator-only handle");
}

int lpc_get_state(lpc_handle e, const char* name, real* dev_out, void* stream) {
  if (!e || !name || !dev_out) return fail("lpc_get_state: null argument");
  e->stream = (lpcStream_t)stream;
  if (e->cfg.algo >= LPC_ALGO_GD) return gd_get_state(e, name, dev_out);
  if (e->cfg.algo == LPC_ALGO_ADMM) return admm_get_state(e, name, dev_out);
  return fail("lpc_get_state: operator-only handle");
}

int lpc_profile_enable(lpc_handle e, int on) {
  if (!e) return fail("null handle");
#if !defined(LPC_SIMT_EMU)
  for (int k = 0; k < LPC_K_COUNT; ++k) e->timer.used[k] = 0;
#endif
  e->timer.on = on != 0;
  e->timer.mask = on > 1 ? (unsigned)on >> 1 : ~0u;      // 1: every hot-loop kernel; otherwise bit k + 1 selects kernel id k
  return 0;
}

int lpc_profile_read(lpc_handle e, double* avg_ms, long* launches) {
  if (!e || !avg_ms || !launches) return fail("null argument");
  for (int k = 0; k < LPC_K_COUNT; ++k) { avg_ms[k] = 0.0; launches[k] = 0; }
#if !defined(LPC_SIMT_EMU)
  LPC_RT(hipStreamSynchronize(e->stream));
  for (int k = 0; k < LPC_K_COUNT; ++k) {
    double tot = 0.0;
    for (size_t i = 0; i < e->timer.used[k]; ++i) {
      float ms = 0.f;  // HIP API type, not the engine's arithmetic type
      LPC_RT(hipEventElapsedTime(&ms, e->timer.ev[k][i].first, e->timer.ev[k][i].second));
      tot += ms;
    }
    launches[k] = (long)e->timer.used[k];
    avg_ms[k] = e->timer.used[k] ? tot / (double)e->timer.used[k] : 0.0;
  }
#endif
  return 0;
}

int lpc_kernel_bytes(lpc_handle e, int kid, double* bytes) {
  if (!e || !bytes) return fail("null argument");
  if (e->cfg.algo == LPC_ALGO_ADMM) return admm_kernel_bytes(e, kid, bytes);
  if (e->cfg.algo >= LPC_ALGO_GD) return gd_kernel_bytes(e, kid, bytes);
  return fail("lpc_kernel_bytes: operator-only handle");
}

int lpc_plan_info(lpc_handle e, char* buf, size_t n) {
  if (!e || !buf || n == 0) return fail("null argument");
  const PlaneGeom& g = e->g;
  const LaunchPlan& pl = e->plan;
  const PlanSpec& sp = pl.spec;
  std::string s = "padded " + std::to_string(g.Hp) + "x" + std::to_string(g.Wp);
  s += pl.rows_half ? "; rows: half-length " + std::to_string(g.Wp / 2) : "; rows: paired " + std::to_string(g.Wp);
  const bool rows_static = e->mod && sp.row_kind && (pl.rows_half || e->cfg.algo == LPC_ALGO_ADMM);
  if (rows_static) s += " [static " + rad_list(sp.row, ".") + ", " + std::to_string(sp.row.nt) + " threads]";
  if (pl.gd_v2) s += " (fused rows: second form, " + std::to_string(sp.row.n / sp.row.rad[0]) + " lanes)";
  if (pl.admm_rows_v2)
    s += std::string(" (ADMM rows: second form, ") + (pl.admm_rows_v2 == 3 ? "forward + inverse, " : pl.admm_rows_v2 == 2 ? "inverse, " : "forward, ") +
         std::to_string(sp.row.n / sp.row.rad[0]) + " lanes)";
  s += "; columns: " + (pl.N1 > 1 ? std::to_string(pl.N1) + " x " + std::to_string(pl.N2) + " split" : std::string("single pass ") + std::to_string(pl.N2));
  s += ", T = " + std::to_string(pl.T);
  if (e->mod && sp.passA.n) s += ", pass A [static " + rad_list(sp.passA, ".") + ", T = " + std::to_string(sp.passA.T) + "]";
  if (e->cfg.algo == LPC_ALGO_ADMM) {
    s += pl.admm_mid == ADMM_MID_REG24 ? ", middle in registers"
         : pl.admm_mid == ADMM_MID_MODULE ? ", LDS middle [static " + rad_list(sp.mid, ".") + (sp.mid_kind == LPC_MID_SEQ ? ", one spectrum at a time" : "") + (g.slay ? ", pair-line spectra]" : "]")
                                          : ", LDS middle";
    s += pl.k1 == ADMM_K1_ROWS ? "; TV / W half and X half inside the forward rows (three launches per iteration)"
         : pl.k1 == ADMM_K1_TV_W ? "; tiled TV / W kernel + X half inside the forward rows" : "; stand-alone image-domain kernel";
    if (pl.xi_window) s += pl.hv_skip ? " (xi inside the sensor window only, H V row transforms skipped outside it)"
                                      : " (xi inside the sensor window only)";
    if (pl.rho_rsp || pl.xi_half)
      s += std::string("; inside a call: ") + (pl.rho_rsp ? "rho read back from r_sp" : "") +
           (pl.rho_rsp && pl.xi_half ? ", " : "") + (pl.xi_half ? "xi half-applied" : "") +
           (pl.hv_fuse ? (pl.hv_fuse == 2 ? ", H V rows on chip (behind the rows of V)" : ", H V rows on chip") : "");
  }
  if (e->cfg.algo == LPC_ALGO_ADMM && e->admm.g_sep) s += "; gram as row + column terms";
  if (e->cfg.algo == LPC_ALGO_FISTA)      // lpc_fista_backward (lpc_gd_bwd.cpp: gd_bwd_rows)
    s += e->mod && e->mod->gd_bwd_head ? "; reverse rows: plan module" : pl.rows_half ? "; reverse rows: half-length, run-time plan"
                                                                                     : "; reverse rows: paired, run-time plan";
  s += e->mod ? "; plan module " + plan_spec_key(sp) : "; run-time plans (" + e->mod_note + ")";
  std::snprintf(buf, n, "%s", s.c_str());
  return 0;
}

int lpc_model_bytes(lpc_handle e, double* bytes) {
  if (!e || !bytes) return fail("null argument");
  if (e->cfg.algo == LPC_ALGO_ADMM) *bytes = admm_model_bytes(e);
  else if (e->cfg.algo >= LPC_ALGO_GD) *bytes = gd_model_bytes(e);
  else return fail("lpc_model_bytes: operator-only handle");
  return 0;
}

}  // extern "C"
