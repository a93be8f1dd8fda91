// lpc_gd_host.cpp -- host side of the gradient-descent family (vanilla / Nesterov / FISTA): workspace, step constants,
// the iteration sequences and the unrolled schedule.  The fused row kernels are launched from lpc_gd.cpp and
// lpc_gd_update*.cpp; the reverse mode of the unrolled iterations is lpc_gd_bwd.cpp, which gd_reset and gd_iterate hand what
// it records.
#include "lpc_engine.h"
#include "lpc_gd_kernels.h"

int gd_alloc(Engine* e) {
  const PlaneGeom& g = e->g;
  const size_t up = (size_t)g.uplane * e->P;
  LPC_OK(dev_alloc(e, &e->gd.gx, up));
  LPC_OK(dev_alloc(e, &e->gd.gaux, up));
  LPC_OK(dev_alloc(e, &e->gd.galpha, 4));
  LPC_OK(dev_alloc(e, &e->gd.gx0, 4));
  LPC_OK(dev_alloc(e, &e->gd.S2, (size_t)g.cplane * e->P));
  return 0;
}

// alpha = lip_fact / max|H* H| per channel (gd.py:107-112); x0 = (max psf + min psf)/2 (gd.py:100-105)
int gd_setup_constants(Engine* e) {
  const int nblk = 64;
  real* partial = (real*)e->gd.S2;  // scratch: 2 * Ppsf * nblk floats
  LPC_OK(plane_minmax(e, e->Hs, nullptr, nblk, e->Ppsf, partial));
  LPC_OK(launch_k(e, -1, k_channel_finish, dim3(1), 64, 0, (const real*)partial, nblk, e->cfg.depth,
                  e->cfg.channels, 0, (real)e->cfg.lip_fact, e->gd.galpha));
  if (e->gd.gx0_pinned) return 0;   // unrolled FISTA: the constructor's start value stays (unrolled_fista.py:55-59)
  LPC_OK(plane_minmax(e, nullptr, e->psf_planar, nblk, e->Ppsf, partial));
  LPC_OK(launch_k(e, -1, k_channel_finish, dim3(1), 64, 0, (const real*)partial, nblk, e->cfg.depth,
                  e->cfg.channels, 1, (real)0., e->gd.gx0));
  return 0;
}

int gd_apply_momentum_reset(Engine* e) {
  if (e->cfg.algo == LPC_ALGO_NESTEROV && e->gd.gaux) {
    return fill_planar(e, e->gd.gaux, (long)e->g.uplane * e->P, (real)e->gd.nest_p);
  }
  return 0;
}

// ---- the unrolled schedule (FistaSchedule) ----
int gd_set_schedule(Engine* e, int n, const real* alpha, const real* coef) {
  FistaSchedule& f = e->fista;
  f.coef.clear();
  f.sched_n = 0;
  e->fista_tape.invalidate();      // what was recorded with another schedule no longer matches (lpc_fista_backward refuses)
  if (n <= 0) return 0;
  if (!alpha || !coef) return fail("lpc_set_fista_schedule: null array");
  const size_t na = (size_t)n * e->cfg.channels;
  if (f.galpha_sched && f.sched_cap < na) {   // grown: give the old table back
    dev_free(e, f.galpha_sched);
    f.galpha_sched = nullptr;
  }
  if (!f.galpha_sched) {
    LPC_OK(dev_alloc(e, &f.galpha_sched, na));
    f.sched_cap = na;
  }
  LPC_OK(upload(e, f.galpha_sched, alpha, na * sizeof(real)));
  f.coef.assign(coef, coef + n);
  f.alpha.assign(alpha, alpha + na);
  f.sched_n = n;
  return 0;
}

int gd_reset(Engine* e) {
  const PlaneGeom& g = e->g;
  const size_t ub = (size_t)g.uplane * e->P * sizeof(real);
  if (e->has_init) {
    LPC_RT(rt::copy_d2d_async(e->gd.gx, e->init_est, ub, e->stream));
  } else {
    LPC_OK(launch_k(e, -1, k_fill_per_channel<256>, grid1d(g.uplane, 256, e->P), 256, 0, e->gd.gx, g.uplane,
                    e->cfg.channels, (const real*)e->gd.gx0));
  }
  if (e->fista.sched_n > 0)  // unrolled FISTA: x_k starts as the initial image (unrolled_fista.py:91-96)
    LPC_RT(rt::copy_d2d_async(e->gd.gaux, e->gd.gx, ub, e->stream));
  else
    LPC_RT(rt::memset_async(e->gd.gaux, 0, ub, e->stream));
  // gd.py:178-181: NesterovGradientDescent.reset(p=0, mu=0.9) -- the defaults win over the
  // constructor arguments because the base constructor calls reset() bare (recon.py:328-329)
  e->gd.nest_p = 0.0;
  e->gd.nest_mu = 0.9;
  e->gd.tk = e->cfg.fista_tk;  // gd.py:227-232
  e->first = true;
  e->gd.split_pending = false;
  e->gd.fwd_done = false;
  e->iters_done = 0;
  return gd_tape_reset(e);
}

// split == 1: one iteration up to (not including) the projection; gd_finish_split completes it
int gd_iterate(Engine* e, int n_iter, int split) {
  const PlaneGeom& g = e->g;
  for (int it = 0; it < n_iter; ++it) {
    // H x  (the row spectra are already there when the previous iteration's update kernel produced them)
    if (!e->gd.fwd_done) LPC_OK(rows_fwd_single(e, src_unpadded(e, e->gd.gx), e->S, e->P, LPC_K_ROW_FWD));
    e->gd.fwd_done = false;
    LPC_OK(conv_middle(e, e->S, e->P, false, g.sh, g.sh + g.H, true));
    // (H x - y), straight back into the frequency domain
    LPC_OK(gd_rows_mid(e, e->S, e->gd.S2));
    // H^T (.)
    LPC_OK(conv_middle(e, e->gd.S2, e->P, true, g.sh, g.sh + g.H, true));
    GdScalars sc;
    sc.kind = e->cfg.algo - LPC_ALGO_GD;
    sc.mu = (real)e->gd.nest_mu;
    sc.negmu = (real)(-e->gd.nest_mu);
    sc.onepmu = (real)(1.0 + e->gd.nest_mu);
    const double tk_new = (1.0 + std::sqrt(1.0 + 4.0 * e->gd.tk * e->gd.tk)) / 2.0;  // gd.py:238
    sc.coef = (real)((e->gd.tk - 1.0) / tk_new);
    sc.first = e->first ? 1 : 0;
    sc.split = split;
    const real* alpha = e->gd.galpha;
    if (e->fista.sched_n > 0) {
      const long i = std::min<long>(e->iters_done, e->fista.sched_n - 1);
      sc.coef = e->fista.coef[(size_t)i];
      sc.first = 0;
      alpha = e->fista.galpha_sched + i * e->cfg.channels;
    }
    if (e->plan.gd_fuse_fwd && !split) {
      LPC_OK(e->mod->gd_rows_update_fwd(e, &sc, alpha));   // (LaunchPlan::gd_fuse_fwd: the module holds it)
      e->gd.fwd_done = true;
    } else {
      LPC_OK(gd_rows_update(e, sc, alpha));
    }
    if (split) { e->gd.split_pending = true; return 0; }
    if (e->cfg.algo == LPC_ALGO_FISTA) e->gd.tk = tk_new;
    e->first = false;
    LPC_OK(gd_tape_push(e));     // (recording: stream-ordered copies; the kernels are the unrecorded forward's)
    ++e->iters_done;
  }
  return 0;
}

int gd_finish_split(Engine* e, const real* dev_projected) {
  const PlaneGeom& g = e->g;
  const double tk_new = (1.0 + std::sqrt(1.0 + 4.0 * e->gd.tk * e->gd.tk)) / 2.0;  // gd.py:238
  real coef = (real)((e->gd.tk - 1.0) / tk_new);
  if (e->fista.sched_n > 0)    // unrolled FISTA: this iteration's factor, as gd_iterate takes it (x_k started as the initial image)
    coef = e->fista.coef[(size_t)std::min<long>(e->iters_done, e->fista.sched_n - 1)];
  LPC_OK(launch_k(e, -1, k_gd_post<256>, grid1d(g.uplane, 256, e->P), 256, 0, g, dev_projected, e->gd.gx, e->gd.gaux,
                  e->cfg.algo - LPC_ALGO_GD, coef));
  if (e->cfg.algo == LPC_ALGO_FISTA) e->gd.tk = tk_new;
  e->first = false;
  e->gd.split_pending = false;
  e->gd.fwd_done = false;
  ++e->iters_done;
  return 0;
}

int gd_form_image(Engine* e, real* dev_out) {     // projection (gd.py:136-140)
  const PlaneGeom& g = e->g;
  return planar_to_hwc(e, e->gd.gx, dev_out, e->cfg.batch * e->cfg.depth, g.H, g.W, g.W, g.uplane, 0, 0, 1);
}

int gd_get_state(Engine* e, const std::string& nm, real* dev_out) {
  const PlaneGeom& g = e->g;
  const int nimg = e->cfg.batch * e->cfg.depth;
  if (nm == "image_est") return planar_to_hwc(e, e->gd.gx, dev_out, nimg, g.H, g.W, g.W, g.uplane, 0, 0, 0);
  if (nm == "alpha" || nm == "start_value") {
    LPC_RT(rt::copy_d2d_async(dev_out, nm == "alpha" ? e->gd.galpha : e->gd.gx0, e->cfg.channels * sizeof(real), e->stream));
    return 0;
  }
  return fail("lpc_get_state: unknown name '" + nm + "'");
}

int gd_kernel_bytes(Engine* e, int kid, double* bytes) {
  const PlaneGeom& g = e->g;
  const double f = (double)g.H / g.Hp;               // fraction of spectrum rows that carry data
  const double eb = (double)sizeof(real);
  const double S = 2 * eb * g.Hp * g.Wc * e->P;
  const double R0 = eb * g.H * g.W * e->P;
  const double Sc = 2 * eb * g.Hp * g.Wc * e->Ppsf;
  const bool split = e->plan.N1 > 1;
  const int kind = e->cfg.algo - LPC_ALGO_GD;
  double b = 0.0;
  switch (kid) {
    // update: gradient rows + x (+aux) read / write (+ the next iteration's row spectra when its forward rows are fused in)
    case LPC_K_SPATIAL: b = f * S + (kind == 0 ? 2.0 : 4.0) * R0 + (e->plan.gd_fuse_fwd ? f * S : 0.0); break;
    case LPC_K_ROW_FWD: b = R0 + f * S; break;
    case LPC_K_COL_A_FWD: b = split ? (f * S + S) : 0.0; break;
    case LPC_K_COL_MID: b = (split ? 2.0 * S : (f * S + S)) + Sc; break;
    case LPC_K_COL_A_INV: b = split ? (S + f * S) : 0.0; break;            // stores only the rows the crop keeps
    case LPC_K_ROW_INV: b = 2.0 * f * S + R0; break;                     // residual pass: rows in, y, rows out
    default: return fail("bad kernel id");
  }
  *bytes = b;
  return 0;
}

double gd_model_bytes(const Engine* e) {
  const PlaneGeom& g = e->g;
  const double eb = (double)sizeof(real), S = 2 * eb * g.Hp * g.Wc * e->P;
  // one PSF per frame: each of the two middles reads a spectrum of H per state plane (shared: once per batch, not counted)
  const double Sc = e->psf_per_frame ? 2 * eb * g.Hp * g.Wc * e->Ppsf : 0.0;
  return (e->cfg.algo == LPC_ALGO_GD ? 6.0 : 8.0) * eb * g.H * g.W * e->P + 14.0 * S + 2.0 * Sc;
}
