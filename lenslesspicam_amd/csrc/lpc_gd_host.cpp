// lpc_gd_host.cpp -- host side of the gradient-descent family (vanilla / Nesterov / FISTA): workspace, step constants,
// the iteration sequences, the unrolled schedule with its tape, and the reverse sweep of lpc_fista_backward.  The fused
// row kernels are launched from lpc_gd.cpp, lpc_gd_update*.cpp and lpc_gd_bwd.cpp.
#include "lpc_engine.h"
#include "lpc_gd_kernels.h"
#include "lpc_gd_bwd_kernels.h"

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

// ---- the unrolled schedule and the tape of the reverse mode (FistaSchedule) ----
int gd_set_schedule(Engine* e, int n, const real* alpha, const real* coef) {
  FistaSchedule& f = e->fista;
  f.coef.clear();
  f.sched_n = 0;
  f.tape_iters = -1;      // a tape recorded with another schedule no longer matches (lpc_fista_backward refuses)
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
void gd_tape_free(Engine* e) {
  FistaSchedule& f = e->fista;
  dev_free(e, f.psf_spec);       // the PSF gradient's workspace goes with the tape
  dev_free(e, f.psf_acc);
  f.psf_spec = nullptr; f.psf_acc = nullptr;
  if (!f.tape) return;
  dev_free(e, f.tape);
  dev_free(e, f.tape_part);
  f.tape = nullptr; f.tape_part = nullptr; f.tape_n = 0; f.tape_iters = -1;
}
// workspace of the PSF gradient (FistaSchedule::psf_spec, psf_acc; include/lpc.h: lpc_fista_backward_psf), on first use
static int gd_psf_ws_alloc(Engine* e) {
  FistaSchedule& f = e->fista;
  if (f.psf_spec) return 0;
  LPC_OK(dev_alloc(e, &f.psf_spec, (size_t)3 * e->g.cplane * e->P));
  if (dev_alloc(e, &f.psf_acc, (size_t)e->g.uplane * e->P)) {      // all or nothing
    dev_free(e, f.psf_spec);
    f.psf_spec = nullptr;
    return 1;
  }
  return 0;
}
int gd_tape_alloc(Engine* e) {
  FistaSchedule& f = e->fista;
  const int n = f.sched_n;
  if (f.tape && f.tape_n == n) return 0;
  gd_tape_free(e);
  const size_t up = (size_t)e->g.uplane * e->P;
  LPC_OK(dev_alloc(e, &f.tape, (size_t)(2 * n + 4) * up));
  if (dev_alloc(e, &f.tape_part, (size_t)n * e->P * e->g.H * 2)) {      // all or nothing
    gd_tape_free(e);
    return 1;
  }
  f.tape_n = n;
  return 0;
}
static inline real* tape_y(Engine* e, int i) { return e->fista.tape + (size_t)i * e->g.uplane * e->P; }
static inline real* tape_xk(Engine* e, int i) { return e->fista.tape + (size_t)(e->fista.tape_n + 1 + i) * e->g.uplane * e->P; }
static inline real* tape_work(Engine* e, int k) { return e->fista.tape + (size_t)(2 * e->fista.tape_n + 1 + k) * e->g.uplane * e->P; }

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
  e->fista.tape_iters = -1;
  if (e->fista.rec_on && e->fista.sched_n > 0) {     // y_0 (= xk_{-1})
    LPC_OK(gd_tape_alloc(e));
    LPC_RT(rt::copy_d2d_async(tape_y(e, 0), e->gd.gx, ub, e->stream));
    e->fista.tape_iters = 0;
  }
  return 0;
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
    if (e->fista.tape_iters >= 0 && e->fista.tape_iters == e->iters_done && e->iters_done < e->fista.tape_n) {
      // the tape: what the update just wrote, stream-ordered copies (the kernels are the unrecorded forward's)
      const size_t ub = (size_t)g.uplane * e->P * sizeof(real);
      LPC_RT(rt::copy_d2d_async(tape_xk(e, (int)e->iters_done), e->gd.gaux, ub, e->stream));
      LPC_RT(rt::copy_d2d_async(tape_y(e, (int)e->iters_done + 1), e->gd.gx, ub, e->stream));
      ++e->fista.tape_iters;
    }
    ++e->iters_done;
  }
  return 0;
}

// reverse sweep over the tape (lpc_fista_backward; lpc_gd_bwd_kernels.h): per iteration the forward's five launches.
// grad_psf (lpc_fista_backward_psf) adds, per iteration i, with r_i = Cv(y_i) - b recomputed from the tape:
//   g_psf += -a_i s sum over the batch of  K(conj(F(P gz_i)) . F(P r_i)) + K(conj(F(P y_i)) . F(P Hg_i))
// (the gradient through D, and through Cv: a convolution is symmetric in its two arguments, so the derivative w.r.t. the
// PSF is the adjoint convolution whose "PSF" is the other argument).  Launches: forward rows of y_i, its copy's column
// passes (-> F(P y_i)), the forward's middle + residual rows (-> rows of P r_i), the column passes of a copy of the head's
// rows (-> F(P gz_i)), the middle with F(P gz_i) as the multiplier + accumulate rows, and after MODE 1 the middle on a
// copy of the rows of P Hg_i with F(P y_i) as the multiplier + accumulate rows.  Without grad_psf nothing changes.
int gd_backward(Engine* e, const real* grad_out, real* grad_data, real* grad_alpha, real* grad_coef,
                       real* grad_init, real* grad_psf) {
  const PlaneGeom& g = e->g;
  const int n = e->fista.tape_n, C = e->cfg.channels;
  const int rows = e->mod && e->mod->gd_bwd_head ? g.H : (e->plan.rows_half ? g.H : (g.H + 1) / 2);   // workgroups per plane
  const long pstride = (long)e->P * rows * 2;
  GdBwd a;
  a.alpha = nullptr;
  a.gz = tape_work(e, 0); a.carry = tape_work(e, 1); a.gb = grad_data ? tape_work(e, 2) : nullptr;
  a.yn = tape_y(e, n);
  a.gb_first = 0; a.tail = 0;
  auto head_of = [&](int j) {
    a.xk = tape_xk(e, j); a.xkp = j > 0 ? tape_xk(e, j - 1) : tape_y(e, 0); a.y = tape_y(e, j);
    a.coef = e->fista.coef[(size_t)j];
    a.part = e->fista.tape_part + (long)j * pstride;
  };
  // PSF gradient: spectrum buffers W0 (rows of y_i -> Cv(y_i); then F(P gz_i); then the rows of P Hg_i -> second cross
  // term), W1 (rows of P r_i -> first cross term), W2 (F(P y_i))
  const size_t sbytes = (size_t)g.cplane * e->P * sizeof(real2);
  real2 *W0 = nullptr, *W1 = nullptr, *W2 = nullptr;
  GdBwd pa{};          // the accumulate's arguments (MODE 3)
  if (grad_psf) {
    LPC_OK(gd_psf_ws_alloc(e));
    W0 = e->fista.psf_spec; W1 = W0 + (size_t)g.cplane * e->P; W2 = W1 + (size_t)g.cplane * e->P;
    double s = 1.0;      // set_psf: the norm factor of the PSF spectrum
    if (e->cfg.norm == LPC_NORM_ORTHO) s = 1.0 / std::sqrt((double)g.Hp * (double)g.Wp);
    if (e->cfg.norm == LPC_NORM_FORWARD) s = 1.0 / ((double)g.Hp * (double)g.Wp);
    pa.gb = e->fista.psf_acc;
    pa.coef = (real)-s;
    pa.gb_first = 1;
  }
  auto psf_term = [&](real2* Srows, const real2* mult) {      // K(conj(mult) . column transform of Srows) -> acc
    LPC_OK(conv_middle(e, Srows, e->P, true, g.sh, g.sh + g.H, true, mult, e->P));
    LPC_OK(gd_bwd_rows(e, 3, pa, Srows));
    pa.gb_first = 0;
    return 0;
  };
  LPC_OK(hwc_to_planar(e, grad_out, a.gz, e->cfg.batch, g.H, g.W, g.W, g.uplane));
  head_of(n - 1);
  LPC_OK(gd_bwd_rows(e, 0, a));
  for (int i = n - 1; i >= 0; --i) {
    a.alpha = e->fista.galpha_sched + (long)i * C;
    if (grad_psf) {
      pa.alpha = a.alpha;
      LPC_OK(rows_fwd_single(e, src_unpadded(e, tape_y(e, i)), W0, e->P, LPC_K_ROW_FWD));
      LPC_OK(rows_fwd_single(e, src_unpadded(e, tape_y(e, i)), W2, e->P, LPC_K_ROW_FWD));   // (cheaper than a copy of W0)
      LPC_OK(cols_fwd_full(e, W2, e->P, g.sh, g.sh + g.H));                     // F(P y_i)
      LPC_OK(conv_middle(e, W0, e->P, false, g.sh, g.sh + g.H, true));         // Cv(y_i)
      LPC_OK(gd_rows_mid(e, W0, W1));                                           // rows of P r_i
      LPC_RT(rt::copy_d2d_async(W0, e->S, sbytes, e->stream));
      LPC_OK(cols_fwd_full(e, W0, e->P, g.sh, g.sh + g.H));                     // F(P gz_i)
      LPC_OK(psf_term(W1, W0));
    }
    LPC_OK(conv_middle(e, e->S, e->P, false, g.sh, g.sh + g.H, true));       // Cv(gz)
    a.gb_first = i == n - 1 ? 1 : 0;
    LPC_OK(gd_bwd_rows(e, 1, a));
    if (grad_psf) {
      LPC_RT(rt::copy_d2d_async(W0, e->gd.S2, sbytes, e->stream));             // rows of P Hg_i
      LPC_OK(psf_term(W0, W2));
    }
    LPC_OK(conv_middle(e, e->gd.S2, e->P, true, g.sh, g.sh + g.H, true));       // D(Hg)
    if (i > 0) head_of(i - 1);
    a.tail = i == 0 ? 1 : 0;
    LPC_OK(gd_bwd_rows(e, 2, a));
  }
  e->gd.fwd_done = false;     // S no longer holds the row spectra of the iterate
  LPC_OK(launch_k(e, -1, k_gd_bwd_finish<256>, dim3(C + 1, n), 256, gd_bwd_red_bytes<256>(), (const double*)e->fista.tape_part,
                  e->P, rows, C, (const real*)e->fista.galpha_sched, grad_alpha, grad_coef));
  if (grad_psf) LPC_OK(gd_bwd_psf_sum(e, e->fista.psf_acc, grad_psf));
  if (grad_init) LPC_OK(planar_to_hwc(e, a.gz, grad_init, e->cfg.batch, g.H, g.W, g.W, g.uplane, 0, 0, 0));
  if (grad_data)
    LPC_OK(launch_k(e, -1, k_gd_bwd_gdata<256>, grid1d(g.uplane, 256, e->cfg.batch), 256, 0, (const real*)a.gb, grad_data,
                    (long)g.uplane, C, e->data_channels));
  return 0;
}

int gd_finish_split(Engine* e, const real* dev_projected) {
  const PlaneGeom& g = e->g;
  const double tk_new = (1.0 + std::sqrt(1.0 + 4.0 * e->gd.tk * e->gd.tk)) / 2.0;  // gd.py:238
  LPC_OK(launch_k(e, -1, k_gd_post<256>, grid1d(g.uplane, 256, e->P), 256, 0, g, dev_projected, e->gd.gx, e->gd.gaux,
                  e->cfg.algo - LPC_ALGO_GD, (real)((e->gd.tk - 1.0) / tk_new)));
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
  return (e->cfg.algo == LPC_ALGO_GD ? 6.0 : 8.0) * eb * g.H * g.W * e->P + 14.0 * S;
}
