// lpc_gd_bwd.cpp -- reverse mode of unrolled FISTA (lpc_fista_record / lpc_fista_backward): the launches of its row kernels,
// the layout of its tape with what a reset and an iteration copy into it, and the reverse sweep
#include "lpc_gd_bwd_launch.h"

// mode 0 / 1 / 2: head, middle rows, update + next head;  3: rows of Sin -> the PSF gradient's accumulator
// (lpc_gd_bwd_kernels.h)
int gd_bwd_rows(Engine* e, int mode, const GdBwd& a, const real2* Sin) {
  const PlaneGeom& g = e->g;
  if (e->mod && e->mod->gd_bwd_head) {
    if (mode == 3) return e->mod->gd_bwd_acc(e, &a, Sin);
    if (mode == 0) return e->mod->gd_bwd_head(e, &a);
    return mode == 1 ? e->mod->gd_bwd_mid(e, &a) : e->mod->gd_bwd_update(e, &a);
  }
  if (e->plan.rows_half)
    return dispatch_row(g.Wp / 2, e->planWh.skew_ok, false, [&](auto NT, auto EM, auto SK, auto) {
      if (mode == 0) return launch_gd_bwd_half<0, NT.value, EM.value, SK.value>(e, e->planWh, a);
      if (mode == 1) return launch_gd_bwd_half<1, NT.value, EM.value, SK.value>(e, e->planWh, a);
      if (mode == 3) return launch_gd_bwd_half<3, NT.value, EM.value, SK.value>(e, e->planWh, a, Sin);
      return launch_gd_bwd_half<2, NT.value, EM.value, SK.value>(e, e->planWh, a);
    });
  const int nblk = (g.H + 1) / 2;
  return dispatch_row(g.Wp, e->planW.skew_ok, false, [&](auto NTc, auto EM, auto SK, auto) {
    constexpr int nt = decltype(NTc)::value, em = decltype(EM)::value;
    constexpr bool sk = decltype(SK)::value;
    const size_t smem = gd_bwd_red_bytes<nt>() + LPC_ROW_SMEM_BYTES(g.Wp, sk);
    if (mode == 0)
      return launch_k(e, -1, k_gd_bwd_paired<0, nt, em, sk>, dim3(nblk, e->P), nt, smem, g, e->planW,
                      (const real2*)e->gd.S2, e->S, a);
    if (mode == 1)
      return launch_k(e, -1, k_gd_bwd_paired<1, nt, em, sk>, dim3(nblk, e->P), nt, smem, g, e->planW,
                      (const real2*)e->S, e->gd.S2, a);
    if (mode == 3)
      return launch_k(e, -1, k_gd_bwd_paired<3, nt, em, sk>, dim3(nblk, e->P), nt, smem, g, e->planW, Sin,
                      (real2*)nullptr, a);
    return launch_k(e, -1, k_gd_bwd_paired<2, nt, em, sk>, dim3(nblk, e->P), nt, smem, g, e->planW,
                    (const real2*)e->gd.S2, e->S, a);
  });
}

// the PSF gradient's finishing sum over the batch (k_gd_bwd_gpsf): acc [B*C][H][W] -> (1, H, W, C)
int gd_bwd_psf_sum(Engine* e, const real* acc, real* grad_psf) {
  const PlaneGeom& g = e->g;
  return launch_k(e, -1, k_gd_bwd_gpsf<256>, grid1d(g.uplane, 256, e->cfg.channels), 256, 0, acc, grad_psf, (long)g.uplane,
                  e->cfg.channels, e->cfg.batch);
}

// planar data gradient (k_gd_bwd_gdata): gb [B*C][H][W] -> (B, H, W, data_channels); the ADMM sweep ends with it too
int gd_bwd_gdata(Engine* e, const real* gb, real* grad_data) {
  const PlaneGeom& g = e->g;
  return launch_k(e, -1, k_gd_bwd_gdata<256>, grid1d(g.uplane, 256, e->cfg.batch), 256, 0, gb, grad_data, (long)g.uplane,
                  e->cfg.channels, e->data_channels);
}

// ---- the tape (struct Tape, lpc_engine.h): 2 n + 4 un-padded state arrays ----
int gd_tape_alloc(Engine* e) {
  const int n = e->fista.sched_n;
  if (n <= 0) return 0;
  return tape_alloc(e, e->fista_tape, n, 2 * (size_t)n + 4, (size_t)e->g.uplane * e->P, (size_t)n * e->P * e->g.H * 2);
}
static inline real* tape_y(Engine* e, int i) { return e->fista_tape.at(i); }
static inline real* tape_xk(Engine* e, int i) { return e->fista_tape.at(e->fista_tape.n + 1 + i); }
static inline real* tape_work(Engine* e, int k) { return e->fista_tape.at(2 * e->fista_tape.n + 1 + k); }

int gd_tape_reset(Engine* e) {
  Tape& t = e->fista_tape;
  t.invalidate();
  if (!t.rec_on || e->fista.sched_n <= 0) return 0;
  LPC_OK(gd_tape_alloc(e));
  LPC_RT(rt::copy_d2d_async(tape_y(e, 0), e->gd.gx, t.slot * sizeof(real), e->stream));     // y_0 (= xk_{-1})
  t.begin();
  return 0;
}

int gd_tape_push(Engine* e) {
  Tape& t = e->fista_tape;
  if (!t.wants(e->iters_done)) return 0;
  LPC_RT(rt::copy_d2d_async(tape_xk(e, (int)e->iters_done), e->gd.gaux, t.slot * sizeof(real), e->stream));
  LPC_RT(rt::copy_d2d_async(tape_y(e, (int)e->iters_done + 1), e->gd.gx, t.slot * sizeof(real), e->stream));
  t.advance();
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
// One PSF per frame (lpc_per_frame_grad): the same launches -- every middle reads PSF plane q % PlaneGeom::PM = q -- and
// the accumulator, one plane per state plane already, is laid out as (B,1,H,W,C) instead of summed over the batch.
int gd_backward(Engine* e, const real* grad_out, real* grad_data, real* grad_alpha, real* grad_coef,
                real* grad_init, real* grad_psf) {
  const PlaneGeom& g = e->g;
  Tape& t = e->fista_tape;
  const int n = t.n, C = e->cfg.channels;
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
    a.part = t.part + (long)j * pstride;
  };
  // PSF gradient: spectrum buffers W0 (rows of y_i -> Cv(y_i); then F(P gz_i); then the rows of P Hg_i -> second cross
  // term), W1 (rows of P r_i -> first cross term), W2 (F(P y_i))
  const size_t sp = (size_t)g.cplane * e->P, sbytes = sp * sizeof(real2);
  real2 *W0 = nullptr, *W1 = nullptr, *W2 = nullptr;
  GdBwd pa{};          // the accumulate's arguments (MODE 3)
  if (grad_psf) {      // (Tape::psf_ws: three spectra, then the accumulator)
    LPC_OK(tape_psf_ws(e, t, 6 * sp + (size_t)g.uplane * e->P));
    W0 = (real2*)t.psf_ws; W1 = W0 + sp; W2 = W1 + sp;
    double s = 1.0;      // set_psf: the norm factor of the PSF spectrum
    if (e->cfg.norm == LPC_NORM_ORTHO) s = 1.0 / std::sqrt((double)g.Hp * (double)g.Wp);
    if (e->cfg.norm == LPC_NORM_FORWARD) s = 1.0 / ((double)g.Hp * (double)g.Wp);
    pa.gb = t.psf_ws + 6 * sp;
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
  LPC_OK(launch_k(e, -1, k_gd_bwd_finish<256>, dim3(C + 1, n), 256, gd_bwd_red_bytes<256>(), (const double*)t.part,
                  e->P, rows, C, (const real*)e->fista.galpha_sched, grad_alpha, grad_coef));
  // one PSF per frame (lpc_set_psf_batch): the accumulator's plane q is PSF q's own gradient -- no sum, only the layout,
  // (B,1,H,W,C).  The sweep above needs nothing else: conv_middle finds a frame's spectrum through PlaneGeom::PM, the
  // explicit multipliers are P planes already and the norm factor s is one number for every PSF
  if (grad_psf && e->psf_per_frame) LPC_OK(planar_to_hwc(e, pa.gb, grad_psf, e->cfg.batch, g.H, g.W, g.W, g.uplane, 0, 0, 0));
  else if (grad_psf) LPC_OK(gd_bwd_psf_sum(e, pa.gb, grad_psf));
  if (grad_init) LPC_OK(planar_to_hwc(e, a.gz, grad_init, e->cfg.batch, g.H, g.W, g.W, g.uplane, 0, 0, 0));
  if (grad_data) LPC_OK(gd_bwd_gdata(e, a.gb, grad_data));
  return 0;
}
