// lpc_gd_engine.inc -- host sequences of the gradient-descent family (included by lpc_engine.cpp)

static int gd_alloc(Engine* e) {
  const PlaneGeom& g = e->g;
  const size_t up = (size_t)g.uplane * e->P;
  LPC_OK(dev_alloc(e, &e->gx, up));
  LPC_OK(dev_alloc(e, &e->gaux, up));
  LPC_OK(dev_alloc(e, &e->galpha, 4));
  LPC_OK(dev_alloc(e, &e->gx0, 4));
  LPC_OK(dev_alloc(e, &e->S2, (size_t)g.cplane * e->P));
  return 0;
}

// alpha = lip_fact / max|H* H| per channel (gd.py:107-112); x0 = (max psf + min psf)/2 (gd.py:100-105)
static int gd_setup_constants(Engine* e) {
  const PlaneGeom& g = e->g;
  const int nblk = 64;
  real* partial = (real*)e->S2;  // scratch: 2 * Ppsf * nblk floats
  LPC_OK(launch_k(e, -1, k_plane_minmax<256>, dim3(nblk, e->Ppsf), 256, 2 * 256 * sizeof(real), g,
                  (const real2*)e->Hs, (const real*)nullptr, 0, partial));
  LPC_OK(launch_k(e, -1, k_channel_finish, dim3(1), 64, 0, (const real*)partial, nblk, e->cfg.depth,
                  e->cfg.channels, 0, (real)e->cfg.lip_fact, e->galpha));
  LPC_OK(launch_k(e, -1, k_plane_minmax<256>, dim3(nblk, e->Ppsf), 256, 2 * 256 * sizeof(real), g,
                  (const real2*)nullptr, (const real*)e->psf_planar, 1, partial));
  LPC_OK(launch_k(e, -1, k_channel_finish, dim3(1), 64, 0, (const real*)partial, nblk, e->cfg.depth,
                  e->cfg.channels, 1, (real)0., e->gx0));
  return 0;
}

static int gd_apply_momentum_reset(Engine* e) {
  if (e->cfg.algo == LPC_ALGO_NESTEROV && e->gaux) {
    const long n = (long)e->g.uplane * e->P;
    LPC_OK(launch_k(e, -1, k_fill<256>, grid1d(n, 256), 256, 0, e->gaux, n, (real)e->nest_p));
  }
  return 0;
}

// ---- the tape of the reverse mode (Engine::tape) ----
static void gd_tape_free(Engine* e) {
  if (!e->tape) return;
  (void)rt::stream_sync(e->stream);
  const size_t up = (size_t)e->g.uplane * e->P;
  for (void* p : {(void*)e->tape, (void*)e->tape_part}) {
    e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), p), e->allocs.end());
    (void)rt::dev_free(p);
  }
  e->total_bytes -= (size_t)(2 * e->tape_n + 4) * up * sizeof(real) + (size_t)e->tape_n * e->P * e->g.H * 2 * sizeof(double);
  e->tape = nullptr; e->tape_part = nullptr; e->tape_n = 0; e->tape_iters = -1;
}
static int gd_tape_alloc(Engine* e) {
  const int n = e->fista_sched_n;
  if (e->tape && e->tape_n == n) return 0;
  gd_tape_free(e);
  const size_t up = (size_t)e->g.uplane * e->P;
  real* tape = nullptr;
  double* part = nullptr;
  LPC_OK(dev_alloc(e, &tape, (size_t)(2 * n + 4) * up));
  if (dev_alloc(e, &part, (size_t)n * e->P * e->g.H * 2)) {      // all or nothing
    e->allocs.pop_back();
    e->total_bytes -= (size_t)(2 * n + 4) * up * sizeof(real);
    (void)rt::dev_free(tape);
    return 1;
  }
  e->tape = tape; e->tape_part = part; e->tape_n = n;
  return 0;
}
static inline real* tape_y(Engine* e, int i) { return e->tape + (size_t)i * e->g.uplane * e->P; }
static inline real* tape_xk(Engine* e, int i) { return e->tape + (size_t)(e->tape_n + 1 + i) * e->g.uplane * e->P; }
static inline real* tape_work(Engine* e, int k) { return e->tape + (size_t)(2 * e->tape_n + 1 + k) * e->g.uplane * e->P; }

static int gd_reset(Engine* e) {
  const PlaneGeom& g = e->g;
  const size_t ub = (size_t)g.uplane * e->P * sizeof(real);
  if (e->has_init) {
    LPC_RT(rt::copy_d2d_async(e->gx, e->init_est, ub, e->stream));
  } else {
    LPC_OK(launch_k(e, -1, k_fill_per_channel<256>, grid1d(g.uplane, 256, e->P), 256, 0, e->gx, g.uplane,
                    e->cfg.channels, (const real*)e->gx0));
  }
  if (e->fista_sched_n > 0)  // unrolled FISTA: x_k starts as the initial image (unrolled_fista.py:91-96)
    LPC_RT(rt::copy_d2d_async(e->gaux, e->gx, ub, e->stream));
  else
    LPC_RT(rt::memset_async(e->gaux, 0, ub, e->stream));
  // gd.py:178-181: NesterovGradientDescent.reset(p=0, mu=0.9) -- the defaults win over the
  // constructor arguments because the base constructor calls reset() bare (recon.py:328-329)
  e->nest_p = 0.0;
  e->nest_mu = 0.9;
  e->tk = e->cfg.fista_tk;  // gd.py:227-232
  e->first = true;
  e->split_pending = false;
  e->gd_fwd_done = false;
  e->iters_done = 0;
  e->tape_iters = -1;
  if (e->rec_on && e->fista_sched_n > 0) {     // y_0 (= xk_{-1})
    LPC_OK(gd_tape_alloc(e));
    LPC_RT(rt::copy_d2d_async(tape_y(e, 0), e->gx, ub, e->stream));
    e->tape_iters = 0;
  }
  return 0;
}

// split == 1: one iteration up to (not including) the projection; gd_finish_split completes it
static int gd_iterate(Engine* e, int n_iter, int split = 0) {
  const PlaneGeom& g = e->g;
  for (int it = 0; it < n_iter; ++it) {
    // H x  (the row spectra are already there when the previous iteration's update kernel produced them)
    if (!e->gd_fwd_done) LPC_OK(rows_fwd_single(e, src_unpadded(e, e->gx), e->S, e->P, LPC_K_ROW_FWD));
    e->gd_fwd_done = false;
    LPC_OK(conv_middle(e, e->S, e->P, false, g.sh, g.sh + g.H, true));
    // (H x - y), straight back into the frequency domain
    LPC_OK(gd_rows_mid(e));
    // H^T (.)
    LPC_OK(conv_middle(e, e->S2, e->P, true, g.sh, g.sh + g.H, true));
    GdScalars sc;
    sc.kind = e->cfg.algo - LPC_ALGO_GD;
    sc.mu = (real)e->nest_mu;
    sc.negmu = (real)(-e->nest_mu);
    sc.onepmu = (real)(1.0 + e->nest_mu);
    const double tk_new = (1.0 + std::sqrt(1.0 + 4.0 * e->tk * e->tk)) / 2.0;  // gd.py:238
    sc.coef = (real)((e->tk - 1.0) / tk_new);
    sc.first = e->first ? 1 : 0;
    sc.split = split;
    const real* alpha = e->galpha;
    if (e->fista_sched_n > 0) {
      const long i = std::min<long>(e->iters_done, e->fista_sched_n - 1);
      sc.coef = e->fista_coef[(size_t)i];
      sc.first = 0;
      alpha = e->galpha_sched + i * e->cfg.channels;
    }
    if (e->plan.gd_fuse_fwd && !split) {
      LPC_OK(e->mod->gd_rows_update_fwd(e, &sc, alpha));   // (LaunchPlan::gd_fuse_fwd: the module holds it)
      e->gd_fwd_done = true;
    } else {
      LPC_OK(gd_rows_update(e, sc, alpha));
    }
    if (split) { e->split_pending = true; return 0; }
    if (e->cfg.algo == LPC_ALGO_FISTA) e->tk = tk_new;
    e->first = false;
    if (e->tape_iters >= 0 && e->tape_iters == e->iters_done && e->iters_done < e->tape_n) {
      // the tape: what the update just wrote, stream-ordered copies (the kernels are the unrecorded forward's)
      const size_t ub = (size_t)g.uplane * e->P * sizeof(real);
      LPC_RT(rt::copy_d2d_async(tape_xk(e, (int)e->iters_done), e->gaux, ub, e->stream));
      LPC_RT(rt::copy_d2d_async(tape_y(e, (int)e->iters_done + 1), e->gx, ub, e->stream));
      ++e->tape_iters;
    }
    ++e->iters_done;
  }
  return 0;
}

// reverse sweep over the tape (lpc_fista_backward; lpc_gd_bwd_kernels.h): per iteration the forward's five launches
static int gd_backward(Engine* e, const real* grad_out, real* grad_data, real* grad_alpha, real* grad_coef,
                       real* grad_init) {
  const PlaneGeom& g = e->g;
  const int n = e->tape_n, C = e->cfg.channels;
  const int rows = e->mod && e->mod->gd_bwd_head ? g.H : (e->plan.rows_half ? g.H : (g.H + 1) / 2);   // workgroups per plane
  const long pstride = (long)e->P * rows * 2;
  GdBwd a;
  a.alpha = nullptr;
  a.gz = tape_work(e, 0); a.carry = tape_work(e, 1); a.gb = grad_data ? tape_work(e, 2) : nullptr;
  a.yn = tape_y(e, n);
  a.gb_first = 0; a.tail = 0;
  auto head_of = [&](int j) {
    a.xk = tape_xk(e, j); a.xkp = j > 0 ? tape_xk(e, j - 1) : tape_y(e, 0); a.y = tape_y(e, j);
    a.coef = e->fista_coef[(size_t)j];
    a.part = e->tape_part + (long)j * pstride;
  };
  LPC_OK(hwc_to_planar(e, grad_out, a.gz, e->cfg.batch, g.H, g.W, g.W, g.uplane));
  head_of(n - 1);
  LPC_OK(gd_bwd_rows(e, 0, a));
  for (int i = n - 1; i >= 0; --i) {
    a.alpha = e->galpha_sched + (long)i * C;
    LPC_OK(conv_middle(e, e->S, e->P, false, g.sh, g.sh + g.H, true));       // Cv(gz)
    a.gb_first = i == n - 1 ? 1 : 0;
    LPC_OK(gd_bwd_rows(e, 1, a));
    LPC_OK(conv_middle(e, e->S2, e->P, true, g.sh, g.sh + g.H, true));       // D(Hg)
    if (i > 0) head_of(i - 1);
    a.tail = i == 0 ? 1 : 0;
    LPC_OK(gd_bwd_rows(e, 2, a));
  }
  e->gd_fwd_done = false;     // S no longer holds the row spectra of the iterate
  LPC_OK(launch_k(e, -1, k_gd_bwd_finish<256>, dim3(C + 1, n), 256, gd_bwd_red_bytes<256>(), (const double*)e->tape_part,
                  e->P, rows, C, (const real*)e->galpha_sched, grad_alpha, grad_coef));
  if (grad_init) LPC_OK(planar_to_hwc(e, a.gz, grad_init, e->cfg.batch, g.H, g.W, g.W, g.uplane, 0, 0, 0));
  if (grad_data)
    LPC_OK(launch_k(e, -1, k_gd_bwd_gdata<256>, grid1d(g.uplane, 256, e->cfg.batch), 256, 0, (const real*)a.gb, grad_data,
                    (long)g.uplane, C, e->data_channels));
  return 0;
}

static int gd_finish_split(Engine* e, const real* dev_projected) {
  const PlaneGeom& g = e->g;
  const double tk_new = (1.0 + std::sqrt(1.0 + 4.0 * e->tk * e->tk)) / 2.0;  // gd.py:238
  LPC_OK(launch_k(e, -1, k_gd_post<256>, grid1d(g.uplane, 256, e->P), 256, 0, g, dev_projected, e->gx, e->gaux,
                  e->cfg.algo - LPC_ALGO_GD, (real)((e->tk - 1.0) / tk_new)));
  if (e->cfg.algo == LPC_ALGO_FISTA) e->tk = tk_new;
  e->first = false;
  e->split_pending = false;
  e->gd_fwd_done = false;
  ++e->iters_done;
  return 0;
}

static int gd_get_state(Engine* e, const std::string& nm, real* dev_out) {
  const PlaneGeom& g = e->g;
  const int nimg = e->cfg.batch * e->cfg.depth;
  if (nm == "image_est") return planar_to_hwc(e, e->gx, dev_out, nimg, g.H, g.W, g.W, g.uplane, 0, 0, 0);
  if (nm == "alpha") {
    LPC_RT(rt::copy_d2d_async(dev_out, e->galpha, e->cfg.channels * sizeof(real), e->stream));
    return 0;
  }
  return fail("lpc_get_state: unknown name '" + nm + "'");
}

static int gd_kernel_bytes(Engine* e, int kid, double* bytes) {
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
