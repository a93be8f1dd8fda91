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
    ++e->iters_done;
  }
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
