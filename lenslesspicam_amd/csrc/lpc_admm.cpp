// lpc_admm.cpp -- host side of ADMM: workspace and spectral constants, the fused iteration, the plug-and-play and
// custom-psi iterations around a caller's step, read-out of the state, and the byte models.  Every image-domain ADMM
// kernel is launched from here; the row and column passes from lpc_rows.cpp / lpc_cols.cpp.
#include "lpc_engine.h"
#include "lpc_admm_kernels.h"
#include "lpc_layout_kernels.h"
#include "lpc_reduce_kernels.h"

// ------------------------------------------------------------------------------ ADMM --
// parameters of iteration `it` (since reset): the schedule if one is set, else the constructor's
static void admm_params(const Engine* e, long it, double out[4]) {
  const lpc_config& c = e->cfg;
  const double dflt[4] = {c.mu1, c.mu2, c.mu3, c.tau};
  for (int k = 0; k < 4; ++k) {
    const std::vector<double>& v = e->admm.sched[k];
    out[k] = v.empty() ? dflt[k] : v[(size_t)std::min<long>(it, (long)v.size() - 1)];
  }
}

// prev_par: the step sizes of the iteration before, for an iteration that is not the next to run (admm_iterate: the X half
// that rides in the previous iteration's H V rows); else the engine's record
static AdmmScalars admm_scalars(const Engine* e, const double cur[4], const double* prev_par = nullptr) {
  AdmmScalars p;
  p.mu1 = (real)cur[0]; p.mu2 = (real)cur[1]; p.mu3 = (real)cur[2];
  p.thr = (real)(cur[3] / cur[1]);               // admm.py:246: python-double division, then float32
  p.m_in = (real)1.0 / ((real)1.0 + p.mu1);                 // admm.py:193 in float32
  p.m_out = (real)1.0 / ((real)0.0 + p.mu1);
  p.first = (e->first && !prev_par) ? 1 : 0;
  const double* prev = prev_par ? prev_par : e->first ? cur : e->admm.last_par;
  p.mu1p = (real)prev[0]; p.mu2p = (real)prev[1]; p.mu3p = (real)prev[2];
  p.thrp = (real)(prev[3] / prev[1]);
  p.m_in_p = (real)1.0 / ((real)1.0 + p.mu1p);
  p.m_out_p = (real)1.0 / ((real)0.0 + p.mu1p);
  p.r_mu2 = (real)(1.0 / (double)p.mu2); p.r_mu3 = (real)(1.0 / (double)p.mu3);      // RN(1/d): see div_by
  p.r_mu2p = (real)(1.0 / (double)p.mu2p); p.r_mu3p = (real)(1.0 / (double)p.mu3p);
  p.clamp_cur = e->admm.vw_cur ? 1 : 0;
  p.clamp_old = e->admm.vw_old ? 1 : 0;
  p.xiw = e->plan.xi_window ? 1 : 0;
  p.xi_store = 1;              // admm_iterate clears it on all but the last iteration of a call
  p.skipa = p.skiphv = 0;      // set by admm_iterate inside a call (AdmmScalars::skipa)
  p.rev = e->plan.rev_k1 ? 1 : 0;
  p.half_in = p.half_out = 0;  // set by admm_iterate between the iterations of one call (AdmmScalars::half_in)
  p.rho_rsp = p.xi_in = p.xi_out = 0;      // likewise (AdmmScalars::rho_rsp, xi_in)
  return p;
}

// what ADMM keeps per PSF plane besides Hs: the pair-line copy of H and the sequential middle's precombined constants.
// Gives back what the handle holds of them first (lpc_set_psf_batch grows them from D*C to batch*D*C planes)
int admm_alloc_psf(Engine* e, int nplanes) {
  const PlaneGeom& g = e->g;
  dev_free(e, e->admm.Hs_t); dev_free(e, e->admm.midc); dev_free(e, e->admm.midrd);
  e->admm.Hs_t = nullptr; e->admm.midc = nullptr; e->admm.midrd = nullptr;
  e->admm.midc_valid = false;
  if (!g.slay) return 0;
  LPC_OK(dev_alloc(e, &e->admm.Hs_t, (size_t)g.cplane * nplanes));
  if (e->mod && e->mod->mid_pc) {
    real2* c = nullptr;
    LPC_OK(dev_alloc(e, &c, (size_t)g.cplane * nplanes * (e->mod->mid_pc == 1 ? 2 : 1)));
    e->admm.midc = c;
    LPC_OK(dev_alloc(e, &e->admm.midrd, (size_t)g.cplane * nplanes));
  }
  return 0;
}

static const int kGsepBlocks = 512;
int admm_alloc(Engine* e) {
  const PlaneGeom& g = e->g;
  const size_t rp = (size_t)g.rplane * e->P;
  // the eight arrays reset() zeroes are ONE block, V[0] first: one fill instead of eight (a reset of a DiffuserCam-sized
  // frame was 8 x 5.3 us of launch-bound fills in a 264-us apply(), profiles/r04k_c1_gaps.txt)
  real* zeroed = nullptr;
  LPC_OK(dev_alloc(e, &zeroed, 8 * rp));
  real** zb[] = {&e->admm.V[0], &e->admm.V[1], &e->admm.HVb[0], &e->admm.HVb[1], &e->admm.xi, &e->admm.eta0[0], &e->admm.eta1[0], &e->admm.rho};
  for (int k = 0; k < 8; ++k) *zb[k] = zeroed + (size_t)k * rp;
  real** bufs[] = {&e->admm.eta0[1], &e->admm.eta1[1], &e->admm.Rsp, &e->admm.Aarr};
  for (real** b : bufs) LPC_OK(dev_alloc(e, b, rp));
  LPC_OK(dev_alloc(e, &e->admm.Gabs, (size_t)g.cplane));
  if (g.slay) LPC_OK(dev_alloc(e, &e->admm.Gabs_t, (size_t)g.cplane));
  LPC_OK(admm_alloc_psf(e, e->Ppsf));
  LPC_OK(dev_alloc(e, &e->admm.Ga, (size_t)g.Hp));
  LPC_OK(dev_alloc(e, &e->admm.Gb, (size_t)g.cpitch));
  LPC_OK(dev_alloc(e, &e->admm.Gpart, (size_t)2 * kGsepBlocks));
  return 0;
}

// |PsiT Psi| as row term + column term (ColPass::ga): taken when the plane in e->admm.Gabs separates to float32 round-off
// (the reference's finite-difference gram does, admm.py:385-397; a caller's psi_gram in general does not)
static int admm_split_gram(Engine* e) {
  const PlaneGeom& g = e->g;
  e->admm.g_sep = 0;
  e->admm.midc_valid = false;      // (a new PSF or gram: the middle's precombined constants are remade at the next step)
  if (g.slay)       // the 8-column middle reads the plane in pair lines
    LPC_OK(launch_k(e, -1, k_to_pair_lines<256, real>, grid1d((long)g.Hp * g.cpitch, 256), 256, 0, (const real*)e->admm.Gabs,
                    e->admm.Gabs_t, g.Hp, g.cpitch, g.cplane));
  if (!e->plan.g_terms) return 0;
  const int n = (int)std::max<long>(g.Hp, g.cpitch);
  LPC_OK(launch_k(e, -1, k_gsep_extract, grid1d((long)n, 256), 256, 0, (const real*)e->admm.Gabs, g.Hp, g.Wc,
                  (long)g.cpitch, e->admm.Ga, e->admm.Gb));
  LPC_OK(launch_k(e, -1, k_gsep_check<256>, dim3(kGsepBlocks), 256, 2 * 256 * sizeof(real), (const real*)e->admm.Gabs, g.Hp,
                  g.Wc, (long)g.cpitch, (const real*)e->admm.Ga, (const real*)e->admm.Gb, e->admm.Gpart));
  std::vector<real> part((size_t)2 * kGsepBlocks);
  LPC_RT(rt::copy_d2h_async(part.data(), e->admm.Gpart, part.size() * sizeof(real), e->stream));
  LPC_RT(rt::stream_sync(e->stream));
  double err = 0., top = 0.;
  for (int b = 0; b < kGsepBlocks; ++b) { err = std::max(err, (double)part[2 * b]); top = std::max(top, -(double)part[2 * b + 1]); }
  const double eps = sizeof(real) == 4 ? 1e-6 : 1e-13;        // a few ulp of the largest entry: FFT round-off of the gram
  e->admm.g_sep = (top > 0. && err <= eps * top) ? 1 : 0;
  return 0;
}

int admm_setup_constants(Engine* e) {
  // R_divmat = 1/(mu1 |H* H| + mu2 |PsiT Psi| + mu3)  (admm.py:186-190) is formed inside the middle
  // kernel; here only |PsiT Psi| is prepared.  The gram spectrum is produced by the engine's own forward
  // transform of the 5-point stencil (admm.py:385-397) so that it lands in the permuted row order.
  const PlaneGeom& g = e->g;
  real* stencil = e->admm.Rsp;  // scratch: one padded plane
  LPC_RT(rt::memset_async(stencil, 0, (size_t)g.rplane * sizeof(real), e->stream));
  std::vector<real> host((size_t)g.rplane, (real)0.);
  // gram[0,0]=4; [0,1]=[0,-1]=[1,0]=[-1,0]=-1 with python negative indexing (later writes win)
  host[0] = (real)4.;
  host[(size_t)(1 % g.Wp)] = -(real)1.;
  host[(size_t)(g.Wp - 1)] = -(real)1.;
  host[(size_t)(1 % g.Hp) * g.rpitch] = -(real)1.;
  host[(size_t)(g.Hp - 1) * g.rpitch] = -(real)1.;
  LPC_OK(upload(e, stencil, host.data(), host.size() * sizeof(real)));
  real2* Gs = e->S;  // scratch spectrum plane
  LPC_OK(fft2_forward_setup(e, src_padded(e, stencil), Gs, 1));
  LPC_OK(launch_k(e, -1, k_abs_complex<256>, grid1d((long)g.cplane, 256), 256, 0, (const real2*)Gs, e->admm.Gabs,
                  (long)g.cplane));
  e->admm.custom_gram = false;
  return admm_split_gram(e);
}

int admm_reset(Engine* e) {
  const PlaneGeom& g = e->g;
  const size_t rb = (size_t)g.rplane * e->P * sizeof(real);
  // V[1], HVb[0], HVb[1], xi, eta0[0], eta1[0], rho: contiguous behind V[0] (admm_alloc)
  if (e->has_init) LPC_RT(rt::memset_async(e->admm.V[1], 0, 7 * rb, e->stream));
  else LPC_RT(rt::memset_async(e->admm.V[0], 0, 8 * rb, e->stream));
  e->admm.vcur = 0;
  e->admm.ecur = 0;
  e->admm.hcur = 0;
  e->admm.vw_cur = e->admm.vw_old = false;
  if (e->has_init) {
    LPC_RT(rt::copy_d2d_async(e->admm.V[0], e->init_est, rb, e->stream));
    // admm.py:172-176: forward_out = convolve(V0)
    LPC_OK(convolve_planar(e, e->admm.V[0], e->admm.HVb[0], e->P, true, false));
  }
  e->first = true;
  e->admm.pnp_mode = e->admm.pnp_pending = false;
  e->iters_done = 0;
  return admm_tape_reset(e);
}

// (r_sp, a) in e->admm.Rsp / e->admm.Aarr  ->  Vout = irfft2(R_div (rfft2 r_sp + s H* rfft2 a)),  HVout = H Vout:
// forward rows, [pass A], fused middle, [inverse pass A], inverse rows
// a_done: the rows of `a` are in SB already, the forward rows run r_sp alone; next: the window's rows of H V stay on chip
// (LaunchPlan::hv_fuse) -- k_hv_rows_v2 turns them into the rows of `a` of the iteration whose scalars *next holds, the
// inverse rows write V alone and HVout is not touched
static int admm_spectral_step(Engine* e, const AdmmScalars& sc, real* Vout, real* HVout, bool xhalf = false,
                              const K1Rows* k1 = nullptr, bool a_done = false, const AdmmScalars* next = nullptr) {
  if (xhalf) LPC_OK(e->mod->admm_rows_fwd_x(e, &sc, k1, a_done ? 1 : 0));   // (LaunchPlan::xhalf_rows: the module holds it)
  else LPC_OK(admm_rows_fwd(e));
  LPC_OK(admm_cols(e, sc));
  if (!next) return admm_rows_inv(e, Vout, HVout, sc.skiphv ? ADMM_HV_ROWS_WINDOW : ADMM_HV_ROWS_ALL);
  // two launches, one entry of the per-iteration profile.  The fused rows first: inverse pass A ends on the planes of SB,
  // and the tiled kernel that follows walks backwards from the tail of V (hv_fuse = 2: the other order, for measurements)
  size_t slot = 0;
  LPC_OK(timer_span_begin(e, LPC_K_ROW_INV, &slot));
  if (e->plan.hv_fuse == 2) LPC_OK(admm_rows_inv(e, Vout, HVout, ADMM_HV_ROWS_NONE));
  LPC_OK(e->mod->admm_rows_hv(e, next));
  if (e->plan.hv_fuse != 2) LPC_OK(admm_rows_inv(e, Vout, HVout, ADMM_HV_ROWS_NONE));
  return timer_span_end(e, LPC_K_ROW_INV, slot);
}
// ... with the step sizes `par` and nothing skipped: the spectral step of the reverse sweep (lpc_admm_bwd.cpp)
int admm_spectral_plain(Engine* e, const double par[4], real* Vout, real* HVout) {
  return admm_spectral_step(e, admm_scalars(e, par), Vout, HVout);
}


// the image-domain kernel of a stand-alone K1 form (half_in: the duals arrive half-applied, AdmmScalars::half_in)
typedef void (*K1Kernel)(PlaneGeom, AdmmScalars, const real*, const real*, const real*, const real*, real*, const real*,
                         const real*, real*, real*, real*, const real*, real*, real*, unsigned);
struct K1Launch { K1Kernel fn; int th, tw; size_t smem; };   // kernel, tile rows x columns, LDS bytes
static K1Launch k1_launch(AdmmK1 form, bool half_in) {
  constexpr int NT = 256, TW4 = 256;
  auto smem4 = [](int th) { return (size_t)2 * (th + 2) * (TW4 + 8) * sizeof(real); };
  switch (form) {
    // the TV / W half alone (X half inside the forward rows) is lighter per pixel: 4-row tiles, one row per wave -- three
    // alternations on one box (r02as): 0.940 -> 0.901 ms at 12 MP (6.03 TB/s), C4 0.641 -> 0.614 ms, C5 unchanged
    case ADMM_K1_TV_W:
      return half_in ? K1Launch{k_admm_spatial_v4<4, NT, false, true>, 4, TW4, smem4(4) / 2}
                     : K1Launch{k_admm_spatial_v4<4, NT, false>, 4, TW4, smem4(4)};
    case ADMM_K1_TILED: return {k_admm_spatial_v4<8, NT>, 8, TW4, smem4(8)};
    default: return {k_admm_spatial<16, 64, NT>, 16, 64, (size_t)(2 * 18 * 66 + 17 * 64 + 16 * 65) * sizeof(real)};
  }
}

int admm_iterate(Engine* e, int n_iter) {
  const PlaneGeom& g = e->g;
  const LaunchPlan& pl = e->plan;
  bool sb_rows_valid = false;   // AdmmScalars::skipa may rely on the rows of SB only after a step of this very call
  bool a_done = false;          // ... and the previous step of this call has left the window's rows of `a` there too (hv_fuse)
  for (int it = 0; it < n_iter; ++it) {
    real* Vc = e->admm.V[e->admm.vcur];
    real* Vo = e->admm.V[e->admm.vcur ^ 1];
    double par[4];
    admm_params(e, e->iters_done, par);
    AdmmScalars sc = admm_scalars(e, par);
    sc.xi_store = (it + 1 == n_iter || !sc.xiw) ? 1 : 0;
    // rows wholly outside the sensor window: once an iteration of THIS call has run, SB still holds their row spectra
    // (sb_rows_valid: set below, local to the call -- no other entry point can have touched the work spectrum in
    // between); the last iteration runs complete (it stores xi out there), and the last three write H V there:
    // xi = mu1p (HV - HV_old) of the final X half and every read-out after the call need HV_{n-2}, HV_{n-1}, HV_n whole
    sc.skipa = (pl.hv_skip && sb_rows_valid && !sc.xi_store) ? 1 : 0;
    sc.skiphv = (pl.hv_skip && it + 3 < n_iter) ? 1 : 0;
    // duals half-applied between the iterations of this call (LaunchPlan::k1_half): the first iteration reads plain
    // duals, the last one writes them -- nothing outside this loop sees the other form
    sc.half_in = (pl.k1_half && it > 0) ? 1 : 0;
    sc.half_out = (pl.k1_half && it + 1 < n_iter) ? 1 : 0;
    // ... and under the same conditions rho~ is read back from r_sp and xi travels as -a inside the window
    // (LaunchPlan::rho_rsp, xi_half): both neighbours of the boundary are iterations of this call
    sc.rho_rsp = (pl.rho_rsp && sc.half_in) ? 1 : 0;
    sc.xi_in = (pl.xi_half && it > 0) ? 1 : 0;
    sc.xi_out = (pl.xi_half && it + 1 < n_iter) ? 1 : 0;
    // ADMM_K1_ROWS: the forward rows take the TV / W half as well -- same buffers, same ping-pong
    AdmmState& a = e->admm;
    const K1Rows k1 = {Vc, Vo, a.eta0[a.ecur], a.eta1[a.ecur], a.eta0[a.ecur ^ 1], a.eta1[a.ecur ^ 1], a.rho, pl.k1_xcd_order};
    if (pl.k1 != ADMM_K1_ROWS) {
      const K1Launch k = k1_launch(pl.k1, sc.half_in != 0);
      const unsigned tiles_x = (g.Wp + k.tw - 1) / k.tw, tiles_y = (g.Hp + k.th - 1) / k.th;
      LPC_OK(launch_k(e, LPC_K_SPATIAL, k.fn, dim3(tiles_x * tiles_y, e->P, 1), 256, k.smem, g, sc, (const real*)Vc,
                      (const real*)Vo, (const real*)a.HVb[a.hcur], (const real*)a.HVb[a.hcur ^ 1], a.xi,
                      (const real*)a.eta0[a.ecur], (const real*)a.eta1[a.ecur], a.eta0[a.ecur ^ 1], a.eta1[a.ecur ^ 1],
                      a.rho, (const real*)e->Y, a.Rsp, a.Aarr, tiles_x));
    }
    e->admm.vw_old = e->admm.vw_cur;          // this iteration's "V as W saw it" becomes the next one's "V_old as W_old saw it"
    e->admm.vw_cur = false;
    e->admm.ecur ^= 1;
    e->first = false;
    // (hcur still names the CURRENT H V here: the X half inside the forward rows reads HVb[hcur] and HVb[hcur ^ 1]
    // before the inverse rows of this same step overwrite HVb[hcur ^ 1] -- stream order)
    // H V on chip (LaunchPlan::hv_fuse): under the condition of skiphv -- the last three iterations of a call run complete --
    // this step's H V rows do the X half of iteration it + 1 themselves, with that iteration's scalars (mu1 is its step size,
    // mu1p this one's).  Iteration it + 1 is a steady-state one (xi half-applied on both sides, no xi_store, skipa): the form
    // k_rfwd_half_x_v2 would run.  The H V buffers keep flipping but are STALE from here until the last three iterations
    // rewrite them; nothing reads them in between: the tiled TV / W kernel does not, H V_old is not read with xi_in, the
    // tape records V, and every read-out comes after the call.
    const bool fuse = pl.hv_fuse && sc.skiphv && pl.xi_half && sc.xiw;
    AdmmScalars scn{};
    if (fuse) {
      double parn[4];
      admm_params(e, e->iters_done + 1, parn);
      scn = admm_scalars(e, parn, par);
    }
    LPC_OK(admm_spectral_step(e, sc, Vo, e->admm.HVb[e->admm.hcur ^ 1], pl.xhalf_rows, pl.k1 == ADMM_K1_ROWS ? &k1 : nullptr,
                              a_done, fuse ? &scn : nullptr));
    a_done = fuse;
    e->admm.vcur ^= 1;  // Vo now holds the new image estimate
    e->admm.hcur ^= 1;  // ... and the other H V buffer its forward model
    sb_rows_valid = true;   // the inverse column passes of this step left rfft(H V row) / Wp in every row of SB
    for (int k = 0; k < 4; ++k) e->admm.last_par[k] = par[k];
    LPC_OK(admm_tape_push(e, Vo));     // (recording: a stream-ordered copy; the kernels are the unrecorded forward's)
    ++e->iters_done;
  }
  return 0;
}

// ---- plug-and-play ADMM (section 8f row N4): one iteration split at the U-update ----
int admm_pnp_begin(Engine* e, int use_dual, real* dev_denoiser_in) {
  e->admm.pnp_mode = true;
  const PlaneGeom& g = e->g;
  const int nimg = e->cfg.batch * e->cfg.depth;
  real* src = e->admm.V[e->admm.vcur];                    // admm.py:242: denoiser(image_est)
  if (use_dual) {                               // admm.py:237-240: denoiser(U + eta / mu2)
    const long n = (long)g.rplane * e->P;
    LPC_OK(launch_k(e, -1, k_pnp_input<256>, grid1d(n, 256), 256, 0, e->admm.Rsp, (const real*)e->admm.eta1[0],
                    (const real*)e->admm.eta0[0], (real)e->cfg.mu2, n));
    src = e->admm.Rsp;
  }
  LPC_OK(planar_to_hwc(e, src, dev_denoiser_in, nimg, g.Hp, g.Wp, g.rpitch, g.rplane, 0, 0, 0));
  e->admm.pnp_pending = true;
  return 0;
}

int admm_pnp_end(Engine* e, int use_dual, const real* dev_U) {
  const PlaneGeom& g = e->g;
  const int nimg = e->cfg.batch * e->cfg.depth;
  real *eta = e->admm.eta0[0], *U = e->admm.eta1[0], *X = e->admm.eta0[1], *W = e->admm.eta1[1];
  LPC_OK(hwc_to_planar(e, dev_U, U, nimg, g.Hp, g.Wp, g.rpitch, g.rplane));
  double par[4];
  admm_params(e, e->iters_done, par);
  const AdmmScalars sc = admm_scalars(e, par);
  const dim3 grid = grid1d((long)g.Hp * g.Wp, 256, e->P);
  real* Vc = e->admm.V[e->admm.vcur];
  real* Vn = e->admm.V[e->admm.vcur ^ 1];
  real* HVn = e->admm.HVb[e->admm.hcur ^ 1];
  LPC_OK(launch_k(e, LPC_K_SPATIAL, k_pnp_pre<256>, grid, 256, 0, g, sc, use_dual ? 1 : 0, (const real*)Vc,
                  (const real*)e->admm.HVb[e->admm.hcur], (const real*)e->admm.xi, (const real*)e->admm.rho, (const real*)U,
                  (const real*)eta, (const real*)e->Y, X, W, e->admm.Rsp, e->admm.Aarr));
  LPC_OK(admm_spectral_step(e, sc, Vn, HVn));
  LPC_OK(launch_k(e, LPC_K_SPATIAL, k_pnp_post<256>, grid, 256, 0, g, sc, use_dual ? 1 : 0, (const real*)Vn,
                  (const real*)HVn, (const real*)X, (const real*)W, (const real*)U, e->admm.xi, eta, e->admm.rho));
  e->admm.vcur ^= 1;
  e->admm.hcur ^= 1;
  e->admm.pnp_pending = false;
  e->first = false;
  ++e->iters_done;
  return 0;
}

// ---- ADMM with a caller-supplied sparsifying operator (admm.py:104-120): one iteration around the caller's Psi / Psi^T ----
int admm_set_psi_gram(Engine* e, const real* dev_gabs) {
  const PlaneGeom& g = e->g;
  LPC_RT(rt::memset_async(e->admm.Gabs, 0, (size_t)g.cplane * sizeof(real), e->stream));
  LPC_OK(launch_k(e, -1, k_permute_spectrum_rows<256>, grid1d((long)g.Hp * g.Wc, 256), 256, 0, dev_gabs, e->admm.Gabs, g.Hp,
                  g.Wc, g.cpitch, e->plan.N1, e->plan.N2));
  e->admm.custom_gram = true;
  return admm_split_gram(e);
}

int admm_psi_step(Engine* e, const real* dev_psit) {
  e->admm.pnp_mode = true;       // explicit state from here on; lpc_iterate refuses until the next reset
  const PlaneGeom& g = e->g;
  const int nimg = e->cfg.batch * e->cfg.depth;
  real *T = e->admm.eta1[0], *X = e->admm.eta0[1], *W = e->admm.eta1[1];
  LPC_OK(hwc_to_planar(e, dev_psit, T, nimg, g.Hp, g.Wp, g.rpitch, g.rplane));
  double par[4];
  admm_params(e, e->iters_done, par);
  const AdmmScalars sc = admm_scalars(e, par);
  const dim3 grid = grid1d((long)g.Hp * g.Wp, 256, e->P);
  real* Vc = e->admm.V[e->admm.vcur];
  real* Vn = e->admm.V[e->admm.vcur ^ 1];
  real* HVn = e->admm.HVb[e->admm.hcur ^ 1];
  LPC_OK(launch_k(e, LPC_K_SPATIAL, k_pnp_pre<256>, grid, 256, 0, g, sc, 2, (const real*)Vc,
                  (const real*)e->admm.HVb[e->admm.hcur], (const real*)e->admm.xi, (const real*)e->admm.rho, (const real*)T,
                  (const real*)e->admm.eta0[0], (const real*)e->Y, X, W, e->admm.Rsp, e->admm.Aarr));
  LPC_OK(admm_spectral_step(e, sc, Vn, HVn));
  LPC_OK(launch_k(e, LPC_K_SPATIAL, k_pnp_post<256>, grid, 256, 0, g, sc, 0, (const real*)Vn, (const real*)HVn,
                  (const real*)X, (const real*)W, (const real*)T, e->admm.xi, e->admm.eta0[0], e->admm.rho));   // xi and rho (eta is the caller's)
  e->admm.vcur ^= 1;
  e->admm.hcur ^= 1;
  e->first = false;
  ++e->iters_done;
  return 0;
}

int admm_form_image(Engine* e, real* dev_out) {
  const PlaneGeom& g = e->g;
  const int nimg = e->cfg.batch * e->cfg.depth;
  if (e->has_init && e->iters_done == 0 && e->init_est) {
    // Right after reset() the reference's state still ALIASES the stored initial estimate (admm.py:154-155,
    // `self._image_est = self._initial_est`), so this read-out's in-place clamp (admm.py:337) lands in the initial
    // estimate too: every later reset() starts from the clamped one.  (apply(plot/save=...) does exactly this
    // before its loop, recon.py:563-566.)
    LPC_OK(launch_k(e, -1, k_clamp_window_inplace<256>, grid1d((long)g.H * g.W, 256, e->P), 256, 0, g, e->init_est));
  }
  if (e->admm.pnp_mode) {   // explicit state: the clamp really is in place
    LPC_OK(planar_to_hwc(e, e->admm.V[e->admm.vcur], dev_out, nimg, g.H, g.W, g.rpitch, g.rplane, g.sh, g.sw, 1));
    return launch_k(e, -1, k_clamp_window_inplace<256>, grid1d((long)g.H * g.W, 256, e->P), 256, 0, g,
                    e->admm.V[e->admm.vcur]);
  }
  // crop + clamp (admm.py:331-338)
  LPC_OK(planar_to_hwc(e, e->admm.V[e->admm.vcur], dev_out, nimg, g.H, g.W, g.rpitch, g.rplane, g.sh, g.sw, 1));
  // ... which the reference applies IN PLACE to its state: the W-updates of the next two iterations see the clamped
  // estimate (everything else keeps using the un-clamped V, exactly like the reference's cached _Psi_out /
  // _forward_out do).  clamp(V) is recomputed where it is needed (AdmmScalars::clamp_cur / clamp_old): no copy.
  e->admm.vw_cur = true;
  return 0;
}

int admm_get_state(Engine* e, const std::string& nm, real* dev_out) {
  const PlaneGeom& g = e->g;
  const int nimg = e->cfg.batch * e->cfg.depth;
  auto out_padded = [&](real* src) {
    return planar_to_hwc(e, src, dev_out, nimg, g.Hp, g.Wp, g.rpitch, g.rplane, 0, 0, 0);
  };
  if (e->admm.pnp_mode) {   // explicit state arrays; U and eta are image-shaped here
    if (nm == "image_est") return out_padded(e->admm.V[e->admm.vcur]);
    if (nm == "forward_out") return out_padded(e->admm.HVb[e->admm.hcur]);
    if (nm == "xi") return out_padded(e->admm.xi);
    if (nm == "rho") return out_padded(e->admm.rho);
    if (nm == "eta") return out_padded(e->admm.eta0[0]);
    if (nm == "U") return out_padded(e->admm.eta1[0]);
    if (nm == "X") return out_padded(e->admm.eta0[1]);
    if (nm == "W") return out_padded(e->admm.eta1[1]);
    return fail("lpc_get_state: unknown name '" + nm + "'");
  }
  if (nm == "image_est")     // after a read-out: the clamped estimate, like the reference's attribute
    return planar_to_hwc(e, e->admm.V[e->admm.vcur], dev_out, nimg, g.Hp, g.Wp, g.rpitch, g.rplane, 0, 0,
                         e->admm.vw_cur ? 2 : 0);
  if (nm == "forward_out") return out_padded(e->admm.HVb[e->admm.hcur]);
  // the rest needs the pending dual update applied: materialise what was asked for into the two padded arrays that are
  // idle between iterations (r_sp and a: no allocation, no host synchronisation)
  int w0 = -1, w1 = -1;
  if (nm == "xi") w0 = 0;
  else if (nm == "rho") w0 = 3;
  else if (nm == "W") w0 = 6;
  else if (nm == "X") w0 = 7;
  else if (nm == "eta") { w0 = 1; w1 = 2; }
  else if (nm == "U") { w0 = 4; w1 = 5; }
  else return fail("lpc_get_state: unknown name '" + nm + "'");
  double par[4];
  admm_params(e, e->iters_done, par);
  AdmmScalars sc = admm_scalars(e, par);
  sc.clamp_old = e->admm.vw_old ? 1 : 0;
  const AdmmState& a = e->admm;
  LPC_OK(launch_k(e, -1, k_admm_flush<256>, grid1d((long)g.Hp * g.Wp, 256, e->P), 256, 0, g, sc,
                  (const real*)a.V[a.vcur], (const real*)a.V[a.vcur ^ 1], (const real*)a.HVb[a.hcur],
                  (const real*)a.HVb[a.hcur ^ 1], (const real*)e->Y, (const real*)a.xi, (const real*)a.eta0[a.ecur],
                  (const real*)a.eta1[a.ecur], (const real*)a.rho, a.Rsp, w1 >= 0 ? a.Aarr : (real*)nullptr, w0,
                  w1 >= 0 ? w1 : 0));
  if (w1 < 0) return out_padded(e->admm.Rsp);
  return planar2_to_hwc2(e, e->admm.Rsp, e->admm.Aarr, dev_out, nimg);
}

int admm_kernel_bytes(Engine* e, int kid, double* bytes) {
  const PlaneGeom& g = e->g;
  const LaunchPlan& pl = e->plan;
  const double eb = (double)sizeof(real);             // 4 (liblpc) or 8 (liblpc_f64)
  const double R = eb * g.Hp * g.Wp * e->P;           // padded real arrays, all planes
  const double S = 2 * eb * g.Hp * g.Wc * e->P;       // half spectra
  const double R0 = eb * g.H * g.W * e->Pdata;
  const double Sc = 2 * eb * g.Hp * g.Wc * e->Ppsf;   // spectral constants
  const bool split = pl.N1 > 1, k1_rows = pl.k1 == ADMM_K1_ROWS;
  // fr R, fr S with fr = H / Hp: the window's rows of a padded array / of a half spectrum (whole numbers, like every term here)
  const double Rh = eb * g.H * g.Wp * e->P, Sh = 2 * eb * g.H * g.Wc * e->P;
  const double nxw = pl.xi_half ? 2.0 : 3.0;          // arrays the X half moves where xi lives: xi in, xi out (+ H V_old)
  double b = 0.0;
  switch (kid) {
    // SURVEY 8(d) figure for the stand-alone kernel (reads 8R+R0, writes 7R; the kernel itself moves 14R + R0: X is
    // recomputed instead of stored).  Fused into the forward rows it reads 8R + R0 (V, V_old, HV, HV_old, xi, eta0,
    // eta1, rho; y) and writes xi, eta0, eta1, rho (4R) + the two row spectra (2S): r_sp and a never reach HBM.
    // X half in the forward rows (default with compile-time row plans): the tiled kernel reads V, V_old, eta0, eta1,
    // rho and writes eta0, eta1, rho, r_sp = 9R (SURVEY's 15R + R0 minus its X part: reads HV, X, xi, y, writes xi, X,
    // a); the row kernel reads r_sp (R) and xi, HV, HV_old, y (3R + R0), writes xi (R) and the two spectra (2S).
    // ... and without V_old once the duals travel half-applied between the iterations of a call (k1_half): 8R
    // ... and without rho in either direction once rho~ is recovered from r_sp, read in place of it (rho_rsp): 7R
    // ... k1_rows (small frames): not launched; the forward rows read V, eta0, eta1, rho (+ V_old without k1_half)
    // instead of r_sp and write eta0, eta1, rho: + 6R (7R)
    case LPC_K_SPATIAL: b = k1_rows ? 0.0 : pl.xhalf_rows ? (pl.rho_rsp ? 7.0 : pl.k1_half ? 8.0 : 9.0) * R : 15.0 * R + R0; break;
    // ... with xi confined to the sensor window (AdmmScalars::xiw) the row kernel reads r_sp, HV everywhere (2R) and
    // xi, HV_old / writes xi only over the window (3 window-sized arrays per plane) and y: 2R + 3 Rw + R0 + 2S
    // ... and with the H V row transforms skipped on rows wholly outside the window (AdmmScalars::skipa, steady state
    // of a long call; fr = H / Hp): rows fwd (1 + fr) R + 3 Rw + R0 + (1 + fr) S, rows inv (1 + fr) (S + R)
    // ... and with xi half-applied between the iterations of a call (xi_half) H V_old is not read where xi is: 2 Rw
    // ... and with H V on chip (hv_fuse, the steady state of a call): rows fwd R + S (r_sp alone); rows inv = the rows of
    // V, S + R, + the fused rows of the window, 2 fr S + 2 Rw + R0 -- the row of H V (2 fr R in all) does not move
    case LPC_K_ROW_FWD: b = (pl.hv_fuse ? R + S : pl.hv_skip ? R + Rh + nxw * eb * g.H * g.W * e->P + R0 + S + Sh
                                : pl.xi_window ? 2.0 * R + nxw * eb * g.H * g.W * e->P + R0 + 2.0 * S
                                : pl.xhalf_rows ? (2.0 + nxw) * R + R0 + 2.0 * S : 2.0 * R + 2.0 * S)
                               + (k1_rows ? (pl.k1_half ? 6.0 : 7.0) * R : 0.0); break;
    case LPC_K_COL_A_FWD: b = split ? 4.0 * S : 0.0; break;
    case LPC_K_COL_MID: b = 4.0 * S + Sc + (e->admm.g_sep ? 0. : eb * g.Hp * g.Wc); break;  // + H (complex) + |G| (real, one plane; two vectors when it separates)
    case LPC_K_COL_A_INV: b = split ? 4.0 * S : 0.0; break;
    case LPC_K_ROW_INV: b = pl.hv_fuse ? S + R + 2.0 * Sh + 2.0 * eb * g.H * g.W * e->P + R0
                               : pl.hv_skip ? S + Sh + R + Rh : 2.0 * S + 2.0 * R; break;
    default: return fail("bad kernel id");
  }
  *bytes = b;
  return 0;
}

double admm_model_bytes(const Engine* e) {
  const PlaneGeom& g = e->g;
  const double eb = (double)sizeof(real);
  const double R = eb * g.Hp * g.Wp * e->P, S = 2 * eb * g.Hp * g.Wc * e->P;
  // one PSF per frame: every frame's middle reads spectral constants of its own (shared, they are read once per batch and
  // stay out of the model)
  const double Sc = e->psf_per_frame ? 2 * eb * g.Hp * g.Wc * e->Ppsf : 0.0;
  return 19.0 * R + eb * g.H * g.W * e->Pdata + 13.5 * S + Sc;
}
