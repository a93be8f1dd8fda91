// lpc_admm_bwd.cpp -- reverse mode of unrolled ADMM (lpc_admm_record / lpc_admm_backward): the tape of iterates, the
// replay that rebuilds H V and the duals of every iteration from it, and the reverse sweep.  The image-domain kernels are
// lpc_admm_bwd_kernels.h; the spectral step of the sweep is the forward's own (lpc_admm.cpp: admm_spectral_plain).
#include "lpc_engine.h"
#include "lpc_admm_bwd_kernels.h"

static constexpr int kBwdTH = 8, kBwdQW = 32;      // k_admm_bwd_step: tiles of 8 rows x 128 columns on 256 lanes
static inline long bwd_tiles_x(const PlaneGeom& g) { return (g.Wp + 4 * kBwdQW - 1) / (4 * kBwdQW); }
static inline long bwd_tiles(const PlaneGeom& g) { return bwd_tiles_x(g) * ((g.Hp + kBwdTH - 1) / kBwdTH); }

// ---- the tape (struct Tape, lpc_engine.h): 6 n + 11 padded state arrays ----
int admm_tape_alloc(Engine* e) {
  const size_t n = e->admm.sched[0].size();
  if (!n) return 0;
  return tape_alloc(e, e->admm_tape, (int)n, 6 * n + 11, (size_t)e->g.rplane * e->P, n * e->P * bwd_tiles(e->g) * 4);
}
static inline real* tape_v(Engine* e, int i) { return e->admm_tape.at(i); }
static inline real* tape_hv(Engine* e, int i) { return e->admm_tape.at(e->admm_tape.n + 1 + i); }
static inline real* tape_dual(Engine* e, int which, int i) {      // which: 0 xi, 1 eta0, 2 eta1, 3 rho
  return e->admm_tape.at(2 * (e->admm_tape.n + 1) + (long)which * e->admm_tape.n + i);
}
static inline real* tape_work(Engine* e, int k) { return e->admm_tape.at(6 * e->admm_tape.n + 2 + k); }

int admm_tape_reset(Engine* e) {
  Tape& t = e->admm_tape;
  t.invalidate();
  // (an initial estimate, a caller's psi and plug-and-play iterations are not differentiated: nothing is recorded, and
  // lpc_admm_backward says why)
  if (!t.rec_on || e->admm.sched[0].empty() || e->has_init) return 0;
  LPC_OK(admm_tape_alloc(e));
  LPC_RT(rt::memset_async(tape_v(e, 0), 0, t.slot * sizeof(real), e->stream));     // V_0
  t.begin();
  return 0;
}

int admm_tape_push(Engine* e, const real* Vnew) {
  Tape& t = e->admm_tape;
  if (!t.wants(e->iters_done)) return 0;
  LPC_RT(rt::copy_d2d_async(tape_v(e, (int)e->iters_done + 1), Vnew, t.slot * sizeof(real), e->stream));
  t.advance();
  return 0;
}

static AdmmBwdScalars bwd_scalars(const Engine* e, int i, int n) {
  const std::vector<double>* s = e->admm.sched;
  AdmmBwdScalars p;
  p.m1 = (real)s[0][i]; p.m2 = (real)s[1][i]; p.m3 = (real)s[2][i];
  p.thr = (real)(s[3][i] / s[1][i]);
  p.m_in = (real)(1.0 / (1.0 + s[0][i])); p.m_out = (real)(1.0 / s[0][i]);
  p.r_m2 = (real)(1.0 / s[1][i]); p.r_m3 = (real)(1.0 / s[2][i]);
  p.pre = i > 0 ? 1 : 0;
  p.n1 = p.pre ? (real)s[0][i - 1] : (real)0.; p.n2 = p.pre ? (real)s[1][i - 1] : (real)0.;
  p.n3 = p.pre ? (real)s[2][i - 1] : (real)0.;
  p.gb_first = i == n - 1 ? 1 : 0;
  return p;
}

// full 2-D spectrum of P padded state arrays, in the PSF spectrum's own layout (the generic path of set_psf)
static int psf_spectrum(Engine* e, const real* x, real2* S) {
  LPC_OK(rows_fwd_single(e, src_padded(e, x), S, e->P, -1));
  return cols_fwd_full(e, S, e->P, 0, e->g.Hp);
}

// grad_psf (lpc_admm_backward_psf; the terms: lpc_admm_bwd_kernels.h) adds per iteration i, in front of its spectral
// step: a_i recomputed into `rbar` (free until that step writes it) and the full spectra of V_{i+1}, a_i and ab = Aarr
// (which k_admm_bwd_step of the same i overwrites); behind it the spectrum of rb and ONE k_admm_bwd_psf_acc.  After the
// sweep the accumulator goes through the convolution middle as the multiplier of a unit impulse's spectrum (= 1
// everywhere: the inverse column passes of the accumulator, 1 / (Hp Wp) folded in) and the inverse rows with the crop to
// the PSF window.  Without grad_psf nothing changes.  On a handle with one PSF per frame (lpc_per_frame_grad) the
// accumulate is k_admm_bwd_psf_acc_frames, the accumulator, the unit spectra, the middle's multiplier and the inverse rows
// are P planes instead of C, and grad_psf is (B,D,H,W,C).
int admm_backward(Engine* e, const real* grad_out, real* grad_data, real* grad_mu1, real* grad_mu2, real* grad_mu3,
                  real* grad_tau, real* grad_psf) {
  const PlaneGeom& g = e->g;
  Tape& t = e->admm_tape;
  const int n = t.n;
  const size_t rb_bytes = (size_t)g.rplane * e->P * sizeof(real);
  const dim3 pw = grid1d((long)g.Hp * g.Wp, 256, e->P);
  const size_t sp = (size_t)g.cplane * e->P;
  real2 *FV = nullptr, *FR = nullptr, *FA = nullptr, *FB = nullptr, *acc = nullptr;
  // one PSF per frame (lpc_set_psf_batch): nothing is summed over the batch, the accumulator holds a plane per state
  // plane and grad_psf is (B,D,H,W,C).  Everything else of the sweep finds a frame's own spectrum through PlaneGeom::PM
  // already: the replay's convolve_planar and admm_spectral_plain are the forward's
  const int accP = e->psf_per_frame ? e->P : g.C;
  if (grad_psf) {
    LPC_OK(tape_psf_ws(e, t, 2 * (4 * sp + (size_t)g.cplane * accP)));      // (in reals: spectra)
    FV = (real2*)t.psf_ws; FR = FV + sp; FA = FR + sp; FB = FA + sp; acc = FB + sp;
  }

  // ---- replay: H V_i and the duals every iteration started from ----
  LPC_RT(rt::memset_async(tape_hv(e, 0), 0, rb_bytes, e->stream));
  for (int k = 0; k < 4; ++k) LPC_RT(rt::memset_async(tape_dual(e, k, 0), 0, rb_bytes, e->stream));
  for (int i = 1; i <= n; ++i) LPC_OK(convolve_planar(e, tape_v(e, i), tape_hv(e, i), e->P, true, false));
  for (int i = 0; i + 1 < n; ++i)
    LPC_OK(launch_k(e, -1, k_admm_bwd_replay<256>, pw, 256, 0, g, bwd_scalars(e, i, n), (const real*)tape_v(e, i),
                    (const real*)tape_hv(e, i), (const real*)tape_v(e, i + 1), (const real*)tape_hv(e, i + 1),
                    (const real*)e->Y, (const real*)tape_dual(e, 0, i), (const real*)tape_dual(e, 1, i),
                    (const real*)tape_dual(e, 2, i), (const real*)tape_dual(e, 3, i), tape_dual(e, 0, i + 1),
                    tape_dual(e, 1, i + 1), tape_dual(e, 2, i + 1), tape_dual(e, 3, i + 1)));

  // ---- the start: vb = pad(dL/dout [crop(V_n) > 0]), every other adjoint 0, so r_sp = vb and a = 0 ----
  real *xib = tape_work(e, 0), *rhob = tape_work(e, 1);      // work 2 .. 5: etab0[0], etab1[0], etab0[1], etab1[1]
  real *rbar = tape_work(e, 6), *hr = tape_work(e, 7), *gb = grad_data ? tape_work(e, 8) : nullptr;
  LPC_RT(rt::memset_async(xib, 0, 4 * rb_bytes, e->stream));
  LPC_RT(rt::memset_async(e->admm.Rsp, 0, rb_bytes, e->stream));
  LPC_RT(rt::memset_async(e->admm.Aarr, 0, rb_bytes, e->stream));
  LPC_OK(hwc_to_planar(e, grad_out, e->admm.Rsp + (long)g.sh * g.rpitch + g.sw, e->cfg.batch, g.H, g.W, g.rpitch, g.rplane));
  LPC_OK(launch_k(e, -1, k_admm_bwd_seed<256>, grid1d((long)g.H * g.W, 256, e->P), 256, 0, g, (const real*)tape_v(e, n),
                  e->admm.Rsp));

  // ---- the sweep: one spectral step and one image-domain launch per iteration ----
  const long tiles = bwd_tiles(g);
  int cur = 0;
  for (int i = n - 1; i >= 0; --i) {
    const double par[4] = {e->admm.sched[0][i], e->admm.sched[1][i], e->admm.sched[2][i], e->admm.sched[3][i]};
    if (grad_psf) {
      LPC_OK(launch_k(e, -1, k_admm_bwd_arec<256>, pw, 256, 0, g, bwd_scalars(e, i, n), (const real*)tape_hv(e, i),
                      (const real*)tape_dual(e, 0, i), (const real*)e->Y, rbar));
      LPC_OK(psf_spectrum(e, rbar, FA));
      LPC_OK(psf_spectrum(e, tape_v(e, i + 1), FV));
      LPC_OK(psf_spectrum(e, e->admm.Aarr, FB));
    }
    LPC_OK(admm_spectral_plain(e, par, rbar, hr));
    if (grad_psf) {
      LPC_OK(psf_spectrum(e, rbar, FR));
      if (e->psf_per_frame)
        LPC_OK(launch_k(e, -1, k_admm_bwd_psf_acc_frames<256>, dim3((unsigned)((g.Wc + 255) / 256), (unsigned)g.Hp, (unsigned)e->P),
                        256, 0, g, (real)(2.0 * par[0]), (const real2*)FV, (const real2*)FR, (const real2*)FA,
                        (const real2*)FB, (const real2*)e->Hs, (const real2*)e->phr, (const real2*)e->phc, acc,
                        i == n - 1 ? 1 : 0));
      else
      LPC_OK(launch_k(e, -1, k_admm_bwd_psf_acc<256>, dim3((unsigned)((g.Wc + 255) / 256), (unsigned)g.Hp, (unsigned)g.C),
                      256, 0, g, e->cfg.batch, (real)(2.0 * par[0]), (const real2*)FV, (const real2*)FR, (const real2*)FA,
                      (const real2*)FB, (const real2*)e->Hs, (const real2*)e->phr, (const real2*)e->phc, acc,
                      i == n - 1 ? 1 : 0));
    }
    AdmmBwd a;
    a.V = tape_v(e, i); a.V2 = tape_v(e, i + 1); a.HV = tape_hv(e, i); a.HV2 = tape_hv(e, i + 1);
    a.xi = tape_dual(e, 0, i); a.eta0 = tape_dual(e, 1, i); a.eta1 = tape_dual(e, 2, i); a.rho = tape_dual(e, 3, i);
    a.Y = e->Y; a.rb = rbar; a.hr = hr; a.xib = xib; a.rhob = rhob;
    a.eb0 = tape_work(e, 2 + 2 * cur); a.eb1 = tape_work(e, 3 + 2 * cur);
    a.eb0o = tape_work(e, 2 + 2 * (cur ^ 1)); a.eb1o = tape_work(e, 3 + 2 * (cur ^ 1));
    a.gb = gb; a.Rsp = e->admm.Rsp; a.Aarr = e->admm.Aarr;
    a.part = t.part + (size_t)i * e->P * tiles * 4;
    LPC_OK(launch_k(e, -1, k_admm_bwd_step<kBwdTH, kBwdQW>, dim3((unsigned)tiles, e->P, 1), kBwdTH * kBwdQW,
                    admm_bwd_step_smem<kBwdTH, kBwdQW>(), g, bwd_scalars(e, i, n), a, (unsigned)bwd_tiles_x(g)));
    cur ^= 1;
    LPC_OK(launch_k(e, -1, k_admm_bwd_finish<256>, dim3(1), 256, admm_bwd_red_bytes<256>(), (const double*)a.part,
                    (long)e->P * tiles, par[3] / (par[1] * par[1]), 1.0 / par[1], grad_mu1 + i, grad_mu2 + i, grad_mu3 + i,
                    grad_tau + i));
  }
  if (grad_data) LPC_OK(gd_bwd_gdata(e, gb, grad_data));
  if (grad_psf) {
    // rbar, hr are free again: one padded plane with a unit impulse at the origin, read as every channel's plane
    LPC_RT(rt::memset_async(rbar, 0, (size_t)g.rplane * sizeof(real), e->stream));
    LPC_OK(fill_planar(e, rbar, 1, (real)1.));
    RealSrc unit = src_padded(e, rbar);
    unit.plane_stride = 0;
    LPC_OK(rows_fwd_single(e, unit, FV, accP, -1));
    LPC_OK(conv_middle(e, FV, accP, false, 0, g.Hp, true, acc, accP));
    LPC_OK(rows_inv_single(e, FV, dst_cropped(e, hr), accP, -1));
    LPC_OK(planar_to_hwc(e, hr, grad_psf, accP / g.C, g.H, g.W, g.W, g.uplane, 0, 0, 0));
  }
  return 0;
}
