// lpc_launch.h -- the launch of every hot-loop kernel that runs on a run-time plan (Fft1dPlan, core library) as well as
// on a compile-time plan (SPlanArg, plan module): one function template per kernel family, over the workgroup shape, the
// layout flags and the plan-argument type PA.  It alone names the kernel, builds its grid, sizes its LDS and lists its
// arguments; the core calls it from dispatch_row / dispatch_cfg, lpc_module.cpp with its constants.  A template is
// instantiated where it is called, so each kernel is still compiled in the unit that launches it.  (Included by
// lpc_rows.cpp, lpc_cols.cpp, lpc_module.cpp and the gradient-descent family's launch headers, lpc_gd_launch.h and
// lpc_gd_bwd_launch.h.)
#pragma once
#include "lpc_engine.h"
#include "lpc_row_kernels.h"
#include "lpc_col_kernels.h"

static inline real2* spec_b(const Engine* e) { return e->S + (size_t)e->P * e->g.cplane; }   // second work spectrum (ADMM)
static inline real inv_points(const PlaneGeom& g) { return (real)1.0 / ((real)g.Hp * (real)g.Wp); }   // unnormalised FFT pair
// the half-length inverse rows' grid.x by the rows of H V they write (k_rinv_half: skip_b_outside)
static inline unsigned admm_rows_inv_grid(const PlaneGeom& g, int hv_rows) {
  return (unsigned)(hv_rows == ADMM_HV_ROWS_NONE ? g.Hp : hv_rows == ADMM_HV_ROWS_WINDOW ? g.Hp + g.H : 2 * g.Hp);
}
static inline PlaneGeom geom_rev(const Engine* e, bool rev) {   // the launch's copy of the geometry (PlaneGeom::rev)
  PlaneGeom g = e->g;
  g.rev = rev ? 1 : 0;
  return g;
}

// ---- rows, one real row per half-length transform (pa: the plan of length Wp / 2) ------------------------------
template <int NT, int EM, int SK, class PA>
static inline int launch_rows_fwd_half(Engine* e, const PA& pa, const RealSrc& src, real2* S, int nplanes, int kid) {
  return launch_k(e, kid, k_rfwd_rows_half<NT, EM, SK, PA>, dim3(src.nrows, nplanes), NT,
                  LPC_ROW_SMEM_BYTES(e->g.Wp / 2, SK), e->g, pa, e->planW.tw, src, S);
}
template <int NT, int EM, int SK, class PA>
static inline int launch_rows_inv_half(Engine* e, const PA& pa, const real2* S, const RealDst& dst, int nplanes, int kid) {
  return launch_k(e, kid, k_rinv_rows_half<NT, EM, SK, PA>, dim3(dst.nrows, nplanes), NT,
                  LPC_ROW_SMEM_BYTES(e->g.Wp / 2, SK), e->g, pa, e->planW.tw, S, dst);
}
// ADMM: e->admm.Rsp, e->admm.Aarr -> the two work spectra, and back to V, H V (hv_rows: ADMM_HV_ROWS_*)
template <int NT, int EM, int SK, class PA>
static inline int launch_admm_rows_fwd_half(Engine* e, const PA& pa) {
  return launch_k(e, LPC_K_ROW_FWD, k_rfwd_half<NT, EM, SK, PA>, dim3(2 * e->g.Hp, e->P), NT,
                  LPC_ROW_SMEM_BYTES(e->g.Wp / 2, SK), e->g, pa, e->planW.tw, (const real*)e->admm.Rsp, (const real*)e->admm.Aarr,
                  e->S, spec_b(e));
}
template <int NT, int EM, int SK, class PA>
static inline int launch_admm_rows_inv_half(Engine* e, const PA& pa, real* Vout, real* HVout, int hv_rows) {
  const PlaneGeom& g = e->g;
  return launch_k(e, LPC_K_ROW_INV, k_rinv_half<NT, EM, SK, PA>, dim3(admm_rows_inv_grid(g, hv_rows), e->P), NT,
                  LPC_ROW_SMEM_BYTES(g.Wp / 2, SK), g, pa, e->planW.tw, (const real2*)e->S, (const real2*)spec_b(e),
                  Vout, HVout, hv_rows);
}

// ---- ADMM rows, two real rows per complex transform of length Wp (SL: PlanSpec::slay) ---------------------------
template <int NT, int EM, int SK, bool R2, int SL, class PA>
static inline int launch_admm_rows_fwd_paired(Engine* e, const PA& pa) {
  return launch_k(e, LPC_K_ROW_FWD, k_rfwd_arrays<NT, EM, SK, R2, PA, SL>, dim3(paired_rows_grid(e->g, false), e->P), NT,
                  LPC_ROW_SMEM_BYTES(e->g.Wp, SK), e->g, pa, (const real*)e->admm.Rsp, (const real*)e->admm.Aarr, e->S, spec_b(e));
}
template <int NT, int EM, int SK, bool R2, int SL, class PA>
static inline int launch_admm_rows_inv_paired(Engine* e, const PA& pa, real* Vout, real* HVout, bool skip_hv) {
  return launch_k(e, LPC_K_ROW_INV, k_rinv_arrays<NT, EM, SK, R2, PA, SL>, dim3(paired_rows_grid(e->g, skip_hv), e->P), NT,
                  LPC_ROW_SMEM_BYTES(e->g.Wp, SK), e->g, pa, (const real2*)e->S, (const real2*)spec_b(e), Vout, HVout,
                  skip_hv ? 1 : 0);
}

// ---- columns -----------------------------------------------------------------------------------------------
// plain pass over `nplanes` planes of S in place.  TWLDS: the plan's and the four-step twiddles sit behind the tile
template <int NT, int EM, int SBT, bool TWLDS, class PA>
static inline int launch_cols(Engine* e, const PA& pa, const ColPass& cp, real2* S, int nplanes, bool inverse, int kid) {
  const dim3 grid(cp.G * cp.ntile_c, nplanes);
  const size_t smem = (size_t)cp.N * (cp.T + (TWLDS ? 2 : 0)) * sizeof(real2);
  if (inverse) return launch_k(e, kid, k_cols<NT, EM, true, PA, SBT, TWLDS>, grid, NT, smem, e->g, pa, cp, S);
  return launch_k(e, kid, k_cols<NT, EM, false, PA, SBT, TWLDS>, grid, NT, smem, e->g, pa, cp, S);
}
// ADMM fused middle, both work spectra side by side in LDS: [N][2 T].  TWLDS: the plan's twiddles behind the tile;
// SL: the work spectra, H and |G| in pair lines (PlanSpec::slay)
template <int NT, int EM, int SBT2, bool TWLDS, int SL, class PA>
static inline int launch_admm_mid(Engine* e, const PA& pa, const ColPass& cp, const AdmmScalars& sc, real sb_outside_scale) {
  return launch_k(e, LPC_K_COL_MID, k_cols_mid_admm<NT, EM, PA, SBT2, TWLDS, SL>, dim3(cp.G * cp.ntile_c, e->P), NT,
                  (size_t)cp.N * (2 * cp.T + (TWLDS ? 1 : 0)) * sizeof(real2), e->g, pa, cp, e->S, spec_b(e),
                  (const real2*)(SL ? e->admm.Hs_t : e->Hs), (const real*)(SL ? e->admm.Gabs_t : e->admm.Gabs), (const real2*)e->phr,
                  (const real2*)e->phc, make_fastdiv((unsigned)(2 * cp.T)), sc.mu1, sc.mu2, sc.mu3, inv_points(e->g),
                  sb_outside_scale);
}
