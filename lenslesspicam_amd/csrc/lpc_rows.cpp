// lpc_rows.cpp -- launches of every row pass (see lpc_engine.h for the split of the library)
#include "lpc_launch.h"

// ------------------------------------------------------------- 2-D transform pieces --
// forward rows of ONE real source (pairs of rows) into spectrum S (planes = nplanes)
int rows_fwd_single(Engine* e, const RealSrc& src, real2* S, int nplanes, int kid) {
  const PlaneGeom& g = e->g;
  if (e->mod && e->mod->rows_fwd_single) return e->mod->rows_fwd_single(e, &src, S, nplanes, kid);
  if (e->plan.rows_half)
    return dispatch_row(g.Wp / 2, e->planWh.skew_ok, false, [&](auto NT, auto EM, auto SK, auto) {
      return launch_rows_fwd_half<NT.value, EM.value, SK.value>(e, e->planWh, src, S, nplanes, kid);
    });
  const int nblk = (src.nrows + 1) / 2;
  return dispatch_row(g.Wp, e->planW.skew_ok, e->rows_r2, [&](auto NT, auto EM, auto SK, auto R2) {
    constexpr int nt = decltype(NT)::value, em = decltype(EM)::value;
    constexpr bool sk = decltype(SK)::value, r2 = decltype(R2)::value;
    return launch_k(e, kid, k_rfwd_rows<nt, em, sk, r2>, dim3(nblk, nplanes), nt, LPC_ROW_SMEM_BYTES(g.Wp, sk), g,
                    e->planW, src, S);
  });
}

int rows_inv_single(Engine* e, const real2* S, const RealDst& dst, int nplanes, int kid) {
  const PlaneGeom& g = e->g;
  if (e->mod && e->mod->rows_inv_single) return e->mod->rows_inv_single(e, S, &dst, nplanes, kid);
  if (e->plan.rows_half)
    return dispatch_row(g.Wp / 2, e->planWh.skew_ok, false, [&](auto NT, auto EM, auto SK, auto) {
      return launch_rows_inv_half<NT.value, EM.value, SK.value>(e, e->planWh, S, dst, nplanes, kid);
    });
  const int nblk = (dst.nrows + 1) / 2;
  const Fft1dPlan& pinv = e->rows_r2 ? e->planWi : e->planW;
  return dispatch_row(g.Wp, pinv.skew_ok, e->rows_r2, [&](auto NT, auto EM, auto SK, auto R2) {
    constexpr int nt = decltype(NT)::value, em = decltype(EM)::value;
    constexpr bool sk = decltype(SK)::value, r2 = decltype(R2)::value;
    return launch_k(e, kid, k_rinv_rows<nt, em, sk, r2>, dim3(nblk, nplanes), nt, LPC_ROW_SMEM_BYTES(g.Wp, sk), g,
                    pinv, S, dst);
  });
}

// ---- ADMM: rows of r_sp and a (e->admm.Rsp, e->admm.Aarr) -> the two work spectra --------------------------------------
int admm_rows_fwd(Engine* e) {
  const PlaneGeom& g = e->g;
  if (e->mod && e->mod->admm_rows_fwd) return e->mod->admm_rows_fwd(e);
  if (e->plan.rows_half)
    return dispatch_row(g.Wp / 2, e->planWh.skew_ok, false, [&](auto NT, auto EM, auto SK, auto) {
      return launch_admm_rows_fwd_half<NT.value, EM.value, SK.value>(e, e->planWh);
    });
  return dispatch_row(g.Wp, e->planW.skew_ok, e->rows_r2, [&](auto NT, auto EM, auto SK, auto R2) {
    return launch_admm_rows_fwd_paired<NT.value, EM.value, SK.value, R2.value, 0>(e, e->planW);
  });
}

// ---- ADMM: the two work spectra -> V and H V (padded, no shift) ------------------------------------------------
int admm_rows_inv(Engine* e, real* Vout, real* HVout, int hv_rows) {
  if (e->mod && e->mod->admm_rows_inv) return e->mod->admm_rows_inv(e, Vout, HVout, hv_rows);
  if (hv_rows != ADMM_HV_ROWS_ALL) return fail("internal: skipping H V rows needs the plan module's row kernels");
  const PlaneGeom& g = e->g;
  const Fft1dPlan& pinv = e->rows_r2 ? e->planWi : e->planW;
  if (e->plan.rows_half)
    return dispatch_row(g.Wp / 2, e->planWh.skew_ok, false, [&](auto NT, auto EM, auto SK, auto) {
      return launch_admm_rows_inv_half<NT.value, EM.value, SK.value>(e, e->planWh, Vout, HVout, ADMM_HV_ROWS_ALL);
    });
  return dispatch_row(g.Wp, pinv.skew_ok, e->rows_r2, [&](auto NT, auto EM, auto SK, auto R2) {
    return launch_admm_rows_inv_paired<NT.value, EM.value, SK.value, R2.value, 0>(e, pinv, Vout, HVout, false);
  });
}
