// lpc_gd.cpp -- launches of the gradient-descent family's fused row kernels (see lpc_engine.h for the split)
#include "lpc_gd_launch.h"

// spectrum rows of H x (Sin) -> irfft -> shift + crop -> - y -> re-pad -> rfft -> spectrum rows (Sout); the iteration's
// own pair is e->S -> e->gd.S2
int gd_rows_mid(Engine* e, const real2* Sin, real2* Sout) {
  const PlaneGeom& g = e->g;
  const int nblk = (g.H + 1) / 2;
  if (e->mod && e->mod->gd_rows_mid) return e->mod->gd_rows_mid(e, Sin, Sout);
  if (e->plan.rows_half)
    return dispatch_row(g.Wp / 2, e->planWh.skew_ok, false, [&](auto NT, auto EM, auto SK, auto) {
      return launch_gd_rows_mid_half<NT.value, EM.value, SK.value>(e, e->planWh, Sin, Sout);
    });
  return dispatch_row(g.Wp, e->planW.skew_ok, e->rows_r2, [&](auto NTc, auto EM, auto SK, auto R2) {
    constexpr int nt = decltype(NTc)::value, em = decltype(EM)::value;
    constexpr bool sk = decltype(SK)::value, r2 = decltype(R2)::value;
    return launch_k(e, LPC_K_ROW_INV, k_rinv_gd_mid<nt, em, sk, r2>, dim3(nblk, e->P), nt,
                    LPC_ROW_SMEM_BYTES(g.Wp, sk), g, e->planW, e->rows_r2 ? e->planWi : e->planW,
                    Sin, Sout, (const real*)e->Y);
  });
}
