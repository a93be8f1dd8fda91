// lpc_gd_launch.h -- lpc_launch.h for the gradient-descent family's fused row kernels.  Apart from it because
// lpc_gd_kernels.h also holds plain (non-template) kernels, which every unit that includes it compiles.
#pragma once
#include "lpc_launch.h"
#include "lpc_gd_kernels.h"

// one real row per half-length transform (pa: the plan of length Wp / 2): H x rows (Sin) -> residual -> rows (Sout);
// gradient rows (e->gd.S2) -> fused update of x
template <int NT, int EM, int SK, class PA>
static inline int launch_gd_rows_mid_half(Engine* e, const PA& pa, const real2* Sin, real2* Sout) {
  return launch_k(e, LPC_K_ROW_INV, k_rinv_gd_mid_half<NT, EM, SK, PA>, dim3(e->g.H, e->P), NT,
                  LPC_ROW_SMEM_BYTES(e->g.Wp / 2, SK), geom_rev(e, e->plan.gd_rev_resid), pa, e->planW.tw,
                  Sin, Sout, (const real*)e->Y);
}
template <int NT, int EM, int SK, class PA>
static inline int launch_gd_rows_update_half(Engine* e, const PA& pa, const GdScalars& sc, const real* alpha) {
  return launch_k(e, LPC_K_SPATIAL, k_rinv_gd_update_half<NT, EM, SK, PA>, dim3(e->g.H, e->P), NT,
                  LPC_ROW_SMEM_BYTES(e->g.Wp / 2, SK), geom_rev(e, e->plan.gd_rev_update), pa, e->planW.tw,
                  (const real2*)e->gd.S2, e->gd.gx, e->gd.gaux, alpha, sc);
}
