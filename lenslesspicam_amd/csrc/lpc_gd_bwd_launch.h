// lpc_gd_bwd_launch.h -- lpc_gd_launch.h for the reverse-mode row kernels of unrolled FISTA (lpc_gd_bwd_kernels.h): the
// half-row launches, written once for the core's run-time plans and the plan modules' compile-time plans.
#pragma once
#include "lpc_launch.h"
#include "lpc_gd_bwd_kernels.h"

// MODE 0: head of the last iteration -> rows (e->S);  1: rows (e->S) -> Hg, g_b -> rows (e->gd.S2);
// 2: rows (e->gd.S2) -> gy -> head of the iteration before (or the tail) -> rows (e->S);  3: rows (Sin) -> the PSF
// gradient's accumulator, no rows out.  pa: the plan of length Wp / 2
template <int MODE, int NT, int EM, int SK, class PA>
static inline int launch_gd_bwd_half(Engine* e, const PA& pa, const GdBwd& a, const real2* Sin = nullptr) {
  return launch_k(e, -1, k_gd_bwd_half<MODE, NT, EM, SK, PA>, dim3(e->g.H, e->P), NT,
                  gd_bwd_red_bytes<NT>() + LPC_ROW_SMEM_BYTES(e->g.Wp / 2, SK),
                  geom_rev(e, MODE == 1 || MODE == 3 ? e->plan.gd_rev_resid : e->plan.gd_rev_update), pa, e->planW.tw,
                  MODE == 3 ? Sin : (const real2*)(MODE == 1 ? e->S : e->gd.S2),
                  MODE == 3 ? (real2*)nullptr : MODE == 1 ? e->gd.S2 : e->S, a);
}
