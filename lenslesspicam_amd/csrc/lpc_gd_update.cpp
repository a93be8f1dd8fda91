// lpc_gd_update.cpp -- launches of the gradient-descent update rows.  This kernel family is the longest to compile (the
// fused momentum / projection update behind an inverse row transform, one instantiation per workgroup shape), so it is
// spread over three translation units that the device compiler works on in parallel: this one (one real row per
// half-length transform) and lpc_gd_update_p0.cpp / lpc_gd_update_p1.cpp (paired rows without / with the folded radix-2
// stage).
#include "lpc_gd_launch.h"

int gd_rows_update_paired_r2(Engine* e, const GdScalars& sc, const real* alpha);   // lpc_gd_update_p1.cpp
int gd_rows_update_paired_plain(Engine* e, const GdScalars& sc, const real* alpha);   // lpc_gd_update_p0.cpp

// spectrum rows of the gradient (e->gd.S2) -> irfft -> shift + crop -> fused momentum / projection update of x
int gd_rows_update(Engine* e, const GdScalars& sc, const real* alpha) {
  const PlaneGeom& g = e->g;
  if (e->mod && e->mod->gd_rows_update) return e->mod->gd_rows_update(e, &sc, alpha);
  if (e->plan.rows_half)
    return dispatch_row(g.Wp / 2, e->planWh.skew_ok, false, [&](auto NT, auto EM, auto SK, auto) {
      return launch_gd_rows_update_half<NT.value, EM.value, SK.value>(e, e->planWh, sc, alpha);
    });
  return e->rows_r2 ? gd_rows_update_paired_r2(e, sc, alpha) : gd_rows_update_paired_plain(e, sc, alpha);
}
