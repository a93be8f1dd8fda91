// lpc_gd_bwd.cpp -- launches of the reverse-mode row kernels of unrolled FISTA (see lpc_engine.h for the split)
#include "lpc_gd_bwd_launch.h"

// mode 0 / 1 / 2: head, middle rows, update + next head;  3: rows of Sin -> the PSF gradient's accumulator
// (lpc_gd_bwd_kernels.h)
int gd_bwd_rows(Engine* e, int mode, const GdBwd& a, const real2* Sin) {
  const PlaneGeom& g = e->g;
  if (e->mod && e->mod->gd_bwd_head) {
    if (mode == 3) return e->mod->gd_bwd_acc(e, &a, Sin);
    if (mode == 0) return e->mod->gd_bwd_head(e, &a);
    return mode == 1 ? e->mod->gd_bwd_mid(e, &a) : e->mod->gd_bwd_update(e, &a);
  }
  if (e->plan.rows_half)
    return dispatch_row(g.Wp / 2, e->planWh.skew_ok, false, [&](auto NT, auto EM, auto SK, auto) {
      if (mode == 0) return launch_gd_bwd_half<0, NT.value, EM.value, SK.value>(e, e->planWh, a);
      if (mode == 1) return launch_gd_bwd_half<1, NT.value, EM.value, SK.value>(e, e->planWh, a);
      if (mode == 3) return launch_gd_bwd_half<3, NT.value, EM.value, SK.value>(e, e->planWh, a, Sin);
      return launch_gd_bwd_half<2, NT.value, EM.value, SK.value>(e, e->planWh, a);
    });
  const int nblk = (g.H + 1) / 2;
  return dispatch_row(g.Wp, e->planW.skew_ok, false, [&](auto NTc, auto EM, auto SK, auto) {
    constexpr int nt = decltype(NTc)::value, em = decltype(EM)::value;
    constexpr bool sk = decltype(SK)::value;
    const size_t smem = gd_bwd_red_bytes<nt>() + LPC_ROW_SMEM_BYTES(g.Wp, sk);
    if (mode == 0)
      return launch_k(e, -1, k_gd_bwd_paired<0, nt, em, sk>, dim3(nblk, e->P), nt, smem, g, e->planW,
                      (const real2*)e->gd.S2, e->S, a);
    if (mode == 1)
      return launch_k(e, -1, k_gd_bwd_paired<1, nt, em, sk>, dim3(nblk, e->P), nt, smem, g, e->planW,
                      (const real2*)e->S, e->gd.S2, a);
    if (mode == 3)
      return launch_k(e, -1, k_gd_bwd_paired<3, nt, em, sk>, dim3(nblk, e->P), nt, smem, g, e->planW, Sin,
                      (real2*)nullptr, a);
    return launch_k(e, -1, k_gd_bwd_paired<2, nt, em, sk>, dim3(nblk, e->P), nt, smem, g, e->planW,
                    (const real2*)e->gd.S2, e->S, a);
  });
}

// the PSF gradient's finishing sum over the batch (k_gd_bwd_gpsf): acc [B*C][H][W] -> (1, H, W, C)
int gd_bwd_psf_sum(Engine* e, const real* acc, real* grad_psf) {
  const PlaneGeom& g = e->g;
  return launch_k(e, -1, k_gd_bwd_gpsf<256>, grid1d(g.uplane, 256, e->cfg.channels), 256, 0, acc, grad_psf, (long)g.uplane,
                  e->cfg.channels, e->cfg.batch);
}
