// lpc_cols.cpp -- launches of every column pass (see lpc_engine.h for the split of the library)
#include "lpc_launch.h"

// column pass A (only when split) over nplanes planes; inverse => conj twiddles before FFT
int cols_passA(Engine* e, real2* S, int nplanes, bool inverse, int zr0, int zr1, int kid,
                      bool crop_rows_only, real sb_outside_scale) {
  if (e->plan.N1 == 1) return 0;
  const PlaneGeom& g = e->g;
  ColPass cp = e->passA;
  cp.tw_mode = inverse ? 2 : 1;
  cp.zr0 = zr0; cp.zr1 = zr1;
  cp.rev = (inverse ? e->plan.rev_passa_inv : e->plan.rev_passa_fwd) ? 1 : 0;
  if (!inverse && sb_outside_scale != (real)0.) {   // ADMM work spectra: planes [P, 2P) = SB, rows outside the window
    cp.sc_plane0 = e->P; cp.sc_r0 = g.sh; cp.sc_r1 = g.sh + g.H; cp.sc = sb_outside_scale;
  }
  if (inverse && crop_rows_only) {   // the row pass that follows reads spectrum rows (sh + u + Hp/2) mod Hp, u < H
    cp.need0 = (g.sh + g.Hp / 2) % g.Hp;
    cp.needn = g.H;
  }
  if (e->mod && e->mod->cols_passA) return e->mod->cols_passA(e, &cp, S, nplanes, inverse ? 1 : 0, kid);
  return dispatch_cfg(cp.N * cp.T, [&](auto NT, auto EM) {
    return launch_cols<NT.value, EM.value, 0, false>(e, e->planA, cp, S, nplanes, inverse, kid);
  });
}

// plain forward pass B (setup transforms only)
int cols_passB_fwd(Engine* e, real2* S, int nplanes, int zr0, int zr1) {
  ColPass cp = e->passB;
  cp.tw_mode = 0;
  cp.zr0 = zr0; cp.zr1 = zr1;
  return dispatch_cfg(cp.N * cp.T, [&](auto NT, auto EM) {
    return launch_cols<NT.value, EM.value, 0, false>(e, e->planB, cp, S, nplanes, false, -1);
  });
}

// middle of a convolution on S (nplanes): [A] -> B fwd * H * B inv -> [A inv]
int conv_middle(Engine* e, real2* S, int nplanes, bool adjoint, int zr0, int zr1,
                       bool crop_rows_only, const real2* mult, int mult_planes) {
  const PlaneGeom& g = e->g;
  const real2* Hs = mult ? mult : e->Hs;
  const int hplanes = mult ? mult_planes : e->Ppsf;
  const bool split = e->plan.N1 > 1;
  if (split) LPC_OK(cols_passA(e, S, nplanes, false, zr0, zr1, LPC_K_COL_A_FWD));
  ColPass cp = e->passB;
  cp.zr0 = split ? 0 : zr0;
  cp.zr1 = split ? g.Hp : zr1;
  const dim3 grid(cp.G * cp.ntile_c, nplanes);
  const real hscale = inv_points(g);
  // LaunchPlan::conv_mid_reg: one lane = one whole pass-B column transform in registers
  auto reg_mid = [&](auto kernel) {
    const dim3 rgrid((g.Wc + 63) / 64, cp.G, nplanes);
    return launch_k(e, LPC_K_COL_MID, kernel, rgrid, 64, 0, geom_rev(e, e->plan.gd_rev_mid), e->planB, cp, S,
                    Hs, adjoint ? 1 : 0, hscale, hplanes);
  };
  const int regN = e->plan.conv_mid_reg;
  if (regN == 48) { LPC_OK(reg_mid(k_cols_mid_mul_reg<8, 6>)); }
  else if (regN == 40) { LPC_OK(reg_mid(k_cols_mid_mul_reg<8, 5>)); }
  else if (regN == 36) { LPC_OK(reg_mid(k_cols_mid_mul_reg<6, 6>)); }
  else if (regN == 32) { LPC_OK(reg_mid(k_cols_mid_mul_reg<8, 4>)); }
  else if (regN == 30) { LPC_OK(reg_mid(k_cols_mid_mul_reg<6, 5>)); }
  else if (regN == 24) { LPC_OK(reg_mid(k_cols_mid_mul_reg<8, 3>)); }
  else
  LPC_OK(dispatch_cfg(cp.N * cp.T, [&](auto NT, auto EM) {
    constexpr int nt = decltype(NT)::value, em = decltype(EM)::value;
    return launch_k(e, LPC_K_COL_MID, k_cols_mid_mul<nt, em>, grid, nt, (size_t)cp.N * cp.T * sizeof(real2), g,
                    e->planB, cp, S, Hs, adjoint ? 1 : 0, hscale, hplanes);
  }));
  if (split) LPC_OK(cols_passA(e, S, nplanes, true, 0, g.Hp, LPC_K_COL_A_INV, crop_rows_only));
  return 0;
}

// ---- ADMM: [pass A] -> fused middle (V-hat, H V-hat) -> [inverse pass A] on the two work spectra ----------------
int admm_cols(Engine* e, const AdmmScalars& sc) {
  const PlaneGeom& g = e->g;
  const bool split = e->plan.N1 > 1;
  // sc.skipa: the rows of SB outside the sensor window were not re-transformed, they still hold what the last inverse
  // row pass consumed = rfft(HV row) / Wp; a = mu1 HV there
  if (split) LPC_OK(cols_passA(e, e->S, 2 * e->P, false, 0, g.Hp, LPC_K_COL_A_FWD, false,
                               sc.skipa ? sc.mu1 * (real)g.Wp : (real)0.));
  {
    ColPass cp = e->passB;
    cp.ga = e->admm.g_sep ? e->admm.Ga : nullptr;
    cp.gb = e->admm.g_sep ? e->admm.Gb : nullptr;
    cp.rev = e->plan.rev_mid ? 1 : 0;
    cp.swz = e->plan.mid_swz;
    const AdmmMid mid = e->plan.admm_mid;
    if (mid == ADMM_MID_REG24) {
      LPC_OK(launch_k(e, LPC_K_COL_MID, k_cols_mid_admm_reg<8, 3>, dim3((g.Wc + 63) / 64, cp.G, e->P), 64, 0, g, e->planB,
                      cp, e->S, spec_b(e), (const real2*)e->Hs, (const real*)e->admm.Gabs, (const real2*)e->phr,
                      (const real2*)e->phc, sc.mu1, sc.mu2, sc.mu3, inv_points(g)));
    } else if (mid == ADMM_MID_MODULE) {   // compile-time plan in LDS: both spectra side by side, or one at a time
      if (e->admm.midc && !(e->admm.midc_valid && e->admm.midc_par[0] == (double)sc.mu1 && e->admm.midc_par[1] == (double)sc.mu2 &&
                       e->admm.midc_par[2] == (double)sc.mu3)) {      // k_mid_consts: once per (PSF, step sizes)
        const long n = (long)((g.Hp + 1) & ~1) * g.cpitch;
        auto consts = [&](auto kernel) {
          return launch_k(e, -1, kernel, grid1d(n, 256, e->Ppsf), 256, 0, (const real2*)e->admm.Hs_t, (const real*)e->admm.Gabs_t,
                          cp.ga, cp.gb, (const real2*)e->phr, (const real2*)e->phc, g.Hp, g.Wc, g.cpitch, g.cplane, sc.mu1,
                          sc.mu2, sc.mu3, inv_points(g), e->admm.midc, e->admm.midrd);
        };
        if (e->plan.spec.mid_pc == 2) LPC_OK(consts(k_mid_consts<256, true>));
        else LPC_OK(consts(k_mid_consts<256, false>));
        e->admm.midc_par[0] = (double)sc.mu1; e->admm.midc_par[1] = (double)sc.mu2; e->admm.midc_par[2] = (double)sc.mu3;
        e->admm.midc_valid = true;
      }
      LPC_OK(e->mod->admm_mid(e, &cp, &sc, (sc.skipa && !split) ? sc.mu1 * (real)g.Wp : (real)0.));
    } else if (mid == ADMM_MID_RT_512X18) {
      LPC_OK((launch_admm_mid<512, 18, 0, false, 0>(e, e->planB, cp, sc, (real)0.)));
    } else
    LPC_OK(dispatch_cfg(cp.N * cp.T * 2, [&](auto NT, auto EM) {
      return launch_admm_mid<NT.value, EM.value, 0, false, 0>(e, e->planB, cp, sc, (real)0.);
    }));
  }
  if (split) LPC_OK(cols_passA(e, e->S, 2 * e->P, true, 0, g.Hp, LPC_K_COL_A_INV));
  return 0;
}
