// lpc_admm_v2_kernels.h -- ADMM's two half-length row kernels in the second form (compile-time one-radix plans, float32).
//
//   k_rinv_half_v2      spectrum row of S / SB -> irfft -> the padded real row of V / H V          (k_rinv_half)
//   k_rfwd_half_x_v2    the stored row of r_sp, or the row of a = mu1 X - xi' formed from xi~, H V, y in registers
//                       (+ the pending xi update) -> rfft -> spectrum row of S / SB                 (k_rfwd_half_x)
//   k_hv_rows_v2        both in one, in place on a row of SB inside the sensor window: the row of H V stays in registers
//
// The form is that of lpc_gd_v2_kernels.h, whose stages these kernels call: M / R lanes per row, every lane owns butterfly j
// of every stage; tangling + first inverse stage straight from global memory; the last stage ends in registers (lane j holds
// pairs j + (M / R) m, which is what it stores, and what the first forward stage wants); stage twiddles requested one stage
// ahead.  Against the first form (512 lanes of which 256 have a butterfly, tile through LDS before the first and behind the
// last stage, twiddles behind the stage's barrier): 5 + 5 LDS trips per row instead of 7 + 7, and the blocks of `a` issue
// all loads of a row in two batches instead of walking four quads per lane one HBM latency after the other.
//
// ARITHMETIC IS THE FIRST FORM'S: the same Dft<R> butterflies, the same lane-ordered stage twiddles in the same products
// (v2_tw_apply), the tangling twiddles are table entries (TC = false: the upper half of a lane's bins is -i times the
// lower half's entry, which is the entry the first form's mirrored statement uses, negated and conjugated), the same
// expressions in tangle / untangle and xhalf_elem for the pixels -- the two forms agree bit for bit and may alternate
// inside a call (tests/test_admm_rows_v2.py).
// Measured at 12 MP (profiles/admm_rows_v2_notes.md): the forward rows gain 8 % and are the default; the inverse rows, which
// read every spectrum element twice (the mirrored run comes from the L2) and have nothing but the transform to speed up,
// lose 10 % against the first form and stay behind option admm_rows_v2=3.
// Needs what GdV2 needs (one radix R = 8 | 16, M / R a multiple of 64) and, for the blocks of `a`, the pair geometry
// (window offset and frame width even); the planner checks (LaunchPlan::admm_rows_v2).
#pragma once
#include "lpc_gd_v2_kernels.h"
#include "lpc_admm_kernels.h"

#ifndef LPC_DOUBLE

// ---- inverse rows: grid mapping of k_rinv_half (array flip every fourth row, skip_b_outside) ----------------------------
template <int NT, int SK, class PL>
__global__ __launch_bounds__(NT, 4) void k_rinv_half_v2(PlaneGeom g, PL plan, const real2* LPC_RESTRICT twW,
                                                        const real2* LPC_RESTRICT SA, const real2* LPC_RESTRICT SB,
                                                        real* LPC_RESTRICT A, real* LPC_RESTRICT B, int skip_b_outside) {
  using P = typename PL::plan;
  constexpr int R = GdV2<P>::R, NB = GdV2<P>::NB, L = GdV2<P>::L;
  static_assert(GdV2<P>::ok && NT == NB, "k_rinv_half_v2: one butterfly per lane and stage");
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int j = LPC_TID(NT);
  const unsigned bx = LPC_BX(g);
  int row = bx >> 1, arr = (bx ^ (bx >> 3)) & 1;
  const long pl = LPC_BY(g);
  if (skip_b_outside == 2) {       // A alone, grid.x = Hp (LaunchPlan::hv_fuse)
    row = (int)bx;
    arr = 0;
  } else if (skip_b_outside) {     // AdmmScalars::skiphv, see k_rinv_half
    if ((int)bx < 2 * g.H) row += g.sh;
    else {
      const int q = (int)bx - 2 * g.H;
      row = q < g.sh ? q : q + g.H;
      arr = 0;
    }
  }
  real2 wb[4];
  v2_tw_load<P, 1>(plan.tws, j, wb);
  v2_load_tangle_first<P, SK, false>(s, (arr ? SB : SA) + pl * g.cplane + (long)row * g.cpitch, twW, j);
  v2_barrier();
  v2_mid_chain<P, SK, true>(s, plan.tws, j, wb, std::make_integer_sequence<int, L - 2>{});
  real2 v[R];
  v2_final_stage<P, SK, true, false>(s, plan.tws, j, wb, v);
  real2* o2 = (real2*)((arr ? B : A) + pl * g.rplane + (long)row * g.rpitch);
#pragma unroll
  for (int m = 0; m < R; ++m) o2[j + NB * m] = v[m];
}

// ---- forward rows with the X half: block roles, skipped `a` rows and XCD parity of k_rfwd_half_x -----------------------
// The steady state of a call only (the launcher checks): xi arrives and leaves half-applied (AdmmScalars::xi_in, xi_out) and
// H V_old is not read (no xi_store where xi lives inside the window alone).
// RSP_ONLY (LaunchPlan::hv_fuse): grid.x = Hp, the rows of r_sp alone -- the previous iteration's k_hv_rows_v2 has left
// the rows of `a` in SB already.
template <int NT, int SK, class PL, bool RSP_ONLY = false>
__global__ __launch_bounds__(NT, 4) void k_rfwd_half_x_v2(PlaneGeom g, AdmmScalars pin, PL plan, const real2* LPC_RESTRICT twW,
                                                          const real* LPC_RESTRICT Rsp, const real* LPC_RESTRICT HV,
                                                          real* LPC_RESTRICT xi, const real* LPC_RESTRICT Y,
                                                          real2* LPC_RESTRICT SA, real2* LPC_RESTRICT SB, FastDiv fdc,
                                                          FastDiv fc) {
  using P = typename PL::plan;
  constexpr int R = GdV2<P>::R, NB = GdV2<P>::NB, L = GdV2<P>::L, H = R / 2;
  static_assert(GdV2<P>::ok && NT == NB, "k_rfwd_half_x_v2: one butterfly per lane and stage");
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int j = LPC_TID(NT);
  const unsigned bx = LPC_BX(g);
  const int gr = RSP_ONLY ? (int)bx : (int)(bx >> 1), arr = RSP_ONLY ? 0 : (int)(bx & 1);
  const unsigned pl = LPC_BY(g);
  const long o_row = (long)pl * g.rplane + (long)gr * g.rpitch;
  const bool row_in = (gr >= g.sh) && (gr < g.sh + g.H);
  if (arr == 1 && pin.skipa && !row_in) return;   // AdmmScalars::skipa (uniform per block)
  real2 r[R], v[R];
  if (arr == 0) {      // the stored row of r_sp: every load of the lane in flight before the first butterfly
    const real2* a2 = (const real2*)(Rsp + o_row);
#pragma unroll
    for (int m = 0; m < R; ++m) r[m] = a2[j + NB * m];
  } else {
    AdmmScalars p = pin;
    p.first = 0; p.xi_in = 1; p.xi_out = 1;
    // xi travels where the first form's quads load and store it: on the whole row (xi_full), or on the quads that touch the
    // sensor window in a row of the window -- as a range-checked buffer (loads outside it return zero and move nothing,
    // stores are dropped); y likewise on the window's columns.  Padded pair i covers columns 2 i, 2 i + 1.
    const int x0 = p.xiw ? g.sw & ~3 : 0, x1 = p.xiw ? (g.sw + g.W + 3) & ~3 : g.Wp;
    const lpc_rsrc xr = lpc_make_rsrc(xi + o_row + x0, (p.xiw && !row_in) ? 0u : (unsigned)(x1 - x0) * (unsigned)sizeof(real));
    const lpc_rsrc yr = lpc_make_rsrc(Y + (long)v2_data_plane(pl, fdc, fc, g.C) * g.uplane + (long)(gr - g.sh) * g.W,
                                      row_in ? (unsigned)g.W * (unsigned)sizeof(real) : 0u);
    const real2* hv2 = (const real2*)(HV + o_row);
    const real ho = lpc_opaque_f((real)0.);      // H V_old, not read in the steady state (xhalf_apply2)
    // (byte offsets are recomputed where they are used -- one integer operation each -- instead of kept across the batch)
    auto xoff = [&](int m) { return lpc_opaque((2 * (j + NB * m) - x0) * (int)sizeof(real)); };
    auto yoff = [&](int m) { return lpc_opaque((2 * (j + NB * m) - g.sw) * (int)sizeof(real)); };
    auto loads = [&](int m0, real2* hh, real2* xx, real2* yy) {
#pragma unroll
      for (int m = 0; m < H; ++m) hh[m] = hv2[j + NB * (m0 + m)];
#pragma unroll
      for (int m = 0; m < H; ++m) xx[m] = lpc_buf_load2(xr, xoff(m0 + m));
#pragma unroll
      for (int m = 0; m < H; ++m) yy[m] = lpc_buf_load2(yr, yoff(m0 + m));
    };
    auto apply = [&](int m0, const real2* hh, const real2* xx, const real2* yy) {
#pragma unroll
      for (int m = 0; m < H; ++m) {
        const bool in = row_in && (unsigned)(2 * (j + NB * (m0 + m)) - g.sw) < (unsigned)g.W;
        real2 xn;
        xhalf_apply2(p, hh[m], xx[m], yy[m], in, ho, xn, r[m0 + m]);
        lpc_buf_store2(xr, xoff(m0 + m), xn);
      }
    };
    // two batches of R / 2 pairs, both in flight before the first use
    real2 h0[H], x0v[H], y0[H], h1[H], x1v[H], y1[H];
    loads(0, h0, x0v, y0);
    loads(H, h1, x1v, y1);
    LPC_SCHED_FENCE();
    apply(0, h0, x0v, y0);
    apply(H, h1, x1v, y1);
  }
  // (stage 1's twiddles behind the row's loads, not in front: the first butterfly does not wait for them, and the blocks of
  // `a` have no registers to spare while their two batches are in flight)
  real2 wb[4];
  v2_tw_load<P, 1>(plan.tws, j, wb);
  v2_first_fwd<P, SK>(s, j, r);
  v2_mid_chain<P, SK, false>(s, plan.tws, j, wb, std::make_integer_sequence<int, L - 2>{});
  v2_final_stage<P, SK, false, false>(s, plan.tws, j, wb, v);
  v2_barrier();
  v2_untangle_store<P, SK, false>(s, twW, j, v, (arr ? SB : SA) + (long)pl * g.cplane + (long)gr * g.cpitch);
}

// ---- H V rows on chip (LaunchPlan::hv_fuse): inverse row -> X half of the NEXT iteration -> forward row, in place in SB ---
// One workgroup per row of the sensor window and plane: k_rinv_half_v2 on the row of SB, whose last stage leaves lane j
// with pairs j + NB m of H V -- the pairs the blocks of `a` of k_rfwd_half_x_v2 load -- then that kernel's statements on
// them (pin: the NEXT iteration's scalars -- mu1 is its step size, mu1p this iteration's) and its forward transform into
// the same row.  The row of H V never reaches memory; xi~ and y travel as in k_rfwd_half_x_v2, the first half in flight
// across the last inverse stage.
// hv goes through lpc_opaque_v2: the unfused path rounds H V to a stored float32 before xhalf_elem sees it, and the
// compiler must not see through it to the butterfly either (the FMA contraction trap at xhalf_apply2).
template <int NT, int SK, class PL>
__global__ __launch_bounds__(NT, 4) void k_hv_rows_v2(PlaneGeom g, AdmmScalars pin, PL plan, const real2* LPC_RESTRICT twW,
                                                      real2* SB, real* LPC_RESTRICT xi, const real* LPC_RESTRICT Y,
                                                      FastDiv fdc, FastDiv fc) {
  using P = typename PL::plan;
  constexpr int R = GdV2<P>::R, NB = GdV2<P>::NB, L = GdV2<P>::L, H = R / 2;
  static_assert(GdV2<P>::ok && NT == NB, "k_hv_rows_v2: one butterfly per lane and stage");
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int j = LPC_TID(NT), u = (int)LPC_BX(g);      // grid.x = H: row u of the sensor window
  const unsigned pl = LPC_BY(g);
  const int gr = g.sh + u;
  real2* row = SB + (long)pl * g.cplane + (long)gr * g.cpitch;
  real2 wb[4];
  v2_tw_load<P, 1>(plan.tws, j, wb);
  v2_load_tangle_first<P, SK, false>(s, row, twW, j);
  v2_barrier();
  v2_mid_chain<P, SK, true>(s, plan.tws, j, wb, std::make_integer_sequence<int, L - 2>{});
  AdmmScalars p = pin;
  p.first = 0; p.xi_in = 1; p.xi_out = 1;
  // xi and y as range-checked buffers: the statements of k_rfwd_half_x_v2 on a row of the window
  const long o_row = (long)pl * g.rplane + (long)gr * g.rpitch;
  const int x0 = p.xiw ? g.sw & ~3 : 0, x1 = p.xiw ? (g.sw + g.W + 3) & ~3 : g.Wp;
  const lpc_rsrc xr = lpc_make_rsrc(xi + o_row + x0, (unsigned)(x1 - x0) * (unsigned)sizeof(real));
  const lpc_rsrc yr = lpc_make_rsrc(Y + (long)v2_data_plane(pl, fdc, fc, g.C) * g.uplane + (long)u * g.W,
                                    (unsigned)g.W * (unsigned)sizeof(real));
  const real ho = lpc_opaque_f((real)0.);      // H V_old, not read in the steady state (xhalf_apply2)
  auto xoff = [&](int m) { return lpc_opaque((2 * (j + NB * m) - x0) * (int)sizeof(real)); };
  auto yoff = [&](int m) { return lpc_opaque((2 * (j + NB * m) - g.sw) * (int)sizeof(real)); };
  auto loads = [&](int m0, real2* xx, real2* yy) {
#pragma unroll
    for (int m = 0; m < H; ++m) xx[m] = lpc_buf_load2(xr, xoff(m0 + m));
#pragma unroll
    for (int m = 0; m < H; ++m) yy[m] = lpc_buf_load2(yr, yoff(m0 + m));
  };
  real2 v[R], r[R];
  auto apply = [&](int m0, const real2* xx, const real2* yy) {
#pragma unroll
    for (int m = 0; m < H; ++m) {
      const bool in = (unsigned)(2 * (j + NB * (m0 + m)) - g.sw) < (unsigned)g.W;
      const real2 hv = lpc_opaque_v2(v[m0 + m]);
      real2 xn;
      xhalf_apply2(p, hv, xx[m], yy[m], in, ho, xn, r[m0 + m]);
      lpc_buf_store2(xr, xoff(m0 + m), xn);
    }
  };
  // Two halves of R / 2 pairs.  The first half's xi~ and y travel across the last inverse stage; the second half's are
  // requested behind the first half's arithmetic: with both halves and the butterfly's outputs alive at once the kernel
  // spills (76 - 160 bytes of scratch per lane in every order tried, profiles/hv_onchip_notes.md) -- this order holds 116
  // VGPRs and no scratch.  The forward transform's first stage twiddles come last.
  real2 xa[H], ya[H], xb[H], yb[H];
  loads(0, xa, ya);
  v2_final_stage<P, SK, true, false>(s, plan.tws, j, wb, v);
  LPC_SCHED_FENCE();
  apply(0, xa, ya);
  LPC_SCHED_FENCE();
  loads(H, xb, yb);
  LPC_SCHED_FENCE();
  apply(H, xb, yb);
  LPC_SCHED_FENCE();
  v2_tw_load<P, 1>(plan.tws, j, wb);
  v2_barrier();
  v2_first_fwd<P, SK>(s, j, r);
  v2_mid_chain<P, SK, false>(s, plan.tws, j, wb, std::make_integer_sequence<int, L - 2>{});
  v2_final_stage<P, SK, false, false>(s, plan.tws, j, wb, v);
  v2_barrier();
  v2_untangle_store<P, SK, false>(s, twW, j, v, row);
}

#endif   // !LPC_DOUBLE
