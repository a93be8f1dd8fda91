// lpc_admm_row_kernels.h -- the forward rows of an ADMM iteration with image-domain work fused in: k_rfwd_half_x (the X
// half; one real row per half-length transform) and k_rfwd_arrays_x (paired rows; the X half, with K1 the TV / W half
// too).  Compile-time plans only: held by plan modules (lpc_module.cpp), never by the library.  Their second form:
// lpc_admm_v2_kernels.h.
#pragma once
#include "lpc_row_kernels.h"
#include "lpc_admm_kernels.h"
// ---- forward rows of r_sp and a, with the X half of the image-domain work (wide frames: one real row per half-length
// transform) -------------------------------------------------------------------------------------------------------
// The image-domain work of an ADMM iteration separates cleanly:
//   r_sp = (mu3 W - rho') + Psi^T(mu2 U - eta')  depends on V, V_old, eta, rho only and needs neighbours (TV stencil),
//   a    = mu1 X - xi'                           depends on xi, HV, HV_old, y only and needs nothing but its own pixel.
// The tiled kernel (k_admm_spatial_v4<.., XHALF = false>) keeps the stencil half at its own occupancy and writes r_sp;
// here block (row, 0) transforms that stored row exactly like k_rfwd_half, and block (row, 1) COMPUTES the row of `a`
// (and the pending xi update) from xi, HV, HV_old, y in registers and transforms it: `a` never exists in HBM and the
// tiled kernel no longer touches xi, HV, HV_old, y (-2R per iteration).  Same arithmetic, statement for statement, as
// the X part of k_admm_spatial_v4.  grid = (2 * Hp, planes); `plan` has length Wp/2, `twW` is the length-Wp table.
// (Three ways to split the image-domain work were built and measured, profiles/r02_notes.md: the stand-alone kernel,
// everything inside the forward rows -- its stencil half then runs at the row kernel's 4 workgroups per CU, no faster
// than the pair once the rows run on compile-time plans -- and this one, a win on every box and shape.)
template <int NT, int EMAX, int SK, class PL = Fft1dPlan>
__global__ __launch_bounds__(NT) void k_rfwd_half_x(PlaneGeom g, AdmmScalars p, PL plan, const real2* LPC_RESTRICT twW,
                                                     const real* LPC_RESTRICT Rsp, const real* LPC_RESTRICT HV,
                                                     const real* LPC_RESTRICT HVold, real* LPC_RESTRICT xi,
                                                     const real* LPC_RESTRICT Y, real2* LPC_RESTRICT SA,
                                                     real2* LPC_RESTRICT SB) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT);
  // No row needs a neighbour, and rows inside the sensor window cost more than rows outside (AdmmScalars::xiw): bands of
  // rows per XCD would leave the XCDs that hold the window rows working while the others idle, so rows go round-robin
  // over the XCDs (block b runs on XCD b % 8: the even XCDs transform the rows of r_sp, the odd ones form and transform
  // the rows of `a` -- about twice the work per row, on half of the rows once those outside the window are skipped.
  // Flipping the pair every fourth row to mix both kinds on every XCD measured SLOWER: 0.47 -> 0.60 ms, r02ak; a compact
  // grid without the empty blocks of skipped `a` rows measured the same: 0.498 / 0.480 vs 0.499 / 0.481 ms, r02an)
  const unsigned bx = LPC_BX(g);
  const int gr = (int)(bx >> 1), arr = (int)(bx & 1);
  const long pl = LPC_BY(g);
  const long poff = pl * g.rplane;
  const long o_row = poff + (long)gr * g.rpitch;
  const int n4 = g.Wp >> 2;
  if (arr == 1 && p.skipa && (gr < g.sh || gr >= g.sh + g.H)) return;   // AdmmScalars::skipa (uniform per block)
  if (arr == 0) {      // the stored row of r_sp: first stage fused into the fill, like k_rfwd_half
    const real2* a2 = (const real2*)(Rsp + o_row);
    auto src = [&](int i, int) { return a2[i]; };
    fft_tile<NT, EMAX, false, SK, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, src, LdsNatural{});
    untangle_half_store<NT, SK>(s, g.Wp >> 1, twW, SA + pl * g.cplane + (long)gr * g.cpitch, tid);
    return;
  }
  {
    const int dpl = (int)(pl / g.DC) * g.C + (int)(pl % g.C);
    const bool row_in = (gr >= g.sh) && (gr < g.sh + g.H);
    const real* y = Y + (long)dpl * g.uplane + (long)(gr - g.sh) * g.W;     // dereferenced only when row_in
    const bool y4 = ((g.sw | g.W) & 3) == 0;                                 // window and pitch allow real4 loads of y
    XQuad nxt = xhalf_load(g, p, HV, HVold, xi, y, o_row, row_in, y4, tid < n4 ? tid : 0);
#pragma unroll 1
    for (int q = tid; q < n4; q += NT) {
      const int gc = 4 * q;
      const XQuad c = nxt;
      if (q + NT < n4) nxt = xhalf_load(g, p, HV, HVold, xi, y, o_row, row_in, y4, q + NT);
      real xin[4], as[4];
      xhalf_apply(p, c, xin, as);
      if (!c.skip || p.xi_store) st4(xi + o_row + gc, make_real4(xin[0], xin[1], xin[2], xin[3]));
      s[lds_slot<SK>(2 * q)] = make_real2(as[0], as[1]);
      s[lds_slot<SK>(2 * q + 1)] = make_real2(as[2], as[3]);
    }
  }
  __syncthreads();
  fft_tile<NT, EMAX, false, SK, false>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, LdsNatural{});
  untangle_half_store<NT, SK>(s, g.Wp >> 1, twW, SB + pl * g.cplane + (long)gr * g.cpitch, tid);
}

// ---- paired forward rows with the X half computed on the fly (narrow frames: C1 / C4, 760 x 1014) ---------------
// Same split of the image-domain work as k_rfwd_half_x, for frames whose rows ride in pairs (paired_rows_of: two rows of
// ONE array per transform).  Blocks of array 0 transform two stored rows of r_sp (k_admm_spatial_v4<.., XHALF = false>
// wrote them); blocks of array 1 form two rows of a = mu1 X - xi' element by element from xi, HV, HV_old and y inside
// the source functor of the first FFT stage (which also stores xi').  p.skipa: `a` on the rows of the sensor window
// alone -- outside it a = mu1 HV needs no transform, SB keeps the row spectra the last inverse row pass read and the
// fused middle rescales them (AdmmScalars::skipa).  Compile-time plans only.
#ifndef LPC_K1ROWS_MINW
#define LPC_K1ROWS_MINW 1
#endif
#ifndef LPC_RFWDX_MINW
#define LPC_RFWDX_MINW 1
#endif
// K1 (rows of at most 4 NT columns): the blocks of array 0 form their two rows of r_sp themselves (k1_two_rows: V,
// V_old, eta, rho in; eta', rho' out) instead of reading what the tiled kernel stored -- that kernel is not launched.
template <int NT, int EMAX, int SK, class PL, bool K1 = false, int SL = 0>
__global__ __launch_bounds__(NT, K1 ? LPC_K1ROWS_MINW : NT == 256 ? LPC_RFWDX_MINW : 1) void k_rfwd_arrays_x(PlaneGeom g, AdmmScalars p, PL plan, const real* LPC_RESTRICT Rsp,
                                                       const real* LPC_RESTRICT HV, const real* LPC_RESTRICT HVold,
                                                       real* LPC_RESTRICT xi, const real* LPC_RESTRICT Y,
                                                       real2* LPC_RESTRICT SA, real2* LPC_RESTRICT SB, K1Rows k1) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT);
  LPC_STAMP_BEGIN(1);
  unsigned bx = LPC_BX(g), by = LPC_BY(g);
  if (K1 && k1.xcd_order) {
    // XCD-aware order (workgroup w runs on XCD w % 8, each with its own L2): the blocks of r_sp read V at rows r0 - 1 and
    // r0 + 2 and eta at row r0 + 2 -- rows that belong to the neighbouring row pairs, which in launch order sit on OTHER
    // XCDs.  Here every XCD walks a contiguous eighth of the (plane, row pair) space.  The host asks for it on small
    // launches only (same box, trees: C1 0.217 -> 0.212 ms, 380 x 507 0.281 -> 0.269 ms per 5 iterations; 8 frames
    // unchanged; C4's 64 frames 0.815 -> 0.855 ms per launch -- profiles/r05zb_xcd_order_trees.log)
    const unsigned gx = gridDim.x, total = gx * gridDim.y, lin = bx + gx * by;
    unsigned l2 = lin;
    if (k1.xcd_order < 0) {
      const unsigned qd = total >> 3, rm = total & 7u, xcd = lin & 7u, idx = lin >> 3;
      l2 = (xcd < rm ? xcd * (qd + 1u) : rm * (qd + 1u) + (xcd - rm) * qd) + idx;
    } else {
      // large launches: runs of G consecutive row blocks per XCD inside spans of 8 G blocks -- the eight XCDs stay within
      // 8 G rows of one another (one stream through every array, not eight), and only one block in G has its
      // neighbours' rows on another XCD
      const unsigned G = (unsigned)k1.xcd_order, span = 8u * G, full = total - total % span;
      if (lin < full) {
        const unsigned c = lin / span, w = lin - c * span;
        l2 = c * span + (w & 7u) * G + (w >> 3);
      }
    }
    by = l2 / gx;
    bx = l2 - by * gx;
  }
  const long pl = by;
  const PairedRows pr = paired_rows_of(g, bx, p.skipa != 0);
  const bool v1 = pr.second;
  const long o_row = pl * g.rplane + (long)pr.r0 * g.rpitch;
  if (K1 && pr.arr == 0) {
    if constexpr (K1) {
      static_assert((PL::n >> 2) <= 2 * NT, "one or two quads per lane and row");
      const long po = pl * g.rplane;
#pragma unroll
      for (int q = tid; q < (PL::n >> 2); q += NT)
        k1_two_rows<SK>(g, p, k1.V + po, k1.Vold + po, k1.eta0 + po, k1.eta1 + po, k1.eta0_out + po, k1.eta1_out + po,
                        k1.rho + po, pr.r0, v1, q, s);
      __syncthreads();
      fft_tile<NT, EMAX, false, SK, false>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, LdsNatural{});
      real2* o0 = SA + pl * g.cplane + (long)pr.r0 * g.cpitch;
      untangle_store<NT, SK, SL>(s, g.Wp, g.Wc, o0, o0 + (SL ? 8 : g.cpitch), v1, tid);
      LPC_STAMP_END();
    }
    return;
  }
  if (pr.arr == 0) {
    const real* ra = Rsp + o_row;
    const real* rb = ra + g.rpitch;
    auto two = [&](int i, int) { return make_real2(ra[i], v1 ? rb[i] : (real)0.); };
    fft_tile<NT, EMAX, false, SK, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, two, LdsNatural{});
    real2* o0 = SA + pl * g.cplane + (long)pr.r0 * g.cpitch;
    untangle_store<NT, SK, SL>(s, g.Wp, g.Wc, o0, o0 + (SL ? 8 : g.cpitch), v1, tid);
    LPC_STAMP_END();
    return;
  }
  // two rows of a = mu1 X - xi' (xhalf_load / xhalf_apply): every 16-byte load of both rows is in flight before the
  // first statement that needs one, the pair of rows goes into the tile as z = a_r0 + i a_r1, then the transform runs
  // from LDS.  (The first form of this kernel formed `a` inside the source functor of the first FFT stage -- one load,
  // one wait, one store at a time behind four data-dependent branches per element; with two rows per block that chain
  // was the whole kernel: C1 0.272 -> 0.293 ms per 5 iterations, r04a/ab_pairing.log.)
  const int dpl = (int)(pl / g.DC) * g.C + (int)(pl % g.C);
  const int r1 = pr.r0 + 1, n4 = g.Wp >> 2;
  const bool v0 = pr.first;     // (false: the row above a window that starts on an odd row -- read like any row outside
                                // the window, neither stored nor transformed)
  const bool in0 = (pr.r0 >= g.sh) && (pr.r0 < g.sh + g.H), in1 = v1 && (r1 >= g.sh) && (r1 < g.sh + g.H);
  const real* y0 = Y + (long)dpl * g.uplane + (long)(pr.r0 - g.sh) * g.W;    // dereferenced only inside the window
  const real* y1 = y0 + g.W;
  const long o_row1 = o_row + g.rpitch;
  const bool y4 = ((g.sw | g.W) & 3) == 0;
  // (compile-time plans: Wp == PL::n.  One quad per lane when the row fits the workgroup -- no loop, no second set of
  // quads in flight: 88 -> VGPRs of the one-trip form, and with them the number of workgroups a CU holds; at C1 1620
  // workgroups are launched and only 1280 of the two-set form were resident, profiles/r05_notes.md section 5)
  constexpr int N4C = PL::n >> 2;
  if constexpr (N4C <= NT) {
    if (tid < N4C) {
      const int gc = 4 * tid;
      const XQuad c0 = xhalf_load(g, p, HV, HVold, xi, y0, o_row, in0, y4, tid);
      const XQuad c1 = xhalf_load(g, p, HV, HVold, xi, y1, v1 ? o_row1 : o_row, in1, y4, tid);
      real x0[4], a0[4], x1[4], a1[4];
      xhalf_apply(p, c0, x0, a0);
      xhalf_apply(p, c1, x1, a1);
      if (v0 && (!c0.skip || p.xi_store)) st4(xi + o_row + gc, make_real4(x0[0], x0[1], x0[2], x0[3]));
      if (v1 && (!c1.skip || p.xi_store)) st4(xi + o_row1 + gc, make_real4(x1[0], x1[1], x1[2], x1[3]));
#pragma unroll
      for (int i = 0; i < 4; ++i) s[lds_slot<SK>(gc + i)] = make_real2(v0 ? a0[i] : (real)0., v1 ? a1[i] : (real)0.);
    }
  } else {
    const int q0 = tid < n4 ? tid : 0;
    XQuad n0 = xhalf_load(g, p, HV, HVold, xi, y0, o_row, in0, y4, q0);
    XQuad n1 = xhalf_load(g, p, HV, HVold, xi, y1, v1 ? o_row1 : o_row, in1, y4, q0);
#pragma unroll 1
    for (int q = tid; q < n4; q += NT) {
      const int gc = 4 * q;
      const XQuad c0 = n0, c1 = n1;
      if (q + NT < n4) {
        n0 = xhalf_load(g, p, HV, HVold, xi, y0, o_row, in0, y4, q + NT);
        n1 = xhalf_load(g, p, HV, HVold, xi, y1, v1 ? o_row1 : o_row, in1, y4, q + NT);
      }
      real x0[4], a0[4], x1[4], a1[4];
      xhalf_apply(p, c0, x0, a0);
      xhalf_apply(p, c1, x1, a1);
      if (v0 && (!c0.skip || p.xi_store)) st4(xi + o_row + gc, make_real4(x0[0], x0[1], x0[2], x0[3]));
      if (v1 && (!c1.skip || p.xi_store)) st4(xi + o_row1 + gc, make_real4(x1[0], x1[1], x1[2], x1[3]));
#pragma unroll
      for (int i = 0; i < 4; ++i) s[lds_slot<SK>(gc + i)] = make_real2(v0 ? a0[i] : (real)0., v1 ? a1[i] : (real)0.);
    }
  }
  __syncthreads();
  fft_tile<NT, EMAX, false, SK, false>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, LdsNatural{});
  real2* o1 = SB + pl * g.cplane + (long)pr.r0 * g.cpitch;
  untangle_store<NT, SK, SL>(s, g.Wp, g.Wc, o1, o1 + (SL ? 8 : g.cpitch), v1, tid, v0);
  LPC_STAMP_END();
}
