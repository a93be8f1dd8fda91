// lpc_admm_kernels.h -- ADMM in the image domain: the pixel arithmetic (w_sees, div_by, soft_thresh_dev, tv_component,
// xhalf_*, k1_two_rows) that the stand-alone kernels here, the fused forward rows (lpc_admm_row_kernels.h,
// lpc_admm_v2_kernels.h) and the reverse mode (lpc_admm_bwd_kernels.h) share, and the kernels only lpc_admm.cpp
// launches: k_admm_spatial, k_admm_spatial_v4, k_pnp_*, k_admm_flush.
#pragma once
#include "lpc_args.h"
// ============================================================ ADMM spatial kernel ==
// K1: everything of one ADMM iteration that lives in the image domain, in ONE pass:
//   (pending) dual updates of the previous iteration  xi, eta, rho
//   U  = soft(Psi V + eta/mu2, tau/mu2)     X = M (xi + mu1 HV + pad(y))     W = max(rho/mu3 + V, 0)
//   r_sp = (mu3 W - rho) + Psi^T(mu2 U - eta)           a = mu1 X - xi
// U and W are never stored: the previous iteration's U, W are recomputed from V_old (kept by
// ping-ponging the V buffer), which replaces 3 reads + 3 writes of padded arrays by 1 read.
// V / V_old tiles (+1 halo) and q = mu2 U - eta (+1 row / +1 col) are staged in LDS.
// eta is read at halo pixels owned by neighbouring workgroups, so its update is written to a
// second buffer (ping-pong, no extra traffic); every other array is touched only at owned pixels.
// the estimate as the W-update saw it
static __device__ __forceinline__ real w_sees(real v, bool clamped, bool inside) {
  return (clamped && inside && v < (real)0.) ? (real)0. : v;
}

// x / d for a wave-uniform divisor d whose reciprocal r = RN(1 / d) was rounded on the host: one Newton step on
// q0 = RN(x r) with the exact residual (Markstein's sequence), q = RN(q0 + RN(x - d q0) r), is the correctly
// rounded quotient -- what the reference's `eta / mu2` computes -- in 3 VALU operations; the compiler's IEEE
// division expands to ~10 (v_div_scale x2, v_rcp, 4 fma, v_div_fmas, v_div_fixup), which made up 47 % of the
// image-domain kernel's instruction stream (34 divisions per 4 pixels).  No scaling / fix-up: the operands are image
// values and duals far away from the overflow and denormal ranges.
// (The emulator runs the same sequence -- std::fma is exact on the host too -- so the CPU suite checks these three
// operations, not a plain division; -DLPC_EMU_PLAIN_DIV brings `x / d` back for a comparison.)
static __device__ __forceinline__ real div_by(real x, real d, real r) {
#if defined(LPC_SIMT_EMU) && defined(LPC_EMU_PLAIN_DIV)
  (void)r;
  return x / d;
#else
  const real q = x * r;
#ifdef LPC_DOUBLE
  const real e = fma(-d, q, x);
  return fma(e, r, q);
#else
  const real e = fmaf(-d, q, x);
  return fmaf(e, r, q);
#endif
#endif
}

static __device__ __forceinline__ real soft_thresh_dev(real a, real thr) {   // sign(a) max(|a| - thr, 0), admm.py:341-346
  const real m = rmax(rabs(a) - thr, (real)0.);
#if defined(LPC_SIMT_EMU) && defined(LPC_EMU_PLAIN_DIV)
  return a > (real)0. ? m : (a < (real)0. ? -m : (real)0.);
#elif defined(LPC_DOUBLE)
  return copysign(m, a);     // a == 0 gives m == 0: the sign of that zero never reaches a result
#else
  return copysignf(m, a);
#endif
}

template <int TH, int TW, int NT>
__global__ __launch_bounds__(NT) void k_admm_spatial(PlaneGeom g, AdmmScalars p,
                                                      const real* LPC_RESTRICT V,
                                                      const real* LPC_RESTRICT Vold,
                                                      const real* LPC_RESTRICT HV,
                                                      const real* LPC_RESTRICT HVold, real* LPC_RESTRICT xi,
                                                      const real* LPC_RESTRICT eta0,
                                                      const real* LPC_RESTRICT eta1,
                                                      real* LPC_RESTRICT eta0_out,
                                                      real* LPC_RESTRICT eta1_out,
                                                      real* LPC_RESTRICT rho,
                                                      const real* LPC_RESTRICT Y,
                                                      real* LPC_RESTRICT Rsp, real* LPC_RESTRICT Aout,
                                                      unsigned tiles_x) {
  LPC_DYN_SMEM(smem);
  constexpr int VW = TW + 2, VH = TH + 2;
  real* sV = (real*)smem;                 // [VH][VW], local (ly+1, lx+1)
  real* sO = sV + VH * VW;                 // same for V_old
  real* sQ0 = sO + VH * VW;                // [TH+1][TW]
  real* sQ1 = sQ0 + (TH + 1) * TW;         // [TH][TW+1]
  const int tid = LPC_TID(NT);
  // XCD-aware tile order: workgroup b runs on XCD b % 8 (observed dispatch rule, used for speed
  // only).  Give each XCD a contiguous band of tiles so that the halo lines shared by neighbouring
  // tiles are re-read from the SAME L2 instead of from the fabric.
  const unsigned nblk = gridDim.x, b = blockIdx.x;
  const unsigned q = nblk >> 3, r = nblk & 7, xcd = b & 7, idx = b >> 3;
  const unsigned tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  const unsigned ty_ = tile / tiles_x;
  const int r0 = (int)ty_ * TH, c0 = (int)(tile - ty_ * tiles_x) * TW;
  const long pl = blockIdx.y;
  const long poff = pl * g.rplane;
  const real* v = V + poff;
  const real* vo = Vold + poff;

  // ---- stage V, V_old (+halo, circular) ----
  for (int e = tid; e < VH * VW; e += NT) {
    const int ly = e / VW, lx = e - ly * VW;
    int gr = r0 + ly - 1, gc = c0 + lx - 1;
    gr = gr < 0 ? gr + g.Hp : gr; gr = gr >= g.Hp ? gr - g.Hp : gr; gr = gr >= g.Hp ? gr % g.Hp : gr;
    gc = gc < 0 ? gc + g.Wp : gc; gc = gc >= g.Wp ? gc - g.Wp : gc; gc = gc >= g.Wp ? gc % g.Wp : gc;
    const long o = (long)gr * g.rpitch + gc;
    sV[e] = v[o];
    sO[e] = p.first ? (real)0. : vo[o];
  }
  __syncthreads();

  // ---- q0 over [0,TH] x [0,TW), q1 over [0,TH) x [0,TW]; eta' stored for owned pixels ----
  for (int e = tid; e < (TH + 1) * (TW + 1); e += NT) {
    const int ly = e / (TW + 1), lx = e - ly * (TW + 1);
    int gr = r0 + ly, gc = c0 + lx;
    const bool own = (ly < TH) && (lx < TW) && (gr < g.Hp) && (gc < g.Wp);
    gr = gr >= g.Hp ? gr % g.Hp : gr;
    gc = gc >= g.Wp ? gc % g.Wp : gc;
    const long o = poff + (long)gr * g.rpitch + gc;
    const int li = (ly + 1) * VW + (lx + 1);
    const real vc = sV[li], oc = sO[li];
    if (lx < TW) {  // component 0 (row difference)
      real e0 = eta0[o];
      const real psi = sV[li - VW] - vc;
      if (!p.first) {
        const real psio = sO[li - VW] - oc;
        const real uo = soft_thresh_dev(psio + div_by(e0, p.mu2p, p.r_mu2p), p.thrp);
        e0 = e0 + p.mu2p * (psi - uo);
      }
      const real un = soft_thresh_dev(psi + div_by(e0, p.mu2, p.r_mu2), p.thr);
      sQ0[ly * TW + lx] = p.mu2 * un - e0;
      if (own) eta0_out[o] = e0;
    }
    if (ly < TH) {  // component 1 (column difference)
      real e1 = eta1[o];
      const real psi = sV[li - 1] - vc;
      if (!p.first) {
        const real psio = sO[li - 1] - oc;
        const real uo = soft_thresh_dev(psio + div_by(e1, p.mu2p, p.r_mu2p), p.thrp);
        e1 = e1 + p.mu2p * (psi - uo);
      }
      const real un = soft_thresh_dev(psi + div_by(e1, p.mu2, p.r_mu2), p.thr);
      sQ1[ly * (TW + 1) + lx] = p.mu2 * un - e1;
      if (own) eta1_out[o] = e1;
    }
  }
  __syncthreads();

  // ---- owned pixels: xi, rho, X, W, r_sp, a ----
  const int dpl = (int)(pl / g.DC) * g.C + (int)(pl % g.C);
  const real* y = Y + (long)dpl * g.uplane;
  for (int e = tid; e < TH * TW; e += NT) {
    const int ly = e / TW, lx = e - ly * TW;
    const int gr = r0 + ly, gc = c0 + lx;
    if (gr >= g.Hp || gc >= g.Wp) continue;
    const long o = poff + (long)gr * g.rpitch + gc;
    const int li = (ly + 1) * VW + (lx + 1);
    const real vc = sV[li];
    const real hv = HV[o];
    real xiv = xi[o], rhov = rho[o];
    const bool inside = (gr >= g.sh) && (gr < g.sh + g.H) && (gc >= g.sw) && (gc < g.sw + g.W);
    const real yv = inside ? y[(long)(gr - g.sh) * g.W + (gc - g.sw)] : (real)0;
    if (!p.first) {
      // X of the previous iteration, recomputed bit-for-bit from what it was computed from (admm.py:252-254)
      const real xo = (inside ? p.m_in_p : p.m_out_p) * (xiv + p.mu1p * HVold[o] + yv);
      xiv = xiv + p.mu1p * (hv - xo);
      const real wo = rmax(div_by(rhov, p.mu3p, p.r_mu3p) + w_sees(sO[li], p.clamp_old, inside), (real)0);
      rhov = rhov + p.mu3p * (vc - wo);
    }
    const real xn = (inside ? p.m_in : p.m_out) * (xiv + p.mu1 * hv + yv);
    const real wn = rmax(div_by(rhov, p.mu3, p.r_mu3) + w_sees(vc, p.clamp_cur, inside), (real)0);
    const real d1 = sQ0[(ly + 1) * TW + lx] - sQ0[ly * TW + lx];
    const real d2 = sQ1[ly * (TW + 1) + lx + 1] - sQ1[ly * (TW + 1) + lx];
    xi[o] = xiv;
    rho[o] = rhov;
    Rsp[o] = (p.mu3 * wn - rhov) + (d1 + d2);
    Aout[o] = p.mu1 * xn - xiv;
  }
}

// ---- K1, 16-byte-lane version (padded width a multiple of 4) -----------------------------------
// Same arithmetic as k_admm_spatial, re-shaped for HBM: every lane moves four pixels (float4: a wave covers 1 KiB of
// one image row per array; the float64 build moves two 16-byte halves), tiles are TH rows x 256 columns, only V / V_old
// are staged in LDS (+1 halo, circular); q = mu2 U - eta of the lower / right neighbour is RECOMPUTED in registers from
// the LDS tile and one extra (L1/L2-resident) load of eta instead of being exchanged through LDS, so there is
// one barrier and 21 KiB of LDS per workgroup (7 workgroups per CU).

// eta' and q for one pixel and one difference direction
static __device__ __forceinline__ void tv_component(const AdmmScalars& p, real vc, real vn, real oc, real on,
                                                     real eta, real& eta_new, real& q) {
  const real psi = vn - vc;                       // finite_diff: roll(+1) - x   (admm.py:349-359)
  if (!p.first) {
    if (p.half_in) {
      eta = eta + p.mu2p * psi;                    // stored: eta - mu2p U_old (AdmmScalars::half_in)
    } else {
      const real uo = soft_thresh_dev((on - oc) + div_by(eta, p.mu2p, p.r_mu2p), p.thrp);
      eta = eta + p.mu2p * (psi - uo);             // pending eta update of the previous iteration
    }
  }
  const real un = soft_thresh_dev(psi + div_by(eta, p.mu2, p.r_mu2), p.thr);
  q = p.mu2 * un - eta;
  eta_new = p.half_out ? -q : eta;
}

// XHALF == false: the TV / W half only (eta, rho, r_sp); xi and a = mu1 X - xi are then produced by the forward row
// kernel itself (k_rfwd_half_x / k_rfwd_arrays_x), which needs nothing but its own row for them.
// HIN: the duals arrive half-applied (AdmmScalars::half_in): no V_old tile is staged or read.
template <int TH, int NT, bool XHALF = true, bool HIN = false>
__global__ __launch_bounds__(NT) void k_admm_spatial_v4(PlaneGeom g, AdmmScalars p,
                                                         const real* LPC_RESTRICT V,
                                                         const real* LPC_RESTRICT Vold,
                                                         const real* LPC_RESTRICT HV,
                                                         const real* LPC_RESTRICT HVold, real* LPC_RESTRICT xi,
                                                         const real* LPC_RESTRICT eta0,
                                                         const real* LPC_RESTRICT eta1,
                                                         real* LPC_RESTRICT eta0_out,
                                                         real* LPC_RESTRICT eta1_out,
                                                         real* LPC_RESTRICT rho,
                                                         const real* LPC_RESTRICT Y,
                                                         real* LPC_RESTRICT Rsp, real* LPC_RESTRICT Aout,
                                                         unsigned tiles_x) {
  LPC_DYN_SMEM(smem);
  constexpr int TW = 256, LP = TW + 8;          // LDS row: [3] = col -1, [4..259] = cols 0..255, [260] = col 256
  constexpr int VH = TH + 2;
  real* sV = (real*)smem;                     // [VH][LP]
  real* sO = sV + VH * LP;
  const int tid = LPC_TID(NT);
  const unsigned nblk = gridDim.x, bid = p.rev ? gridDim.x - 1u - blockIdx.x : blockIdx.x;   // XCD-aware tile order (see k_admm_spatial)
  const unsigned qd = nblk >> 3, rm = nblk & 7, xcd = bid & 7, idx = bid >> 3;
  const unsigned tile = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + idx;
  const unsigned ty_ = tile / tiles_x;
  const int r0 = (int)ty_ * TH, c0 = (int)(tile - ty_ * tiles_x) * TW;
  const long pl = p.rev ? gridDim.y - 1u - blockIdx.y : blockIdx.y;
  const long poff = pl * g.rplane;
  const real* v = V + poff;
  const real* vo = Vold + poff;
  // circular neighbours: -1 -> n - 1 and n -> 0 are the only wraps a VALID pixel ever needs (its neighbours lie in
  // [-1, n]); indices further out belong to the overhang of the last tile, whose values no valid pixel reads -- they are
  // clamped to a safe address.  (A general `% n` here was 8 integer divisions per lane: a third of the kernel's VALU.)
  auto wrap = [](int x, int n) { x = x < 0 ? x + n : x; x = x >= n ? x - n : x; return x < n ? x : n - 1; };
  auto wrap_r = [&](int r) { return wrap(r, g.Hp); };
  auto wrap_c = [&](int c) { return wrap(c, g.Wp); };
  auto wrap_c4 = [&](int c) { c = c >= g.Wp ? c - g.Wp : c; return c < g.Wp ? c : g.Wp - 4; };   // quads: c, Wp multiples of 4

  // ---- stage V, V_old: body as real4, the two halo columns as scalars ----
  for (int e = tid; e < VH * (TW / 4); e += NT) {
    const int ly = e / (TW / 4), l4 = e - ly * (TW / 4);
    const long o = (long)wrap_r(r0 + ly - 1) * g.rpitch + wrap_c4(c0 + 4 * l4);
    st4(sV + ly * LP + 4 + 4 * l4, ld4(v + o));
    if (!HIN) st4(sO + ly * LP + 4 + 4 * l4, p.first ? make_real4((real)0., (real)0., (real)0., (real)0.) : ld4(vo + o));
  }
  for (int e = tid; e < VH * 2; e += NT) {
    const int ly = e >> 1, side = e & 1;
    const long o = (long)wrap_r(r0 + ly - 1) * g.rpitch + wrap_c(side ? c0 + TW : c0 - 1);
    sV[ly * LP + (side ? 4 + TW : 3)] = v[o];
    if (!HIN) sO[ly * LP + (side ? 4 + TW : 3)] = p.first ? (real)0. : vo[o];
  }
  __syncthreads();

  const int dpl = (int)(pl / g.DC) * g.C + (int)(pl % g.C);
  const real* y = Y + (long)dpl * g.uplane;
  const int lane = tid & 63, wv = tid >> 6;
  const int gc = c0 + 4 * lane;
#pragma unroll
  for (int rr = 0; rr < TH / (NT / 64); ++rr) {
    const int ly = wv + rr * (NT / 64);
    const int gr = r0 + ly;
    if (gr >= g.Hp || gc >= g.Wp) continue;
    const long o = poff + (long)gr * g.rpitch + gc;
    const long o_dn = poff + (long)wrap_r(gr + 1) * g.rpitch + gc;        // eta0 of the row below
    const long o_rt = poff + (long)gr * g.rpitch + wrap_c(gc + 4);        // eta1 of the pixel right of the quad
    // global loads first (all independent)
    const real4 z4 = make_real4((real)0., (real)0., (real)0., (real)0.);
    const bool rsp_in = HIN && p.rho_rsp;      // rho~ recovered from this pixel's r_sp (AdmmScalars::rho_rsp)
    const real4 hv4 = XHALF ? ld4(HV + o) : z4, xi4 = XHALF ? ld4(xi + o) : z4, rho4 = ld4((rsp_in ? Rsp : rho) + o);
    const real4 e04 = ld4(eta0 + o), e14 = ld4(eta1 + o), e0d4 = ld4(eta0 + o_dn);
    const real e1r = eta1[o_rt];
    real4 ho4 = z4;
    if (XHALF && !p.first) ho4 = ld4(HVold + o);      // previous H V: lets the previous X be recomputed instead of stored
    // LDS neighbourhood: rows ly-1, ly, ly+1 of the quad, plus the pixel left and right of it
    const real* rowm = sV + ly * LP + 4 + 4 * lane;        // global row gr-1  (local ly)
    const real* rowc = rowm + LP;                          // gr
    const real* rowp = rowc + LP;                          // gr+1
    const real* orm = sO + ly * LP + 4 + 4 * lane;
    const real* orc = orm + LP;
    const real* orp = orc + LP;
    const real4 vm4 = ld4(rowm), vc4 = ld4(rowc), vp4 = ld4(rowp);
    const real4 zo4 = make_real4((real)0., (real)0., (real)0., (real)0.);
    const real4 om4 = HIN ? zo4 : ld4(orm), oc4 = HIN ? zo4 : ld4(orc), op4 = HIN ? zo4 : ld4(orp);
    const real vl = rowc[-1], vr = rowc[4], ol = HIN ? (real)0. : orc[-1], orr = HIN ? (real)0. : orc[4];
    const real vcs[6] = {vl, vc4.x, vc4.y, vc4.z, vc4.w, vr};       // cols gc-1 .. gc+4 of row gr
    const real ocs[6] = {ol, oc4.x, oc4.y, oc4.z, oc4.w, orr};
    const real vms[4] = {vm4.x, vm4.y, vm4.z, vm4.w}, vps[4] = {vp4.x, vp4.y, vp4.z, vp4.w};
    const real oms[4] = {om4.x, om4.y, om4.z, om4.w}, ops[4] = {op4.x, op4.y, op4.z, op4.w};
    const real hvs[4] = {hv4.x, hv4.y, hv4.z, hv4.w}, xis[4] = {xi4.x, xi4.y, xi4.z, xi4.w};
    const real rhs[4] = {rho4.x, rho4.y, rho4.z, rho4.w}, hos[4] = {ho4.x, ho4.y, ho4.z, ho4.w};
    const real e0s[4] = {e04.x, e04.y, e04.z, e04.w}, e0ds[4] = {e0d4.x, e0d4.y, e0d4.z, e0d4.w};
    const real e1s[5] = {e14.x, e14.y, e14.z, e14.w, e1r};
    real q1[5], e1n[5];
#pragma unroll
    for (int i = 0; i < 5; ++i)   // column-difference component at cols gc .. gc+4 (the 5th only for q)
      tv_component(p, vcs[i + 1], vcs[i], ocs[i + 1], ocs[i], e1s[i], e1n[i], q1[i]);
    real xin[4], e0n[4], rhn[4], rs[4], as[4];
    const bool row_in = (gr >= g.sh) && (gr < g.sh + g.H);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      real q0c, q0d, dummy;
      tv_component(p, vcs[i + 1], vms[i], ocs[i + 1], oms[i], e0s[i], e0n[i], q0c);   // this pixel
      tv_component(p, vps[i], vcs[i + 1], ops[i], ocs[i + 1], e0ds[i], dummy, q0d);   // the pixel below
      const real vc = vcs[i + 1], hv = hvs[i];
      real xiv = xis[i], rhov = rhs[i];
      const int cc = gc + i;
      const bool inside = row_in && (cc >= g.sw) && (cc < g.sw + g.W);
      const real yv = (XHALF && inside) ? y[(long)(gr - g.sh) * g.W + (cc - g.sw)] : (real)0.;
      if (!p.first) {
        if (XHALF) {
          const real xo = (inside ? p.m_in_p : p.m_out_p) * (xiv + p.mu1p * hos[i] + yv);   // previous X
          xiv = xiv + p.mu1p * (hv - xo);
        }
        if (HIN || p.half_in) {
          // rhov holds r_sp_old: rho~ = (d1 + d2)_old - r_sp_old with q_old = -eta~ (AdmmScalars::rho_rsp)
          if (rsp_in) rhov = ((e0s[i] - e0ds[i]) + (e1s[i] - e1s[i + 1])) - rhov;
          rhov = rhov + p.mu3p * vc;                // stored: rho - mu3p W_old (AdmmScalars::half_in)
        } else {
          const real wo = rmax(div_by(rhov, p.mu3p, p.r_mu3p) + w_sees(ocs[i + 1], p.clamp_old, inside), (real)0.);
          rhov = rhov + p.mu3p * (vc - wo);
        }
      }
      const real xnew = (inside ? p.m_in : p.m_out) * (xiv + p.mu1 * hv + yv);
      const real wn = rmax(div_by(rhov, p.mu3, p.r_mu3) + w_sees(vc, p.clamp_cur, inside), (real)0.);
      const real d1 = q0d - q0c;
      const real d2 = q1[i + 1] - q1[i];
      xin[i] = xiv; rhn[i] = p.half_out ? rhov - p.mu3 * wn : rhov;
      rs[i] = (p.mu3 * wn - rhov) + (d1 + d2);
      as[i] = p.mu1 * xnew - xiv;
    }
    if (XHALF) st4(xi + o, make_real4(xin[0], xin[1], xin[2], xin[3]));
    if (!(rsp_in && p.half_out)) st4(rho + o, make_real4(rhn[0], rhn[1], rhn[2], rhn[3]));   // (the next iteration reads r_sp instead)
    st4(eta0_out + o, make_real4(e0n[0], e0n[1], e0n[2], e0n[3]));
    st4(eta1_out + o, make_real4(e1n[0], e1n[1], e1n[2], e1n[3]));
    st4(Rsp + o, make_real4(rs[0], rs[1], rs[2], rs[3]));
    if (XHALF) st4(Aout + o, make_real4(as[0], as[1], as[2], as[3]));
  }
}

// ---- the X half of the image-domain work on four adjacent pixels of one row (k_rfwd_half_x, k_rfwd_arrays_x) ---------
// Loads first (xhalf_load: up to four 16-byte loads, all independent -- callers issue the loads of every quad they own
// before the arithmetic of the first), then the statements of the X part of k_admm_spatial_v4 (xhalf_apply).
struct XQuad { real4 hv, xi, ho; real ys[4]; bool ins[4]; bool skip; };
// row_in: the row lies inside the sensor window; y: that row of the measurement (dereferenced only when row_in);
// y4: window offset and width allow 16-byte loads of y
static __device__ __forceinline__ XQuad xhalf_load(const PlaneGeom& g, const AdmmScalars& p, const real* LPC_RESTRICT HV,
                                                   const real* LPC_RESTRICT HVold, const real* xi,
                                                   const real* LPC_RESTRICT y, long o_row, bool row_in, bool y4, int q) {
  XQuad c;
  const int gc = 4 * q;
  // the whole quad lies outside the sensor window: HV is all it needs (see AdmmScalars::xiw)
  c.skip = p.xiw && !(row_in && gc + 4 > g.sw && gc < g.sw + g.W);
  c.hv = ld4(HV + o_row + gc);
  c.xi = c.ho = make_real4((real)0., (real)0., (real)0., (real)0.);
  if (!c.skip) c.xi = ld4(xi + o_row + gc);
  // H V_old: to recompute the previous X inside the window -- not with xi half-applied (AdmmScalars::xi_in) -- and for
  // xi = mu1p (HV - HV_old) outside it when that is stored (xi_store: the last iteration of a call; that launch loads it
  // for every quad, those wholly inside the window included, where nothing reads it -- deliberate: one launch per call, the
  // parent form's traffic, no test per quad in the other ninety-nine)
  if (!p.first && (p.xi_in ? (p.xiw && p.xi_store) : (!c.skip || p.xi_store))) c.ho = ld4(HVold + o_row + gc);
#pragma unroll
  for (int i = 0; i < 4; ++i) { c.ys[i] = (real)0.; c.ins[i] = false; }
  if (row_in) {
    if (y4) {
      if (gc >= g.sw && gc < g.sw + g.W) {
        const real4 yv = ld4(y + (gc - g.sw));
        c.ys[0] = yv.x; c.ys[1] = yv.y; c.ys[2] = yv.z; c.ys[3] = yv.w;
        c.ins[0] = c.ins[1] = c.ins[2] = c.ins[3] = true;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cc = gc + i;
        c.ins[i] = (cc >= g.sw) && (cc < g.sw + g.W);
        if (c.ins[i]) c.ys[i] = y[cc - g.sw];
      }
    }
  }
  return c;
}
// xin: the updated xi -- half-applied, -a, with p.xi_out -- (stored by the caller unless c.skip && !p.xi_store);
// as: a = mu1 X - xi'
// One pixel (the per-element body of the quad form below and of the pair form of lpc_admm_v2_kernels.h): hv, ho = H V,
// H V_old; xiv: the stored xi; yv: the measurement (0 outside the window); in: the pixel lies inside the sensor window.
// Both results are assigned exactly once, at the end (profiles/dual_elision_notes.md: written any other way the callers'
// arrays go to scratch).
struct XElem { real xi, a; };
static __device__ __forceinline__ XElem xhalf_elem(const AdmmScalars& p, real hv, real xiv, real ho, real yv, bool in) {
  real a;
  // outside the window: a = mu1 HV, xi = mu1p (HV - HV_old) -- stored on request only (xi_store).  In a quad that
  // straddles the window's edge these lanes are stored with the quad in every iteration, and with xi_in H V_old is not
  // loaded (ho = 0): between the iterations of a call they hold GARBAGE.  Nothing reads them (this branch never reads
  // xi) until the last iteration, which loads H V_old and rewrites them.
  if (p.xiw && !in) {
    xiv = p.first ? (real)0. : p.mu1p * (hv - ho);
    a = p.mu1 * hv;
  } else {
    if (!p.first) {
      if (p.xi_in) {
        xiv = xiv + p.mu1p * hv;                   // stored: xi' - mu1p X_old (AdmmScalars::xi_in)
      } else {
        const real xo = (in ? p.m_in_p : p.m_out_p) * (xiv + p.mu1p * ho + yv);   // previous X
        xiv = xiv + p.mu1p * (hv - xo);
      }
    }
    const real xnew = (in ? p.m_in : p.m_out) * (xiv + p.mu1 * hv + yv);
    a = p.mu1 * xnew - xiv;
    if (p.xi_out) xiv = -a;
  }
  XElem r;
  r.xi = xiv;
  r.a = a;
  return r;
}
static __device__ __forceinline__ void xhalf_apply(const AdmmScalars& p, const XQuad& c, real xin[4], real as[4]) {
  const real hvs[4] = {c.hv.x, c.hv.y, c.hv.z, c.hv.w}, xis[4] = {c.xi.x, c.xi.y, c.xi.z, c.xi.w};
  const real hos[4] = {c.ho.x, c.ho.y, c.ho.z, c.ho.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const XElem r = xhalf_elem(p, hvs[i], xis[i], hos[i], c.ys[i], c.ins[i]);
    xin[i] = r.xi;
    as[i] = r.a;
  }
}
// the same on the two pixels of one pair (no H V_old: the steady state of a call, xi_in without xi_store): xa = (xi, xi),
// as = (a, a) of columns 2 i, 2 i + 1, which lie both inside or both outside the window (pair geometry).
// ho: the zero that stands for the H V_old the quad form did not load, as a value the compiler cannot see through
// (lpc_opaque_f) -- with a literal 0 it merges mu1p (hv - 0) of the branch outside the window with the mu1p hv inside
// xi + mu1p hv of the other branch into one product with two uses, which then is no longer contracted into an FMA: the
// quad form's xi' and this one's differed by a rounding (profiles/admm_rows_v2_notes.md)
static __device__ __forceinline__ void xhalf_apply2(const AdmmScalars& p, real2 hv, real2 xi, real2 y, bool in, real ho,
                                                    real2& xin, real2& as) {
  const XElem r0 = xhalf_elem(p, hv.x, xi.x, ho, y.x, in), r1 = xhalf_elem(p, hv.y, xi.y, ho, y.y, in);
  xin = make_real2(r0.xi, r1.xi);
  as = make_real2(r0.a, r1.a);
}

// ---- the TV / W half of the image-domain work on the quads of TWO adjacent rows (k_rfwd_arrays_x<.., K1 = true>) ----
// Small frames are a chain of dependent launches, each a chain of memory latencies (profiles/r05_notes.md section 5):
// here the forward row block of r_sp rows (r0, r0 + 1) forms them itself -- the statements of k_admm_spatial_v4<..,
// XHALF = false>, quad by quad, with the stencil's neighbours read straight from global memory (L2-resident at these
// sizes) instead of a staged tile -- so that an iteration is three launches instead of four and r_sp never exists in
// memory.  v, vo, eta*, rho: plane bases; q: the lane's quad (columns 4 q .. 4 q + 3); second: row r0 + 1 exists; the
// rows go into the tile s as z = r_sp[r0] + i r_sp[r0 + 1].  Rows wrap circularly like the tiled kernel's; eta is read at
// rows owned by other blocks, hence eta*_out (ping-pong).
template <int SK>
static __device__ __forceinline__ void k1_two_rows(const PlaneGeom& g, const AdmmScalars& p, const real* LPC_RESTRICT v,
                                                   const real* LPC_RESTRICT vo, const real* LPC_RESTRICT eta0,
                                                   const real* LPC_RESTRICT eta1, real* LPC_RESTRICT eta0_out,
                                                   real* LPC_RESTRICT eta1_out, real* rho, int r0, bool second, int q,
                                                   real2* s) {
  constexpr unsigned eb = (unsigned)sizeof(real);
  const int gc = 4 * q;
  // 32-bit byte offsets from the plane bases (a plane is < 4 GB); circular column / row neighbours (a row that does not
  // exist is never used: `second`)
  const unsigned bq = (unsigned)gc * eb;
  const unsigned bl = (unsigned)(gc == 0 ? g.Wp - 1 : gc - 1) * eb, br = (unsigned)(gc + 4 >= g.Wp ? 0 : gc + 4) * eb;
  const unsigned rp = (unsigned)g.rpitch * eb;
  unsigned ro[4];
  ro[0] = (unsigned)(r0 == 0 ? g.Hp - 1 : r0 - 1) * rp;
  ro[1] = (unsigned)r0 * rp;
  ro[2] = (unsigned)(r0 + 1 >= g.Hp ? r0 + 1 - g.Hp : r0 + 1) * rp;
  ro[3] = (unsigned)(r0 + 2 >= g.Hp ? r0 + 2 - g.Hp : r0 + 2) * rp;
  auto L4 = [](const real* b, unsigned off) { return *(const real4*)((const char*)b + off); };
  auto L1 = [](const real* b, unsigned off) { return *(const real*)((const char*)b + off); };
  auto S4 = [](real* b, unsigned off, real4 x) { *(real4*)((char*)b + off) = x; };
  const bool need_old = !p.first && !p.half_in;
  // every load of both rows first -- except V_old's, which only a call's first iteration without a reset (or k1_half=0)
  // reads: those are requested row by row below (their registers would otherwise cost every launch a workgroup per CU)
  real4 v4[4], e04[3], e14[2], rh4[2];
  real vl[2], vr[2], e1r[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) v4[k] = L4(v, ro[k] + bq);
#pragma unroll
  for (int k = 0; k < 2; ++k) { vl[k] = L1(v, ro[1 + k] + bl); vr[k] = L1(v, ro[1 + k] + br); }
#pragma unroll
  for (int k = 0; k < 3; ++k) e04[k] = L4(eta0, ro[1 + k] + bq);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    e14[k] = L4(eta1, ro[1 + k] + bq);
    e1r[k] = L1(eta1, ro[1 + k] + br);
    rh4[k] = L4(rho, ro[1 + k] + bq);
  }
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    if (row == 1 && !second) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s[lds_slot<SK>(gc + i)].y = (real)0.;
      break;
    }
    const int gr = r0 + row;
    const real4 z4 = make_real4((real)0., (real)0., (real)0., (real)0.);
    real4 om4 = z4, oc4 = z4, op4 = z4;
    real ol = (real)0., orr = (real)0.;
    if (need_old) {
      om4 = L4(vo, ro[row] + bq); oc4 = L4(vo, ro[row + 1] + bq); op4 = L4(vo, ro[row + 2] + bq);
      ol = L1(vo, ro[row + 1] + bl); orr = L1(vo, ro[row + 1] + br);
    }
    const real4 vm4 = v4[row], vc4 = v4[row + 1], vp4 = v4[row + 2];
    const real vcs[6] = {vl[row], vc4.x, vc4.y, vc4.z, vc4.w, vr[row]};       // cols gc-1 .. gc+4 of row gr
    const real ocs[6] = {ol, oc4.x, oc4.y, oc4.z, oc4.w, orr};
    const real vms[4] = {vm4.x, vm4.y, vm4.z, vm4.w}, vps[4] = {vp4.x, vp4.y, vp4.z, vp4.w};
    const real oms[4] = {om4.x, om4.y, om4.z, om4.w}, ops[4] = {op4.x, op4.y, op4.z, op4.w};
    const real4 rho4 = rh4[row], e0c4 = e04[row], e0d4 = e04[row + 1], e1c4 = e14[row];
    const real rhs[4] = {rho4.x, rho4.y, rho4.z, rho4.w};
    const real e0s[4] = {e0c4.x, e0c4.y, e0c4.z, e0c4.w}, e0ds[4] = {e0d4.x, e0d4.y, e0d4.z, e0d4.w};
    const real e1s[5] = {e1c4.x, e1c4.y, e1c4.z, e1c4.w, e1r[row]};
    real q1[5], e1n[5];
#pragma unroll
    for (int i = 0; i < 5; ++i)   // column-difference component at cols gc .. gc+4 (the 5th only for q)
      tv_component(p, vcs[i + 1], vcs[i], ocs[i + 1], ocs[i], e1s[i], e1n[i], q1[i]);
    real e0n[4], rhn[4];
    const bool row_in = (gr >= g.sh) && (gr < g.sh + g.H);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      real q0c, q0d, dummy;
      tv_component(p, vcs[i + 1], vms[i], ocs[i + 1], oms[i], e0s[i], e0n[i], q0c);   // this pixel
      tv_component(p, vps[i], vcs[i + 1], ops[i], ocs[i + 1], e0ds[i], dummy, q0d);   // the pixel below
      const real vc = vcs[i + 1];
      real rhov = rhs[i];
      const int cc = gc + i;
      const bool inside = row_in && (cc >= g.sw) && (cc < g.sw + g.W);
      if (!p.first) {
        if (p.half_in) {
          rhov = rhov + p.mu3p * vc;                // stored: rho - mu3p W_old (AdmmScalars::half_in)
        } else {
          const real wo = rmax(div_by(rhov, p.mu3p, p.r_mu3p) + w_sees(ocs[i + 1], p.clamp_old, inside), (real)0.);
          rhov = rhov + p.mu3p * (vc - wo);
        }
      }
      const real wn = rmax(div_by(rhov, p.mu3, p.r_mu3) + w_sees(vc, p.clamp_cur, inside), (real)0.);
      const real d1 = q0d - q0c;
      const real d2 = q1[i + 1] - q1[i];
      rhn[i] = p.half_out ? rhov - p.mu3 * wn : rhov;
      const real rs = (p.mu3 * wn - rhov) + (d1 + d2);
      // z = r_sp[r0] + i r_sp[r0 + 1]: the tile entry's real / imaginary part
      if (row == 0) s[lds_slot<SK>(gc + i)].x = rs;
      else s[lds_slot<SK>(gc + i)].y = rs;
    }
    const unsigned o = ro[1 + row] + bq;
    S4(rho, o, make_real4(rhn[0], rhn[1], rhn[2], rhn[3]));
    S4(eta0_out, o, make_real4(e0n[0], e0n[1], e0n[2], e0n[3]));
    S4(eta1_out, o, make_real4(e1n[0], e1n[1], e1n[2], e1n[3]));
  }
}

// ---- plug-and-play ADMM: the U-prox is an external denoiser (admm.py:126-133,235-243,266-275,300-311) ----------
// Explicit state (U and eta are image-shaped, Psi^T is the identity), plain streaming kernels around the caller's
// function; the reference's branch is reproduced as written, including what its conditional expression drops:
//   use_dual:  r_k = (mu3 W - rho) + mu2 U - eta                 (no data term)
//   else:      r_k = mu2 U + H^T (mu1 X - xi)                    (no W term)
template <int NT>
__global__ __launch_bounds__(NT) void k_pnp_input(real* LPC_RESTRICT out, const real* LPC_RESTRICT U,
                                                   const real* LPC_RESTRICT eta, real mu2, long n) {
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) out[e] = U[e] + eta[e] / mu2;
}

// X, W of this iteration (kept for the dual updates) and the two inputs of the spectral step
template <int NT>
__global__ __launch_bounds__(NT) void k_pnp_pre(PlaneGeom g, AdmmScalars p, int dual, const real* LPC_RESTRICT V,
                                                 const real* LPC_RESTRICT HV, const real* LPC_RESTRICT xi,
                                                 const real* LPC_RESTRICT rho, const real* LPC_RESTRICT U,
                                                 const real* LPC_RESTRICT eta, const real* LPC_RESTRICT Y,
                                                 real* LPC_RESTRICT X, real* LPC_RESTRICT W, real* LPC_RESTRICT Rsp,
                                                 real* LPC_RESTRICT Aout) {
  const long n = (long)g.Hp * g.Wp;
  const long pl = blockIdx.y;
  const int dpl = (int)(pl / g.DC) * g.C + (int)(pl % g.C);
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int r = (int)(e / g.Wp), c = (int)(e - (long)r * g.Wp);
    const long o = pl * g.rplane + (long)r * g.rpitch + c;
    const bool inside = (r >= g.sh) && (r < g.sh + g.H) && (c >= g.sw) && (c < g.sw + g.W);
    const real yv = inside ? Y[(long)dpl * g.uplane + (long)(r - g.sh) * g.W + (c - g.sw)] : (real)0.;
    const real x = (inside ? p.m_in : p.m_out) * (xi[o] + p.mu1 * HV[o] + yv);   // admm.py:252-254
    const real w = rmax(div_by(rho[o], p.mu3, p.r_mu3) + V[o], (real)0.);                        // admm.py:256-262
    X[o] = x;
    W[o] = w;
    if (dual == 2) {   // caller-supplied prior (admm.py:104-120, 277-281): U holds Psi^T(mu2 U - eta), computed by the caller
      Rsp[o] = (p.mu3 * w - rho[o]) + U[o];
      Aout[o] = p.mu1 * x - xi[o];
    } else if (dual) {
      Rsp[o] = (p.mu3 * w - rho[o]) + p.mu2 * U[o] - eta[o];
      Aout[o] = (real)0.;
    } else {
      Rsp[o] = p.mu2 * U[o];
      Aout[o] = p.mu1 * x - xi[o];
    }
  }
}

// dual updates with the new image estimate (admm.py:296-311)
template <int NT>
__global__ __launch_bounds__(NT) void k_pnp_post(PlaneGeom g, AdmmScalars p, int dual, const real* LPC_RESTRICT Vn,
                                                  const real* LPC_RESTRICT HVn, const real* LPC_RESTRICT X,
                                                  const real* LPC_RESTRICT W, const real* LPC_RESTRICT U,
                                                  real* LPC_RESTRICT xi, real* LPC_RESTRICT eta,
                                                  real* LPC_RESTRICT rho) {
  const long n = (long)g.Hp * g.Wp;
  const long pl = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int r = (int)(e / g.Wp), c = (int)(e - (long)r * g.Wp);
    const long o = pl * g.rplane + (long)r * g.rpitch + c;
    xi[o] = xi[o] + p.mu1 * (HVn[o] - X[o]);
    if (dual) eta[o] = eta[o] + p.mu2 * (Vn[o] - U[o]);
    rho[o] = rho[o] + p.mu3 * (Vn[o] - W[o]);
  }
}

// materialise U, W and the flushed duals for inspection (tests / get_state); no state change
template <int NT>
__global__ __launch_bounds__(NT) void k_admm_flush(PlaneGeom g, AdmmScalars p,
                                                    const real* LPC_RESTRICT V,
                                                    const real* LPC_RESTRICT Vold,
                                                    const real* LPC_RESTRICT HV,
                                                    const real* LPC_RESTRICT HVold,
                                                    const real* LPC_RESTRICT Y,
                                                    const real* LPC_RESTRICT xi,
                                                    const real* LPC_RESTRICT eta0,
                                                    const real* LPC_RESTRICT eta1,
                                                    const real* LPC_RESTRICT rho, real* LPC_RESTRICT out0,
                                                    real* LPC_RESTRICT out1, int which0, int which1) {
  // quantities: 0 xi', 1 eta0', 2 eta1', 3 rho', 4 U0, 5 U1, 6 W, 7 X; out0 receives `which0`, out1 (if not null)
  // `which1` -- the caller asks for what it reads out, the scratch is two padded arrays the loop leaves idle
  const long n = (long)g.Hp * g.Wp;
  const long pl = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int r = (int)(e / g.Wp), c = (int)(e - (long)r * g.Wp);
    const long o = pl * g.rplane + (long)r * g.rpitch + c;
    const long ou = pl * g.rplane + (long)wrap_add(r, -1, g.Hp) * g.rpitch + c;
    const long ol = pl * g.rplane + (long)r * g.rpitch + wrap_add(c, -1, g.Wp);
    real xiv = xi[o], e0 = eta0[o], e1 = eta1[o], rh = rho[o];
    real u0 = (real)0., u1 = (real)0., w = (real)0., x = (real)0.;
    if (!p.first) {
      const bool inside = (r >= g.sh) && (r < g.sh + g.H) && (c >= g.sw) && (c < g.sw + g.W);
      const int dpl = (int)(pl / g.DC) * g.C + (int)(pl % g.C);
      const real yv = inside ? Y[(long)dpl * g.uplane + (long)(r - g.sh) * g.W + (c - g.sw)] : (real)0.;
      x = (inside ? p.m_in_p : p.m_out_p) * (xiv + p.mu1p * HVold[o] + yv);   // X of the last iteration
      const real oc = Vold[o], vc = V[o];
      u0 = soft_thresh_dev((Vold[ou] - oc) + div_by(e0, p.mu2p, p.r_mu2p), p.thrp);
      u1 = soft_thresh_dev((Vold[ol] - oc) + div_by(e1, p.mu2p, p.r_mu2p), p.thrp);
      w = rmax(div_by(rh, p.mu3p, p.r_mu3p) + w_sees(oc, p.clamp_old, inside), (real)0.);
      xiv = xiv + p.mu1p * (HV[o] - x);
      e0 = e0 + p.mu2p * ((V[ou] - vc) - u0);
      e1 = e1 + p.mu2p * ((V[ol] - vc) - u1);
      rh = rh + p.mu3p * (vc - w);
    }
    const real val[8] = {xiv, e0, e1, rh, u0, u1, w, x};
    out0[o] = val[which0];
    if (out1) out1[o] = val[which1];
  }
}
