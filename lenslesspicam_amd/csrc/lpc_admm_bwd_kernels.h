// lpc_admm_bwd_kernels.h -- reverse mode of the unrolled ADMM iterations (lpc_admm_backward): the image-domain kernels.
//
// Iteration i (unrolled_admm.py:181-234) with m1, m2, m3, tau, th = tau / m2, incoming state v, hv = H v, xi, eta, rho:
//   s = Psi v + eta / m2;  U = soft(s, th);  X = (xi + m1 hv + b) / (M + m1);  q = rho / m3 + v;  W = max(q, 0)
//   v' = S(m3 W - rho + PsiT(m2 U - eta) + HT(m1 X - xi));  hv' = H v'
//   xi' = xi + m1 (hv' - X);  eta' = eta + m2 (Psi v' - U);  rho' = rho + m3 (v' - W)
// S = irfft2 . R_i . rfft2 is self-adjoint and H, HT are each other's adjoints for even padded lengths, so the reverse
// iteration needs ONE spectral step of the forward's own shape, (r_sp, a) -> (rb = S(r_sp + HT a), hr = H rb):
//   r_sp = vb + m3 rhob + PsiT(pb + m2 etab);   a = hb + m1 xib                         [pre-spectral half]
//   g1 = <xib - hr, hv' - X>;  g2 = <etab - Psi rb, Psi v' - U>;  g3 = <rhob - rb, v' - W>     [post-spectral half]
//   Xb = m1 (hr - xib);  Ub = m2 (Psi rb - etab);  Wb = m3 (rb - rhob);   xib -= hr;  etab -= Psi rb;  rhob -= rb
//   qb = Wb [q > 0];  rhob += qb / m3;  g3 -= <qb, rho> / m3^2
//   xb = Xb / (M + m1);  xib += xb;  g_b += xb;  g1 += <xb, hv - X>
//   sb = Ub [|s| > th];  thb = -<sb, sign s>;  etab += sb / m2;  g2 += -<sb, eta> / m2^2 - thb tau / m2^2;  g_tau = thb / m2
//   vb <- qb;  hb <- m1 xb;  pb <- sb
// (vb, hb, pb: the adjoints of v, H v, Psi v; the dR/dm terms of the spectral step are the <.., hr>, <.., Psi rb>, <.., rb>
// parts of g1, g2, g3 by Parseval: no reduction over a spectrum.)
//
// The tape holds the iterates V_0 .. V_n only; k_admm_bwd_replay steps the explicit recurrences above from V_i, H V_i,
// V_{i+1}, H V_{i+1} and writes xi, eta, rho of every iteration next to them, whatever form the launch plan kept them in.
// U, X, W, s, q are never stored: k_admm_bwd_step recomputes them.
//
// k_admm_bwd_step is everything between two spectral steps: the post-spectral half of iteration i and the pre-spectral
// half of iteration i - 1 in one launch (the structure of the forward's k_admm_spatial_v4).  Tiles of TH rows x 4 QW
// columns, one quad (16 bytes in float32) per lane; V_i, V_{i+1} and rb are staged in LDS with a one-pixel circular halo,
// z = pb + m2' etab of the lower / right neighbour is recomputed from that tile and one extra (cache-resident) load of
// eta and etab, so there is one barrier in front of the arithmetic.  etab is read at pixels owned by neighbouring
// workgroups: its update goes to a second buffer (ping-pong).  No division per element: the reciprocals arrive in
// AdmmBwdScalars.  The four sums leave every workgroup as double partial sums; k_admm_bwd_finish adds them in a fixed
// order.  No atomics.
#pragma once
#include "lpc_admm_kernels.h"

struct AdmmBwdScalars {
  real m1, m2, m3, thr;      // iteration i
  real m_in, m_out;          // 1 / (1 + m1), 1 / m1
  real r_m2, r_m3;           // 1 / m2, 1 / m3
  real n1, n2, n3;           // m1, m2, m3 of iteration i - 1 (pre-spectral half)
  int pre;                   // 0: i == 0, there is no earlier iteration: r_sp and a are not written
  int gb_first;              // i == n - 1: g_b is written, not added to
};

struct AdmmBwd {
  const real *V, *V2, *HV, *HV2;       // V_i, V_{i+1}, H V_i, H V_{i+1}          (padded planes)
  const real *xi, *eta0, *eta1, *rho;  // the state iteration i started from
  const real* Y;                       // measurement, un-padded planes
  const real *rb, *hr;                 // what the spectral step of iteration i returned
  real *xib, *rhob;                    // carried adjoints, updated in place
  const real *eb0, *eb1;               // etab in
  real *eb0o, *eb1o;                   // etab out
  real* gb;                            // [P][H][W] sum of xb over the iterations, or null
  real *Rsp, *Aarr;                    // inputs of the next spectral step
  double* part;                        // [P][gridDim.x][4]: g1, g2 without the thb term, g3, thb
};

// ---- a quad of one padded row, columns gc .. gc + 3 circular in Wp (rows have rpitch = 4 k reals: aligned) -------------
static __device__ __forceinline__ real4 admm_bwd_ldq(const real* LPC_RESTRICT row, int gc, int Wp) {
  if (gc + 3 < Wp) return ld4(row + gc);
  real4 r;
  r.x = row[gc % Wp]; r.y = row[(gc + 1) % Wp]; r.z = row[(gc + 2) % Wp]; r.w = row[(gc + 3) % Wp];
  return r;
}
static __device__ __forceinline__ void admm_bwd_stq(real* LPC_RESTRICT row, int gc, int Wp, const real v[4]) {
  if (gc + 3 < Wp) { st4(row + gc, make_real4(v[0], v[1], v[2], v[3])); return; }
  for (int k = 0; k < 4; ++k)
    if (gc + k < Wp) row[gc + k] = v[k];
}
static __device__ __forceinline__ void admm_bwd_unpack(real4 q, real v[4]) { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }

// one pixel, one difference direction: (vc, vn) = V_i here / at the upper or left neighbour, (wc, wn) = V_{i+1}, (rc, rn) = rb
static __device__ __forceinline__ void admm_bwd_tv(const AdmmBwdScalars& p, real vc, real vn, real wc, real wn, real rc,
                                                   real rn, real eta, real etab, bool own, real& etab_new, real& z,
                                                   double& g2, double& gth) {
  const real s = (vn - vc) + eta * p.r_m2;
  const real a = rabs(s) - p.thr;
  const bool act = a > (real)0.;
  const real em = etab - (rn - rc);                     // etab - Psi rb
  const real sb = act ? -p.m2 * em : (real)0.;          // Ub [|s| > th]
  etab_new = em + sb * p.r_m2;
  z = sb + p.n2 * etab_new;
  if (own) {
    const real u = act ? (s > (real)0. ? a : -a) : (real)0.;
    g2 += (double)em * (double)((wn - wc) - u) - (double)sb * (double)eta * ((double)p.r_m2 * (double)p.r_m2);
    gth -= s > (real)0. ? (double)sb : -(double)sb;     // (sb != 0 only where s != 0)
  }
}

template <int NT>
static __host__ __device__ constexpr size_t admm_bwd_red_bytes() {
#if !defined(LPC_SIMT_EMU)
  return (size_t)(NT / 64 > 0 ? NT / 64 : 1) * 4 * sizeof(double);
#else
  return (size_t)NT * 4 * sizeof(double);
#endif
}
// the four sums of a workgroup, valid in thread 0 (the fixed order of gd_bwd_block_sum2)
template <int NT>
static __device__ __forceinline__ void admm_bwd_block_sum4(double s[4], double* red, int tid) {
#if !defined(LPC_SIMT_EMU)
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 4; ++k) s[k] += __shfl_down(s[k], off, 64);
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0)
    for (int k = 0; k < 4; ++k) red[4 * wave + k] = s[k];
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < NT / 64; ++w)
      for (int k = 0; k < 4; ++k) s[k] += red[4 * w + k];
#else
  for (int k = 0; k < 4; ++k) red[4 * tid + k] = s[k];
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < NT; ++w)
      for (int k = 0; k < 4; ++k) s[k] += red[4 * w + k];
#endif
}

template <int TH, int QW>
static __host__ __device__ constexpr size_t admm_bwd_step_smem() {
  return admm_bwd_red_bytes<TH * QW>() + (size_t)3 * (TH + 2) * (4 * QW + 2) * sizeof(real);
}

template <int TH, int QW>
__global__ __launch_bounds__(TH * QW) void k_admm_bwd_step(PlaneGeom g, AdmmBwdScalars p, AdmmBwd a, unsigned tiles_x) {
  constexpr int NT = TH * QW, TW = 4 * QW, LW = TW + 2, LH = TH + 2;
  LPC_DYN_SMEM(smem);
  double* red = (double*)smem;
  real* sV = (real*)(smem + admm_bwd_red_bytes<NT>());     // [LH][LW], pixel (ly, lx) of the tile at (ly + 1) * LW + lx + 1
  real* sW = sV + LH * LW;
  real* sR = sW + LH * LW;
  const int tid = LPC_TID(NT);
  const unsigned ty_ = blockIdx.x / tiles_x;
  const int r0 = (int)ty_ * TH, c0 = (int)(blockIdx.x - ty_ * tiles_x) * TW;
  const long pl = blockIdx.y, poff = pl * g.rplane;
  const real *V = a.V + poff, *V2 = a.V2 + poff, *RB = a.rb + poff;

  // ---- stage V_i, V_{i+1}, rb with a one-pixel halo, circular in (Hp, Wp) ----
  for (int e = tid; e < LH * QW; e += NT) {
    const int ly = e / QW, qx = e - ly * QW;
    const int gr = (r0 + ly - 1 + g.Hp) % g.Hp, gc = c0 + 4 * qx;
    const long ro = (long)gr * g.rpitch;
    real v[4], w[4], r[4];
    admm_bwd_unpack(admm_bwd_ldq(V + ro, gc, g.Wp), v);
    admm_bwd_unpack(admm_bwd_ldq(V2 + ro, gc, g.Wp), w);
    admm_bwd_unpack(admm_bwd_ldq(RB + ro, gc, g.Wp), r);
    const int li = ly * LW + 4 * qx + 1;
    for (int k = 0; k < 4; ++k) { sV[li + k] = v[k]; sW[li + k] = w[k]; sR[li + k] = r[k]; }
  }
  for (int e = tid; e < LH * 2; e += NT) {
    const int ly = e >> 1, right = e & 1;
    const int gr = (r0 + ly - 1 + g.Hp) % g.Hp, gc = right ? (c0 + TW) % g.Wp : (c0 - 1 + g.Wp) % g.Wp;
    const long o = (long)gr * g.rpitch + gc;
    const int li = ly * LW + (right ? TW + 1 : 0);
    sV[li] = V[o]; sW[li] = V2[o]; sR[li] = RB[o];
  }
  __syncthreads();

  const int ly = tid / QW, qx = tid - ly * QW;
  const int gr = r0 + ly, gc = c0 + 4 * qx;
  double sum[4] = {0., 0., 0., 0.};
  if (gr < g.Hp && gc < g.Wp) {
    const long ro = poff + (long)gr * g.rpitch;
    const long rd = poff + (long)((gr + 1) % g.Hp) * g.rpitch;         // the row below
    const int li = (ly + 1) * LW + 4 * qx + 1;
    real e0[4], b0[4], e0d[4], b0d[4], e1[5], b1[5];
    admm_bwd_unpack(admm_bwd_ldq(a.eta0 + ro, gc, g.Wp), e0);
    admm_bwd_unpack(admm_bwd_ldq(a.eb0 + ro, gc, g.Wp), b0);
    admm_bwd_unpack(admm_bwd_ldq(a.eta0 + rd, gc, g.Wp), e0d);
    admm_bwd_unpack(admm_bwd_ldq(a.eb0 + rd, gc, g.Wp), b0d);
    admm_bwd_unpack(admm_bwd_ldq(a.eta1 + ro, gc, g.Wp), e1);
    admm_bwd_unpack(admm_bwd_ldq(a.eb1 + ro, gc, g.Wp), b1);
    e1[4] = a.eta1[ro + (gc + 4) % g.Wp];
    b1[4] = a.eb1[ro + (gc + 4) % g.Wp];
    real hv[4], hv2[4], hr[4], xi[4], rho[4], xib[4], rhob[4];
    admm_bwd_unpack(admm_bwd_ldq(a.HV + ro, gc, g.Wp), hv);
    admm_bwd_unpack(admm_bwd_ldq(a.HV2 + ro, gc, g.Wp), hv2);
    admm_bwd_unpack(admm_bwd_ldq(a.hr + ro, gc, g.Wp), hr);
    admm_bwd_unpack(admm_bwd_ldq(a.xi + ro, gc, g.Wp), xi);
    admm_bwd_unpack(admm_bwd_ldq(a.rho + ro, gc, g.Wp), rho);
    admm_bwd_unpack(admm_bwd_ldq(a.xib + ro, gc, g.Wp), xib);
    admm_bwd_unpack(admm_bwd_ldq(a.rhob + ro, gc, g.Wp), rhob);

    // z = pb + m2' etab: component 0 here and one row below, component 1 here and one column to the right
    real z0[4], z0d[4], z1[5], n0[4], n1[5], unused;
    double none = 0.;
    for (int k = 0; k < 4; ++k) {
      const int l = li + k;
      const bool own = gc + k < g.Wp;
      admm_bwd_tv(p, sV[l], sV[l - LW], sW[l], sW[l - LW], sR[l], sR[l - LW], e0[k], b0[k], own, n0[k], z0[k], sum[1], sum[3]);
      admm_bwd_tv(p, sV[l + LW], sV[l], sW[l + LW], sW[l], sR[l + LW], sR[l], e0d[k], b0d[k], false, unused, z0d[k], none, none);
    }
    for (int k = 0; k < 5; ++k) {
      const int l = li + k;
      const bool own = k < 4 && gc + k < g.Wp;
      admm_bwd_tv(p, sV[l], sV[l - 1], sW[l], sW[l - 1], sR[l], sR[l - 1], e1[k], b1[k], own, n1[k], z1[k], sum[1], sum[3]);
    }

    // the point-wise rest: X, W recomputed; xib, rhob, g_b; r_sp and a of iteration i - 1
    const int dpl = (int)(pl / g.DC) * g.C + (int)(pl % g.C);
    const bool row_in = gr >= g.sh && gr < g.sh + g.H;
    const long yo = (long)dpl * g.uplane + (long)(gr - g.sh) * g.W - g.sw;       // + c: the un-padded pixel, inside only
    const long go = pl * g.uplane + (long)(gr - g.sh) * g.W - g.sw;
    real xin[4], rhn[4], rsp[4], aa[4];
    for (int k = 0; k < 4; ++k) {
      const int c = gc + k;
      const bool own = c < g.Wp;
      const bool inside = own && row_in && c >= g.sw && c < g.sw + g.W;
      const real yv = inside ? a.Y[yo + c] : (real)0.;
      const real m = inside ? p.m_in : p.m_out;
      const real vc = sV[li + k], wc = sW[li + k], rc = sR[li + k];
      const real X = m * (xi[k] + p.m1 * hv[k] + yv);
      const real q = rho[k] * p.r_m3 + vc;
      const real W = rmax(q, (real)0.);
      const real xm = xib[k] - hr[k], rm = rhob[k] - rc;
      const real qb = q > (real)0. ? -p.m3 * rm : (real)0.;
      const real xb = -p.m1 * xm * m;
      rhn[k] = rm + qb * p.r_m3;
      xin[k] = xm + xb;
      if (own) {
        sum[0] += (double)xm * (double)(hv2[k] - X) + (double)xb * (double)(hv[k] - X);
        sum[2] += (double)rm * (double)(wc - W) - (double)qb * (double)rho[k] * ((double)p.r_m3 * (double)p.r_m3);
      }
      if (inside && a.gb) a.gb[go + c] = p.gb_first ? xb : a.gb[go + c] + xb;
      rsp[k] = (qb + p.n3 * rhn[k]) + ((z0d[k] - z0[k]) + (z1[k + 1] - z1[k]));
      aa[k] = p.m1 * xb + p.n1 * xin[k];
    }
    admm_bwd_stq(a.xib + ro, gc, g.Wp, xin);
    admm_bwd_stq(a.rhob + ro, gc, g.Wp, rhn);
    admm_bwd_stq(a.eb0o + ro, gc, g.Wp, n0);
    admm_bwd_stq(a.eb1o + ro, gc, g.Wp, n1);
    if (p.pre) {
      admm_bwd_stq(a.Rsp + ro, gc, g.Wp, rsp);
      admm_bwd_stq(a.Aarr + ro, gc, g.Wp, aa);
    }
  }
  admm_bwd_block_sum4<NT>(sum, red, tid);
  if (tid == 0) {
    double* o = a.part + 4 * (pl * gridDim.x + blockIdx.x);
    for (int k = 0; k < 4; ++k) o[k] = sum[k];
  }
}

// ---- the replay: duals of iteration i + 1 from those of iteration i (the forward's recurrences, written out) -----------
template <int NT>
__global__ __launch_bounds__(NT) void k_admm_bwd_replay(PlaneGeom g, AdmmBwdScalars p, const real* LPC_RESTRICT V,
                                                         const real* LPC_RESTRICT HV, const real* LPC_RESTRICT V2,
                                                         const real* LPC_RESTRICT HV2, const real* LPC_RESTRICT Y,
                                                         const real* LPC_RESTRICT xi, const real* LPC_RESTRICT eta0,
                                                         const real* LPC_RESTRICT eta1, const real* LPC_RESTRICT rho,
                                                         real* LPC_RESTRICT xi_o, real* LPC_RESTRICT eta0_o,
                                                         real* LPC_RESTRICT eta1_o, real* LPC_RESTRICT rho_o) {
  const long n = (long)g.Hp * g.Wp;
  const long pl = blockIdx.y;
  const int dpl = (int)(pl / g.DC) * g.C + (int)(pl % g.C);
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int r = (int)(e / g.Wp), c = (int)(e - (long)r * g.Wp);
    const long o = pl * g.rplane + (long)r * g.rpitch + c;
    const long ou = pl * g.rplane + (long)wrap_add(r, -1, g.Hp) * g.rpitch + c;
    const long ol = pl * g.rplane + (long)r * g.rpitch + wrap_add(c, -1, g.Wp);
    const bool inside = (r >= g.sh) && (r < g.sh + g.H) && (c >= g.sw) && (c < g.sw + g.W);
    const real yv = inside ? Y[(long)dpl * g.uplane + (long)(r - g.sh) * g.W + (c - g.sw)] : (real)0.;
    const real vc = V[o], wc = V2[o];
    const real x = (inside ? p.m_in : p.m_out) * (xi[o] + p.m1 * HV[o] + yv);
    const real w = rmax(rho[o] * p.r_m3 + vc, (real)0.);
    const real u0 = soft_thresh_dev((V[ou] - vc) + eta0[o] * p.r_m2, p.thr);
    const real u1 = soft_thresh_dev((V[ol] - vc) + eta1[o] * p.r_m2, p.thr);
    xi_o[o] = xi[o] + p.m1 * (HV2[o] - x);
    eta0_o[o] = eta0[o] + p.m2 * ((V2[ou] - wc) - u0);
    eta1_o[o] = eta1[o] + p.m2 * ((V2[ol] - wc) - u1);
    rho_o[o] = rho[o] + p.m3 * (wc - w);
  }
}

// the start of the sweep: dL/dV_n = pad(dL/dout [crop(V_n) > 0]); `gv` holds the padded dL/dout on entry
template <int NT>
__global__ __launch_bounds__(NT) void k_admm_bwd_seed(PlaneGeom g, const real* LPC_RESTRICT Vn, real* LPC_RESTRICT gv) {
  const long n = (long)g.H * g.W;
  const long pl = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int r = (int)(e / g.W), c = (int)(e - (long)r * g.W);
    const long o = pl * g.rplane + (long)(r + g.sh) * g.rpitch + (c + g.sw);
    if (!(Vn[o] > (real)0.)) gv[o] = (real)0.;
  }
}

// ---- the gradient w.r.t. the PSF (lpc_admm_backward_psf) -----------------------------------------------------------------
// The PSF spectrum Hs enters iteration i in H V_{i+1} (the X half and the xi update of what follows), in HT a_i inside
// r_k, and in R_i = 1 / (m1 |Hs|^2 + m2 |G| + m3).  With F = rfft2, phi the +-1 phase of the ifftshift (even padded
// lengths; the engine's Hs does not carry it), ab the adjoint of H V_{i+1} (Aarr before the spectral step of iteration i),
// rb what that step returns and a_i = m1 X_i - xi_i, iteration i adds, summed over the frames of the batch,
//   g^ += phi conj(F V_{i+1}) F ab  +  phi conj(F rb) F a_i  -  2 m1 Re(conj(F rb) F V_{i+1}) Hs
// and g_psf = s crop_to_the_PSF_window(irfft2(g^)).  The accumulator holds phi g^: the generic inverse rows apply the
// ifftshift (a multiplication of the spectrum by phi) on the way out, so phi lands on the third term alone.

// a_i = m1 X_i - xi_i, recomputed from the tape (X as in k_admm_bwd_step / k_admm_bwd_replay)
template <int NT>
__global__ __launch_bounds__(NT) void k_admm_bwd_arec(PlaneGeom g, AdmmBwdScalars p, const real* LPC_RESTRICT HV,
                                                       const real* LPC_RESTRICT xi, const real* LPC_RESTRICT Y,
                                                       real* LPC_RESTRICT a_o) {
  const long n = (long)g.Hp * g.Wp;
  const long pl = blockIdx.y;
  const int dpl = (int)(pl / g.DC) * g.C + (int)(pl % g.C);
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int r = (int)(e / g.Wp), c = (int)(e - (long)r * g.Wp);
    const long o = pl * g.rplane + (long)r * g.rpitch + c;
    const bool inside = (r >= g.sh) && (r < g.sh + g.H) && (c >= g.sw) && (c < g.sw + g.W);
    const real yv = inside ? Y[(long)dpl * g.uplane + (long)(r - g.sh) * g.W + (c - g.sw)] : (real)0.;
    const real x = (inside ? p.m_in : p.m_out) * (xi[o] + p.m1 * HV[o] + yv);
    a_o[o] = p.m1 * x - xi[o];
  }
}

// One thread per spectral point (row blockIdx.y, column k) and channel (blockIdx.z): the B frames of the channel in a loop,
// one read-modify-write of the accumulator (`first`: a write).  Point-wise in the spectra's own layout -- whatever row
// order the launch plan keeps, Hs, the phase tables and the four work spectra share it.  No atomics.
template <int NT>
__global__ __launch_bounds__(NT) void k_admm_bwd_psf_acc(PlaneGeom g, int nframes, real two_m1,
                                                          const real2* LPC_RESTRICT FV, const real2* LPC_RESTRICT FR,
                                                          const real2* LPC_RESTRICT FA, const real2* LPC_RESTRICT FB,
                                                          const real2* LPC_RESTRICT Hs, const real2* LPC_RESTRICT phr,
                                                          const real2* LPC_RESTRICT phc, real2* LPC_RESTRICT acc,
                                                          int first) {
  const int k = (int)blockIdx.x * NT + (int)threadIdx.x;
  if (k >= g.Wc) return;
  const int row = blockIdx.y, c = blockIdx.z;
  const long off = (long)row * g.cpitch + k;
  const real2 h = Hs[(long)c * g.cplane + off];
  const real w = -two_m1 * (phr[row].x * phc[k].x);      // phi is real: +-1
  real2 s = first ? make_real2((real)0., (real)0.) : acc[(long)c * g.cplane + off];
  for (int b = 0; b < nframes; ++b) {
    const long o = (long)(b * g.C + c) * g.cplane + off;
    const real2 v = FV[o], r = FR[o], a = FA[o], ab = FB[o];
    const real t = w * (r.x * v.x + r.y * v.y);           // -2 m1 phi Re(conj(F rb) F V_{i+1})
    s.x += (v.x * ab.x + v.y * ab.y) + (r.x * a.x + r.y * a.y) + t * h.x;
    s.y += (v.x * ab.y - v.y * ab.x) + (r.x * a.y - r.y * a.x) + t * h.y;
  }
  acc[(long)c * g.cplane + off] = s;
}

// One PSF per frame (lpc_set_psf_batch; PlaneGeom::PM == all the planes): nothing is shared between the frames, so nothing
// is summed.  One thread per spectral point (row blockIdx.y, column k) and STATE plane q (blockIdx.z): it reads Hs[q] and
// the four work spectra at q and does one read-modify-write of acc[q] (`first`: a write) -- the term of
// k_admm_bwd_psf_acc for one frame, in its order.  Seven streams of consecutive real2 along k per wave, no loop, no atomics.
template <int NT>
__global__ __launch_bounds__(NT) void k_admm_bwd_psf_acc_frames(PlaneGeom g, real two_m1, const real2* LPC_RESTRICT FV,
                                                                 const real2* LPC_RESTRICT FR, const real2* LPC_RESTRICT FA,
                                                                 const real2* LPC_RESTRICT FB, const real2* LPC_RESTRICT Hs,
                                                                 const real2* LPC_RESTRICT phr, const real2* LPC_RESTRICT phc,
                                                                 real2* LPC_RESTRICT acc, int first) {
  const int k = (int)blockIdx.x * NT + (int)threadIdx.x;
  if (k >= g.Wc) return;
  const int row = blockIdx.y;
  const long o = (long)blockIdx.z * g.cplane + (long)row * g.cpitch + k;
  const real2 h = Hs[o];
  const real w = -two_m1 * (phr[row].x * phc[k].x);      // phi is real: +-1
  real2 s = first ? make_real2((real)0., (real)0.) : acc[o];
  const real2 v = FV[o], r = FR[o], a = FA[o], ab = FB[o];
  const real t = w * (r.x * v.x + r.y * v.y);             // -2 m1 phi Re(conj(F rb) F V_{i+1})
  s.x += (v.x * ab.x + v.y * ab.y) + (r.x * a.x + r.y * a.y) + t * h.x;
  s.y += (v.x * ab.y - v.y * ab.x) + (r.x * a.y - r.y * a.x) + t * h.y;
  acc[o] = s;
}

// ---- the finishing sum of iteration i: block q adds quantity q of every workgroup in a fixed order ----------------------
// g_mu1 = s0;  g_mu2 = s1 - s3 thr / m2;  g_mu3 = s2;  g_tau = s3 / m2        (thr = tau / m2)
template <int NT>
__global__ __launch_bounds__(NT) void k_admm_bwd_finish(const double* LPC_RESTRICT part, long nblk, double thr_over_m2,
                                                         double r_m2, real* LPC_RESTRICT g_mu1, real* LPC_RESTRICT g_mu2,
                                                         real* LPC_RESTRICT g_mu3, real* LPC_RESTRICT g_tau) {
  LPC_DYN_SMEM(smem);
  double* red = (double*)smem;
  const int tid = LPC_TID(NT);
  double s[4] = {0., 0., 0., 0.};
  for (long e = tid; e < nblk; e += NT)
    for (int k = 0; k < 4; ++k) s[k] += part[4 * e + k];
  admm_bwd_block_sum4<NT>(s, red, tid);
  if (tid == 0) {
    *g_mu1 = (real)s[0];
    *g_mu2 = (real)(s[1] - s[3] * thr_over_m2);
    *g_mu3 = (real)s[2];
    *g_tau = (real)(s[3] * r_m2);
  }
}
