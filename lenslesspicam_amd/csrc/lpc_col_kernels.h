// lpc_col_kernels.h -- the column passes: plain pass A / single pass (k_cols), the fused middles of a convolution
// (k_cols_mid_mul, _reg) and of an ADMM iteration (k_cols_mid_admm, _reg, _seq), and the sequential middle's
// precombined constants (k_mid_consts).  Launched by lpc_cols.cpp and the plan modules (lpc_launch.h).
#pragma once
#include "lpc_args.h"
#ifndef LPC_MID_FUSE1
#define LPC_MID_FUSE1 false  // measured: no gain on the fused middle (profiles/r01b_notes.md)
#endif
#ifndef LPC_MID_CONSTS_LATE
#define LPC_MID_CONSTS_LATE 1
#endif
#ifndef LPC_COLS_FUSEL
#define LPC_COLS_FUSEL true
#endif
// ================================================================== column passes ==
// element at a 32-bit byte offset from a workgroup-uniform base (SGPR base + VGPR offset addressing)
template <class T>
static __device__ __forceinline__ T ld_off(const T* LPC_RESTRICT ubase, unsigned byte_off) {
  return *(const T*)((const char*)ubase + byte_off);
}
template <class T>
static __device__ __forceinline__ void st_off(T* LPC_RESTRICT ubase, unsigned byte_off, T v) {
  *(T*)((char*)ubase + byte_off) = v;
}

// plain pass over ONE spectrum array, in place (global -> registers -> [LDS] -> registers -> global)
// PL / SBT: run-time plan (SBT unused), or a compile-time plan with SBT == cp.T columns per tile (lpc_sfft.h)
template <int NT, int EMAX, bool INV, class PL = Fft1dPlan, int SBT = 0, bool TWLDS = false>
__global__ __launch_bounds__(NT) void k_cols(PlaneGeom g, PL plan, ColPass cp,
                                              real2* LPC_RESTRICT S) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT);
  const unsigned bx = cp.rev ? gridDim.x - 1u - blockIdx.x : blockIdx.x;     // ColPass::rev
  const unsigned by = cp.rev ? gridDim.y - 1u - blockIdx.y : blockIdx.y;
  const int grp = (int)fd_div(bx, cp.tcdiv);
  const int c0 = ((int)bx - grp * cp.ntile_c) * cp.T;
  real2* base = S + (long)by * g.cplane + (long)grp * cp.gstride * g.cpitch + c0;
  const long rstep = (long)cp.istride * g.cpitch;
  // compile-time plans address the tile with 32-bit byte offsets from the workgroup-uniform base, row index x row step
  // as a 24-bit product (choose_plan() admits them only when the step is below 2^24 bytes): one full-rate v_mad_u32_u24
  // per access instead of a quarter-rate 64-bit multiply-add and a 64-bit shift-add
  constexpr bool O32 = is_static_plan<PL>::value;
  constexpr unsigned c8 = (unsigned)sizeof(real2);
  const unsigned r8 = (unsigned)rstep * c8;
  const int row0 = grp * cp.gstride;
  auto in = [&](int i, int c) {
    real2 x = make_real2((real)0., (real)0.);
    const int row = row0 + i * cp.istride;
    if (c0 + c < g.Wc && (INV || (row >= cp.zr0 && row < cp.zr1)))
      x = O32 ? ld_off(base, mul24((unsigned)i, r8) + (unsigned)c * c8) : base[i * rstep + c];
    // (a select + an unconditional product instead of this branch measured slower: pass A 0.47 -> 0.50 ms, r02am)
    if (!INV && (int)by >= cp.sc_plane0 && (row < cp.sc_r0 || row >= cp.sc_r1)) x = cscale(x, cp.sc);
    return x;
  };
  // compile-time plans (short transforms): the plan's twiddles and this group's four-step twiddles
  // twH[grp * i] live in LDS behind the tile (the host adds 2 n entries to the launch's LDS size)
  constexpr bool TWL = is_static_plan<PL>::value && TWLDS;
  const real2* tws = nullptr;
  if constexpr (TWL) {
    real2* t0 = s + PL::n * SBT;
    plan = twiddles_to_lds<NT>(plan, t0, tid);
    if ((!INV && cp.tw_mode == 1) || (INV && cp.tw_mode == 2)) {
      for (int i = tid; i < PL::n; i += NT) t0[PL::n + i] = cp.twH[grp * i];
      tws = t0 + PL::n;
    }
  }
  auto untwiddle = [&](int i, int, real2 x) {   // inverse pass A: conj four-step twiddle on the way in
    return (INV && cp.tw_mode == 2) ? cmul_conj(x, TWL ? tws[i] : cp.twH[grp * i]) : x;
  };
  auto out = [&](int i, int c, real2 x) {
    if (c0 + c < g.Wc) {
      if (!INV && cp.tw_mode == 1) x = cmul(x, TWL ? tws[i] : cp.twH[grp * i]);
      if (INV && cp.needn < g.Hp) {
        int d = row0 + i * cp.istride - cp.need0;
        d = d < 0 ? d + g.Hp : d;
        if (d >= cp.needn) return;
      }
      if (O32) st_off(base, mul24((unsigned)i, r8) + (unsigned)c * c8, x);
      else base[i * rstep + c] = x;
    }
  };
  if constexpr (is_static_plan<PL>::value) {
    // (SRC_LDS = TWL: the barrier between the tile's loads and `untwiddle` makes the staged twiddles visible)
    if (INV) fft_tile<NT, EMAX, INV, false, TWL, true, LPC_COLS_FUSEL, SBT>(s, plan, cp.T, cp.tdiv, tid, in, out, untwiddle);
    else fft_tile<NT, EMAX, INV, false, false, false, LPC_COLS_FUSEL, SBT>(s, plan, cp.T, cp.tdiv, tid, in, out);
  } else {
    if (INV) fft_tile<NT, EMAX, INV, false, false, true, LPC_COLS_FUSEL>(s, plan, cp.T, cp.tdiv, tid, in, out, untwiddle);
    else fft_tile<NT, EMAX, INV, false, false, false, LPC_COLS_FUSEL>(s, plan, cp.T, cp.tdiv, tid, in, out);
  }
}

// fused middle of a convolution: forward pass B -> multiply by the PSF spectrum (or its
// conjugate) -> inverse pass B, one trip through HBM.  hscale folds 1/(Hp*Wp).
template <int NT, int EMAX>
__global__ __launch_bounds__(NT) void k_cols_mid_mul(PlaneGeom g, Fft1dPlan plan, ColPass cp,
                                                      real2* LPC_RESTRICT S,
                                                      const real2* LPC_RESTRICT Hs, int conjH,
                                                      real hscale, int psf_planes) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT);
  const int T = cp.T;
  const int grp = (int)fd_div(blockIdx.x, cp.tcdiv);
  const int c0 = ((int)blockIdx.x - grp * cp.ntile_c) * T;
  const long rowoff = ((long)grp * cp.gstride) * g.cpitch + c0;
  real2* base = S + (long)blockIdx.y * g.cplane + rowoff;
  const real2* hb = Hs + (long)((int)blockIdx.y % psf_planes) * g.cplane + rowoff;
  const int nelem = cp.N * T;
  const long rstep = (long)cp.istride * g.cpitch;
  const int row0 = grp * cp.gstride;
  real2 h[EMAX];
#pragma unroll
  for (int k = 0; k < EMAX; ++k) {   // PSF spectrum tile: in flight during the forward transform
    const int e = tid + k * NT;
    h[k] = make_real2((real)0., (real)0.);
    if (e < nelem) {
      const int i = (int)fd_div((unsigned)e, cp.tdiv);
      const int j = e - i * T;
      if (c0 + j < g.Wc) h[k] = hb[i * rstep + j];
    }
  }
  auto in = [&](int i, int c) {
    const int row = row0 + i * cp.istride;
    return (c0 + c < g.Wc && row >= cp.zr0 && row < cp.zr1) ? base[i * rstep + c] : make_real2((real)0., (real)0.);
  };
  fft_tile<NT, EMAX, false, false, false, LPC_MID_FUSE1>(s, plan, T, cp.tdiv, tid, in, LdsNatural{});
#pragma unroll
  for (int k = 0; k < EMAX; ++k) {
    const int e = tid + k * NT;
    if (e < nelem) {
      real2 x = s[e];
      x = conjH ? cmul_conj(x, h[k]) : cmul(x, h[k]);
      s[e] = cscale(x, hscale);
    }
  }
  __syncthreads();
  auto out = [&](int i, int c, real2 x) {
    if (c0 + c < g.Wc) base[i * rstep + c] = x;
  };
  fft_tile<NT, EMAX, true, false, true, false, LPC_COLS_FUSEL>(s, plan, T, cp.tdiv, tid, LdsNatural{}, out);
}

// ---- register-resident middle (split column passes, short pass-B transforms) ---------------------------
// When the fused middle transform is short (N = R1*R2 <= 64, e.g. 48 = 8*6 at 6144 rows) ONE LANE can hold a whole
// column transform: N complex values in VGPRs, two-factor Cooley-Tukey with compile-time indices -- no LDS, no
// barriers, no index arithmetic, twiddles at constant table offsets (scalar loads).  A wave covers 64 adjacent
// columns, so every row access is one 512-byte segment.  Measured on MI355X (profiles/r01b_notes.md) the LDS
// version of this kernel spent a third of its time on un-hidden butterflies.
//
// forward: x[j1*R2 + j2] = element n = j1*R2 + j2 (natural)  ->  x[k1*R2 + k2] = X[k1 + R1*k2]
template <int R1, int R2>
static __device__ __forceinline__ void reg_fft_fwd(real2* x, const real2* LPC_RESTRICT tw) {
  constexpr int N = R1 * R2;
#pragma unroll
  for (int j2 = 0; j2 < R2; ++j2) {
    real2 v[R1];
#pragma unroll
    for (int j1 = 0; j1 < R1; ++j1) v[j1] = x[j1 * R2 + j2];
    Dft<R1, false>::run(v);
#pragma unroll
    for (int k1 = 0; k1 < R1; ++k1) x[k1 * R2 + j2] = (k1 * j2) ? cmul(v[k1], tw[(k1 * j2) % N]) : v[k1];
  }
#pragma unroll
  for (int k1 = 0; k1 < R1; ++k1) Dft<R2, false>::run(x + k1 * R2);
}
// inverse (unnormalised): x[k1*R2 + k2] = X[k1 + R1*k2] (what reg_fft_fwd leaves)  ->  x[s] = element s (natural)
template <int R1, int R2>
static __device__ __forceinline__ void reg_fft_inv(real2* x, const real2* LPC_RESTRICT tw) {
  constexpr int N = R1 * R2;
#pragma unroll
  for (int k1 = 0; k1 < R1; ++k1) {           // length-R2 transforms over k2, then the twiddle w^(m1*k1)
    Dft<R2, true>::run(x + k1 * R2);
#pragma unroll
    for (int m1 = 0; m1 < R2; ++m1)
      if (m1 * k1) x[k1 * R2 + m1] = cmul_conj(x[k1 * R2 + m1], tw[(m1 * k1) % N]);
  }
#pragma unroll
  for (int m1 = 0; m1 < R2; ++m1) {           // length-R1 transforms over k1: output m1 + R2*m2 at slot m2*R2 + m1
    real2 v[R1];
#pragma unroll
    for (int k1 = 0; k1 < R1; ++k1) v[k1] = x[k1 * R2 + m1];
    Dft<R1, true>::run(v);
#pragma unroll
    for (int m2 = 0; m2 < R1; ++m2) x[m2 * R2 + m1] = v[m2];
  }
}

// keeps the instruction scheduler from hoisting every load of a later phase to the top (which costs more
// registers than the lane has: measured 996 bytes of scratch per lane without the fences)
#if defined(LPC_SIMT_EMU)
#define LPC_SCHED_FENCE() ((void)0)
#else
#define LPC_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif
// 1 / d for the ADMM middles' R_divmat (admm.py:186-190; d = mu1 |H|^2 + mu2 |G| + mu3 > 0, far from the overflow and
// denormal ranges): the hardware reciprocal (1 ulp) + one Newton step = 3 VALU operations, against ~10 for the compiler's
// IEEE division (v_div_scale x2, v_rcp, 4 fma, v_div_fmas, v_div_fixup) -- 170 of the sequential middle's 3100.
static __device__ __forceinline__ real recip_pos(real d) {
#if defined(LPC_SIMT_EMU) || defined(LPC_DOUBLE)
  return (real)1.0 / d;
#else
  const float r = __builtin_amdgcn_rcpf(d);
  return fmaf(fmaf(-d, r, 1.0f), r, r);
#endif
}
// fused middle of a convolution, register-resident (same contract as k_cols_mid_mul; split passes only:
// cp.istride == 1, every row valid).  grid = (ceil(Wc/64), groups, planes), 64 threads.
template <int R1, int R2>
__global__ __launch_bounds__(64) void k_cols_mid_mul_reg(PlaneGeom g, Fft1dPlan plan, ColPass cp,
                                                          real2* LPC_RESTRICT S, const real2* LPC_RESTRICT Hs,
                                                          int conjH, real hscale, int psf_planes) {
  constexpr int N = R1 * R2;
  const int col = (int)LPC_BX(g) * 64 + (int)threadIdx.x;
  if (col >= g.Wc) return;
  // plain 64-bit addresses on purpose: with wave-uniform bases + 32-bit offsets this kernel needs 58 instead of
  // 214 AGPRs but runs 65 % slower (0.62 vs 0.38 ms at 12 MP) -- the hoisted address arithmetic is what lets
  // all 2N loads of a lane be in flight at once
  const long rowoff = (long)LPC_BY(g) * cp.gstride * g.cpitch + col;
  real2* base = S + (long)LPC_BZ(g) * g.cplane + rowoff;
  const real2* hb = Hs + (long)((int)LPC_BZ(g) % psf_planes) * g.cplane + rowoff;
  real2 x[N], h[N];
#pragma unroll
  for (int n = 0; n < N; ++n) x[n] = base[(long)n * g.cpitch];
#pragma unroll
  for (int n = 0; n < N; ++n) h[n] = hb[(long)n * g.cpitch];
  reg_fft_fwd<R1, R2>(x, plan.tw);
  const real hs = conjH ? -hscale : hscale;
#pragma unroll
  for (int k1 = 0; k1 < R1; ++k1)
#pragma unroll
    for (int k2 = 0; k2 < R2; ++k2) {
      const real2 hh = make_real2(h[k1 + R1 * k2].x * hscale, h[k1 + R1 * k2].y * hs);   // H or conj(H), scaled
      x[k1 * R2 + k2] = cmul(x[k1 * R2 + k2], hh);
    }
  reg_fft_inv<R1, R2>(x, plan.tw);
#pragma unroll
  for (int n = 0; n < N; ++n) base[(long)n * g.cpitch] = x[n];
}

// fused middle of one ADMM iteration, register-resident (same contract as k_cols_mid_admm below; split passes
// only, SHORT pass-B transforms: the lane holds 2 x N complex values).  One lane owns column c of BOTH spectra,
// one after the other: a = FFT(SB column) is turned into t = s conj(H) a in place, then r = FFT(SA column),
// Vh = Rdiv (r + t) and HVh = s H Vh overwrite the two register arrays, which are inverse-transformed and stored.
// The row phases are wave-uniform (scalar loads), H is simply read twice.
// grid = (ceil(Wc/64), groups, planes), 64 threads.
template <int R1, int R2>
__global__ __launch_bounds__(64) void k_cols_mid_admm_reg(PlaneGeom g, Fft1dPlan plan, ColPass cp,
                                                           real2* LPC_RESTRICT SA, real2* LPC_RESTRICT SB,
                                                           const real2* LPC_RESTRICT Hs,
                                                           const real* LPC_RESTRICT Gabs,
                                                           const real2* LPC_RESTRICT phr,
                                                           const real2* LPC_RESTRICT phc, real mu1, real mu2,
                                                           real mu3, real rscale) {
  constexpr int N = R1 * R2;
  const int col = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (col >= g.Wc) return;
  const int row0 = (int)blockIdx.y * cp.gstride;
  // wave-uniform bases (SGPR pairs) + 32-bit per-lane byte offsets: global_load ... v_off, s[base]
  const long urow = (long)row0 * g.cpitch;
  real2* ba = SA + (long)blockIdx.z * g.cplane + urow;
  real2* bb = SB + (long)blockIdx.z * g.cplane + urow;
  const real2* hb = Hs + (long)((int)blockIdx.z % g.PM) * g.cplane + urow;
  const real* gb = Gabs + urow;
  const bool gsep = cp.ga != nullptr;
  const real* gar = gsep ? cp.ga + row0 : Gabs;          // wave-uniform row terms (scalar loads, like the row phases)
  const real gcol = gsep ? cp.gb[col] : (real)0.;
  const real2* pr = phr + row0;
  const real2 pc = phc[col];
  const unsigned c8 = (unsigned)col * (unsigned)sizeof(real2), c4 = (unsigned)col * (unsigned)sizeof(real);
  const unsigned p8 = (unsigned)g.cpitch * (unsigned)sizeof(real2), p4 = (unsigned)g.cpitch * (unsigned)sizeof(real);
  real2 a[N], r[N];
#pragma unroll
  for (int n = 0; n < N; ++n) a[n] = ld_off(bb, c8 + (unsigned)n * p8);
#pragma unroll
  for (int n = 0; n < N; ++n) r[n] = ld_off(ba, c8 + (unsigned)n * p8);
  LPC_SCHED_FENCE();
  reg_fft_fwd<R1, R2>(a, plan.tw);
  LPC_SCHED_FENCE();
#pragma unroll
  for (int k1 = 0; k1 < R1; ++k1) {
    LPC_SCHED_FENCE();
#pragma unroll
    for (int k2 = 0; k2 < R2; ++k2) {          // slot k1*R2 + k2 holds frequency k = k1 + R1*k2
      const int k = k1 + R1 * k2;
      a[k1 * R2 + k2] = cmul(cmul_conj(a[k1 * R2 + k2], ld_off(hb, c8 + (unsigned)k * p8)), cmul(pr[k], pc));
    }
  }
  LPC_SCHED_FENCE();
  reg_fft_fwd<R1, R2>(r, plan.tw);
  LPC_SCHED_FENCE();
#pragma unroll
  for (int k1 = 0; k1 < R1; ++k1) {
    LPC_SCHED_FENCE();
#pragma unroll
    for (int k2 = 0; k2 < R2; ++k2) {
      const int k = k1 + R1 * k2, sl = k1 * R2 + k2;
      const real2 hh = ld_off(hb, c8 + (unsigned)k * p8);
      const real gk = gsep ? gar[k] + gcol : ld_off(gb, c4 + (unsigned)k * p4);
      const real rdiv = rscale * recip_pos(mu1 * rabs(hh.x * hh.x + hh.y * hh.y) + mu2 * gk + mu3);
      const real2 vh = cscale(cadd(r[sl], a[sl]), rdiv);
      r[sl] = vh;
      a[sl] = cmul(cmul(vh, hh), cmul(pr[k], pc));
    }
  }
  LPC_SCHED_FENCE();
  reg_fft_inv<R1, R2>(r, plan.tw);
#pragma unroll
  for (int n = 0; n < N; ++n) st_off(ba, c8 + (unsigned)n * p8, r[n]);
  LPC_SCHED_FENCE();
  reg_fft_inv<R1, R2>(a, plan.tw);
#pragma unroll
  for (int n = 0; n < N; ++n) st_off(bb, c8 + (unsigned)n * p8, a[n]);
}

// fused middle of one ADMM iteration (4-FFT form).  In: SA = rows+colsA transform of
// r_sp, SB = same of a = mu1 X - xi.  After forward pass B:
//   Vh  = Rdiv * (Rh + s * conj(H) * Ah)        (Rdiv formed in-kernel, includes 1/(Hp*Wp))
//   HVh = s * H * Vh                             (s = spectral phase of ifftshift)
// then inverse pass B; SA <- Vh path, SB <- HVh path.
// Tile: [N][2T] -- columns 0..T-1 belong to SA, T..2T-1 to SB.
// PL / SBT2: run-time plan, or a compile-time plan with SBT2 == 2 * cp.T tile columns (both arrays)
// SL = 1 (single-pass columns, T == 8, compile-time plans): the work spectra and the copies of H / |G| passed in are in
// the pair-line layout (spec_col): the tile's rows (2p, 2p + 1) of either array are one 128-byte line.
template <int NT, int EMAX, class PL = Fft1dPlan, int SBT2 = 0, bool TWLDS = false, int SL = 0>
__global__ __launch_bounds__(NT) void k_cols_mid_admm(PlaneGeom g, PL plan, ColPass cp,
                                                       real2* LPC_RESTRICT SA,
                                                       real2* LPC_RESTRICT SB,
                                                       const real2* LPC_RESTRICT Hs,
                                                       const real* LPC_RESTRICT Gabs,
                                                       const real2* LPC_RESTRICT phr,
                                                       const real2* LPC_RESTRICT phc,
                                                       FastDiv t2div, real mu1, real mu2, real mu3,
                                                       real rscale, real sb_outside_scale) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT);
  LPC_STAMP_BEGIN(2);
  // (compile-time plans: the tile width is a constant -- e / T, e % T are shifts, not reciprocal multiplies)
  const int T = is_static_plan<PL>::value ? SBT2 / 2 : cp.T, T2 = 2 * T;
  unsigned bid = cp.rev ? gridDim.x - 1u - blockIdx.x : blockIdx.x;
  const unsigned by = cp.rev ? gridDim.y - 1u - blockIdx.y : blockIdx.y;
  if (cp.swz && bid < (gridDim.x & ~15u)) bid = (bid & ~15u) + ((bid & 7u) << 1) + ((bid >> 3) & 1u);   // ColPass::swz
  const int grp = (int)fd_div(bid, cp.tcdiv);
  const int c0 = ((int)bid - grp * cp.ntile_c) * T;
  static_assert(!SL || (is_static_plan<PL>::value && SBT2 == 16), "pair lines: 8 columns per array, compile-time plans");
  const long rowoff = ((long)grp * cp.gstride) * g.cpitch + (SL ? 2 * c0 : c0);      // (SL: single pass, grp == 0)
  real2* ba = SA + (long)by * g.cplane + rowoff;
  real2* bb = SB + (long)by * g.cplane + rowoff;
  const int pp = (int)by % g.PM;
  const real2* hb = Hs + (long)pp * g.cplane + rowoff;
  const real* rb = Gabs + rowoff;  // |PsiT Psi| spectrum: one plane, the same for every channel
  const int npair = cp.N * T;
  const long rstep = (long)cp.istride * g.cpitch;
  constexpr int EP = (EMAX + 1) / 2;
  constexpr bool O32 = is_static_plan<PL>::value;      // 32-bit byte offsets, see k_cols
  constexpr unsigned c8 = (unsigned)sizeof(real2), c4 = (unsigned)sizeof(real);
  const unsigned r8 = (unsigned)rstep * c8, r4 = (unsigned)rstep * c4;
  // byte offsets of (row i, column j of the array's 8): see k_cols_mid_admm_seq
  auto off8 = [=](int i, int j) {
    const unsigned e8 = ((unsigned)i << 3) | (unsigned)j;
    return SL ? mul24(e8 >> 4, 2u * r8) + ((e8 & 15u) << 3) : mul24((unsigned)i, r8) + (unsigned)j * c8;
  };
  auto off4 = [=](int i, int j) {
    const unsigned e8 = ((unsigned)i << 3) | (unsigned)j;
    return SL ? mul24(e8 >> 4, 2u * r4) + ((e8 & 15u) << 2) : mul24((unsigned)i, r4) + (unsigned)j * c4;
  };
  real2 h[EP];
  real rd[EP];
  // spectral constants: in flight during the forward FFT.  Compile-time plans issue them BEHIND the tile loads (hook of
  // fft_tile): the memory counter is in order, and in front of them they delayed the first stage by their own latency --
  // one small frame is a chain of latencies (profiles/r05_notes.md section 5)
  // Branch-free: loads behind `if (e < npair)` / `if (c0 + j < Wc)` each got a `s_waitcnt vmcnt(0)` of their own (five
  // latencies one after the other per lane at C1).  Lanes without an element load element 0, columns past the frame's edge
  // the frame's last column; neither value is used.
  const int jmax = g.Wc - 1 - c0;
  auto consts_of = [&](auto terms_c) {
    constexpr bool TERMS = decltype(terms_c)::value;
#pragma unroll
    for (int k = 0; k < EP; ++k) {
      const int e = tid + k * NT, ec = e < npair ? e : 0;
      const int i = (is_static_plan<PL>::value ? ec / T : (int)fd_div((unsigned)ec, cp.tdiv));
      const int j = ec - i * T, jc = j < jmax ? j : jmax;
      if (O32) h[k] = ld_off(hb, off8(i, jc));
      else h[k] = hb[i * rstep + jc];
      if (TERMS) rd[k] = cp.ga[grp * cp.gstride + i * cp.istride] + cp.gb[c0 + jc];      // rd: |G| for now
      else if (O32) rd[k] = ld_off(rb, off4(i, jc));
      else rd[k] = rb[i * rstep + jc];
    }
  };
  auto consts = [&]() {
    if (cp.ga) consts_of(std::true_type{});
    else consts_of(std::false_type{});
  };
  if constexpr (!(is_static_plan<PL>::value && LPC_MID_CONSTS_LATE)) consts();
  // sb_outside_scale != 0 (AdmmScalars::skipa, single-pass columns only): the rows of SB outside the sensor window were
  // not re-transformed; they hold rfft(H V row) / Wp from the last inverse row pass, and a = mu1 H V there
  const real sb_k = sb_outside_scale != (real)0. ? sb_outside_scale : (real)1.;
  // The tile loads carry neither a branch nor arithmetic (a column past the frame's edge is a copy of the frame's last
  // column: an independent transform that is never stored); the scale of SB's rows is applied where the value goes into
  // LDS (`fix` of fft_tile) -- with the product behind the load the one guarded element of a lane waited for ALL loads.
  auto in = [&](int i, int c) {
    const int j = c < T ? c : c - T, jc = j < jmax ? j : jmax;
    return O32 ? ld_off(c < T ? ba : bb, off8(i, jc)) : (c < T ? ba : bb)[i * rstep + jc];
  };
  auto in_fix = [&](int i, int c, real2 x) {
    return cscale(x, (c >= T && (unsigned)(i - g.sh) >= (unsigned)g.H) ? sb_k : (real)1.);
  };
  if constexpr (is_static_plan<PL>::value) {
    if constexpr (LPC_MID_CONSTS_LATE) {
      // behind the tile loads: the twiddle table's loads (-> LDS, lpc_sfft.h), then the constants
      const PL gplan = plan;
      if constexpr (TWLDS) plan.tw = s + PL::n * SBT2;
      real2* twl = s + PL::n * SBT2;
      auto hook = [&]() {
        if constexpr (TWLDS) twiddles_to_lds_around<NT>(gplan, twl, tid, consts);
        else consts();
      };
      fft_tile<NT, EMAX, false, false, false, LPC_MID_FUSE1, false, SBT2>(s, plan, T2, t2div, tid, in, LdsNatural{}, in_fix, hook);
    } else {
      if constexpr (TWLDS) plan = twiddles_to_lds<NT>(plan, s + PL::n * SBT2, tid);
      fft_tile<NT, EMAX, false, false, false, LPC_MID_FUSE1, false, SBT2>(s, plan, T2, t2div, tid, in, LdsNatural{}, in_fix);
    }
  } else
    fft_tile<NT, EMAX, false, false, false, LPC_MID_FUSE1>(s, plan, T2, t2div, tid, in, LdsNatural{}, in_fix);
  // (branch-free like the constants, only the two LDS stores are conditional; all phase factors are requested before the
  // first is used: loaded where they were used, every element waited for its own pair)
  real2 pr[EP], pc[EP];
#pragma unroll
  for (int k = 0; k < EP; ++k) {
    const int e = tid + k * NT, ec = e < npair ? e : 0;
    const int i = (is_static_plan<PL>::value ? ec / T : (int)fd_div((unsigned)ec, cp.tdiv));
    const int j = ec - i * T, jc = j < jmax ? j : jmax;
    pr[k] = phr[grp * cp.gstride + i * cp.istride];
    pc[k] = phc[c0 + jc];
  }
#pragma unroll
  for (int k = 0; k < EP; ++k) {
    const int e = tid + k * NT, ec = e < npair ? e : 0;
    const int i = (is_static_plan<PL>::value ? ec / T : (int)fd_div((unsigned)ec, cp.tdiv));
    const int j = ec - i * T, jc = j < jmax ? j : jmax;
    const real2 hh = h[k];
    // R_divmat = 1 / (mu1 |H* H| + mu2 |PsiT Psi| + mu3)  (admm.py:186-190), formed on the fly so
    // that per-iteration step sizes cost nothing; rscale folds the inverse FFT's 1/(Hp*Wp)
    const real rdiv = rscale * recip_pos(mu1 * rabs(hh.x * hh.x + hh.y * hh.y) + mu2 * rd[k] + mu3);
    const real2 ph = cmul(pr[k], pc[k]);
    const real2 rh = s[i * T2 + jc];
    const real2 ah = s[i * T2 + T + jc];
    real2 t = cmul(cmul_conj(ah, hh), ph);          // s * conj(H) * Ah
    real2 vh = cscale(cadd(rh, t), rdiv);
    real2 hv = cmul(cmul(vh, hh), ph);
    if (e < npair && j <= jmax) {
      s[i * T2 + j] = vh;
      s[i * T2 + T + j] = hv;
    }
  }
  __syncthreads();
  auto out = [&](int i, int c, real2 x) {
    const int j = c < T ? c : c - T;
    if (c0 + j < g.Wc) {
      if (O32) st_off(c < T ? ba : bb, off8(i, j), x);
      else (c < T ? ba : bb)[i * rstep + j] = x;
    }
  };
  if constexpr (is_static_plan<PL>::value)
    fft_tile<NT, EMAX, true, false, true, false, LPC_COLS_FUSEL, SBT2>(s, plan, T2, t2div, tid, LdsNatural{}, out);
  else
    fft_tile<NT, EMAX, true, false, true, false, LPC_COLS_FUSEL>(s, plan, T2, t2div, tid, LdsNatural{}, out);
  LPC_STAMP_END();
}

// ---- the point-wise step's constants of the pair-line sequential middle, precombined ------------------------------------
// Step 3 of k_cols_mid_admm_seq needs, per tile element, H, |G|, the row and the column phase: four loads and a
// reciprocal per element, nine elements per lane, each waiting for its own loads -- a third of a workgroup's lifetime at C4
// (profiles/r05_notes.md section 5).  They depend on the PSF plane and the step sizes only, not on the frame: one small
// kernel forms  c1 = conj(H) ph,  c2 = H ph  (ph = phr[row] phc[column])  and  rd = rscale / (mu1 |H|^2 + mu2 |G| + mu3)
// once per (PSF, step sizes) -- every iteration of an unrolled schedule, never again otherwise -- in the pair-line
// layout; the step then is one 16-byte and one 4-byte load and three products per element.
// ---- the same fused middle, ONE ARRAY AT A TIME through a tile of T image columns (single-pass columns only) ------
// k_cols_mid_admm keeps both spectra in one [N][2T] tile; when a whole column is long (540 rows for the
// DiffuserCam-sized frames of C1 / C4) that tile allows only T = 8 columns per array -- 64-byte row segments, half a
// cache line per access.  Here the transform of `a` is parked in registers (N*T/NT values per lane) while the same
// LDS tile transforms `r_sp`: either T = 16 columns per workgroup in the same 69 KiB (every row access a whole 128-byte
// line, half as many workgroups), or -- the default since round 3 -- T = 8 columns in 39 KiB on 256 lanes: four
// workgroups per CU, each barrier over 4 waves instead of 8, and the frames-fastest block order below puts the two
// tiles that share a cache line on the same XCD 1.5 MB apart (C4: 0.608 -> 0.550 ms per launch, r03_notes.md section 15).
// H and |G| are shared by all frames of a batch (L2-resident) and are loaded where they are used.  Compile-time plans
// only (SBT == cp.T).
// SL = 1: the work spectra AND the copies of H / |G| passed in are in the pair-line layout (spec_col; T == 8): a tile's
// rows (2p, 2p + 1) are one 128-byte line.
// PC (with SL): Hs / Gabs are the precombined constants of k_mid_consts (1: MidConst planes, 2: c1 planes -- real phases --
// and the rd planes), phr / phc are not read.
template <int NT, int EMAX, class PL, int SBT, int MINW = 1, bool PRE = false, int SL = 0, int PC = 0>
__global__ __launch_bounds__(NT, MINW) void k_cols_mid_admm_seq(PlaneGeom g, PL plan, ColPass cp, real2* LPC_RESTRICT SA,
                                                           real2* LPC_RESTRICT SB, const real2* LPC_RESTRICT Hs,
                                                           const real* LPC_RESTRICT Gabs, const real2* LPC_RESTRICT phr,
                                                           const real2* LPC_RESTRICT phc, real mu1, real mu2, real mu3,
                                                           real rscale, real sb_outside_scale) {
  static_assert(!PC || SL, "precombined constants live in the pair-line layout");
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  // (plain threadIdx.x, not LPC_TID: knowing tid < NT the optimiser keeps all 17 row indices of a lane -- as 64-bit
  // offsets for ga[] / phr[] -- alive from the tile loads to the point-wise step and spills them: 144 bytes of scratch,
  // C4's middle 0.484 -> 0.797 ms, profiles/r04g_ab.log)
  const int tid = threadIdx.x;
  constexpr int T = SBT, N = PL::n, NELEM = N * T, EM = (NELEM + NT - 1) / NT;
  static_assert(EM <= EMAX, "tile does not fit the workgroup shape");
  LPC_STAMP_BEGIN(2);
  // 1-D grid of (column tiles x planes) workgroups, FRAMES FASTEST: all frames of a batch share H and |G|, and block b
  // runs on XCD b % 8 -- consecutive blocks are the same column tile of the same PSF plane in different frames, so each
  // XCD's L2 fetches that tile of H / |G| from HBM once and serves it to the frames it owns.  (With the tile index
  // fastest, the 64 frames of C4 re-read H 64 times: PMC traffic 2.29 GB per launch against 1.60 GB algorithmic.)
  // (One PSF per frame, PlaneGeom::PM == all the planes: nfr == 1 and pp is the state plane itself -- nothing is shared
  // between frames then, and the order is neutral)
  const int nfr = (int)(gridDim.x / (unsigned)(cp.ntile_c * g.PM));       // frames (that share a PSF plane)
  const unsigned bx = cp.rev ? gridDim.x - 1u - blockIdx.x : blockIdx.x;   // ColPass::rev
  const int fr = (int)(bx % (unsigned)nfr), rest = (int)(bx / (unsigned)nfr);
  const int tile = rest % cp.ntile_c, pp = rest / cp.ntile_c;             // column tile, PSF plane
  const long pl = (long)fr * g.PM + pp;
  const int c0 = tile * T;
  static_assert(!SL || T == 8, "pair lines hold 8 columns of two rows");
  const int cb = SL ? 2 * c0 : c0;                  // first element of the tile's column chunk within a row (pair)
  real2* ba = SA + pl * g.cplane + cb;
  real2* bb = SB + pl * g.cplane + cb;
  const real2* hb = Hs + (PC == 1 ? 2 : 1) * ((long)pp * g.cplane + cb);       // (PC == 1: 16-byte elements)
  const real* rb = Gabs + (PC ? (long)pp * g.cplane : 0) + cb;
  // 32-bit byte offsets from workgroup-uniform bases (a plane is < 4 GB): one v_mad_u32 per access instead of a
  // 64-bit multiply-add (quarter rate) + 64-bit shift-add
  const unsigned r8 = (unsigned)g.cpitch * (unsigned)sizeof(real2), r4 = (unsigned)g.cpitch * (unsigned)sizeof(real);
  constexpr unsigned c8 = (unsigned)sizeof(real2), c4 = (unsigned)sizeof(real);
  // byte offset of tile element (row i, column j) of an array of 8- / 4-byte elements.  Pair lines: with e = 8 i + j (the
  // element's index in the [N][8] tile) the pair is e >> 4 (2 cpitch elements each) and the place in its line e & 15 --
  // the same two operations as the plain layout's i * pitch + j
  auto off8 = [=](int i, int j) {
    const unsigned e8 = ((unsigned)i << 3) | (unsigned)j;
    return SL ? mul24(e8 >> 4, 2u * r8) + ((e8 & 15u) << 3) : mul24((unsigned)i, r8) + (unsigned)j * c8;
  };
  auto off4 = [=](int i, int j) {
    const unsigned e8 = ((unsigned)i << 3) | (unsigned)j;
    return SL ? mul24(e8 >> 4, 2u * r4) + ((e8 & 15u) << 2) : mul24((unsigned)i, r4) + (unsigned)j * c4;
  };
  // A lane's elements in tile order, e = tid + k NT, keep their column j0 and advance RSTEP rows per round: every tile-order
  // access is (uniform base + k * rstep elements) + ONE lane-constant byte offset -- no address arithmetic, no address
  // registers per access (under the 64-VGPR bound of four workgroups per CU a per-access v_mad spilled: 44-88 bytes of
  // scratch with the pair-line offsets, the 8-frame shard's middle 0.068 -> 0.089 ms)
  static_assert(NT % T == 0 && (!SL || (NT / T) % 2 == 0), "a lane keeps its column (and its row parity) from round to round");
  constexpr int RSTEP = NT / T, KFULL = NELEM / NT;   // (KFULL: rounds in which every lane has an element)
  const int i0 = tid / T, j0 = tid % T;
  const unsigned l8 = off8(i0, j0), l4 = off4(i0, j0);
  const long rstep = (long)RSTEP * g.cpitch;
  // sb_outside_scale != 0 (AdmmScalars::skipa): the rows of SB outside the sensor window were not re-transformed; they
  // hold rfft(H V row) / Wp from the last inverse row pass, and a = mu1 H V there
  const real sb_k = sb_outside_scale != (real)0. ? sb_outside_scale : (real)1.;
  const int wc = g.Wc - c0, sh = g.sh, hwin = g.H;
  // Loads are UNCONDITIONAL and carry no arithmetic: the columns of a tile are independent transforms, so a column past
  // the frame's edge may hold whatever the row padding holds (cpitch is a multiple of 16 >= every tile width: the
  // address is always inside the plane) -- it is never stored; the tail lanes of the last round load the round's first
  // element.  The scale of SB's rows is applied where the value goes into LDS.
  static_assert(16 % T == 0, "tile columns must stay inside the padded row pitch");
  auto tile_ld = [=](const real2* base, int k) {
    return ld_off(base + k * rstep, (k < KFULL || tid + k * NT < NELEM) ? l8 : 0u);
  };
  auto fixB = [=](int i, real2 x) {
    return cscale(x, (unsigned)(i - sh) >= (unsigned)hwin ? sb_k : (real)1.);   // one compare, one select, one product
  };
  // the twiddle table moves into LDS behind the tile (lpc_sfft.h twiddles_to_lds)
  plan = twiddles_to_lds<NT>(plan, s + NELEM, tid);
  real2 a[EM];
  {
    // PRE: both tiles' loads are issued up front, `a` first, r_sp right behind it: the transform of `a` then runs while
    // the tile of r_sp is still in flight (the wait for `a` is a vmcnt(EM), not a vmcnt(0)), instead of every workgroup
    // sitting out two full load latencies.  The registers that later park Ah hold the r_sp tile until then.  Otherwise
    // (launches of few workgroups per CU) r_sp's loads go out behind the transform of `a`.
    real2 pb[EM], pa[EM];
#pragma unroll
    for (int k = 0; k < EM; ++k) pb[k] = tile_ld(bb, k);
    if constexpr (PRE) {
#pragma unroll
      for (int k = 0; k < EM; ++k) pa[k] = tile_ld(ba, k);
    }
#pragma unroll
    for (int k = 0; k < EM; ++k)
      if (k < KFULL || tid + k * NT < NELEM) s[tid + k * NT] = fixB(i0 + k * RSTEP, pb[k]);
    __syncthreads();
    // 1. Ah = FFT(a), parked in registers in tile order
    fft_tile<NT, EMAX, false, false, false, false, false, SBT>(s, plan, T, cp.tdiv, tid, LdsNatural{}, LdsNatural{});
#pragma unroll
    for (int k = 0; k < EM; ++k) {
      a[k] = make_real2((real)0., (real)0.);
      if (k < KFULL || tid + k * NT < NELEM) a[k] = s[tid + k * NT];
    }
    if constexpr (!PRE) {
#pragma unroll
      for (int k = 0; k < EM; ++k) pa[k] = tile_ld(ba, k);
    }
    __syncthreads();
    // 2. Rh = FFT(r_sp) in the same tile
#pragma unroll
    for (int k = 0; k < EM; ++k)
      if (k < KFULL || tid + k * NT < NELEM) s[tid + k * NT] = pa[k];
    __syncthreads();
    fft_tile<NT, EMAX, false, false, false, false, false, SBT>(s, plan, T, cp.tdiv, tid, LdsNatural{}, LdsNatural{});
  }
  // 3. Vh = Rdiv (Rh + s conj(H) Ah) -> tile;  HVh = s H Vh -> the registers that held Ah
#pragma unroll
  for (int k = 0; k < EM; ++k) {
    if (k < KFULL || tid + k * NT < NELEM) {
      if (j0 < wc) {
        const int e = tid + k * NT, i = i0 + k * RSTEP;
        if constexpr (PC == 1) {
          const MidConst mc = ld_off((const MidConst*)hb + k * rstep, 2u * l8);
          const real rdiv = ld_off(rb + k * rstep, l4);
          const real2 vh = cscale(cadd(s[e], cmul(a[k], mc.c1)), rdiv);
          s[e] = vh;
          a[k] = cmul(vh, mc.c2);
        } else if constexpr (PC == 2) {
          const real2 c1 = ld_off(hb + k * rstep, l8);
          const real rdiv = ld_off(rb + k * rstep, l4);
          const real2 vh = cscale(cadd(s[e], cmul(a[k], c1)), rdiv);
          s[e] = vh;
          a[k] = cmul_conj(vh, c1);
        } else {
          const real2 hh = ld_off(hb + k * rstep, l8);
          const real gk = cp.ga ? cp.ga[i] + cp.gb[c0 + j0] : ld_off(rb + k * rstep, l4);
          const real rdiv = rscale * recip_pos(mu1 * rabs(hh.x * hh.x + hh.y * hh.y) + mu2 * gk + mu3);
          const real2 ph = cmul(phr[i], phc[c0 + j0]);
          const real2 t = cmul(cmul_conj(a[k], hh), ph);
          const real2 vh = cscale(cadd(s[e], t), rdiv);
          s[e] = vh;
          a[k] = cmul(cmul(vh, hh), ph);
        }
      }
    }
  }
  __syncthreads();
  // 4. V-hat back through the inverse transform, straight to SA
  auto outA = [=](int i, int j, real2 x) { if (j < wc) st_off(ba, off8(i, j), x); };
  fft_tile<NT, EMAX, true, false, true, false, LPC_COLS_FUSEL, SBT>(s, plan, T, cp.tdiv, tid, LdsNatural{}, outA);
  __syncthreads();
  // 5. H V-hat: registers -> tile -> inverse transform -> SB
#pragma unroll
  for (int k = 0; k < EM; ++k) {
    const int e = tid + k * NT;
    if (e < NELEM) s[e] = a[k];
  }
  __syncthreads();
  auto outB = [=](int i, int j, real2 x) { if (j < wc) st_off(bb, off8(i, j), x); };
  fft_tile<NT, EMAX, true, false, true, false, LPC_COLS_FUSEL, SBT>(s, plan, T, cp.tdiv, tid, LdsNatural{}, outB);
  LPC_STAMP_END();
}

// REALPH: the phases are +-1 (even padded sizes: ifftshift = (-1)^k per axis), c2 = conj(c1): only c1 is stored (8 bytes)
template <int NT, bool REALPH>
__global__ __launch_bounds__(NT) void k_mid_consts(const real2* LPC_RESTRICT Hs_t, const real* LPC_RESTRICT Gabs_t,
                                                    const real* LPC_RESTRICT ga, const real* LPC_RESTRICT gb,
                                                    const real2* LPC_RESTRICT phr, const real2* LPC_RESTRICT phc, int Hp,
                                                    int Wc, int cpitch, long cplane, real mu1, real mu2, real mu3,
                                                    real rscale, void* LPC_RESTRICT Cv, real* LPC_RESTRICT RD) {
  const long n = (long)((Hp + 1) & ~1) * cpitch;          // pair-line positions of one plane
  const long pl = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const long pair = e / (2 * cpitch);
    const int w = (int)(e - pair * 2 * cpitch);
    const int i = 2 * (int)pair + ((w >> 3) & 1), j = ((w >> 4) << 3) + (w & 7);
    MidConst mc;
    mc.c1 = mc.c2 = make_real2((real)0., (real)0.);
    real rd = (real)0.;
    if (i < Hp && j < Wc) {
      const real2 hh = Hs_t[pl * cplane + e];
      const real gk = ga ? ga[i] + gb[j] : Gabs_t[e];
      const real2 ph = cmul(phr[i], phc[j]);
      mc.c1 = cmul(make_real2(hh.x, -hh.y), ph);
      mc.c2 = cmul(hh, ph);
      rd = rscale * recip_pos(mu1 * rabs(hh.x * hh.x + hh.y * hh.y) + mu2 * gk + mu3);
    }
    if (REALPH) ((real2*)Cv)[pl * cplane + e] = mc.c1;
    else ((MidConst*)Cv)[pl * cplane + e] = mc;
    RD[pl * cplane + e] = rd;
  }
}
