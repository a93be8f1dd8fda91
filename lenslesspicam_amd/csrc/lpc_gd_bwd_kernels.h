// lpc_gd_bwd_kernels.h -- reverse mode of the unrolled FISTA iterations (lpc_fista_backward): the fused row kernels.
//
// Forward iteration i (unrolled_fista.py:102-106):   gr = D(Cv(y_i) - b);  z = y_i - a_i gr;  xk_i = max(z, 0);
//                                                    y_{i+1} = xk_i + c_i (xk_i - xk_{i-1})
// Reverse iteration i, given gy = dL/dy_{i+1} and the carry (dL/dxk_i through y_{i+2}):
//   HEAD     g_c[i] = sum gy (xk_i - xk_{i-1});  gxk = (1 + c_i) gy + carry;  carry = -c_i gy;  gz = gxk [xk_i > 0];
//            g_a[i,c] = -(1 / a_i[c]) sum gz (y_i - xk_i)          (on the mask y_i - xk_i = a_i gr_i)
//   MIDDLE   Hg = Cv(gz);  g_b += a_i Hg
//   UPDATE   gy = gz - a_i D(Hg)                                   (Cv and D are each other's adjoints: even Hp, Wp only)
// The dataflow is the forward iteration's (two FFT convolutions with the point-wise work inside the row passes), so the
// column passes and spectral middles are the forward's, and the three row kernels have the shape of
// k_rinv_gd_mid[_half] / k_rinv_gd_update_fwd_half: the point-wise work is the source functor of the forward row
// transform's first stage.
//   MODE 0   head of iteration n-1 (gy = dL/dout [y_n > 0], carry = 0)           -> rfft rows (S)
//   MODE 1   rows (S) -> irfft -> shift + crop = Hg -> g_b -> re-pad              -> rfft rows (S2)
//   MODE 2   rows (S2) -> irfft -> shift + crop = D(Hg) -> gy -> head of i-1      -> rfft rows (S);
//            for i = 0 the tail instead: g_init = gy + carry, no transform
//   MODE 3   rows (any spectrum buffer) -> irfft -> shift + crop = v -> acc (+)= -a_i s v, no transform afterwards:
//            the PSF gradient's accumulate (lpc_fista_backward_psf).  Per iteration the sweep hands it two cross terms,
//            v = K(conj(F(P gz_i)) . F(P r_i)) and v = K(conj(F(P y_i)) . F(P Hg_i)); k_gd_bwd_gpsf sums acc over the batch
//            (one PSF per frame: no sum, k_planar_to_hwc lays acc out as (B,1,H,W,C))
// The sums are deterministic: every workgroup (one image row, or one row pair) leaves its two partial sums, accumulated in
// double, in a scratch array; k_gd_bwd_finish adds them up in a fixed order.  No atomics.
#pragma once
#include "lpc_row_kernels.h"

struct GdBwd {
  const real* alpha;   // [C] a_i of the iteration whose rows pass through (MODE 1, 2)
  real* gz;            // [P][H][W] work: gy in (MODE 0: dL/dout, planar) / gz out; MODE 2 reads gz back; tail: g_init out
  real* carry;         // [P][H][W] work
  real* gb;            // [P][H][W] MODE 1: a_i Hg summed over the iterations, or null (no data gradient asked for);
                       // MODE 3: the PSF gradient's accumulator
  const real* xk;      // the head's iteration j: tape slots xk_j, xk_{j-1} (j = 0: y_0) and y_j
  const real* xkp;
  const real* y;
  const real* yn;      // MODE 0: y_n
  double* part;        // the head's partial sums: [P][gridDim.x][2] = (g_c, g_a) terms
  real coef;           // c_j; MODE 3: -s, the PSF spectrum's norm factor negated
  int gb_first;        // MODE 1 of iteration n-1 (MODE 3: the first term of the sweep): gb is written, not added to
  int tail;            // MODE 2 of iteration 0
};

struct GdBwdIn { real v, gz, carry, xk, xkp, y, yn, gb; };
struct GdBwdOut { real ret, gz, carry, gb; };

// one element: `in.v` is the sample the inverse transform produced for it (MODE 1: Hg, MODE 2: D(Hg), MODE 3: a cross
// term); returns what the forward transform takes (out.ret) and what goes back to memory.  `al`: a_i (MODE 3: -s a_i)
template <int MODE>
static __device__ __forceinline__ GdBwdOut gd_bwd_val(const GdBwdIn& in, const GdBwd& a, real al, double& sc, double& sa) {
  GdBwdOut o;
  o.ret = o.gz = o.carry = o.gb = (real)0.;
  if (MODE == 1 || MODE == 3) {
    const real t = al * in.v;
    o.gb = a.gb_first ? t : in.gb + t;
    o.ret = in.v;
    return o;
  }
  real gy, carry = (real)0.;
  if (MODE == 0) {
    gy = in.yn > (real)0. ? in.gz : (real)0.;
  } else {
    gy = in.gz - al * in.v;
    carry = in.carry;
    if (a.tail) { o.gz = gy + carry; return o; }
  }
  sc += (double)gy * (double)(in.xk - in.xkp);
  const real gxk = ((real)1. + a.coef) * gy + carry;
  o.carry = -a.coef * gy;
  o.gz = in.xk > (real)0. ? gxk : (real)0.;
  sa += (double)o.gz * (double)(in.y - in.xk);
  o.ret = o.gz;
  return o;
}

template <int MODE>
static __device__ __forceinline__ real gd_bwd_one(const GdBwd& a, long o, real v, real al, double& sc, double& sa) {
  GdBwdIn in;
  in.v = v;
  in.gz = in.carry = in.xk = in.xkp = in.y = in.yn = in.gb = (real)0.;
  if (MODE == 1 || MODE == 3) {
    if (!a.gb) return v;
    if (!a.gb_first) in.gb = a.gb[o];
  } else {
    in.gz = a.gz[o];
    if (MODE == 0) in.yn = a.yn[o];
    else in.carry = a.carry[o];
    if (MODE == 0 || !a.tail) { in.xk = a.xk[o]; in.xkp = a.xkp[o]; in.y = a.y[o]; }
  }
  const GdBwdOut r = gd_bwd_val<MODE>(in, a, al, sc, sa);
  if (MODE == 1 || MODE == 3) {
    a.gb[o] = r.gb;
  } else {
    a.gz[o] = r.gz;
    if (MODE == 0 || !a.tail) a.carry[o] = r.carry;
  }
  return r.ret;
}

// two neighbouring columns at once (o even: 8-byte accesses, see gd_update_pair)
template <int MODE>
static __device__ __forceinline__ real2 gd_bwd_pair(const GdBwd& a, long o, real2 v, real al, double& sc, double& sa) {
  const real2 z2 = make_real2((real)0., (real)0.);
  real2 gz = z2, carry = z2, xk = z2, xkp = z2, y = z2, yn = z2, gb = z2;
  if (MODE == 1 || MODE == 3) {
    if (!a.gb) return v;
    if (!a.gb_first) gb = *(const real2*)(a.gb + o);
  } else {
    gz = *(const real2*)(a.gz + o);
    if (MODE == 0) yn = *(const real2*)(a.yn + o);
    else carry = *(const real2*)(a.carry + o);
    if (MODE == 0 || !a.tail) {
      xk = *(const real2*)(a.xk + o); xkp = *(const real2*)(a.xkp + o); y = *(const real2*)(a.y + o);
    }
  }
  GdBwdIn i0, i1;
  i0.v = v.x; i0.gz = gz.x; i0.carry = carry.x; i0.xk = xk.x; i0.xkp = xkp.x; i0.y = y.x; i0.yn = yn.x; i0.gb = gb.x;
  i1.v = v.y; i1.gz = gz.y; i1.carry = carry.y; i1.xk = xk.y; i1.xkp = xkp.y; i1.y = y.y; i1.yn = yn.y; i1.gb = gb.y;
  const GdBwdOut r0 = gd_bwd_val<MODE>(i0, a, al, sc, sa), r1 = gd_bwd_val<MODE>(i1, a, al, sc, sa);
  if (MODE == 1 || MODE == 3) {
    *(real2*)(a.gb + o) = make_real2(r0.gb, r1.gb);
  } else {
    *(real2*)(a.gz + o) = make_real2(r0.gz, r1.gz);
    if (MODE == 0 || !a.tail) *(real2*)(a.carry + o) = make_real2(r0.carry, r1.carry);
  }
  return make_real2(r0.ret, r1.ret);
}

// ---- workgroup sum of two doubles in a fixed order: wavefront shuffles, then lane 0 adds the waves (block_minmax) ----
// `red` is the head of the dynamic LDS (gd_bwd_red_bytes), in front of the FFT tile; the result is valid in thread 0
template <int NT>
static __host__ __device__ constexpr size_t gd_bwd_red_bytes() {
#if !defined(LPC_SIMT_EMU)
  return (size_t)(NT / 64 > 0 ? NT / 64 : 1) * 2 * sizeof(double);
#else
  return (size_t)NT * 2 * sizeof(double);
#endif
}
template <int NT>
static __device__ __forceinline__ void gd_bwd_block_sum2(double& a, double& b, double* red, int tid) {
#if !defined(LPC_SIMT_EMU)
  for (int off = 32; off > 0; off >>= 1) {  // 64-lane wavefront
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0) { red[2 * wave] = a; red[2 * wave + 1] = b; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NT / 64; ++w) { a += red[2 * w]; b += red[2 * w + 1]; }
  }
#else
  red[2 * tid] = a; red[2 * tid + 1] = b;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NT; ++w) { a += red[2 * w]; b += red[2 * w + 1]; }
  }
#endif
}

// ---- one real row per half-length transform (k_rinv_gd_mid_half / k_rinv_gd_update_fwd_half are the models) ----------
template <int MODE, int NT, int EMAX, int SK, class PL = Fft1dPlan>
__global__ __launch_bounds__(NT) void k_gd_bwd_half(PlaneGeom g, PL plan, const real2* LPC_RESTRICT twW,
                                                     const real2* LPC_RESTRICT Sin, real2* LPC_RESTRICT Sout,
                                                     GdBwd a) {
  LPC_DYN_SMEM(smem);
  double* red = (double*)smem;
  real2* s = (real2*)(smem + gd_bwd_red_bytes<NT>());
  const int tid = LPC_TID(NT), u = (int)LPC_BX(g);
  const long pl = LPC_BY(g);
  const int hh = g.Hp / 2, hw = g.Wp / 2, M = g.Wp >> 1;
  if (MODE != 0) {
    const int sr = wrap_add(g.sh + u, hh, g.Hp);
    tangle_half_load<NT, EMAX, SK>(s, M, twW, Sin + pl * g.cplane + (long)sr * g.cpitch, tid);
    __syncthreads();
    fft_tile<NT, EMAX, true, SK, true>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, LdsNatural{});
  }
  // slot j now holds samples (2j, 2j+1) of the convolution before the shift; padded sample m of the NEW row =
  // (m in window) ? element [m - sw], which takes convolution sample (m + Wp/2) mod Wp : 0
  const real al = MODE == 3 ? a.coef * a.alpha[pl % g.C] : MODE != 0 ? a.alpha[pl % g.C] : (real)0.;
  const long base = pl * g.uplane + (long)u * g.W;
  const bool pair = ((g.sw | g.W | hw) & 1) == 0;
  double sc = 0., sa = 0.;
  auto sample = [&](int m) {
    const int c = m - g.sw;
    if (c < 0 || c >= g.W) return (real)0.;
    real v = (real)0.;
    if (MODE != 0) {
      const int q = wrap_add(m, hw, g.Wp);
      const real2 z = s[lds_slot<SK>(q >> 1)];
      v = (q & 1) ? z.y : z.x;
    }
    return gd_bwd_one<MODE>(a, base + c, v, al, sc, sa);
  };
  auto newrow = [&](int i, int) {
    if (pair) {
      const int c = 2 * i - g.sw;
      if (c < 0 || c >= g.W) return make_real2((real)0., (real)0.);
      real2 z = make_real2((real)0., (real)0.);
      if (MODE != 0) z = s[lds_slot<SK>(wrap_add(2 * i, hw, g.Wp) >> 1)];
      return gd_bwd_pair<MODE>(a, base + c, z, al, sc, sa);
    }
    return make_real2(sample(2 * i), sample(2 * i + 1));
  };
  if (MODE == 3 || (MODE == 2 && a.tail)) {     // acc / g_init: the elements of the row, nothing to transform
    for (int i = tid; i < M; i += NT) (void)newrow(i, 0);
    return;
  }
  fft_tile<NT, EMAX, false, SK, MODE != 0, true>(s, plan, 1, make_fastdiv_dev1(), tid, newrow, LdsNatural{});
  untangle_half_store<NT, SK>(s, M, twW, Sout + pl * g.cplane + (long)(g.sh + u) * g.cpitch, tid);
  if (MODE != 1) {
    gd_bwd_block_sum2<NT>(sc, sa, red, tid);
    if (tid == 0) {
      double* p = a.part + 2 * (pl * gridDim.x + u);
      p[0] = sc; p[1] = sa;
    }
  }
}

// ---- two real rows per complex transform of length Wp (k_rinv_gd_mid is the model; the radix-2 stage is not folded into
// the Hermitian tangling here: `plan` runs whole in both directions) ----------------------------------------------------
template <int MODE, int NT, int EMAX, int SK>
__global__ __launch_bounds__(NT) void k_gd_bwd_paired(PlaneGeom g, Fft1dPlan plan, const real2* LPC_RESTRICT Sin,
                                                       real2* LPC_RESTRICT Sout, GdBwd a) {
  LPC_DYN_SMEM(smem);
  double* red = (double*)smem;
  real2* s = (real2*)(smem + gd_bwd_red_bytes<NT>());
  const int tid = LPC_TID(NT);
  const int u0 = 2 * blockIdx.x, u1 = u0 + 1;
  const long pl = blockIdx.y;
  const bool v1 = u1 < g.H;
  const int hh = g.Hp / 2, hw = g.Wp / 2;
  if (MODE != 0) {
    const int sr0 = wrap_add(g.sh + u0, hh, g.Hp);
    const int sr1 = wrap_add(g.sh + (v1 ? u1 : u0), hh, g.Hp);
    const real2* sp = Sin + pl * g.cplane;
    tangle_load<NT, EMAX, SK>(s, g.Wp, g.Wc, sp + (long)sr0 * g.cpitch, sp + (long)sr1 * g.cpitch, v1, tid);
    __syncthreads();
    fft_tile<NT, EMAX, true, SK, true>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, LdsNatural{}, NoFix{}, 0, 0);
  }
  const real al = MODE == 3 ? a.coef * a.alpha[pl % g.C] : MODE != 0 ? a.alpha[pl % g.C] : (real)0.;
  const long base = pl * g.uplane + (long)u0 * g.W;
  double sc = 0., sa = 0.;
  auto newrow = [&](int i, int) {
    const int c = i - g.sw;
    if (c < 0 || c >= g.W) return make_real2((real)0., (real)0.);
    real2 z = make_real2((real)0., (real)0.);
    if (MODE != 0) z = s[lds_slot<SK>(wrap_add(i, hw, g.Wp))];
    real2 r;
    r.x = gd_bwd_one<MODE>(a, base + c, z.x, al, sc, sa);
    r.y = v1 ? gd_bwd_one<MODE>(a, base + g.W + c, z.y, al, sc, sa) : (real)0.;
    return r;
  };
  if (MODE == 3 || (MODE == 2 && a.tail)) {
    for (int i = tid; i < g.Wp; i += NT) (void)newrow(i, 0);
    return;
  }
  fft_tile<NT, EMAX, false, SK, MODE != 0, true>(s, plan, 1, make_fastdiv_dev1(), tid, newrow, LdsNatural{}, NoFix{}, 0, 0);
  real2* o = Sout + pl * g.cplane + (long)(g.sh + u0) * g.cpitch;
  untangle_store<NT, SK>(s, g.Wp, g.Wc, o, o + g.cpitch, v1, tid);
  if (MODE != 1) {
    gd_bwd_block_sum2<NT>(sc, sa, red, tid);
    if (tid == 0) {
      double* p = a.part + 2 * (pl * gridDim.x + blockIdx.x);
      p[0] = sc; p[1] = sa;
    }
  }
}

// ---- the finishing sum: block (q, i) adds the partials of iteration i in a fixed order --------------------------------
// q < C: g_alpha[i][q] = -(1 / alpha[i][q]) * sum over the planes of channel q;  q == C: g_coef[i] = sum over all planes
template <int NT>
__global__ __launch_bounds__(NT) void k_gd_bwd_finish(const double* LPC_RESTRICT part, int P, int rows, int C,
                                                       const real* LPC_RESTRICT alpha, real* LPC_RESTRICT g_alpha,
                                                       real* LPC_RESTRICT g_coef) {
  LPC_DYN_SMEM(smem);
  double* red = (double*)smem;
  const int tid = LPC_TID(NT);
  const int q = blockIdx.x, i = blockIdx.y;
  const double* p = part + (long)i * P * rows * 2;
  const long n = (long)P * rows;
  double sum = 0., unused = 0.;
  for (long e = tid; e < n; e += NT) {
    const int pl = (int)(e / rows);
    if (q == C) sum += p[2 * e];
    else if (pl % C == q) sum += p[2 * e + 1];
  }
  gd_bwd_block_sum2<NT>(sum, unused, red, tid);
  if (tid == 0) {
    if (q == C) g_coef[i] = (real)sum;
    else g_alpha[i * C + q] = (real)(-sum / (double)alpha[i * C + q]);
  }
}

// planar (P = B*C planes) data gradient -> (B, H, W, dc); dc == 1 < C: the forward broadcast the measurement, so the
// gradient is the sum over the channels
template <int NT>
__global__ __launch_bounds__(NT) void k_gd_bwd_gdata(const real* LPC_RESTRICT gb, real* LPC_RESTRICT out, long uplane,
                                                      int C, int dc) {
  const long img = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < uplane; e += (long)gridDim.x * NT) {
    const real* p = gb + img * C * uplane + e;
    if (dc == C) {
      for (int c = 0; c < C; ++c) out[(img * uplane + e) * C + c] = p[(long)c * uplane];
    } else {
      real sum = p[0];
      for (int c = 1; c < C; ++c) sum += p[(long)c * uplane];
      out[img * uplane + e] = sum;
    }
  }
}

// planar (P = B*C planes) PSF-gradient accumulator -> (1, H, W, C), the PSF's layout: the sum over the batch in the order
// of the frames
template <int NT>
__global__ __launch_bounds__(NT) void k_gd_bwd_gpsf(const real* LPC_RESTRICT acc, real* LPC_RESTRICT out, long uplane,
                                                     int C, int B) {
  const int c = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < uplane; e += (long)gridDim.x * NT) {
    const real* p = acc + (long)c * uplane + e;
    real sum = p[0];
    for (int b = 1; b < B; ++b) sum += p[(long)b * C * uplane];
    out[e * C + c] = sum;
  }
}
