// lpc_row_kernels.h -- the row passes: real rows <-> half-spectrum rows, two rows per complex transform or one row per
// half-length transform, ADMM work arrays and the generic source / sink.  Launched by lpc_rows.cpp and the plan modules
// (lpc_launch.h); the fused rows of the other families build on the (un)tangling here.
#pragma once
#include "lpc_args.h"
// ===================================================================== row passes ==
// Two real rows ride through ONE complex FFT of length Wp (re = row A, im = row B) and are
// separated afterwards by Hermitian symmetry; works for even and odd Wp alike.
// The first FFT stage pulls its inputs straight from global memory (source lambda) and the last
// stage pushes its outputs straight out (sink lambda); LDS only carries the tile between stages
// and the Hermitian (un)tangling, which pairs bins k and Wp-k held by different lanes.

// s[] holds Z = FFT(a + i b) in natural order; writes A[k], B[k] for k in [0, Wc)
// (SL = 1: outA = the pair's base, outB = base + 8, see spec_col; validA: row A exists -- the first pair of a window that
// starts on an odd row holds the row above it, which is not stored)
template <int NT, int SK, int SL = 0>
static __device__ __forceinline__ void untangle_store(const real2* s, int Wp, int Wc, real2* outA,
                                                       real2* outB, bool validB, int tid, bool validA = true) {
  for (int k = tid; k < Wc; k += NT) {
    real2 zk = s[lds_slot<SK>(k)];
    real2 zn = s[lds_slot<SK>(k == 0 ? 0 : Wp - k)];
    if (validA) outA[spec_col<SL>(k)] = make_real2((real)0.5 * (zk.x + zn.x), (real)0.5 * (zk.y - zn.y));
    if (validB) outB[spec_col<SL>(k)] = make_real2((real)0.5 * (zk.y + zn.y), -(real)0.5 * (zk.x - zn.x));
  }
}

// builds Z[k] = A[k] + i B[k] over the full length from two half spectra (irfft semantics:
// imaginary parts of the DC and Nyquist bins are ignored).  All loads are issued before the
// first LDS write (unrolled to the compile-time bound) so they overlap in flight.
template <int NT, int EMAX, int SK, int SL = 0>
static __device__ __forceinline__ void tangle_load(real2* s, int Wp, int Wc, const real2* inA,
                                                    const real2* inB, bool validB, int tid, bool validA = true) {
  constexpr int EH = EMAX / 2 + 1;
  if constexpr (SL == 1) {
    // pair lines: bins k, k + 1 (k even) of one row are 16 adjacent, 16-byte-aligned bytes: ONE load per row and lane instead
    // of two (C4's inverse rows 0.276 -> 0.268 ms, same box, two trees; the same for the stores of the forward rows bought
    // nothing).  The load of a row's last pair may reach bin Wc in the padding of the row pitch -- never used.
    constexpr int EP = (EH + 1) / 2;
    real4 a4[EP], b4[EP];
    const real4 z4 = make_real4((real)0., (real)0., (real)0., (real)0.);
#pragma unroll
    for (int q = 0; q < EP; ++q) {
      const int k = 2 * (tid + q * NT);
      a4[q] = b4[q] = z4;
      if (k < Wc) {
        if (validA) a4[q] = ld4((const real*)(inA + spec_col<SL>(k)));
        if (validB) b4[q] = ld4((const real*)(inB + spec_col<SL>(k)));
      }
    }
#pragma unroll
    for (int q = 0; q < EP; ++q) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int k = 2 * (tid + q * NT) + u;
        if (k < Wc) {
          real2 av = u ? make_real2(a4[q].z, a4[q].w) : make_real2(a4[q].x, a4[q].y);
          real2 bv = u ? make_real2(b4[q].z, b4[q].w) : make_real2(b4[q].x, b4[q].y);
          const bool selfconj = (k == 0) || (2 * k == Wp);
          if (selfconj) { av.y = (real)0.; bv.y = (real)0.; }
          s[lds_slot<SK>(k)] = make_real2(av.x - bv.y, av.y + bv.x);
          if (!selfconj) s[lds_slot<SK>(Wp - k)] = make_real2(av.x + bv.y, bv.x - av.y);
        }
      }
    }
    return;
  }
  real2 a[EH], b[EH];
#pragma unroll
  for (int q = 0; q < EH; ++q) {
    const int k = tid + q * NT;
    a[q] = make_real2((real)0., (real)0.);
    b[q] = make_real2((real)0., (real)0.);
    if (k < Wc) {
      if (validA) a[q] = inA[spec_col<SL>(k)];
      if (validB) b[q] = inB[spec_col<SL>(k)];
    }
  }
#pragma unroll
  for (int q = 0; q < EH; ++q) {
    const int k = tid + q * NT;
    if (k < Wc) {
      real2 av = a[q], bv = b[q];
      const bool selfconj = (k == 0) || (2 * k == Wp);
      if (selfconj) { av.y = (real)0.; bv.y = (real)0.; }
      s[lds_slot<SK>(k)] = make_real2(av.x - bv.y, av.y + bv.x);
      if (!selfconj) s[lds_slot<SK>(Wp - k)] = make_real2(av.x + bv.y, bv.x - av.y);
    }
  }
}

// Radix-2 stage folded into the Hermitian (un)tangling (row lengths whose plan ends in a radix-2 stage,
// e.g. 8192 = 8*8*8*8*2).  With nb = Wp/2, the lane that owns butterflies j and nb-j of that stage holds
// Z[j], Z[nb+j], Z[nb-j], Z[Wp-j] -- exactly what the (un)tangling of bins j and nb-j needs -- so the stage
// never makes its own trip through LDS.
//
// forward: s[] holds the tile BEFORE the last (radix-2, ns = nb) stage; writes A[k], B[k], k in [0, nb]
template <int NT, int SK>
static __device__ __forceinline__ void untangle_r2_store(const real2* s, int Wp, const real2* LPC_RESTRICT tw,
                                                          real2* outA, real2* outB, bool validB, int tid) {
  const int nb = Wp >> 1;
  auto emit = [&](int k, real2 zk, real2 zn) {     // zk = Z[k], zn = Z[Wp - k]
    outA[k] = make_real2((real)0.5 * (zk.x + zn.x), (real)0.5 * (zk.y - zn.y));
    if (validB) outB[k] = make_real2((real)0.5 * (zk.y + zn.y), (real)-0.5 * (zk.x - zn.x));
  };
  for (int j = tid; j <= nb / 2; j += NT) {
    const int jm = nb - j;                          // mirror butterfly (== nb for j == 0: no such butterfly)
    const real2 u0 = s[lds_slot<SK>(j)];
    const real2 v0 = j ? cmul(s[lds_slot<SK>(j + nb)], tw[j]) : s[lds_slot<SK>(nb)];
    const real2 zj = cadd(u0, v0), zjn = csub(u0, v0);            // Z[j], Z[j + nb]
    if (j == 0) {
      emit(0, zj, zj);                                           // DC pairs with itself
      emit(nb, zjn, zjn);                                        // so does the Nyquist bin
    } else if (j == jm) {
      emit(j, zj, zjn);                                          // Wp - j == j + nb
    } else {
      const real2 u1 = s[lds_slot<SK>(jm)];
      const real2 v1 = cmul(s[lds_slot<SK>(jm + nb)], tw[jm]);
      const real2 zm = cadd(u1, v1), zmn = csub(u1, v1);         // Z[nb - j], Z[Wp - j]
      emit(j, zj, zmn);
      emit(jm, zm, zjn);                                         // Wp - (nb - j) == nb + j
    }
  }
}

// inverse: builds Z from the half spectra and applies the FIRST (radix-2, ns = 1, twiddle-free) stage of the
// inverse plan: writes y[2j] = Z[j] + Z[j+nb], y[2j+1] = Z[j] - Z[j+nb] into the (un-skewed) LDS tile.
// Every spectrum element is loaded exactly once.
template <int NT>
static __device__ __forceinline__ void tangle_r2_load(real2* s, int Wp, const real2* inA, const real2* inB,
                                                       bool validB, int tid) {
  const int nb = Wp >> 1;
  const real2 zero = make_real2((real)0, (real)0);
  for (int j = tid; j <= nb / 2; j += NT) {
    const int jm = nb - j;
    real2 a0 = inA[j], b0 = validB ? inB[j] : zero;
    real2 a1 = inA[jm], b1 = validB ? inB[jm] : zero;               // j == 0: the Nyquist bin
    if (j == 0) { a0.y = (real)0; b0.y = (real)0; a1.y = (real)0; b1.y = (real)0; }
    // Z[k] = A[k] + i B[k];  Z[Wp - k] = conj(A[k]) + i conj(B[k])
    const real2 zj = make_real2(a0.x - b0.y, a0.y + b0.x);          // Z[j]
    const real2 zm = make_real2(a1.x - b1.y, a1.y + b1.x);          // Z[nb - j]   (j == 0: Z[nb])
    const real2 zjn = make_real2(a1.x + b1.y, b1.x - a1.y);         // Z[j + nb]  = mirror of bin nb - j
    const real2 zmn = make_real2(a0.x + b0.y, b0.x - a0.y);         // Z[Wp - j]  = mirror of bin j
    if (j == 0) {
      s[0] = cadd(zj, zm);
      s[1] = csub(zj, zm);
    } else {
      s[2 * j] = cadd(zj, zjn);
      s[2 * j + 1] = csub(zj, zjn);
      if (j != jm) {
        s[2 * jm] = cadd(zm, zmn);
        s[2 * jm + 1] = csub(zm, zmn);
      }
    }
  }
}

// which rows block bx of a paired launch transforms (PairedRows, lpc_args.h)
static __device__ __forceinline__ PairedRows paired_rows_of(const PlaneGeom& g, unsigned bx, bool window_b) {
  const int nB = window_b ? paired_rows_window(g) : (g.Hp + 1) >> 1;
  PairedRows r;
  int idx;
  if ((int)bx < 2 * nB) { r.arr = (int)((bx ^ (bx >> 3)) & 1u); idx = (int)(bx >> 1); }
  else { r.arr = 0; idx = (int)bx - nB; }
  r.first = true;
  if (r.arr == 1 && window_b) {
    r.r0 = (g.slay ? g.sh & ~1 : g.sh) + 2 * idx;
    r.first = r.r0 >= g.sh;
    r.second = r.r0 + 1 < g.sh + g.H;
  }
  else { r.r0 = 2 * idx; r.second = r.r0 + 1 < g.Hp; }
  return r;
}

// ---- forward, ADMM: rows (r, r + 1) of array A -> SA, of array B -> SB ------------
template <int NT, int EMAX, int SK, bool R2, class PL = Fft1dPlan, int SL = 0>
__global__ __launch_bounds__(NT) void k_rfwd_arrays(PlaneGeom g, PL plan,
                                                     const real* LPC_RESTRICT A,
                                                     const real* LPC_RESTRICT B,
                                                     real2* LPC_RESTRICT SA,
                                                     real2* LPC_RESTRICT SB) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT);
  const long pl = blockIdx.y;
  const PairedRows pr = paired_rows_of(g, blockIdx.x, false);
  const real* a = (pr.arr ? B : A) + pl * g.rplane + (long)pr.r0 * g.rpitch;
  const real* b = a + g.rpitch;
  const bool v1 = pr.second;
  auto src = [&](int i, int) { return make_real2(a[i], v1 ? b[i] : (real)0.); };
  if constexpr (is_static_plan<PL>::value)     // compile-time plans: no radix-2 folding (R2 == false)
    fft_tile<NT, EMAX, false, SK, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, src, LdsNatural{});
  else
    fft_tile<NT, EMAX, false, SK, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, src, LdsNatural{}, NoFix{}, 0,
                                               R2 ? 1 : 0);
  real2* oa = (pr.arr ? SB : SA) + pl * g.cplane + (long)pr.r0 * g.cpitch;
  real2* ob = oa + (SL ? 8 : g.cpitch);
  static_assert(!(R2 && SL), "pair-line spectra: compile-time plans only");
  if (R2) untangle_r2_store<NT, SK>(s, g.Wp, plan.tw, oa, ob, v1, tid);
  else untangle_store<NT, SK, SL>(s, g.Wp, g.Wc, oa, ob, v1, tid);
}

// ---- ADMM rows, one real row per HALF-length complex transform ---------------------------------------
// Even / odd packing: z[j] = x[2j] + i x[2j+1], Z = FFT_M(z), M = Wp/2, then
//   X[k] = E + w^k O,  X[M-k] = conj(E - w^k O),   E = (Z[k] + conj Z[M-k])/2,  O = -i (Z[k] - conj Z[M-k])/2,
// w = exp(-2 pi i / Wp).  Same arithmetic per row as pairing two arrays in one length-Wp transform, but the tile
// is half as large (4 workgroups of 256 threads per CU instead of 2 of 512 at Wp = 8192): measured on MI355X the
// row passes are bound by compute that two workgroups per CU cannot hide (profiles/r01b_notes.md).
// blockIdx.x = 2*row + array.  `plan` has length M, `twW` is the length-Wp table.  Needs Wp even.
// s[] holds Z = FFT_M(z) in natural order; writes X[0 .. M] (M = Wp/2) to o
template <int NT, int SK>
static __device__ __forceinline__ void untangle_half_store(const real2* s, int M, const real2* LPC_RESTRICT twW,
                                                            real2* LPC_RESTRICT o, int tid) {
  for (int k = tid; k <= M / 2; k += NT) {
    const int km = M - k;
    const real2 zk = s[lds_slot<SK>(k)];
    const real2 zm = s[lds_slot<SK>(k == 0 ? 0 : km)];
    const real ex = (real)0.5 * (zk.x + zm.x), ey = (real)0.5 * (zk.y - zm.y);
    const real2 od = make_real2((real)0.5 * (zk.y + zm.y), (real)-0.5 * (zk.x - zm.x));   // O
    const real2 wo = cmul(twW[k], od);
    o[k] = make_real2(ex + wo.x, ey + wo.y);
    if (k != km) o[km] = make_real2(ex - wo.x, wo.y - ey);
  }
}

template <int NT, int EMAX, int SK, class PL = Fft1dPlan>
__global__ __launch_bounds__(NT) void k_rfwd_half(PlaneGeom g, PL plan, const real2* LPC_RESTRICT twW,
                                                   const real* LPC_RESTRICT A, const real* LPC_RESTRICT B,
                                                   real2* LPC_RESTRICT SA, real2* LPC_RESTRICT SB) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT), row = blockIdx.x >> 1, arr = blockIdx.x & 1;
  const long pl = blockIdx.y;
  const real2* a2 = (const real2*)((arr ? B : A) + pl * g.rplane + (long)row * g.rpitch);
  auto src = [&](int i, int) { return a2[i]; };
  fft_tile<NT, EMAX, false, SK, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, src, LdsNatural{});
  untangle_half_store<NT, SK>(s, g.Wp >> 1, twW, (arr ? SB : SA) + pl * g.cplane + (long)row * g.cpitch, tid);
}

// inverse: Z[k] = E' + i O',  Z[M-k] = conj(E') + i conj(O'),  E' = X[k] + conj X[M-k],
// O' = (X[k] - conj X[M-k]) conj(w^k); the unnormalised inverse FFT_M of Z is (x[2j], x[2j+1]).
// irfft semantics: the imaginary parts of the DC and Nyquist bins are ignored.
// builds Z (natural order, length M) in LDS from one half-spectrum row; ends WITHOUT a barrier
template <int NT, int EMAX, int SK>
static __device__ __forceinline__ void tangle_half_load(real2* s, int M, const real2* LPC_RESTRICT twW,
                                                         const real2* LPC_RESTRICT in, int tid) {
  constexpr int EH = EMAX / 2 + 1;
  real2 xk[EH], xm[EH];
#pragma unroll
  for (int q = 0; q < EH; ++q) {          // every spectrum element is loaded once; all loads before the LDS writes
    const int k = tid + q * NT;
    xk[q] = make_real2((real)0., (real)0.);
    xm[q] = xk[q];
    if (k <= M / 2) { xk[q] = in[k]; xm[q] = in[M - k]; }
  }
#pragma unroll
  for (int q = 0; q < EH; ++q) {
    const int k = tid + q * NT;
    if (k <= M / 2) {
      real2 a = xk[q], b = xm[q];
      if (k == 0) { a.y = (real)0.; b.y = (real)0.; }
      const real2 e = make_real2(a.x + b.x, a.y - b.y);            // E'
      const real2 d = make_real2(a.x - b.x, a.y + b.y);            // X[k] - conj X[M-k]
      const real2 od = cmul_conj(d, twW[k]);                       // O'
      s[lds_slot<SK>(k)] = make_real2(e.x - od.y, e.y + od.x);
      if (k != 0 && k != M - k) s[lds_slot<SK>(M - k)] = make_real2(e.x + od.y, od.x - e.y);
    }
  }
}

template <int NT, int EMAX, int SK, class PL = Fft1dPlan>
__global__ __launch_bounds__(NT) void k_rinv_half(PlaneGeom g, PL plan, const real2* LPC_RESTRICT twW,
                                                   const real2* LPC_RESTRICT SA, const real2* LPC_RESTRICT SB,
                                                   real* LPC_RESTRICT A, real* LPC_RESTRICT B, int skip_b_outside) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  // block b runs on XCD b % 8: the array flips every fourth row so that each XCD transforms rows of both (the rows of
  // B outside the sensor window may be skipped: with `arr = b & 1` only the odd XCDs would have less to do: 0.49 -> 0.47 ms, r02ak)
  const int tid = LPC_TID(NT);
  const unsigned bx = LPC_BX(g);
  int row = bx >> 1, arr = (bx ^ (bx >> 3)) & 1;
  const long pl = LPC_BY(g);
  // AdmmScalars::skiphv: grid.x = 2 H + (Hp - H) -- both arrays on the rows of the sensor window, then A (= V) alone on
  // the rows above and below it (no empty workgroups: each would still claim its LDS and a launch slot)
  // skip_b_outside == 2 (LaunchPlan::hv_fuse): grid.x = Hp, A alone -- the rows of B stay in the spectrum (k_hv_rows_v2)
  if (skip_b_outside == 2) {
    row = (int)bx;
    arr = 0;
  } else if (skip_b_outside) {
    if ((int)bx < 2 * g.H) row += g.sh;
    else {
      const int q = (int)bx - 2 * g.H;
      row = q < g.sh ? q : q + g.H;
      arr = 0;
    }
  }
  tangle_half_load<NT, EMAX, SK>(s, g.Wp >> 1, twW, (arr ? SB : SA) + pl * g.cplane + (long)row * g.cpitch, tid);
  __syncthreads();
  real2* o2 = (real2*)((arr ? B : A) + pl * g.rplane + (long)row * g.rpitch);
  auto out = [&](int i, int, real2 v) { o2[i] = v; };
  fft_tile<NT, EMAX, true, SK, true, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, out);
}

// ---- forward, generic: rows (2b, 2b+1) of ONE real source -> spectrum rows ------------
template <int NT, int EMAX, int SK, bool R2>
__global__ __launch_bounds__(NT) void k_rfwd_rows(PlaneGeom g, Fft1dPlan plan, RealSrc src,
                                                   real2* LPC_RESTRICT S) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT);
  const int r0 = 2 * blockIdx.x, r1 = r0 + 1;
  const long pl = blockIdx.y;
  const bool v1 = r1 < src.nrows;
  const real* a = src.base + pl * src.plane_stride + (long)r0 * src.pitch;
  const real* b = src.base + pl * src.plane_stride + (long)r1 * src.pitch;
  auto in = [&](int i, int) {   // pad on load
    const int c = i - src.col0;
    const bool ok = (c >= 0) && (c < src.ncols);
    return make_real2(ok ? a[c] : (real)0., (ok && v1) ? b[c] : (real)0.);
  };
  fft_tile<NT, EMAX, false, SK, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, in, LdsNatural{}, NoFix{}, 0,
                                             R2 ? 1 : 0);
  real2* o = S + pl * g.cplane + (long)(src.out_row0 + r0) * g.cpitch;
  if (R2) untangle_r2_store<NT, SK>(s, g.Wp, plan.tw, o, o + g.cpitch, v1, tid);
  else untangle_store<NT, SK>(s, g.Wp, g.Wc, o, o + g.cpitch, v1, tid);
}

// one real row per half-length transform (see k_rfwd_half), generic source with pad on load
template <int NT, int EMAX, int SK, class PL = Fft1dPlan>
__global__ __launch_bounds__(NT) void k_rfwd_rows_half(PlaneGeom g, PL plan, const real2* LPC_RESTRICT twW,
                                                        RealSrc src, real2* LPC_RESTRICT S) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT), r = blockIdx.x;
  const long pl = blockIdx.y;
  const real* a = src.base + pl * src.plane_stride + (long)r * src.pitch;
  auto in = [&](int i, int) {   // z[i] = (x[2i], x[2i+1]), x zero outside [col0, col0 + ncols)
    const int c = 2 * i - src.col0;
    return make_real2((c >= 0 && c < src.ncols) ? a[c] : (real)0.,
                      (c + 1 >= 0 && c + 1 < src.ncols) ? a[c + 1] : (real)0.);
  };
  fft_tile<NT, EMAX, false, SK, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, in, LdsNatural{});
  untangle_half_store<NT, SK>(s, g.Wp >> 1, twW, S + pl * g.cplane + (long)(src.out_row0 + r) * g.cpitch, tid);
}

// ---- inverse, ADMM: spectra SA, SB -> real arrays A, B (no shift, padded), two rows of one array per transform -------
// R2: `plan` is the inverse-row plan whose FIRST stage is the radix-2 one (fused into the tangling); SK is
// false in that case (the skew is not affine for ns = 2).
// window_only (AdmmScalars::skiphv): B (= H V) is produced on the rows of the sensor window alone (paired_rows_of).
template <int NT, int EMAX, int SK, bool R2, class PL = Fft1dPlan, int SL = 0>
__global__ __launch_bounds__(NT) void k_rinv_arrays(PlaneGeom g, PL plan,
                                                     const real2* LPC_RESTRICT SA,
                                                     const real2* LPC_RESTRICT SB,
                                                     real* LPC_RESTRICT A, real* LPC_RESTRICT B, int window_only) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT);
  LPC_STAMP_BEGIN(3);
  const long pl = LPC_BY(g);
  const PairedRows pr = paired_rows_of(g, LPC_BX(g), window_only != 0);
  const bool va = pr.first, vb = pr.second;
  const real2* ia = (pr.arr ? SB : SA) + pl * g.cplane + (long)pr.r0 * g.cpitch;
  const real2* ib = ia + (SL ? 8 : g.cpitch);
  static_assert(!(R2 && SL), "pair-line spectra: compile-time plans only");
  if (R2) tangle_r2_load<NT>(s, g.Wp, ia, ib, vb, tid);
  else tangle_load<NT, EMAX, SK, SL>(s, g.Wp, g.Wc, ia, ib, vb, tid, va);
  __syncthreads();
  real* a = (pr.arr ? B : A) + pl * g.rplane + (long)pr.r0 * g.rpitch;
  real* b = a + g.rpitch;
  auto out = [&](int i, int, real2 v) { if (va) a[i] = v.x; if (vb) b[i] = v.y; };
  if constexpr (is_static_plan<PL>::value)
    fft_tile<NT, EMAX, true, SK, true, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, out);
  else
    fft_tile<NT, EMAX, true, SK, true, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, out, NoFix{},
                                                    R2 ? 1 : 0, 0);
  LPC_STAMP_END();
}

// ---- inverse, generic: spectrum rows -> ONE real sink with ifftshift (+ crop) -----------
// Output row i of the shifted frame comes from spectrum row (i + Hp/2) mod Hp and output
// column c from FFT sample (c + Wp/2) mod Wp (fft.ifftshift is a roll by -(n//2)).  That is pure
// index arithmetic in the sink of the last FFT stage: exact, and no extra pass over HBM.
// FFT sample i of a row lands in output column (i - Wp/2 - col0) mod Wp (if < ncols)
static __device__ __forceinline__ int shifted_col(int i, int hw, int col0, int Wp) {
  int c = i - hw - col0;
  if (c < 0) c += Wp;
  if (c < 0) c += Wp;
  return c;
}

template <int NT, int EMAX, int SK, bool R2>
__global__ __launch_bounds__(NT) void k_rinv_rows(PlaneGeom g, Fft1dPlan plan,
                                                   const real2* LPC_RESTRICT S, RealDst dst) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT);
  const int r0 = 2 * blockIdx.x, r1 = r0 + 1;
  const long pl = blockIdx.y;
  const bool v1 = r1 < dst.nrows;
  const int hh = g.Hp / 2, hw = g.Wp / 2;
  const int sr0 = wrap_add(dst.row0 + r0, hh, g.Hp);
  const int sr1 = wrap_add(dst.row0 + (v1 ? r1 : r0), hh, g.Hp);
  if (R2) tangle_r2_load<NT>(s, g.Wp, S + pl * g.cplane + (long)sr0 * g.cpitch,
                             S + pl * g.cplane + (long)sr1 * g.cpitch, v1, tid);
  else tangle_load<NT, EMAX, SK>(s, g.Wp, g.Wc, S + pl * g.cplane + (long)sr0 * g.cpitch,
                                 S + pl * g.cplane + (long)sr1 * g.cpitch, v1, tid);
  __syncthreads();
  real* a = dst.base + pl * dst.plane_stride + (long)r0 * dst.pitch;
  real* b = dst.base + pl * dst.plane_stride + (long)r1 * dst.pitch;
  auto out = [&](int i, int, real2 v) {
    const int c = shifted_col(i, hw, dst.col0, g.Wp);
    if (c < dst.ncols) {
      a[c] = v.x;
      if (v1) b[c] = v.y;
    }
  };
  fft_tile<NT, EMAX, true, SK, true, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, out, NoFix{},
                                                  R2 ? 1 : 0, 0);
}

// one real row per half-length transform, generic sink with ifftshift (+ crop)
template <int NT, int EMAX, int SK, class PL = Fft1dPlan>
__global__ __launch_bounds__(NT) void k_rinv_rows_half(PlaneGeom g, PL plan, const real2* LPC_RESTRICT twW,
                                                        const real2* LPC_RESTRICT S, RealDst dst) {
  LPC_DYN_SMEM(smem);
  real2* s = (real2*)smem;
  const int tid = LPC_TID(NT), r = blockIdx.x;
  const long pl = blockIdx.y;
  const int hh = g.Hp / 2, hw = g.Wp / 2;
  const int sr = wrap_add(dst.row0 + r, hh, g.Hp);
  tangle_half_load<NT, EMAX, SK>(s, g.Wp >> 1, twW, S + pl * g.cplane + (long)sr * g.cpitch, tid);
  __syncthreads();
  real* a = dst.base + pl * dst.plane_stride + (long)r * dst.pitch;
  auto out = [&](int i, int, real2 v) {     // samples 2i and 2i+1 of the row
    const int c0 = shifted_col(2 * i, hw, dst.col0, g.Wp);
    if (c0 < dst.ncols) a[c0] = v.x;
    const int c1 = shifted_col(2 * i + 1, hw, dst.col0, g.Wp);
    if (c1 < dst.ncols) a[c1] = v.y;
  };
  fft_tile<NT, EMAX, true, SK, true, false, true>(s, plan, 1, make_fastdiv_dev1(), tid, LdsNatural{}, out);
}
