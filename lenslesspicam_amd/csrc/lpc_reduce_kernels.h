// lpc_reduce_kernels.h -- workgroup reductions (wavefront shuffles, then lane 0 combines the waves) and the set-up
// kernels built on them: per-plane min / max, and the separability check of ADMM's gram plane.
#pragma once
#include "lpc_args.h"

template <int NT>
static __device__ __forceinline__ void block_minmax(real& mx, real& mn, real* scratch, int tid) {
#if !defined(LPC_SIMT_EMU)
  for (int off = 32; off > 0; off >>= 1) {  // 64-lane wavefront
    mx = rmax(mx, __shfl_down(mx, off, 64));
    mn = rmin(mn, __shfl_down(mn, off, 64));
  }
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0) { scratch[2 * wave] = mx; scratch[2 * wave + 1] = mn; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NT / 64; ++w) { mx = rmax(mx, scratch[2 * w]); mn = rmin(mn, scratch[2 * w + 1]); }
  }
#else
  scratch[2 * tid] = mx; scratch[2 * tid + 1] = mn;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NT; ++w) { mx = rmax(mx, scratch[2 * w]); mn = rmin(mn, scratch[2 * w + 1]); }
  }
#endif
}

// mode 0: values are |H* H| of a spectrum plane (pitch cpitch, Wc valid columns);
// mode 1: values are an un-padded image plane.  Writes (max, min) per (plane, block).
template <int NT>
__global__ __launch_bounds__(NT) void k_plane_minmax(PlaneGeom g, const real2* LPC_RESTRICT Hs,
                                                      const real* LPC_RESTRICT plane, int mode,
                                                      real* LPC_RESTRICT partial) {
  LPC_DYN_SMEM(smem);
  real* scratch = (real*)smem;
  const int tid = LPC_TID(NT);
  const long pl = blockIdx.y;
  real mx = -INFINITY, mn = INFINITY;
  if (mode == 0) {
    const long n = (long)g.Hp * g.Wc;
    for (long e = (long)blockIdx.x * NT + tid; e < n; e += (long)gridDim.x * NT) {
      const int r = (int)(e / g.Wc), c = (int)(e - (long)r * g.Wc);
      const real2 h = Hs[pl * g.cplane + (long)r * g.cpitch + c];
      const real a = h.x * h.x + h.y * h.y;
      mx = rmax(mx, a); mn = rmin(mn, a);
    }
  } else {
    const long n = g.uplane;
    for (long e = (long)blockIdx.x * NT + tid; e < n; e += (long)gridDim.x * NT) {
      const real a = plane[pl * g.uplane + e];
      mx = rmax(mx, a); mn = rmin(mn, a);
    }
  }
  block_minmax<NT>(mx, mn, scratch, tid);
  if (tid == 0) {
    partial[2 * (pl * gridDim.x + blockIdx.x)] = mx;
    partial[2 * (pl * gridDim.x + blockIdx.x) + 1] = mn;
  }
}

// ---- is a real spectrum plane G[r][c] the sum of a row term and a column term?  (ADMM set-up, ColPass::ga) -----
// ga[r] = G[r][0], gb[c] = G[0][c] - G[0][0]
static __global__ void k_gsep_extract(const real* LPC_RESTRICT G, int Hp, int Wc, long cpitch, real* LPC_RESTRICT ga,
                                      real* LPC_RESTRICT gb) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < Hp) ga[e] = G[e * cpitch];
  if (e < cpitch) gb[e] = e < Wc ? G[e] - G[0] : (real)0.;
}
// partial[2 b] = max |G - ga - gb|, partial[2 b + 1] = -max |G| over the block's share of the plane
template <int NT>
__global__ __launch_bounds__(NT) void k_gsep_check(const real* LPC_RESTRICT G, int Hp, int Wc, long cpitch,
                                                    const real* LPC_RESTRICT ga, const real* LPC_RESTRICT gb,
                                                    real* LPC_RESTRICT partial) {
  LPC_DYN_SMEM(smem);
  real* scratch = (real*)smem;
  const int tid = LPC_TID(NT);
  real mx = (real)0., mn = (real)0.;
  const long n = (long)Hp * Wc;
  for (long e = (long)blockIdx.x * NT + tid; e < n; e += (long)gridDim.x * NT) {
    const int r = (int)(e / Wc), c = (int)(e - (long)r * Wc);
    const real v = G[(long)r * cpitch + c];
    mx = rmax(mx, rabs(v - (ga[r] + gb[c])));
    mn = rmin(mn, -rabs(v));
  }
  block_minmax<NT>(mx, mn, scratch, tid);
  if (tid == 0) { partial[2 * blockIdx.x] = mx; partial[2 * blockIdx.x + 1] = mn; }
}

template <int NT>
static __device__ __forceinline__ double block_sum(double v, double* scratch, int tid) {
#if !defined(LPC_SIMT_EMU)
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);   // 64-lane wavefront
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < NT / 64; ++w) v += scratch[w];
#else
  scratch[tid] = v;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < NT; ++w) v += scratch[w];
#endif
  return v;
}
