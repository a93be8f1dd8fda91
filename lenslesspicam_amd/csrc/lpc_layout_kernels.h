// lpc_layout_kernels.h -- layout / set-up kernels: channels-last <-> planar, clamp, |.|, row permutation, pair lines,
// scale, fill.  Launched by lpc_setup.cpp and lpc_admm.cpp.
#pragma once
#include "lpc_args.h"
// ========================================================= layout / setup kernels ==
// channels-last (n, rows, cols, C) <-> planar (n*C planes)[rows][pitch]
// Csrc: channels of the source, C or 1 (a one-channel source is broadcast over the C planes, the way the
// reference's `vpad[...] = v` / `rfft2(x) * H` broadcast a grayscale input against an RGB PSF)
template <int NT>
__global__ __launch_bounds__(NT) void k_hwc_to_planar(const real* LPC_RESTRICT src, real* LPC_RESTRICT dst,
                                                       int rows, int cols, int C, int pitch, long dplane, int Csrc) {
  const long n = (long)rows * cols * C;
  const long nsrc = (long)rows * cols * Csrc;
  const long img = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int c = (int)(e % C);
    const long rc = e / C;
    const int col = (int)(rc % cols);
    const int row = (int)(rc / cols);
    dst[(img * C + c) * dplane + (long)row * pitch + col] = src[img * nsrc + (Csrc == C ? e : rc)];
  }
}

// planar -> channels-last with optional crop window and clamp (>= 0).  clamp_src: also write
// the clamped value back into the planar source (the reference's ADMM._form_image clamps
// its state IN PLACE, admm.py:331-338).
template <int NT>
__global__ __launch_bounds__(NT) void k_planar_to_hwc(real* LPC_RESTRICT src, real* LPC_RESTRICT dst,
                                                       int rows, int cols, int C, int pitch, long splane,
                                                       int row0, int col0, int clamp, int clamp_src, int wr0, int wr1,
                                                       int wc0, int wc1) {
  const long n = (long)rows * cols * C;
  const long img = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int c = (int)(e % C);
    const long rc = e / C;
    const int col = (int)(rc % cols);
    const int row = (int)(rc / cols);
    const long so = (img * C + c) * splane + (long)(row0 + row) * pitch + (col0 + col);
    real v = src[so];
    if (clamp && v < (real)0. && row >= wr0 && row < wr1 && col >= wc0 && col < wc1) {   // [wr0,wr1) x [wc0,wc1): where
      v = (real)0.;
      if (clamp_src) src[so] = (real)0.;
    }
    dst[img * n + e] = v;
  }
}

// the in-place clamp of ADMM._form_image on the sensor window (plug-and-play ADMM keeps its image estimate in one
// explicit array; also applied to the stored initial estimate, see lpc_form_image)
template <int NT>
__global__ __launch_bounds__(NT) void k_clamp_window_inplace(PlaneGeom g, real* x) {
  const long n = (long)g.H * g.W;
  const long pl = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int r = (int)(e / g.W), c = (int)(e - (long)r * g.W);
    const long o = pl * g.rplane + (long)(g.sh + r) * g.rpitch + (g.sw + c);
    if (x[o] < (real)0.) x[o] = (real)0.;
  }
}

// |G| of the TV gram spectrum (admm.py:188 takes torch.abs of it), one plane
template <int NT>
__global__ __launch_bounds__(NT) void k_abs_complex(const real2* LPC_RESTRICT Gs, real* LPC_RESTRICT out, long n) {
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const real2 gg = Gs[e];
    out[e] = rsqrt_of(gg.x * gg.x + gg.y * gg.y);
  }
}

// a real spectrum plane in natural row order [Hp][Wc] -> the engine's stored (four-step) row order [Hp][cpitch]:
// stored row p = k1*N2 + k2 holds frequency k1 + N1*k2
template <int NT>
__global__ __launch_bounds__(NT) void k_permute_spectrum_rows(const real* LPC_RESTRICT nat, real* LPC_RESTRICT out,
                                                               int Hp, int Wc, int cpitch, int N1, int N2) {
  const long n = (long)Hp * Wc;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int prow = (int)(e / Wc), c = (int)(e - (long)prow * Wc);
    const int k = (prow / N2) + N1 * (prow % N2);
    out[(long)prow * cpitch + c] = nat[(long)k * Wc + c];
  }
}

// spectrum planes [Hp][cpitch] -> the pair-line layout (spec_col): the copies of H and |G| an 8-column fused middle reads
template <int NT, class Tp>
__global__ __launch_bounds__(NT) void k_to_pair_lines(const Tp* LPC_RESTRICT src, Tp* LPC_RESTRICT dst, int Hp, int cpitch,
                                                       long cplane) {
  const long n = (long)Hp * cpitch;
  const long pl = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int i = (int)(e / cpitch), j = (int)(e - (long)i * cpitch);
    dst[pl * cplane + (long)(i >> 1) * 2 * cpitch + spec_col<1>(j) + (i & 1) * 8] = src[pl * cplane + e];
  }
}

// return_fft=True (rfft_convolve.py:148-150,193-195): the engine's work spectrum (planar, permuted row order: stored row
// p = k1*N2 + k2 holds frequency k1 + N1*k2) times H or conj(H) -> the reference's layout (img, Hp, Wc, C) complex,
// natural frequency order, channels last.  grid = (blocks over Hp*Wc*C, images).
template <int NT>
__global__ __launch_bounds__(NT) void k_spectrum_mul_to_hwc(PlaneGeom g, const real2* LPC_RESTRICT S,
                                                             const real2* LPC_RESTRICT Hs, int conjH,
                                                             real2* LPC_RESTRICT out, int N1, int N2) {
  const long n = (long)g.Hp * g.Wc * g.C;
  const long img = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int c = (int)(e % g.C);
    const long kk = e / g.C;
    const int kc = (int)(kk % g.Wc), kr = (int)(kk / g.Wc);
    const int p = (kr % N1) * N2 + kr / N1;
    const long q = img * g.C + c;
    const long off = (long)p * g.cpitch + kc;
    const real2 v = S[q * g.cplane + off], h = Hs[(q % g.PM) * g.cplane + off];
    out[img * n + e] = conjH ? cmul_conj(v, h) : cmul(v, h);
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_scale_complex(real2* LPC_RESTRICT S, long n, real sc) {
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    S[e] = cscale(S[e], sc);
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_fill(real* LPC_RESTRICT p, long n, real v) {
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) p[e] = v;
}

// two planar arrays (component 0 / 1) -> channels-last with a trailing axis of 2
template <int NT>
__global__ __launch_bounds__(NT) void k_planar2_to_hwc2(const real* LPC_RESTRICT a0, const real* LPC_RESTRICT a1,
                                                         real* LPC_RESTRICT dst, int rows, int cols, int C,
                                                         int pitch, long splane) {
  const long n = (long)rows * cols * C;
  const long img = blockIdx.y;
  for (long e = (long)blockIdx.x * NT + threadIdx.x; e < n; e += (long)gridDim.x * NT) {
    const int c = (int)(e % C);
    const long rc = e / C;
    const int col = (int)(rc % cols);
    const int row = (int)(rc / cols);
    const long so = (img * C + c) * splane + (long)row * pitch + col;
    dst[(img * n + e) * 2 + 0] = a0[so];
    dst[(img * n + e) * 2 + 1] = a1[so];
  }
}
