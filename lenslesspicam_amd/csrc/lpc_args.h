// lpc_args.h -- what crosses from the host to the kernels of the MI355X deconvolution engine: the frame geometry and the
// argument structs of the kernel families (their comments are the documentation of the kernels' flags), plus the few
// helpers more than one family uses.  No kernel is defined here: the host-only units see this header and no kernel body.
//
// Memory layout in HBM (every element is `real`: float in liblpc.so, double in liblpc_f64.so):
//   * images are PLANAR: plane q = (b*D + d)*C + c, rows contiguous.  The reference keeps
//     channels innermost (stride-3 FFTs); planar turns B, D and C into one batch index.
//   * padded real plane:   [Hp][rpitch]  (rpitch >= Wp)
//   * half spectrum plane: [Hp][cpitch]  real2 (cpitch >= Wc = Wp/2+1, 16-element padded so
//     every tile row is a whole number of 128-byte lines)
//   * un-padded plane:     [H][W]
// Column (H-axis) transforms longer than LDS allows are split four-step style,
// Hp = N1*N2: pass A = length-N1 FFTs over rows {n1*N2 + n2} (+ twiddle), pass B =
// length-N2 FFTs over the contiguous row block {k1*N2 + n2}.  Frequencies therefore stay
// in a PERMUTED row order (row k1*N2+k2 holds frequency k1 + N1*k2); every spectral
// constant (H, |PsiT Psi|, phase tables) is generated in the same order, so no transpose
// or reordering pass ever touches HBM.
#pragma once
#include "lpc_sfft.h"

struct PlaneGeom {
  int H, W;        // un-padded spatial size
  int Hp, Wp, Wc;  // padded rows / cols, half-spectrum cols
  int sh, sw;      // origin of the sensor window inside the padded frame
  int rpitch;      // floats per padded real row
  int cpitch;      // real2 per spectrum row
  long rplane;     // floats per padded real plane
  long cplane;     // real2 per spectrum plane
  long uplane;     // floats per un-padded plane
  int DC;          // D*C: planes of one frame
  int C;           // channels (data plane of state plane q = (q / DC) * C + q % C)
  int rev;         // per launch (the launcher sets it on its copy): the row kernels that honour it hand their workgroups
                   // out from the last (plane, row) to the first (see ColPass::rev)
  int slay;        // layout of the ADMM work spectra (and of the copies of H / |G| the fused middle reads): 0 rows of cpitch
                   // elements; 1 PAIR LINES (spec_col below) -- kernels take it as a template argument, the host and
                   // paired_rows_of read this copy
  int PM;          // PSF planes the handle holds: state plane q uses PSF plane q % PM.  DC: one PSF for the batch
                   // (lpc_set_psf); batch * DC: one PSF per frame (lpc_set_psf_batch), q % PM == q.  (Last, so that a
                   // kernel that does not read it finds every other field where it was)
};
// ---- pair-line layout of a half spectrum (paired rows + 8-column middles: DiffuserCam-sized frames) --------------------
// The single-pass fused middle of a 540-row frame holds 8 image columns per tile: 64-byte row segments, half a cache line
// per access, and a line whose two halves are written by different workgroups is evicted half-dirty in between (the other
// half is fetched and the whole line written back: 1.19 x the algorithmic traffic at C4, profiles/r05_notes.md section 3).
// Here rows (2p, 2p + 1) x columns [8c, 8c + 8) share ONE 128-byte line:
//     element (r, k)  at  (r >> 1) * 2 cpitch + (k >> 3) * 16 + (r & 1) * 8 + (k & 7)
// -- a tile row pair is a full line for the middle (16 consecutive lanes), and the paired row kernels, which hold rows
// 2p and 2p + 1 of one array in one transform, still write / read whole lines (their two stores per bin are the two
// halves of the same line).  The base of a row pair is r0 * cpitch as before (r0 even: paired_rows_of aligns the
// window's pairs), SL = 0 is the plain layout.
template <int SL>
static __host__ __device__ __forceinline__ int spec_col(int k) { return SL ? k + (k & ~7) : k; }

// block coordinates of a kernel that honours PlaneGeom::rev
#define LPC_BX(g) ((g).rev ? gridDim.x - 1u - blockIdx.x : blockIdx.x)
#define LPC_BY(g) ((g).rev ? gridDim.y - 1u - blockIdx.y : blockIdx.y)
#define LPC_BZ(g) ((g).rev ? gridDim.z - 1u - blockIdx.z : blockIdx.z)

static __device__ __forceinline__ int wrap_add(int i, int d, int n) {  // (i + d) mod n for |d| <= n
  int r = i + d;
  if (r >= n) r -= n;
  if (r < 0) r += n;
  return r;
}

// four adjacent reals (16 bytes in float32; the float64 build moves two 16-byte halves)
#ifdef LPC_DOUBLE
struct alignas(16) real4 { double x, y, z, w; };     // two 16-byte halves per lane
#else
typedef float4 real4;
#endif
static __host__ __device__ __forceinline__ real4 make_real4(real x, real y, real z, real w) {
  real4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r;
}
static __device__ __forceinline__ real4 ld4(const real* p) { return *reinterpret_cast<const real4*>(p); }
static __device__ __forceinline__ void st4(real* p, real4 v) { *reinterpret_cast<real4*>(p) = v; }

// LDS bytes of a row tile of Wp points (row kernels, their launches and the planner)
#define LPC_ROW_SMEM_BYTES(Wp, skew) ((size_t)lds_slots_of((Wp), (int)(skew)) * sizeof(real2))

// ---- ADMM, paired rows: which two rows a workgroup transforms ------------------------------------------------------
// Two real rows share one complex transform of length Wp -- always two rows of the SAME array (rows r, r + 1 of r_sp; of
// `a`; of V; of H V).  Round 3 paired row r of one array with row r of the other (r_sp with a, V with H V): the smaller
// signal then inherits eps x |larger signal| of rounding noise through the Hermitian separation, which the reference
// does not have (it transforms every array on its own) -- 2e-5 instead of 4e-7 after six iterations with norm="forward"
// or a PSF scaled to l2 = 1e-3, where a and H V sit 3-6 decades below r_sp and V (tests/test_norm_scale.py).  Two
// adjacent rows of one array are of one magnitude, like the rows of the reference's own 2-D transform.
// Array 0 always has all its rows transformed: pairs (2j, 2j + 1), j < nA = ceil(Hp / 2).  Array 1 either likewise
// (nB = nA) or on the rows of the sensor window alone: pairs (sh + 2j, sh + 2j + 1), j < nB = ceil(H / 2)
// (AdmmScalars::skipa / skiphv).  grid.x = nA + nB; the first 2 nB blocks alternate between the arrays (block b runs on
// XCD b % 8, flipped every eighth block so that every XCD gets both kinds), the rest are array 0.
// Pair-line spectra (PlaneGeom::slay) need r0 even: the window's pairs then start at sh & ~1, and a pair that straddles the
// window's edge has one row that is neither formed nor stored (first / second).
struct PairedRows { int arr, r0; bool first, second; };
static inline int paired_rows_count(int rows) { return (rows + 1) >> 1; }
static __host__ __device__ __forceinline__ int paired_rows_window(const PlaneGeom& g) {
  return g.slay ? ((g.sh + g.H + 1) >> 1) - (g.sh >> 1) : (g.H + 1) >> 1;
}
static inline int paired_rows_grid(const PlaneGeom& g, bool window_b) {
  return paired_rows_count(g.Hp) + (window_b ? paired_rows_window(g) : paired_rows_count(g.Hp));
}

// ---- row passes (lpc_row_kernels.h): the real source / sink of the generic rows --------------------------------------
struct RealSrc {
  const real* base;
  long plane_stride;  // floats
  int pitch;          // floats per row
  int nrows;          // rows >= nrows are implicit zeros
  int ncols, col0;    // column c of the padded frame maps to base[...][c-col0] if in [col0,col0+ncols)
  int out_row0;       // source row r lands in spectrum row out_row0 + r
};

struct RealDst {
  real* base;
  long plane_stride;
  int pitch;
  int nrows;       // number of output rows (Hp if not cropping, H if cropping)
  int row0, col0;  // output (r, c) = shifted-frame (row0 + r, col0 + c); (0,0) when not cropping
  int ncols;       // Wp or W
};

// ---- column passes (lpc_col_kernels.h) ---------------------------------------------------------------------------------
struct ColPass {
  int N;            // transform length of this pass
  int G;            // groups along H (Hp / N)
  int istride;      // rows between consecutive transform elements
  int gstride;      // rows between consecutive groups:  row(g,i) = g*gstride + i*istride
  int T;            // image columns per tile
  int ntile_c;      // ceil(Wc / T)
  int tw_mode;      // 0: none; 1: multiply result k by twH[g*k] (forward pass A);
                    // 2: multiply input k by conj(twH[g*k]) (inverse pass A)
  int zr0, zr1;     // forward only: rows outside [zr0,zr1) are implicit zeros on load
  int need0, needn; // inverse only: rows r with ((r - need0) mod Hp) >= needn are never read again
                    // (they fall outside the crop window after ifftshift) and are not stored
  const real2* twH;  // exp(-2 pi i q / Hp), q in [0, Hp)
  // forward pass A of the ADMM work spectra: planes >= sc_plane0 (the spectrum of `a`) are multiplied by `sc` on load
  // in rows outside [sc_r0, sc_r1) -- rows whose forward row transform was skipped because it is mu1 * Wp times the
  // row spectrum the last inverse row pass consumed (AdmmScalars::skipa).  sc_plane0 = INT_MAX: off.
  int sc_plane0, sc_r0, sc_r1;
  real sc;
  FastDiv tdiv;     // fast divide by T
  FastDiv tcdiv;    // fast divide by ntile_c
  // ADMM LDS middle: hand the workgroups out so that two adjacent column tiles run on the SAME XCD (block b runs on XCD
  // b % 8): within every 16 consecutive blocks, block 8 s + x takes tile 2 x + s.  With 8-column tiles (64-byte row
  // segments: single-pass columns of one DiffuserCam-sized frame) the two tiles share every cache line, and on one L2 the
  // second one's loads are hits.
  int swz;
  // ADMM middles: |PsiT Psi| = ga[spectrum row] + gb[column] (null: read it from the plane).  The reference's gram
  // separates; read as a plane its 64-byte tile rows are fetched as whole lines once per colour plane -- 0.5 GB of the
  // 12-MP middle's 3.65 GB (profiles/r03_notes.md section 17)
  const real* ga;
  const real* gb;
  // walk the grid backwards (planes and blocks): a pass that starts where the previous kernel finished finds the last
  // ~256 MB that one wrote still in the memory-side cache (MI355X: 256 MB Infinity Cache in front of HBM)
  int rev;
};

// one element of the sequential middle's precombined constants (lpc_col_kernels.h: k_mid_consts)
struct alignas(16) MidConst { real2 c1, c2; };     // (k_mid_consts: behind the kernel that reads them)

// ---- ADMM, image domain (lpc_admm_kernels.h; the K1 comment there says what one pass computes) -------------------------
struct AdmmScalars {
  real mu1, mu2, mu3;  // this iteration's step sizes
  real thr;            // (real)(tau / mu2)
  real m_in, m_out;    // X_divmat inside / outside the sensor window
  int first;            // 1: no pending dual update (first iteration after reset)
  // the PREVIOUS iteration's values: its dual updates are still pending and its U, W are recomputed.
  // Equal to the current ones for plain ADMM; differ for unrolled ADMM (unrolled_admm.py:171-211)
  real mu1p, mu2p, mu3p, thrp;
  real m_in_p, m_out_p;  // X_divmat of the previous iteration (its X is recomputed, never stored)
  // correctly rounded reciprocals of the step sizes the kernels divide by (see div_by)
  real r_mu2, r_mu3, r_mu2p, r_mu3p;
  // Outside the sensor window the data term has no measurement: X_divmat = 1/mu1 there (admm.py:193), so
  //   X = xi/mu1 + HV,   a = mu1 X - xi = mu1 HV,   xi' = xi + mu1 (HV' - X) = mu1 (HV' - HV)
  // -- neither `a` nor the next xi depends on the stored xi.  xiw: the X half of the forward rows works from HV alone
  // outside the window (3/4 of the padded frame: no xi read, no HV_old read, no xi write); xi_store: this is the last
  // iteration of the lpc_iterate() call, write xi = mu1p (HV - HV_old) there as well so that every read-out between
  // calls (lpc_get_state, plug-and-play entries) finds the whole array valid.
  int xiw, xi_store;
  // Rows that lie outside the sensor window altogether carry a = mu1 HV, and HV of such a row is the (unnormalised)
  // inverse row transform of the spectrum row SB[r] that the last inverse row pass read: rfft(a row) = mu1 Wp SB[r].
  // skipa: the forward row blocks of `a` outside the window do nothing (SB[r] is still in place from the previous
  // iteration of this call; forward pass A applies the factor, ColPass::sc); skiphv: the inverse row blocks of HV
  // outside the window do nothing (no later iteration of this call reads those rows of HV -- the engine keeps the last
  // three iterations of a call complete so that xi, X and HV read out whole).
  int skipa, skiphv;
  // The reference clamps the image estimate IN PLACE whenever _form_image runs (admm.py:331-338: negative entries of
  // the sensor window become 0), and only the W-update ever sees that clamped copy (everything else works from the
  // cached Psi V / H V).  The clamp is a pure function of V, so no copy is kept: clamp_cur / clamp_old say that the
  // W-update of this / of the previous iteration saw clamp(V) / clamp(V_old).
  int clamp_cur, clamp_old;
  int rev;    // the tiled kernel walks its grid backwards (see ColPass::rev)
  // Half-applied duals between the iterations of ONE lpc_iterate() call (k_admm_spatial_v4, option k1_half):
  //   eta~ = eta - mu2 U,   rho~ = rho - mu3 W          (stored by an iteration with half_out)
  //   eta' = eta~ + mu2p Psi V_new,   rho' = rho~ + mu3p V_new      (the pending update, read by one with half_in)
  // -- algebraically eta + mu2p (Psi V_new - U), the reference's update (admm.py:300-311), but U and W of the previous
  // iteration need not be RECOMPUTED from V_old, so the kernel does not read V_old: 9 R -> 8 R of HBM traffic per launch.
  // The first iteration of a call reads, and the last one writes, the plain duals: every other entry point (read-outs,
  // plug-and-play, a caller's psi) sees the state of round 3.  Rounding differs from the reference's order of operations
  // by one ulp of the dual per iteration (float64 build: identical to 1e-16).
  int half_in, half_out;
  // Two arrays that travel between the iterations of a call are exact functions of others that travel anyway:
  // rho_rsp (k_admm_spatial_v4<.., HIN = true>, option rho_rsp): the previous iteration stored, in one statement,
  //   rho~ = rho' - mu3 W   and   r_sp = (mu3 W - rho') + D(q),  D(q) = (q0[below] - q0) + (q1[right] - q1),  eta~ = -q,
  // so rho~ = D(-eta~) - r_sp: the kernel loads its own pixel of r_sp where it would load rho~, forms D from the four
  // stored eta~ values it loads anyway (same association as d1 + d2) and overwrites that r_sp in place; rho is neither
  // written nor read between the iterations of a call (8 R -> 7 R), the last iteration writes the plain dual as before.
  // (The FIRST iteration of a call runs the non-HIN kernel, which still writes a rho~ that nobody reads: one launch per call.)
  // One rounding of r_sp's magnitude per iteration (float64 build: identical to 1e-15).
  int rho_rsp;
  // xi_in / xi_out (X half of the forward rows, option xi_half): inside the window xi travels half-applied as well,
  //   xi~ = xi' - mu1 X = -a   (stored by an iteration with xi_out),   xi'' = xi~ + mu1p HV_new   (read with xi_in)
  // -- the previous X need not be recomputed, so H V_old is not read inside the window (3 Rw -> 2 Rw).  Outside the
  // window nothing changes (xi is not stored there inside a call; xi_store on the last iteration still reads H V_old).
  int xi_in, xi_out;
};

// k_rfwd_arrays_x<.., K1 = true> (lpc_admm_row_kernels.h): the arrays of the TV / W half its row blocks work on
struct K1Rows {
  const real *V, *Vold, *eta0, *eta1;
  real *eta0_out, *eta1_out, *rho;
  int xcd_order;      // hand the row blocks out XCD by XCD: -1 an eighth of the launch each (small launches), G > 0 runs of G
                      // blocks (see the kernel), 0 launch order
};
