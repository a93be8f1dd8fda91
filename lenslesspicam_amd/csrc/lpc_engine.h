// lpc_engine.h -- what the translation units of the engine share: the handle, error plumbing, the launcher and the
// workgroup-shape dispatchers, and the host functions that cross translation units.  It defines no kernel and includes
// no header that does: a unit sees the kernels of the family headers it includes, and only those.
//
// One unit per role; the device compiler works on them in parallel, and a kernel is launched from the unit that
// instantiates it:
//   lpc_abi.cpp      the C ABI of include/lpc.h: argument checks, the call's stream, dispatch by algorithm, life cycle,
//                    profile read-out.  No kernel launch, no arithmetic of the method
//   lpc_planner.cpp  the option-driven rule table: frame geometry and the launch plan.  Nothing on the device
//   lpc_setup.cpp    twiddles and plans, geometry set-up, the common workspace, PSF spectrum, the bare operator, and the
//                    host helpers every algorithm shares with their layout / fill / min-max kernels
//   lpc_admm.cpp     ADMM: host sequences and every image-domain ADMM kernel
//   lpc_gd_host.cpp  the gradient-descent family: host sequences of the forward iterations
//   lpc_eval.cpp     evaluation reductions and the handle-free raw-frame / resize paths
//   lpc_rows.cpp     every row-pass launch (real <-> half-spectrum transforms, incl. the fused ADMM rows)
//   lpc_cols.cpp     every column-pass launch (pass A, the fused middles)
//   lpc_gd.cpp, lpc_gd_update.cpp, lpc_gd_update_p0.cpp, lpc_gd_update_p1.cpp   the gradient-descent family's fused row
//                    kernels (the update rows in three units: half-length rows, paired rows without / with the folded
//                    radix-2 stage)
//   lpc_gd_bwd.cpp   reverse mode of unrolled FISTA: its tape's layout, the sweep of lpc_fista_backward and its fused row
//                    kernels
//   lpc_admm_bwd.cpp reverse mode of unrolled ADMM: its tape's layout, the replay and the sweep of lpc_admm_backward
//   lpc_jit.cpp      plan modules: find / compile / load (lpc_plan.h)
//   lpc_module.cpp   NOT part of the library: the source of a plan module (compile-time-plan kernels of one frame shape)
//
// One header per kernel family, each included by the units that launch from it (tests/test_kernel_headers.py: every
// header compiles on its own, and lpc_abi.cpp, lpc_planner.cpp and lpc_jit.cpp see no kernel at all):
//   lpc_args.h             frame geometry and the kernels' argument structs; no kernel           this header, every family
//   lpc_row_kernels.h      row passes                                lpc_launch.h, lpc_gd_kernels.h, lpc_gd_bwd_kernels.h
//   lpc_col_kernels.h      column passes and fused middles           lpc_launch.h
//   lpc_admm_kernels.h     ADMM pixel arithmetic, image-domain kernels   lpc_admm.cpp, lpc_admm_bwd_kernels.h, the two below
//   lpc_admm_row_kernels.h forward rows with ADMM work fused in (k_rfwd_half_x, k_rfwd_arrays_x)   lpc_module.cpp alone
//   lpc_admm_v2_kernels.h  ... and the half-length ADMM rows in their second form                  lpc_module.cpp alone
//   lpc_layout_kernels.h   layout / set-up kernels                   lpc_setup.cpp, lpc_admm.cpp
//   lpc_reduce_kernels.h   workgroup reductions, min / max, gram separability   lpc_setup.cpp, lpc_admm.cpp, metric / prep
//   lpc_gd_kernels.h, lpc_gd_v2_kernels.h   gradient-descent family's fused rows   lpc_gd_launch.h, lpc_gd_host.cpp, lpc_gd_update_p*.cpp
//   lpc_gd_bwd_kernels.h, lpc_admm_bwd_kernels.h   the reverse modes    lpc_gd_bwd_launch.h, lpc_admm_bwd.cpp
//   lpc_metric_kernels.h, lpc_prep_kernels.h   evaluation and raw-frame paths   lpc_eval.cpp
// The launches of the kernels that the library and its plan modules both hold are written once, over the plan type:
// lpc_launch.h (rows, columns), lpc_gd_launch.h, lpc_gd_bwd_launch.h; each includes this header and its kernels.
#pragma once
#include "lpc_args.h"
#include "lpc.h"
#include "lpc_plan.h"

#ifndef LPC_SRC_FP
#define LPC_SRC_FP "dev"     // fingerprint of the sources (build.py): a module must be built from the same ones
#endif

#include <algorithm>
#include <climits>
#include <string>
#include <type_traits>
#include <unordered_set>
#include <vector>

// --------------------------------------------------------------------------- errors --
int fail(const std::string& msg);   // records the message for lpc_last_error() (thread-local), returns 1
#define LPC_RT(expr)                                                                      \
  do {                                                                                    \
    lpcError_t e_ = (expr);                                                               \
    if (e_ != lpcSuccess)                                                                 \
      return fail(std::string(#expr) + " failed: " + rt::err_string(e_));                 \
  } while (0)
#define LPC_OK(expr)          \
  do {                        \
    int r_ = (expr);          \
    if (r_) return r_;        \
  } while (0)


// Workgroup shape for an FFT tile of `nelem` complex points: NT threads x EMAX points per thread:
// the fewest threads that hold the tile with <= 16 points per thread.  Measured on MI355X
// (profiles/r01b_notes.md): the alternatives "twice the threads, half the points" (same LDS, twice
// the waves) and "half the threads, 32 points" are both slower.
// LDS holds 160 KiB per workgroup: 16384 complex64 points (128 KiB) or 8192 complex128 points
static constexpr int kMaxTilePoints = (int)(131072 / sizeof(real2));
template <class F>
static inline int dispatch_cfg(int nelem, F&& f) {
  using std::integral_constant;
  if (nelem <= 1024) return f(integral_constant<int, 256>{}, integral_constant<int, 4>{});
  if (nelem <= 2048) return f(integral_constant<int, 256>{}, integral_constant<int, 8>{});
  if (nelem <= 4096) return f(integral_constant<int, 256>{}, integral_constant<int, 16>{});
  if (nelem <= 8192) return f(integral_constant<int, 512>{}, integral_constant<int, 16>{});
  if (nelem <= kMaxTilePoints) return f(integral_constant<int, 1024>{}, integral_constant<int, 16>{});
  return fail("FFT tile of " + std::to_string(nelem) + " points exceeds the LDS budget (" +
              std::to_string(kMaxTilePoints) + ")");
}

// row kernels: (NT, EMAX) by row length, the LDS-skew flag and the radix-2-folding flag of the plan
template <class F>
static inline int dispatch_row(int Wp, int skew, bool r2, F&& f) {
  using std::integral_constant;
  return dispatch_cfg(Wp, [&](auto NT, auto EM) {
    if (skew && r2) return f(NT, EM, integral_constant<bool, true>{}, integral_constant<bool, true>{});
    if (skew) return f(NT, EM, integral_constant<bool, true>{}, integral_constant<bool, false>{});
    if (r2) return f(NT, EM, integral_constant<bool, false>{}, integral_constant<bool, true>{});
    return f(NT, EM, integral_constant<bool, false>{}, integral_constant<bool, false>{});
  });
}

struct KernelTimer {
#if !defined(LPC_SIMT_EMU)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[LPC_K_COUNT];
  size_t used[LPC_K_COUNT] = {0};
#endif
  bool on = false;
  unsigned mask = ~0u;      // bit k: launches of kernel id k are bracketed (lpc_profile_enable)
  int span = -1;            // kernel id whose launches share ONE event pair at the moment (timer_span_begin): not bracketed singly
};

// ADMM image-domain kernel (K1): inside the forward rows (TV / W half and X half: three launches per iteration); tiled
// TV / W half with the X half inside the forward rows; stand-alone on 16-byte lanes (padded width a multiple of 4) or scalar
enum AdmmK1 { ADMM_K1_ROWS, ADMM_K1_TV_W, ADMM_K1_TILED, ADMM_K1_SCALAR };
// ADMM fused middle: 24-point pass B in registers; the plan module's LDS middle; run-time plan in LDS on 512 threads x 18
// points, or on the workgroup shape of its tile size
// the rows of H V the inverse rows write: all; those of the sensor window (AdmmScalars::skiphv); none -- V alone, the window's
// rows of SB go through admm_rows_hv instead (LaunchPlan::hv_fuse)
enum AdmmHvRows { ADMM_HV_ROWS_ALL = 0, ADMM_HV_ROWS_WINDOW = 1, ADMM_HV_ROWS_NONE = 2 };
enum AdmmMid { ADMM_MID_REG24, ADMM_MID_MODULE, ADMM_MID_RT_512X18, ADMM_MID_RT_LDS };

// The launch plan of a handle: every kernel, tile shape, block order and fusion it runs, decided once at lpc_create
// (lpc_planner.cpp: choose_plan, finish_plan).  The launch code reads this record and nothing else of the options.
struct LaunchPlan {
  // -- choose_plan: what the plan module's key needs
  PlanSpec spec;           // the compile-time-plan kernels this handle runs (lpc_plan.h)
  int N1 = 1, N2 = 1;      // column split Hp = N1*N2 (N1 == 1: single pass)
  int T = 16;              // image columns per column-pass tile
  bool rows_half = false;  // one real row per half-length transform
  // -- finish_plan: once the module is loaded or refused
  bool xhalf_rows = false; // ADMM: xi / a = mu1 X - xi computed by the forward row kernel of the module
  bool xi_window = false;  // ... which then skips xi / HV_old outside the sensor window (AdmmScalars::xiw)
  bool hv_skip = false;    // ... and rows wholly outside it skip the H V row transforms in both directions (AdmmScalars::skipa)
  AdmmK1 k1 = ADMM_K1_SCALAR;
  bool k1_half = false;    // duals half-applied between the iterations of one call (AdmmScalars::half_in)
  bool rho_rsp = false;    // ... rho~ recovered from r_sp by the tiled TV / W kernel: rho not moved inside a call (AdmmScalars::rho_rsp)
  bool xi_half = false;    // ... xi half-applied too: the X half does not read H V_old where xi lives (AdmmScalars::xi_in)
  int admm_rows_v2 = 0;    // half-length rows in their second form (lpc_admm_v2_kernels.h; option admm_rows_v2): bit 0 the
                           // forward rows with the X half, bit 1 the inverse rows
  int hv_fuse = 0;         // ... and between the steady-state iterations of a call H V stays on chip: inverse row, the next X half and
                           // forward row of `a` in one kernel (k_hv_rows_v2; option hv_fuse).  1: that launch in front of the rows
                           // of V, 2: behind them
  int k1_xcd_order = 0;    // K1Rows::xcd_order
  AdmmMid admm_mid = ADMM_MID_RT_LDS;
  int conv_mid_reg = 0;    // convolution middle (conv_middle) in registers: its pass-B length; 0: in LDS
  bool gd_fuse_fwd = false;   // gradient-descent family: update kernel + next forward rows in one launch
  bool gd_v2 = false;         // ... its two fused row kernels in their second form (lpc_gd_v2_kernels.h; option gd_v2)
  // block orders, backwards (EngineOpts::rev_order, gd_rev): permutations, results unchanged
  bool rev_k1 = false, rev_passa_fwd = false, rev_passa_inv = false, rev_mid = false;
  bool gd_rev_resid = false, gd_rev_update = false, gd_rev_mid = false;
  int mid_swz = 0;         // ColPass::swz of the ADMM middle
  bool g_terms = false;    // ADMM middles read |PsiT Psi| as row + column terms when it separates (EngineOpts::g_plane)
};

// what a launch needs: the call's stream and the optional event bracketing.  A handle is one; the handle-free entry
// points (lpc_eval.cpp) make one of their own
struct LaunchCtx {
  KernelTimer timer;
  lpcStream_t stream = nullptr;
};

// ADMM: state (padded real planes) and constants
struct AdmmState {
  // copies of the PSF spectrum and |G| in the pair-line layout for the module's 8-column middle (PlaneGeom::slay)
  real2* Hs_t = nullptr;
  real* Gabs_t = nullptr;
  // ... and the sequential middle's point-wise constants, precombined per (PSF, step sizes) (lpc_col_kernels.h: k_mid_consts)
  void* midc = nullptr;       // MidConst (mid_pc 1) or real2 (mid_pc 2: real phases) per element
  real* midrd = nullptr;
  double midc_par[3] = {0, 0, 0};   // the step sizes the tables were made for
  bool midc_valid = false;
  real* Gabs = nullptr;    // |PsiT Psi| spectrum, ONE plane (identical for every channel)
  // ... and, when that plane is a sum of a row term and a column term (the reference's finite-difference gram is:
  // (2 - 2 cos th_r) + (2 - 2 cos th_c)), the two vectors the middles read instead of it: Ga[row] + Gb[col]
  real* Ga = nullptr;      // [Hp], the engine's (permuted) spectrum row order
  real* Gb = nullptr;      // [cpitch]
  real* Gpart = nullptr;   // partial maxima of the separability check
  int g_sep = 0;
  std::vector<double> sched[4];  // optional per-iteration mu1, mu2, mu3, tau (unrolled ADMM)
  double last_par[4] = {0, 0, 0, 0};  // parameters of the most recent iteration
  real *V[2] = {nullptr, nullptr}, *HVb[2] = {nullptr, nullptr}, *xi = nullptr, *rho = nullptr,
        *Rsp = nullptr, *Aarr = nullptr;
  real *eta0[2] = {nullptr, nullptr}, *eta1[2] = {nullptr, nullptr};  // ping-pong (halo reads)
  int vcur = 0, ecur = 0, hcur = 0;  // HVb[hcur] = H V of the current estimate, HVb[hcur^1] = of the previous one
  // the reference clamps the image estimate IN PLACE whenever _form_image runs (admm.py:331-338); only the W-update ever
  // sees that clamped copy, and it is a pure function of V: vw_cur = the next iteration's W sees clamp(V),
  // vw_old = the previous iteration's W saw clamp(V_old) (needed to recompute W_old) -- AdmmScalars::clamp_cur / _old
  bool vw_cur = false, vw_old = false;
  // plug-and-play ADMM (lpc_admm_pnp_begin / _end): explicit state in the arrays the fused path uses for the TV duals
  //   eta0[0] = eta, eta1[0] = U, eta0[1] = X, eta1[1] = W   (all image-shaped)
  bool pnp_mode = false, pnp_pending = false;
  bool custom_gram = false;    // lpc_set_psi_gram replaced the finite-difference gram (until the next lpc_set_psf)
};

// gradient-descent family: state (un-padded planes)
struct GdState {
  real *gx = nullptr, *gaux = nullptr;  // x and (p | xk_prev)
  real* galpha = nullptr;               // [C] device
  real* gx0 = nullptr;                  // [C] default start value per channel
  bool gx0_pinned = false;              // lpc_set_start_value: lpc_set_psf leaves gx0 alone
  real2* S2 = nullptr;                  // second spectrum buffer (row-inverse+forward is out of place)
  double tk = 1.0, nest_mu = 0.9, nest_p = 0.0;
  bool fwd_done = false;       // the row spectra of H x's input are already in S (written by the fused update kernel)
  bool split_pending = false;  // lpc_iterate_begin ran, lpc_iterate_end has not yet
};

// unrolled FISTA (unrolled_fista.py:91-106): per-iteration step alpha[i][c] and momentum factor coef[i]
struct FistaSchedule {
  std::vector<real> coef;
  real* galpha_sched = nullptr;  // device [n][C]
  size_t sched_cap = 0;          // elements allocated for it (re-used by later schedules that fit)
  int sched_n = 0;
  std::vector<real> alpha;       // host copy of the schedule's alpha (lpc_fista_backward refuses a zero step)
};

// The tape of a reverse mode (lpc_fista_record / lpc_admm_record; tape_alloc .. tape_record below).  ONE allocation of state
// arrays (`slot` elements each) for a schedule of n iterations, plus the per-workgroup partial sums of the sweep's reductions:
//   FISTA (lpc_gd_bwd.cpp), 2 n + 4 un-padded arrays:  y_0 .. y_n | xk_0 .. xk_{n-1} | work: gy / gz, carry, g_b
//       (y_i = gx before iteration i, xk_i = gaux after it); part: n * P * H * 2 doubles (g_coef / g_alpha per row)
//   ADMM (lpc_admm_bwd.cpp), 6 n + 11 padded arrays:  V_0 .. V_n | H V_0 .. H V_n | xi_0 .. xi_{n-1} | eta0_i | eta1_i |
//       rho_i | work: xib, rhob, etab0[0], etab1[0], etab0[1], etab1[1], rb, hr | g_b (un-padded planes inside a padded
//       array's room).  The recorded forward writes V_i only; the backward's replay fills in the rest.  part: 4 doubles per
//       workgroup of k_admm_bwd_step and iteration
// psf_ws, the PSF gradient's workspace, is ONE allocation too, made at its first call and freed with the tape:
//   FISTA: three spectrum buffers of P planes (residual rows / cross term; full spectrum of P gz_i / rows of P Hg_i; full
//       spectrum of P y_i) | the accumulator, P un-padded planes
//   ADMM: four work spectra of P planes (F V_{i+1}, F rb, F a_i, F ab) | the accumulator, C spectrum planes (one PSF per
//       frame: P planes -- a backward that needs more room than psf_ws has gives it back and allocates it again)
struct Tape {
  bool rec_on = false;
  real* buf = nullptr;
  size_t slot = 0;             // elements of one state array
  double* part = nullptr;
  int n = 0;                   // iterations the tape was allocated for
  long iters = -1;             // iterations recorded since the last reset (-1: nothing recorded)
  real* psf_ws = nullptr;
  size_t psf_ws_n = 0;         // elements psf_ws has room for
  real* at(long k) const { return buf + (size_t)k * slot; }
  void begin() { iters = 0; }
  void invalidate() { iters = -1; }      // what was recorded no longer matches the schedule / data / state: backward refuses
  bool wants(long iters_done) const { return iters >= 0 && iters == iters_done && iters_done < n; }   // push this iteration?
  void advance() { ++iters; }
  bool complete(long sched_n, long iters_done) const { return iters_done == sched_n && iters == sched_n && n == sched_n; }
};

struct lpc_engine : LaunchCtx {
  lpc_config cfg{};
  PlaneGeom g{};
  Fft1dPlan planW{}, planA{}, planB{};
  Fft1dPlan planWi{};   // inverse-row plan with the radix-2 stage FIRST (rows_r2 only)
  Fft1dPlan planWh{};   // length Wp/2: ADMM rows, one real row per half-length transform (rows_half)
  EngineOpts opt;          // lpc_config::options, as parsed (read by the planner and lpc_jit.cpp only)
  LaunchPlan plan;
  const struct LpcModule* mod = nullptr;   // the loaded plan module that holds plan.spec's kernels (null: run-time plans only)
  std::string mod_note;    // why there is no module, for lpc_plan_info
  bool rows_r2 = false; // row plans end in a radix-2 stage: fold it into the Hermitian (un)tangling
  ColPass passA{}, passB{};
  int P = 0, Ppsf = 0, Pdata = 0;      // Ppsf: PSF planes in use = g.PM (DC, or P with one PSF per frame)
  int psf_cap = 0;                      // ... and the planes Hs, psf_planar, Hs_t, midc and midrd have room for
  bool psf_per_frame = false;           // lpc_set_psf_batch set the PSFs (until the next lpc_set_psf)
  bool per_frame_grad = false;          // lpc_per_frame_grad: such a handle records and runs the backward entries
  std::vector<std::pair<void*, size_t>> allocs;   // every device allocation of the handle and its bytes (dev_alloc / dev_free)
  size_t total_bytes = 0;

  real2* Hs = nullptr;     // [Ppsf] PSF spectrum, permuted row order, norm applied
  real2* phr = nullptr;    // [Hp] ifftshift phase, stored row order
  real2* phc = nullptr;    // [Wc]
  real2* twH = nullptr;
  real2* tws_row = nullptr;   // stage twiddles of the module's row plan in lane order (lpc_sfft.h: SPlan::tws_off)
  // work spectra: [2][P] planes (ADMM uses both halves, others the first)
  real2* S = nullptr;
  real* Y = nullptr;         // data planes, un-padded [Pdata][H][W]
  int data_channels = 0;     // of the last lpc_set_data
  real* init_est = nullptr;  // planar copy of the initial estimate (or null)
  real* psf_planar = nullptr;
  real *conv_in = nullptr, *conv_out = nullptr;   // LPC_ALGO_CONV: staging planes of the channels-last <-> planar hop
  bool has_init = false, psf_set = false, data_set = false, first = true;
  long iters_done = 0;
  AdmmState admm;
  GdState gd;
  FistaSchedule fista;
  Tape fista_tape, admm_tape;
};
typedef lpc_engine Engine;

template <class Tp>
static inline int dev_alloc(Engine* e, Tp** out, size_t count) {
  void* p = nullptr;
  size_t bytes = count * sizeof(Tp);
  LPC_RT(rt::dev_malloc(&p, bytes));
  e->allocs.push_back({p, bytes});
  e->total_bytes += bytes;
  *out = (Tp*)p;
  return 0;
}
// gives one allocation of the handle back once the stream has drained (null: nothing to do)
static inline void dev_free(Engine* e, void* p) {
  if (!p) return;
  (void)rt::stream_sync(e->stream);
  for (auto it = e->allocs.begin(); it != e->allocs.end(); ++it)
    if (it->first == p) {
      e->total_bytes -= it->second;
      e->allocs.erase(it);
      break;
    }
  (void)rt::dev_free(p);
}

// ---- the tape of a reverse mode (struct Tape): what unrolled FISTA and unrolled ADMM do alike ----
static inline void tape_free(Engine* e, Tape& t) {
  dev_free(e, t.psf_ws);         // the PSF gradient's workspace goes with the tape
  dev_free(e, t.buf);
  dev_free(e, t.part);
  t.psf_ws = nullptr; t.buf = nullptr; t.part = nullptr; t.n = 0;
  t.psf_ws_n = 0;
  t.invalidate();
}
// the PSF gradient's workspace of `count` elements: made at the first call, made again when a later call needs more
static inline int tape_psf_ws(Engine* e, Tape& t, size_t count) {
  if (t.psf_ws && t.psf_ws_n >= count) return 0;
  dev_free(e, t.psf_ws);
  t.psf_ws = nullptr; t.psf_ws_n = 0;
  LPC_OK(dev_alloc(e, &t.psf_ws, count));
  t.psf_ws_n = count;
  return 0;
}
// for n iterations: nslots state arrays of `slot` elements and nparts partial sums, all or nothing (allocated for n: no-op)
static inline int tape_alloc(Engine* e, Tape& t, int n, size_t nslots, size_t slot, size_t nparts) {
  if (t.buf && t.n == n) return 0;
  tape_free(e, t);
  LPC_OK(dev_alloc(e, &t.buf, nslots * slot));
  if (dev_alloc(e, &t.part, nparts)) {
    tape_free(e, t);
    return 1;
  }
  t.n = n; t.slot = slot;
  return 0;
}
// lpc_fista_record / lpc_admm_record: on > 0 records, on < 0 pauses (the tape stays allocated, nothing is recorded), 0 frees.
// alloc: the solver's gd_tape_alloc / admm_tape_alloc, which does nothing without a schedule (lpc_reset allocates then)
static inline int tape_record(Engine* e, Tape& t, int on, int (*alloc)(Engine*)) {
  t.rec_on = on > 0;
  t.invalidate();
  if (on < 0) return 0;
  if (!t.rec_on) { tape_free(e, t); return 0; }
  return alloc(e);
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of a kernel: the (device, function) pairs that have
// it live in the CORE library (lpc_setup.cpp) -- launch_k is instantiated inside every plan module too, and a
// thread_local set there would register a TLS destructor that pins the module: dlclose() would never unload it
int big_smem_once(const void* fn, size_t smem);

// event bracketing of hot-loop kernels: one pair per launch, or one pair around the launches of kernel id `kid` between
// timer_span_begin and timer_span_end (two launches that are one entry of the per-iteration profile)
#if !defined(LPC_SIMT_EMU)
static inline bool timer_wants(const LaunchCtx* e, int kid) { return e->timer.on && kid >= 0 && ((e->timer.mask >> kid) & 1u); }
static inline int timer_open(LaunchCtx* e, int kid, size_t* slot) {
  auto& v = e->timer.ev[kid];
  *slot = e->timer.used[kid]++;
  if (*slot >= v.size()) {
    hipEvent_t a, b;
    LPC_RT(hipEventCreate(&a));
    LPC_RT(hipEventCreate(&b));
    v.push_back({a, b});
  }
  LPC_RT(hipEventRecord(v[*slot].first, e->stream));
  return 0;
}
#endif
static inline int timer_span_begin(LaunchCtx* e, int kid, size_t* slot) {
#if !defined(LPC_SIMT_EMU)
  if (!timer_wants(e, kid)) return 0;
  LPC_OK(timer_open(e, kid, slot));
  e->timer.span = kid;
#else
  (void)e; (void)kid; (void)slot;
#endif
  return 0;
}
static inline int timer_span_end(LaunchCtx* e, int kid, size_t slot) {
#if !defined(LPC_SIMT_EMU)
  if (e->timer.span != kid) return 0;
  e->timer.span = -1;
  LPC_RT(hipEventRecord(e->timer.ev[kid][slot].second, e->stream));
#else
  (void)e; (void)kid; (void)slot;
#endif
  return 0;
}

// generic launcher (+ optional event bracketing of hot-loop kernels)
template <class K, class... A>
static inline int launch_k(LaunchCtx* e, int kid, K kernel, dim3 grid, int nt, size_t smem, A... args) {
  if (smem > 48 * 1024) LPC_OK(big_smem_once((const void*)kernel, smem));
#if !defined(LPC_SIMT_EMU)
  const bool timed = timer_wants(e, kid) && kid != e->timer.span;
  size_t slot = 0;
  if (timed) LPC_OK(timer_open(e, kid, &slot));
  hipLaunchKernelGGL(kernel, grid, dim3(nt), smem, e->stream, args...);
  if (timed) LPC_RT(hipEventRecord(e->timer.ev[kid][slot].second, e->stream));
#else
  (void)kid;
  lpc_emu::launch(grid, dim3(nt), smem, [=]() { kernel(args...); });
#endif
  LPC_RT(rt::last_error());
  return 0;
}

static inline dim3 grid1d(long n, int nt, long planes = 1) {
  long b = (n + nt - 1) / nt;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return dim3((unsigned)b, (unsigned)planes, 1);
}

static inline RealSrc src_unpadded(const Engine* e, const real* base) {
  const PlaneGeom& g = e->g;
  RealSrc s;
  s.base = base; s.plane_stride = g.uplane; s.pitch = g.W; s.nrows = g.H; s.ncols = g.W; s.col0 = g.sw;
  s.out_row0 = g.sh;
  return s;
}
static inline RealSrc src_padded(const Engine* e, const real* base) {
  const PlaneGeom& g = e->g;
  RealSrc s;
  s.base = base; s.plane_stride = g.rplane; s.pitch = g.rpitch; s.nrows = g.Hp; s.ncols = g.Wp; s.col0 = 0;
  s.out_row0 = 0;
  return s;
}
static inline RealDst dst_padded(const Engine* e, real* base) {
  const PlaneGeom& g = e->g;
  RealDst d;
  d.base = base; d.plane_stride = g.rplane; d.pitch = g.rpitch; d.nrows = g.Hp; d.row0 = 0; d.col0 = 0;
  d.ncols = g.Wp;
  return d;
}
static inline RealDst dst_cropped(const Engine* e, real* base) {
  const PlaneGeom& g = e->g;
  RealDst d;
  d.base = base; d.plane_stride = g.uplane; d.pitch = g.W; d.nrows = g.H; d.row0 = g.sh; d.col0 = g.sw;
  d.ncols = g.W;
  return d;
}

// ---- plan module: launchers of the compile-time-plan kernels of one frame shape (lpc_module.cpp) -------------------
// An entry is null when the module does not hold that kernel; the core then launches its run-time-plan kernel.
struct GdScalars;
struct GdBwd;
struct LpcModule {
  int (*rows_fwd_single)(Engine*, const RealSrc*, real2* S, int nplanes, int kid);
  int (*rows_inv_single)(Engine*, const real2* S, const RealDst*, int nplanes, int kid);
  int (*admm_rows_fwd)(Engine*);
  // k1: + the TV / W half (k1_rows); a_done: the rows of `a` are in SB already (admm_rows_hv), r_sp alone
  int (*admm_rows_fwd_x)(Engine*, const AdmmScalars*, const K1Rows* k1, int a_done);
  int (*admm_rows_inv)(Engine*, real* Vout, real* HVout, int hv_rows);      // hv_rows: ADMM_HV_ROWS_*
  // H V rows on chip (k_hv_rows_v2): the window's rows of SB -> H V -> X half with the NEXT iteration's scalars -> rows of `a`
  int (*admm_rows_hv)(Engine*, const AdmmScalars* next);
  int (*gd_rows_mid)(Engine*, const real2* Sin, real2* Sout);
  int (*gd_rows_update)(Engine*, const GdScalars*, const real* alpha);
  int (*gd_rows_update_fwd)(Engine*, const GdScalars*, const real* alpha);
  int (*gd_bwd_head)(Engine*, const GdBwd*);       // reverse mode of unrolled FISTA (lpc_gd_bwd_kernels.h), half rows
  int (*gd_bwd_mid)(Engine*, const GdBwd*);
  int (*gd_bwd_update)(Engine*, const GdBwd*);
  int (*gd_bwd_acc)(Engine*, const GdBwd*, const real2* Sin);   // ... the PSF gradient's accumulate (MODE 3)
  int (*cols_passA)(Engine*, const ColPass*, real2* S, int nplanes, int inverse, int kid);
  int (*admm_mid)(Engine*, const ColPass*, const AdmmScalars*, real sb_outside_scale);
  int k1_rows;    // admm_rows_fwd_x takes the TV / W half of the image-domain work as well (k_rfwd_arrays_x<.., K1>)
  int mid_pc;     // its sequential middle reads the precombined constants (AdmmState::midc / midrd)
  int slay;       // its ADMM row kernels and fused middle keep the work spectra in pair lines (PlanSpec::slay)
  int gd_v2;      // the module holds k_gd_resid_v2 / k_gd_update_fwd_v2 for its row plan (lpc_gd_v2_kernels.h)
  int admm_rows_v2;   // ... k_rinv_half_v2 / k_rfwd_half_x_v2 (lpc_admm_v2_kernels.h)
};
// lpc_jit.cpp: the module of `spec` -- from the process cache, from disk, or (allow_compile) compiled now; null + `why`
const LpcModule* get_plan_module(const PlanSpec& spec, const EngineOpts& opt, bool allow_compile, std::string* why);
void release_plan_module(const LpcModule* mod);     // a handle that got a module from get_plan_module is done with it
int build_plan_module(const PlanSpec& spec, const EngineOpts& opt, std::string* path_or_error);   // compile only (no load); no-op when the module is on disk

// ---- host functions that cross translation units ------------------------------------------------------------
// lpc_planner.cpp: frame geometry (rfft_convolve.py:110-117), plane counts and the launch plan of a configuration
struct ShapePlan {
  PlaneGeom g{};
  int P = 0, Ppsf = 0, Pdata = 0;
  LaunchPlan plan;
  bool want_static = false;   // the frame is large enough for compile-time plans and the options allow them
};
int plan_cu_count();
bool plan_radices(int n, std::vector<int>& rad);
int setup_shape(const lpc_config& c, const EngineOpts& o, int cu, ShapePlan* out);
void choose_plan(const lpc_config& c, const EngineOpts& o, const PlaneGeom& g, int P, bool allow_static, int cu, LaunchPlan* pl);
void finish_plan(const lpc_config& c, const EngineOpts& o, const PlaneGeom& g, int P, const LpcModule* mod, bool lane_twiddles,
                 int cu, LaunchPlan* pl);
// lpc_setup.cpp
int upload(Engine* e, void* dst, const void* src, size_t bytes);
int setup_geometry(Engine* e);
int alloc_common(Engine* e);                                    // PSF spectrum, work spectra, data / staging planes
int set_psf(Engine* e, const real* dev_psf);
int set_psf_batch(Engine* e, const real* dev_psfs);             // one PSF per frame: (B, D, H, W, C)
int fft2_forward_setup(Engine* e, const RealSrc& src, real2* S, int nplanes);
int cols_fwd_full(Engine* e, real2* S, int nplanes, int zr0, int zr1);   // row spectra (rows [zr0, zr1)) -> full 2-D spectra, Hs layout
int convolve_planar(Engine* e, const real* xin, real* xout, int nplanes, bool padded_io, bool adjoint);
int convolve_hwc(Engine* e, const real* dev_x, real* dev_out, int n, int x_channels, bool adjoint, bool spectrum);
int hwc_to_planar(Engine* e, const real* src, real* dst, int nimg, int rows, int cols, int pitch, long dplane,
                  int src_channels = 0);
int planar_to_hwc(Engine* e, real* src, real* dst, int nimg, int rows, int cols, int pitch, long splane, int row0, int col0,
                  int clamp);
int planar2_to_hwc2(Engine* e, const real* a0, const real* a1, real* dst, int nimg);   // two padded arrays -> (.., 2)
int check_channels(const Engine* e, int ch, const char* who);
int fill_planar(Engine* e, real* p, long n, real v);
int plane_minmax(Engine* e, const real2* Hs, const real* plane, int nblk, int nplanes, real* partial);   // k_plane_minmax
// lpc_admm.cpp
int admm_alloc(Engine* e);
int admm_alloc_psf(Engine* e, int nplanes);                     // the copies of H and what is precombined from it, for nplanes PSF planes
int admm_setup_constants(Engine* e);
int admm_reset(Engine* e);
int admm_iterate(Engine* e, int n_iter);
int admm_pnp_begin(Engine* e, int use_dual, real* dev_denoiser_in);
int admm_pnp_end(Engine* e, int use_dual, const real* dev_U);
int admm_set_psi_gram(Engine* e, const real* dev_gabs);
int admm_psi_step(Engine* e, const real* dev_psit);
int admm_form_image(Engine* e, real* dev_out);
int admm_get_state(Engine* e, const std::string& nm, real* dev_out);
int admm_kernel_bytes(Engine* e, int kid, double* bytes);
double admm_model_bytes(const Engine* e);
int admm_spectral_plain(Engine* e, const double par[4], real* Vout, real* HVout);   // (Rsp, Aarr) -> S(Rsp + HT Aarr), H of it, with par's R_divmat
// lpc_admm_bwd.cpp
int admm_tape_alloc(Engine* e);                    // for the handle's schedule (none yet: nothing, lpc_reset allocates)
int admm_tape_reset(Engine* e);                    // admm_reset: V_0, or nothing when the handle does not record
int admm_tape_push(Engine* e, const real* Vnew);   // admm_iterate: the iterate an iteration just wrote
int admm_backward(Engine* e, const real* grad_out, real* grad_data, real* grad_mu1, real* grad_mu2, real* grad_mu3,
                  real* grad_tau, real* grad_psf = nullptr);
// lpc_gd_host.cpp
int gd_alloc(Engine* e);
int gd_setup_constants(Engine* e);
int gd_apply_momentum_reset(Engine* e);
int gd_set_schedule(Engine* e, int n, const real* alpha, const real* coef);
int gd_reset(Engine* e);
int gd_iterate(Engine* e, int n_iter, int split = 0);
int gd_finish_split(Engine* e, const real* dev_projected);
int gd_form_image(Engine* e, real* dev_out);
int gd_get_state(Engine* e, const std::string& nm, real* dev_out);
int gd_kernel_bytes(Engine* e, int kid, double* bytes);
double gd_model_bytes(const Engine* e);
// lpc_rows.cpp
int rows_fwd_single(Engine* e, const RealSrc& src, real2* S, int nplanes, int kid);
int rows_inv_single(Engine* e, const real2* S, const RealDst& dst, int nplanes, int kid);
int admm_rows_fwd(Engine* e);                                   // e->admm.Rsp, e->admm.Aarr -> the two work spectra
int admm_rows_inv(Engine* e, real* Vout, real* HVout, int hv_rows = ADMM_HV_ROWS_ALL);          // the two work spectra -> V, H V
// lpc_cols.cpp
int cols_passA(Engine* e, real2* S, int nplanes, bool inverse, int zr0, int zr1, int kid, bool crop_rows_only = false,
               real sb_outside_scale = (real)0.);
int cols_passB_fwd(Engine* e, real2* S, int nplanes, int zr0, int zr1);
// mult (mult_planes planes, Hs layout): the multiplier spectrum in place of the PSF's; plane p reads plane p % mult_planes
int conv_middle(Engine* e, real2* S, int nplanes, bool adjoint, int zr0, int zr1, bool crop_rows_only = false,
                const real2* mult = nullptr, int mult_planes = 0);
int admm_cols(Engine* e, const AdmmScalars& sc);   // sc.skipa: forward pass A rescales the kept rows of SB                // [pass A] -> fused ADMM middle -> [inverse pass A]
// lpc_gd.cpp, lpc_gd_update.cpp (one kernel family each)
int gd_rows_mid(Engine* e, const real2* Sin, real2* Sout);      // irfft rows -> residual -> rfft rows (the iteration: S -> S2)
int gd_rows_update(Engine* e, const GdScalars& sc, const real* alpha);   // irfft rows -> fused projected update
// lpc_gd_bwd.cpp
int gd_tape_alloc(Engine* e);                      // for the handle's schedule (none yet: nothing, lpc_reset allocates)
int gd_tape_reset(Engine* e);                      // gd_reset: y_0, or nothing when the handle does not record
int gd_tape_push(Engine* e);                       // gd_iterate: what the update of an iteration just wrote
int gd_backward(Engine* e, const real* grad_out, real* grad_data, real* grad_alpha, real* grad_coef, real* grad_init,
                real* grad_psf = nullptr);
int gd_bwd_rows(Engine* e, int mode, const GdBwd& a, const real2* Sin = nullptr);   // reverse-mode rows: 0 head, 1 middle, 2 update + next head, 3 PSF-gradient accumulate (rows of Sin)
int gd_bwd_psf_sum(Engine* e, const real* acc, real* grad_psf); // ... and its sum over the batch -> (1, H, W, C)
int gd_bwd_gdata(Engine* e, const real* gb, real* grad_data);   // planar data gradient -> the measurement's layout (both sweeps)
