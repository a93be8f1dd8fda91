// lpc_planner.cpp -- the option-driven rule table: frame geometry and the launch plan of a configuration, decided from
// (lpc_config, EngineOpts, compute units) and, once known, the loaded plan module.  Touches nothing on the device and
// launches nothing; lpc_create (lpc_setup.cpp: setup_geometry) and the device-less lpc_plan_module call it alike.
#include "lpc_engine.h"

static int next_5smooth(int n) {  // scipy.fftpack.next_fast_len (rfft_convolve.py:112)
  int m = n < 1 ? 1 : n;
  for (;; ++m) {
    int r = m;
    while (r % 2 == 0) r /= 2;
    while (r % 3 == 0) r /= 3;
    while (r % 5 == 0) r /= 5;
    if (r == 1) return m;
  }
}
// radices of a length-n transform (5-smooth): few, fat stages -- the number of radix-6 stages (each pairs a 2 with a 3)
// that minimises the stage count; ties keep more radix-8 stages.  8s first (the twiddle-free first stage should be fat).
bool plan_radices(int n, std::vector<int>& rad) {
  rad.clear();
  int r = n, a = 0, b3 = 0;
  while (r % 2 == 0) { r /= 2; ++a; }
  while (r % 3 == 0) { r /= 3; ++b3; }
  int c5 = 0;
  { int t = r; while (t % 5 == 0) { t /= 5; ++c5; } }
  int best_k6 = 0, best_cnt = 1 << 30;
  for (int k6 = 0; k6 <= std::min(a, b3); ++k6) {
    const int a2 = a - k6;
    const int cnt = k6 + a2 / 3 + (a2 % 3 ? 1 : 0) + (b3 - k6) + c5;
    if (cnt < best_cnt) { best_cnt = cnt; best_k6 = k6; }
  }
  a -= best_k6;
  for (int i = 0; i < a / 3; ++i) rad.push_back(8);
  a %= 3;
  for (int i = 0; i < best_k6; ++i) rad.push_back(6);
  b3 -= best_k6;
  if (a == 2) rad.push_back(4);
  if (a == 1) rad.push_back(2);
  while (r % 5 == 0) { r /= 5; rad.push_back(5); }
  for (int i = 0; i < b3; ++i) rad.push_back(3);
  return r == 1;
}
// same rule as plan_from_radices(): the i + i/8 LDS skew stays affine in every stage
static bool radices_skew_ok(int n, const std::vector<int>& rad) {
  int ns = 1;
  for (int r : rad) {
    if ((n / r) % 8 != 0) return false;
    if (!(ns % 8 == 0 || (ns == 1 && r % 8 == 0))) return false;
    ns *= r;
  }
  return true;
}

// LDS layout of a compile-time row plan (lpc_fft.h: lds_slot): i + i/8 where the plan keeps it affine.  (The conflict-free
// xor layout and i + i/16 were built and measured in rounds 4 / 5: LDS busy 47 % -> 20 %, kernel time unchanged -- the row
// kernels wait for the vector-memory path, not for LDS; profiles/HISTORY.md)
static int row_layout(int n, const std::vector<int>& rad) { return radices_skew_ok(n, rad) ? 1 : 0; }

// choose the column split Hp = N1*N2 and the tile width
static void choose_split(const EngineOpts& opt, int Hp, int Wc, int* N1, int* N2, int* T, bool prefer24 = false,
                         bool admm_f32 = false) {
  int t = 16;
  if (opt.col_t > 0) t = opt.col_t;  // option col_t
  while (t > 1 && t / 2 >= Wc) t /= 2;  // tiny images: do not waste lanes on empty columns
  int budget = kMaxTilePoints;          // points per LDS tile, worst case two arrays (ADMM middle)
  if (opt.tile_budget > 0) budget = std::max(64, opt.tile_budget);  // option tile_budget (tests)
  for (int tt = t; tt >= (t >= 8 ? 8 : t); tt /= 2) {
    if ((long)Hp * 2 * tt <= budget) { *N1 = 1; *N2 = Hp; *T = tt; return; }
    if (tt == 1) break;
  }
  int best1 = 1, best2 = Hp, bestcost = 1 << 30;
  for (int d = 1; d <= Hp; ++d) {
    if (Hp % d) continue;
    const int n2 = d, n1 = Hp / d;
    if ((long)n2 * 2 * t > budget / 2 || (long)n1 * t > budget / 2) continue;
    const int cost = std::max(n1, 2 * n2);
    // ADMM (float32), equal cost: the shorter pass A and the longer LDS middle -- 6144 rows as 96 x 64 instead of 128 x 48:
    // pass A 0.466 / 0.460 -> 0.448 / 0.434 ms, middle +0.012 ms, iteration -1.1 % (same box, three instances each)
    if (cost < bestcost || (admm_f32 && cost == bestcost && n2 > best2)) { bestcost = cost; best1 = n1; best2 = n2; }
  }
  // A 24-point pass B runs the fused middle in registers (k_cols_mid_admm_reg / k_cols_mid_mul_reg<8,3>) with the
  // fewest registers; worth it as long as pass A stays short.  Measured (r01b_notes.md): 2160 rows, 90 x 24 vs
  // 72 x 30: ADMM 72.8 vs 68.3 it/s, FISTA 2134 vs 2013 it/s; 6144 rows, 256 x 24 vs 128 x 48: ADMM 191 vs 204 it/s.
  // (ADMM: up to a 96-point pass A only -- 3072 rows run 1.6 % faster as 64 x 48 with the LDS middle than as 128 x 24,
  // 82.1 against 83.4-83.7 ms per 100 iterations of a 1520 x 2028 x 3 frame, r03z_ab.log)
  if (prefer24 && Hp % 24 == 0 && Hp / 24 <= (admm_f32 ? 96 : 128) && Hp / 24 >= 2 && (long)(Hp / 24) * t <= budget / 2) {
    best2 = 24; best1 = Hp / 24;
  }
  if (opt.split_n2 > 0) {  // option split_n2: force the length of the fused middle transform
    const int n2 = opt.split_n2;
    if (n2 > 0 && Hp % n2 == 0 && (long)n2 * 2 * t <= budget && (long)(Hp / n2) * t <= budget) { best2 = n2; best1 = Hp / n2; }
  }
  *N1 = best1; *N2 = best2; *T = t;
}
// ---- the launch plan: everything that is decided once per handle, no device work -----------------------------------
static void set_static_fft(StaticFft& f, int n, const std::vector<int>& rad, int T, int nt, int em) {
  f = StaticFft{};
  if ((int)rad.size() > LPC_SPEC_MAX_ST) return;    // (cannot happen for n <= 16384 with these radices: leaves n == 0)
  f.n = n; f.nst = (int)rad.size();
  for (int i = 0; i < f.nst; ++i) f.rad[i] = rad[(size_t)i];
  f.T = T; f.nt = nt; f.em = em;
}
static inline int round_up64(int v) { return (v + 63) / 64 * 64; }
// option row_rad: "16.16.8" replaces `rad` when it is a factorisation of n into radices that have a butterfly
// (lpc_fft.h: Dft<R>)
static void override_radices(const std::string& opt, int n, std::vector<int>& rad) {
  if (opt.empty()) return;
  std::vector<int> r;
  long prod = 1;
  size_t i = 0;
  while (i < opt.size()) {
    size_t j = opt.find('.', i);
    if (j == std::string::npos) j = opt.size();
    const int v = std::atoi(opt.substr(i, j - i).c_str());
    static const int ok[] = {2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16, 18, 20, 24, 30};
    if (std::find(std::begin(ok), std::end(ok), v) == std::end(ok)) return;
    r.push_back(v);
    prod *= v;
    i = j + 1;
  }
  if (prod == n && (int)r.size() <= LPC_SPEC_MAX_ST) rad = r;
}

// compute units the launch plan is sized for: the device's when there is one, an MI355X's for the device-less
// lpc_plan_module() path (build.py pre-building modules in a container without a GPU)
int plan_cu_count() {
#if defined(LPC_SIMT_EMU)
  return 256;       // (the emulator chooses the plans the MI355X would)
#endif
  int n = 0;
  if (rt::device_count(&n) != lpcSuccess || n <= 0) return 256;
  return rt::cu_count();
}

// `allow_static`: choose compile-time plans (-> pl->spec, served by a plan module) wherever the kernels exist; false: the
// run-time plans of the core library alone.  Starts the record afresh and sets N1, N2, T, rows_half and the spec; `P`: planes
// of a batch, `cu`: compute units the plan is sized for (plan_cu_count).
void choose_plan(const lpc_config& c, const EngineOpts& o, const PlaneGeom& g, int P, bool allow_static, int cu, LaunchPlan* out) {
  const bool admm = c.algo == LPC_ALGO_ADMM, f32 = sizeof(real) == 4;
  LaunchPlan& pl = *out;
  pl = LaunchPlan{};
  pl.spec.family = admm ? LPC_FAM_ADMM : LPC_FAM_GD;
  pl.spec.f64 = f32 ? 0 : 1;
  // (a 24-point register middle for ADMM in float32 only: 2 x 24 complex128 values do not fit a lane's registers)
  // (the gradient-descent family keeps 128 x 48 at 6144 rows: its 48-point middle lives in registers)
  choose_split(o, g.Hp, g.Wc, &pl.N1, &pl.N2, &pl.T, !admm || f32, admm && f32);
  // the column kernels of a plan module address their tiles with 24-bit row-index x row-step products (k_cols): the step
  // between two rows of one column transform must stay below 2^24 bytes (12 MP: 48 rows x 32.8 KB = 1.6 MB)
  const long col_step = (long)(pl.N1 > 1 ? pl.N2 : 1) * g.cpitch * (long)sizeof(real2);
  const bool st_cols = allow_static && col_step < (1L << 24) && g.Hp < (1 << 24) &&
                       (unsigned long long)g.Hp * g.cpitch * sizeof(real2) < (1ULL << 32);   // ... and offsets are 32-bit
  // Single-pass ADMM columns whose two-spectra tile allows only 8 image columns (DiffuserCam-sized frames, 540 padded
  // rows): the fused middle takes the two spectra one after the other through the tile (k_cols_mid_admm_seq), one
  // parked in registers while the other is transformed ... when the batch is large enough to fill the chip with
  // workgroups that each hold one spectrum (64 frames 1.20 -> 0.96 ms per launch; ONE frame 0.032 -> 0.042 ms: 93
  // workgroups for 256 CUs): four 39-KB workgroups of 512 lanes x 9 points per CU inside 64 VGPRs.  (Whole 6144-point
  // columns two at a time through the same kernel -- one launch instead of three per column step -- were built and measured
  // in round 4: 2.25 ms against 1.455 ms; 16-column tiles: 30 % slower.  profiles/HISTORY.md)
  const bool seq = admm && f32 && st_cols && pl.N1 == 1 && pl.T == 8 && g.Wc > 8 && (long)g.Hp * 16 <= kMaxTilePoints &&
                   o.col_t == 0 && o.mid_seq != 0 && ((long)P * ((g.Wc + 15) / 16) >= 512 || o.mid_seq == 1);
  // Row passes: one real row per half-length complex transform (k_r*_half kernels) once the
  // paired tile is so large that fewer than 5 workgroups fit a CU's 160 KiB of LDS.  Measured (r01b_notes.md):
  // 8192 columns +3 % it/s, 3840 columns (C5) +1.8 %; 960 columns (C4) -5 %: the short transforms leave most
  // of a 256-thread group idle.
  // The gradient-descent family switches earlier (its irfft -> residual -> rfft kernel runs two transforms per
  // workgroup): 2048 columns FISTA +6.8 %, ADMM -1 %.
  // ... and with compile-time plans at every even width: its paired-row kernels exist on run-time plans only, and a
  // half-length transform on its own plan beats them (same-box A/B, profiles/r03_notes.md: FISTA 270x480x3 3.85 -> 3.35 ms
  // per 60 iterations, 380x507x3 4.40 -> 3.75 ms).  ADMM keeps the size rule with either kind of plan (540 x 960: paired
  // 0.298 vs half 0.311 ms per 5 iterations; 768 x 1024: 0.374 vs 0.364; 3072 x 4096: paired 43.6 vs half 44.6 ms per 50).
  // Round 6: ADMM on compile-time plans keeps PAIRED rows up to 4096 columns -- paired rows take the TV / W half of the
  // image-domain work (two quads per lane: three launches per iteration, r_sp never stored), which half-length rows cannot
  // (four quads per lane: slower than the tiled kernel).  Same box, paired + fused against half-length + tiled kernel
  // (profiles/r06_notes.md): 16 x 1080p (3840 columns) 175.3 -> 170.7 ms per 20 iterations, two of its planes 54.5 -> 52.3,
  // 1520 x 2028 x 3 (4096) 30.18 -> 29.23 ms per 40; 5000 / 5760 columns -1.3 / -0.5 %, 6000 +1.4 %, 8192 (12 MP) +3 %,
  // 5120 = 8.8.8.2.5 +10 %: half-length rows above 4096.
  const bool half_ok = g.Wp % 2 == 0 && g.Wp >= 4;
  const bool admm_wide = (allow_static && g.Wp % 4 == 0 && o.k1_rows != 0) ? g.Wp > 4096
                                                                            : 5 * LPC_ROW_SMEM_BYTES(g.Wp, 1) > 160 * 1024;
  const bool wide = admm ? admm_wide : (g.Wp >= 2048 || (allow_static && g.Wp >= 128));
  pl.rows_half = half_ok && wide;
  if (o.rows_half == 0) pl.rows_half = false;
  if (o.rows_half == 1 && half_ok) pl.rows_half = true;
  if (!allow_static) return;

  PlanSpec& sp = pl.spec;
  std::vector<int> rad;
  // the X half of the image-domain work moves into the forward rows when the stencil half can run as the tiled
  // four-pixel-lane kernel (k_admm_spatial_v4<.., XHALF = false>): padded width a multiple of 4
  const bool xhalf = admm && g.Wp % 4 == 0;
  // ---- rows
  if (pl.rows_half) {
    const int n = g.Wp / 2;
    plan_radices(n, rad);
    if (n == 4096) rad = {16, 16, 16};   // one butterfly per thread and stage, one LDS round trip fewer than 8.8.8.8
                                          // (same-box A/B, profiles/r02_notes.md: inverse rows 0.518 -> 0.487 ms)
    if (n == 2048 && admm) rad = {16, 16, 8};   // same idea, 256 threads x 8 points: 3072 x 4096 frames 44.4 -> 43.1 ms per
                                                 // 50 iterations (profiles/r03k_ab.log; the paired 2048-point rows of
                                                 // 1536 x 2048 frames and the 1024-point rows are faster on 8.8.8.x)
    if (n == 1920 && admm) rad = {16, 8, 15};   // 1080p frames, three stages on 128 threads x 15 points: 4 of C5's planes
                                                 // 49.1 -> 46.4 ms per 20 iterations (r03u_ab.log; 16.15.8 47.9, 24.10.8
                                                 // 48.4, 20.12.8 47.4; the gradient-descent family is FASTER on 8.8.6.5)
    override_radices(o.row_rad, n, rad);
    int nt = std::min(1024, std::max(64, round_up64(n / rad[0])));   // every lane owns a first-stage butterfly
    if (n == 2048 && admm && rad[0] == 16) nt = 256;
    // twice the lanes for 4096 = 16.16.16 (512 x 8 points: every other lane has no butterfly, but the tangling, the
    // loads and the stores get twice the waves): 12 MP FISTA 75.8 -> 73.4 ms per 40 iterations, ADMM 135.4 -> 134.3
    // (r03v_ab.log; 1024 lanes: 81.4 / 148.2); likewise the gradient-descent family's 1024 = 8.8.8.2 on 256 lanes
    // (1536 x 2048 frames: 4.43 -> 4.30 ms per 60 iterations); 2048-point rows are faster on 256 in both families
    if (n == 4096 && rad[0] == 16) nt = 512;
    if (n == 1024 && !admm) nt = 256;
    set_static_fft(sp.row, n, rad, 1, nt, (n + nt - 1) / nt);
    if (sp.row.n && sp.row.em <= 16) {
      sp.row_kind = LPC_ROWS_HALF;
      sp.row_sk = row_layout(n, rad);
      sp.row_x = xhalf;
    }
  } else if (admm) {    // paired rows: ADMM's own kernels only (set-up transforms keep the run-time plan)
    const int n = g.Wp;
    plan_radices(n, rad);
    // no folded radix-2 stage on compile-time plans: 8 ... 2 -> 4 ... 4
    if (rad.size() >= 2 && rad.back() == 2) {
      for (size_t i = rad.size() - 1; i-- > 0;)
        if (rad[i] == 8) { rad[i] = 4; rad.back() = 4; std::stable_sort(rad.begin(), rad.end(), [](int a, int b) { return (a == 8) > (b == 8); }); break; }
    }
    override_radices(o.row_rad, n, rad);
    int nt = std::min(1024, std::max(64, round_up64(n / rad[0])));
    // short rows (960 = 8.8.5.3: 120 first-stage butterflies): 128 threads x 8 points for batches, where every lane
    // then owns a butterfly of the stage that issues the global loads (forward rows 0.642 -> 0.576 ms at 64 frames);
    // ONE frame is faster on 256 x 4 (0.460 vs 0.470 ms per 5 iterations, profiles/r02_notes.md)
    // Round 5: ... unless the rows can take the TV / W half of the image-domain work as well (Engine::k1_rows: one
    // quad per lane and row, i.e. 256 lanes here) -- three launches per iteration beat the better row shape at every batch
    // size (64 frames 33.1 -> 31.0 ms per 20 iterations, 8 frames 4.27 -> 4.00 ms; profiles/r05_notes.md section 5)
    if (nt < 256 && n >= 512) {
      const bool batch = (long)P * g.Hp >= 8192;
      const bool k1r = xhalf && o.k1_rows != 0 && n % 4 == 0 && n / 4 <= 256;   // (lpc_module.cpp: kK1Rows)
      if (o.prow_nt128 == 0 || (o.prow_nt128 < 0 && (!batch || k1r))) nt = 256;
    }
    set_static_fft(sp.row, n, rad, 1, nt, (n + nt - 1) / nt);
    if (sp.row.n && sp.row.em <= 16) {
      sp.row_kind = LPC_ROWS_PAIRED;
      sp.row_sk = row_layout(n, rad);
      sp.row_x = xhalf;
    }
  }
  // ---- pass A of a split column transform: 32 columns per tile (256-byte row segments at its long row stride) while
  // the fused middle keeps 16 -- the two passes tile the columns independently.  Same-box A/B at 12 MP with T = 32 for
  // both (profiles/r02_notes.md): pass A 0.578 / 0.575 -> 0.530 / 0.510 ms, the middle 0.655 -> 0.71 ms.
  if (st_cols && pl.N1 > 1) {
    int T = pl.T;
    if (pl.T == 16 && g.Wc >= 256 && o.col_t == 0) T = 32;
    if (o.passa_t > 0) T = o.passa_t;
    while (T > 1 && (long)pl.N1 * T > kMaxTilePoints) T /= 2;
    plan_radices(pl.N1, rad);
    if (pl.N1 == 90) rad = {10, 9};      // two stages instead of 6.5.3: 16 x 1080p planes 48.1 -> 46.9 ms per 20 iterations
                                          // (r03k_ab.log; 9.10, 18.5, 30.3 are slower, and 128 = 16.8 is slower than 8.8.2 at 12 MP)
    const int pts = pl.N1 * T;
    int nt = T >= 32 ? 512 : 256;
    while (nt < 1024 && (pts + nt - 1) / nt > 16) nt *= 2;
    set_static_fft(sp.passA, pl.N1, rad, T, nt, (pts + nt - 1) / nt);
    if (sp.passA.em > 16) sp.passA = StaticFft{};
  }
  // ---- ADMM's fused middle in LDS (a 24-point pass B lives in registers: k_cols_mid_admm_reg, core library)
  const bool reg_mid = pl.N1 > 1 && f32 && pl.N2 == 24;
  if (admm && st_cols && !reg_mid) {
    const int n = pl.N2, T = pl.T;
    plan_radices(n, rad);
    // 540 = 30.18 side by side (two fat register butterflies, one LDS trip; 184 registers, one workgroup per CU);
    // one spectrum at a time: 6.10.9 inside a 128-register budget = TWO workgroups per CU overlapping one another's
    // loads and barriers -- 0.650 ms per launch at 64 frames against 0.84 ms for 30.18 and 0.95 ms for 6.6.5.3
    // (on 512 lanes the order 10.6.9 is 2 % faster than 6.10.9 -- 0.453 vs 0.464 ms at 64 frames, two instances each,
    // profiles/r04u_ab_shard5.log; 9.10.6 0.479, 10.9.6 0.482, 6.9.10 0.498)
    if (n == 540) rad = seq ? std::vector<int>{10, 6, 9} : std::vector<int>{30, 18};
    // A launch of fewer workgroups than the chip holds at once (one DiffuserCam frame: 183 tiles on 256 CUs) lasts as
    // long as ONE workgroup takes: twice the lanes on half the points each shorten that chain -- 540 x 16 points on 1024
    // lanes as 6.10.9 (every stage has >= 864 butterflies; 30.18 has 288 / 480): C1's middle 21.2 -> 19.1 us, the
    // 5-iteration call 0.243 -> 0.234 ms (profiles/r04t_ab_c1.log; 30.18 on 1024 lanes 19.8 us, 768 lanes 19.6 us).
    // Only while every workgroup has a CU of its own (256 on an MI355X): two frames = 366 tiles are 6 % SLOWER that way
    // (0.370 -> 0.392 ms, r04t_ab_c1c.log).
    const bool one_wave_of_tiles = !seq && pl.N1 == 1 && (long)P * ((g.Wc + T - 1) / T) <= cu && n * 2 * T > 8192;
    if (one_wave_of_tiles && n == 540) rad = {6, 10, 9};
    const int pts = n * (seq ? T : 2 * T);
    int nt = pts <= 4096 ? 256 : (pts <= 9216 ? 512 : 1024);
    // one spectrum at a time: 8 columns x 540 points on 512 lanes x 9 points (round 3: 256 x 17) -- the middle of a batch
    // of 8 / 16 / 32 / 64 frames 79.6 -> 75.7 / 140 -> 136 / 262 -> 255 / 505 -> 491 us, the 8-frame shard's 20-iteration
    // call 4.55 -> 4.44 ms (profiles/r04u_ab_shard2.log; 384 lanes 103 us, 1024 lanes 77.9 us, 16 columns x 1024: 84 us);
    // three instances of each at 64 / 8 frames (r04u_ab_shard4.log): 256 lanes 0.499 ms / 78.5 us, 512 lanes 0.493 / 74.2,
    // 512 lanes inside 64 VGPRs 0.464 / 70.6
    if (seq) nt = pts <= 9 * 256 ? 256 : (pts <= 18 * 512 ? 512 : 1024);
    if (one_wave_of_tiles) nt = 1024;
    set_static_fft(sp.mid, n, rad, T, nt, (pts + nt - 1) / nt);
    if (sp.mid.n && sp.mid.em <= 18) {
      sp.mid_kind = seq ? LPC_MID_SEQ : LPC_MID_PAIR;
      if (seq) {   // waves per SIMD the register allocation must allow: as many workgroups as the LDS holds
        // both tiles' loads up front (round 4: large batches only; round 6: the 8-frame shard too, 3.86 -> 3.83 ms per call)
        sp.mid_pre = o.mid_pre >= 0 ? (o.mid_pre ? 1 : 0) : 1;
        const size_t lds = (size_t)n * (T + 1) * sizeof(real2);        // tile + the plan's twiddles behind it
        const int wgs = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds));
        // (512 lanes: 8 = a 64-VGPR allocation, four workgroups per CU as the LDS allows -- 68 registers without the
        // bound, i.e. three; the middle of 64 / 8 frames 0.493 -> 0.464 ms / 74.2 -> 70.6 us)
        sp.mid_minw = std::min(8, std::max(1, (wgs * nt + 255) / 256));
      }
    } else {
      sp.mid = StaticFft{};
    }
  }
  // pair-line work spectra (lpc_args.h: spec_col): paired rows + a single-pass middle of 8-column tiles, float32 (a tile row
  // of 8 complex128 columns is a whole line already)
  sp.slay = (admm && f32 && sp.row_kind == LPC_ROWS_PAIRED && sp.mid_kind != LPC_MID_RUNTIME && pl.N1 == 1 && sp.mid.T == 8 &&
             o.spec_lay != 0) ? 1 : 0;
  // ... the sequential middle's point-wise constants precombined (k_mid_consts); even padded sizes: the ifftshift phases are
  // +-1, one complex constant per element instead of two (mid_pc = 2)
  sp.mid_pc = (sp.slay && sp.mid_kind == LPC_MID_SEQ && o.mid_pc != 0) ? ((g.Hp % 2 == 0 && g.Wp % 2 == 0) ? 2 : 1) : 0;
}

// the rest of the launch plan, once the module is loaded or refused (mod, g.slay) and it is known whether the row plan's
// stage twiddles exist in lane order (lane_twiddles)
void finish_plan(const lpc_config& c, const EngineOpts& o, const PlaneGeom& g, int P, const LpcModule* mod, bool lane_twiddles,
                 int cu, LaunchPlan* out) {
  LaunchPlan& pl = *out;
  const bool admm = c.algo == LPC_ALGO_ADMM, gd = c.algo >= LPC_ALGO_GD, split = pl.N1 > 1;
  // The half of the image-domain work that needs no neighbours rides in the module's forward row kernel: the blocks of
  // `a` compute xi' and a = mu1 X - xi' from xi, HV, HV_old, y themselves (-2R per iteration), the tiled kernel keeps
  // the stencil half at its own occupancy (without a module: the full stand-alone kernel) ...
  pl.xhalf_rows = admm && mod && mod->admm_rows_fwd_x;
  // ... narrow frames (paired rows of one quad per lane: padded widths up to 1024) hand it the TV / W half too: three
  // launches per iteration, r_sp never stored.  One small frame is a chain of launch boundaries and memory latencies
  // (C1 -7.6 %), a batch saves the trip of r_sp through memory and the tiled kernel's launch (C4 -6.3 %);
  // profiles/r05_notes.md section 5 (option k1_rows=0: off)
  // (round 6: rows of TWO quads per lane as well -- padded widths up to 2048: the reference's own profile frame 760 x 1014
  // gray 0.458 -> 0.442 ms per 5 iterations, 8 frames of 600 x 800 x 3 22.1 -> 20.8 ms per 20; profiles/r06_notes.md.  FOUR
  // quads per lane -- 12-MP half-length rows -- are slower than the tiled kernel: not built)
  const bool k1_rows = pl.xhalf_rows && g.Wp % 4 == 0 && mod->k1_rows != 0 && o.k1_rows != 0;
  pl.k1 = k1_rows ? ADMM_K1_ROWS : pl.xhalf_rows ? ADMM_K1_TV_W : g.Wp % 4 == 0 ? ADMM_K1_TILED : ADMM_K1_SCALAR;
  // duals half-applied between the iterations of one call (option k1_half=0: never)
  pl.k1_half = pl.xhalf_rows && o.k1_half != 0;
  // ... then two of the arrays that travel are functions of the others: the tiled TV / W kernel reads rho~ back out of
  // the r_sp it overwrites (the three-launch plan stores no r_sp), and the X half keeps xi as -a (options rho_rsp=0,
  // xi_half=0: off; k1_half=0 implies both off)
  pl.rho_rsp = pl.k1_half && pl.k1 == ADMM_K1_TV_W && o.rho_rsp != 0;
  pl.xi_half = pl.k1_half && o.xi_half != 0;
  // the second form of the half-length row kernels (one-radix row plan, float32: the module says so); the blocks of `a` make
  // 8-byte accesses to y and xi: even window offset and frame width
  // (bit 0: the forward rows -- the default; bit 1: the inverse rows as well, slower at 12 MP: profiles/admm_rows_v2_notes.md)
  pl.admm_rows_v2 = (admm && pl.rows_half && mod && mod->admm_rows_v2 && lane_twiddles && ((g.sw | g.W) & 1) == 0 && g.W >= 2)
                        ? (o.admm_rows_v2 & 3) : 0;
  // K1Rows::xcd_order.  (The XCD-aware block orders assume the MI355X's 8 XCDs x 32 CUs and its dispatch rule "workgroup w
  // on XCD w % 8"; any other part gets launch order: the orders are permutations, results are the same.)
  pl.k1_xcd_order = cu != 256 ? 0 : (long)paired_rows_grid(g, false) * P <= 8192 ? -1 : std::max(0, o.k1_group);
  // ... outside the sensor window that half works from HV alone (AdmmScalars::xiw; option xi_full: every pixel alike) ...
  pl.xi_window = pl.xhalf_rows && !o.xi_full;
  // ... and rows wholly outside it skip the H V row transforms in both directions: the kept rows of SB are rescaled by
  // forward pass A (any plan) or, for single-pass columns, by the module's fused middle (option hv_full: off)
  pl.hv_skip = pl.xi_window && !o.hv_full && mod->admm_rows_inv && (split || mod->admm_mid);
  // ... and in the steady state of a call the window's rows of H V stay in registers between the inverse row and the next
  // iteration's forward row (k_hv_rows_v2: the forward rows' second form, float32; option hv_fuse=0: off, 2: behind the rows of V)
  pl.hv_fuse = ((pl.admm_rows_v2 & 1) && pl.hv_skip && pl.xi_half && mod->admm_rows_hv && pl.k1 == ADMM_K1_TV_W) ? (o.hv_fuse & 3) : 0;
  if (pl.hv_fuse == 3) pl.hv_fuse = 1;
  // ADMM middle.  Two arrays per lane: only short pass-B transforms fit the register file.  Measured at 12 MP
  // (profiles/r01b_notes.md): 24 points 0.89 ms and 32 points 0.83 ms beat the LDS middle (0.99 / 0.92 ms) but
  // need a 256- / 192-point pass A that costs more than it saves; 48 points is 1.62 ms (AGPR traffic).
  // Just above 8192 points (C1 / C4: 540 rows x 8 columns x 2 arrays = 8640): 512 threads x 18 points keeps
  // TWO workgroups per CU inside the 128-VGPR budget; 1024 x 16 is one 16-wave workgroup per CU in lock-step
  // at every barrier (C4: middle 1.435 -> 1.331 ms, 17.5k -> 18.0k frame-it/s)
  const long mid_pts = (long)pl.N2 * pl.T * 2;
  pl.admm_mid = split && sizeof(real) == 4 && pl.N2 == 24 ? ADMM_MID_REG24
                : mod && mod->admm_mid ? ADMM_MID_MODULE
                : mid_pts > 8192 && mid_pts <= 9216 ? ADMM_MID_RT_512X18 : ADMM_MID_RT_LDS;
  // convolution middle: one lane = one whole pass-B column transform in registers, for the lengths choose_split produces most
  static const int kRegMid[] = {48, 40, 36, 32, 30, 24};
  pl.conv_mid_reg = split && std::find(std::begin(kRegMid), std::end(kRegMid), pl.N2) != std::end(kRegMid) ? pl.N2 : 0;
  pl.gd_fuse_fwd = gd && mod && mod->gd_rows_update_fwd && !o.gd_no_fuse_fwd;
  // the second form of the fused row kernels: 8-byte accesses to y / x need an even window offset and frame width
  pl.gd_v2 = gd && mod && mod->gd_v2 && lane_twiddles && o.gd_v2 != 0 && ((g.sw | g.W) & 1) == 0 && g.W >= 2;
  pl.rev_k1 = o.rev_order & 1;
  pl.rev_passa_fwd = o.rev_order & 2;
  pl.rev_passa_inv = o.rev_order & 4;
  pl.rev_mid = o.rev_order & 8;
  // EngineOpts::gd_rev -1: all three (the row kernels and the register middle alternate with the forward-walking pass A, so
  // every kernel starts where its predecessor finished): 12 MP FISTA 75.4 / 74.1 / 73.8 -> 74.5 / 73.0 / 72.8 ms per 40 iterations
  // on three instances of one box against the middle alone (r03z_ab.log); no effect at 1080p, where nothing is reversed
  const int gd_rev = o.gd_rev >= 0 ? o.gd_rev : ((size_t)g.cplane * P * sizeof(real2) > ((size_t)200 << 20)) ? 7 : 0;
  const bool mod_gd_rows = mod && mod->gd_rows_mid;     // the run-time-plan row kernels walk forwards only
  pl.gd_rev_resid = mod_gd_rows && (gd_rev & 1);
  pl.gd_rev_update = mod_gd_rows && (gd_rev & 2);
  pl.gd_rev_mid = gd_rev & 4;
  // pairs of column tiles on one XCD: measured (profiles/r03_notes.md) -6 % on the 5-iteration C1 call, whose 8-column
  // tiles read half cache lines (middle 0.0278 -> 0.0228 ms); at 12 MP (16 columns = whole lines) it removes a third of
  // the middle's excess HBM reads (2.44 -> 2.28 GB against 1.91 GB asked for) but runs 3 % slower -- off there
  pl.mid_swz = o.mid_swz >= 0 ? o.mid_swz : ((size_t)pl.T * sizeof(real2) < 128 && !g.slay ? 1 : 0);
  // Measured (r03z_ab.log): at 12 MP (100-MB plane, 64-byte tile rows fetched as whole lines once per colour plane) the
  // terms take 0.5 GB off the middle's HBM traffic, 0.622 -> 0.563 ms; on DiffuserCam-sized frames the 1-MB plane lives
  // in the L2 and one load beats two (C1 middle 0.0206 -> 0.0221 ms with the terms)
  pl.g_terms = o.g_plane >= 0 ? !o.g_plane : ((size_t)g.cplane * sizeof(real) > ((size_t)8 << 20));
}

// frame geometry (rfft_convolve.py:110-117), plane counts and the launch plan before the module is known
int setup_shape(const lpc_config& c, const EngineOpts& o, int cu, ShapePlan* out) {
  PlaneGeom& g = out->g;
  g.H = c.height; g.W = c.width;
  g.Hp = next_5smooth(2 * g.H - 1);
  g.Wp = next_5smooth(2 * g.W - 1);
  g.Wc = g.Wp / 2 + 1;
  g.sh = (g.Hp - g.H) / 2;
  g.sw = (g.Wp - g.W) / 2;
  g.rpitch = (g.Wp + 3) / 4 * 4;
  g.cpitch = (g.Wc + 15) / 16 * 16;
  g.rplane = (long)g.Hp * g.rpitch;
  g.cplane = (long)((g.Hp + 1) & ~1) * g.cpitch;      // whole row pairs (PlaneGeom::slay)
  g.slay = 0;
  g.uplane = (long)g.H * g.W;
  g.DC = c.depth * c.channels;
  g.C = c.channels;
  g.PM = g.DC;
  g.rev = 0;
  out->Ppsf = g.DC;
  out->P = c.batch * g.DC;
  out->Pdata = c.batch * c.channels;
  if (g.Wp > kMaxTilePoints)
    return fail("padded width " + std::to_string(g.Wp) + " > " + std::to_string(kMaxTilePoints) + " is not supported");
  // compile-time plans live in a plan module (lpc_plan.h): look for it, build it if allowed, else run-time plans
  out->want_static = !o.no_static && (long)g.Hp * g.Wp >= o.jit_min_points;
  choose_plan(c, o, g, out->P, out->want_static, cu, &out->plan);
  return 0;
}
