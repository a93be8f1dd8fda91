// lpc_setup.cpp -- set-up and the host helpers every algorithm shares: twiddles and run-time plans, the geometry of a
// handle, its common workspace, the PSF spectrum, the bare operator (LPC_ALGO_CONV), channels-last <-> planar layout.
// The layout, fill and plane min / max kernels are instantiated here alone; other units call the host functions
// (declared in lpc_engine.h).
#include "lpc_engine.h"
#include "lpc_layout_kernels.h"
#include <mutex>
#include <unordered_map>
#include "lpc_reduce_kernels.h"

// ------------------------------------------------------------------------ FFT plans --
int upload(Engine* e, void* dst, const void* src, size_t bytes) {
  LPC_RT(rt::copy_h2d_async(dst, src, bytes, e->stream));
  LPC_RT(rt::stream_sync(e->stream));
  return 0;
}

int big_smem_once(const void* fn, size_t smem) {
  static std::mutex mu;
  static std::unordered_map<uint64_t, size_t> granted;      // (function, device) -> dynamic LDS the kernel may use
  int dev = 0;
  LPC_RT(rt::current_device(&dev));
  const uint64_t key = (uint64_t)(uintptr_t)fn ^ ((uint64_t)(dev + 1) << 56);
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = granted[key];
  if (have < smem) {            // first launch, or a later one (another handle, a wider tile) that needs more
    // (a kernel with static LDS of its own -- the stamped timing builds, lpc_rt.h: LPC_STAMP -- cannot have the whole
    // 160 KiB as dynamic LDS: ask for what this launch needs then)
    size_t want = smem > 65536 ? (size_t)160 * 1024 : (size_t)65536;
    if (rt::set_max_dyn_smem(fn, want) != lpcSuccess) {
      (void)rt::last_error();
      want = smem;
      LPC_RT(rt::set_max_dyn_smem(fn, want));
    }
    have = want;
  }
  return 0;
}

static int make_twiddles(Engine* e, int n, real2** out) {
  std::vector<real2> h((size_t)std::max(n, 1));
  for (int q = 0; q < n; ++q) {
    const double a = -2.0 * M_PI * (double)q / (double)n;
    h[q] = make_real2((real)std::cos(a), (real)std::sin(a));
  }
  LPC_OK(dev_alloc(e, out, h.size()));
  return upload(e, *out, h.data(), h.size() * sizeof(real2));
}

// stage twiddles of a compile-time plan in lane order: layout and purpose in lpc_sfft.h (SPlan::tws_off)
static int make_stage_twiddles(Engine* e, const StaticFft& f, real2** out) {
  *out = nullptr;
  std::vector<real2> h;
  int ns = f.rad[0];
  auto w = [&](long q) {
    const double a = -2.0 * M_PI * (double)(q % f.n) / (double)f.n;
    return make_real2((real)std::cos(a), (real)std::sin(a));
  };
  for (int st = 1; st < f.nst; ++st) {
    const int R = f.rad[st], nb = f.n / R, step = f.n / (ns * R);
    const size_t base = h.size();
    if (R == 8 || R == 16) {         // base powers {q, 2q}, {4q, 8q}: [pair][j][2]
      h.resize(base + (size_t)4 * nb);
      for (int hh = 0; hh < 2; ++hh)
        for (int j = 0; j < nb; ++j)
          for (int i = 0; i < 2; ++i)
            h[base + ((size_t)hh * nb + j) * 2 + i] = w((long)(j % ns) * step * (1L << (2 * hh + i)));
    } else {                         // every power: [m - 1][j]
      h.resize(base + (size_t)(R - 1) * nb);
      for (int m = 1; m < R; ++m)
        for (int j = 0; j < nb; ++j) h[base + (size_t)(m - 1) * nb + j] = w((long)(j % ns) * step * m);
    }
    ns *= R;
  }
  if (h.empty()) return 0;
  LPC_OK(dev_alloc(e, out, h.size()));
  return upload(e, *out, h.data(), h.size() * sizeof(real2));
}

static int plan_from_radices(Engine* e, Fft1dPlan& p, int n, const std::vector<int>& rad) {
  p.n = n;
  p.nst = 0;
  if ((int)rad.size() > LPC_MAX_STAGES) return fail("too many FFT stages");
  int ns = 1;
  for (size_t s = 0; s < rad.size(); ++s) {
    p.radix[s] = rad[s];
    p.ns[s] = ns;
    p.nsdiv[s] = make_fastdiv((unsigned)ns);
    p.twstep[s] = n / (ns * rad[s]);
    ns *= rad[s];
  }
  if (ns != n) return fail("internal: radices do not multiply to the length");
  p.nst = (int)rad.size();
  p.skew_ok = 1;  // see lpc_fft.h: every butterfly stride must be a multiple of 8
  for (int st = 0; st < p.nst; ++st) {
    const int nb = n / p.radix[st];
    if (nb % 8 != 0) p.skew_ok = 0;
    if (!(p.ns[st] % 8 == 0 || (p.ns[st] == 1 && p.radix[st] % 8 == 0))) p.skew_ok = 0;
  }
  // diagnostic only (results are garbage): no butterflies at all, every pass degenerates to "tile in, tile out"
  // through LDS -- times the memory access pattern of the passes alone (profiles/r01b_notes.md)
#ifdef LPC_DEBUG_KNOBS   // never in the product build: the results are garbage by construction
  if (std::getenv("LPC_DEBUG_NOFFT")) p.nst = 0;
#endif
  real2* tw = nullptr;
  LPC_OK(make_twiddles(e, n, &tw));
  p.tw = tw;
  return 0;
}
static int build_plan(Engine* e, Fft1dPlan& p, int n) {
  p.n = n;
  p.nst = 0;
  std::vector<int> rad;
  if (!plan_radices(n, rad)) return fail("length " + std::to_string(n) + " is not 5-smooth");
  return plan_from_radices(e, p, n, rad);
}
// stored row p = k1*N2 + k2  <->  frequency k = k1 + N1*k2
static inline int stored_row_freq(const Engine* e, int p) { return (p / e->plan.N2) + e->plan.N1 * (p % e->plan.N2); }
int setup_geometry(Engine* e) {
  const int cu = plan_cu_count();
  ShapePlan sp;
  LPC_OK(setup_shape(e->cfg, e->opt, cu, &sp));
  e->g = sp.g; e->P = sp.P; e->Ppsf = sp.Ppsf; e->Pdata = sp.Pdata; e->plan = sp.plan;
  const PlaneGeom& g = e->g;
  e->mod = nullptr;
  if (!sp.want_static) e->mod_note = e->opt.no_static ? "no_static" : "small frame";
  else if (e->plan.spec.any()) {
    e->mod = get_plan_module(e->plan.spec, e->opt, e->opt.jit != 0, &e->mod_note);
    if (!e->mod) {      // lpc_plan_info() names the module a deployment without a compiler would have to ship
      const std::string key = plan_spec_key(e->plan.spec);
      if (e->mod_note.find(key) == std::string::npos) e->mod_note = "module " + key + ": " + e->mod_note;
      choose_plan(e->cfg, e->opt, g, e->P, false, cu, &e->plan);
    }
  }
  if (!e->mod) e->plan.spec = PlanSpec{};
  e->g.slay = (e->mod && e->mod->slay) ? 1 : 0;
  LPC_OK(build_plan(e, e->planW, g.Wp));
  e->rows_r2 = e->planW.nst >= 2 && e->planW.radix[e->planW.nst - 1] == 2;
  if (e->rows_r2) {
    std::vector<int> rad{2};
    for (int st = 0; st + 1 < e->planW.nst; ++st) rad.push_back(e->planW.radix[st]);
    LPC_OK(plan_from_radices(e, e->planWi, g.Wp, rad));
    e->planWi.skew_ok = 0;
  }
  if (e->plan.rows_half) LPC_OK(build_plan(e, e->planWh, g.Wp / 2));
  e->tws_row = nullptr;
  if (e->mod && e->plan.spec.row_kind != LPC_ROWS_RUNTIME) LPC_OK(make_stage_twiddles(e, e->plan.spec.row, &e->tws_row));
  LPC_OK(build_plan(e, e->planB, e->plan.N2));
  if (e->plan.N1 > 1) LPC_OK(build_plan(e, e->planA, e->plan.N1));
  finish_plan(e->cfg, e->opt, g, e->P, e->mod, e->tws_row != nullptr, cu, &e->plan);
  LPC_OK(make_twiddles(e, g.Hp, &e->twH));
  const int ntc = (g.Wc + e->plan.T - 1) / e->plan.T;
  ColPass& A = e->passA;
  A.N = e->plan.N1; A.G = e->plan.N2; A.istride = e->plan.N2; A.gstride = 1; A.T = e->plan.T; A.ntile_c = ntc;
  A.tw_mode = 0; A.zr0 = 0; A.zr1 = g.Hp; A.twH = e->twH; A.need0 = 0; A.needn = g.Hp;
  A.sc_plane0 = INT_MAX; A.sc_r0 = 0; A.sc_r1 = g.Hp; A.sc = (real)1.;
  A.tdiv = make_fastdiv((unsigned)e->plan.T); A.tcdiv = make_fastdiv((unsigned)ntc);
  A.swz = 0;
  A.rev = 0;
  A.ga = A.gb = nullptr;
  ColPass& B = e->passB;
  B = A;
  B.N = e->plan.N2; B.G = e->plan.N1; B.istride = 1; B.gstride = e->plan.N2;
  if (e->plan.spec.passA.n) {       // the module's pass A tiles the columns on its own (choose_plan)
    A.T = e->plan.spec.passA.T;
    A.ntile_c = (g.Wc + A.T - 1) / A.T;
    A.tdiv = make_fastdiv((unsigned)A.T);
    A.tcdiv = make_fastdiv((unsigned)A.ntile_c);
  }
  // ifftshift phases: out[i] = in[(i + n/2) mod n]  <=>  multiply bin k by exp(+2 pi i k (n/2) / n)
  std::vector<real2> pr((size_t)g.Hp), pc((size_t)g.Wc);
  for (int p = 0; p < g.Hp; ++p) {
    const long k = stored_row_freq(e, p);
    const double a = 2.0 * M_PI * (double)((k * (g.Hp / 2)) % g.Hp) / (double)g.Hp;
    pr[p] = make_real2((real)std::cos(a), (real)std::sin(a));
  }
  for (int k = 0; k < g.Wc; ++k) {
    const double a = 2.0 * M_PI * (double)(((long)k * (g.Wp / 2)) % g.Wp) / (double)g.Wp;
    pc[k] = make_real2((real)std::cos(a), (real)std::sin(a));
  }
  LPC_OK(dev_alloc(e, &e->phr, pr.size()));
  LPC_OK(dev_alloc(e, &e->phc, pc.size()));
  LPC_OK(upload(e, e->phr, pr.data(), pr.size() * sizeof(real2)));
  LPC_OK(upload(e, e->phc, pc.data(), pc.size() * sizeof(real2)));
  return 0;
}

// full forward 2-D transform of a real source into S (used for the PSF and the TV gram)
int fft2_forward_setup(Engine* e, const RealSrc& src, real2* S, int nplanes) {
  const int zr0 = src.out_row0, zr1 = src.out_row0 + src.nrows;
  LPC_OK(rows_fwd_single(e, src, S, nplanes, -1));
  return cols_fwd_full(e, S, nplanes, zr0, zr1);
}
// the column half of it: row spectra in rows [zr0, zr1) of S (the others count as zero) -> full spectra, in place
int cols_fwd_full(Engine* e, real2* S, int nplanes, int zr0, int zr1) {
  if (e->plan.N1 > 1) {
    LPC_OK(cols_passA(e, S, nplanes, false, zr0, zr1, -1));
    return cols_passB_fwd(e, S, nplanes, 0, e->g.Hp);
  }
  return cols_passB_fwd(e, S, nplanes, zr0, zr1);
}

// planar real (padded or not) -> convolution with H / H* -> planar real, same kind
int convolve_planar(Engine* e, const real* xin, real* xout, int nplanes, bool padded_io, bool adjoint) {
  const PlaneGeom& g = e->g;
  if (padded_io) {
    LPC_OK(rows_fwd_single(e, src_padded(e, xin), e->S, nplanes, LPC_K_ROW_FWD));
    LPC_OK(conv_middle(e, e->S, nplanes, adjoint, 0, g.Hp));
    LPC_OK(rows_inv_single(e, e->S, dst_padded(e, xout), nplanes, LPC_K_ROW_INV));
  } else {
    LPC_OK(rows_fwd_single(e, src_unpadded(e, xin), e->S, nplanes, LPC_K_ROW_FWD));
    LPC_OK(conv_middle(e, e->S, nplanes, adjoint, g.sh, g.sh + g.H, true));
    LPC_OK(rows_inv_single(e, e->S, dst_cropped(e, xout), nplanes, LPC_K_ROW_INV));
  }
  return 0;
}

// ------------------------------------------------------------------ layout helpers --
int hwc_to_planar(Engine* e, const real* src, real* dst, int nimg, int rows, int cols, int pitch, long dplane,
                  int src_channels) {
  const long n = (long)rows * cols * e->cfg.channels;
  return launch_k(e, -1, k_hwc_to_planar<256>, grid1d(n, 256, nimg), 256, 0, src, dst, rows, cols,
                  e->cfg.channels, pitch, dplane, src_channels > 0 ? src_channels : e->cfg.channels);
}
// channel count of a caller's buffer: the handle's own, or 1 (broadcast) -- anything else would make the kernels
// read past the end of the buffer
int check_channels(const Engine* e, int ch, const char* who) {
  if (ch == e->cfg.channels || ch == 1) return 0;
  return fail(std::string(who) + ": buffer has " + std::to_string(ch) + " channel(s), the PSF " +
              std::to_string(e->cfg.channels) + " (only 1 -> C broadcasts)");
}
int planar_to_hwc(Engine* e, real* src, real* dst, int nimg, int rows, int cols, int pitch, long splane, int row0, int col0,
                  int clamp) {
  const long n = (long)rows * cols * e->cfg.channels;
  // clamp: 0 none, 1 everywhere, 2 inside the sensor window only (rows / cols then span the padded frame)
  const PlaneGeom& g = e->g;
  return launch_k(e, -1, k_planar_to_hwc<256>, grid1d(n, 256, nimg), 256, 0, src, dst, rows, cols,
                  e->cfg.channels, pitch, splane, row0, col0, clamp, 0, clamp == 2 ? g.sh : 0,
                  clamp == 2 ? g.sh + g.H : rows, clamp == 2 ? g.sw : 0, clamp == 2 ? g.sw + g.W : cols);
}
// two padded planar arrays (component 0 / 1) -> channels-last with a trailing axis of 2
int planar2_to_hwc2(Engine* e, const real* a0, const real* a1, real* dst, int nimg) {
  const PlaneGeom& g = e->g;
  const long n = (long)g.Hp * g.Wp * e->cfg.channels;
  return launch_k(e, -1, k_planar2_to_hwc2<256>, grid1d(n, 256, nimg), 256, 0, a0, a1, dst, g.Hp, g.Wp, e->cfg.channels,
                  g.rpitch, g.rplane);
}
int fill_planar(Engine* e, real* p, long n, real v) {
  return launch_k(e, -1, k_fill<256>, grid1d(n, 256), 256, 0, p, n, v);
}
// (max, min) per (plane, block) of |H* H| of spectrum planes (Hs) or of un-padded image planes (plane)
int plane_minmax(Engine* e, const real2* Hs, const real* plane, int nblk, int nplanes, real* partial) {
  return launch_k(e, -1, k_plane_minmax<256>, dim3(nblk, nplanes), 256, 2 * 256 * sizeof(real), e->g, Hs, plane, Hs ? 0 : 1,
                  partial);
}

// ------------------------------------------------------------ workspace, PSF, operator --
int alloc_common(Engine* e) {
  const PlaneGeom& g = e->g;
  LPC_OK(dev_alloc(e, &e->Hs, (size_t)g.cplane * e->Ppsf));
  LPC_OK(dev_alloc(e, &e->psf_planar, (size_t)g.uplane * e->Ppsf));
  e->psf_cap = e->Ppsf;
  const int nspec = e->cfg.algo == LPC_ALGO_ADMM ? 2 : 1;
  LPC_OK(dev_alloc(e, &e->S, (size_t)g.cplane * e->P * nspec));
  if (e->cfg.algo != LPC_ALGO_CONV) return dev_alloc(e, &e->Y, (size_t)g.uplane * e->Pdata);
  const size_t n = (size_t)(e->cfg.pad ? g.uplane : g.rplane) * e->P;
  LPC_OK(dev_alloc(e, &e->conv_in, n));
  return dev_alloc(e, &e->conv_out, n);
}

// The handle holds n PSF planes from here on and addresses H by state plane q % n (PlaneGeom::PM): D*C planes, one PSF
// for the batch, or batch*D*C, one per frame.  More planes than there is room for: Hs, psf_planar and ADMM's copies are
// given back and allocated again for n planes (once per handle: they do not shrink).  The reverse modes read the PSF
// through the same launches as the forward (convolve_planar, conv_middle, admm_spectral_plain) and through
// k_admm_bwd_psf_acc / k_admm_bwd_psf_acc_frames, chosen by psf_per_frame: nothing else holds a plane count of its own
static int psf_planes(Engine* e, int n) {
  const PlaneGeom& g = e->g;
  if (n > e->psf_cap) {
    e->psf_set = false;
    dev_free(e, e->Hs); dev_free(e, e->psf_planar);
    e->Hs = nullptr; e->psf_planar = nullptr;
    e->psf_cap = 0;
    LPC_OK(dev_alloc(e, &e->Hs, (size_t)g.cplane * n));
    LPC_OK(dev_alloc(e, &e->psf_planar, (size_t)g.uplane * n));
    if (e->cfg.algo == LPC_ALGO_ADMM) LPC_OK(admm_alloc_psf(e, n));
    e->psf_cap = n;
  }
  e->Ppsf = n;
  e->g.PM = n;
  return 0;
}

// nimg PSFs (D,H,W,C) each -> planar [nimg*D*C][H][W] -> their spectra, norm applied (+ the pair-line copy): one launch
// sequence for all of them
static int psf_spectra(Engine* e, const real* dev_psf, int npsf);

int set_psf(Engine* e, const real* dev_psf) {
  LPC_OK(psf_planes(e, e->g.DC));
  e->psf_per_frame = false;
  return psf_spectra(e, dev_psf, 1);
}
int set_psf_batch(Engine* e, const real* dev_psfs) {
  LPC_OK(psf_planes(e, e->P));
  e->psf_per_frame = true;
  return psf_spectra(e, dev_psfs, e->cfg.batch);
}

static int psf_spectra(Engine* e, const real* dev_psf, int npsf) {
  const PlaneGeom& g = e->g;
  LPC_OK(hwc_to_planar(e, dev_psf, e->psf_planar, npsf * e->cfg.depth, g.H, g.W, g.W, g.uplane));
  LPC_OK(fft2_forward_setup(e, src_unpadded(e, e->psf_planar), e->Hs, e->Ppsf));
  double sc = 1.0;  // rfft_convolve.py:121 norm= of the PSF spectrum
  if (e->cfg.norm == LPC_NORM_ORTHO) sc = 1.0 / std::sqrt((double)g.Hp * (double)g.Wp);
  if (e->cfg.norm == LPC_NORM_FORWARD) sc = 1.0 / ((double)g.Hp * (double)g.Wp);
  if (sc != 1.0) {
    const long n = (long)g.cplane * e->Ppsf;
    LPC_OK(launch_k(e, -1, k_scale_complex<256>, grid1d(n, 256), 256, 0, e->Hs, n, (real)sc));
  }
  e->psf_set = true;
  if (g.slay)
    LPC_OK(launch_k(e, -1, k_to_pair_lines<256, real2>, grid1d((long)g.Hp * g.cpitch, 256, e->Ppsf), 256, 0,
                    (const real2*)e->Hs, e->admm.Hs_t, g.Hp, g.cpitch, g.cplane));
  return 0;
}

// the bare operator on channels-last frames: H x / H* x, or (spectrum) rfft2(x) * H as channels-last complex
int convolve_hwc(Engine* e, const real* dev_x, real* dev_out, int n, int x_channels, bool adjoint, bool spectrum) {
  const PlaneGeom& g = e->g;
  const int nplanes = n * g.DC, nimg = n * e->cfg.depth;
  const bool padded_io = !e->cfg.pad;
  real *xin = e->conv_in, *xout = e->conv_out;
  if (padded_io) LPC_OK(hwc_to_planar(e, dev_x, xin, nimg, g.Hp, g.Wp, g.rpitch, g.rplane, x_channels));
  else LPC_OK(hwc_to_planar(e, dev_x, xin, nimg, g.H, g.W, g.W, g.uplane, x_channels));
  if (spectrum) {
    LPC_OK(fft2_forward_setup(e, padded_io ? src_padded(e, xin) : src_unpadded(e, xin), e->S, nplanes));
    return launch_k(e, -1, k_spectrum_mul_to_hwc<256>, grid1d((long)g.Hp * g.Wc * g.C, 256, nimg), 256, 0, g,
                    (const real2*)e->S, (const real2*)e->Hs, adjoint ? 1 : 0, (real2*)dev_out, e->plan.N1, e->plan.N2);
  }
  LPC_OK(convolve_planar(e, xin, xout, nplanes, padded_io, adjoint));
  if (padded_io) return planar_to_hwc(e, xout, dev_out, nimg, g.Hp, g.Wp, g.rpitch, g.rplane, 0, 0, 0);
  return planar_to_hwc(e, xout, dev_out, nimg, g.H, g.W, g.W, g.uplane, 0, 0, 0);
}
