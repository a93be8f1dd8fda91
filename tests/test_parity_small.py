"""
Parity of the engine with (a) the golden vectors produced by the REAL reference and (b) the
pinned CPU oracle, on small frames.  Every case runs twice: on the SIMT emulator in the
default CPU suite ('emu' -- same kernel sources, executed on the host) and on the MI355X
through the product library ('hip', -m gpu).

Float32 tolerances, relative to max|reference|:
  operator <= 2e-6;  ADMM after 5 / 20 / 50 iterations <= 5e-6 / 1e-5 / 5e-5;
  GD family <= 5e-6 up to 20 iterations, 5e-5 after 60.
The engine uses the 4-FFT form of ADMM and its own FFT, so agreement is to round-off, not
bit-exact; iteration counts are exact by construction (no early exit exists).
"""
import glob
import os

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from oracle import lensless_oracle as orc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def engine_opts(monkeypatch, **kw):
    """Launch-plan options (include/lpc.h, lpc_config.options) for every solver built during this test: the package's
    default-options table is patched, the process environment is never touched."""
    from lenslesspicam_amd import _native

    new = {**_native.DEFAULT_OPTIONS, **kw}
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {k: v for k, v in new.items() if v is not None})


def rel(a, b):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    if isinstance(b, torch.Tensor):
        b = b.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# --------------------------------------------------------------------------- operator --
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_convolver_golden(backend, tag):
    g = np.load(os.path.join(GOLDEN, "operators.npz"))
    psf, x = g[f"{tag}_psf"], g[f"{tag}_x"]
    for norm in ("ortho", "backward"):
        cv = lpa.RealFFTConvolve2D(psf, pad=True, norm=norm)
        assert cv._padded_shape == [int(v) for v in g[f"{tag}_padded_shape"]]
        assert list(cv._start_idx) == list(g[f"{tag}_start"])
        assert rel(cv.convolve(x), g[f"{tag}_{norm}_conv"]) <= 2e-6
        assert rel(cv.deconvolve(x), g[f"{tag}_{norm}_deconv"]) <= 2e-6
        assert np.array_equal(cv._pad(x), g[f"{tag}_{norm}_pad"])
        assert np.array_equal(cv._crop(cv._pad(x)), x)          # test/test_convolver.py:11-29
    cvn = lpa.RealFFTConvolve2D(psf, pad=False, norm="backward")
    assert rel(cvn.convolve(g[f"{tag}_xp"]), g[f"{tag}_nopad_conv"]) <= 2e-6
    assert rel(cvn.deconvolve(g[f"{tag}_xp"]), g[f"{tag}_nopad_deconv"]) <= 2e-6


def test_convolver_return_fft_golden(backend):
    """convolve / deconvolve(return_fft=True): the spectrum rfft2(pad(x)) * H resp. * conj(H) in the reference's layout
    (natural frequency order, channels last) although the engine keeps spectra planar in a permuted row order
    (lpc_convolve_spectrum); golden vectors from the reference's own calls (rfft_convolve.py:148-150,193-195)."""
    g = np.load(os.path.join(GOLDEN, "return_fft.npz"))
    for tag in ("a", "b"):
        psf, x, xp = g[f"{tag}_psf"], g[f"{tag}_x"], g[f"{tag}_xp"]
        for norm in ("ortho", "backward"):
            cv = lpa.RealFFTConvolve2D(psf, pad=True, norm=norm)
            for name, fn in (("conv", cv.convolve), ("deconv", cv.deconvolve)):
                got, want = fn(x, return_fft=True), g[f"{tag}_{norm}_{name}_fft"]
                assert got.shape == want.shape and np.iscomplexobj(got)
                assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max(), (tag, norm, name)
        cvn = lpa.RealFFTConvolve2D(torch.from_numpy(psf), pad=False, norm="backward")
        got = cvn.convolve(torch.from_numpy(xp), return_fft=True)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.complex64
        assert np.abs(got.cpu().numpy() - g[f"{tag}_nopad_conv_fft"]).max() <= 2e-6 * np.abs(g[f"{tag}_nopad_conv_fft"]).max()
        got = cvn.deconvolve(torch.from_numpy(xp), return_fft=True).cpu().numpy()
        assert np.abs(got - g[f"{tag}_nopad_deconv_fft"]).max() <= 2e-6 * np.abs(g[f"{tag}_nopad_deconv_fft"]).max()
    # a frame with a four-step column split (stored rows permuted): natural order must still come back
    psf = orc.synthetic_psf(1, 48, 20, 1, seed=2)
    x = np.random.default_rng(3).standard_normal((1, 1, 48, 20, 1)).astype(np.float32)
    cv = lpa.RealFFTConvolve2D(psf, pad=True, norm="backward", engine_options={"tile_budget": 512, "col_t": 4, "split_n2": 12})
    assert "split" in cv._handle.plan_info()
    xpad = np.zeros((1, 1, 96, 40, 1), np.float32)
    xpad[:, :, 24:72, 10:30] = x
    ppad = np.zeros((1, 96, 40, 1), np.float32)
    ppad[:, 24:72, 10:30] = psf
    want = np.fft.rfft2(xpad.astype(np.float64), axes=(-3, -2)) * np.fft.rfft2(ppad.astype(np.float64), axes=(-3, -2))
    got = cv.convolve(x, return_fft=True)
    assert np.abs(got - want).max() <= 5e-6 * np.abs(want).max()


def test_convolver_slice_commutes(backend):
    """test/test_convolver.py:32-59: no cross-batch / cross-depth / cross-channel coupling."""
    rng = np.random.default_rng(0)
    psf = torch.from_numpy(rng.random((5, 47, 29, 3), dtype=np.float32))
    data = torch.from_numpy(rng.random((6, 1, 47, 29, 3), dtype=np.float32))
    cv = lpa.RealFFTConvolve2D(psf, pad=True)
    full = cv.convolve(data)
    assert isinstance(full, torch.Tensor) and full.shape == (6, 5, 47, 29, 3)
    part = cv.convolve(data[:1])
    torch.testing.assert_close(full[:1], part, rtol=0, atol=0)  # frames are independent: identical bits
    psf1 = psf[:1].contiguous()
    cv1 = lpa.RealFFTConvolve2D(psf1, pad=True)
    torch.testing.assert_close(cv1.convolve(data[:2])[:, 0], full[:2, 0], rtol=0, atol=0)


def test_convolver_adjointness(backend):
    """<H x, y> == <x, H^T y>: a size-independent property of the operator pair.  It holds for
    EVEN padded sizes only (ifftshift is then an involution that commutes with the circular
    convolution); for odd sizes the reference's deconvolve is not the exact adjoint either."""
    rng = np.random.default_rng(1)
    psf = rng.random((1, 24, 32, 3), dtype=np.float32)
    x = rng.standard_normal((1, 1, 24, 32, 3)).astype(np.float32)
    y = rng.standard_normal((1, 1, 24, 32, 3)).astype(np.float32)
    cv = lpa.RealFFTConvolve2D(psf, pad=True, norm="ortho")
    lhs = float(np.sum(cv.convolve(x).astype(np.float64) * y))
    rhs = float(np.sum(x * cv.deconvolve(y).astype(np.float64)))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs), 1.0)


# -------------------------------------------------------------------------------- ADMM --
ADMM_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "admm_*.npz")))
ADMM_TOL = {1: 2e-6, 2: 2e-6, 5: 5e-6, 10: 1e-5, 20: 1e-5, 50: 5e-5}
F64_TOL = 1e-11   # dtype="float64" (liblpc_f64: the same kernels compiled over double)


@pytest.mark.parametrize("name", ADMM_CASES)
def test_admm_matches_reference_golden(backend, name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    mu1, mu2, mu3, tau = [float(v) for v in g["params"]]
    kw = dict(mu1=mu1, mu2=mu2, mu3=mu3, tau=tau)
    f64 = str(g["dtype"]) == "float64"
    if f64:
        kw["dtype"] = "float64"
    if "initial_est" in g:
        kw["initial_est"] = g["initial_est"].copy()
    rec = lpa.ADMM(g["psf"].astype(np.float64) if f64 else g["psf"], **kw)
    assert rec._padded_shape == [int(v) for v in g["padded_shape"]]
    rec.set_data(g["data"].astype(np.float64) if f64 else g["data"])
    bg = g["background"] if "background" in g else None
    # reset (+ background subtraction) through the public entry, then step WITHOUT _form_image in
    # between: the golden snapshots were taken by calling _update() directly, and _form_image clamps
    # the state in place (admm.py:331-338), which the engine reproduces (see the two-stage check below)
    rec.apply(n_iter=0, disp_iter=None, plot=False, background=bg)
    done = 0
    for n in [int(i) for i in g["iters"]]:
        rec._iterate(n - done)
        done = n
        for key, attr in (("V", "_image_est"), ("X", "_X"), ("W", "_W"), ("U", "_U"), ("xi", "_xi"),
                          ("eta", "_eta"), ("rho", "_rho"), ("HV", "_forward_out")):
            ref = g[f"it{n}_{key}"]
            got = getattr(rec, attr)
            if np.max(np.abs(ref)) == 0:
                assert float(np.abs(got).max()) == 0.0, (key, n)
            else:
                tol = ADMM_TOL[n] * (10 if key in ("eta", "rho", "U") else 1)  # duals sit 5 decades below V
                tol = F64_TOL * (100 if key in ("eta", "rho", "U", "xi") else 1) if f64 else tol
                assert got.dtype == (np.float64 if f64 else np.float32)
                assert rel(got, ref) <= tol, (key, n, rel(got, ref))
    res = rec.get_image_estimate()[0]
    assert isinstance(res, np.ndarray) and res.dtype == (np.float64 if f64 else np.float32)
    assert res.shape == g["psf"].shape
    assert rel(res, g["final"]) <= (F64_TOL if f64 else ADMM_TOL[done])
    if "two_stage" in g:
        # apply(n1) then apply(n2, reset=False): the clamp at the end of the first apply() is an in-place
        # side effect in the reference and changes the continuation; the engine must follow it
        n1, n2 = [int(v) for v in g["two_stage"]]
        two = lpa.ADMM(g["psf"], **kw)
        two.set_data(g["data"])
        two.apply(n_iter=n1, disp_iter=None, plot=False)
        cont = two.apply(n_iter=n2, disp_iter=None, plot=False, reset=False)
        assert rel(cont, g["two_stage_final"]) <= 1e-5


def test_admm_vs_oracle_odd_and_gray(backend):
    rng = np.random.default_rng(3)
    psf = orc.synthetic_psf(1, 21, 13, 1, seed=3)          # pads to 45 x 25: odd x odd
    data = rng.random((21, 13, 1), dtype=np.float32)
    rec = lpa.ADMM(torch.from_numpy(psf), tau=1e-6, mu2=5e-5)
    assert rec._padded_shape[1] % 2 == 1 and rec._padded_shape[2] % 2 == 1
    rec.set_data(torch.from_numpy(data))
    res = rec.apply(n_iter=15, disp_iter=None)
    o = orc.ADMMOracle(psf, tau=1e-6, mu2=5e-5)
    o.set_data(data)
    assert isinstance(res, torch.Tensor) and res.dtype == torch.float32
    assert rel(res, o.apply(15)) <= 1e-5


def test_admm_batch_equals_singles(backend):
    """Config 4's contract: a batch equals B independent apply() calls."""
    rng = np.random.default_rng(4)
    psf = orc.synthetic_psf(1, 16, 20, 3, seed=4)
    frames = rng.random((3, 16, 20, 3), dtype=np.float32)
    rec = lpa.ADMM(psf, tau=2e-6, mu2=1e-4)
    rec.set_data(frames[:, None])
    batch = rec.apply_batch(n_iter=8)
    assert batch.shape == (3, 1, 16, 20, 3)
    for b in range(3):
        single = lpa.ADMM(psf, tau=2e-6, mu2=1e-4)
        single.set_data(frames[b])
        assert np.array_equal(single.apply(n_iter=8, disp_iter=None), batch[b])


def test_admm_depth_planes_are_independent(backend):
    """Row A9: D > 1 = D independent problems sharing the measurement; oracle = per-plane loop."""
    rng = np.random.default_rng(5)
    psf = orc.synthetic_psf(3, 12, 18, 3, seed=5)
    data = rng.random((12, 18, 3), dtype=np.float32)
    rec = lpa.ADMM(psf, tau=2e-6, mu2=1e-4)
    rec.set_data(data)
    res = rec.apply(n_iter=10, disp_iter=None)
    assert res.shape == (3, 12, 18, 3)
    for d in range(3):
        o = orc.ADMMOracle(psf[d:d + 1], tau=2e-6, mu2=1e-4)
        o.set_data(data)
        assert rel(res[d], o.apply(10)[0]) <= 1e-5


def test_unrolled_admm_matches_reference_golden(backend):
    """Row N1: UnrolledADMM.forward (reference: lensless/recon/unrolled_admm.py) on a batch of 3 with a
    different (mu1, mu2, mu3, tau) in each of the 6 iterations."""
    g = np.load(os.path.join(GOLDEN, "unrolled_admm_24x32x3_b3.npz"))
    n = int(g["n_iter"])
    rec = lpa.UnrolledADMM(torch.from_numpy(g["psf"]), n_iter=n, mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-6)
    rec.set_parameters(mu1=g["mu1"], mu2=g["mu2"], mu3=g["mu3"], tau=g["tau"])
    out = rec.forward(torch.from_numpy(g["data"]))
    assert out.shape == g["out"].shape
    assert rel(out, g["out"]) <= 5e-6
    # constant schedule == plain ADMM
    const = lpa.UnrolledADMM(torch.from_numpy(g["psf"]), n_iter=n, mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-6)
    plain = lpa.ADMM(torch.from_numpy(g["psf"]), mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-6)
    plain.set_data(torch.from_numpy(g["data"]))
    torch.testing.assert_close(const.forward(torch.from_numpy(g["data"])), plain.apply_batch(n_iter=n), rtol=0, atol=0)


def test_unrolled_fista_matches_reference_golden(backend):
    """Row N1: UnrolledFISTA.forward (lensless/recon/unrolled_fista.py) with per-iteration, per-channel
    steps and a perturbed t_k sequence on a batch of 3."""
    g = np.load(os.path.join(GOLDEN, "unrolled_fista_24x32x3_b3.npz"))
    n = int(g["n_iter"])
    rec = lpa.UnrolledFISTA(torch.from_numpy(g["psf"]), n_iter=n)
    assert rel(rec._alpha_p[0], lpa.FISTA(torch.from_numpy(g["psf"]))._alpha) <= 1e-7
    rec.set_parameters(alpha=g["alpha"], tk=g["tk"])
    out = rec.forward(torch.from_numpy(g["data"]))
    assert out.shape == g["out"].shape
    assert rel(out, g["out"]) <= 5e-6


# --------------------------------------------------------------------------- GD family --
GD_CLASSES = {"gd": lpa.GradientDescent, "nesterov": lpa.NesterovGradientDescent, "fista": lpa.FISTA}
GD_CASES = sorted(
    os.path.basename(p)[:-4]
    for p in glob.glob(os.path.join(GOLDEN, "*.npz"))
    if os.path.basename(p).split("_")[0] in GD_CLASSES
)


@pytest.mark.parametrize("name", GD_CASES)
def test_gd_family_matches_reference_golden(backend, name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    cls = GD_CLASSES[name.split("_")[0]]
    kw = {}
    if name.endswith("_tk"):
        kw["tk"] = 2.5
    if name.endswith("_mu"):
        kw["mu"] = 0.7
    if "initial_est" in g:
        kw["initial_est"] = g["initial_est"].copy()
    f64 = str(g["dtype"]) == "float64"
    if f64:
        kw["dtype"] = "float64"
    rec = cls(g["psf"].astype(np.float64) if f64 else g["psf"], **kw)
    rec.set_data(g["data"].astype(np.float64) if f64 else g["data"])
    assert rel(rec._alpha, g["alpha"]) <= (F64_TOL if f64 else 2e-6)
    assert rel(rec._image_est, g["x0"]) <= 1e-7
    done = 0
    for n in [int(i) for i in g["iters"]]:
        rec.apply(n_iter=n - done, disp_iter=None, reset=(done == 0))
        done = n
        r = rel(rec._image_est, g[f"it{n}_x"])
        assert r <= (F64_TOL if f64 else (5e-6 if n <= 20 else 5e-5)), (n, r)
    out = rec.get_image_estimate()[0]
    assert out.dtype == (np.float64 if f64 else np.float32)       # test/test_algos.py:107: res.dtype == psf.dtype
    assert rel(out, g["final"]) <= (F64_TOL if f64 else 5e-5)


@pytest.mark.parametrize("shape", [(10, 64, 3), (5, 512, 1)])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_rows_with_radix2_tail_fold_it_into_the_tangling(backend, shape, dtype):
    """Padded widths 128 = 8*8*2 and 1024 = 8*8*8*2: the row plans end in a radix-2 stage, which
    the row kernels fold into the Hermitian (un)tangling (untangle_r2_store / tangle_r2_load).  Checked
    against the oracle for the operator pair, ADMM (incl. dual state) and all three GD variants."""
    H, W, C = shape
    tdt = torch.float32 if dtype == "float32" else torch.float64
    tol = 5e-6 if dtype == "float32" else 1e-11
    rng = np.random.default_rng(H * W)
    psf = orc.synthetic_psf(1, H, W, C, seed=H + W).astype(dtype)
    y = rng.random((H, W, C)).astype(dtype)
    x = rng.standard_normal((2, 1, H, W, C)).astype(dtype)
    cv = lpa.RealFFTConvolve2D(psf, dtype=dtype, pad=True)
    oc = orc.ConvolverOracle(psf, dtype=tdt, pad=True)
    assert cv._padded_shape[2] in (128, 1024)
    assert rel(cv.convolve(x), oc.convolve(torch.from_numpy(x))) <= tol
    assert rel(cv.deconvolve(x), oc.deconvolve(torch.from_numpy(x))) <= tol
    rec = lpa.ADMM(psf, dtype=dtype, tau=2e-6, mu2=1e-4)
    rec.set_data(y)
    o = orc.ADMMOracle(psf, dtype=tdt, tau=2e-6, mu2=1e-4)
    o.set_data(y)
    got = rec.apply(n_iter=6, disp_iter=None)
    assert got.dtype == np.dtype(dtype)
    ref = o.apply(6)
    assert rel(got, ref) <= 2 * tol
    assert rel(rec._xi, o.xi) <= 40 * tol and rel(rec._X, o.X) <= 4 * tol
    for kind, cls in (("vanilla", lpa.GradientDescent), ("nesterov", lpa.NesterovGradientDescent),
                      ("fista", lpa.FISTA)):
        g = cls(psf, dtype=dtype)
        g.set_data(y)
        og = orc.GDOracle(psf, kind=kind, dtype=tdt)
        og.set_data(y)
        assert rel(g.apply(n_iter=8, disp_iter=None), og.apply(8)) <= 2 * tol, kind


@pytest.mark.parametrize("h,hp,n2", [(48, 96, 48), (48, 96, 12), (48, 96, 24), (48, 96, 32), (60, 120, 30),
                                     (60, 120, 40), (54, 108, 36)])
def test_forced_four_step_column_split(backend, monkeypatch, h, hp, n2):
    """The split column passes (pass A + fused middle + inverse pass A) normally start at ~1000 padded rows;
    tuning knobs force them on ~100-row padded frames so that the CPU suite executes those kernels too:
    every pass-B length that has a register-resident middle (48, 40, 36, 32, 30, 24) and one that takes the
    LDS middle (12)."""
    engine_opts(monkeypatch, tile_budget=512)
    engine_opts(monkeypatch, col_t=4)
    engine_opts(monkeypatch, split_n2=int(n2))
    psf = orc.synthetic_psf(1, h, 20, 3, seed=8)
    y = np.random.default_rng(8).random((h, 20, 3), dtype=np.float32)
    rec = lpa.ADMM(torch.from_numpy(psf), tau=2e-6, mu2=1e-4)
    assert rec._padded_shape[1] == hp
    rec.set_data(torch.from_numpy(y))
    o = orc.ADMMOracle(psf, tau=2e-6, mu2=1e-4)
    o.set_data(y)
    assert rel(rec.apply(n_iter=6, disp_iter=None), o.apply(6)) <= 5e-6
    fis = lpa.FISTA(torch.from_numpy(psf))
    fis.set_data(torch.from_numpy(y))
    of = orc.GDOracle(psf, kind="fista")
    of.set_data(y)
    assert rel(fis.apply(n_iter=6, disp_iter=None), of.apply(6)) <= 5e-6
    conv = lpa.RealFFTConvolve2D(torch.from_numpy(psf))
    x = torch.from_numpy(np.random.default_rng(9).random((1, h, 20, 3), dtype=np.float32))
    assert rel(conv.deconvolve(x), of.conv.deconvolve(x)) <= 2e-6


@pytest.mark.parametrize("static", [False, True], ids=["runtime_plan", "plan_module"])
@pytest.mark.parametrize("name", ["admm_24x32x3_tv", "admm_47x29x3_tv", "admm_24x32x3_init_bg", "admm_24x32x3_default",
                                  "admm_24x32x1_f64"])
def test_admm_half_length_row_kernels(backend, monkeypatch, name, static):
    """ADMM's row passes switch to one real row per half-length complex transform for wide frames only; the option
    rows_half=1 forces them on the golden-vector sizes (row transforms of 32 and 30 points, the second one without the
    LDS skew): same trajectory checks as the regular golden test.  `static`: the same frames through a plan module
    compiled for them (jit_min_points=0) -- 47x29 pads to 60 columns, not a multiple of 4, so its module keeps the
    stand-alone image-domain kernel; 24x32 runs the X half inside the forward rows."""
    engine_opts(monkeypatch, rows_half=1, jit_min_points=0 if static else None)
    test_admm_matches_reference_golden(backend, name)


@pytest.mark.parametrize("name", ["gd_24x32x3", "nesterov_24x32x3", "fista_24x32x3", "fista_47x29x3_d3",
                                  "fista_24x32x1_f64"])
def test_gd_family_half_length_row_kernels(backend, monkeypatch, name):
    """Same for the gradient-descent family: pad-on-load forward rows, the irfft -> residual -> rfft kernel and the
    fused update, each with one real row per half-length transform (k_rfwd_rows_half, k_rinv_gd_mid_half,
    k_rinv_gd_update_half), float32 and float64, depth 3, 32- and 30-point row transforms."""
    engine_opts(monkeypatch, rows_half=1)
    test_gd_family_matches_reference_golden(backend, name)


def test_convolver_half_length_row_kernels(backend, monkeypatch):
    engine_opts(monkeypatch, rows_half=1)
    for tag in ("a", "b", "c"):
        test_convolver_golden(backend, tag)
    test_convolver_slice_commutes(backend)


@pytest.mark.parametrize("static", [True, False], ids=["static_plan", "runtime_plan"])
def test_8192_column_rows_static_plan(backend, monkeypatch, static):
    """12 MP's ROW shape on a frame with only a few rows: 4096 columns pad to 8192, the half-row transform has 4096
    points = 8.8.8.8, which is served by kernels instantiated on a compile-time plan (lpc_sfft.h) -- ADMM through the
    X-half row kernel, the gradient-descent family's residual / update kernels, and the convolver's
    pad-on-load / crop-on-store rows, all from the frame's plan module.  no_static=1 runs the same frame through the
    run-time plans."""
    engine_opts(monkeypatch, jit_min_points=0, no_static=0 if static else 1)
    H, W, C = 3, 4096, 1
    rng = np.random.default_rng(11)
    psf = orc.synthetic_psf(1, H, W, C, seed=4)
    y = rng.random((H, W, C), dtype=np.float32)
    rec = lpa.ADMM(torch.from_numpy(psf), tau=2e-6, mu2=1e-4)
    assert rec._padded_shape == [1, 5, 8192, 1]
    rec.set_data(torch.from_numpy(y))
    o = orc.ADMMOracle(psf, dtype=torch.float64, tau=2e-6, mu2=1e-4)
    o.set_data(y)
    assert rel(rec.apply(n_iter=4, disp_iter=None), o.apply(4)) <= 5e-6
    fis = lpa.FISTA(torch.from_numpy(psf))
    fis.set_data(torch.from_numpy(y))
    of = orc.GDOracle(psf, kind="fista", dtype=torch.float64)
    of.set_data(y)
    assert rel(fis.apply(n_iter=4, disp_iter=None), of.apply(4)) <= 5e-6
    cv = lpa.RealFFTConvolve2D(torch.from_numpy(psf), pad=True)
    oc = orc.ConvolverOracle(psf, pad=True)
    x = torch.from_numpy(rng.standard_normal((1, 1, H, W, C)).astype(np.float32))
    assert rel(cv.convolve(x), oc.convolve(x)) <= 2e-6
    assert rel(cv.deconvolve(x), oc.deconvolve(x)) <= 2e-6


@pytest.mark.parametrize("static", [True, False], ids=["static_plan", "runtime_plan"])
def test_6144_row_columns_static_plan(backend, monkeypatch, static):
    """12 MP's COLUMN shape on a frame only 9 columns wide: 3072 rows pad to 6144 = 96 x 64 for ADMM (pass A 96 points =
    8.4.3, fused middle 64 points = 8.8 over both spectra) and 128 x 48 for the gradient-descent family (pass A 8.8.2,
    48-point middle in registers), 16-column tiles -- on compile-time plans; no_static=1 is the same frame on the
    run-time plans."""
    engine_opts(monkeypatch, jit_min_points=0, no_static=0 if static else 1)
    H, W, C = 3072, 9, 1
    rng = np.random.default_rng(12)
    psf = orc.synthetic_psf(1, H, W, C, seed=5)
    y = rng.random((H, W, C), dtype=np.float32)
    rec = lpa.ADMM(torch.from_numpy(psf), tau=2e-6, mu2=1e-4)
    assert rec._padded_shape == [1, 6144, 18, 1]
    rec.set_data(torch.from_numpy(y))
    o = orc.ADMMOracle(psf, dtype=torch.float64, tau=2e-6, mu2=1e-4)
    o.set_data(y)
    assert rel(rec.apply(n_iter=3, disp_iter=None), o.apply(3)) <= 5e-6
    fis = lpa.FISTA(torch.from_numpy(psf))
    fis.set_data(torch.from_numpy(y))
    of = orc.GDOracle(psf, kind="fista", dtype=torch.float64)
    of.set_data(y)
    assert rel(fis.apply(n_iter=3, disp_iter=None), of.apply(3)) <= 5e-6


def _admm_fista_vs_oracle(H, W, C, padded, n_admm=3, n_fista=3, seed=13, tol=5e-6):
    rng = np.random.default_rng(seed)
    psf = orc.synthetic_psf(1, H, W, C, seed=seed)
    y = rng.random((H, W, C), dtype=np.float32)
    rec = lpa.ADMM(torch.from_numpy(psf), tau=2e-6, mu2=1e-4)
    assert rec._padded_shape[1:3] == list(padded)
    rec.set_data(torch.from_numpy(y))
    o = orc.ADMMOracle(psf, dtype=torch.float64, tau=2e-6, mu2=1e-4)
    o.set_data(y)
    assert rel(rec.apply(n_iter=n_admm, disp_iter=None), o.apply(n_admm)) <= tol
    fis = lpa.FISTA(torch.from_numpy(psf))
    fis.set_data(torch.from_numpy(y))
    of = orc.GDOracle(psf, kind="fista", dtype=torch.float64)
    of.set_data(y)
    assert rel(fis.apply(n_iter=n_fista, disp_iter=None), of.apply(n_fista)) <= tol


@pytest.mark.parametrize("static", [True, False], ids=["static_plan", "runtime_plan"])
@pytest.mark.parametrize("shape,padded", [((3, 1920, 1), (5, 3840)), ((1080, 9, 1), (2160, 18)),
                                          ((270, 480, 1), (540, 960)), ((3, 1014, 1), (5, 2048)),
                                          ((760, 9, 1), (1536, 18)), ((3, 2028, 1), (5, 4096))],
                         ids=["rows1920", "cols90x24", "c1_540x960", "rows2048", "cols64x24", "rows2048half"])
def test_other_baseline_shapes_static_plans(backend, monkeypatch, static, shape, padded):
    """The remaining BASELINE shapes with compile-time plans, each on a frame that keeps the emulator fast:
    1080p's half rows (1920 = 8.8.6.5; ADMM through the fused image-domain + row kernel), its column split
    2160 = 90 x 24 (pass A 90 = 6.5.3 + the register-resident 24-point middle), and the DiffuserCam-sized frame of
    C1 / C4 in full (single-pass 540-point ADMM middle = 6.6.5.3 over 2 x 8 tile columns, paired 960-point rows)."""
    engine_opts(monkeypatch, jit_min_points=0, no_static=0 if static else 1)
    _admm_fista_vs_oracle(*shape, padded, n_admm=2 if shape[0] == 270 else 3, n_fista=2 if shape[0] == 270 else 3)
    psf = orc.synthetic_psf(1, *shape, seed=1)
    info = lpa.ADMM(torch.from_numpy(psf))._handle.plan_info() + " | " + lpa.FISTA(torch.from_numpy(psf))._handle.plan_info()
    assert ("[static" in info) == static, info        # the plan tables really matched (no silent run-time fallback)


@pytest.mark.parametrize("shape", [(270, 480, 1), (3, 1014, 1)], ids=["paired960", "paired2048"])
def test_xi_outside_the_sensor_window(backend, monkeypatch, shape):
    """Outside the sensor window X_divmat = 1/mu1, so a = mu1 X - xi = mu1 HV and xi' = mu1 (HV' - HV): the X half
    of the forward rows skips xi / HV_old there on all but the last iteration of a call (AdmmScalars::xiw).  Every
    read-out between calls must still see the reference's xi and X on the WHOLE padded frame, multi-iteration calls
    must equal single-iteration calls, and the image must stay on the full-xi path's (option xi_full) to round-off."""
    H, W, C = shape
    # (hv_full: the H V row transforms run on every row, so that calls of any length are the same instruction stream;
    # the plan that also skips those outside the window is compared at the end and in the next test)
    # (k1_half=0 likewise: with the duals half-applied between the iterations of a call, a 4-iteration call and four
    # 1-iteration calls round the dual updates differently; the default plan is compared at the end)
    engine_opts(monkeypatch, jit_min_points=0, hv_full=1, k1_half=0)
    rng = np.random.default_rng(8)
    psf = orc.synthetic_psf(1, H, W, C, seed=8)
    y = rng.random((H, W, C), dtype=np.float32)
    o = orc.ADMMOracle(psf, dtype=torch.float64, tau=2e-6, mu2=1e-4)
    o.set_data(y)
    o.reset()
    for _ in range(4):
        o.step()                                      # (no _form_image: it clamps V in place)

    def run(steps):
        rec = lpa.ADMM(torch.from_numpy(psf), tau=2e-6, mu2=1e-4)
        assert "X half" in rec._handle.plan_info()
        rec.set_data(torch.from_numpy(y))
        rec.apply(n_iter=0, disp_iter=None, plot=False)
        for n in steps:
            rec._iterate(n)
        return rec, np.asarray(rec._xi).copy(), np.asarray(rec._X).copy(), np.asarray(rec._image_est).copy()

    rec, xi4, x4, v4 = run([4])                       # one call: three iterations never store xi outside the window
    _, xi1, x1, v1 = run([1, 1, 1, 1])                # four calls: every iteration stores it
    scale = float(np.abs(o.xi.numpy()).max())
    assert scale > 0
    assert np.abs(xi4 - o.xi.numpy()).max() <= 2e-5 * scale and np.abs(xi1 - o.xi.numpy()).max() <= 2e-5 * scale
    assert rel(x4, o.X.numpy()) <= 5e-6 and rel(x1, o.X.numpy()) <= 5e-6
    assert rel(v4, o.V.numpy()) <= 5e-6
    assert np.array_equal(v4, v1) and np.array_equal(x4, x1) and np.array_equal(xi4, xi1)
    sh, sw = (int(v) for v in rec._start_idx)
    outside = np.ones(xi4.shape[1:3], bool)
    outside[sh:sh + H, sw:sw + W] = False
    assert np.abs(xi4[0][outside]).max() > 0          # the dual is alive out there, not just zeros
    engine_opts(monkeypatch, xi_full=1)
    _, xif, xf, vf = run([4])
    assert rel(vf, v4) <= 2e-6 and np.abs(xif - xi4).max() <= 2e-5 * scale
    engine_opts(monkeypatch, xi_full=None, hv_full=None, k1_half=None)           # the default plan
    recd, xid, xd, vd = run([4])
    assert "row transforms skipped" in recd._handle.plan_info()
    assert rel(vd, v4) <= 2e-6 and rel(xd, x4) <= 2e-6 and np.abs(xid - xi4).max() <= 2e-5 * scale


@pytest.mark.parametrize("kind", ["half_rows_split_columns", "paired_rows_c4"])
def test_hv_rows_outside_the_sensor_window_are_skipped(backend, monkeypatch, kind):
    """Wide frames on compile-time plans with a column split: rows wholly outside the sensor window carry a = mu1 HV,
    whose row spectrum is mu1 Wp times the spectrum row the last inverse row pass read -- inside a call neither their
    forward nor their inverse H V row transform runs (AdmmScalars::skipa / skiphv); the last three iterations run
    complete.  Read-outs (V, HV, xi, X on the WHOLE padded frame) must match the float64 oracle after calls of every
    length around those boundaries, and continuations (reset=False) must too."""
    if kind == "paired_rows_c4":
        # C4's shape for ONE frame: 960-point paired rows (the rows of r_sp / V outside the window ride two per
        # transform: 135 rows above and below = 67 pairs + one single each), sequential 540-point middle rescaling SB
        H, W, C = 270, 480, 1
        engine_opts(monkeypatch, mid_seq=1)
        engine_opts(monkeypatch, prow_nt128=1)
        runs = ([2], [5], [4, 1, 5])
    else:
        H, W, C = 12, 1014, 1       # 24 x 2048 padded: half rows of 1024 points (compile-time plan), columns split
        engine_opts(monkeypatch, rows_half=1, tile_budget=256, jit_min_points=0)
        runs = ([2], [4], [5], [9], [6, 1, 5])
    rng = np.random.default_rng(11)
    psf = orc.synthetic_psf(1, H, W, C, seed=11)
    y = rng.random((H, W, C), dtype=np.float32)
    probe = lpa.ADMM(torch.from_numpy(psf), tau=2e-6, mu2=1e-4)
    info = probe._handle.plan_info()
    assert "H V row transforms skipped" in info, info

    def oracle(n):
        o = orc.ADMMOracle(psf, dtype=torch.float64, tau=2e-6, mu2=1e-4)
        o.set_data(y)
        o.reset()
        for _ in range(n):
            o.step()
        return o

    def engine(steps):
        rec = lpa.ADMM(torch.from_numpy(psf), tau=2e-6, mu2=1e-4)
        rec.set_data(torch.from_numpy(y))
        rec.apply(n_iter=0, disp_iter=None, plot=False)
        for n in steps:
            rec._iterate(n)
        return rec

    for steps in runs:
        rec, o = engine(steps), oracle(sum(steps))
        for attr, ref, tol in (("_image_est", o.V, 1e-5), ("_forward_out", o.HV, 1e-5), ("_X", o.X, 1e-5)):
            assert rel(np.asarray(getattr(rec, attr)), ref.numpy()) <= tol, (steps, attr)
        scale = float(np.abs(o.xi.numpy()).max())
        assert np.abs(np.asarray(rec._xi) - o.xi.numpy()).max() <= 5e-5 * scale, steps
    engine_opts(monkeypatch, hv_full=1)
    full = engine([6])
    engine_opts(monkeypatch, hv_full=None)
    assert rel(np.asarray(engine([6])._image_est), np.asarray(full._image_est)) <= 2e-6


def test_window_structure_with_a_per_iteration_schedule(backend, monkeypatch):
    """Unrolled ADMM changes mu1 from one iteration to the next: outside the sensor window a = mu1_k HV uses THIS
    iteration's step size and the stored xi = mu1_{k-1} (HV - HV_old) the previous one's.  The window-aware launch plan
    must agree with the plan that keeps xi and H V whole (options xi_full, hv_full), for a batch of two frames."""
    H, W, C, n_iter = 12, 1014, 1, 7
    engine_opts(monkeypatch, rows_half=1, tile_budget=256, jit_min_points=0)
    rng = np.random.default_rng(17)
    psf = torch.from_numpy(orc.synthetic_psf(1, H, W, C, seed=17))
    batch = torch.from_numpy(rng.random((2, 1, H, W, C), dtype=np.float32))
    sched = dict(mu1=1e-6 * (1 + 0.3 * np.arange(n_iter)), mu2=1e-4 * (1 + 0.1 * np.arange(n_iter)),
                 mu3=4e-5 * (1 + 0.2 * np.arange(n_iter)), tau=2e-6 * np.ones(n_iter))

    def run():
        net = lpa.UnrolledADMM(psf, n_iter=n_iter)
        net.set_parameters(**sched)
        return net.forward(batch), net._handle.plan_info()

    out, info = run()
    assert "H V row transforms skipped" in info, info
    engine_opts(monkeypatch, xi_full=1)
    engine_opts(monkeypatch, hv_full=1)
    ref, info_full = run()
    assert "xi inside the sensor window" not in info_full
    assert float(ref.abs().max()) > 0 and rel(out, ref) <= 2e-6


def test_c4_sequential_middle_on_one_frame(backend, monkeypatch):
    """C4's fused ADMM middle takes the two spectra one after the other through one tile of 8 image columns
    (k_cols_mid_admm_seq, 512 lanes); the engine selects it for large batches only, the option mid_seq=1 forces it onto one
    DiffuserCam-sized frame so that the CPU suite executes it -- with the work spectra in pair lines (the default) and in
    plain rows (spec_lay=0), and with the second tile's loads behind the first transform (mid_pre=0)."""
    psf = orc.synthetic_psf(1, 270, 480, 1, seed=1)
    engine_opts(monkeypatch, mid_seq=1)
    _admm_fista_vs_oracle(270, 480, 1, (540, 960), n_admm=2, n_fista=1)
    info = lpa.ADMM(torch.from_numpy(psf))._handle.plan_info()
    assert "one spectrum at a time, pair-line spectra" in info and "T = 8" in info, info
    for extra in ({"spec_lay": 0}, {"mid_pre": 0}):
        engine_opts(monkeypatch, mid_seq=1, **extra)
        _admm_fista_vs_oracle(270, 480, 1, (540, 960), n_admm=2, n_fista=0)
    engine_opts(monkeypatch, mid_seq=1, spec_lay=0)
    info = lpa.ADMM(torch.from_numpy(psf))._handle.plan_info()
    assert "one spectrum at a time]" in info, info


def test_c4_sequential_middle_frames_fastest_block_order(backend):
    """The sequential middle hands its workgroups out frames-fastest (all frames of a batch share H and |G|: one XCD's L2
    serves a column tile of them to the frames it owns).  A batch of 3 colour frames -- 3 frames x 3 PSF planes x 31
    column tiles, none of them a power of two -- must equal the single-frame runs of the same plan bit for bit."""
    rng = np.random.default_rng(31)
    psf = torch.from_numpy(orc.synthetic_psf(1, 270, 480, 3, seed=2))
    ys = torch.from_numpy(rng.random((3, 1, 270, 480, 3), dtype=np.float32))
    opts = {"mid_seq": 1, "prow_nt128": 1, "jit_min_points": 0}
    rec = lpa.ADMM(psf, engine_options=opts)
    rec.set_data(ys)
    assert "one spectrum at a time" in rec._handle.plan_info()
    got = rec.apply_batch(n_iter=2)
    single = lpa.ADMM(psf, engine_options=opts)
    for b in range(3):
        single.set_data(ys[b, 0])
        assert torch.equal(single.apply(n_iter=2, disp_iter=None), got[b]), b


def test_pair_line_spectra_odd_window_and_odd_height(backend):
    """Pair-line work spectra (lpc_args.h: spec_col -- rows (2p, 2p + 1) x 8 columns of a half spectrum share one
    128-byte line; paired rows + a single-pass middle of 8-column tiles): the window's row pairs are aligned to even rows,
    so a window that starts on an ODD row (270 x 480: sh = 135; 23 x 40: sh = 11) gets a first and a last pair with one
    row that is neither formed nor stored, and an odd padded height (45) a last pair of one row.  Long enough calls to run
    the steady state (a on the window's rows only, H V rows skipped outside it); against the float64 oracle, against the
    plain layout, and -- a batch -- against its single frames bit for bit.  Both middles: one spectrum at a time and side
    by side."""
    rng = np.random.default_rng(61)
    for (H, W, C, B), opts in (((23, 40, 1, 1), {"mid_seq": 1, "tile_budget": 720}), ((23, 40, 3, 2), {"mid_seq": 0, "tile_budget": 720}),
                               ((24, 40, 3, 2), {"mid_seq": 1, "tile_budget": 768}), ((270, 480, 1, 1), {})):
        psf = orc.synthetic_psf(1, H, W, C, seed=3)
        ys = rng.random((B, 1, H, W, C), dtype=np.float32)
        outs = {}
        for lay in (1, 0):
            rec = lpa.ADMM(torch.from_numpy(psf).to(backend.device), tau=2e-6, mu2=1e-4,
                           engine_options={"jit_min_points": 0, "spec_lay": lay, **opts})
            info = rec._handle.plan_info()
            assert ("pair-line spectra" in info) == bool(lay) and "row transforms skipped" in info, info
            rec.set_data(torch.from_numpy(ys).to(backend.device))
            outs[lay] = rec.apply_batch(n_iter=9)
            if lay and B > 1:
                for b in range(B):
                    rec.set_data(torch.from_numpy(ys[b, 0]).to(backend.device))
                    assert torch.equal(rec.apply(n_iter=9, disp_iter=None), outs[1][b]), (H, W, b)
        o = orc.ADMMOracle(psf, dtype=torch.float64, tau=2e-6, mu2=1e-4)
        o.set_data(ys[0, 0])
        assert rel(outs[1][0], o.apply(9)) <= 5e-6 and rel(outs[1], outs[0]) <= 2e-6, (H, W)


def test_xcd_runs_of_the_fused_forward_rows_change_nothing(backend, monkeypatch):
    """K1Rows::xcd_order: launches of more than 8192 row blocks hand the blocks of the fused forward rows out in runs of
    k1_group consecutive blocks per XCD (the stencil's neighbour rows then come from that XCD's L2), smaller ones an eighth
    of the launch per XCD -- permutations of the block order: every setting must give the launch order's result bit for
    bit.  16 gray frames of 270 x 480: 8640 row blocks by the host's count (6496 launched once the rows outside the sensor
    window are skipped: not a multiple of either run length, the tail keeps launch order)."""
    rng = np.random.default_rng(62)
    psf = torch.from_numpy(orc.synthetic_psf(1, 270, 480, 1, seed=2)).to(backend.device)
    ys = torch.from_numpy(rng.random((16, 1, 270, 480, 1), dtype=np.float32)).to(backend.device)
    outs = []
    for grp in (0, 16, 5):
        rec = lpa.ADMM(psf, tau=2e-6, mu2=1e-4, engine_options={"k1_group": grp})
        assert "three launches per iteration" in rec._handle.plan_info()
        rec.set_data(ys)
        outs.append(rec.apply_batch(n_iter=3))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_middle_tile_pairs_on_one_xcd(backend):
    """Option mid_swz: the side-by-side LDS middle hands its workgroups out so that the two 128-byte column tiles of a
    256-byte pair run on the same XCD (ColPass::swz) -- a permutation of the block order, so the result must be bit for
    bit the default order's.  61 column tiles x 2 planes: full groups of 16 and a tail that keeps the natural order."""
    rng = np.random.default_rng(41)
    psf = torch.from_numpy(orc.synthetic_psf(2, 270, 480, 1, seed=3))
    y = torch.from_numpy(rng.random((270, 480, 1), dtype=np.float32))
    outs = []
    for swz in (0, 1):
        rec = lpa.ADMM(psf, engine_options={"mid_swz": swz})
        assert "LDS middle [static" in rec._handle.plan_info()
        rec.set_data(y)
        outs.append(rec.apply(n_iter=2, disp_iter=None, plot=False))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("shape,opts", [((2, 96, 40, 1), {"tile_budget": 512, "col_t": 4, "split_n2": 12}),
                                        ((1, 270, 480, 1), {"mid_seq": 1}), ((2, 270, 480, 1), {})],
                         ids=["split_columns", "sequential_middle", "side_by_side_middle"])
def test_backward_grid_walks_change_nothing(backend, shape, opts):
    """Option rev_order: which ADMM kernels hand their workgroups out from the last block to the first (so that a kernel
    starts on what its predecessor wrote last, still in the memory-side cache).  A permutation of the block order of
    kernels whose blocks are independent: every setting must give the default's result bit for bit."""
    psf = torch.from_numpy(orc.synthetic_psf(*shape, seed=1))
    y = torch.from_numpy(np.random.default_rng(2).random((shape[1], shape[2], 1), dtype=np.float32))
    outs = []
    for ro in (0, 9, 15):
        rec = lpa.ADMM(psf, tau=2e-6, mu2=1e-4, engine_options={"rev_order": ro, "jit_min_points": 0, **opts})
        rec.set_data(y)
        outs.append(rec.apply(n_iter=3, disp_iter=None))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_c4_rows_on_128_threads(backend, monkeypatch):
    """960-point paired rows of a large batch run on 128 threads x 8 points (every lane owns one radix-8 butterfly of
    the fused first stage); the option prow_nt128 forces that shape onto one frame.  Same plan, same arithmetic: the result
    must be bitwise the one of the 256-thread kernels."""
    rng = np.random.default_rng(5)
    psf = torch.from_numpy(orc.synthetic_psf(1, 270, 480, 1, seed=1))
    y = torch.from_numpy(rng.random((270, 480, 1), dtype=np.float32))
    outs = []
    for nt128 in (0, 1):
        # (k1_rows=0: the same kernels on both shapes -- one quad per lane and row, the three-launch plan's condition,
        # holds on 256 lanes only)
        rec = lpa.ADMM(psf, engine_options={"prow_nt128": nt128, "k1_rows": 0})
        assert f"{128 if nt128 else 256} threads" in rec._handle.plan_info()
        rec.set_data(y)
        outs.append(rec.apply(n_iter=3, disp_iter=None, plot=False))
    assert torch.equal(outs[0], outs[1])
    engine_opts(monkeypatch, prow_nt128=1)
    _admm_fista_vs_oracle(270, 480, 1, (540, 960), n_admm=2, n_fista=1)


@pytest.mark.parametrize("shape,padded", [((3072, 20, 1), (6144, 40)), ((1080, 20, 1), (2160, 40)), ((760, 20, 1), (1536, 40))],
                         ids=["passA128", "passA90", "passA64"])
def test_pass_a_32_column_tiles(backend, monkeypatch, shape, padded):
    """Wide frames run pass A (compile-time plans) on 32-column tiles while the fused middle keeps 16; the option passa_t=32
    forces that split tiling onto frames only 21 spectrum columns wide (one partly filled pass-A tile, two middle
    tiles)."""
    engine_opts(monkeypatch, passa_t=32, jit_min_points=0)
    _admm_fista_vs_oracle(*shape, padded, n_admm=2, n_fista=2)


@pytest.mark.parametrize("kind,cls", [("fista", lpa.FISTA), ("nesterov", lpa.NesterovGradientDescent),
                                       ("vanilla", lpa.GradientDescent)])
def test_gd_update_with_fused_forward_rows(backend, monkeypatch, kind, cls):
    """Wide frames on compile-time plans: the update kernel also transforms the updated rows, so the next iteration
    skips its forward row pass (k_rinv_gd_update_fwd_half).  The cached row spectra must survive `reset=False`
    continuations and be dropped when something else overwrites the work spectrum (reconstruction_error) or the
    iterate (reset, warm start)."""
    H, W, C = 3, 4096, 1
    rng = np.random.default_rng(21)
    psf = orc.synthetic_psf(1, H, W, C, seed=6)
    y = rng.random((H, W, C), dtype=np.float32)
    rec = cls(torch.from_numpy(psf))
    rec.set_data(torch.from_numpy(y))
    o = orc.GDOracle(psf, kind=kind, dtype=torch.float64)
    o.set_data(y)
    rec.apply(n_iter=2, disp_iter=None)
    err = rec.reconstruction_error()                      # one convolution through the same work spectrum
    assert np.isfinite(float(err[0]))
    got = rec.apply(n_iter=3, disp_iter=None, reset=False)
    assert rel(got, o.apply(5)) <= 5e-6
    got2 = rec.apply(n_iter=4, disp_iter=None)            # reset: the cached spectra of the old iterate are dropped
    assert rel(got2, o.apply(4)) <= 5e-6
    engine_opts(monkeypatch, gd_no_fuse_fwd=1)
    plain = cls(torch.from_numpy(psf))
    plain.set_data(torch.from_numpy(y))
    assert rel(plain.apply(n_iter=4, disp_iter=None), got2) <= 1e-6


@pytest.mark.parametrize("seed", range(6))
def test_random_small_shapes_through_plan_modules(backend, monkeypatch, seed):
    """Random small frames with jit_min_points=0: every one gets a plan module compiled for it (g++ under the emulator,
    hipcc on the GPU) whatever its padded sizes factor into -- odd widths (paired rows), widths that are not a multiple
    of 4 (no X half), single-pass and forced four-step columns -- and ADMM / FISTA must match the float64 oracle."""
    engine_opts(monkeypatch, jit_min_points=0, **({"tile_budget": 512, "col_t": 4} if seed % 2 else {}))
    rng = np.random.default_rng(500 + seed)
    H, W, C = int(rng.integers(9, 70)), int(rng.integers(9, 90)), int(rng.choice([1, 3]))
    psf = orc.synthetic_psf(1, H, W, C, seed=seed)
    y = rng.random((H, W, C), dtype=np.float32)
    rec = lpa.ADMM(torch.from_numpy(psf), tau=2e-6, mu2=1e-4)
    info = rec._handle.plan_info()
    assert "plan module" in info, (H, W, C, info)
    rec.set_data(torch.from_numpy(y))
    o = orc.ADMMOracle(psf, dtype=torch.float64, tau=2e-6, mu2=1e-4)
    o.set_data(y)
    assert rel(rec.apply(n_iter=6, disp_iter=None), o.apply(6)) <= 5e-6, (H, W, C, info)
    f = lpa.FISTA(torch.from_numpy(psf))
    f.set_data(torch.from_numpy(y))
    of = orc.GDOracle(psf, kind="fista", dtype=torch.float64)
    of.set_data(y)
    assert rel(f.apply(n_iter=6, disp_iter=None), of.apply(6)) <= 5e-6, (H, W, C, f._handle.plan_info())


@pytest.mark.parametrize("shape", [(2, 4, 3), (3, 150, 1), (5, 70, 1), (130, 2, 1), (2, 2, 1)])
def test_tiny_frames_circular_neighbours(backend, shape):
    """The tiled image-domain kernel takes its circular TV neighbours without an integer division: -1 -> n - 1 and
    n -> 0 exactly, anything further out (the overhang of the last 4 x 256 tile) clamped to a safe address.  Frames of
    two to five rows, and a 300-column padded width that ends 44 columns into its second tile, with the TV term active,
    against the float64 oracle."""
    H, W, C = shape
    rng = np.random.default_rng(H * 1000 + W)
    psf = orc.synthetic_psf(1, H, W, C, seed=H + W)
    y = rng.random((H, W, C), dtype=np.float32)
    kw = dict(tau=5e-3, mu1=1e-2, mu2=1e-2, mu3=1e-2)
    rec = lpa.ADMM(torch.from_numpy(psf), **kw)
    rec.set_data(torch.from_numpy(y))
    o = orc.ADMMOracle(psf, dtype=torch.float64, **kw)
    o.set_data(y)
    want = np.asarray(o.apply(8))
    assert float(np.abs(want).max()) > 0
    assert rel(rec.apply(n_iter=8, disp_iter=None), want) <= 1e-5, rec._handle.plan_info()


@pytest.mark.parametrize("shape", [(24, 32, 3), (13, 40, 1), (5, 128, 3), (2, 36, 1), (33, 50, 1), (3, 640, 1), (2, 1014, 3)])
def test_tv_half_inside_forward_rows(backend, monkeypatch, shape):
    """Small frames run an ADMM iteration in three launches: the forward row blocks of r_sp form their two rows
    themselves (k_rfwd_arrays_x<.., K1>, k1_two_rows: the tiled kernel's TV / W statements with the stencil's circular
    neighbours read from global memory) and the tiled kernel is not launched (default wherever a paired row is one or two
    quads per lane -- the last two shapes: 1280 points on 192 lanes, 2048 on 256; option k1_rows=0: the tiled kernel).  Against the float64 oracle with the TV term active, across two calls
    (plain duals at the call boundary, half-applied ones inside), with the duals stored plain throughout (k1_half=0: the
    V_old path), and against the four-launch plan of the same engine; frames of 2 ... 33 rows, an odd number of padded
    rows included."""
    H, W, C = shape
    rng = np.random.default_rng(H * 100 + W)
    psf = orc.synthetic_psf(1, H, W, C, seed=H + 3 * W)
    y = rng.random((H, W, C), dtype=np.float32)
    kw = dict(tau=5e-3, mu1=1e-2, mu2=1e-2, mu3=1e-2)
    o = orc.ADMMOracle(psf, dtype=torch.float64, **kw)
    o.set_data(y)
    want5 = np.asarray(o.apply(5)).copy()
    want8 = np.asarray(o.apply(3, reset=False)).copy()
    assert float(np.abs(want8).max()) > 0
    outs = {}
    for tag, opts in (("rows", dict(k1_rows=1)), ("rows_plain_duals", dict(k1_rows=1, k1_half=0)), ("tiled", dict(k1_rows=0))):
        engine_opts(monkeypatch, jit_min_points=0, **opts)
        rec = lpa.ADMM(torch.from_numpy(psf), **kw)
        rec.set_data(torch.from_numpy(y))
        info = rec._handle.plan_info()
        assert ("three launches per iteration" in info) == (tag != "tiled"), info
        got5 = np.asarray(rec.apply(n_iter=5, disp_iter=None)).copy()
        got8 = np.asarray(rec.apply(n_iter=3, disp_iter=None, reset=False)).copy()
        assert rel(got5, want5) <= 1e-5 and rel(got8, want8) <= 1e-5, (tag, info)
        outs[tag] = got8
    assert rel(outs["rows"], outs["tiled"]) <= 2e-6


@pytest.mark.parametrize("name", ["admm_24x32x3_tv", "admm_24x32x3_init_bg", "admm_24x32x3_default"])
def test_tv_half_inside_forward_rows_golden(backend, monkeypatch, name):
    """... and the reference's own trajectories (golden vectors: TV term, initial estimate + background, defaults) through
    the three-launch plan."""
    engine_opts(monkeypatch, jit_min_points=0, k1_rows=1)
    test_admm_matches_reference_golden(backend, name)


def test_gram_as_row_and_column_terms(backend, monkeypatch):
    """The reference's finite-difference gram |PsiT Psi| (admm.py:385-397) is a row term plus a column term; the engine
    detects that at set-up and its fused middles read two vectors instead of the plane (option g_plane=1: the plane).
    Both forms against the float64 oracle, on a single-pass and on a split column plan; a caller's psi_gram that does not
    separate keeps the plane."""
    for opts, shape in (({}, (40, 56, 3)), ({"tile_budget": 512, "col_t": 4, "jit_min_points": 0}, (33, 50, 1))):
        H, W, C = shape
        rng = np.random.default_rng(H)
        psf = orc.synthetic_psf(1, H, W, C, seed=3)
        y = rng.random((H, W, C), dtype=np.float32)
        kw = dict(tau=2e-4, mu2=1e-3)
        o = orc.ADMMOracle(psf, dtype=torch.float64, **kw)
        o.set_data(y)
        want = np.asarray(o.apply(6))
        outs = {}
        for g_plane in (0, 1):
            rec = lpa.ADMM(torch.from_numpy(psf), engine_options={**opts, "g_plane": g_plane}, **kw)
            info = rec._handle.plan_info()
            assert ("gram as row + column terms" in info) == (g_plane == 0), info
            rec.set_data(torch.from_numpy(y))
            outs[g_plane] = rec.apply(n_iter=6, disp_iter=None)
            assert rel(outs[g_plane], want) <= 5e-6, info
        assert rel(outs[0], outs[1]) <= 5e-6

    def gram(shape):                        # a gram that is NOT separable: r * c term
        D, Hp, Wp, Cc = shape
        gsp = np.zeros(shape, dtype=np.float32)
        gsp[0, 0, 0] = 4.0
        gsp[0, 1 % Hp, 1 % Wp] = gsp[0, -1, -1] = -1.0
        gsp[0, 0, 1] = gsp[0, 0, -1] = -1.0
        return torch.fft.rfft2(torch.from_numpy(gsp), dim=(-3, -2))

    psf = orc.synthetic_psf(1, 24, 32, 1, seed=5)
    rec = lpa.ADMM(torch.from_numpy(psf), psi=lambda x: torch.stack([x, x], dim=-1), psi_adj=lambda u: u.sum(-1),
                   psi_gram=gram)
    assert "gram as row + column terms" not in rec._handle.plan_info()


@pytest.mark.parametrize("shape,algo,rad,extra", [
    ((1, 5, 512, 1), "fista", "8.8.8", {}),
    ((2, 4, 512, 3), "fista", "8.8.8", {"gd_rev": 7}),
    ((1, 5, 512, 3), "nesterov", "8.8.8", {}),
    ((1, 3, 512, 1), "gd", "8.8.8", {}),
    ((1, 3, 4092, 1), "fista", "16.16.16", {}),
    ((1, 3, 4092, 3), "nesterov", "8.8.8.8", {"row_rad": "8.8.8.8"}),
    ((1, 3, 4092, 1), "nesterov", "16.16.16", {}),
    ((1, 3, 4092, 1), "gd", "16.16.16", {}),
])
def test_gd_fused_rows_second_form(backend, monkeypatch, shape, algo, rad, extra):
    """option gd_v2 (default on): the gradient-descent family's two fused row kernels in their second form
    (lpc_gd_v2_kernels.h: M / R lanes per row, tangling + first inverse stage straight from global memory, the last inverse
    stage handing its samples to the first forward stage in registers, y / x / aux through range-checked buffer
    accesses, the tangling twiddles of a lane from ONE table entry times constants).  The iterates agree to round-off with
    the first form and with the float64 oracle; a frame whose window offset is odd keeps the first form.  gd.py:128-134,183-188,235-241."""
    D, H, W, C = shape
    rng = np.random.default_rng(W + C)
    psf = orc.synthetic_psf(D, H, W, C, seed=5)
    y = rng.random((H, W, C), dtype=np.float32)
    cls = {"fista": lpa.FISTA, "nesterov": lpa.NesterovGradientDescent, "gd": lpa.GradientDescent}[algo]
    outs = []
    for v2 in (0, 1):
        engine_opts(monkeypatch, gd_v2=v2, jit_min_points=0, **extra)
        rec = cls(torch.from_numpy(psf).to(backend.device))
        info = rec._handle.plan_info()
        assert "half-length %d [static %s" % (rec._padded_shape[2] // 2, rad) in info, info
        assert ("second form" in info) == bool(v2), info
        rec.set_data(torch.from_numpy(y).to(backend.device))
        a = rec.apply(n_iter=4, disp_iter=None).detach().cpu().numpy().copy()
        b = rec.apply(n_iter=3, disp_iter=None, reset=False).detach().cpu().numpy().copy()   # continuation: state intact
        outs.append((a, b))
    assert rel(outs[1][0], outs[0][0]) <= 2e-6 and rel(outs[1][1], outs[0][1]) <= 2e-6
    o = orc.GDOracle(psf, kind={"gd": "vanilla"}.get(algo, algo), dtype=torch.float64)
    o.set_data(y)
    assert rel(outs[1][1], o.apply(7)) <= 5e-6
    # odd window offset: 8-byte accesses to y / x are not aligned -> first form
    engine_opts(monkeypatch, jit_min_points=0)
    rec = lpa.FISTA(torch.from_numpy(orc.synthetic_psf(1, 3, 510, 1, seed=1)).to(backend.device))
    assert "second form" not in rec._handle.plan_info()
