"""
Reverse mode of unrolled FISTA (lpc_fista_record / lpc_fista_backward) over shapes, launch plans and options, with the
projection's masks ACTIVE, against torch.autograd over the restated formula (tests/unrolled_restated.py), through the
public API, on the SIMT emulator ('emu') and on the MI355X ('hip', -m gpu).

tests/test_unrolled_grad.py compares with the reference's own gradients, but its fixtures (non-negative PSF, measurement in
[0, 1)) clamp under 1 % of the elements in every projection: a reverse sweep that took the mask from the wrong tape slot
would pass there.  Here the measurement is signed (``rng.random - 0.5``, otherwise gen_unrolled_grad.py's recipe), and
for every case the float64 restatement asserts (``conditions``) that
  * no argument of any projection (z_0 .. z_{n-1}, y_n) has an element on the kink, 0 < |z| < 1e-5 max|z| (the generator's
    own rule: there float32 and float64 may legitimately take different branches), and
  * every projection clamps between 20 % and 80 % of its elements.
The seeds in the table below were chosen on the CPU so that both hold.  One exception, by construction: with steps of
0.01 x the default (variant ``small_steps``) the iterates stay within about 1 % of the positive default start, so no
projection clamps anything whatever the seed.  That variant is there for the float32 digits of y_i - xk_i = a_i gr_i on
the OPEN mask; it asserts the kink condition only.

Reference: ``restated()`` in float64; it is pinned to the reference's fixtures first (test_restatement_is_pinned).
Bounds (the rule of tests/test_unrolled_grad.py; max-norm over whole arrays, relative to the max of the float64 array):
  float32 engine:  rel(q, restated64) <= 4 * max(rel(restated32, restated64), 2e-6) for out, g_alpha, g_tk, g_data, g_init
                   -- the yardstick is the float32 restatement of the same case, computed here, never the engine;
  float64 engine:  <= 100 * F64_TOL = 1e-9; g_tk <= 5e-7 (``_tk_p`` and its gradient are kept in float32).
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from unrolled_restated import F64_TOL, KINK, PLANS, default_steps, rel, restated

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["unrolled_fista_grad_24x32x3_b3", "unrolled_fista_grad_19x27x1_b2", "unrolled_fista_grad_20x28_gray_rgb"]
SPLIT = {"tile_budget": 512, "col_t": 4}

# name: (H, W, C, B, n), padded (Hp, Wp), seed, and why it is there
CASES = {
    # smallest legal frame (a 4-point half transform in a 64-lane group); n = 1: gb_first and tail in one iteration; B = 1
    "4x4": dict(shape=(4, 4, 1, 1, 1), padded=(8, 8), seed=2000),
    # `pair` of k_gd_bwd_half false through odd hw alone (sw 14, hw 27); odd H: the last row pair has one row; Wp % 4 != 0
    "11x26": dict(shape=(11, 26, 1, 2, 3), padded=(24, 54), seed=2000),
    # `pair` false through odd sw alone (sw 15, hw 30); C = 3
    "12x30": dict(shape=(12, 30, 3, 2, 4), padded=(24, 60), seed=2000),
    # odd W, Wp % 4 != 0; B = 1 with C = 3
    "10x25": dict(shape=(10, 25, 3, 1, 3), padded=(20, 50), seed=2000),
    # Wp = 128 = 8.8.2: the paired reverse rows on a plan with a trailing radix-2 stage; n = 2
    "6x64": dict(shape=(6, 64, 1, 2, 2), padded=(12, 128), seed=2000),
    # split columns (Hp = 96 = 4 x 24 / 8 x 12) under the reverse sweep: the register middle and the LDS middle
    "48x20_reg": dict(shape=(48, 20, 1, 2, 3), padded=(96, 40), seed=2000, opts={**SPLIT, "split_n2": 24},
                      info="columns: 4 x 24 split"),
    "48x20_lds": dict(shape=(48, 20, 1, 2, 3), padded=(96, 40), seed=2000, opts={**SPLIT, "split_n2": 12},
                      info="columns: 8 x 12 split"),
    # a one-channel measurement against an RGB PSF: the channel-summing branch of k_gd_bwd_gdata, with active masks
    "12x30_gray": dict(shape=(12, 30, 3, 2, 3), padded=(24, 60), seed=2001, data_channels=1),
}
ROW_CASES = ["4x4", "11x26", "12x30", "10x25", "6x64"]
MODULE_CASES = ["11x26", "12x30", "6x64"]        # a plan module is compiled per shape (seconds each)
OTHER_CASES = ["48x20_reg", "48x20_lds", "12x30_gray"]
VARIANT_CASES = ["11x26", "12x30"]
# (a) negative parameters, (b) alpha x 0.01, (c) no data gradient, (d) learn_tk=False, (e) a learnt initial estimate;
# (c) and (d) run the inputs of the plain case
VARIANTS = ["signs", "small_steps", "no_data_grad", "no_tk_grad", "init"]


def conditions(args, tag, active=True):
    """the two input conditions on the float64 arguments of the projection; returns the clamped fractions"""
    fracs = []
    for i, z in enumerate(args):
        a = z.abs()
        kinks = int(((a > 0) & (a < KINK * float(a.max()))).sum())
        assert kinks == 0, f"{tag}: {kinks} element(s) on the kink of projection {i}: pick another seed"
        fracs.append(float((z <= 0).double().mean()))
        assert not active or 0.2 <= fracs[-1] <= 0.8, f"{tag}: projection {i} clamps {100 * fracs[-1]:.1f} % of its elements"
    return fracs


@functools.lru_cache(maxsize=None)
def inputs(name, variant="plain"):
    """inputs of a case (gen_unrolled_grad.py's recipe with a signed measurement) and the float64 / float32 restatement's
    output and gradients of (out * w).sum(); computed once per (case, variant), never written to"""
    case = CASES[name]
    H, W, C, B, n = case["shape"]
    seed = case["seed"]      # (the variants hold the conditions at their case's seed)
    rng = np.random.default_rng(seed)
    psf = rng.random((1, H, W, C)).astype(np.float32) ** 6
    psf /= np.linalg.norm(psf.ravel())
    data = (rng.random((B, 1, H, W, case.get("data_channels", C))) - 0.5).astype(np.float32)
    w = rng.standard_normal((B, 1, H, W, C)).astype(np.float32)
    rng = np.random.default_rng(seed + 50)
    alpha0, tk0 = default_steps(torch.from_numpy(psf), n)
    factor = 0.01 if variant == "small_steps" else 1.0
    alpha = (alpha0 * (0.6 + 0.4 * rng.random((n, C))) * factor).astype(np.float32)
    tk = (tk0 * (1 + 0.2 * rng.random(n + 1))).astype(np.float32)
    flipped = []
    if variant == "signs":      # |.| is taken inside: the iteration is the plain one, the gradients change sign
        flipped = [("g_alpha", (0, 0)), ("g_alpha", (1, C - 1)), ("g_tk", (n,))]
        alpha[0, 0], alpha[1, C - 1], tk[n] = -alpha[0, 0], -alpha[1, C - 1], -tk[n]
    init = None
    if variant == "init":
        init = np.random.default_rng(seed + 100).random((1,) + psf.shape, dtype=np.float32) * np.float32(0.1)
    inp = SimpleNamespace(name=name, variant=variant, n=n, psf=psf, data=data, w=w, alpha=alpha, tk=tk, init=init,
                          flipped=flipped, ref={})
    for tdt in (torch.float64, torch.float32):
        ap = torch.from_numpy(alpha).to(tdt).requires_grad_()
        tp = torch.from_numpy(tk).requires_grad_()
        d = torch.from_numpy(data).to(tdt).requires_grad_()
        ini = None if init is None else torch.from_numpy(init).to(tdt).requires_grad_()
        out, args = restated(torch.from_numpy(psf), d, ap, tp, n, init=ini, dtype=tdt)
        (out * torch.from_numpy(w).to(tdt)).sum().backward()
        r = {"out": out.detach().numpy(), "g_alpha": ap.grad.numpy(), "g_tk": tp.grad.numpy(), "g_data": d.grad.numpy()}
        if ini is not None:
            r["g_init"] = ini.grad.numpy()
        inp.ref[tdt] = r
        if tdt == torch.float64:
            inp.clamped = conditions(args, f"{name} {variant} seed {seed}", active=variant != "small_steps")
    for k, idx in flipped:      # a gradient of the wrong sign must be visible in the max-norm
        g = inp.ref[torch.float64][k]
        assert abs(g[idx]) >= 1e-3 * np.abs(g).max(), (name, k, idx, g)
    return inp


def engine_run(inp, dtype, backend, data_grad=True, learn_tk=True):
    tdt = torch.float64 if dtype == "float64" else torch.float32
    dev = backend.device
    est = None if inp.init is None else torch.from_numpy(inp.init).to(device=dev, dtype=tdt).requires_grad_()
    rec = lpa.UnrolledFISTA(torch.from_numpy(inp.psf).to(dev), n_iter=inp.n, dtype=dtype, learn_tk=learn_tk,
                            initial_est=est)
    rec.set_parameters(alpha=inp.alpha, tk=inp.tk)
    batch = torch.from_numpy(inp.data).to(device=dev, dtype=tdt).requires_grad_(data_grad)
    out = rec(batch)
    (out * torch.from_numpy(inp.w).to(device=dev, dtype=tdt)).sum().backward()
    got = {"out": out, "g_alpha": rec._alpha_p.grad, "g_tk": rec._tk_p.grad, "g_data": batch.grad}
    if est is not None:
        got["g_init"] = est.grad
    return rec, got


def check_parity(monkeypatch, inp, dtype, backend, tag, opts, absent=()):
    """one forward and one backward on the engine under the launch-plan options ``opts``; every quantity but those in
    ``absent`` (which must come back as None) against the float64 restatement"""
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **CASES[inp.name].get("opts", {}), **opts})
    rec, got = engine_run(inp, dtype, backend, data_grad="g_data" not in absent, learn_tk="g_tk" not in absent)
    assert tuple(rec._padded_shape[1:3]) == CASES[inp.name]["padded"], rec._padded_shape
    ref64, ref32 = inp.ref[torch.float64], inp.ref[torch.float32]
    bad = []
    for k, want in ref64.items():
        if k in absent:
            assert got[k] is None, k
            continue
        assert got[k] is not None and tuple(got[k].shape) == want.shape, (k, got[k])
        r = rel(got[k], want)
        if dtype == "float64":
            bound = 5e-7 if k == "g_tk" else 100 * F64_TOL
        else:
            bound = 4 * max(rel(ref32[k], want), 2e-6)
        print(f"{tag} {dtype} {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))
    assert not bad, bad
    for k, idx in inp.flipped:       # abs': the gradient of a negated parameter has the sign the restatement gives it
        assert float(got[k][idx]) * float(ref64[k][idx]) > 0, (k, idx, float(got[k][idx]), float(ref64[k][idx]))
    return rec


# ------------------------------------------------------------------------------------------------- CPU only --
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_is_pinned(name):
    """the float64 restatement against the reference's own float64 output and gradients, on every fixture of
    test_unrolled_grad.py (the gray-measurement / RGB-PSF broadcast included)"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    ap, tp = torch.from_numpy(g["alpha"]).double().requires_grad_(), torch.from_numpy(g["tk"]).requires_grad_()
    data = torch.from_numpy(g["data"]).double().requires_grad_()
    out, args = restated(torch.from_numpy(g["psf"]), data, ap, tp, int(g["n_iter"]))
    assert len(args) == int(g["n_iter"]) + 1 and not any(z.requires_grad for z in args)
    (out * torch.from_numpy(g["w"]).double()).sum().backward()
    bad = []
    for k, v in (("out", out), ("g_alpha", ap.grad), ("g_tk", tp.grad), ("g_data", data.grad)):
        r, bound = rel(v, g[k + "64"]), 5e-7 if k == "g_tk" else 100 * F64_TOL
        print(f"{name} restated float64 {k}: rel {r:.3e} (bound {bound:.1e})")
        if not (r <= bound and tuple(v.shape) == g[k + "64"].shape):
            bad.append((k, r, bound))
    assert not bad, bad
    # what the fixtures leave open: their projections clamp almost nothing
    assert max(float((z <= 0).double().mean()) for z in args) < 0.01


def test_inputs_meet_their_conditions():
    """every case and variant: kink-free, and 20 % to 80 % clamped in every projection (asserted in ``inputs``; the
    small steps clamp nothing, see the module docstring)"""
    for name in CASES:
        for variant in ["plain"] + (["signs", "small_steps", "init"] if name in VARIANT_CASES else []):
            inp = inputs(name, variant)
            print(f"{name} {variant}: clamped per projection", " ".join(f"{100 * f:.0f}%" for f in inp.clamped),
                  "| float32 restatement:", " ".join(f"{k} {rel(inp.ref[torch.float32][k], v):.1e}"
                                                     for k, v in inp.ref[torch.float64].items()))
            assert len(inp.clamped) == inp.n + 1


# ----------------------------------------------------------------------------------------- emulator and card --
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name,plan", [(c, p) for c in ROW_CASES for p in sorted(PLANS)
                                       if p != "module" or c in MODULE_CASES])
def test_sweep_every_row_form(backend, monkeypatch, name, plan, dtype):
    opts, marker = PLANS[plan]
    rec = check_parity(monkeypatch, inputs(name), dtype, backend, f"{name} {plan}", opts)
    assert marker in rec._handle.plan_info(), rec._handle.plan_info()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("plan", ["default", "rows_half", "rows_paired"])
@pytest.mark.parametrize("name", OTHER_CASES)
def test_sweep_split_columns_and_gray_measurement(backend, monkeypatch, name, plan, dtype):
    opts, marker = PLANS[plan] if plan != "default" else ({}, "reverse rows: ")
    rec = check_parity(monkeypatch, inputs(name), dtype, backend, f"{name} {plan}", opts)
    info = rec._handle.plan_info()
    assert marker in info and CASES[name].get("info", "columns: single pass") in info, info


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("plan", ["rows_half", "rows_paired"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_sweep_variants(backend, monkeypatch, name, variant, plan, dtype):
    opts, marker = PLANS[plan]
    absent = {"no_data_grad": ("g_data",), "no_tk_grad": ("g_tk",)}.get(variant, ())
    inp = inputs(name, "plain" if absent else variant)
    rec = check_parity(monkeypatch, inp, dtype, backend, f"{name} {variant} {plan}", opts, absent=absent)
    assert marker in rec._handle.plan_info(), rec._handle.plan_info()
    if variant == "no_tk_grad":
        assert not isinstance(rec._tk_p, torch.nn.Parameter) and [tuple(p.shape) for p in rec.parameters()] == \
            [tuple(inp.alpha.shape)]
