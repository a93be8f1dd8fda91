"""
A PSF swap on a solver that already ran (``_set_psf(p2)``, ``forward(batch, psfs=p2)``), over the launch plans that keep
something derived from the PSF -- the spectrum, its pair-line copy, the split middles, the sequential middle's precombined
tables, the step alpha, the default start value -- on the SIMT emulator ('emu') and on the MI355X ('hip', -m gpu).

1. Swap equals a fresh solver.  ADMM, UnrolledADMM (with a schedule), FISTA, NesterovGradientDescent and UnrolledFISTA with
   an explicit ``initial_est``: built from p1 and run, swapped to p2 and run again = a solver built from p2, bit for bit,
   and more than 1e-2 from the p1 result.  The GD family follows the new PSF with its step too (gd.py:94-112).
2. The default start value of UnrolledFISTA.  The reference computes ``_image_init`` once, in the constructor, from the
   constructor's PSF (unrolled_fista.py:55-59); ``reset()`` reuses it (:91-96), ``forward(batch, psfs=...)`` rebuilds the
   convolver only (trainable_recon.py:346-350) and ``_set_psf`` changes PSF and convolver and calls that ``reset()``
   (recon.py:448-470).  So after a swap the iteration still starts from (max p1 + min p1) / 2, a constant with no gradient
   into the PSF.  Three forwards p1, p2, p1 on one solver, both ways in, against ``restated(p, init=default_init(p1))``:
   out, g_psf, g_data, g_alpha, g_tk under the bounds of tests/test_unrolled_psf_grad.py.  Inputs: sweep case "12x30";
   p2 = rng(P2_SEED).random ** 6, normalised, x P2_SCALE, chosen on the CPU so that the swapped run too is kink-free with every
   projection 20 - 80 % clamped (``conditions`` of tests/test_unrolled_grad_sweep.py, asserted in ``swap_refs``).
3. The same against the reference itself: tests/golden/unrolled_fista_psf_swap_12x30x3_b2.npz (gen_unrolled_psf_grad.py:
   the reference's UnrolledFISTA constructed from p1, ``forward(batch, psfs=p2)`` with p2 a leaf).
"""
import functools
import os

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from oracle import lensless_oracle as orc
from test_unrolled_admm_sweep import BASE, CASES as ADMM_CASES, N_ITER, markers, schedule
from test_unrolled_grad_sweep import conditions, inputs as fista_inputs
from test_unrolled_psf_grad import ROW_PLANS, bound_of, default_init
from unrolled_restated import F64_TOL, PLANS, default_steps, rel, restated

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SWAP_FIXTURE = "unrolled_fista_psf_swap_12x30x3_b2"
P2_SEED, P2_SCALE = 99, 0.7

ADMM_SWAP_CASES = ["rt", "mod", "split_reg", "split_mod", "seq_odd", "seq_even", "pair", "gterms"]
# the gradient-descent family: name -> (H, W, C, B), options, marker
GD_CASES = {
    "rt": dict(shape=(24, 32, 3, 2), opts={}, info="run-time plans"),
    "rows_half": dict(shape=(24, 32, 3, 2), opts={"jit_min_points": 0, "rows_half": 1}, info="half-length 32"),
    "split_mod": dict(shape=(48, 20, 1, 2), opts={"tile_budget": 512, "col_t": 4, "split_n2": 12, "jit_min_points": 0},
                      info="pass A [static"),
    "module": dict(shape=(12, 30, 3, 2), opts=PLANS["module"][0], info=PLANS["module"][1]),     # UnrolledFISTA only
}
GD_ITERS = 4


def two_psfs(H, W, C, seed):
    """two PSFs of one shape with different content and a different max + min"""
    p1, p2 = orc.synthetic_psf(1, H, W, C, seed), orc.synthetic_psf(1, H, W, C, seed + 1000) * np.float32(0.7)
    s1, s2 = float(p1.max() + p1.min()), float(p2.max() + p2.min())
    assert abs(s1 - s2) > 0.1 * max(s1, s2) and rel(p2, p1) > 0.5
    return p1, p2


def on(backend, a, tdt=torch.float32):
    return torch.from_numpy(a).to(device=backend.device, dtype=tdt)


def check_swap(tag, first, swapped, fresh):
    moved = rel(first, fresh)
    print(f"{tag}: p1 result against the p2 result: {moved:.3e}; swapped against fresh: {rel(swapped, fresh):.3e}")
    assert float(fresh.abs().max()) > 0 and moved > 1e-2, moved
    assert torch.equal(swapped, fresh), rel(swapped, fresh)


# ------------------------------------------------------------------- 1. swap equals a fresh solver --
@pytest.mark.parametrize("name", ADMM_SWAP_CASES)
@pytest.mark.parametrize("cls", ["ADMM", "UnrolledADMM"])
def test_admm_swap_equals_a_fresh_solver(backend, monkeypatch, cls, name):
    case = ADMM_CASES[name]
    H, W, C, B = case["shape"]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **case["opts"]})
    p1, p2 = (on(backend, p) for p in two_psfs(H, W, C, case["seed"]))
    data = on(backend, np.random.default_rng(case["seed"]).random((B, 1, H, W, C), dtype=np.float32))

    def build(p):
        if cls == "ADMM":
            rec = lpa.ADMM(p, n_iter=GD_ITERS, **BASE)
            rec.set_data(data)
        else:
            rec = lpa.UnrolledADMM(p, n_iter=N_ITER, **BASE)
            rec.set_parameters(**schedule())
        return rec

    def run(rec, swap_to=None):
        if cls == "ADMM":
            if swap_to is not None:
                rec._set_psf(swap_to)
            out = rec.apply_batch()
        else:
            out = rec.forward(data, psfs=swap_to)
        info = rec._handle.plan_info()
        for marker in markers(name, "float32"):
            assert marker in info, (marker, info)
        return out.clone()

    rec = build(p1)
    first = run(rec)
    swapped = run(rec, swap_to=p2)
    check_swap(f"{cls} {name}", first, swapped, run(build(p2)))


@pytest.mark.parametrize("name,cls", [(n, c) for c in ("FISTA", "NesterovGradientDescent", "UnrolledFISTA")
                                      for n in GD_CASES if n != "module" or c == "UnrolledFISTA"])
def test_gd_family_swap_equals_a_fresh_solver(backend, monkeypatch, name, cls):
    case = GD_CASES[name]
    H, W, C, B = case["shape"]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **case["opts"]})
    p1n, p2n = two_psfs(H, W, C, 40)
    p1, p2 = on(backend, p1n), on(backend, p2n)
    rng = np.random.default_rng(41)
    data = on(backend, rng.random((B, 1, H, W, C), dtype=np.float32))
    est = on(backend, rng.random((1, 1, H, W, C), dtype=np.float32) * np.float32(0.05))
    alpha, tk = default_steps(torch.from_numpy(p1n), GD_ITERS)        # one schedule for both PSFs: the smaller steps
    alpha = np.minimum(alpha, default_steps(torch.from_numpy(p2n), GD_ITERS)[0])

    def build(p):
        if cls == "UnrolledFISTA":
            rec = lpa.UnrolledFISTA(p, n_iter=GD_ITERS, initial_est=est)
            rec.set_parameters(alpha=alpha * 0.8, tk=tk * 1.1)
        else:
            rec = getattr(lpa, cls)(p, n_iter=GD_ITERS)
            rec.set_data(data)
        return rec

    def run(rec, swap_to=None):
        with torch.no_grad():
            if cls == "UnrolledFISTA":
                out = rec(data, psfs=swap_to)
            else:
                if swap_to is not None:
                    rec._set_psf(swap_to)
                out = rec.apply_batch()
        assert case["info"] in rec._handle.plan_info(), rec._handle.plan_info()
        return out.clone()

    rec = build(p1)
    first, alpha1 = run(rec), rec._alpha.clone()
    swapped = run(rec, swap_to=p2)
    fresh = build(p2)
    check_swap(f"{cls} {name}", first, swapped, run(fresh))
    assert float(alpha1.min()) > 0 and rel(alpha1, fresh._alpha) > 1e-2 and torch.equal(rec._alpha, fresh._alpha)      # gd.py:107-112


# ------------------------------------------- 2. the default start value of UnrolledFISTA after a swap --
def second_psf(shape):
    p2 = np.random.default_rng(P2_SEED).random(shape).astype(np.float32) ** 6
    p2 /= np.linalg.norm(p2.ravel())
    return p2 * np.float32(P2_SCALE)


def restated_run(p, p1, data, w, alpha, tk, n, tdt):
    """the restatement in ``tdt`` with the PSF ``p`` a leaf and the CONSTRUCTOR's start value, default_init(p1): out, the
    gradients of (out * w).sum(), and the arguments of every projection"""
    leaf = torch.from_numpy(p).to(tdt).requires_grad_()
    ap, tp = torch.from_numpy(alpha).to(tdt).requires_grad_(), torch.from_numpy(tk).requires_grad_()
    d = torch.from_numpy(data).to(tdt).requires_grad_()
    out, args = restated(leaf, d, ap, tp, n, init=default_init(torch.from_numpy(p1).to(tdt)), dtype=tdt)
    (out * torch.from_numpy(w).to(tdt)).sum().backward()
    return {"out": out.detach().numpy(), "g_psf": leaf.grad.numpy(), "g_data": d.grad.numpy(), "g_alpha": ap.grad.numpy(),
            "g_tk": tp.grad.numpy()}, args


@functools.lru_cache(maxsize=None)
def swap_refs():
    """sweep case "12x30" with a second PSF: the float64 / float32 restatement of the forwards with p1 and with p2, both
    started at default_init(p1); computed once, never written to"""
    inp = fista_inputs("12x30")
    p1, p2 = inp.psf, second_psf(inp.psf.shape)
    s1, s2 = float(p1.max() + p1.min()), float(p2.max() + p2.min())
    assert abs(s1 - s2) > 0.1 * max(s1, s2), (s1, s2)
    refs = {}
    for tag, p in (("p1", p1), ("p2", p2)):
        for tdt in (torch.float64, torch.float32):
            refs[tag, tdt], args = restated_run(p, p1, inp.data, inp.w, inp.alpha, inp.tk, inp.n, tdt)
            if tdt == torch.float64:
                refs[tag, "clamped"] = conditions(args, f"12x30 with {tag}, start value of p1")
    return inp, p1, p2, refs


def test_swap_inputs_meet_their_conditions():
    """kink-free and 20 - 80 % clamped with either PSF (asserted in ``swap_refs``); and the start value matters: the
    restatement started from the NEW PSF's default is far outside every bound"""
    inp, p1, p2, refs = swap_refs()
    for tag in ("p1", "p2"):
        print(f"{tag}: clamped per projection", " ".join(f"{100 * f:.0f}%" for f in refs[tag, "clamped"]))
    wrong, _ = restated_run(p2, p2, inp.data, inp.w, inp.alpha, inp.tk, inp.n, torch.float64)
    for k in ("out", "g_psf"):
        moved, bound = rel(wrong[k], refs["p2", torch.float64][k]), bound_of("float32", refs["p2", torch.float32][k],
                                                                              refs["p2", torch.float64][k], k)
        print(f"start value of p2 instead of p1: {k} moves by {moved:.3e} (float32 bound {bound:.1e})")
        assert moved >= 100 * bound, (k, moved, bound)


@pytest.mark.parametrize("how", ["forward", "set_psf"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("plan", ROW_PLANS + ["module"])
def test_default_start_value_survives_a_swap(backend, monkeypatch, plan, dtype, how):
    opts, marker = PLANS[plan]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **opts})
    inp, p1, p2, refs = swap_refs()
    tdt = torch.float64 if dtype == "float64" else torch.float32
    rec = lpa.UnrolledFISTA(on(backend, p1), n_iter=inp.n, dtype=dtype)
    rec.set_parameters(alpha=inp.alpha, tk=inp.tk)
    w = on(backend, inp.w, tdt)
    bad = []
    for step, tag in enumerate(("p1", "p2", "p1")):
        p = on(backend, p1 if tag == "p1" else p2, tdt).requires_grad_()
        batch = on(backend, inp.data, tdt).requires_grad_()
        rec.zero_grad()
        if how == "forward":
            out = rec(batch, psfs=p)
        else:
            rec._set_psf(p)
            out = rec(batch)
        (out * w).sum().backward()
        assert marker in rec._handle.plan_info(), rec._handle.plan_info()
        got = {"out": out, "g_psf": p.grad, "g_data": batch.grad, "g_alpha": rec._alpha_p.grad, "g_tk": rec._tk_p.grad}
        for k, want in refs[tag, torch.float64].items():
            assert got[k] is not None and tuple(got[k].shape) == want.shape, (k, got[k])
            r, bound = rel(got[k], want), bound_of(dtype, refs[tag, torch.float32][k], want, k)
            print(f"forward {step} ({tag}) {plan} {dtype} {how} {k}: rel {r:.3e} (bound {bound:.1e})")
            if not r <= bound:
                bad.append((step, tag, k, r, bound))
    assert not bad, bad


def test_start_value_survives_a_new_batch_size_and_costs_no_memory(backend):
    """a swap leaves lpc_workspace_bytes where it was (the start value is no initial estimate: nothing is allocated for it),
    and the handle a new batch size creates -- which gets the CURRENT PSF, p2 -- still starts from the constructor's value"""
    inp, p1, p2, refs = swap_refs()
    rec = lpa.UnrolledFISTA(on(backend, p1), n_iter=inp.n, dtype="float64")
    rec.set_parameters(alpha=inp.alpha, tk=inp.tk)
    data = on(backend, inp.data, torch.float64)
    with torch.no_grad():
        rec(data)
        base = rec._handle.workspace_bytes()
        out2 = rec(data, psfs=on(backend, p2, torch.float64))
        assert rec._handle.workspace_bytes() == base
        first = rec._handle
        out1 = rec(data[:1])                              # a new handle, set up with p2
        assert rec._handle is not first and rec._handle_batch == 1
    want = refs["p2", torch.float64]["out"]
    for tag, got, ref in (("batch of 2", out2, want), ("batch of 1", out1, want[:1])):
        r = rel(got, ref)
        print(f"p2 after p1, {tag}: rel {r:.3e} (bound {100 * F64_TOL:.1e})")
        assert r <= 100 * F64_TOL, (tag, r)


# ------------------------------------------------------------------- 3. pinned to the reference itself --
def test_restatement_with_the_constructors_start_value_is_pinned():
    """the restatement with the PSF p2 a leaf and ``init=default_init(p1)`` against the reference's UnrolledFISTA built from
    p1 and called with ``psfs=p2``: float64 to 100 * F64_TOL, float32 as far as the reference's own float32 run allows"""
    g = np.load(os.path.join(GOLDEN, SWAP_FIXTURE + ".npz"))
    n = int(g["n_iter"])
    assert g["psf"].shape == g["p2"].shape == (1, 12, 30, 3) and g["data"].shape == (2, 1, 12, 30, 3) and n == 4
    s1, s2 = float(g["psf"].max() + g["psf"].min()), float(g["p2"].max() + g["p2"].min())
    assert abs(s1 - s2) > 0.1 * max(s1, s2) and g["clamped"].shape == (n + 1,)
    assert 0.2 <= float(g["clamped"].min()) and float(g["clamped"].max()) <= 0.8
    for tdt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        got, _ = restated_run(g["p2"], g["psf"], g["data"], g["w"], g["alpha"], g["tk"], n, tdt)
        for k in ("out", "g_psf"):
            r = rel(got[k], g[k + "64"])
            bound = 100 * F64_TOL if tag == "64" else bound_of("float32", g[k + "32"], g[k + "64"])
            print(f"restated float{tag} {k}: rel {r:.3e} (bound {bound:.1e})")
            assert got[k].shape == g[k + "64"].shape and r <= bound, (k, r, bound)
    wrong, _ = restated_run(g["p2"], g["p2"], g["data"], g["w"], g["alpha"], g["tk"], n, torch.float64)
    assert rel(wrong["out"], g["out64"]) > 1e-3          # the fixture tells the two start values apart


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("plan", ROW_PLANS)
def test_swap_against_the_reference(backend, monkeypatch, plan, dtype):
    """the engine, built from p1 and called with ``psfs=p2``, against the reference's own output and ``psfs`` gradient"""
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **PLANS[plan][0]})
    g = np.load(os.path.join(GOLDEN, SWAP_FIXTURE + ".npz"))
    tdt = torch.float64 if dtype == "float64" else torch.float32
    rec = lpa.UnrolledFISTA(on(backend, g["psf"]), n_iter=int(g["n_iter"]), dtype=dtype)
    rec.set_parameters(alpha=g["alpha"], tk=g["tk"])
    p = on(backend, g["p2"], tdt).requires_grad_()
    out = rec(on(backend, g["data"], tdt), psfs=p)
    (out * on(backend, g["w"], tdt)).sum().backward()
    assert PLANS[plan][1] in rec._handle.plan_info()
    bad = []
    for k, v in (("out", out), ("g_psf", p.grad)):
        assert v is not None, k
        r, bound = rel(v, g[k + "64"]), bound_of(dtype, g[k + "32"], g[k + "64"])
        print(f"swap fixture {plan} {dtype} {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))
    assert not bad, bad
