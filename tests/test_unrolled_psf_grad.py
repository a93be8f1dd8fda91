"""
Gradient of unrolled FISTA with respect to the PSF (lpc_fista_backward_psf; ``UnrolledFISTA.forward(batch, psfs=p)`` and
``_set_psf(p)`` with ``p.requires_grad``), through the public API, on the SIMT emulator ('emu') and on the MI355X ('hip',
-m gpu).

Inputs: the cases of tests/test_unrolled_grad_sweep.py (signed measurement; every projection kink-free and 20 - 80 %
clamped, asserted there in ``inputs``; the forward pass is that sweep's).  Reference: ``restated()`` with the PSF as a leaf and
``init`` passed explicitly, computed from the DETACHED PSF -- the default start value is a constant in the reference's
``forward(batch, psfs=...)``, which rebuilds the convolver and nothing else: it stays (max + min) / 2 of the CONSTRUCTOR's
PSF.  Every ``psfs`` here has the constructor's values, so the two coincide; tests/test_psf_swap.py passes another PSF and
tells them apart -- loss ``(out * w).sum()``.
The restatement with a PSF leaf is itself pinned to the reference's own ``psfs`` gradient
(tests/golden/gen_unrolled_psf_grad.py, test_restatement_with_psf_leaf_is_pinned).

Bounds (the sweep's rule; max-norm over whole arrays, relative to the max of the float64 array):
  float32 engine:  rel(g_psf, ref64) <= 4 * max(rel(ref32, ref64), 2e-6), ref32 the float32 restatement (or the fixture's
                   own float32 run);
  float64 engine:  <= 100 * F64_TOL = 1e-9;
and in the same run out, g_alpha, g_tk and g_data meet the bounds of the sweep.
"""
import functools
import os

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from test_unrolled_grad_sweep import CASES, inputs
from unrolled_restated import F64_TOL, PLANS, rec_padded, rel, restated

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = "unrolled_fista_psf_grad_12x30x3_b2"
ROW_PLANS = ["rows_half", "rows_paired"]
BATCH2_CASES = [c for c in CASES if CASES[c]["shape"][3] == 2]


def default_init(psf):
    """the constructor's start value, gd.py:100-105, of a DETACHED PSF: (1, D, H, W, C)"""
    p = psf.detach()
    flat = p.reshape(-1, p.shape[-1])
    return torch.ones_like(p[None]) * ((flat.max(0).values + flat.min(0).values) / 2)


def restated_psf_grad(psf, data, w, alpha, tk, n, tdt):
    """out and d (out * w).sum() / d psf of the restatement in ``tdt``, the PSF a leaf, the start value a constant"""
    p = torch.from_numpy(psf).to(tdt).requires_grad_()
    out, _ = restated(p, torch.from_numpy(data).to(tdt), torch.from_numpy(alpha).to(tdt), torch.from_numpy(tk), n,
                      init=default_init(p), dtype=tdt)
    (out * torch.from_numpy(w).to(tdt)).sum().backward()
    return out.detach().numpy(), p.grad.numpy()


@functools.lru_cache(maxsize=None)
def psf_refs(name, frame=None):
    """float64 / float32 reference PSF gradient of a sweep case (``frame``: of that frame of the batch alone); computed
    once, never written to"""
    inp = inputs(name)
    sel = slice(None) if frame is None else slice(frame, frame + 1)
    return {tdt: restated_psf_grad(inp.psf, inp.data[sel], inp.w[sel], inp.alpha, inp.tk, inp.n, tdt)[1]
            for tdt in (torch.float64, torch.float32)}


def bound_of(dtype, ref32, ref64, key="g_psf"):
    if dtype == "float64":
        return 5e-7 if key == "g_tk" else 100 * F64_TOL
    return 4 * max(rel(ref32, ref64), 2e-6)


def engine_run(inp, dtype, backend, frame=None, how="forward"):
    tdt = torch.float64 if dtype == "float64" else torch.float32
    dev = backend.device
    sel = slice(None) if frame is None else slice(frame, frame + 1)
    rec = lpa.UnrolledFISTA(torch.from_numpy(inp.psf).to(dev), n_iter=inp.n, dtype=dtype)
    rec.set_parameters(alpha=inp.alpha, tk=inp.tk)
    p = torch.from_numpy(inp.psf).to(device=dev, dtype=tdt).requires_grad_()
    batch = torch.from_numpy(inp.data[sel]).to(device=dev, dtype=tdt).requires_grad_()
    if how == "forward":
        out = rec(batch, psfs=p)
    else:
        rec._set_psf(p)
        out = rec(batch)
    (out * torch.from_numpy(inp.w[sel]).to(device=dev, dtype=tdt)).sum().backward()
    return rec, p, {"out": out, "g_alpha": rec._alpha_p.grad, "g_tk": rec._tk_p.grad, "g_data": batch.grad, "g_psf": p.grad}


def check_case(monkeypatch, name, plan, dtype, backend):
    opts, marker = PLANS[plan]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **CASES[name].get("opts", {}), **opts})
    inp = inputs(name)
    rec, p, got = engine_run(inp, dtype, backend)
    info = rec._handle.plan_info()
    assert tuple(rec._padded_shape[1:3]) == CASES[name]["padded"] and marker in info, info
    assert CASES[name].get("info", "columns: single pass") in info, info
    ref64 = {**inp.ref[torch.float64], "g_psf": psf_refs(name)[torch.float64]}
    ref32 = {**inp.ref[torch.float32], "g_psf": psf_refs(name)[torch.float32]}
    bad = []
    for k, want in ref64.items():
        assert got[k] is not None and tuple(got[k].shape) == want.shape, (k, got[k])
        r, bound = rel(got[k], want), bound_of(dtype, ref32[k], want, k)
        print(f"{name} {plan} {dtype} {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))
    assert not bad, bad
    assert p.grad.dtype == p.dtype and p.grad.device == p.device


# ------------------------------------------------------------------------------------------------- CPU only --
def test_restatement_with_psf_leaf_is_pinned():
    """the float64 restatement with the PSF as a leaf and a constant start value against the reference's own float64 output
    and ``psfs`` gradient; its float32 flavour is no further from them than the reference's own float32 run allows"""
    g = np.load(os.path.join(GOLDEN, FIXTURE + ".npz"))
    n = int(g["n_iter"])
    assert g["psf"].shape == (1, 12, 30, 3) and g["data"].shape == (2, 1, 12, 30, 3) and n == 4
    assert float(g["data"].min()) < 0 and g["clamped"].shape == (n + 1,)
    assert 0.2 <= float(g["clamped"].min()) and float(g["clamped"].max()) <= 0.8
    out, gp = restated_psf_grad(g["psf"], g["data"], g["w"], g["alpha"], g["tk"], n, torch.float64)
    for k, v in (("out", out), ("g_psf", gp)):
        r = rel(v, g[k + "64"])
        print(f"restated float64 {k}: rel {r:.3e} (bound {100 * F64_TOL:.1e})")
        assert v.shape == g[k + "64"].shape and r <= 100 * F64_TOL, (k, r)
    out, gp = restated_psf_grad(g["psf"], g["data"], g["w"], g["alpha"], g["tk"], n, torch.float32)
    for k, v in (("out", out), ("g_psf", gp)):
        r, bound = rel(v, g[k + "64"]), bound_of("float32", g[k + "32"], g[k + "64"])
        print(f"restated float32 {k}: rel {r:.3e} (bound {bound:.1e})")
        assert r <= bound, (k, r, bound)


# ----------------------------------------------------------------------------------------- emulator and card --
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("plan", ROW_PLANS)
@pytest.mark.parametrize("name", list(CASES))
def test_psf_gradient_parity(backend, monkeypatch, name, plan, dtype):
    check_case(monkeypatch, name, plan, dtype, backend)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_psf_gradient_parity_plan_module(backend, monkeypatch, dtype):
    check_case(monkeypatch, "12x30", "module", dtype, backend)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", BATCH2_CASES)
def test_batch_sum_is_the_sum_of_the_frames(backend, monkeypatch, name, dtype):
    """g_psf of a batch of two = g_psf of frame 0 alone + g_psf of frame 1 alone"""
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **CASES[name].get("opts", {})})
    inp = inputs(name)
    both = engine_run(inp, dtype, backend)[2]["g_psf"]
    singles = []
    for b in range(2):
        g1 = engine_run(inp, dtype, backend, frame=b)[2]["g_psf"]
        r, bound = rel(g1, psf_refs(name, b)[torch.float64]), bound_of(dtype, psf_refs(name, b)[torch.float32],
                                                                     psf_refs(name, b)[torch.float64])
        print(f"{name} {dtype} frame {b}: rel {r:.3e} (bound {bound:.1e})")
        assert r <= bound, (b, r, bound)
        singles.append(g1)
    refs = psf_refs(name)
    r, bound = rel(singles[0] + singles[1], both), bound_of(dtype, refs[torch.float32], refs[torch.float64])
    print(f"{name} {dtype} frame 0 + frame 1 against the batch: rel {r:.3e} (bound {bound:.1e})")
    assert r <= bound, (r, bound)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("plan", ROW_PLANS)
def test_psf_gradient_against_the_reference(backend, monkeypatch, plan, dtype):
    """the engine against the reference's own gradient w.r.t. a leaf ``psfs`` (fixture of gen_unrolled_psf_grad.py)"""
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **PLANS[plan][0]})
    g = np.load(os.path.join(GOLDEN, FIXTURE + ".npz"))
    tdt = torch.float64 if dtype == "float64" else torch.float32
    dev = backend.device
    rec = lpa.UnrolledFISTA(torch.from_numpy(g["psf"]).to(dev), n_iter=int(g["n_iter"]), dtype=dtype)
    rec.set_parameters(alpha=g["alpha"], tk=g["tk"])
    p = torch.from_numpy(g["psf"]).to(device=dev, dtype=tdt).requires_grad_()
    out = rec(torch.from_numpy(g["data"]).to(device=dev, dtype=tdt), psfs=p)
    (out * torch.from_numpy(g["w"]).to(device=dev, dtype=tdt)).sum().backward()
    assert PLANS[plan][1] in rec._handle.plan_info()
    bad = []
    for k, v in (("out", out), ("g_psf", p.grad)):
        assert v is not None, k
        r, bound = rel(v, g[k + "64"]), bound_of(dtype, g[k + "32"], g[k + "64"])
        print(f"fixture {plan} {dtype} {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))
    assert not bad, bad


def psf_workspace_bytes(B, H, W, C, itemsize):
    """include/lpc.h, lpc_fista_backward_psf"""
    Hp, Wp = rec_padded(H), rec_padded(W)
    cpitch = (Wp // 2 + 1 + 15) // 16 * 16
    return 3 * B * C * Hp * cpitch * 2 * itemsize + B * C * H * W * itemsize


@pytest.mark.parametrize("how", ["forward", "set_psf"])
def test_both_ways_in(backend, how):
    """``rec(batch, psfs=p)`` and ``rec._set_psf(p); rec(batch)``: p.grad has p's shape, dtype and device, and the value of
    the float64 restatement; a second backward pass accumulates; the backward is deterministic"""
    inp = inputs("12x30")
    rec, p, got = engine_run(inp, "float64", backend, how=how)
    want = psf_refs("12x30")[torch.float64]
    assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device == p.device
    assert rel(p.grad, want) <= 100 * F64_TOL
    first = p.grad.clone()
    dev = backend.device
    batch = torch.from_numpy(inp.data).to(device=dev, dtype=torch.float64)
    out = rec(batch, psfs=p) if how == "forward" else rec(batch)
    (out * torch.from_numpy(inp.w).to(device=dev, dtype=torch.float64)).sum().backward()
    assert torch.equal(p.grad, first + first)          # the same bits again, added like into any leaf


def test_psf_correction_network_trains(backend):
    """``rec(batch, psfs=psf + net(psf))`` with a one-parameter net: the parameter's gradient is autograd's over the
    restatement (float64 build), started like the reference's from the default of the CONSTRUCTOR's PSF (the net changes the
    PSF's maximum: unrolled_fista.py:55-59, tests/test_psf_swap.py)"""
    inp = inputs("12x30")
    dev = backend.device
    psf = torch.from_numpy(inp.psf).double()
    w = torch.from_numpy(inp.w).double()

    def net(theta, x):
        return theta * x * (1 - x)

    theta = torch.tensor(0.3, dtype=torch.float64, device=dev, requires_grad=True)
    rec = lpa.UnrolledFISTA(psf.to(dev), n_iter=inp.n, dtype="float64")
    rec.set_parameters(alpha=inp.alpha, tk=inp.tk)
    out = rec(torch.from_numpy(inp.data).double().to(dev), psfs=psf.to(dev) + net(theta, psf.to(dev)))
    (out * w.to(dev)).sum().backward()
    rtheta = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    eff = psf + net(rtheta, psf)
    rout, _ = restated(eff, torch.from_numpy(inp.data), torch.from_numpy(inp.alpha).double(), torch.from_numpy(inp.tk), inp.n,
                       init=default_init(psf))
    (rout * w).sum().backward()
    assert theta.grad is not None and theta.grad.shape == theta.shape
    r = abs(float(theta.grad) - float(rtheta.grad)) / abs(float(rtheta.grad))
    print(f"d loss / d theta: engine {float(theta.grad):.12e}, restated {float(rtheta.grad):.12e}, rel {r:.3e}")
    assert rel(out, rout.detach().numpy()) <= 100 * F64_TOL and r <= 100 * F64_TOL


def test_workspace(backend):
    """no PSF gradient asked for: the workspace is base + tape as before and p.grad stays None; asked for: + the documented
    formula, and release_tape() gives all of it back"""
    inp = inputs("12x30")
    H, W, C, B, n = CASES["12x30"]["shape"]
    dev = backend.device
    rec = lpa.UnrolledFISTA(torch.from_numpy(inp.psf).to(dev), n_iter=n)
    rec.set_parameters(alpha=inp.alpha, tk=inp.tk)
    data = torch.from_numpy(inp.data).to(dev)
    wts = torch.from_numpy(inp.w).to(dev)
    with torch.no_grad():
        rec(data)
    base = rec._handle.workspace_bytes()
    tape = (2 * n + 4) * B * C * H * W * 4 + n * B * C * H * 2 * 8     # include/lpc.h: lpc_fista_record
    p = torch.from_numpy(inp.psf).to(dev)
    (rec(data, psfs=p) * wts).sum().backward()
    assert rec._handle.workspace_bytes() == base + tape and p.grad is None and rec._alpha_p.grad is not None
    p = p.clone().requires_grad_()
    out = rec(data, psfs=p)
    assert rec._handle.workspace_bytes() == base + tape      # allocated by the first backward that needs it
    (out * wts).sum().backward()
    extra = psf_workspace_bytes(B, H, W, C, 4)
    assert p.grad is not None and rec._handle.workspace_bytes() == base + tape + extra
    with torch.no_grad():          # a pause keeps it
        rec(data)
    assert rec._handle.workspace_bytes() == base + tape + extra
    rec.release_tape()
    assert rec._handle.workspace_bytes() == base
    (rec(data, psfs=p) * wts).sum().backward()
    assert rec._handle.workspace_bytes() == base + tape + extra


def test_refusals(backend):
    rng = np.random.default_rng(0)
    dev = backend.device

    def solver(h, w, d=1):
        psf = torch.from_numpy(rng.random((d, h, w, 3)).astype(np.float32)).to(dev)
        rec = lpa.UnrolledFISTA(psf, n_iter=3)
        return rec, psf.clone().requires_grad_(), torch.from_numpy(rng.random((2, 1, h, w, 3)).astype(np.float32)).to(dev)

    rec, p, data = solver(10, 12)
    with pytest.raises(NotImplementedError, match="per-frame"):
        rec(data, psfs=torch.stack([p, p]))
    rec, p, data = solver(8, 12)                            # padded 15 x 24
    assert rec._padded_shape[1] == 15
    out = rec(data, psfs=p)
    with pytest.raises(NotImplementedError, match="odd"):
        out.sum().backward()
    rec, p, data = solver(10, 12, d=2)
    out = rec(data, psfs=p)
    with pytest.raises(NotImplementedError, match="depth"):
        out.sum().backward()
    # native level: no tape; and the old entry point with its old argument list
    rec, p, data = solver(10, 12)
    with torch.no_grad():
        out = rec(data)
    go = torch.ones(out.numel(), dtype=torch.float32, device=dev)
    buf = torch.zeros(out.numel(), dtype=torch.float32, device=dev)
    gp = torch.zeros(p.numel(), dtype=torch.float32, device=dev)
    h, ptrs = rec._handle, (go.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), None)
    with pytest.raises(_native.NativeError, match="nothing recorded"):
        h.fista_backward_psf(*ptrs, gp.data_ptr(), 0)
    rec(data)
    h = rec._handle
    h.fista_backward(*ptrs, 0)
    h.fista_backward_psf(*ptrs, gp.data_ptr(), 0)
    assert float(gp.abs().max()) > 0
