"""
Reverse mode of unrolled FISTA (lpc_fista_record / lpc_fista_backward, UnrolledFISTA as an nn.Module) against the
gradients of the REAL reference's ``forward()`` + ``backward()`` (tests/golden/gen_unrolled_grad.py), through the public
API, on the SIMT emulator ('emu') and on the MI355X ('hip', -m gpu).

Bounds (max-norm over whole arrays, relative to the max of the reference array):
  float32 engine:  rel(q, ref64) <= 4 * max(rel(ref32, ref64), 2e-6) -- the yardstick is the reference's own float32
                   noise stored in the fixture, 2e-6 the project's float32 operator tolerance, the factor 4 allows for
                   another FFT factorisation and summation order;
  float64 engine:  <= 100 * F64_TOL = 1e-9 for alpha_p.grad and batch.grad, <= 5e-7 for tk_p.grad (the reference keeps
                   _tk_p and its gradient in float32).
tests/test_unrolled_grad_sweep.py carries the shape / plan / option sweep with ACTIVE masks (20 - 80 % clamped in every
projection): reference there is the float64 / float32 restatement of tests/unrolled_restated.py, itself pinned to these
fixtures; same bound rule; largest measured distance on the MI355X: float32 2.5e-6 (g_tk, bound 8.9e-6), float64 8.6e-15.
"""
import os

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from unrolled_restated import F64_TOL, PLANS, rel, restated

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["unrolled_fista_grad_24x32x3_b3", "unrolled_fista_grad_19x27x1_b2", "unrolled_fista_grad_20x28_gray_rgb"]


def run(g, dtype, backend):
    tdt = torch.float64 if dtype == "float64" else torch.float32
    rec = lpa.UnrolledFISTA(torch.from_numpy(g["psf"]).to(backend.device), n_iter=int(g["n_iter"]), tk=float(g["tk0"]),
                            dtype=dtype)
    rec.set_parameters(alpha=g["alpha"], tk=g["tk"])
    batch = torch.from_numpy(g["data"]).to(device=backend.device, dtype=tdt).requires_grad_()
    out = rec(batch)
    (out * torch.from_numpy(g["w"]).to(device=backend.device, dtype=tdt)).sum().backward(retain_graph=True)
    return rec, batch, out


def check_parity(g, dtype, backend, tag):
    rec, batch, out = run(g, dtype, backend)
    got = {"out": out, "g_alpha": rec._alpha_p.grad, "g_tk": rec._tk_p.grad, "g_data": batch.grad}
    bad = []
    for k, v in got.items():
        r = rel(v, g[k + "64"])
        if dtype == "float64":
            bound = 5e-7 if k == "g_tk" else 100 * F64_TOL
        else:
            bound = 4 * max(rel(g[k + "32"], g[k + "64"]), 2e-6)
        print(f"{tag} {dtype} {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))
    assert not bad, bad
    return rec


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", FIXTURES)
def test_gradient_parity(backend, name, dtype):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    check_parity(g, dtype, backend, name)


@pytest.mark.gpu
def test_gradient_parity_diffusercam_size():
    """270 x 480 x 3, B = 2, n = 5 (padded 540 x 960: 480-point half rows, the pre-built plan module), inputs in closed
    form, float32 engine; out / batch.grad compared on the fixture's crops + lattice of the whole frame.  GPU only: the
    frame takes minutes on the emulator."""
    import sys
    from types import SimpleNamespace

    from lenslesspicam_amd import recon

    backend = SimpleNamespace(device=recon.runtime()[1])
    sys.path.insert(0, GOLDEN)
    import longrun_inputs as lin

    g = np.load(os.path.join(GOLDEN, "unrolled_fista_grad_c1.npz"))
    B, H, W, C = (int(v) for v in g["shape"])
    seed, n = int(g["seed"]), int(g["n_iter"])
    psf = lin.psf12(1, H, W, C, 100 + seed)
    data = np.stack([lin.measurement(H, W, C, 10 * seed + b) for b in range(B)])[:, None]
    w = np.random.default_rng(300 + seed).random((B, 1, H, W, C), dtype=np.float32) - np.float32(0.5)
    for a, fp in ((psf, "fp_psf"), (data, "fp_data"), (w, "fp_w")):
        assert np.array_equal(lin.fingerprint(a), g[fp]), fp
    rec = lpa.UnrolledFISTA(torch.from_numpy(psf).to(backend.device), n_iter=n, tk=float(g["tk0"]))
    rec.set_parameters(alpha=g["alpha"], tk=g["tk"])
    assert "reverse rows: plan module" in rec._handle.plan_info() and "half-length 480" in rec._handle.plan_info()
    batch = torch.from_numpy(data).to(backend.device).requires_grad_()
    out = rec(batch)
    (out * torch.from_numpy(w).to(backend.device)).sum().backward()
    bad = []

    def check(k, r):
        bound = 4 * max(float(g["rel32_" + k]), 2e-6)
        print(f"c1 float32 {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))

    check("g_alpha", rel(rec._alpha_p.grad, g["g_alpha64"]))
    check("g_tk", rel(rec._tk_p.grad, g["g_tk64"]))
    for k, arr in (("out", out), ("g_data", batch.grad)):
        arr = arr.detach().cpu().numpy()
        parts = [lin.samples(arr[b, 0]) for b in range(B)]
        crops, lattice = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
        err = max(np.abs(crops - g[k + "64_crops"]).max(), np.abs(lattice - g[k + "64_lattice"]).max())
        check(k, float(err) / float(g[k + "64_max"]))
    assert not bad, bad


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("name", FIXTURES[:2])
def test_gradient_parity_every_kernel_family(backend, monkeypatch, name, plan):
    opts, marker = PLANS[plan]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **opts})
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    for dtype in ("float32", "float64"):
        rec = check_parity(g, dtype, backend, name + " " + plan)
        assert marker in rec._handle.plan_info(), rec._handle.plan_info()


def test_recorded_forward_is_bit_equal(backend):
    g = np.load(os.path.join(GOLDEN, FIXTURES[0] + ".npz"))
    rec, batch, out = run(g, "float32", backend)
    with torch.no_grad():
        plain = rec(batch.detach())
    assert not plain.requires_grad and torch.equal(plain, out.detach())
    old = np.load(os.path.join(GOLDEN, "unrolled_fista_24x32x3_b3.npz"))
    rec = lpa.UnrolledFISTA(torch.from_numpy(old["psf"]).to(backend.device), n_iter=int(old["n_iter"]))
    rec.set_parameters(alpha=old["alpha"], tk=old["tk"])
    out = rec(torch.from_numpy(old["data"]).to(backend.device))
    assert out.requires_grad and rel(out, old["out"]) <= 5e-6


def test_backward_is_deterministic(backend):
    g = np.load(os.path.join(GOLDEN, FIXTURES[0] + ".npz"))
    rec, batch, out = run(g, "float32", backend)
    first = [t.grad.clone() for t in (rec._alpha_p, rec._tk_p, batch)]
    for t in (rec._alpha_p, rec._tk_p, batch):
        t.grad = None
    (out * torch.from_numpy(g["w"]).to(backend.device)).sum().backward(retain_graph=True)
    for a, t in zip(first, (rec._alpha_p, rec._tk_p, batch)):
        assert torch.equal(a, t.grad)


def test_it_trains(backend):
    """10 SGD steps on alpha_p, tk_p towards the fixture's float64 output: the loss falls, and the parameters equal those
    of the same loop driven by torch.autograd over the restated formula (float64 build, 100 * F64_TOL)"""
    g = np.load(os.path.join(GOLDEN, FIXTURES[1] + ".npz"))
    n, dev = int(g["n_iter"]), backend.device
    rec = lpa.UnrolledFISTA(torch.from_numpy(g["psf"]).to(dev), n_iter=n, tk=float(g["tk0"]), dtype="float64")
    rec.set_parameters(alpha=g["alpha"] * 0.8, tk=g["tk"] * 1.05)
    ap = rec._alpha_p.detach().cpu().clone().requires_grad_()
    tp = rec._tk_p.detach().cpu().clone().requires_grad_()
    assert ap.dtype == torch.float64 and tp.dtype == torch.float32
    target, data = torch.from_numpy(g["out64"]), torch.from_numpy(g["data"]).double()
    a_scale = float(np.abs(g["alpha"]).max())
    norm = float((target ** 2).mean())

    def loop(params, model):
        opt = torch.optim.SGD([{"params": [params[0]], "lr": 0.05 * a_scale ** 2}, {"params": [params[1]], "lr": 1e-3}])
        losses = []
        for _ in range(10):
            opt.zero_grad()
            loss = ((model() - target.to(params[0].device)) ** 2).mean() / norm
            loss.backward()
            losses.append(float(loss.detach()))
            opt.step()
        return losses

    # the restatement itself against the fixture: the reference's own float64 gradients
    fa, ft = torch.from_numpy(g["alpha"]).double().requires_grad_(), torch.from_numpy(g["tk"]).requires_grad_()
    (restated(torch.from_numpy(g["psf"]), data, fa, ft, n)[0] * torch.from_numpy(g["w"]).double()).sum().backward()
    assert rel(fa.grad, g["g_alpha64"]) <= 100 * F64_TOL and rel(ft.grad, g["g_tk64"]) <= 5e-7
    losses = loop([rec._alpha_p, rec._tk_p], lambda: rec(data.to(dev)))
    ref_losses = loop([ap, tp], lambda: restated(torch.from_numpy(g["psf"]), data, ap, tp, n)[0])
    print("losses", losses, "restated", ref_losses)
    assert losses[-1] < losses[0] and ref_losses[-1] < ref_losses[0]
    ra, rt = rel(rec._alpha_p, ap.detach().numpy()), rel(rec._tk_p, tp.detach().numpy())
    print(f"after 10 steps: alpha_p rel {ra:.3e}, tk_p rel {rt:.3e} (bound {100 * F64_TOL:.0e})")
    assert ra <= 100 * F64_TOL and rt <= 100 * F64_TOL


def test_initial_estimate_gradient(backend):
    """dL/d(initial estimate) -- one estimate shared by the batch: the sum over its items -- against torch.autograd over the
    restated formula (float64 build)"""
    g = np.load(os.path.join(GOLDEN, FIXTURES[0] + ".npz"))
    n, dev = int(g["n_iter"]), backend.device
    psf, data, w = torch.from_numpy(g["psf"]), torch.from_numpy(g["data"]).double(), torch.from_numpy(g["w"]).double()
    rng = np.random.default_rng(3)
    for nb in (1,):     # (the constructor takes one estimate for the batch)
        init = torch.from_numpy(rng.random((nb,) + tuple(psf.shape)) * 0.1)
        est = init.clone().to(dev).requires_grad_()
        rec = lpa.UnrolledFISTA(psf.to(dev), n_iter=n, dtype="float64", initial_est=est)
        rec.set_parameters(alpha=g["alpha"], tk=g["tk"])
        (rec(data.to(dev)) * w.to(dev)).sum().backward()
        ri = init.clone().requires_grad_()
        ap, tp = torch.from_numpy(g["alpha"]).double().requires_grad_(), torch.from_numpy(g["tk"]).requires_grad_()
        (restated(psf, data, ap, tp, n, init=ri)[0] * w).sum().backward()
        got = est.grad
        assert got is not None and tuple(got.shape) == tuple(ri.grad.shape)
        r = rel(got, ri.grad.numpy())
        print(f"initial estimate ({nb} for the batch): rel {r:.3e}")
        assert r <= 100 * F64_TOL and rel(rec._alpha_p.grad, ap.grad.numpy()) <= 100 * F64_TOL


def test_refusals(backend):
    rng = np.random.default_rng(0)
    dev = backend.device

    def solver(h, w, d=1, **kw):
        psf = rng.random((d, h, w, 3)).astype(np.float32)
        rec = lpa.UnrolledFISTA(torch.from_numpy(psf).to(dev), n_iter=3, **kw)
        return rec, torch.from_numpy(rng.random((2, 1, h, w, 3)).astype(np.float32)).to(dev)

    def forward_only_works(rec, data, expect):
        with torch.no_grad():
            again = rec(data)
        assert not again.requires_grad and torch.equal(again, expect.detach())

    rec, data = solver(8, 12)                               # padded 15 x 24
    assert rec._padded_shape[1] == 15
    out = rec(data)
    with pytest.raises(NotImplementedError, match="odd"):
        out.sum().backward()
    forward_only_works(rec, data, out)
    with pytest.raises(_native.NativeError, match="odd"):   # the C entry point refuses it itself
        rec(data)
        buf = torch.zeros(out.numel(), dtype=torch.float32, device=dev)
        rec._handle.fista_backward(buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), None, 0)
    rec, data = solver(10, 12, d=2)
    out = rec(data)
    with pytest.raises(NotImplementedError, match="depth"):
        out.sum().backward()
    forward_only_works(rec, data, out)
    rec, data = solver(10, 12)
    first = rec(data)
    rec(data)
    with pytest.raises(RuntimeError, match="tape overwritten"):
        first.sum().backward()
    forward_only_works(rec, data, first)
    # a custom projection is not differentiated: with gradients asked for the refusal is a NotImplementedError; without
    # them it runs as split iterations on the schedule (tests/test_hooks_over_plans.py has the parity) -- here non_neg in
    # disguise against the fused forward -- and a handle that is writing its tape refuses a split iteration itself
    rec, data = solver(10, 12, proj=lambda x: torch.clamp(x, min=0.0))
    with pytest.raises(NotImplementedError, match="non_neg"):
        rec(data)
    with torch.no_grad():
        hooked = rec(data)
    fused = lpa.UnrolledFISTA(rec._psf, n_iter=3)
    with torch.no_grad():
        want = fused(data)
    assert float(want.abs().max()) > 0 and rel(hooked, want) <= 2e-6
    fused(data)                                               # (the parameters require gradients: this forward records)
    with pytest.raises(_native.NativeError, match="records a tape"):
        fused._handle.iterate_begin()
    # raw ABI: a FISTA handle without a schedule
    fis = lpa.FISTA(torch.from_numpy(rng.random((1, 10, 12, 3)).astype(np.float32)).to(dev))
    buf = torch.zeros(2 * 10 * 12 * 3, dtype=torch.float32, device=dev)
    with pytest.raises(_native.NativeError, match="no schedule"):
        fis._handle.fista_backward(buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), None, 0)
    # raw ABI: a new schedule or new data after the recorded iterations invalidates the tape
    rec, data = solver(10, 12)
    out = rec(data)
    h, ptrs = rec._handle, (buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), None, 0)
    h.fista_backward(*ptrs)
    h.set_fista_schedule([[1e-3] * 3] * 3, [0.1] * 3, 0)
    with pytest.raises(_native.NativeError, match="nothing recorded"):
        h.fista_backward(*ptrs)
    rec._sched_key = None
    out = rec(data)
    h.fista_backward(*ptrs)
    h.set_data(rec._data_dev.data_ptr(), 3, 0)
    with pytest.raises(_native.NativeError, match="nothing recorded"):
        h.fista_backward(*ptrs)


def test_module_surface(backend):
    g = np.load(os.path.join(GOLDEN, FIXTURES[0] + ".npz"))
    psf, n = torch.from_numpy(g["psf"]).to(backend.device), int(g["n_iter"])
    rec = lpa.UnrolledFISTA(psf, n_iter=n)
    assert isinstance(rec, torch.nn.Module)
    assert [tuple(p.shape) for p in rec.parameters()] == [(n, 3), (n + 1,)]
    assert list(rec.state_dict().keys()) == ["_alpha_p", "_tk_p"]
    assert list(lpa.UnrolledFISTA(psf, n_iter=n, learn_tk=False).state_dict().keys()) == ["_alpha_p"]
    assert list(lpa.UnrolledFISTA(psf, n_iter=n, skip_unrolled=True).parameters()) == []
    data = torch.from_numpy(g["data"]).to(backend.device)
    with torch.no_grad():
        rec(data)
    base = rec._handle.workspace_bytes()
    rec(data)
    B, _, H, W, C = data.shape
    tape = (2 * n + 4) * B * C * H * W * 4 + n * B * C * H * 2 * 8     # include/lpc.h: lpc_fista_record
    assert rec._handle.workspace_bytes() == base + tape
    with torch.no_grad():          # evaluation between training steps pauses the recording, the tape stays
        rec(data)
    assert rec._handle.workspace_bytes() == base + tape
    rec.release_tape()
    assert rec._handle.workspace_bytes() == base
    out = rec(data)
    assert rec._handle.workspace_bytes() == base + tape
    out.sum().backward()
    assert rec._alpha_p.grad is not None
