"""
Reverse mode of unrolled ADMM (lpc_admm_record / lpc_admm_backward, UnrolledADMM as an nn.Module) against the gradients of
the REAL reference's ``forward()`` + ``backward()`` (tests/golden/gen_unrolled_admm_grad.py), through the public API, on
the SIMT emulator ('emu') and on the MI355X ('hip', -m gpu).

Bounds (max-norm over whole arrays, relative to the max of the reference array):
  float32 engine:  rel(q, ref64) <= 4 * max(rel(ref32, ref64), 2e-6) for every quantity q -- the yardstick is the
                   reference's own float32 noise stored in the fixture, 2e-6 the project's float32 operator tolerance, the
                   factor 4 allows for another FFT factorisation and summation order;
  float64 engine:  <= 100 * F64_TOL = 1e-9 against the float64 values of the restatement stored in the fixture
                   (tests/unrolled_admm_restated.py, itself pinned to the reference below: the reference keeps the
                   parameters, their gradients and tau / mu2 in float32 and is no float64 yardstick).  The four parameter
                   gradients are compared as lpc_admm_backward writes them, in float64; ``_mu1_p.grad`` etc. are float32
                   tensors and must be exactly those values rounded.
The small fixtures are free of kink elements and have 5 - 95 % of U non-zero and of q positive from the second iteration
on (asserted by the generator on the reference alone); the DiffuserCam-sized one is compared on crops + lattice, kinks
and all, like the FISTA one.

Largest distances measured on the MI355X (30 cases of this file on the 'hip' backend):
  quantity     small fixtures, float32 (bound)   270 x 480 x 3, float32 (bound)   float64 engine
  out               6.7e-7  (8.0e-6)                  7.0e-7  (1.2e-5)                1.5e-15
  batch.grad        7.1e-7  (8.0e-6)                  6.8e-4  (5.8e-3)                1.4e-15
  g_mu1             1.7e-6  (8.0e-6)                  6.8e-5  (4.4e-4)                3.6e-14
  g_mu2             1.0e-5  (8.9e-5); 3.4e-6 (8.0e-6) 2.1e-3  (8.9e-3)                5.5e-14
  g_mu3             4.0e-6  (8.0e-6)                  2.3e-4  (7.4e-4)                8.3e-15
  g_tau             1.2e-6  (8.0e-6)                  1.6e-3  (6.7e-3)                2.9e-15
(the large frame has 757 elements on a kink in the reference's float64 run: its yardsticks, the reference's own float32
run, are that large); ten SGD steps in float64 end on the restatement's parameters exactly.
"""
import os
import sys

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from unrolled_admm_restated import F64_PLANS, F64_TOL, NAMES, PLANS, activity, rel, restated_admm, restated_grads

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["unrolled_admm_grad_19x27x1_b2", "unrolled_admm_grad_16x20x3_b2", "unrolled_admm_grad_16x20_gray_rgb"]
PLAN_FIXTURES = sorted({p["fixture"] for p in PLANS.values()})
KEYS = ("out", "g_data") + tuple("g_" + k for k in NAMES)
BASE = dict(mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-7)


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def sched_of(g):
    return {k: g[k] for k in NAMES}


def params_of(rec):
    return [getattr(rec, f"_{k}_p") for k in NAMES]


def solver(g, dtype, backend, sched=None):
    rec = lpa.UnrolledADMM(torch.from_numpy(g["psf"]).to(backend.device), dtype=dtype, n_iter=int(g["n_iter"]), **BASE)
    rec.set_parameters(**(sched_of(g) if sched is None else sched))
    return rec


def run(g, dtype, backend, sched=None):
    tdt = torch.float64 if dtype == "float64" else torch.float32
    rec = solver(g, dtype, backend, sched)
    batch = torch.from_numpy(g["data"]).to(device=backend.device, dtype=tdt).requires_grad_()
    out = rec(batch)
    (out * torch.from_numpy(g["w"]).to(device=backend.device, dtype=tdt)).sum().backward(retain_graph=True)
    return rec, batch, out


def raw_backward(rec, grad_out):
    """lpc_admm_backward itself, on the tape of the last forward: (4, n) in the solver's dtype"""
    gp = rec._empty((4, rec._n_iter))
    go = rec._to_dev(grad_out)
    rec._handle.admm_backward(go.data_ptr(), None, *(gp[k].data_ptr() for k in range(4)), rec._stream())
    return gp


def check_parity(g, dtype, backend, tag):
    rec, batch, out = run(g, dtype, backend)
    got = {"out": out, "g_data": batch.grad}
    got.update({"g_" + k: p.grad for k, p in zip(NAMES, params_of(rec))})
    bad = []
    if dtype == "float64":
        raw = raw_backward(rec, torch.from_numpy(g["w"]).double())
        for i, (k, p) in enumerate(zip(NAMES, params_of(rec))):
            assert p.grad.dtype == torch.float32
            assert torch.equal(p.grad.cpu(), (raw[i].cpu() * torch.sign(p.detach().cpu()).double()).float()), k
            got["g_" + k] = raw[i]
    for k, v in got.items():
        assert v is not None and float(np.abs(g[k + "64"]).max()) > 0, k
        if dtype == "float64":
            r, bound = rel(v, g["r_" + k]), 100 * F64_TOL
        else:
            r, bound = rel(v, g[k + "64"]), 4 * max(rel(g[k + "32"], g[k + "64"]), 2e-6)
        print(f"{tag} {dtype} {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))
    assert not bad, bad
    return rec


# ------------------------------------------------------------------------------------------------- CPU only --
@pytest.mark.parametrize("name", FIXTURES + [f for f in PLAN_FIXTURES if f not in FIXTURES])
def test_restatement_is_pinned_to_the_reference(name):
    """torch.autograd over the restatement against the reference's float64 run: batch.grad to 100 * F64_TOL, out to 1e-7,
    the parameter gradients to 5e-6 (the reference holds the parameters and tau / mu2 in float32); and the values stored
    in the fixture are what the restatement gives today"""
    g = load(name)
    res, args = restated_grads(g["psf"], g["data"], g["w"], sched_of(g), int(g["n_iter"]))
    act = activity(args)
    assert sum(a[2] for a in act) == 0 and all(0.05 <= a[0] <= 0.95 and 0.05 <= a[1] <= 0.95 for a in act[1:]), act
    for k in KEYS:
        r = rel(res[k], g[k + "64"])
        bound = 100 * F64_TOL if k == "g_data" else 1e-7 if k == "out" else 5e-6
        print(f"{name} restated {k}: rel {r:.3e} (bound {bound:.0e}), to the stored values {rel(res[k], g['r_' + k]):.1e}")
        assert r <= bound, (k, r, bound)
        assert rel(res[k], g["r_" + k]) <= F64_TOL, k


def test_the_check_has_teeth():
    """restatement alone: a backward that treats the soft threshold or the W clamp as the identity, or drops the dR/dm terms
    of the spectral step, moves some gradient by at least 100 x the float32 bound of that quantity"""
    g = load(FIXTURES[0])
    n = int(g["n_iter"])
    good, _ = restated_grads(g["psf"], g["data"], g["w"], sched_of(g), n)
    for tooth in ("soft", "clamp", "rdiv"):
        bad, _ = restated_grads(g["psf"], g["data"], g["w"], sched_of(g), n, teeth=(tooth,))
        assert rel(bad["out"], good["out"]) == 0.0          # (the forward is untouched)
        moved = {k: rel(bad[k], good[k]) / (4 * max(rel(g[k + "32"], g[k + "64"]), 2e-6)) for k in KEYS[1:]}
        print(tooth, {k: f"{v:.0f} x" for k, v in moved.items()})
        assert max(moved.values()) >= 100, (tooth, moved)
        if tooth == "rdiv":      # the terms only the parameter gradients have
            assert moved["g_data"] == 0.0 and min(moved[k] for k in ("g_mu1", "g_mu2", "g_mu3")) >= 100, moved


# ----------------------------------------------------------------------------------------- emulator and card --
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", FIXTURES)
def test_gradient_parity(backend, name, dtype):
    check_parity(load(name), dtype, backend, name)


@pytest.mark.parametrize("plan,dtype", [(p, "float32") for p in sorted(PLANS)] + [(p, "float64") for p in F64_PLANS])
def test_gradient_parity_every_launch_plan(backend, monkeypatch, plan, dtype):
    """the tape holds the iterates only and the backward replays the rest: the same gradients whatever form the forward's
    launch plan keeps H V, xi and the duals in"""
    case = PLANS[plan]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **case["opts"]})
    rec = check_parity(load(case["fixture"]), dtype, backend, plan)
    info = rec._handle.plan_info()
    for marker in case["info"] + case.get("f32" if dtype == "float32" else "f64", []):
        assert marker in info, (marker, info)


@pytest.mark.gpu
def test_gradient_parity_diffusercam_size():
    """270 x 480 x 3, B = 2, n = 5 (padded 540 x 960, the pre-built plan module), inputs in closed form, float32 engine;
    out / batch.grad compared on the fixture's crops + lattice of the whole frame.  GPU only: the frame takes minutes on
    the emulator."""
    from types import SimpleNamespace

    from lenslesspicam_amd import recon

    backend = SimpleNamespace(device=recon.runtime()[1])
    sys.path.insert(0, GOLDEN)
    import longrun_inputs as lin

    g = load("unrolled_admm_grad_c1")
    B, H, W, C = (int(v) for v in g["shape"])
    seed, n = int(g["seed"]), int(g["n_iter"])
    psf = lin.psf12(1, H, W, C, 100 + seed)
    data = np.stack([lin.measurement(H, W, C, 10 * seed + b) for b in range(B)])[:, None]
    w = np.random.default_rng(300 + seed).random((B, 1, H, W, C), dtype=np.float32) - np.float32(0.5)
    for a, fp in ((psf, "fp_psf"), (data, "fp_data"), (w, "fp_w")):
        assert np.array_equal(lin.fingerprint(a), g[fp]), fp
    rec = lpa.UnrolledADMM(torch.from_numpy(psf).to(backend.device), n_iter=n, **BASE)
    rec.set_parameters(**sched_of(g))
    batch = torch.from_numpy(data).to(backend.device).requires_grad_()
    out = rec(batch)
    info = rec._handle.plan_info()
    assert "padded 540x960" in info and "; plan module " in info, info
    (out * torch.from_numpy(w).to(backend.device)).sum().backward()
    bad = []

    def check(k, r):
        bound = 4 * max(float(g["rel32_" + k]), 2e-6)
        print(f"c1 float32 {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))

    for k, p in zip(NAMES, params_of(rec)):
        check("g_" + k, rel(p.grad, g["g_" + k + "64"]))
    for k, arr in (("out", out), ("g_data", batch.grad)):
        arr = arr.detach().cpu().numpy()
        parts = [lin.samples(arr[b, 0]) for b in range(B)]
        crops, lattice = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
        err = max(np.abs(crops - g[k + "64_crops"]).max(), np.abs(lattice - g[k + "64_lattice"]).max())
        check(k, float(err) / float(g[k + "64_max"]))
    assert not bad, bad


def test_recorded_forward_is_bit_equal(backend):
    g = load(FIXTURES[1])
    rec, batch, out = run(g, "float32", backend)
    with torch.no_grad():
        plain = rec(batch.detach())
    assert not plain.requires_grad and out.requires_grad and torch.equal(plain, out.detach())
    fresh = solver(g, "float32", backend)       # a solver that never recorded
    with torch.no_grad():
        assert torch.equal(fresh(batch.detach()), plain)
    old = load("unrolled_admm_24x32x3_b3")      # today's inference fixture, now through the recording forward
    rec = lpa.UnrolledADMM(torch.from_numpy(old["psf"]).to(backend.device), n_iter=int(old["n_iter"]), mu1=1e-6, mu2=1e-4,
                           mu3=4e-5, tau=2e-6)
    rec.set_parameters(**sched_of(old))
    out = rec(torch.from_numpy(old["data"]).to(backend.device))
    assert out.requires_grad and rel(out, old["out"]) <= 1e-5      # (test_oracle_golden.py: UNROLLED_TOL)


def test_backward_is_deterministic(backend):
    g = load(FIXTURES[1])
    rec, batch, out = run(g, "float32", backend)
    leaves = params_of(rec) + [batch]
    first = [t.grad.clone() for t in leaves]
    for t in leaves:
        t.grad = None
    (out * torch.from_numpy(g["w"]).to(backend.device)).sum().backward(retain_graph=True)
    for a, t in zip(first, leaves):
        assert float(a.abs().max()) > 0 and torch.equal(a, t.grad)


def test_negated_entries(backend):
    """the learnt values enter through abs (unrolled_admm.py:140-144): the same output bits, and the gradient of a negated
    entry flips its sign"""
    g = load(FIXTURES[0])
    rec, batch, out = run(g, "float32", backend)
    neg = {k: v.copy() for k, v in sched_of(g).items()}
    flipped = {"mu1": [0], "mu2": [2], "mu3": [4], "tau": [1, 3]}
    for k, idx in flipped.items():
        neg[k][idx] = -neg[k][idx]
    rec2, batch2, out2 = run(g, "float32", backend, sched=neg)
    assert torch.equal(out2.detach(), out.detach()) and torch.equal(batch2.grad, batch.grad)
    for k, p, p2 in zip(NAMES, params_of(rec), params_of(rec2)):
        sign = torch.ones_like(p.grad)
        sign[flipped[k]] = -1
        # (tau_0 thresholds zeros: its gradient is 0; every flipped entry has one)
        assert float(p.grad[flipped[k]].abs().min()) > 0 and torch.equal(p2.grad, p.grad * sign), k


def test_it_trains(backend):
    """10 SGD steps on all four parameter vectors towards the fixture's float64 output (float64 build): the loss falls, and
    the parameters equal those of the same loop driven by torch.autograd over the restatement (100 * F64_TOL)"""
    g = load(FIXTURES[0])
    n, dev = int(g["n_iter"]), backend.device
    start = {k: g[k] * f for k, f in zip(NAMES, (0.8, 1.25, 0.9, 1.3))}
    rec = solver(g, "float64", backend, sched=start)
    mine = params_of(rec)
    theirs = [p.detach().cpu().clone().requires_grad_() for p in mine]
    assert all(p.dtype == torch.float32 for p in mine)
    target, data, psf = torch.from_numpy(g["out64"]), torch.from_numpy(g["data"]).double(), torch.from_numpy(g["psf"])
    norm = float((target ** 2).mean())

    def loop(params, model):
        opt = torch.optim.SGD([{"params": [p], "lr": 0.02 * float(np.abs(g[k]).max()) ** 2} for k, p in zip(NAMES, params)])
        losses = []
        for _ in range(10):
            opt.zero_grad()
            loss = ((model() - target.to(params[0].device)) ** 2).mean() / norm
            loss.backward()
            losses.append(float(loss.detach()))
            opt.step()
        return losses

    losses = loop(mine, lambda: rec(data.to(dev)))
    ref_losses = loop(theirs, lambda: restated_admm(psf, data, *theirs, n)[0])
    print("losses", losses, "restated", ref_losses)
    assert losses[-1] < losses[0] and ref_losses[-1] < ref_losses[0]
    for k, p, q, s in zip(NAMES, mine, theirs, start.values()):
        r = rel(p, q.detach().numpy())
        print(f"after 10 steps: {k} rel {r:.3e} (bound {100 * F64_TOL:.0e}), moved by {rel(p, s):.2e}")
        assert r <= 100 * F64_TOL and rel(p, s) > 1e-4, k


def test_refusals(backend):
    rng = np.random.default_rng(0)
    dev = backend.device

    def solver_of(h, w, d=1, c=3, **kw):
        psf = rng.random((d, h, w, c)).astype(np.float32)
        rec = lpa.UnrolledADMM(torch.from_numpy(psf).to(dev), n_iter=3, **kw)
        return rec, torch.from_numpy(rng.random((2, 1, h, w, c)).astype(np.float32)).to(dev)

    def forward_only_works(rec, data):
        with torch.no_grad():
            out = rec(data)
        assert not out.requires_grad and float(out.abs().max()) > 0
        return out

    def raw(rec, data):       # lpc_admm_backward on whatever the handle holds
        buf = torch.zeros(data.numel(), dtype=torch.float32, device=dev)
        rec._handle.admm_backward(buf.data_ptr(), None, *(buf[4 * k:].data_ptr() for k in range(4)), 0)

    def record_by_hand(rec, data, n):      # the recorded forward without the refusals of forward()
        rec._data = data
        rec._upload_data()
        rec._record(True)
        rec.reset()
        rec._iterate(n)

    # -- the Python surface: NotImplementedError before anything runs, then the solver still does inference
    rec, data = solver_of(8, 12)                               # padded 15 x 24
    assert rec._padded_shape[1] == 15
    out = rec(data)              # (from backward(): the forward under autograd is inference code's as well)
    with pytest.raises(NotImplementedError, match="odd"):
        out.sum().backward()
    assert torch.equal(forward_only_works(rec, data), out.detach())
    record_by_hand(rec, data, 3)
    with pytest.raises(_native.NativeError, match="odd"):     # the C entry point refuses it itself
        raw(rec, data)
    rec, data = solver_of(10, 12, d=2)
    out = rec(data)
    with pytest.raises(NotImplementedError, match="depth"):
        out.sum().backward()
    assert torch.equal(forward_only_works(rec, data), out.detach())
    record_by_hand(rec, data, 3)
    with pytest.raises(_native.NativeError, match="depth"):
        raw(rec, data)
    rec, data = solver_of(10, 12)
    with pytest.raises(NotImplementedError, match="PSF"):
        rec(data, psfs=rec._psf.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="per-frame"):
        rec(data, psfs=torch.stack([rec._psf, rec._psf]))
    forward_only_works(rec, data)
    rec._psf = rec._psf.clone().requires_grad_()
    with pytest.raises(NotImplementedError, match="PSF"):
        rec(data)
    forward_only_works(rec, data)
    est = torch.from_numpy(rng.random((1, 1, 20, 24, 3)).astype(np.float32) * 0.1).to(dev)
    rec, data = solver_of(10, 12, initial_est=est.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="initial estimate"):
        rec(data)
    forward_only_works(rec, data)
    rec, data = solver_of(10, 12, initial_est=est)
    out = rec(data)
    with pytest.raises(NotImplementedError, match="initial estimate"):
        out.sum().backward()
    with pytest.raises(_native.NativeError, match="initial estimate"):
        raw(rec, data)
    assert torch.equal(forward_only_works(rec, data), out.detach())
    rec, data = solver_of(10, 12)
    first = rec(data)
    rec(data)
    with pytest.raises(RuntimeError, match="tape overwritten"):
        first.sum().backward()
    forward_only_works(rec, data)
    # a custom psi / a denoiser: the engine has never run them together with an unrolled schedule (lpc_admm_psi_step and
    # lpc_admm_pnp_begin refuse); with gradients asked for the refusal is a NotImplementedError
    ident = dict(psi=lambda x: torch.stack((x, x), dim=x.dim()), psi_adj=lambda u: u[..., 0] + u[..., 1],
                 psi_gram=lambda shape: 2 * torch.ones(shape[0], shape[1], shape[2] // 2 + 1, shape[3]))
    for kw in (ident, dict(denoiser={"network": lambda x, s: x, "noise_level": 0.1})):
        rec, data = solver_of(10, 12, **kw)
        with pytest.raises(NotImplementedError, match="custom psi and a denoiser"):
            rec(data)
        with torch.no_grad(), pytest.raises(_native.NativeError, match="unrolled schedule"):
            rec(data)
    # -- the C entry point
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    ptrs = (buf.data_ptr(), None) + (buf.data_ptr(),) * 4 + (0,)
    fis = lpa.FISTA(torch.from_numpy(rng.random((1, 10, 12, 3)).astype(np.float32)).to(dev))
    with pytest.raises(_native.NativeError, match="not an ADMM handle"):
        fis._handle.admm_backward(*ptrs)
    with pytest.raises(_native.NativeError, match="not an ADMM handle"):
        fis._handle.admm_record(1)
    plain = lpa.ADMM(torch.from_numpy(rng.random((1, 10, 12, 3)).astype(np.float32)).to(dev))
    with pytest.raises(_native.NativeError, match="no schedule"):
        plain._handle.admm_backward(*ptrs)
    rec, data = solver_of(10, 12)
    forward_only_works(rec, data)
    with pytest.raises(_native.NativeError, match="nothing recorded"):
        raw(rec, data)
    record_by_hand(rec, data, 2)                               # one iteration short of the schedule
    with pytest.raises(_native.NativeError, match="2 iterations since the reset, the schedule has 3"):
        raw(rec, data)
    record_by_hand(rec, data, 4)                               # one too many
    with pytest.raises(_native.NativeError, match="4 iterations since the reset, the schedule has 3"):
        raw(rec, data)
    record_by_hand(rec, data, 3)
    raw(rec, data)
    # a caller's gram in R_divmat: the prior is no longer the one the sweep differentiates
    gram = torch.ones(20, 13, dtype=torch.float32, device=dev)
    rec._handle.set_psi_gram(gram.data_ptr(), 0)
    record_by_hand(rec, data, 3)
    with pytest.raises(_native.NativeError, match="psi"):
        raw(rec, data)
    rec._set_psf(rec._psf)                                      # (restores the finite-difference gram)
    record_by_hand(rec, data, 3)
    raw(rec, data)
    # a new schedule, new data or a new PSF after the recorded iterations invalidates the tape
    h = rec._handle
    for invalidate in (lambda: h.set_admm_schedule(*([[1e-4] * 3] * 4)),
                       lambda: h.set_data(rec._data_dev.data_ptr(), 3, 0),
                       lambda: h.set_psf(rec._psf_dev.data_ptr(), 0)):
        invalidate()
        with pytest.raises(_native.NativeError, match="nothing recorded|0 iterations since the reset"):
            raw(rec, data)
        record_by_hand(rec, data, 3)
        raw(rec, data)
    forward_only_works(rec, data)
    # plug-and-play iterations since the reset (a plain ADMM handle that gets a schedule afterwards)
    pnp = lpa.ADMM(torch.from_numpy(rng.random((1, 10, 12, 3)).astype(np.float32)).to(dev),
                   denoiser={"network": lambda x, s: x, "noise_level": 0.1})
    pnp.set_data(data[:1])
    pnp.apply(n_iter=1, disp_iter=None)
    pnp._handle.set_admm_schedule(*([[1e-4]] * 4))
    pnp._handle.admm_record(1)
    with pytest.raises(_native.NativeError, match="plug-and-play"):
        pnp._handle.admm_backward(*ptrs)
    # a forward whose backward is refused anyway keeps no tape
    rec, data = solver_of(8, 12)
    with torch.no_grad():
        rec(data)
    base = rec._handle.workspace_bytes()
    rec(data)
    assert rec._handle.workspace_bytes() == base


def test_module_surface(backend):
    g = load(FIXTURES[1])
    psf, n = torch.from_numpy(g["psf"]).to(backend.device), int(g["n_iter"])
    rec = lpa.UnrolledADMM(psf, n_iter=n, **BASE)
    assert isinstance(rec, torch.nn.Module)
    assert [tuple(p.shape) for p in rec.parameters()] == [(n,)] * 4
    assert all(p.dtype == torch.float32 and p.device == psf.device for p in rec.parameters())
    assert list(rec.state_dict().keys()) == ["_mu1_p", "_mu2_p", "_mu3_p", "_tau_p"]
    for k, p in zip(NAMES, rec.parameters()):
        assert torch.equal(p.detach().cpu(), torch.ones(n) * BASE[k])
    skipped = lpa.UnrolledADMM(psf, n_iter=n, skip_unrolled=True, **BASE)
    assert list(skipped.parameters()) == [] and not isinstance(skipped._mu1_p, torch.nn.Parameter)
    # set_parameters and load_state_dict copy in place
    before = params_of(rec)
    rec.set_parameters(**sched_of(g))
    state = {k: v.clone() * 2 for k, v in rec.state_dict().items()}
    rec.load_state_dict(state)
    assert all(a is b for a, b in zip(before, params_of(rec)))
    assert all(torch.equal(p.detach(), state[f"_{k}_p"]) for k, p in zip(NAMES, params_of(rec)))
    rec.set_parameters(**sched_of(g))
    data = torch.from_numpy(g["data"]).to(backend.device)
    with torch.no_grad():
        rec(data)
    base = rec._handle.workspace_bytes()
    rec(data)
    B, _, H, W, C = data.shape
    Hp, Wp = rec._padded_shape[1:3]
    rpitch = (Wp + 3) // 4 * 4
    tape = (6 * n + 11) * B * C * Hp * rpitch * 4 + n * B * C * -(-Hp // 8) * -(-Wp // 128) * 4 * 8    # include/lpc.h: lpc_admm_record
    assert rec._handle.workspace_bytes() == base + tape
    with torch.no_grad():          # evaluation between training steps pauses the recording, the tape stays
        rec(data)
    assert rec._handle.workspace_bytes() == base + tape
    rec.release_tape()
    assert rec._handle.workspace_bytes() == base
    out = rec(data)
    assert rec._handle.workspace_bytes() == base + tape
    # code that only wants the image still gets it: the result converts to NumPy although it carries a graph
    assert out.requires_grad and np.array_equal(out[0].cpu().numpy(), np.asarray(out.detach().cpu())[0])
    out.sum().backward()
    assert all(p.grad is not None for p in rec.parameters())
