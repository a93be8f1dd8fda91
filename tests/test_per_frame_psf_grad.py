"""
Training with one PSF per measurement: ``UnrolledADMM(psf, ..., psf_grad=True, per_frame_grad=True)`` and
``UnrolledFISTA(psf, ..., per_frame_grad=True)`` with ``rec(batch, psfs=P5)``, ``P5.shape == (B, 1, H, W, C)`` a leaf, and
``.backward()`` (lpc_per_frame_grad; the reverse sweeps on a handle that holds B C PSF spectra, k_admm_bwd_psf_acc_frames),
through the public API, on the SIMT emulator ('emu') and on the MI355X ('hip', -m gpu).

What per-frame PSFs cross in the reverse mode: the replay's convolutions, every spectral step of the two sweeps (the
precombined middle constants under a per-iteration schedule included), the FISTA cross terms with their explicit
multipliers, ADMM's accumulate kernel -- state plane q against PSF plane q, where it was q % C -- and the layout of the
result, (B, 1, H, W, C) with nothing summed over the batch.

1. The reference itself: tests/golden/unrolled_{admm,fista}_psfs5d_grad_*.npz (gen_per_frame_psf_grad.py: the reference's
   own ``forward(batch, psfs=P5)`` + ``backward()`` in float64 and float32; kink-free, U and W live, asserted there).
2. Every launch plan: the kink-free gradient fixtures (ADMM) / the sweep's signed case 12x30 (FISTA) with a second PSF
   for frame 1 (seeds chosen on the CPU so that frame 1 stays kink-free: asserted in ``frames_ref``), against the float64 /
   float32 restatement run frame by frame with that frame's PSF a leaf, parameter gradients summed.
3. Structure: a frame of the batch against a one-frame solver with ``psfs=P5[b]``; ``stack([p] * B)`` against the
   shared-PSF training run; exchanged PSFs move the gradient.
4. Nothing else moves: a solver with the switch on trains with one PSF exactly as a default one; per-frame -> shared ->
   per-frame reproduces the first step; a ``no_grad`` forward keeps the tape; the raw entries are deterministic.
5. Workspace formulas of include/lpc.h.  6. Refusals with the switch on, and the native ones with it off.
7. Ten SGD steps on a per-mask residual ``psfs = P5 + delta`` end on the restatement's ``delta``.

Bounds (those of tests/test_unrolled_admm_psf_grad.py and tests/test_unrolled_psf_grad.py; max-norm over whole arrays,
relative to the max of the float64 array):
  float32 engine:  rel(x, ref64) <= 4 * max(rel(ref32, ref64), 2e-6) per array, ref32 the reference's own float32 run
                   (item 2: the float32 restatement);
  float64 engine:  <= 100 * F64_TOL = 1e-9; g_tk <= 5e-7 (``_tk_p`` and its gradient are kept in float32).
As in those files, the float64 ENGINE is compared with the float64 restatement (frame by frame, summed) for ``out``,
``g_data`` and the parameter gradients of ADMM -- the reference keeps its parameters in float32, divides tau / mu2 in
float32 and rounds their gradients to float32, which puts its float64 run 1e-9 .. 2e-7 from any float64 computation
(tests/test_unrolled_admm_grad.py: ``dist_out``) -- with the parameter gradients read from the raw entry, in float64;
``g_psfs`` is compared with the reference itself in both precisions, and so is everything of FISTA.

Largest distances measured on the MI355X (the 55 cases of this file on the 'hip' backend; g_psfs | the other arrays):
  ADMM  fixtures   float32  6.0e-7 (bound 8.0e-6) | 4.3e-6 (g_mu2, bound 3.9e-5)    float64  1.2e-10 (1e-9) | 1.3e-14
        every plan float32  1.1e-6 (bound 8.0e-6) | 3.6e-6 (g_mu1, bound 5.0e-5)    float64  2.1e-15        | 1.4e-14
  FISTA fixtures   float32  1.3e-7 (bound 8.0e-6) | 2.2e-6 (g_alpha, bound 8.0e-6)  float64  7.1e-16        | 5.5e-15
        every plan float32  1.8e-7 (bound 8.0e-6) | 9.1e-7 (g_tk, bound 8.0e-6)     float64  4.3e-16        | 9.6e-8 (g_tk, 5e-7)
A frame of the batch against the one-frame solver: the same plan and the same bits in every case, both solvers, both
precisions.  ``stack([p] * B)`` against the shared-PSF run: everything bitwise except ADMM's ``g_psfs.sum(0)`` (2.2e-7 in
float32, 3.3e-16 in float64: torch adds the frames in another order than the shared accumulate's loop).  Ten SGD steps on
the residual end 1.3e-14 (ADMM) and 3.1e-15 (FISTA) from the restatement's.
"""
import functools
import os

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from test_unrolled_grad_sweep import conditions as fista_conditions
from test_unrolled_grad_sweep import inputs as fista_inputs
from unrolled_admm_restated import F64_PLANS, NAMES, PLANS, activity, restated_admm
from unrolled_restated import F64_TOL
from unrolled_restated import PLANS as FISTA_PLANS
from unrolled_restated import rec_padded, rel, restated

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
KINDS = ["admm", "fista"]
CASES = ["19x27x1_b3", "16x20x3_b2"]
RGB = "16x20x3_b2"
ABASE = dict(mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-7)
PARAMS = {"admm": NAMES, "fista": ("alpha", "tk")}
# item 2: seed of the PSF of frame 1 per source fixture (frame 0 keeps the fixture's own PSF), found on the CPU
SECOND_PSF = {"unrolled_admm_grad_19x27x1_b2": 7002, "unrolled_admm_grad_24x32x1_b2": 7003,
              "unrolled_admm_grad_48x20x1_b2": 7021, "unrolled_admm_grad_24x40x1_b2": 7002, "fista_12x30": 7000}
ROW_PLANS = ["rows_half", "rows_paired"]      # tests/test_unrolled_psf_grad.py (both are in FISTA_PLANS as well)


def tdt_of(dtype):
    return torch.float64 if dtype == "float64" else torch.float32


def keys_of(kind):
    return ("out", "g_data", "g_psfs") + tuple("g_" + k for k in PARAMS[kind])


def bound_of(dtype, ref32, ref64, key):
    if dtype == "float64":
        return 5e-7 if key == "g_tk" else 100 * F64_TOL
    return 4 * max(rel(ref32, ref64), 2e-6)


def random_psf(seed, shape):
    p = np.random.default_rng(seed).random(shape).astype(np.float32) ** 6
    return p / np.linalg.norm(p.ravel())


def default_init(psf):
    """the constructor's start value of FISTA, gd.py:100-105: (1, D, H, W, C), a constant"""
    flat = psf.reshape(-1, psf.shape[-1])
    return torch.ones_like(psf[None]) * ((flat.max(0).values + flat.min(0).values) / 2)


@functools.lru_cache(maxsize=None)
def load(kind, case):
    """a fixture of gen_per_frame_psf_grad.py as (inputs dict, fixture)"""
    g = np.load(os.path.join(GOLDEN, f"unrolled_{kind}_psfs5d_grad_{case}.npz"))
    inp = dict(psf=g["psf"], psfs=g["psfs"], data=g["data"], w=g["w"], n=int(g["n_iter"]),
               sched={k: g[k] for k in PARAMS[kind]})
    assert g["psfs"].shape == (g["data"].shape[0],) + g["psf"].shape and g["g_psfs64"].shape == g["psfs"].shape
    assert all(not np.array_equal(g["psf"], p) for p in g["psfs"])
    return inp, g


@functools.lru_cache(maxsize=None)
def sweep_inputs(kind, source):
    """item 2: an existing kink-free case with a second PSF for frame 1"""
    if kind == "admm":
        g = np.load(os.path.join(GOLDEN, source + ".npz"))
        psf, data, w, n, sched = g["psf"], g["data"], g["w"], int(g["n_iter"]), {k: g[k] for k in NAMES}
    else:
        f = fista_inputs("12x30")
        psf, data, w, n, sched = f.psf, f.data, f.w, f.n, dict(alpha=f.alpha, tk=f.tk)
    assert data.shape[0] == 2
    psfs = np.stack([psf, random_psf(SECOND_PSF[source], psf.shape)])
    return dict(psf=psf, psfs=psfs, data=data, w=w, n=n, sched=sched)


def restated_frame(kind, inp, b, tdt, psf_b=None, param_leaves=None):
    """the restatement of frame ``b`` alone with its PSF a leaf: (results as tensors with a graph cut, projection / kink
    arguments); ``param_leaves``: shared leaves (the training loop), else fresh float64 ones holding the float32 values"""
    sched, n = inp["sched"], inp["n"]
    p = torch.from_numpy(inp["psfs"][b]).to(tdt).requires_grad_() if psf_b is None else psf_b
    batch = torch.from_numpy(inp["data"][b:b + 1]).to(tdt).requires_grad_()
    if kind == "admm":
        ps = param_leaves or [torch.from_numpy(sched[k]).double().requires_grad_() for k in NAMES]
        out, args = restated_admm(p, batch, *ps, n, dtype=tdt)
    else:
        ps = param_leaves or [torch.from_numpy(sched["alpha"]).to(tdt).requires_grad_(),
                              torch.from_numpy(sched["tk"]).requires_grad_()]
        out, args = restated(p, batch, *ps, n, init=default_init(torch.from_numpy(inp["psf"]).to(tdt)), dtype=tdt)
    return out, args, p, batch, ps


def frames_ref_of(kind, inp, tag):
    """float64 / float32 restatement run frame by frame: out, g_data, g_psfs stacked, the parameter gradients summed.
    Asserts on the float64 run that no element of any frame sits on a kink."""
    refs = {}
    for tdt in (torch.float64, torch.float32):
        outs, gds, gps, total = [], [], [], None
        for b in range(inp["data"].shape[0]):
            out, args, p, batch, ps = restated_frame(kind, inp, b, tdt)
            (out * torch.from_numpy(inp["w"][b:b + 1]).to(tdt)).sum().backward()
            if tdt == torch.float64 and kind == "admm":
                act = activity(args)
                assert sum(a[2] for a in act) == 0, f"{tag} frame {b}: on a kink {act}: pick another seed"
            elif tdt == torch.float64:
                fista_conditions(args, f"{tag} frame {b}", active=False)
            outs.append(out.detach()[0]), gds.append(batch.grad[0]), gps.append(p.grad)
            grads = [q.grad.double() for q in ps]
            total = grads if total is None else [a + c for a, c in zip(total, grads)]
        r = {"out": torch.stack(outs).numpy(), "g_data": torch.stack(gds).numpy(), "g_psfs": torch.stack(gps).numpy()}
        r.update({"g_" + k: v.numpy() for k, v in zip(PARAMS[kind], total)})
        refs[tdt] = r
    return refs


@functools.lru_cache(maxsize=None)
def fixture_frames_ref(kind, case):
    return frames_ref_of(kind, load(kind, case)[0], f"{kind} {case}")


@functools.lru_cache(maxsize=None)
def sweep_frames_ref(kind, source):
    return frames_ref_of(kind, sweep_inputs(kind, source), f"{kind} {source}")


def solver(kind, inp, dtype, backend, per_frame_grad=True, **kw):
    psf = torch.from_numpy(inp["psf"]).to(backend.device)
    flags = {"per_frame_grad": True} if per_frame_grad else {}
    if kind == "admm":
        rec = lpa.UnrolledADMM(psf, dtype=dtype, n_iter=inp["n"], **ABASE, **{"psf_grad": True, **flags, **kw})
        rec.set_parameters(**inp["sched"])
    else:
        rec = lpa.UnrolledFISTA(psf, n_iter=inp["n"], dtype=dtype, **flags, **kw)
        rec.set_parameters(**inp["sched"])
    return rec


def params_of(rec, kind):
    return [getattr(rec, f"_{k}_p") for k in PARAMS[kind]]


def step(rec, kind, inp, dtype, backend, psfs, frames=slice(None), how="forward"):
    """one training step of ``(out * w).sum()``: ``psfs`` (a numpy array or a tensor; 5-D or 4-D) as a fresh leaf"""
    tdt, dev = tdt_of(dtype), backend.device
    rec.zero_grad()
    p = torch.as_tensor(psfs).detach().clone().to(device=dev, dtype=tdt).requires_grad_()
    batch = torch.from_numpy(inp["data"][frames]).to(device=dev, dtype=tdt).requires_grad_()
    if how == "forward":
        out = rec(batch, psfs=p)
    else:
        rec._set_psf(p)
        out = rec(batch)
    (out * torch.from_numpy(inp["w"][frames]).to(device=dev, dtype=tdt)).sum().backward()
    assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device == p.device
    assert batch.grad.shape == batch.shape
    got = {"out": out.detach().clone(), "g_data": batch.grad, "g_psfs": p.grad}
    got.update({"g_" + k: q.grad.clone() for k, q in zip(PARAMS[kind], params_of(rec, kind))})
    if kind == "admm" and dtype == "float64":
        # ``_mu1_p`` .. ``_tau_p`` are float32 tensors whatever the dtype, and so are their gradients: take the parameter
        # gradients as the raw entry writes them, in float64 (tests/test_unrolled_admm_psf_grad.py: check_case)
        raw = raw_backward(rec, kind, torch.from_numpy(inp["w"][frames]).double(), tuple(p.shape[:-4]))
        assert torch.equal(raw[-1], p.grad) and torch.equal(raw[0].reshape(batch.shape), batch.grad)
        for i, (k, q) in enumerate(zip(NAMES, params_of(rec, kind))):
            assert torch.equal(q.grad.cpu(), (raw[1 + i].cpu() * torch.sign(q.detach().cpu()).double()).float()), k
            got["g_" + k] = raw[1 + i]
    return got


def raw_backward(rec, kind, grad_out, psf_frames):
    """the native _psf entry itself on the tape of the last forward: [g_data, parameter gradients ..., g_psf], in the
    engine's precision; ``psf_frames``: leading axis of g_psf (the batch on a per-frame handle, else ())"""
    go = rec._to_dev(grad_out)
    gd = rec._empty((go.shape[0],) + tuple(go.shape[2:]))
    gpsf = rec._empty(tuple(psf_frames) + tuple(int(v) for v in rec._psf_shape))
    if kind == "admm":
        gp = rec._empty((4, rec._n_iter))
        rec._handle.admm_backward_psf(go.data_ptr(), gd.data_ptr(), *(gp[k].data_ptr() for k in range(4)), gpsf.data_ptr(),
                                      rec._stream())
        return [gd] + [gp[k].clone() for k in range(4)] + [gpsf]
    ga, gc = rec._empty((rec._n_iter, int(rec._psf_shape[3]))), rec._empty((rec._n_iter,))
    rec._handle.fista_backward_psf(go.data_ptr(), gd.data_ptr(), ga.data_ptr(), gc.data_ptr(), None, gpsf.data_ptr(),
                                   rec._stream())
    return [gd, ga, gc, gpsf]


def check(kind, inp, dtype, backend, ref64, ref32, tag, restated64=None):
    """one per-frame training step against (ref64, ref32) with the bounds of the module docstring.  ``restated64``
    (float64 ADMM against the reference): what out, g_data and the parameter gradients are compared with instead (``step``
    reads the parameter gradients from the raw entry, in float64)."""
    rec = solver(kind, inp, dtype, backend)
    got = step(rec, kind, inp, dtype, backend, inp["psfs"])
    B = inp["data"].shape[0]
    assert got["g_psfs"].shape == (B,) + inp["psf"].shape
    raw = raw_backward(rec, kind, torch.from_numpy(inp["w"]).to(tdt_of(dtype)), (B,))
    again = raw_backward(rec, kind, torch.from_numpy(inp["w"]).to(tdt_of(dtype)), (B,))
    for a, b in zip(raw, again):      # (item 4: a second call of the raw entry gives the same bits)
        assert float(a.abs().max()) > 0 and torch.equal(a, b)
    assert torch.equal(raw[-1], got["g_psfs"]) and torch.equal(raw[0].reshape(got["g_data"].shape), got["g_data"])
    bad = []
    for k in keys_of(kind):
        want64 = ref64[k] if restated64 is None or k == "g_psfs" else restated64[k]
        assert tuple(got[k].shape) == tuple(want64.shape), (k, got[k].shape, want64.shape)
        r, bound = rel(got[k], want64), bound_of(dtype, ref32[k], ref64[k], k)
        print(f"{tag} {dtype} {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))
    assert not bad, bad
    return rec


# ------------------------------------------------------------------------------------------------- CPU only --
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_frame_by_frame_is_pinned(kind, case):
    """the yardstick of items 2, 3 and 7 -- the restatement run frame by frame, parameter gradients summed -- against the
    reference's own per-frame run: g_psfs and (FISTA) everything within 100 * F64_TOL in float64; ADMM's out, g_data and
    parameter gradients within the distances tests/test_unrolled_admm_grad.py allows its restatement (1e-7 for out; the
    reference rounds its parameter gradients to float32)"""
    inp, g = load(kind, case)
    refs = fixture_frames_ref(kind, case)
    for k in keys_of(kind):
        r = rel(refs[torch.float64][k], g[k + "64"])
        loose = kind == "admm" and k != "g_psfs"
        bound = (1e-7 if k in ("out", "g_data") else 1e-6) if loose else bound_of("float64", None, None, k)
        print(f"{kind} {case} restated frame by frame, float64, {k}: rel {r:.3e} (bound {bound:.1e})")
        assert r <= bound, (k, r, bound)
        r, bound = rel(refs[torch.float32][k], g[k + "64"]), bound_of("float32", g[k + "32"], g[k + "64"], k)
        assert r <= bound, (k, r, bound)


# ----------------------------------------------------------------------------------------- emulator and card --
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_reference(backend, kind, case, dtype):
    """item 1.  On the parent: NotImplementedError ... per-frame"""
    inp, g = load(kind, case)
    ref64, ref32 = ({k: g[k + s] for k in keys_of(kind)} for s in ("64", "32"))
    restated64 = fixture_frames_ref(kind, case)[torch.float64] if kind == "admm" and dtype == "float64" else None
    check(kind, inp, dtype, backend, ref64, ref32, f"{kind} {case}", restated64)


@pytest.mark.parametrize("plan,dtype", [(p, "float32") for p in sorted(PLANS)] + [(p, "float64") for p in F64_PLANS])
def test_admm_every_launch_plan(backend, monkeypatch, plan, dtype):
    """item 2, ADMM: the accumulate and every H of the sweep work in the spectra's own layout, whatever the plan"""
    case = PLANS[plan]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **case["opts"]})
    refs = sweep_frames_ref("admm", case["fixture"])
    rec = check("admm", sweep_inputs("admm", case["fixture"]), dtype, backend, refs[torch.float64], refs[torch.float32],
                f"admm {plan}")
    info = rec._handle.plan_info()
    for marker in case["info"] + case.get("f32" if dtype == "float32" else "f64", []):
        assert marker in info, (marker, info)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("plan", sorted(set(FISTA_PLANS) | set(ROW_PLANS)))
def test_fista_every_launch_plan(backend, monkeypatch, plan, dtype):
    """item 2, FISTA"""
    opts, marker = FISTA_PLANS[plan]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **opts})
    refs = sweep_frames_ref("fista", "fista_12x30")
    rec = check("fista", sweep_inputs("fista", "fista_12x30"), dtype, backend, refs[torch.float64], refs[torch.float32],
                f"fista {plan}")
    assert marker in rec._handle.plan_info(), rec._handle.plan_info()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_frame_of_the_batch_is_the_single_frame_run(backend, kind, case, dtype):
    """item 3a: frame b of the per-frame batch against a one-frame solver with ``psfs=P5[b]`` (a 4-D leaf: the one-PSF
    kernels).  out, g_data[b], g_psfs[b]: bit for bit where ``plan_info()`` of the two handles agrees, else within the
    bound; the parameter gradients of the batch are the sum over the frames within the bound."""
    inp, g = load(kind, case)
    rec = solver(kind, inp, dtype, backend)
    got = step(rec, kind, inp, dtype, backend, inp["psfs"])
    B = inp["data"].shape[0]
    total = {k: 0.0 for k in keys_of(kind)[3:]}
    one = solver(kind, inp, dtype, backend)
    for b in range(B):
        single = step(one, kind, inp, dtype, backend, inp["psfs"][b], frames=slice(b, b + 1))
        same_plan = one._handle.plan_info() == rec._handle.plan_info()
        for k in ("out", "g_data", "g_psfs"):
            a, want = got[k][b], single[k].reshape(got[k][b].shape)
            bitwise = torch.equal(a, want)
            r, bound = rel(a, want), bound_of(dtype, g[k + "32"][b], g[k + "64"][b], k)
            print(f"{kind} {case} {dtype} frame {b} {k}: same plan {same_plan}, bitwise {bitwise}, rel {r:.3e} (bound {bound:.1e})")
            assert bitwise if same_plan else r <= bound, (b, k, r, bound)
        for k in total:
            total[k] = total[k] + single[k].double()
    for k, v in total.items():
        r, bound = rel(got[k], v), bound_of(dtype, g[k + "32"], g[k + "64"], k)
        print(f"{kind} {case} {dtype} {k}: batch against the sum of the frames: rel {r:.3e} (bound {bound:.1e})")
        assert r <= bound, (k, r, bound)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind", KINDS)
def test_equal_psfs_are_the_shared_psf_run(backend, kind, dtype):
    """item 3b: ``P5 = stack([p] * B)`` -- out has the bits of the shared-PSF training run (``psfs=p``, 4-D),
    ``g_psfs.sum(0)`` is its ``g_psf`` within the bound, g_data and the parameter gradients are within the bound (measured,
    emulator and MI355X: g_data and the parameter gradients bitwise as well, both solvers and precisions -- the frames'
    arithmetic is the same and the parameters' partial sums are added in the same order; FISTA's g_psfs.sum(0) too, ADMM's
    to rounding).  Teeth, item 3c: exchanging the PSFs of frames 0 and 1 of the
    fixture moves g_psfs by more than 1e-2."""
    inp, g = load(kind, RGB)
    B = inp["data"].shape[0]
    p = inp["psfs"][0]
    rec = solver(kind, inp, dtype, backend)
    shared = step(rec, kind, inp, dtype, backend, p)
    same = step(rec, kind, inp, dtype, backend, np.stack([p] * B))
    assert same["g_psfs"].shape == (B,) + p.shape and shared["g_psfs"].shape == p.shape
    assert float(same["out"].abs().max()) > 0 and torch.equal(same["out"], shared["out"])
    for k in keys_of(kind)[1:]:
        a = same[k].sum(0) if k == "g_psfs" else same[k]
        r, bound = rel(a, shared[k]), bound_of(dtype, g[k + "32"], g[k + "64"], k)
        print(f"{kind} {dtype} {k}: equal PSFs against the shared run: bitwise {torch.equal(a, shared[k])}, rel {r:.3e} "
              f"(bound {bound:.1e})")
        assert r <= bound, (k, r, bound)
    plain = step(rec, kind, inp, dtype, backend, inp["psfs"])
    swapped = inp["psfs"].copy()
    swapped[[0, 1]] = inp["psfs"][[1, 0]]
    moved = rel(step(rec, kind, inp, dtype, backend, swapped)["g_psfs"], plain["g_psfs"])
    print(f"{kind} {dtype}: exchanging the PSFs of frames 0 and 1 moves g_psfs by {moved:.2e}")
    assert moved > 1e-2


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind", KINDS)
def test_nothing_else_moves(backend, kind, dtype):
    """item 4: one PSF for the batch on a solver with the switch on -- ``psfs=p`` and ``_set_psf(p)`` -- has the bits of a
    default solver in every output; per-frame -> shared -> per-frame on ONE solver reproduces the first step bit for bit;
    a ``no_grad`` forward between two steps keeps the tape (``workspace_bytes()``)"""
    inp, g = load(kind, RGB)
    p = inp["psfs"][1]
    on, off = solver(kind, inp, dtype, backend), solver(kind, inp, dtype, backend, per_frame_grad=False)
    assert on.per_frame_grad and not off.per_frame_grad
    for how in ("forward", "set_psf"):
        a, b = step(on, kind, inp, dtype, backend, p, how=how), step(off, kind, inp, dtype, backend, p, how=how)
        for k in keys_of(kind):
            assert float(a[k].abs().max()) > 0 and torch.equal(a[k], b[k]), (how, k)
    first = step(on, kind, inp, dtype, backend, inp["psfs"])
    ws = on._handle.workspace_bytes()
    with torch.no_grad():
        frozen = on(torch.from_numpy(inp["data"]).to(device=backend.device, dtype=tdt_of(dtype)))
    assert on._handle.workspace_bytes() == ws and torch.equal(frozen, first["out"])      # (the PSFs stay current)
    shared = step(on, kind, inp, dtype, backend, p)
    for k in keys_of(kind):
        assert torch.equal(shared[k], a[k]), k
    third = step(on, kind, inp, dtype, backend, inp["psfs"])
    assert on._handle.workspace_bytes() == ws
    for k in keys_of(kind):
        assert torch.equal(first[k], third[k]), k
    # PSFs that are current from an earlier forward: a later recording forward without ``psfs`` trains with them
    on.zero_grad()
    tdt, dev = tdt_of(dtype), backend.device
    batch = torch.from_numpy(inp["data"]).to(device=dev, dtype=tdt).requires_grad_()
    out = on(batch)
    (out * torch.from_numpy(inp["w"]).to(device=dev, dtype=tdt)).sum().backward()
    assert torch.equal(out.detach(), first["out"]) and torch.equal(batch.grad, first["g_data"])
    # ... and a tape overwritten by a later forward is still refused
    stale = on(batch)
    on(batch)
    with pytest.raises(RuntimeError, match="tape overwritten"):
        stale.sum().backward()


def spectrum_plane_bytes(Hp, Wp, itemsize):
    return Hp * ((Wp // 2 + 1 + 15) // 16 * 16) * 2 * itemsize


@pytest.mark.parametrize("kind", KINDS)
def test_workspace(backend, kind):
    """item 5: base + tape + the documented formula (include/lpc.h: lpc_per_frame_grad, lpc_fista_backward_psf) from the
    first backward with a per-frame PSF gradient on; ``release_tape()`` gives all of it back"""
    inp, g = load(kind, RGB)
    dev = backend.device
    rec = solver(kind, inp, "float32", backend)
    data = torch.from_numpy(inp["data"]).to(dev)
    with torch.no_grad():
        rec(data)
    base = rec._handle.workspace_bytes()
    B, _, H, W, C = data.shape
    n, P = inp["n"], B * C
    Hp, Wp = rec._padded_shape[1:3]
    assert (Hp, Wp) == (rec_padded(H), rec_padded(W)) and Hp % 2 == 0
    with torch.no_grad():      # per-frame PSFs grow the handle's PSF buffers once (lpc_set_psf_batch): part of the base
        rec(data, psfs=torch.from_numpy(inp["psfs"]).to(dev))
    grown = rec._handle.workspace_bytes()
    assert grown > base
    if kind == "admm":
        rpitch = (Wp + 3) // 4 * 4
        tape = (6 * n + 11) * P * Hp * rpitch * 4 + n * P * -(-Hp // 8) * -(-Wp // 128) * 4 * 8      # lpc_admm_record
        extra = (4 * P + P) * spectrum_plane_bytes(Hp, Wp, 4)
        shared_extra = (4 * P + C) * spectrum_plane_bytes(Hp, Wp, 4)
    else:
        tape = (2 * n + 4) * P * H * W * 4 + n * P * H * 2 * 8                                      # lpc_fista_record
        extra = shared_extra = 3 * P * spectrum_plane_bytes(Hp, Wp, 4) + P * H * W * 4
    step(rec, kind, inp, "float32", backend, inp["psfs"])
    assert rec._handle.workspace_bytes() == grown + tape + extra
    rec.release_tape()
    assert rec._handle.workspace_bytes() == grown
    # one PSF first: the one-PSF formula, unchanged; a per-frame step afterwards makes room for the P-plane accumulator
    step(rec, kind, inp, "float32", backend, inp["psfs"][0])
    assert rec._handle.workspace_bytes() == grown + tape + shared_extra
    step(rec, kind, inp, "float32", backend, inp["psfs"])
    assert rec._handle.workspace_bytes() == grown + tape + extra
    rec.release_tape()
    assert rec._handle.workspace_bytes() == grown


def test_refusals_with_the_switch_on(backend):
    """item 6: what stays refused, with the existing messages"""
    rng = np.random.default_rng(0)
    dev = backend.device

    def make(cls, h, w, d=1, B=2, **kw):
        psf = torch.from_numpy(rng.random((d, h, w, 3)).astype(np.float32)).to(dev)
        rec = cls(psf, n_iter=3, per_frame_grad=True, **kw)
        P5 = torch.stack([psf * (1 + 0.1 * b) for b in range(B)]).requires_grad_()
        return rec, P5, torch.from_numpy(rng.random((2, 1, h, w, 3)).astype(np.float32)).to(dev)

    for cls, kw in ((lpa.UnrolledADMM, {"psf_grad": True}), (lpa.UnrolledFISTA, {})):
        rec, P5, data = make(cls, 8, 12, **kw)                     # padded 15 x 24
        assert rec._padded_shape[1] == 15
        out = rec(data, psfs=P5)
        with pytest.raises(NotImplementedError, match="odd"):
            out.sum().backward()
        rec, P5, data = make(cls, 10, 12, d=2, **kw)
        out = rec(data, psfs=P5)
        with pytest.raises(NotImplementedError, match="depth"):
            out.sum().backward()
        rec, P5, data = make(cls, 10, 12, B=3, **kw)               # three PSFs against two measurements
        with pytest.raises(AssertionError, match="one PSF per measurement"):
            rec(data, psfs=P5)
        rec, P5, data = make(cls, 10, 12, **kw)                    # ... and the plain case works
        rec(data, psfs=P5).sum().backward()
        assert P5.grad is not None and P5.grad.shape == P5.shape and float(P5.grad.abs().max()) > 0
    rec, P5, data = make(lpa.UnrolledADMM, 10, 12)                 # no psf_grad=True
    with pytest.raises(NotImplementedError, match="gradient with respect to the PSF is not implemented"):
        rec(data, psfs=P5)
    rec(data, psfs=P5.detach()).sum().backward()                   # (the parameters and the measurement still train)
    assert rec._mu1_p.grad is not None
    rec, P5, data = make(lpa.UnrolledADMM, 10, 12, psf_grad=True, norm="ortho")
    with pytest.raises(NotImplementedError, match='norm="backward" only'):
        rec(data, psfs=P5)
    rec, P5, data = make(lpa.UnrolledFISTA, 10, 12, proj=lambda x: torch.clamp(x, min=0.01))
    with pytest.raises(NotImplementedError, match="only proj=non_neg"):
        rec(data, psfs=P5)
    with pytest.raises(NotImplementedError, match="background"):
        rec(data, psfs=P5, background=data)


def test_native_switch(backend):
    """item 6, the C ABI: the symbol is exported; with the switch off a per-frame handle refuses as include/lpc.h says
    (lpc_set_psf_batch: "per-frame"), with it on it records, takes PSFs while it records, and the backward entries run"""
    assert hasattr(backend.lib.dll, "lpc_per_frame_grad")
    header = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "lpc.h")).read()
    assert "int lpc_per_frame_grad(lpc_handle h, int on);" in header
    assert 'Refused, with a message that says "per-frame"' in header
    for kind in KINDS:
        inp, g = load(kind, RGB)
        rec = solver(kind, inp, "float32", backend)
        got = step(rec, kind, inp, "float32", backend, inp["psfs"])
        h = rec._handle
        w = torch.from_numpy(inp["w"])
        on = raw_backward(rec, kind, w, (2,))
        assert torch.equal(on[-1], got["g_psfs"])
        h.per_frame_grad(0)                                    # the parent's answers
        with pytest.raises(_native.NativeError, match="per-frame"):
            raw_backward(rec, kind, w, (2,))
        with pytest.raises(_native.NativeError, match="per-frame"):
            getattr(h, rec._record_method)(1)
        with pytest.raises(_native.NativeError, match="per-frame"):
            h.set_psf_batch(rec._psfs_dev.data_ptr(), 0)       # (the handle records)
        h.per_frame_grad(1)
        h.set_psf_batch(rec._psfs_dev.data_ptr(), 0)           # invalidates what was recorded, like lpc_set_psf
        with pytest.raises(_native.NativeError, match="iterations since the reset"):
            raw_backward(rec, kind, w, (2,))
        h.iterate(inp["n"], 0)
        again = raw_backward(rec, kind, w, (2,))
        for a, b in zip(on, again):
            assert torch.equal(a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_it_trains_a_per_mask_residual(backend, kind):
    """item 7: ten SGD steps in float64 on ``psfs = P5 + delta``, ``delta`` (B, 1, H, W, C) a leaf, towards another output:
    the loss falls and ``delta`` ends on the one of the same loop driven by torch.autograd over the restatement, frame by
    frame (100 * F64_TOL)"""
    inp, g = load(kind, RGB)
    dev = backend.device
    B = inp["data"].shape[0]
    rec = solver(kind, inp, "float64", backend)
    for q in params_of(rec, kind):
        q.requires_grad_(False)
    P5 = torch.from_numpy(inp["psfs"]).double()
    data = torch.from_numpy(inp["data"]).double()
    target = torch.from_numpy(g["out64"]) * (1 + 0.3 * torch.from_numpy(np.random.default_rng(5).random(g["out64"].shape) - 0.5))
    norm = float((target ** 2).mean())
    lr = (3.0 if kind == "admm" else 0.1) * float(P5.abs().max()) ** 2      # (ADMM's PSF gradient is the smaller one)

    def ours(delta):
        return rec(data.to(dev), psfs=P5.to(dev) + delta)

    def theirs(delta):
        outs = []
        for b in range(B):
            if kind == "admm":
                ps = [torch.from_numpy(inp["sched"][k]).double() for k in NAMES]
            else:
                ps = [torch.from_numpy(inp["sched"]["alpha"]).double(), torch.from_numpy(inp["sched"]["tk"])]
            outs.append(restated_frame(kind, inp, b, torch.float64, psf_b=P5[b] + delta[b], param_leaves=ps)[0][0])
        return torch.stack(outs)

    def loop(model, device):
        delta = torch.zeros(P5.shape, dtype=torch.float64, device=device, requires_grad=True)
        opt = torch.optim.SGD([delta], lr=lr)
        losses = []
        for _ in range(10):
            opt.zero_grad()
            loss = ((model(delta) - target.to(device)) ** 2).mean() / norm
            loss.backward()
            losses.append(float(loss.detach()))
            opt.step()
        return delta.detach(), losses

    mine, losses = loop(ours, dev)
    want, ref_losses = loop(theirs, torch.device("cpu"))
    r, moved = rel(mine, want.numpy()), float(want.abs().max() / P5.abs().max())
    print(f"{kind}: losses {losses[0]:.4e} -> {losses[-1]:.4e} (restated {ref_losses[-1]:.4e}); delta rel {r:.3e} "
          f"(bound {100 * F64_TOL:.0e}), moved by {moved:.2e} of the PSFs' scale")
    assert losses[-1] < losses[0] and ref_losses[-1] < ref_losses[0]
    assert moved > 1e-4 and r <= 100 * F64_TOL
