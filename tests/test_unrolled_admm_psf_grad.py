"""
Gradient of unrolled ADMM with respect to the PSF (lpc_admm_backward_psf; ``UnrolledADMM(psf, ..., psf_grad=True)`` with
``forward(batch, psfs=p)`` or ``_set_psf(p)`` and ``p.requires_grad``), through the public API, on the SIMT emulator
('emu') and on the MI355X ('hip', -m gpu).

Inputs: the fixtures of tests/test_unrolled_admm_grad.py (kink-free, 5 - 95 % of U non-zero and of q positive from the
second iteration on, asserted by their generator), loss ``(out * w).sum()``.  Reference: the gradient w.r.t. a leaf ``psfs``
of the REAL reference's ``UnrolledADMM.forward(batch, psfs=...)`` in float64 and float32
(tests/golden/gen_unrolled_admm_psf_grad.py, same inputs, ``out64`` bit-equal to the source fixture's).  The reference
refuses ``psfs`` when the data has fewer channels than the PSF: the gray-data / RGB-PSF case is checked against the float64
restatement (tests/unrolled_admm_restated.py with the PSF as a leaf), which test_restatement_with_psf_leaf_is_pinned pins
to the fixtures.

Bounds (those of tests/test_unrolled_psf_grad.py; max-norm over whole arrays, relative to the max of the float64 array):
  float32 engine:  rel(g_psf, ref64) <= 4 * max(rel(ref32, ref64), 2e-6), ref32 the reference's own float32 run (or the
                   float32 restatement);
  float64 engine:  <= 100 * F64_TOL = 1e-9;
and in the same run out, batch.grad and the four parameter gradients meet the bounds of tests/test_unrolled_admm_grad.py.

Largest distances of g_psf measured on the MI355X (31 cases of this file on the 'hip' backend):
  small fixtures, every launch plan, float32:  9.7e-7 (bound 8.0e-6);   gray data / RGB PSF: 5.0e-7 (8.0e-6)
  270 x 480 x 3, B = 2, n = 5, float32:        4.3e-5 (bound 1.1e-3; 757 kink elements in the reference's float64 run)
  float64 engine:                              1.8e-10 against the reference (the restatement's own distance; the engine is
                                               2e-15 from the restatement), 6.9e-16 against the restatement (gray / RGB)
ten SGD steps in float64 end on the restatement's PSF to 5.5e-17 and on its parameters exactly.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from unrolled_admm_restated import (F64_PLANS, F64_TOL, NAMES, PLANS, finite_diff, finite_diff_adj, rec_padded, rel,
                                    restated_admm)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SMALL = ["19x27x1_b2", "16x20x3_b2", "24x32x1_b2", "48x20x1_b2", "24x40x1_b2"]
RGB, GRAY = "16x20x3_b2", "16x20_gray_rgb"
KEYS = ("out", "g_data") + tuple("g_" + k for k in NAMES)
BASE = dict(mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-7)


@functools.lru_cache(maxsize=None)
def load(case):
    """(the source fixture of tests/test_unrolled_admm_grad.py, the PSF-gradient fixture or None)"""
    g = np.load(os.path.join(GOLDEN, f"unrolled_admm_grad_{case}.npz"))
    path = os.path.join(GOLDEN, f"unrolled_admm_psf_grad_{case}.npz")
    gp = np.load(path) if os.path.exists(path) else None
    assert gp is None or str(gp["source"]) == f"unrolled_admm_grad_{case}"
    return g, gp


def sched_of(g):
    return {k: g[k] for k in NAMES}


def params_of(rec):
    return [getattr(rec, f"_{k}_p") for k in NAMES]


def tdt_of(dtype):
    return torch.float64 if dtype == "float64" else torch.float32


def restated_psf_grad(g, tdt, frame=None, model=restated_admm, **kw):
    """out and d (out * w).sum() / d psf of the restatement in ``tdt``, the PSF a leaf"""
    sel = slice(None) if frame is None else slice(frame, frame + 1)
    p = torch.from_numpy(g["psf"]).to(tdt).requires_grad_()
    ps = [torch.from_numpy(g[k]).double() for k in NAMES]
    out = model(p, torch.from_numpy(g["data"][sel]).to(tdt), *ps, int(g["n_iter"]), dtype=tdt, **kw)
    out = out[0] if isinstance(out, tuple) else out
    (out * torch.from_numpy(g["w"][sel]).to(tdt)).sum().backward()
    return out.detach().numpy(), p.grad.numpy()


@functools.lru_cache(maxsize=None)
def psf_refs(case, frame=None):
    """float64 / float32 restatement's PSF gradient (``frame``: of that frame of the batch alone); computed once, never
    written to"""
    g = load(case)[0]
    return {tdt: restated_psf_grad(g, tdt, frame)[1] for tdt in (torch.float64, torch.float32)}


def f32_bound(ref32, ref64):
    return 4 * max(rel(ref32, ref64), 2e-6)


def psf_bound(dtype, ref32, ref64):
    return 100 * F64_TOL if dtype == "float64" else f32_bound(ref32, ref64)


def solver(g, dtype, backend, **kw):
    rec = lpa.UnrolledADMM(torch.from_numpy(g["psf"]).to(backend.device), dtype=dtype, n_iter=int(g["n_iter"]), **BASE,
                           **kw)
    rec.set_parameters(**sched_of(g))
    return rec


def engine_run(g, dtype, backend, frame=None, how="forward", psf_grad=True):
    """forward + backward of ``(out * w).sum()``; ``how``: "forward" psfs=p, "set_psf" _set_psf(p), "plain" no PSF leaf"""
    tdt, dev = tdt_of(dtype), backend.device
    sel = slice(None) if frame is None else slice(frame, frame + 1)
    rec = solver(g, dtype, backend, **({"psf_grad": True} if psf_grad else {}))
    p = torch.from_numpy(g["psf"]).to(device=dev, dtype=tdt).requires_grad_()
    batch = torch.from_numpy(g["data"][sel]).to(device=dev, dtype=tdt).requires_grad_()
    if how == "forward":
        out = rec(batch, psfs=p)
    elif how == "set_psf":
        rec._set_psf(p)
        out = rec(batch)
    else:
        out = rec(batch)
    (out * torch.from_numpy(g["w"][sel]).to(device=dev, dtype=tdt)).sum().backward()
    got = {"out": out.detach(), "g_data": batch.grad, "g_psf": p.grad}
    got.update({"g_" + k: q.grad for k, q in zip(NAMES, params_of(rec))})
    return rec, p, got


def raw_backward_psf(rec, grad_out, with_psf=True, entry="psf"):
    """lpc_admm_backward_psf (or lpc_admm_backward) itself, on the tape of the last forward: the six outputs"""
    gp = rec._empty((4, rec._n_iter))
    go = rec._to_dev(grad_out)
    gd = rec._empty((go.shape[0],) + tuple(go.shape[2:]))
    gpsf = rec._empty(tuple(int(v) for v in rec._psf_shape)) if with_psf else None
    ptrs = (go.data_ptr(), gd.data_ptr()) + tuple(gp[k].data_ptr() for k in range(4))
    if entry == "psf":
        rec._handle.admm_backward_psf(*ptrs, None if gpsf is None else gpsf.data_ptr(), rec._stream())
    else:
        rec._handle.admm_backward(*ptrs, rec._stream())
    return [gd] + [gp[k].clone() for k in range(4)] + ([gpsf] if with_psf else [])


def check_case(case, dtype, backend, tag):
    """g_psf against the PSF-gradient fixture, and out, batch.grad, the parameter gradients of the same run against the
    source fixture with the bounds of tests/test_unrolled_admm_grad.py: check_parity"""
    g, gp = load(case)
    rec, p, got = engine_run(g, dtype, backend)
    assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device == p.device
    if dtype == "float64":      # the parameter gradients as the entry point writes them, in float64
        raw = raw_backward_psf(rec, torch.from_numpy(g["w"]).double())
        assert torch.equal(raw[5].reshape(p.shape), p.grad)
        for i, (k, q) in enumerate(zip(NAMES, params_of(rec))):
            assert torch.equal(q.grad.cpu(), (raw[1 + i].cpu() * torch.sign(q.detach().cpu()).double()).float()), k
            got["g_" + k] = raw[1 + i]
    bad = []
    for k in KEYS:
        if dtype == "float64":
            r, bound = rel(got[k], g["r_" + k]), 100 * F64_TOL
        else:
            r, bound = rel(got[k], g[k + "64"]), f32_bound(g[k + "32"], g[k + "64"])
        print(f"{tag} {dtype} {k}: rel {r:.3e} (bound {bound:.1e})")
        if not r <= bound:
            bad.append((k, r, bound))
    r, bound = rel(got["g_psf"], gp["g_psf64"]), psf_bound(dtype, gp["g_psf32"], gp["g_psf64"])
    print(f"{tag} {dtype} g_psf: rel {r:.3e} (bound {bound:.1e})")
    if not r <= bound:
        bad.append(("g_psf", r, bound))
    assert not bad, bad
    return rec


# ------------------------------------------------------------------------------------------------- CPU only --
@pytest.mark.parametrize("case", SMALL)
def test_restatement_with_psf_leaf_is_pinned(case):
    """The float64 restatement with the PSF as a leaf against the reference's own float64 output and ``psfs`` gradient.
    The reference divides tau / mu2 in float32 (its parameters are float32 tensors); the restatement that does the same
    (``split_psf_admm(theta32=True)``) meets BOTH ``out64`` and ``g_psf64`` within 100 * F64_TOL (measured: 5.5e-16 ..
    9.6e-16 and 3.0e-16 .. 4.2e-16).  ``restated_admm`` divides in the working dtype, as the engine does: its ``g_psf``
    meets 100 * F64_TOL as well (2.9e-11 .. 1.8e-10), its ``out`` sits 1.0e-9 .. 1.6e-9 from ``out64`` -- the source
    fixture's ``dist_out``, which tests/test_unrolled_admm_grad.py bounds by 1e-7 for this reason -- and is pinned to the
    values stored there.  The float32 flavour is no further from ``g_psf64`` than the reference's own float32 run allows."""
    g, gp = load(case)
    assert np.array_equal(gp["out64"], g["out64"]) and gp["g_psf64"].shape == g["psf"].shape
    assert rel(gp["g_psf32"], gp["g_psf64"]) <= 5e-5
    out, gpsf = restated_psf_grad(g, torch.float64, model=split_psf_admm, theta32=True)
    for k, v in (("out", out), ("g_psf", gpsf)):
        r = rel(v, gp[k + "64"])
        print(f"{case} restated float64, float32 tau / mu2, {k}: rel {r:.3e} (bound {100 * F64_TOL:.1e})")
        assert v.shape == gp[k + "64"].shape and r <= 100 * F64_TOL, (k, r)
    out, gpsf = restated_psf_grad(g, torch.float64)
    r = rel(gpsf, gp["g_psf64"])
    print(f"{case} restated_admm float64 g_psf: rel {r:.3e} (bound {100 * F64_TOL:.1e}), out {rel(out, gp['out64']):.3e}")
    assert r <= 100 * F64_TOL and rel(out, g["r_out"]) <= F64_TOL and rel(out, gp["out64"]) <= 1e-7, r
    assert rel(gpsf, psf_refs(case)[torch.float64]) <= F64_TOL
    out, gpsf = restated_psf_grad(g, torch.float32)
    r, bound = rel(gpsf, gp["g_psf64"]), f32_bound(gp["g_psf32"], gp["g_psf64"])
    print(f"{case} restated float32 g_psf: rel {r:.3e} (bound {bound:.1e})")
    assert r <= bound, (r, bound)


def split_psf_admm(psf, data, mu1_p, mu2_p, mu3_p, tau_p, n, dtype=torch.float64, detach=(), theta32=False):
    """restated_admm with the PSF spectrum entering H V ("hv"), HT ("ht") and R_divmat ("rdiv") as three copies, each of
    which ``detach`` can cut off the graph: what a backward that forgets one of the three terms computes.  ``theta32``: the
    threshold tau / mu2 divided in float32, as the reference divides its float32 parameters"""
    psf, data = psf.to(dtype), data.to(dtype)
    D, H, W, C = psf.shape
    Hp, Wp = rec_padded(H), rec_padded(W)
    sh, sw = (Hp - H) // 2, (Wp - W) // 2

    def pad(v):
        o = torch.zeros(v.shape[:-3] + (Hp, Wp, C), dtype=v.dtype)
        o[..., sh:sh + H, sw:sw + W, :] = v
        return o

    Hs = torch.fft.rfft2(pad(psf), dim=(-3, -2))
    Hs_hv, Hs_ht, Hs_r = (Hs.detach() if k in detach else Hs for k in ("hv", "ht", "rdiv"))
    HH = (Hs_r.conj() * Hs_r).abs()
    gram = torch.zeros((D, Hp, Wp, C), dtype=dtype)
    gram[0, 0, 0] = 4
    gram[0, 0, 1] = gram[0, 0, -1] = gram[0, 1, 0] = gram[0, -1, 0] = -1
    G = torch.fft.rfft2(gram, dim=(-3, -2)).abs()

    def conv(x, spec):
        X = torch.fft.rfft2(x, dim=(-3, -2)) * spec
        return torch.fft.ifftshift(torch.fft.irfft2(X, dim=(-3, -2), s=(Hp, Wp)), dim=(-3, -2))

    m1, m2, m3, tau = (p.abs().to(dtype) for p in (mu1_p, mu2_p, mu3_p, tau_p))
    b, mask = pad(data), pad(torch.ones_like(psf))
    v = torch.zeros((data.shape[0], D, Hp, Wp, C), dtype=dtype)
    hv, xi, rho = torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)
    pv = torch.zeros(v.shape + (2,), dtype=dtype)
    eta = torch.zeros_like(pv)
    for i in range(n):
        s = pv + eta / m2[i]
        theta = (tau[i].float() / m2[i].float()).to(dtype) if theta32 else tau[i] / m2[i]
        U = torch.sign(s) * torch.clamp(s.abs() - theta, min=0)
        X = (xi + m1[i] * hv + b) / (mask + m1[i])
        Wv = torch.clamp(rho / m3[i] + v, min=0)
        rk = (m3[i] * Wv - rho) + finite_diff_adj(m2[i] * U - eta) + conv(m1[i] * X - xi, Hs_ht.conj())
        R = 1.0 / (m1[i] * HH + m2[i] * G + m3[i])
        v = torch.fft.irfft2(R * torch.fft.rfft2(rk, dim=(-3, -2)), dim=(-3, -2), s=(Hp, Wp))
        hv, pv = conv(v, Hs_hv), finite_diff(v)
        xi = xi + m1[i] * (hv - X)
        eta = eta + m2[i] * (pv - U)
        rho = rho + m3[i] * (v - Wv)
    return torch.clamp(v[..., sh:sh + H, sw:sw + W, :], min=0)


@pytest.mark.parametrize("case", [RGB, "24x32x1_b2"])
def test_the_check_has_teeth(case):
    """restatement alone: a PSF gradient that leaves out the term through H V, through HT or through R_divmat is off by
    more than 100 x the float32 bound"""
    g, gp = load(case)
    out, good = restated_psf_grad(g, torch.float64, model=split_psf_admm)
    assert rel(good, psf_refs(case)[torch.float64]) <= F64_TOL and rel(out, g["out64"]) <= 1e-7
    bound = f32_bound(gp["g_psf32"], gp["g_psf64"])
    for tooth in ("hv", "ht", "rdiv"):
        out_t, bad = restated_psf_grad(g, torch.float64, model=split_psf_admm, detach=(tooth,))
        moved = rel(bad, good) / bound
        print(f"{case} without the {tooth} term: g_psf moves by {rel(bad, good):.2e} = {moved:.0f} x the float32 bound")
        assert np.array_equal(out_t, out) and moved > 100, (tooth, moved)


# ----------------------------------------------------------------------------------------- emulator and card --
@pytest.mark.parametrize("plan,dtype", [(p, "float32") for p in sorted(PLANS)] + [(p, "float64") for p in F64_PLANS])
def test_psf_gradient_parity_every_launch_plan(backend, monkeypatch, plan, dtype):
    """the point-wise accumulate works in the spectra's own layout: the same gradient on every launch plan"""
    case = PLANS[plan]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **case["opts"]})
    rec = check_case(case["fixture"][len("unrolled_admm_grad_"):], dtype, backend, plan)
    info = rec._handle.plan_info()
    for marker in case["info"] + case.get("f32" if dtype == "float32" else "f64", []):
        assert marker in info, (marker, info)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_three_channels(backend, dtype):
    check_case(RGB, dtype, backend, RGB)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gray_data_rgb_psf(backend, dtype):
    """one data channel against a three-channel PSF (the reference refuses ``psfs`` there): against the restatement"""
    g = load(GRAY)[0]
    assert g["data"].shape[-1] == 1 and g["psf"].shape[-1] == 3
    rec, p, got = engine_run(g, dtype, backend)
    refs = psf_refs(GRAY)
    r, bound = rel(got["g_psf"], refs[torch.float64]), psf_bound(dtype, refs[torch.float32], refs[torch.float64])
    print(f"{GRAY} {dtype} g_psf: rel {r:.3e} (bound {bound:.1e})")
    assert got["g_psf"].shape == p.shape and r <= bound, (r, bound)
    assert got["g_data"].shape == tuple(g["data"].shape)
    if dtype == "float32":
        for k in ("out", "g_data"):
            assert rel(got[k], g[k + "64"]) <= f32_bound(g[k + "32"], g[k + "64"]), k


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_set_psf_route_gives_the_same_bits(backend, dtype):
    g = load(RGB)[0]
    a = engine_run(g, dtype, backend, how="forward")[2]
    rec, p, b = engine_run(g, dtype, backend, how="set_psf")
    assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.device == p.device
    for k in a:
        assert float(a[k].abs().max()) > 0 and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_batch_sum_is_the_sum_of_the_frames(backend, dtype):
    """g_psf of a batch of two = g_psf of frame 0 alone + g_psf of frame 1 alone"""
    g = load(RGB)[0]
    both = engine_run(g, dtype, backend)[2]["g_psf"]
    singles = []
    for b in range(2):
        g1 = engine_run(g, dtype, backend, frame=b)[2]["g_psf"]
        refs = psf_refs(RGB, b)
        r, bound = rel(g1, refs[torch.float64]), psf_bound(dtype, refs[torch.float32], refs[torch.float64])
        print(f"{RGB} {dtype} frame {b}: rel {r:.3e} (bound {bound:.1e})")
        assert r <= bound, (b, r, bound)
        singles.append(g1)
    refs = psf_refs(RGB)
    assert rel(psf_refs(RGB, 0)[torch.float64] + psf_refs(RGB, 1)[torch.float64], refs[torch.float64]) <= F64_TOL
    r, bound = rel(singles[0] + singles[1], both), psf_bound(dtype, refs[torch.float32], refs[torch.float64])
    print(f"{RGB} {dtype} frame 0 + frame 1 against the batch: rel {r:.3e} (bound {bound:.1e})")
    assert r <= bound, (r, bound)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_nothing_else_moves(backend, dtype):
    """out, batch.grad and the parameter gradients have the bits of a default solver's; the entry point is deterministic;
    without a PSF pointer it is lpc_admm_backward"""
    g = load(RGB)[0]
    rec, p, got = engine_run(g, dtype, backend)
    plain = engine_run(g, dtype, backend, how="plain", psf_grad=False)[2]
    assert plain["g_psf"] is None and float(got["g_psf"].abs().max()) > 0
    for k in KEYS:
        assert float(got[k].abs().max()) > 0 and torch.equal(got[k], plain[k]), k
    w = torch.from_numpy(g["w"])
    first, second = raw_backward_psf(rec, w), raw_backward_psf(rec, w)
    assert len(first) == 6 and torch.equal(first[5].reshape(p.shape), p.grad)
    for a, b in zip(first, second):
        assert float(a.abs().max()) > 0 and torch.equal(a, b)
    null, old = raw_backward_psf(rec, w, with_psf=False), raw_backward_psf(rec, w, with_psf=False, entry="plain")
    for a, b, c in zip(null, old, first):
        assert torch.equal(a, b) and torch.equal(a, c)


def psf_workspace_bytes(B, C, Hp, Wp, itemsize):
    """include/lpc.h, lpc_admm_backward_psf"""
    cpitch = (Wp // 2 + 1 + 15) // 16 * 16
    return (4 * B * C + C) * Hp * cpitch * 2 * itemsize


def test_workspace(backend):
    """no PSF gradient asked for: the workspace is base + tape as before and p.grad stays None; asked for: + the documented
    formula from the first backward that needs it on, through a pause, and release_tape() gives all of it back"""
    g = load(RGB)[0]
    dev = backend.device
    rec = solver(g, "float32", backend, psf_grad=True)
    data, wts = torch.from_numpy(g["data"]).to(dev), torch.from_numpy(g["w"]).to(dev)
    with torch.no_grad():
        rec(data)
    base = rec._handle.workspace_bytes()
    B, _, H, W, C = data.shape
    n = int(g["n_iter"])
    Hp, Wp = rec._padded_shape[1:3]
    rpitch = (Wp + 3) // 4 * 4
    tape = (6 * n + 11) * B * C * Hp * rpitch * 4 + n * B * C * -(-Hp // 8) * -(-Wp // 128) * 4 * 8    # lpc_admm_record
    p = torch.from_numpy(g["psf"]).to(dev)
    (rec(data, psfs=p) * wts).sum().backward()
    assert rec._handle.workspace_bytes() == base + tape and p.grad is None and rec._mu1_p.grad is not None
    p = p.clone().requires_grad_()
    out = rec(data, psfs=p)
    assert rec._handle.workspace_bytes() == base + tape      # allocated by the first backward that needs it
    (out * wts).sum().backward()
    extra = psf_workspace_bytes(B, C, Hp, Wp, 4)
    assert p.grad is not None and rec._handle.workspace_bytes() == base + tape + extra
    with torch.no_grad():          # a pause keeps it
        rec(data)
    assert rec._handle.workspace_bytes() == base + tape + extra
    (rec(data, psfs=p) * wts).sum().backward()
    assert rec._handle.workspace_bytes() == base + tape + extra
    rec.release_tape()
    assert rec._handle.workspace_bytes() == base
    (rec(data, psfs=p) * wts).sum().backward()
    assert rec._handle.workspace_bytes() == base + tape + extra


def test_refusals(backend):
    rng = np.random.default_rng(0)
    dev = backend.device

    def solver_of(h, w, d=1, **kw):
        psf = torch.from_numpy(rng.random((d, h, w, 3)).astype(np.float32)).to(dev)
        rec = lpa.UnrolledADMM(psf, n_iter=3, psf_grad=True, **kw)
        return rec, psf.clone().requires_grad_(), torch.from_numpy(rng.random((2, 1, h, w, 3)).astype(np.float32)).to(dev)

    def forward_only_works(rec, data):
        with torch.no_grad():
            out = rec(data)
        assert not out.requires_grad and float(out.abs().max()) > 0
        return out

    rec, p, data = solver_of(10, 12)
    with pytest.raises(NotImplementedError, match="per-frame"):
        rec(data, psfs=torch.stack([p, p]))
    forward_only_works(rec, data)
    rec, p, data = solver_of(8, 12)                            # padded 15 x 24
    assert rec._padded_shape[1] == 15
    out = rec(data, psfs=p)
    with pytest.raises(NotImplementedError, match="odd"):
        out.sum().backward()
    assert torch.equal(forward_only_works(rec, data), out.detach())
    rec, p, data = solver_of(10, 12, d=2)
    out = rec(data, psfs=p)
    with pytest.raises(NotImplementedError, match="depth"):
        out.sum().backward()
    assert torch.equal(forward_only_works(rec, data), out.detach())
    # a norm other than "backward": the Python surface before anything runs, and the C entry point itself
    rec, p, data = solver_of(10, 12, norm="ortho")
    with pytest.raises(NotImplementedError, match='norm="backward" only'):
        rec(data, psfs=p)
    forward_only_works(rec, data)
    rec._set_psf(p)
    with pytest.raises(NotImplementedError, match='norm="backward" only'):
        rec(data)
    rec._set_psf(p.detach())
    plain = forward_only_works(rec, data)
    out = rec(data)                                            # the parameters and the measurement still train
    out.sum().backward()
    assert torch.equal(out.detach(), plain) and rec._mu1_p.grad is not None
    buf = torch.zeros(data.numel(), dtype=torch.float32, device=dev)
    ptrs = (buf.data_ptr(), None) + tuple(buf[4 * k:].data_ptr() for k in range(4))
    gp = torch.zeros(p.numel(), dtype=torch.float32, device=dev)
    with pytest.raises(_native.NativeError, match='norm "backward" only'):
        rec._handle.admm_backward_psf(*ptrs, gp.data_ptr(), 0)
    rec._handle.admm_backward_psf(*ptrs, None, 0)
    # the initial estimate, a custom psi and a denoiser are refused as before
    est = torch.from_numpy(rng.random((1, 1, 20, 24, 3)).astype(np.float32) * 0.1).to(dev)
    rec, p, data = solver_of(10, 12, initial_est=est)
    out = rec(data, psfs=p)
    with pytest.raises(NotImplementedError, match="initial estimate"):
        out.sum().backward()
    forward_only_works(rec, data)
    rec, p, data = solver_of(10, 12, denoiser={"network": lambda x, s: x, "noise_level": 0.1})
    with pytest.raises(NotImplementedError, match="custom psi and a denoiser"):
        rec(data, psfs=p)
    # native level: no tape
    rec, p, data = solver_of(10, 12)
    forward_only_works(rec, data)
    with pytest.raises(_native.NativeError, match="nothing recorded"):
        rec._handle.admm_backward_psf(*ptrs, gp.data_ptr(), 0)
    rec(data)
    go = torch.ones(data.numel(), dtype=torch.float32, device=dev)
    rec._handle.admm_backward_psf(go.data_ptr(), *ptrs[1:], gp.data_ptr(), 0)
    assert float(gp.abs().max()) > 0


def test_it_trains_the_psf(backend):
    """10 SGD steps on the PSF and all four parameter vectors towards the fixture's float64 output, from a perturbed PSF
    (float64 build): the loss falls, and PSF and parameters equal those of the same loop driven by torch.autograd over the
    restatement (100 * F64_TOL)"""
    g = load(RGB)[0]
    n, dev = int(g["n_iter"]), backend.device
    start = {k: g[k] * f for k, f in zip(NAMES, (0.8, 1.25, 0.9, 1.3))}
    rec = solver(g, "float64", backend, psf_grad=True)
    rec.set_parameters(**start)
    mine = params_of(rec)
    theirs = [q.detach().cpu().clone().requires_grad_() for q in mine]
    psf0 = torch.from_numpy(g["psf"]).double()
    psf0 = psf0 * (1 + 0.2 * torch.from_numpy(np.random.default_rng(5).random(psf0.shape) - 0.5))
    p_mine, p_theirs = psf0.clone().to(dev).requires_grad_(), psf0.clone().requires_grad_()
    target, data = torch.from_numpy(g["out64"]), torch.from_numpy(g["data"]).double()
    norm = float((target ** 2).mean())

    def loop(params, p, model):
        groups = [{"params": [q], "lr": 0.02 * float(np.abs(g[k]).max()) ** 2} for k, q in zip(NAMES, params)]
        opt = torch.optim.SGD(groups + [{"params": [p], "lr": 0.1 * float(psf0.abs().max()) ** 2}])
        losses = []
        for _ in range(10):
            opt.zero_grad()
            loss = ((model() - target.to(p.device)) ** 2).mean() / norm
            loss.backward()
            losses.append(float(loss.detach()))
            opt.step()
        return losses

    losses = loop(mine, p_mine, lambda: rec(data.to(dev), psfs=p_mine))
    ref_losses = loop(theirs, p_theirs, lambda: restated_admm(p_theirs, data, *theirs, n)[0])
    print("losses", losses, "restated", ref_losses)
    assert losses[-1] < losses[0] and ref_losses[-1] < ref_losses[0]
    for k, q, t, s in zip(NAMES, mine, theirs, start.values()):
        r = rel(q, t.detach().numpy())
        print(f"after 10 steps: {k} rel {r:.3e} (bound {100 * F64_TOL:.0e}), moved by {rel(q, s):.2e}")
        assert r <= 100 * F64_TOL and rel(q, s) > 1e-4, k
    r, moved = rel(p_mine, p_theirs.detach().numpy()), rel(p_mine, psf0.numpy())
    print(f"after 10 steps: psf rel {r:.3e} (bound {100 * F64_TOL:.0e}), moved by {moved:.2e}")
    assert r <= 100 * F64_TOL and moved > 1e-4


@pytest.mark.gpu
def test_psf_gradient_diffusercam_size():
    """270 x 480 x 3, B = 2, n = 5 (padded 540 x 960, the pre-built plan module), inputs in closed form, float32 engine;
    g_psf compared on the fixture's crops + lattice.  GPU only: the frame takes minutes on the emulator."""
    from types import SimpleNamespace

    from lenslesspicam_amd import recon

    backend = SimpleNamespace(device=recon.runtime()[1])
    sys.path.insert(0, GOLDEN)
    import longrun_inputs as lin

    g, gp = load("c1")
    B, H, W, C = (int(v) for v in g["shape"])
    seed, n = int(g["seed"]), int(g["n_iter"])
    psf = lin.psf12(1, H, W, C, 100 + seed)
    data = np.stack([lin.measurement(H, W, C, 10 * seed + b) for b in range(B)])[:, None]
    w = np.random.default_rng(300 + seed).random((B, 1, H, W, C), dtype=np.float32) - np.float32(0.5)
    for a, fp in ((psf, "fp_psf"), (data, "fp_data"), (w, "fp_w")):
        assert np.array_equal(lin.fingerprint(a), g[fp]), fp
    rec = lpa.UnrolledADMM(torch.from_numpy(psf).to(backend.device), n_iter=n, psf_grad=True, **BASE)
    rec.set_parameters(**sched_of(g))
    p = torch.from_numpy(psf).to(backend.device).requires_grad_()
    out = rec(torch.from_numpy(data).to(backend.device), psfs=p)
    info = rec._handle.plan_info()
    assert "padded 540x960" in info and "; plan module " in info, info
    (out * torch.from_numpy(w).to(backend.device)).sum().backward()
    crops, lattice = lin.samples(p.grad.cpu().numpy()[0])
    err = max(np.abs(crops - gp["g_psf64_crops"]).max(), np.abs(lattice - gp["g_psf64_lattice"]).max())
    r, bound = float(err) / float(gp["g_psf64_max"]), 4 * max(float(gp["rel32_g_psf"]), 2e-6)
    print(f"c1 float32 g_psf: rel {r:.3e} (bound {bound:.1e})")
    assert r <= bound, (r, bound)
    for k, q in zip(NAMES, params_of(rec)):      # ... and the parameter gradients of the same run
        assert rel(q.grad, g["g_" + k + "64"]) <= 4 * max(float(g["rel32_g_" + k]), 2e-6), k
