"""
One PSF per measurement (``forward(batch, psfs=P5)``, ``ADMM.apply_batch(psfs=P5)``, ``RealFFTConvolve2D(P5)``,
lpc_set_psf_batch) over launch plans, shapes and dtypes, through the public API, on the SIMT emulator ('emu') and on the
MI355X ('hip', -m gpu).  Inference only: a forward that records refuses a 5-D ``psfs``.

What per-frame PSFs cross inside the engine: every kernel that multiplies by H -- the run-time and register convolution
middles, ADMM's 24-point register middle, its side-by-side LDS middle, the sequential middle with its precombined
constants (k_mid_consts, complex and real phases), the pair-line copy of H, lpc_convolve_spectrum -- picks PSF plane
``q % PlaneGeom::PM`` where it picked ``q % (D C)``.  The ADMM cases, their options and their plan markers are those of
tests/test_unrolled_admm_sweep.py (asserted in ``plan_info()``), with B = 3 where C = 1 and B = 2 where C = 3; the
gradient-descent cases those of tests/test_psf_swap.py.

1. Against the oracle, per frame: ``ADMMOracle(P5[b], dtype=float64, schedule=...)``; for UnrolledFISTA the oracle's
   convolver and gradient (``GDOracle(P5[b])``) under the loop of ``unrolled_fista_oracle`` started from the CONSTRUCTOR's
   PSF's start value with the constructor's steps (unrolled_fista.py:57-72: a per-frame PSF changes nothing but H).
   Bounds (the rule of tests/test_unrolled_admm_sweep.py; max-norm over a frame's array, relative to the max of the float64
   array):
     float32 engine:  rel(q, oracle64) <= 4 * max(rel(oracle32, oracle64), 2e-6); a final-image yardstick above
                      YARDSTICK_MAX = 2.5e-6 (x 10 for U, eta, rho) is refused: pick another seed;
     float64 engine:  ADMM F64_TOL = 1e-11 (x 100 for U, eta, rho, xi); FISTA 100 * F64_TOL, the bound its float64 forward
                      has in tests/test_unrolled_psf_grad.py and tests/test_psf_swap.py.
   The yardstick is always the float32 oracle, never the engine.  One D = 2 ADMM case: the engine runs D independent planes
   per frame (state plane fr * D C + d * C + c); the oracle, like the reference, takes D = 1, so plane d of frame b is
   compared with ``ADMMOracle(P5[b][d:d+1])``.
2. Teeth, on the oracle alone: with the PSFs of frames 0 and 1 swapped each frame's result moves by more than 100 x its
   float32 bound.
3. Bitwise: (a) ``psfs = stack([p] * B)`` equals the shared-PSF run; (b) a frame of the per-frame batch equals the
   single-frame run with that PSF wherever ``plan_info()`` of the two handles agrees (else: bound 1); (c) per-frame ->
   one PSF -> per-frame again on one solver reproduces the first result (stale precombined constants / pair-line copies).
4. The reference itself: tests/golden/unrolled_{admm,fista}_psfs5d_*.npz (gen_per_frame_psf.py), same 4 x rule.
5. The operator: ``RealFFTConvolve2D(P5)`` against torch.fft in float64 per frame at the 2e-6 of
   tests/test_parity_small.py's operator tests; ``reconstruction_error`` at tests/test_metrics.py's 2e-5.
6. Refusals and the ABI: recording forwards, lpc_*_record and the backwards say "per-frame"; a plain FISTA handle refuses
   lpc_set_psf_batch; ``workspace_bytes()`` grows by the formula of include/lpc.h.
"""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from oracle import lensless_oracle as orc
from test_custom_psi import psi2, psi2_adj, psi2_gram
from test_pnp_hook import pnp_denoise
from test_psf_swap import GD_CASES
from test_unrolled_admm_sweep import (BASE, CASES as SWEEP_CASES, DUALS, F64_CASES as SWEEP_F64, N_ITER, STATES,
                                      YARDSTICK_MAX, bound_of, compare, markers, schedule, states_of)
from test_unrolled_psf_grad import default_init
from unrolled_restated import F64_TOL, default_steps, rel

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ["rt", "rt_odd", "mod", "mod_tiled", "rows_half", "split_reg", "split_lds", "split_mod", "seq_odd", "seq_even",
         "pair", "gterms"]
CASES = {}
for _i, _n in enumerate(NAMES):
    _H, _W, _C, _ = SWEEP_CASES[_n]["shape"]
    CASES[_n] = dict(SWEEP_CASES[_n], shape=(_H, _W, _C, 3 if _C == 1 else 2), seed=700 + 10 * _i, depth=1)
CASES["depth2"] = dict(SWEEP_CASES["mod"], shape=(24, 32, 3, 2), seed=900, depth=2)     # plane fr * D C + d * C + c
F64_CASES = [n for n in NAMES if n in SWEEP_F64]
CASE_DTYPES = [(c, "float32") for c in CASES] + [(c, "float64") for c in F64_CASES]
STATE_CASES = ["rt_odd", "mod", "seq_odd", "split_reg"]
GD_ITERS = 4
PNP, PNP_LEVEL = dict(mu1=1e-4, mu2=1e-3, mu3=1e-3), 12.0       # the step sizes of tests/test_hooks_over_plans.py
PSI = dict(mu1=1e-2, mu2=1e-2, mu3=1e-2, tau=2e-4)
FISTA_F64 = ["rt", "split_mod"]
FISTA_CASE_DTYPES = [(c, "float32") for c in GD_CASES] + [(c, "float64") for c in FISTA_F64]


def tdt_of(dtype):
    return torch.float64 if dtype == "float64" else torch.float32


def on(backend, a, tdt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=backend.device, dtype=tdt)


def _snapshot(o):
    return {k: getattr(o, k).numpy().copy() for k, _ in STATES}


# ------------------------------------------------------------------------------------------------ ADMM inputs --
@functools.lru_cache(maxsize=None)
def inputs(name):
    """per-frame PSFs and measurement of a case and, per frame and depth plane, the float64 / float32 oracle under
    ``schedule()``: the eight states after N_ITER iterations (no form_image before) and the final image; computed once,
    never written to"""
    case = CASES[name]
    (H, W, C, B), D = case["shape"], case["depth"]
    rng = np.random.default_rng(case["seed"])
    psfs = np.stack([orc.synthetic_psf(D, H, W, C, case["seed"] + b) for b in range(B)])
    data = rng.random((B, 1, H, W, C), dtype=np.float32)
    inp = SimpleNamespace(name=name, psfs=psfs, data=data, sched=schedule(), ref={})
    for tdt in (torch.float64, torch.float32):
        inp.ref[tdt] = [[oracle_frame(psfs[b][d:d + 1], data[b, 0], inp.sched, tdt) for d in range(D)] for b in range(B)]
    for b in range(B):
        for d in range(D):
            f32, f64 = inp.ref[torch.float32][b][d], inp.ref[torch.float64][b][d]
            pairs = [("final", f32.final, f64.final)] + [(k, f32.states[k], f64.states[k]) for k, _ in STATES]
            for key, a32, a64 in pairs:
                y, most = rel(a32, a64), YARDSTICK_MAX * (10 if key in ("U", "eta", "rho") else 1)
                assert y <= most, f"{name} frame {b} plane {d} {key}: float32 oracle {y:.2e} from the float64 oracle: pick another seed"
    return inp


def oracle_frame(psf, y, sched, tdt):
    o = orc.ADMMOracle(psf, dtype=tdt, schedule=sched, **BASE)
    o.set_data(y)
    o.reset()
    for _ in range(N_ITER):
        o.step()
    states = _snapshot(o)
    return SimpleNamespace(states=states, final=o.form_image()[0].numpy().copy())


def solver(name, dtype, backend, monkeypatch, frames=None, cls=lpa.UnrolledADMM, psf_frame=0):
    """a solver of the case, constructed from the PSF of frame ``psf_frame``, on its launch plan (asserted) with the handle
    of the batch ``frames`` selects; the measurement and the PSFs of those frames on the backend's device"""
    case, inp = CASES[name], inputs(name)
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **case["opts"]})
    tdt = tdt_of(dtype)
    sel = slice(None) if frames is None else frames
    rec = cls(on(backend, inp.psfs[psf_frame], tdt), dtype=dtype, n_iter=N_ITER, **BASE)
    if cls is lpa.UnrolledADMM:
        rec.set_parameters(**inp.sched)
    data, psfs = on(backend, inp.data[sel], tdt), on(backend, inp.psfs[sel], tdt)
    rec._data = data
    rec._upload_data()
    info = rec._handle.plan_info()
    for marker in markers(name if name in SWEEP_CASES else "mod", dtype):
        assert marker in info, (marker, info)
    assert info.endswith(case.get("ends", "") if dtype == "float32" else ""), info
    return rec, data, psfs


def check_frames(name, dtype, out, inp, bad, frames=None):
    B, D = inp.data.shape[0], inp.psfs.shape[1]
    frames = range(B) if frames is None else frames
    assert tuple(out.shape) == (len(frames), D) + inp.data.shape[2:4] + (inp.psfs.shape[-1],), tuple(out.shape)
    for i, b in enumerate(frames):
        for d in range(D):
            compare(f"{name} frame {b} plane {d}", dtype, "final", out[i, d:d + 1].cpu().numpy(),
                    inp.ref[torch.float32][b][d].final, inp.ref[torch.float64][b][d].final, bad)


# ----------------------------------------------------------------------------------------------- FISTA inputs --
def fista_oracle(p0, psf, y, alpha, tk, tdt):
    """``orc.unrolled_fista_oracle`` with the convolver of ``psf`` and the start value of the constructor's PSF ``p0``"""
    g = orc.GDOracle(psf, kind="fista", dtype=tdt, initial_est=default_init(torch.from_numpy(p0).to(tdt)))
    g.set_data(y)
    # (t_k and the momentum factor in float32 whatever the dtype, like unrolled_fista.py:104 and unrolled_restated.restated)
    a, t = torch.abs(torch.as_tensor(alpha, dtype=tdt)), torch.abs(torch.as_tensor(tk, dtype=torch.float32))
    x = g.x
    xk_prev = x
    for i in range(a.shape[0]):
        g.x = x
        x = x - a[i] * g.grad()
        xk = torch.maximum(x, torch.zeros_like(x))
        x = xk + (t[i] - 1) / t[i + 1] * (xk - xk_prev)
        xk_prev = xk
    return torch.maximum(x, torch.zeros_like(x))[0].numpy().copy()


@functools.lru_cache(maxsize=None)
def fista_inputs(name):
    """the constructor's PSF p0 (another one than any frame's), per-frame PSFs, measurement, one schedule (0.8 x the smallest
    default step of all the PSFs) and the float64 / float32 oracle per frame; computed once, never written to"""
    H, W, C, _ = GD_CASES[name]["shape"]
    B = 3 if C == 1 else 2
    seed = 1100 + 10 * list(GD_CASES).index(name)
    p0 = orc.synthetic_psf(1, H, W, C, seed + 50)
    psfs = np.stack([orc.synthetic_psf(1, H, W, C, seed + b) for b in range(B)])
    data = np.random.default_rng(seed).random((B, 1, H, W, C), dtype=np.float32)
    alpha, tk = default_steps(torch.from_numpy(p0), GD_ITERS)
    for p in psfs:
        alpha = np.minimum(alpha, default_steps(torch.from_numpy(p), GD_ITERS)[0])
    alpha = (alpha * np.float32(0.8)).astype(np.float32)
    inp = SimpleNamespace(name=name, p0=p0, psfs=psfs, data=data, alpha=alpha, tk=tk, ref={})
    for tdt in (torch.float64, torch.float32):
        inp.ref[tdt] = [fista_oracle(p0, psfs[b], data[b, 0], alpha, tk, tdt) for b in range(B)]
    for b in range(B):
        y = rel(inp.ref[torch.float32][b], inp.ref[torch.float64][b])
        assert y <= YARDSTICK_MAX, f"FISTA {name} frame {b}: float32 oracle {y:.2e} from the float64 oracle: pick another seed"
    return inp


def fista_bound(dtype, ref32, ref64):
    return 100 * F64_TOL if dtype == "float64" else 4 * max(rel(ref32, ref64), 2e-6)


def fista_solver(name, dtype, backend, monkeypatch, frames=None):
    case, inp = GD_CASES[name], fista_inputs(name)
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **case["opts"]})
    tdt = tdt_of(dtype)
    sel = slice(None) if frames is None else frames
    rec = lpa.UnrolledFISTA(on(backend, inp.p0, tdt), n_iter=GD_ITERS, dtype=dtype)
    rec.set_parameters(alpha=inp.alpha, tk=inp.tk)
    return rec, on(backend, inp.data[sel], tdt), on(backend, inp.psfs[sel], tdt)


def fista_check(name, dtype, out, inp, bad, frames=None):
    frames = range(inp.data.shape[0]) if frames is None else frames
    for i, b in enumerate(frames):
        ref32, ref64 = inp.ref[torch.float32][b], inp.ref[torch.float64][b]
        r, bound = rel(out[i], ref64), fista_bound(dtype, ref32, ref64)
        print(f"FISTA {name} frame {b} {dtype}: rel {r:.3e} (bound {bound:.1e}, float32 oracle {rel(ref32, ref64):.3e})")
        if not r <= bound:
            bad.append((b, r, bound))


# --------------------------------------------------------------------------------------------------- CPU only --
def test_inputs_meet_their_conditions():
    """every case's float32 yardstick stays under YARDSTICK_MAX (asserted in ``inputs`` / ``fista_inputs``) and the PSFs of a
    case differ"""
    for name in CASES:
        inp = inputs(name)
        assert all(rel(inp.psfs[b], inp.psfs[0]) > 0.5 for b in range(1, inp.psfs.shape[0])), name
    for name in GD_CASES:
        inp = fista_inputs(name)
        assert all(rel(inp.psfs[b], inp.psfs[0]) > 0.5 for b in range(1, inp.psfs.shape[0])), name
        assert all(rel(p, inp.p0) > 0.5 for p in inp.psfs), name


def test_the_check_has_teeth():
    """the oracle alone, cases ``rt``: with the PSFs of frames 0 and 1 swapped, each of the two frames' float64 result moves
    by more than 100 x its float32 bound -- an engine that gave a frame another frame's PSF (or one PSF to all) cannot pass"""
    inp = inputs("rt")
    for b, other in ((0, 1), (1, 0)):
        ref64, ref32 = inp.ref[torch.float64][b][0].final, inp.ref[torch.float32][b][0].final
        moved = rel(oracle_frame(inp.psfs[other], inp.data[b, 0], inp.sched, torch.float64).final, ref64)
        bound = bound_of("float32", "final", ref32, ref64)
        print(f"ADMM frame {b} with the PSF of frame {other}: moves by {moved:.3e} (bound {bound:.1e})")
        assert moved >= 100 * bound, (b, moved, bound)
    inp = fista_inputs("rt")
    for b, other in ((0, 1), (1, 0)):
        ref64, ref32 = inp.ref[torch.float64][b], inp.ref[torch.float32][b]
        moved = rel(fista_oracle(inp.p0, inp.psfs[other], inp.data[b, 0], inp.alpha, inp.tk, torch.float64), ref64)
        bound = fista_bound("float32", ref32, ref64)
        print(f"FISTA frame {b} with the PSF of frame {other}: moves by {moved:.3e} (bound {bound:.1e})")
        assert moved >= 100 * bound, (b, moved, bound)


# ------------------------------------------------------------------------------- 1. against the oracle --
@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_unrolled_admm_forward(backend, monkeypatch, name, dtype):
    """``UnrolledADMM.forward(batch, psfs=P5)`` under no_grad, constructed from the PSF of frame 0, per frame and plane"""
    inp = inputs(name)
    rec, data, psfs = solver(name, dtype, backend, monkeypatch)
    with torch.no_grad():
        out = rec.forward(data, psfs=psfs)
    assert out.dtype == data.dtype and not out.requires_grad
    bad = []
    check_frames(name, dtype, out, inp, bad)
    assert not bad, bad


@pytest.mark.parametrize("name,dtype", [(c, d) for c, d in CASE_DTYPES if c in STATE_CASES])
def test_admm_states(backend, monkeypatch, name, dtype):
    """the eight ADMM states of every frame after N_ITER iterations in one call on a handle with per-frame PSFs"""
    inp = inputs(name)
    rec, data, psfs = solver(name, dtype, backend, monkeypatch)
    rec._set_psfs(psfs)
    rec.reset()
    rec._iterate(N_ITER)
    got = states_of(rec)
    bad = []
    for b in range(data.shape[0]):
        ref64, ref32 = inp.ref[torch.float64][b][0].states, inp.ref[torch.float32][b][0].states
        for key, _ in STATES:
            compare(f"{name} frame {b}", dtype, key, got[key][b:b + 1], ref32[key], ref64[key], bad)
    assert not bad, bad


@pytest.mark.parametrize("name,dtype", FISTA_CASE_DTYPES)
def test_unrolled_fista_forward(backend, monkeypatch, name, dtype):
    """``UnrolledFISTA.forward(batch, psfs=P5)`` under no_grad: the start value and the steps stay the constructor's"""
    inp = fista_inputs(name)
    rec, data, psfs = fista_solver(name, dtype, backend, monkeypatch)
    with torch.no_grad():
        out = rec.forward(data, psfs=psfs)
    assert GD_CASES[name]["info"] in rec._handle.plan_info(), rec._handle.plan_info()
    assert tuple(out.shape) == (data.shape[0], 1) + tuple(data.shape[2:4]) + (psfs.shape[-1],)
    bad = []
    fista_check(name, dtype, out.cpu().numpy(), inp, bad)
    assert not bad, bad


@pytest.mark.parametrize("name", ["mod", "seq_even", "split_reg"])
def test_apply_batch(backend, monkeypatch, name):
    """``ADMM.apply_batch(psfs=P5)`` with constant step sizes = per frame ``_set_psf(P5[b])``, ``set_data``, ``apply``: bit for
    bit where the two handles run one plan, and against the oracle"""
    inp = inputs(name)
    rec, data, psfs = solver(name, "float32", backend, monkeypatch, cls=lpa.ADMM)
    out = rec.apply_batch(n_iter=N_ITER, psfs=psfs).clone()
    info = rec._handle.plan_info()
    assert rec._psfs is psfs
    for b in range(data.shape[0]):
        one, d1, _ = solver(name, "float32", backend, monkeypatch, frames=slice(b, b + 1), cls=lpa.ADMM)
        one._set_psf(psfs[b])
        one.set_data(d1)
        want = one.apply(n_iter=N_ITER, disp_iter=None)
        o = orc.ADMMOracle(inp.psfs[b], dtype=torch.float64, **BASE)
        o.set_data(inp.data[b, 0])
        ref64 = o.apply(N_ITER).numpy()
        o32 = orc.ADMMOracle(inp.psfs[b], dtype=torch.float32, **BASE)
        o32.set_data(inp.data[b, 0])
        bound = 4 * max(rel(o32.apply(N_ITER).numpy(), ref64), 2e-6)
        r = rel(out[b], ref64)
        print(f"apply_batch {name} frame {b}: rel {r:.3e} (bound {bound:.1e}); against apply(): {rel(out[b], want):.3e}")
        assert r <= bound, (b, r, bound)
        if one._handle.plan_info() == info:
            assert torch.equal(out[b], want), rel(out[b], want)
        else:
            assert rel(want, ref64) <= bound


def test_apply_batch_with_a_denoiser_and_a_custom_psi(backend, monkeypatch):
    """the caller hooks go through the same spectral kernels: a denoiser (lpc_admm_pnp_begin / _end) and a custom psi
    (lpc_admm_psi_step, whose gram a later lpc_set_psf_batch leaves in place) with per-frame PSFs equal, bit for bit, the
    per-frame solvers with that PSF"""
    inp = inputs("mod")
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **CASES["mod"]["opts"]})
    data, psfs = on(backend, inp.data), on(backend, inp.psfs)
    # (a start away from zero, like tests/test_hooks_over_plans.py: the smoothing denoiser keeps zeros zero; it also puts
    # lpc_reset's H V_0 through the per-frame spectra)
    Hp, Wp = lpa.ADMM(psfs[0])._padded_shape[1:3]
    init = on(backend, np.random.default_rng(5).random((1, Hp, Wp, psfs.shape[-1]), dtype=np.float32) * np.float32(0.1))

    hooks = {"denoiser": dict(denoiser={"network": pnp_denoise, "noise_level": PNP_LEVEL, "use_dual": True}, **PNP),
             "custom psi": dict(psi=psi2, psi_adj=psi2_adj, psi_gram=psi2_gram, **PSI)}
    for tag, kw in hooks.items():
        rec = lpa.ADMM(psfs[0], initial_est=init, **kw)
        rec.set_data(data)
        out = rec.apply_batch(n_iter=3, psfs=psfs).clone()
        for b in range(data.shape[0]):
            one = lpa.ADMM(psfs[b], initial_est=init, **kw)
            one.set_data(data[b:b + 1])
            want = one.apply(n_iter=3, disp_iter=None)
            other = lpa.ADMM(psfs[1 - b], initial_est=init, **kw)
            other.set_data(data[b:b + 1])
            moved = rel(other.apply(n_iter=3, disp_iter=None), want)
            print(f"{tag} frame {b}: against the per-frame solver {rel(out[b], want):.3e}; another frame's PSF moves it by {moved:.3e}")
            assert float(want.abs().max()) > 0 and moved > 1e-2
            assert torch.equal(out[b], want), (tag, b, rel(out[b], want))


# ----------------------------------------------------------------------------------------------- 3. bitwise --
@pytest.mark.parametrize("name", NAMES + ["depth2"])
def test_equal_psfs_are_the_shared_run(backend, monkeypatch, name):
    """(a) ``psfs = stack([p] * B)``: the same kernels on the same values, only the addresses of H differ"""
    rec, data, psfs = solver(name, "float32", backend, monkeypatch)
    with torch.no_grad():
        shared = rec.forward(data).clone()
        same = rec.forward(data, psfs=torch.stack([psfs[0]] * data.shape[0]))
        assert rec._psfs is not None and float(shared.abs().max()) > 0
        assert torch.equal(same, shared), rel(same, shared)
        assert torch.equal(rec.forward(data, psfs=psfs[0]), shared)        # ... and back


@pytest.mark.parametrize("name", list(GD_CASES))
def test_equal_psfs_are_the_shared_run_fista(backend, monkeypatch, name):
    rec, data, psfs = fista_solver(name, "float32", backend, monkeypatch)
    with torch.no_grad():
        shared = rec.forward(data, psfs=psfs[0]).clone()
        same = rec.forward(data, psfs=torch.stack([psfs[0]] * data.shape[0]))
    assert float(shared.abs().max()) > 0 and torch.equal(same, shared), rel(same, shared)


@pytest.mark.parametrize("name", NAMES)
def test_a_frame_of_the_batch_is_the_single_frame_run(backend, monkeypatch, name):
    """(b) frame b of the per-frame batch against ``forward(batch[b:b+1], psfs=P5[b])`` on a solver of one frame: bit for bit
    where ``plan_info()`` of the two handles agrees, else both under the bound of 1."""
    inp = inputs(name)
    rec, data, psfs = solver(name, "float32", backend, monkeypatch)
    with torch.no_grad():
        out = rec.forward(data, psfs=psfs).clone()
    info = rec._handle.plan_info()
    for b in range(data.shape[0]):
        one, d1, p1 = solver(name, "float32", backend, monkeypatch, frames=slice(b, b + 1))
        with torch.no_grad():
            want = one.forward(d1, psfs=p1[0])
        if one._handle.plan_info() == info:
            assert torch.equal(out[b], want[0]), (b, rel(out[b], want[0]))
        else:
            bad = []
            check_frames(name, "float32", want, inp, bad, frames=[b])
            check_frames(name, "float32", out[b:b + 1], inp, bad, frames=[b])
            assert not bad, bad


@pytest.mark.parametrize("name", ["mod", "split_mod", "seq_odd", "seq_even", "pair"])
def test_per_frame_shared_per_frame(backend, monkeypatch, name):
    """(c) per-frame -> one PSF -> per-frame again on ONE solver: the first result again, bit for bit, and the one-PSF run in
    between is a fresh solver's; a later ``forward(batch)`` without ``psfs`` keeps the per-frame PSFs current"""
    rec, data, psfs = solver(name, "float32", backend, monkeypatch)
    with torch.no_grad():
        first = rec.forward(data, psfs=psfs).clone()
        again = rec.forward(data).clone()
        shared = rec.forward(data, psfs=psfs[1]).clone()
        assert rec._psfs is None
        third = rec.forward(data, psfs=psfs).clone()
        fresh, _, _ = solver(name, "float32", backend, monkeypatch, psf_frame=1)
        want_shared = fresh.forward(data)
    assert torch.equal(again, first) and torch.equal(third, first), (rel(again, first), rel(third, first))
    assert torch.equal(shared, want_shared) and rel(shared[0], first[0]) > 1e-2


def test_a_new_batch_size_needs_new_psfs(backend, monkeypatch):
    rec, data, psfs = solver("rt", "float32", backend, monkeypatch)
    with torch.no_grad():
        rec.forward(data, psfs=psfs)
        with pytest.raises(ValueError, match="per-frame"):
            rec.forward(data[:1])
        out = rec.forward(data[:1], psfs=psfs[0])
    assert out.shape[0] == 1 and rec._psfs is None


# ------------------------------------------------------------------------------------- 4. the reference itself --
FIXTURES = ["19x27x1_b3", "16x20x3_b2"]
# (the gradient-descent family takes compile-time plans for half-length rows: unrolled_restated.PLANS["module"])
PIN_PLANS = {"rt": {"admm": {}, "fista": {}}, "mod": {"admm": {"jit_min_points": 0}, "fista": {"jit_min_points": 0, "rows_half": 1}}}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("plan", list(PIN_PLANS))
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("kind", ["admm", "fista"])
def test_against_the_reference(backend, monkeypatch, kind, fixture, plan, dtype):
    """the reference's own ``forward(batch, psfs=P5)`` (gen_per_frame_psf.py), its float32 run the yardstick.  The float64
    engine against the reference's float64 run: 1e-7 for ADMM, the bound tests/test_unrolled_admm_grad.py and
    tests/test_unrolled_admm_psf_grad.py hold ``out`` to against the reference's float64 ``out64`` (the reference keeps
    float32 constants in its float64 run); 100 * F64_TOL for FISTA, like tests/test_psf_swap.py's fixture"""
    g = np.load(os.path.join(GOLDEN, f"unrolled_{kind}_psfs5d_{fixture}.npz"))
    n, tdt = int(g["n_iter"]), tdt_of(dtype)
    assert n == 4 and g["psfs"].shape[1:] == g["psf"].shape and g["psfs"].shape[0] == g["data"].shape[0]
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **PIN_PLANS[plan][kind]})
    if kind == "admm":
        rec = lpa.UnrolledADMM(on(backend, g["psf"], tdt), dtype=dtype, n_iter=n, **BASE)
        rec.set_parameters(**{k: g[k] for k in BASE})
    else:
        rec = lpa.UnrolledFISTA(on(backend, g["psf"], tdt), n_iter=n, dtype=dtype)
        rec.set_parameters(alpha=g["alpha"], tk=g["tk"])
    with torch.no_grad():
        out = rec.forward(on(backend, g["data"], tdt), psfs=on(backend, g["psfs"], tdt)).cpu().numpy()
    assert ("plan module" in rec._handle.plan_info()) == (plan == "mod"), rec._handle.plan_info()
    bad = []
    for b in range(out.shape[0]):
        y = rel(g["out32"][b], g["out64"][b])
        assert y <= YARDSTICK_MAX
        bound = (1e-7 if kind == "admm" else 100 * F64_TOL) if dtype == "float64" else 4 * max(y, 2e-6)
        r = rel(out[b], g["out64"][b])
        print(f"{kind} {fixture} {plan} {dtype} frame {b}: rel {r:.3e} (bound {bound:.1e}, float32 reference {y:.3e})")
        if not r <= bound:
            bad.append((b, r, bound))
    assert not bad, bad


# ------------------------------------------------------------------------------------------- 5. the operator --
def _fft_operator(psf, x, pad, adjoint, norm, return_fft):
    """rfft_convolve.py:133-223 in float64 for one PSF (D, H, W, C) and one item x (D|1, Hx, Wx, C|1)"""
    p, v = torch.from_numpy(psf).double(), torch.from_numpy(x).double()
    D, H, W, C = p.shape
    g = orc.Geometry(H, W)
    Hs = torch.fft.rfft2(g.pad(p), norm=norm, dim=(-3, -2))
    X = torch.fft.rfft2(g.pad(v) if pad else v, dim=(-3, -2)) * (Hs.conj() if adjoint else Hs)
    if return_fft:
        return X.numpy()
    y = torch.fft.ifftshift(torch.fft.irfft2(X, dim=(-3, -2), s=tuple(g.pad(p).shape[-3:-1])), dim=(-3, -2))
    return (g.crop(y) if pad else y).numpy()


OPERATOR_CASES = {"rt": ((21, 13, 1, 3, 1), {}), "rgb_depth2": ((24, 32, 3, 2, 2), {}),
                  "split": ((48, 20, 1, 3, 1), {"tile_budget": 512, "col_t": 4, "split_n2": 12}),
                  "split_reg": ((48, 20, 1, 3, 1), {"tile_budget": 512, "col_t": 4, "split_n2": 24}),
                  "module": ((24, 32, 3, 2, 1), {"jit_min_points": 0, "rows_half": 1})}


@pytest.mark.parametrize("pad", [True, False], ids=["pad", "nopad"])
@pytest.mark.parametrize("name", list(OPERATOR_CASES))
def test_operator(backend, name, pad):
    """``RealFFTConvolve2D(P5)``: convolve / deconvolve / return_fft, item b against PSF b, at the operator tests' 2e-6"""
    (H, W, C, B, D), opts = OPERATOR_CASES[name]
    psfs = np.stack([orc.synthetic_psf(D, H, W, C, 1500 + b) for b in range(B)])
    cv = lpa.RealFFTConvolve2D(psfs, pad=pad, norm="backward", engine_options=opts)
    Hp, Wp = cv._padded_shape[1:3]
    assert cv._padded_shape == [D, Hp, Wp, C] and len(cv._psf_shape) == 5
    x = np.random.default_rng(1500).standard_normal((B, 1) + ((H, W) if pad else (Hp, Wp)) + (C,)).astype(np.float32)
    if pad:
        xp = cv._pad(x)
        assert xp.shape == (B, D, Hp, Wp, C) and np.array_equal(cv._crop(xp), np.broadcast_to(x, (B, D, H, W, C)))
    for adjoint, fn in ((False, cv.convolve), (True, cv.deconvolve)):
        for return_fft in (False, True):
            got = fn(x, return_fft=return_fft)
            for b in range(B):
                want = _fft_operator(psfs[b], x[b], pad, adjoint, "backward", return_fft)
                assert got[b].shape == want.shape, (got.shape, want.shape)
                r = float(np.abs(got[b] - want).max() / np.abs(want).max())
                assert r <= 2e-6, (name, pad, adjoint, return_fft, b, r)
            other = _fft_operator(psfs[1], x[0], pad, adjoint, "backward", return_fft)
            assert float(np.abs(got[0] - other).max() / np.abs(other).max()) > 1e-2       # (the PSFs are told apart)
    with pytest.raises(ValueError, match="per-frame"):
        cv.convolve(x[:1])


def test_reconstruction_error(backend, monkeypatch):
    """``reconstruction_error`` of a solver that holds per-frame PSFs, and with an explicit 5-D ``psfs``, against the oracle
    per frame at tests/test_metrics.py's tolerance"""
    inp = inputs("rt")
    rec, data, psfs = solver("rt", "float32", backend, monkeypatch, cls=lpa.ADMM)
    pred = rec.apply_batch(n_iter=3, psfs=psfs)
    own = rec.reconstruction_error()
    explicit = rec.reconstruction_error(prediction=pred, lensless=data, psfs=psfs)
    for b in range(data.shape[0]):
        conv = orc.ConvolverOracle(inp.psfs[b], dtype=torch.float64, pad=True, norm="backward")
        want = orc.reconstruction_error(conv, pred[b:b + 1].cpu().double(), torch.from_numpy(inp.data[b:b + 1]).double())
        wrong = orc.reconstruction_error(orc.ConvolverOracle(inp.psfs[1 - b], dtype=torch.float64, pad=True, norm="backward"),
                                         pred[b:b + 1].cpu().double(), torch.from_numpy(inp.data[b:b + 1]).double())
        assert rel(own[b:b + 1], want) <= 2e-5 and rel(explicit[b:b + 1], want) <= 2e-5, (b, own[b], explicit[b], want)
        assert rel(wrong, want) > 1e-2


# ------------------------------------------------------------------------------------ 6. refusals and the ABI --
def test_a_recording_forward_refuses(backend, monkeypatch):
    rec, data, psfs = solver("rt", "float32", backend, monkeypatch)
    with pytest.raises(NotImplementedError, match="per-frame"):
        rec.forward(data, psfs=psfs)                       # the parameters require a gradient
    with torch.no_grad():
        out = rec.forward(data, psfs=psfs)
    with pytest.raises(NotImplementedError, match="per-frame"):
        rec.forward(data)                                  # ... and the per-frame PSFs are still current
    assert not out.requires_grad
    rec.forward(data, psfs=psfs[0]).sum().backward()       # one PSF for the batch trains as before
    assert rec._mu1_p.grad is not None
    fis, fdata, fpsfs = fista_solver("rt", "float32", backend, monkeypatch)
    with pytest.raises(NotImplementedError, match="per-frame"):
        fis.forward(fdata, psfs=fpsfs)
    for cls in (lpa.FISTA, lpa.GradientDescent, lpa.NesterovGradientDescent):
        plain = cls(fpsfs[0])
        plain.set_data(fdata)
        with pytest.raises(NotImplementedError, match="per-frame"):
            plain.apply_batch(n_iter=1, psfs=fpsfs)
    with pytest.raises(NotImplementedError, match="background"):
        rec.forward(data, psfs=psfs, background=data)


def test_the_handle_refuses_gradients(backend, monkeypatch):
    """lpc_admm_record / lpc_fista_record and the backwards on a handle with per-frame PSFs; lpc_set_psf lifts it"""
    rec, data, psfs = solver("rt", "float32", backend, monkeypatch)
    fis, fdata, fpsfs = fista_solver("rt", "float32", backend, monkeypatch)
    with torch.no_grad():
        rec.forward(data, psfs=psfs)
        fis.forward(fdata, psfs=fpsfs)
    g = torch.zeros(64, dtype=torch.float32, device=backend.device)
    p = g.data_ptr()
    for h, record, backward in ((rec._handle, "admm_record", lambda h: h.admm_backward(p, None, p, p, p, p)),
                                (fis._handle, "fista_record", lambda h: h.fista_backward(p, None, p, p))):
        with pytest.raises(_native.NativeError, match="per-frame"):
            getattr(h, record)(1)
        getattr(h, record)(0)                            # (switching it off is no gradient)
        with pytest.raises(_native.NativeError, match="per-frame"):
            backward(h)
    rec._handle.set_psf(rec._psf_dev.data_ptr())
    rec._handle.admm_record(1)
    with pytest.raises(_native.NativeError, match="per-frame"):
        rec._handle.set_psf_batch(psfs.contiguous().data_ptr())      # a recording handle takes none
    rec._handle.admm_record(0)


def test_a_plain_gradient_descent_handle_refuses(backend):
    lib = backend.lib
    psfs = on(backend, np.stack([orc.synthetic_psf(1, 10, 12, 3, 5 + b) for b in range(2)]))
    for algo in (_native.ALGO_GD, _native.ALGO_NESTEROV, _native.ALGO_FISTA):
        h = lib.create(algo=algo, height=10, width=12, channels=3, batch=2)
        with pytest.raises(_native.NativeError, match="per-frame"):
            h.set_psf_batch(psfs.data_ptr())
        h.close()


@pytest.mark.parametrize("name", ["rt", "pair", "seq_odd", "seq_even"])
def test_workspace_bytes(backend, monkeypatch, name):
    """lpc_set_psf_batch gives the D C-plane buffers back and takes B D C planes, once: include/lpc.h's formula"""
    rec, data, psfs = solver(name, "float32", backend, monkeypatch)
    h = rec._handle
    (H, W, C, B), info = CASES[name]["shape"], h.plan_info()
    before = h.workspace_bytes()
    with torch.no_grad():
        rec.forward(data, psfs=psfs)
    cpitch = (h.Wp // 2 + 1 + 15) // 16 * 16
    spectrum, frame = 2 * 4 * ((h.Hp + 1) & ~1) * cpitch, 4 * H * W
    planes = 1.0 + ("pair-line spectra" in info) + (0 if "one spectrum at a time" not in info else 1.5 if info.endswith("pLr") else 2.5)
    assert h.workspace_bytes() == before + (B - 1) * C * (planes * spectrum + frame), (before, h.workspace_bytes(), planes)
    grown = h.workspace_bytes()
    with torch.no_grad():
        rec.forward(data, psfs=psfs[0])
        rec.forward(data, psfs=psfs)
    assert h is rec._handle and h.workspace_bytes() == grown          # (they do not shrink, nothing is allocated twice)
    model = h.model_bytes()
    rec._handle.set_psf(rec._psf_dev.data_ptr())
    assert model == h.model_bytes() + 2 * 4 * h.Hp * (h.Wp // 2 + 1) * B * C   # the model counts a frame's own H


def test_the_abi_exports_the_entry(backend):
    assert isinstance(backend.lib.dll.lpc_set_psf_batch, ctypes._CFuncPtr)
