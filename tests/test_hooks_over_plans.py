"""
The paths where the CALLER'S code runs inside every iteration, over the launch plans the planner can choose, against the CPU
oracle in float64, through the public API, on the SIMT emulator ('emu') and on the MI355X ('hip', -m gpu):

  * ``GradientDescent / NesterovGradientDescent / FISTA(psf, proj=fn)`` and ``denoiser={...}`` on them: lpc_iterate_begin /
    lpc_iterate_end, the ``split`` branch of gd_update_val, k_gd_post -- also mixed with fused iterations on one handle (the
    ``fwd_done`` row-spectrum cache of the fused-forward update kernel, crossed in both directions);
  * ``ADMM(psf, denoiser={..., "use_dual": b})``: lpc_admm_pnp_begin / _end, k_pnp_input, k_pnp_pre, k_pnp_post;
  * ``ADMM(psf, psi=, psi_adj=, psi_gram=)``: lpc_set_psi_gram, k_permute_spectrum_rows, lpc_admm_psi_step;
  * ``UnrolledFISTA(psf, proj=fn)`` without gradients: split iterations on a step schedule.

tests/test_pnp_hook.py and tests/test_custom_psi.py pin these to the reference's own outputs on frames of 24 x 32 and less
(run-time plans, one frame, depth 1); here every case sits on another launch plan and asserts its marker in ``plan_info()``.

References: ``GDOracle(proj=)``, ``ADMMOracle(denoiser=)``, ``ADMMOracle(psi=)`` in float64 (pinned to the reference by
tests/test_oracle_golden.py, tests/test_custom_psi.py) and ``unrolled_restated.restated(proj=)``; yardstick: the same in float32,
never the engine.  A gradient-descent solver of depth D is compared with the oracle of depth D -- its step and start value
are taken over all planes (gd.py:100-112), a depth-1 oracle per plane would be another problem; ADMM runs D independent
problems and is compared plane by plane with the depth-1 oracle.

Bounds (the rule of tests/test_unrolled_admm_sweep.py; max-norm over whole arrays, relative to the max of the float64 array):
  float32 engine:  rel(q, oracle64) <= 4 * max(rel(oracle32, oracle64), 2e-6) for every quantity q;
  float64 engine:  F64_TOL = 1e-11, x 100 for xi, eta and rho;
  same engine, another plan (hook == fused, fused and split mixed):  2e-6.
test_the_check_has_teeth shows on the oracle alone that each hook matters: done in the wrong way it moves the result by over
100 x the float32 bound.

The 135 x 240 frame gets ``tile_budget=4320`` on top of the (empty) option set of ``c1``: its middle takes 16-column tiles by
default, and pair-line spectra -- the marker the frame is here for -- exist for 8-column tiles only.

Inputs: ``synthetic_psf(D, H, W, C, seed)``, measurements ``0.5 * rng.random`` (the 0.01 of ``shrink`` is then over 1 % of the
estimate), the initial estimate ``0.2 * rng.random ** 6`` on the padded frame (sparse: with a dense one the use_dual
trajectory drives W to an array of zeros by the fifth iteration on the widest frame).

The comparison that came closest to its bound, over every case, frame, plane, state and call (float32 engine: distance | its
bound | the float32 oracle's own distance; float64 engine: distance, bound 1e-11):
  family                       emulator                                   MI355X
  GD hooks                     7.7e-7 | 8.0e-6 | 7.6e-7;  1.2e-15         7.2e-7 | 8.0e-6 | 6.1e-7;  1.1e-15
  plug-and-play ADMM           1.6e-6 | 8.0e-6 | 2.0e-6;  2.8e-14         1.4e-6 | 8.2e-6 | 2.0e-6;  3.3e-14
  custom prior                 8.4e-7 | 8.0e-6 | 1.2e-6                   8.4e-7 | 8.0e-6 | 1.1e-6
  unrolled FISTA with proj     3.6e-7 | 8.0e-6 | 4.7e-7;  9.3e-16         3.9e-7 | 8.0e-6 | 3.7e-7;  7.8e-16
  hook == fused, mixed calls   5.7e-7 (bound 2e-6)                        4.5e-7 (bound 2e-6)
"""
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
from unrolled_restated import F64_TOL, default_steps, rel, restated

SAME_ENGINE = 2e-6                   # the suite's bound for "same engine, another plan"
MOD = {"jit_min_points": 0}
# name: PSF shape (D, H, W, C), launch-plan options, what plan_info() of a GD-family / an ADMM handle must hold (``f32``: of the
# float32 build only -- the float64 build has neither pair lines nor the sequential middle nor the second-form rows)
CASES = {
    "half_split": dict(shape=(1, 12, 1014, 1), opts={"rows_half": 1, "tile_budget": 256, **MOD},
                       gd=["half-length 1024 [static", "split"],
                       admm=["X half inside the forward rows", "H V row transforms skipped"]),
    "c1": dict(shape=(1, 270, 480, 1), opts={}, gd=["half-length 480 [static"],
               admm=["paired 960 [static", "three launches per iteration"], admm_f32=["pair-line spectra"]),
    "rows8192": dict(shape=(1, 3, 4096, 1), opts=MOD, gd=[], gd_f32=["second form"], admm=["half-length 4096 [static"]),
    "fourstep": dict(shape=(1, 48, 20, 3), opts={"tile_budget": 512, "col_t": 4, "split_n2": 12},
                     gd=["8 x 12 split", "run-time plans"], admm=["8 x 12 split", "run-time plans"]),
    # padded height 45, the window starts on row 11
    "pairline_odd": dict(shape=(1, 23, 40, 3), opts={"mid_seq": 1, "tile_budget": 720, **MOD}, gd=["padded 45x80"],
                         admm=["padded 45x80"], admm_f32=["one spectrum at a time, pair-line spectra"]),
    "oddodd": dict(shape=(1, 21, 13, 1), opts={}, gd=["padded 45x25"], admm=["padded 45x25"]),
    "v2_depth2": dict(shape=(2, 5, 512, 3), opts=MOD, gd=[], gd_f32=["second form, 64 lanes"], admm=None),     # GD family only
    "k1rows": dict(shape=(1, 13, 40, 1), opts={**MOD, "k1_rows": 1}, gd=[],
                   admm=["three launches per iteration", "xi half-applied"]),
    # batch / depth / float64 only
    "f135": dict(shape=(1, 135, 240, 1), opts={"tile_budget": 4320}, gd=["half-length 240 [static"],
                 admm=["three launches per iteration"], admm_f32=["pair-line spectra"]),
}
for _i, _c in enumerate(CASES.values()):
    _c["seed"] = 500 + _i
SWEEP = [c for c in CASES if c != "f135"]
DEPTH1 = [c for c in SWEEP if CASES[c]["admm"] is not None]
BATCH_CASES = ["half_split", "fourstep", "pairline_odd", "f135"]
MIXED_CASES = ["rows8192", "v2_depth2", "half_split"]
GD = (("vanilla", "GradientDescent"), ("nesterov", "NesterovGradientDescent"), ("fista", "FISTA"))
PNP = dict(mu1=1e-4, mu2=1e-3, mu3=1e-3)
PNP_LEVEL = 12.0
# (step sizes picked on the oracle: with tau / mu2 = 0.02 half to nine tenths of U pass the soft threshold on every case, after 3
# and after 5 iterations -- the step sizes of tests/golden/custom_psi_admm.npz leave U an array of zeros at tau = 2e-4)
PSI = dict(mu1=1e-2, mu2=1e-2, mu3=1e-2, tau=2e-4)
ADMM_STATES = (("V", "_image_est"), ("U", "_U"), ("X", "_X"), ("W", "_W"), ("xi", "_xi"), ("eta", "_eta"), ("rho", "_rho"))
F64, F32 = torch.float64, torch.float32
WORST = {}                          # family -> dtype -> (rel, bound, float32 oracle) of the worst rel / bound seen in this run


def shrink(x):                      # not idempotent: the read-out projects again, and that shows
    return torch.clamp(x - 0.01, min=0)


def plain_non_neg(x):               # non_neg in disguise: another callable, so the iterations are split
    return torch.clamp(x, min=0)


def psi2_gram64(shape):
    return psi2_gram(shape, torch.float64)


def tdt_of(dtype):
    return F64 if dtype == "float64" else F32


@functools.lru_cache(maxsize=None)
def inputs(name, depth=None):
    """PSF(s), two measurements and a non-zero initial estimate on the padded frame of a case (``depth``: another depth than
    the table's); never written to"""
    case = CASES[name]
    D, H, W, C = case["shape"]
    D = depth or D
    rng = np.random.default_rng(case["seed"] + 50 * D)
    geom = orc.Geometry(H, W)
    return SimpleNamespace(name=name, D=D, H=H, W=W, C=C, Hp=geom.hp, Wp=geom.wp,
                           psf=orc.synthetic_psf(D, H, W, C, case["seed"]),
                           psf_other=orc.synthetic_psf(D, H, W, C, case["seed"] + 1000),
                           data=rng.random((2, 1, H, W, C), dtype=np.float32) * np.float32(0.5),
                           init=(0.2 * rng.random((D, geom.hp, geom.wp, C), dtype=np.float32) ** 6).astype(np.float32))


def npy(t):
    return t.detach().cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.array(t)


# ------------------------------------------------------------------------------------------ the references --
@functools.lru_cache(maxsize=None)
def gd_ref(name, kind, depth=None, calls=(3, 2), proj=shrink, frames=(0,)):
    """{dtype: [per frame: {"final0", "state0", "final1", "state1"}]}: image and un-projected state after each of the two calls"""
    inp, out = inputs(name, depth), {}
    for tdt in (F64, F32):
        out[tdt] = []
        for b in frames:
            o = orc.GDOracle(inp.psf, kind=kind, dtype=tdt, proj=proj)
            o.set_data(inp.data[b, 0])
            r = {}
            for i, n in enumerate(calls):
                r[f"final{i}"] = npy(o.apply(n, reset=i == 0))
                r[f"state{i}"] = npy(o.x[0])
            out[tdt].append(r)
    return out


def admm_oracle(inp, tdt, mode, plane=0, other=False, wrong=False):
    """``mode``: "plain" / "dual" (plug-and-play) or "psi" (the custom prior); ``wrong``: the hook done in the wrong way
    (test_the_check_has_teeth): the denoiser fed V where U + eta / mu2 is due, the finite-difference gram for psi2's"""
    psf = (inp.psf_other if other else inp.psf)[plane:plane + 1]
    if mode == "psi":
        gram = psi2_gram64 if tdt == F64 else psi2_gram
        if wrong:
            gram = lambda shape: orc.finite_diff_gram([int(v) for v in shape], tdt)  # noqa: E731
        return orc.ADMMOracle(psf, dtype=tdt, psi=(psi2, psi2_adj, gram), **PSI)
    box = []
    fn = (lambda x, level: pnp_denoise(box[0].V, level)) if wrong else pnp_denoise
    o = orc.ADMMOracle(psf, dtype=tdt, denoiser=(fn, PNP_LEVEL, mode == "dual"), initial_est=inp.init[plane:plane + 1].copy(),
                       **PNP)
    box.append(o)
    return o


def admm_run(o, data, calls):
    r = {}
    for i, n in enumerate(calls):
        r[f"final{i}"] = npy(o.apply(n, reset=i == 0))
    for key, _ in ADMM_STATES:
        r[key] = npy(getattr(o, key)[0, 0])
    return r


@functools.lru_cache(maxsize=None)
def admm_ref(name, mode, depth=None, calls=(3, 2), frames=(0,), other=False):
    """{dtype: {(frame, plane): {"final0", "final1", the seven states after the last call on the padded frame}}}"""
    inp = inputs(name, depth)
    out = {}
    for tdt in (F64, F32):
        out[tdt] = {}
        for b in frames:
            for d in range(inp.D):
                o = admm_oracle(inp, tdt, mode, plane=d, other=other)
                o.set_data(inp.data[b, 0])
                out[tdt][(b, d)] = admm_run(o, inp.data[b, 0], calls)
    return out


# ------------------------------------------------------------------------------------------------ comparing --
def bound_of(dtype, key, ref32, ref64):
    if dtype == "float64":
        return F64_TOL * (100 if key in ("xi", "eta", "rho") else 1)
    return 4 * max(rel(ref32, ref64), 2e-6)


def compare(family, tag, dtype, key, got, ref32, ref64, bad):
    got = npy(got)
    assert float(np.abs(ref64).max()) > 0, (tag, key)
    assert tuple(got.shape) == ref64.shape, (tag, key, tuple(got.shape), ref64.shape)
    r, y, bound = rel(got, ref64), rel(ref32, ref64), bound_of(dtype, key, ref32, ref64)
    print(f"{tag} {dtype} {key}: rel {r:.3e} (bound {bound:.1e}, float32 oracle {y:.3e})")
    worst = WORST.setdefault(family, {})
    if dtype not in worst or r / bound > worst[dtype][0] / worst[dtype][1]:
        worst[dtype] = (r, bound, y)
    if not r <= bound:
        bad.append((tag, key, r, bound))


def compare_admm(family, tag, dtype, rec, refs, b, d, bad, eta_is_zero=False):
    for key, attr in ADMM_STATES:
        got = npy(getattr(rec, attr))[b, d]
        if key == "eta" and eta_is_zero:        # use_dual=False never touches eta (admm.py:326): zeros, not "close to" zeros
            assert not refs[F64][(b, d)][key].any() and not got.any(), (tag, key)
            continue
        compare(family, tag, dtype, key, got, refs[F32][(b, d)][key], refs[F64][(b, d)][key], bad)


def report(family):
    for dtype, (r, bound, y) in sorted(WORST.get(family, {}).items()):
        print(f"worst so far, {family}, {dtype}: rel {r:.3e} (bound {bound:.1e}, float32 oracle {y:.3e})")


def set_plan(monkeypatch, name):
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **CASES[name]["opts"]})


def check_plan(rec, name, dtype, which):
    info, case = rec._handle.plan_info(), CASES[name]
    for marker in case[which] + (case.get(which + "_f32", []) if dtype == "float32" else []):
        assert marker in info, (name, which, marker, info)


def on_device(a, backend, dtype="float32"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=backend.device, dtype=tdt_of(dtype))


# ------------------------------------------------------------------------------------------------- CPU only --
def unrolled_inputs(name):
    """(psf, batch, alpha, tk, n) of the two unrolled cases: the 24 x 32 x 3, B = 3 fixture with its per-iteration alpha and
    perturbed t_k, and ``rows8192`` (second-form rows) with the default steps x another factor per iteration"""
    if name == "golden":
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "unrolled_fista_grad_24x32x3_b3.npz"))
        return g["psf"], g["data"], g["alpha"], g["tk"], int(g["n_iter"])
    inp, n = inputs(name), 4
    alpha, tk = default_steps(torch.from_numpy(inp.psf), n)
    alpha = (alpha * np.asarray([1.0, 0.6, 1.4, 0.8], dtype=np.float32)[:, None]).astype(np.float32)
    tk = (tk * np.asarray([1.0, 1.1, 0.9, 1.2, 0.95], dtype=np.float32)).astype(np.float32)
    return inp.psf, inp.data, alpha, tk, n


@functools.lru_cache(maxsize=None)
def unrolled_ref(name, proj=shrink):
    psf, data, alpha, tk, n = unrolled_inputs(name)
    return {tdt: npy(restated(torch.from_numpy(psf), torch.from_numpy(data), torch.from_numpy(alpha), torch.from_numpy(tk), n,
                              dtype=tdt, proj=proj)[0]) for tdt in (F64, F32)}


def test_the_check_has_teeth():
    """on the oracle alone, every case: each hook done in the wrong way -- ``proj`` replaced by plain non-negativity, the
    denoiser fed V where U + eta / mu2 is due, the finite-difference gram in place of psi2's -- moves the float64 result by at
    least 100 x the float32 bound; every reference array compared is no array of zeros (eta without use_dual excepted: zeros
    by construction, compared as such); use_dual=True has no data term (``_step_pnp``): without an initial estimate its
    trajectory is identically zero and with one it is the same for every frame -- so every such case carries an initial
    estimate, and the data wiring is judged on use_dual=False, where two frames do differ"""
    weak = []

    def must_move(tag, wrong64, ref32, ref64, what):
        bound, moved = bound_of("float32", "", ref32, ref64), rel(wrong64, ref64)
        print(f"{tag}: {what} moves it by {moved:.3e} = {moved / bound:.0f} x the float32 bound {bound:.1e}")
        if not moved >= 100 * bound:
            weak.append((tag, moved, bound))

    for name in SWEEP:
        for kind, _ in GD:
            ref, wrong = gd_ref(name, kind), gd_ref(name, kind, proj=plain_non_neg)
            for key, a64 in ref[F64][0].items():
                assert float(np.abs(a64).max()) > 0, (name, kind, key)
                must_move(f"{name} {kind} {key}", wrong[F64][0][key], ref[F32][0][key], a64, "plain non-negativity")
    for name in DEPTH1 + ["f135"]:
        inp = inputs(name)
        for mode in ("plain", "dual", "psi"):
            ref = admm_ref(name, mode)
            for key, a64 in ref[F64][(0, 0)].items():
                if mode == "plain" and key == "eta":
                    assert not a64.any()
                elif not float(np.abs(a64).max()) > 0:
                    weak.append((name, mode, key, "an array of zeros"))
            if mode == "plain":
                continue
            o = admm_oracle(inp, F64, mode, wrong=True)
            o.set_data(inp.data[0, 0])
            wrong = admm_run(o, inp.data[0, 0], (3, 2))
            for key in ("final0", "final1"):
                must_move(f"{name} {mode} {key}", wrong[key], ref[F32][(0, 0)][key], ref[F64][(0, 0)][key],
                          "V as the denoiser's input" if mode == "dual" else "the finite-difference gram")
        for kw in ({}, {"calls": (3,), "other": True}):                           # the soft threshold is neither off nor all
            live = float((admm_ref(name, "psi", **kw)[F64][(0, 0)]["U"] != 0).mean())
            print(f"{name} psi {kw}: {100 * live:.1f} % of U non-zero")
            assert 0.05 <= live <= 0.95, (name, live)
        # use_dual=True: no data term
        o = orc.ADMMOracle(inp.psf, dtype=F64, denoiser=(pnp_denoise, PNP_LEVEL, True), **PNP)
        o.set_data(inp.data[0, 0])
        assert not o.apply(3).any()
        two = admm_ref(name, "dual", frames=(0, 1))[F64]
        assert np.array_equal(two[(0, 0)]["final1"], two[(1, 0)]["final1"])
        two = admm_ref(name, "plain", frames=(0, 1))
        must_move(f"{name} plain final1", two[F64][(0, 0)]["final1"], two[F32][(1, 0)]["final1"], two[F64][(1, 0)]["final1"],
                  "the other frame's measurement")
    for name in ("golden", "rows8192"):
        ref, wrong = unrolled_ref(name), unrolled_ref(name, proj=plain_non_neg)
        assert float(np.abs(ref[F64]).max()) > 0
        must_move(f"unrolled {name}", wrong[F64], ref[F32], ref[F64], "plain non-negativity")
    assert not weak, weak


# ----------------------------------------------------------------------------------------- emulator and card --
@pytest.mark.parametrize("name", SWEEP)
def test_gd_custom_projection(backend, monkeypatch, name):
    """all three classes with ``proj=shrink``: apply(3), apply(2, reset=False); the returned image (projected once more on
    read-out, gd.py:136-140) and ``_image_est``, the un-projected state, after either call"""
    inp, bad = inputs(name), []
    set_plan(monkeypatch, name)
    for kind, cls in GD:
        ref = gd_ref(name, kind)
        rec = getattr(lpa, cls)(on_device(inp.psf, backend), proj=shrink)
        check_plan(rec, name, "float32", "gd")
        rec.set_data(on_device(inp.data[0, 0], backend))
        for i, n in enumerate((3, 2)):
            out = rec.apply(n_iter=n, disp_iter=None, reset=i == 0)
            for key, got in ((f"final{i}", out), (f"state{i}", rec._image_est[0])):
                compare("GD hooks", f"{name} {kind}", "float32", key, got, ref[F32][0][key], ref[F64][0][key], bad)
    report("GD hooks")
    assert not bad, bad


def test_fista_denoiser_is_called_on_the_whole_estimate(backend, monkeypatch):
    """``denoiser={"network": fn, "noise_level": 7.0}`` on ``v2_depth2``: n_iter + 1 calls (the read-out is one), each with
    the (B, D, H, W, C) estimate and the level; against the oracle with the same function as its projection"""
    name = "v2_depth2"
    inp, seen, bad = inputs(name), [], []

    def denoise(x, noise_level):
        seen.append((tuple(x.shape), float(noise_level)))
        return torch.clamp(x, min=0) * (1.0 - noise_level / 100.0)

    set_plan(monkeypatch, name)
    rec = lpa.FISTA(on_device(inp.psf, backend), denoiser={"network": denoise, "noise_level": 7.0})
    check_plan(rec, name, "float32", "gd")
    rec.set_data(on_device(inp.data[0, 0], backend))
    out = rec.apply(n_iter=4, disp_iter=None)
    assert seen == [((1, inp.D, inp.H, inp.W, inp.C), 7.0)] * 5, seen
    refs = {}
    for tdt in (F64, F32):
        o = orc.GDOracle(inp.psf, kind="fista", dtype=tdt, proj=lambda x: torch.clamp(x, min=0) * (1.0 - 7.0 / 100.0))
        o.set_data(inp.data[0, 0])
        refs[tdt] = npy(o.apply(4))
    compare("GD hooks", f"{name} denoiser", "float32", "final", out, refs[F32], refs[F64], bad)
    assert not bad, bad


@pytest.mark.parametrize("name", SWEEP)
def test_hook_equals_fused(backend, monkeypatch, name):
    """5 split iterations with non-negativity handed in as a callable against 5 fused ones: the same engine on another
    path (the same update kernel, or the fused-forward second-form kernel on ``rows8192`` / ``v2_depth2``)"""
    inp, bad = inputs(name), []
    set_plan(monkeypatch, name)
    for kind, cls in GD:
        runs = []
        for kw in ({"proj": plain_non_neg}, {}):
            rec = getattr(lpa, cls)(on_device(inp.psf, backend), **kw)
            check_plan(rec, name, "float32", "gd")
            rec.set_data(on_device(inp.data[0, 0], backend))
            runs.append((npy(rec.apply(n_iter=5, disp_iter=None)), npy(rec._image_est)))
        (hook, hook_state), (fused, fused_state) = runs
        assert float(np.abs(fused).max()) > 0 and float(np.abs(fused_state).max()) > 0
        for key, a, b in (("image", hook, fused), ("state", hook_state, fused_state)):
            r = rel(a, b)
            print(f"{name} {kind} {key}: hook against fused {r:.3e} (bound {SAME_ENGINE:.0e})")
            if not r <= SAME_ENGINE:
                bad.append((kind, key, r))
    assert not bad, bad


@pytest.mark.parametrize("name", MIXED_CASES)
def test_fused_and_split_iterations_on_one_handle(backend, monkeypatch, name):
    """_iterate(2), one split iteration through the raw entry points, _iterate(2) against _iterate(5): the split iteration
    starts from the row spectra the fused update kernel left, and the fused one after it must not take stale ones"""
    inp, bad = inputs(name), []
    set_plan(monkeypatch, name)
    for kind, cls in GD:
        rec, ref = (getattr(lpa, cls)(on_device(inp.psf, backend)) for _ in range(2))
        check_plan(rec, name, "float32", "gd")
        for r in (rec, ref):
            r.set_data(on_device(inp.data[0, 0], backend))
        rec._iterate(2)
        rec._handle.iterate_begin(rec._stream())
        x = rec._empty(rec._state_shape())
        rec._handle.get_state("image_est", x.data_ptr(), rec._stream())
        proj = torch.clamp(x, min=0).contiguous()
        rec._handle.iterate_end(proj.data_ptr(), rec._stream())
        rec._iterate(2)
        ref._iterate(5)
        want = npy(ref._image_est)
        r = rel(rec._image_est, want)
        print(f"{name} {kind}: 2 fused + 1 split + 2 fused against 5 fused {r:.3e} (bound {SAME_ENGINE:.0e})")
        assert float(np.abs(want).max()) > 0
        if not r <= SAME_ENGINE or not rel(rec.get_image_estimate(), ref.get_image_estimate()) <= SAME_ENGINE:
            bad.append((kind, r))
    assert not bad, bad


@pytest.mark.parametrize("dual", [False, True], ids=["plain", "dual"])
@pytest.mark.parametrize("name", DEPTH1)
def test_admm_plug_and_play(backend, monkeypatch, name, dual):
    """apply(3), reconstruction_error() (which must not disturb the run), apply(2, reset=False) with the smoothing denoiser
    and a non-zero initial estimate: both images, and all seven states on the WHOLE padded frame (three of the plans keep xi
    inside the window only when fused; the explicit-state path must hold all of it)"""
    inp, bad, mode = inputs(name), [], "dual" if dual else "plain"
    refs = admm_ref(name, mode)
    set_plan(monkeypatch, name)
    rec = lpa.ADMM(on_device(inp.psf, backend), initial_est=on_device(inp.init, backend),
                   denoiser={"network": pnp_denoise, "noise_level": PNP_LEVEL, "use_dual": dual}, **PNP)
    check_plan(rec, name, "float32", "admm")
    rec.set_data(on_device(inp.data[0, 0], backend))
    for i, n in enumerate((3, 2)):
        out = rec.apply(n_iter=n, disp_iter=None, reset=i == 0)
        compare("PnP", f"{name} {mode}", "float32", f"final{i}", out, refs[F32][(0, 0)][f"final{i}"],
                refs[F64][(0, 0)][f"final{i}"], bad)
        if i == 0:
            err = float(rec.reconstruction_error())
            assert np.isfinite(err) and err > 0
    compare_admm("PnP", f"{name} {mode}", "float32", rec, refs, 0, 0, bad, eta_is_zero=not dual)
    report("PnP")
    assert not bad, bad


@pytest.mark.parametrize("name", DEPTH1)
def test_admm_custom_prior(backend, monkeypatch, name):
    """the ``psi2`` triple of tests/test_custom_psi.py: the same two calls and states; then, on a solver that ran 2 iterations,
    ``_set_psf(other)`` and apply(3) against a fresh oracle on the other PSF (the gram pushed again, on ``fourstep`` /
    ``half_split`` into the permuted row order)"""
    inp, bad = inputs(name), []
    refs, refs_other = admm_ref(name, "psi"), admm_ref(name, "psi", calls=(3,), other=True)
    set_plan(monkeypatch, name)
    rec = lpa.ADMM(on_device(inp.psf, backend), psi=psi2, psi_adj=psi2_adj, psi_gram=psi2_gram, **PSI)
    check_plan(rec, name, "float32", "admm")
    rec.set_data(on_device(inp.data[0, 0], backend))
    for i, n in enumerate((3, 2)):
        out = rec.apply(n_iter=n, disp_iter=None, reset=i == 0)
        compare("custom prior", name, "float32", f"final{i}", out, refs[F32][(0, 0)][f"final{i}"],
                refs[F64][(0, 0)][f"final{i}"], bad)
        if i == 0:
            err = float(rec.reconstruction_error())
            assert np.isfinite(err) and err > 0
    compare_admm("custom prior", name, "float32", rec, refs, 0, 0, bad)
    rec.apply(n_iter=2, disp_iter=None)
    rec._set_psf(on_device(inp.psf_other, backend))
    out = rec.apply(n_iter=3, disp_iter=None)
    compare("custom prior", f"{name} other PSF", "float32", "final0", out, refs_other[F32][(0, 0)]["final0"],
            refs_other[F64][(0, 0)]["final0"], bad)
    compare_admm("custom prior", f"{name} other PSF", "float32", rec, refs_other, 0, 0, bad)
    report("custom prior")
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", BATCH_CASES)
def test_batch_depth_and_float64(backend, monkeypatch, name, dtype):
    """B = 2 frames x D = 2 planes: FISTA with the hook through apply_batch(4) + apply_batch(2, reset=False) per frame
    against the oracle of depth 2, plug-and-play ADMM (both use_dual values) through apply_batch(3) + apply_batch(2,
    reset=False) per frame and per plane against the depth-1 oracle"""
    inp, bad = inputs(name, 2), []
    set_plan(monkeypatch, name)
    psf, data = on_device(inp.psf, backend, dtype), on_device(inp.data, backend, dtype)
    ref = gd_ref(name, "fista", depth=2, calls=(4, 2), frames=(0, 1))
    rec = lpa.FISTA(psf, dtype=dtype, proj=shrink)
    rec.set_data(data)
    check_plan(rec, name, dtype, "gd")
    for i, n in enumerate((4, 2)):
        out = rec.apply_batch(n_iter=n, reset=i == 0)
        state = rec._image_est
        assert tuple(out.shape) == (2, 2, inp.H, inp.W, inp.C)
        for b in range(2):
            for key, got in ((f"final{i}", out[b]), (f"state{i}", state[b])):
                compare("GD hooks", f"{name} fista frame {b}", dtype, key, got, ref[F32][b][key], ref[F64][b][key], bad)
    for dual in (False, True):
        mode = "dual" if dual else "plain"
        refs = admm_ref(name, mode, depth=2, frames=(0, 1))
        rec = lpa.ADMM(psf, dtype=dtype, initial_est=on_device(inp.init, backend, dtype),
                       denoiser={"network": pnp_denoise, "noise_level": PNP_LEVEL, "use_dual": dual}, **PNP)
        rec.set_data(data)
        check_plan(rec, name, dtype, "admm")
        outs = [rec.apply_batch(n_iter=n, reset=i == 0).clone() for i, n in enumerate((3, 2))]
        for b in range(2):
            for d in range(2):
                tag = f"{name} {mode} frame {b} plane {d}"
                for i in range(2):
                    compare("PnP", tag, dtype, f"final{i}", outs[i][b, d], refs[F32][(b, d)][f"final{i}"][0],
                            refs[F64][(b, d)][f"final{i}"][0], bad)
                compare_admm("PnP", tag, dtype, rec, refs, b, d, bad, eta_is_zero=not dual)
    report("GD hooks")
    report("PnP")
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", ["golden", "rows8192"])
def test_unrolled_fista_custom_projection(backend, monkeypatch, name, dtype):
    """``UnrolledFISTA(psf, proj=shrink)`` under torch.no_grad(): split iterations that take iteration i's step and momentum
    factor from the schedule, against the restatement with the same projection; and non-negativity in disguise against the
    fused forward"""
    psf, data, alpha, tk, n = unrolled_inputs(name)
    ref, bad = unrolled_ref(name), []
    if name != "golden":
        set_plan(monkeypatch, name)
    psf, batch = on_device(psf, backend, dtype), on_device(data, backend, dtype)
    outs = {}
    for key, kw in (("shrink", {"proj": shrink}), ("disguise", {"proj": plain_non_neg}), ("fused", {})):
        rec = lpa.UnrolledFISTA(psf, n_iter=n, dtype=dtype, **kw)
        rec.set_parameters(alpha=alpha, tk=tk)
        if name != "golden":
            check_plan(rec, name, dtype, "gd")
        with torch.no_grad():
            outs[key] = npy(rec(batch))
    compare("unrolled proj", f"unrolled {name}", dtype, "out", outs["shrink"], ref[F32], ref[F64], bad)
    r = rel(outs["disguise"], outs["fused"])
    print(f"unrolled {name} {dtype}: non-negativity as a callable against the fused forward {r:.3e} (bound {SAME_ENGINE:.0e})")
    assert float(np.abs(outs["fused"]).max()) > 0 and r <= SAME_ENGINE
    report("unrolled proj")
    assert not bad, bad
