"""
Unrolled ADMM with a per-iteration schedule (``UnrolledADMM``, lpc_set_admm_schedule) over launch plans, shapes and dtypes,
against the CPU oracle in float64, through the public API, on the SIMT emulator ('emu') and on the MI355X ('hip', -m gpu).

What a schedule crosses inside the engine: the pending dual updates take the PREVIOUS iteration's step sizes and the prox
the current ones (admm_params / admm_scalars, k_admm_flush at a read-out), R_divmat is formed per iteration, and several
launch plans keep something derived from the step sizes -- the duals half-applied between the iterations of a call
(k1_half), the TV / W half inside the forward rows, the sequential middle's precombined constants (k_mid_consts), the
pair-line copies of H and |G|, the split middles.  Every case below asserts the marker of its plan in ``plan_info()``.

Reference: ``ADMMOracle(psf, dtype=torch.float64, schedule=...)``, pinned to the reference's own ``UnrolledADMM`` by
tests/test_oracle_golden.py::test_unrolled_admm_schedule_matches_reference; it gets the schedule as the float32 values the
engine receives.  Yardstick: the same oracle in float32, never the engine.

Inputs: ``synthetic_psf(1, H, W, C, seed)``, measurement ``rng.random((B, 1, H, W, C))``, 6 iterations, step sizes
(1e-6, 1e-4, 4e-5, 2e-6) x the per-iteration factors of ``FACTORS`` (in [0.5, 2], another table for each parameter,
neighbouring iterations -- cyclically -- at least 30 % apart: asserted).  test_the_check_has_teeth shows on the oracle alone
that taking any one entry from the neighbouring iteration moves the final image by over 100 x the float32 bound.

Bounds (the rule of tests/test_unrolled_grad_sweep.py; max-norm over whole arrays, relative to the max of the float64 array):
  float32 engine:  rel(q, oracle64) <= 4 * max(rel(oracle32, oracle64), 2e-6) for every quantity q; a yardstick above 2.5e-6
                   (which would make the bound looser than the 1e-5 ADMM_TOL allows at 10 iterations) is refused: pick
                   another seed.  U, eta and rho sit five decades below V and get 10 x ADMM_TOL in
                   test_admm_matches_reference_golden: their yardstick may reach 2.5e-5, by the same rule;
  float64 engine:  F64_TOL = 1e-11, x 100 for U, eta, rho and xi (test_admm_matches_reference_golden's rule).
Worst values on the emulator, over every case, frame and call pattern:
  quantity          float32 engine   float32 oracle   float64 engine
  final image          8.1e-7           1.0e-6           2.1e-15
  V, HV, W          <= 8.4e-7        <= 8.3e-7        <= 1.9e-15
  X                    1.6e-6           2.0e-6           4.0e-15
  xi                   4.3e-7           4.0e-7           7.7e-16
  U                    5.6e-6           6.4e-6           1.4e-14
  eta                  4.5e-6           4.0e-6           1.0e-14
  rho                  3.5e-6           3.5e-6           6.9e-15
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from oracle import lensless_oracle as orc
from unrolled_restated import F64_TOL, rel

N_ITER = 6
BASE = dict(mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-6)
FACTORS = dict(mu1=[1.0, 0.6, 1.5, 0.8, 2.0, 0.5], mu2=[0.7, 1.4, 2.0, 0.9, 0.55, 1.2],
               mu3=[1.8, 1.1, 0.5, 1.3, 0.75, 1.0], tau=[1.2, 1.7, 0.5, 0.9, 2.0, 0.65])
# a second schedule, for the tests that change the parameters of a solver that already ran
FACTORS_B = dict(mu1=[1.9, 0.7, 1.2, 0.5, 0.9, 1.4], mu2=[1.5, 0.6, 2.0, 1.0, 1.7, 0.8],
                 mu3=[0.6, 1.7, 0.9, 2.0, 1.2, 0.9], tau=[0.5, 1.8, 0.8, 1.3, 0.6, 2.0])
STATES = (("V", "_image_est"), ("HV", "_forward_out"), ("X", "_X"), ("W", "_W"), ("U", "_U"), ("xi", "_xi"),
          ("eta", "_eta"), ("rho", "_rho"))
SPLIT = {"tile_budget": 512, "col_t": 4}
MOD = {"jit_min_points": 0}

# name: (H, W, C, B), seed, launch-plan options, what plan_info() must hold (``f32`` / ``f64``: in that build only; ``ends``:
# how the float32 plan module's name ends)
CASES = {
    "rt": dict(shape=(24, 32, 3, 2), opts={}, info=["run-time plans", "stand-alone image-domain kernel"]),
    # the scalar image kernel, odd x odd
    "rt_odd": dict(shape=(21, 13, 1, 2), opts={}, info=["padded 45x25", "stand-alone image-domain kernel"]),
    "mod": dict(shape=(24, 32, 3, 2), opts=MOD, info=["TV / W half and X half inside the forward rows",
                                                      "row transforms skipped"]),
    "mod_tiled": dict(shape=(24, 32, 3, 2), opts={**MOD, "k1_rows": 0}, info=["tiled TV / W kernel + X half"]),
    "mod_nohalf": dict(shape=(24, 32, 3, 2), opts={**MOD, "k1_half": 0},
                       info=["TV / W half and X half inside the forward rows", "row transforms skipped"]),
    "mod_60": dict(shape=(47, 29, 3, 1), opts=MOD, info=["paired 60 [static 4.5.3"]),
    "rows_half": dict(shape=(24, 32, 3, 2), opts={**MOD, "rows_half": 1}, info=["half-length 32"]),
    "split_reg": dict(shape=(48, 20, 1, 2), opts={**SPLIT, "split_n2": 24}, info=["4 x 24 split"],
                      f32=["middle in registers"]),
    "split_lds": dict(shape=(48, 20, 1, 2), opts={**SPLIT, "split_n2": 12}, info=["8 x 12 split"]),
    "split_mod": dict(shape=(48, 20, 1, 2), opts={**SPLIT, "split_n2": 12, **MOD}, info=["pass A [static"]),
    # the sequential middle's precombined constants, with complex (odd window start) and real phases
    # (the float64 build has neither that middle nor pair lines -- a tile row of 8 complex128 columns is a whole line
    # already: there the same options give the side-by-side middle of 8-column tiles on a plan module)
    "seq_odd": dict(shape=(23, 40, 1, 2), opts={"mid_seq": 1, "tile_budget": 720, **MOD}, info=[],
                    f32=["one spectrum at a time, pair-line spectra"], ends="pLc"),
    "seq_even": dict(shape=(24, 40, 3, 2), opts={"mid_seq": 1, "tile_budget": 768, **MOD}, info=[],
                     f32=["one spectrum at a time, pair-line spectra"], f64=["T = 8, LDS middle [static 8.6]"], ends="pLr"),
    "pair": dict(shape=(23, 40, 3, 2), opts={"mid_seq": 0, "tile_budget": 720, **MOD}, info=["pair-line spectra"]),
    "gterms": dict(shape=(24, 32, 3, 2), opts={**MOD, "g_plane": 0}, info=["gram as row + column terms"]),
}
for _i, _c in enumerate(CASES.values()):
    _c["seed"] = 300 + _i
F64_CASES = ["rt", "rt_odd", "mod", "split_reg", "split_mod", "seq_even"]      # the other float64 modules are the same code
CASE_DTYPES = [(c, "float32") for c in CASES] + [(c, "float64") for c in F64_CASES]
STATE_CASES = ["rt", "rt_odd", "mod", "mod_tiled", "mod_nohalf", "seq_odd"]
CALL_PATTERNS = [(3,), (1, 2), (4, 2), (6,)]
DUALS = ("U", "eta", "rho", "xi")
YARDSTICK_MAX = 2.5e-6


def schedule(factors=FACTORS, n=N_ITER):
    """the float32 values the engine receives (unrolled_admm.py:147-151), as float32 arrays"""
    return {k: (np.float64(BASE[k]) * np.asarray(factors[k][:n])).astype(np.float32) for k in BASE}


def _snapshot(o):
    return {k: getattr(o, k).numpy().copy() for k, _ in STATES}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """PSF and measurement of a case, and the float64 / float32 oracle's trajectory of every frame under ``schedule()``:
    the eight states after 3 and after 6 iterations (no form_image in between) and the final image; computed once, never
    written to"""
    case = CASES[name]
    H, W, C, B = case["shape"]
    rng = np.random.default_rng(case["seed"])
    psf = orc.synthetic_psf(1, H, W, C, case["seed"])
    data = rng.random((B, 1, H, W, C), dtype=np.float32)
    inp = SimpleNamespace(name=name, psf=psf, data=data, sched=schedule(), ref={})
    for tdt in (torch.float64, torch.float32):
        frames = []
        for b in range(B):
            o = orc.ADMMOracle(psf, dtype=tdt, schedule=inp.sched, **BASE)
            o.set_data(data[b, 0])
            o.reset()
            states = {}
            for i in range(N_ITER):
                o.step()
                if i + 1 in (3, N_ITER):
                    states[i + 1] = _snapshot(o)
            frames.append(SimpleNamespace(states=states, final=o.form_image()[0].numpy().copy()))
        inp.ref[tdt] = frames
    for b in range(B):
        f32, f64 = inp.ref[torch.float32][b], inp.ref[torch.float64][b]
        for n, states in f64.states.items():     # the prox is active where the states are read: U is no array of zeros
            live = float((states["U"] != 0).mean())
            assert live >= 0.05, f"{name} frame {b}: {100 * live:.1f} % of U non-zero after {n} iterations"
        # the yardstick must not loosen the bound beyond what ADMM_TOL allows at 10 iterations (x 10 for U, eta and rho)
        pairs = [("final", f32.final, f64.final)] + [(f"{k} after {n}", f32.states[n][k], f64.states[n][k])
                                                     for n in f64.states for k, _ in STATES]
        for key, a32, a64 in pairs:
            y, most = rel(a32, a64), YARDSTICK_MAX * (10 if key.split()[0] in ("U", "eta", "rho") else 1)
            assert y <= most, f"{name} frame {b} {key}: float32 oracle {y:.2e} from the float64 oracle: pick another seed"
    return inp


def bound_of(dtype, key, ref32, ref64):
    if dtype == "float64":
        return F64_TOL * (100 if key in DUALS else 1)
    return 4 * max(rel(ref32, ref64), 2e-6)


def compare(tag, dtype, key, got, ref32, ref64, bad):
    assert float(np.abs(ref64).max()) > 0, (tag, key)
    assert tuple(got.shape) == ref64.shape, (tag, key, tuple(got.shape), ref64.shape)
    r, y, bound = rel(got, ref64), rel(ref32, ref64), bound_of(dtype, key, ref32, ref64)
    print(f"{tag} {dtype} {key}: rel {r:.3e} (bound {bound:.1e}, float32 oracle {y:.3e})")
    if not r <= bound:
        bad.append((key, r, bound))


def markers(name, dtype):
    case = CASES[name]
    return case["info"] + case.get("f32" if dtype == "float32" else "f64", [])


def solver(name, dtype, backend, monkeypatch, sched, frames=None, extra=None, cls=lpa.UnrolledADMM):
    """a solver of the case on its launch plan (asserted) and its measurement on the backend's device; ``extra``: further
    options (hv_full=1 runs the H V row transforms everywhere: that marker is then not asked for)"""
    case, inp = CASES[name], inputs(name)
    monkeypatch.setattr(_native, "DEFAULT_OPTIONS", {**_native.DEFAULT_OPTIONS, **case["opts"], **(extra or {})})
    tdt = torch.float64 if dtype == "float64" else torch.float32
    psf = torch.from_numpy(inp.psf).to(device=backend.device, dtype=tdt)
    rec = cls(psf, dtype=dtype, n_iter=N_ITER, **BASE)
    if sched is not None:
        rec.set_parameters(**sched)
    data = torch.from_numpy(inp.data[slice(None) if frames is None else frames]).to(device=backend.device, dtype=tdt)
    rec._data = data
    rec._upload_data()          # (the handle of this batch size: the plan is the one the run uses)
    info = rec._handle.plan_info()
    for marker in markers(name, dtype):
        if not ((extra or {}).get("hv_full") and marker == "row transforms skipped"):
            assert marker in info, (marker, info)
    assert info.endswith(case.get("ends", "") if dtype == "float32" else ""), info
    return rec, data


def states_of(rec):
    return {k: getattr(rec, attr).detach().cpu().numpy().copy() for k, attr in STATES}


# ------------------------------------------------------------------------------------------------- CPU only --
def test_inputs_meet_their_conditions():
    """the factor tables: in [0.5, 2], another table per parameter, cyclic neighbours at least 30 % apart; and every case's
    float32 yardstick of the final image stays under 2.5e-6 (asserted in ``inputs``)"""
    for factors in (FACTORS, FACTORS_B):
        tables = [tuple(factors[k]) for k in BASE]
        assert len(set(tables)) == 4 and all(len(t) == N_ITER for t in tables)
        for t in tables:
            assert 0.5 <= min(t) and max(t) <= 2.0
            for i in range(N_ITER):
                a, b = t[i], t[(i + 1) % N_ITER]
                assert max(a, b) / min(a, b) >= 1.3, (t, i)
    for name in CASES:
        inp = inputs(name)
        ys = [rel(f32.final, f64.final) for f32, f64 in zip(inp.ref[torch.float32], inp.ref[torch.float64])]
        worst = {k: max(rel(f32.states[n][k], f64.states[n][k]) for n in (3, N_ITER)
                        for f32, f64 in zip(inp.ref[torch.float32], inp.ref[torch.float64])) for k, _ in STATES}
        print(f"{name}: float32 oracle, final image:", " ".join(f"{y:.2e}" for y in ys), "| states:",
              " ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def test_the_check_has_teeth():
    """on the ``rt`` inputs, the oracle alone: mu1, mu2, mu3 at every iteration and tau at iterations >= 1 (tau_0 thresholds
    zeros) taken from the next iteration (cyclically) move the float64 final image by at least 100 x the float32 bound --
    an engine that took any one step size from the wrong iteration cannot pass the forward parity"""
    inp = inputs("rt")
    ref64, ref32 = inp.ref[torch.float64][0].final, inp.ref[torch.float32][0].final
    bound = bound_of("float32", "final", ref32, ref64)
    worst = None
    for key in BASE:
        for i in range(1 if key == "tau" else 0, N_ITER):
            sched = {k: v.copy() for k, v in inp.sched.items()}
            sched[key][i] = inp.sched[key][(i + 1) % N_ITER]
            o = orc.ADMMOracle(inp.psf, dtype=torch.float64, schedule=sched, **BASE)
            o.set_data(inp.data[0, 0])
            moved = rel(o.apply(N_ITER).numpy(), ref64)
            print(f"{key}[{i}] <- {key}[{(i + 1) % N_ITER}]: final image moves by {moved:.3e} (bound {bound:.1e})")
            assert moved >= 100 * bound, (key, i, moved, bound)
            worst = moved if worst is None else min(worst, moved)
    print(f"smallest move {worst:.3e} = {worst / bound:.0f} x the float32 bound")


# ----------------------------------------------------------------------------------------- emulator and card --
@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_forward_parity(backend, monkeypatch, name, dtype):
    """``UnrolledADMM.forward(batch)`` against the oracle's ``apply(6)``, per frame"""
    inp = inputs(name)
    rec, data = solver(name, dtype, backend, monkeypatch, inp.sched)
    out = rec.forward(data)
    assert tuple(out.shape) == inp.data.shape[:4] + (inp.psf.shape[-1],) and out.dtype == data.dtype
    bad = []
    for b in range(out.shape[0]):
        compare(f"{name} frame {b}", dtype, "final", out[b].cpu().numpy(), inp.ref[torch.float32][b].final,
                inp.ref[torch.float64][b].final, bad)
    assert not bad, bad


@pytest.mark.parametrize("name", ["rt", "mod"])
def test_negated_entries_change_nothing(backend, monkeypatch, name):
    """the engine and the reference take ``abs`` of the learnt values (unrolled_admm.py:147-151): the same bits"""
    inp = inputs(name)
    rec, data = solver(name, "float32", backend, monkeypatch, inp.sched)
    plain = rec.forward(data)
    neg = {k: v.copy() for k, v in inp.sched.items()}
    neg["mu1"][0], neg["mu2"][2], neg["mu3"][5], neg["tau"][1], neg["tau"][4] = (
        -neg["mu1"][0], -neg["mu2"][2], -neg["mu3"][5], -neg["tau"][1], -neg["tau"][4])
    rec2, _ = solver(name, "float32", backend, monkeypatch, neg)
    assert float(plain.abs().max()) > 0 and torch.equal(rec2.forward(data), plain)


@pytest.mark.parametrize("calls", CALL_PATTERNS, ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("name,dtype", [(c, d) for c, d in CASE_DTYPES if c in STATE_CASES])
def test_state_parity_in_the_middle_of_a_schedule(backend, monkeypatch, name, dtype, calls):
    """every state after calls of these lengths (a read-out flushes the pending dual updates with the PREVIOUS iteration's
    step sizes), against the oracle stepped as many times without form_image; frame 0"""
    inp = inputs(name)
    rec, _ = solver(name, dtype, backend, monkeypatch, inp.sched, frames=slice(0, 1))
    rec.reset()
    for k in calls:
        rec._iterate(k)
    got = states_of(rec)
    ref64, ref32 = inp.ref[torch.float64][0].states[sum(calls)], inp.ref[torch.float32][0].states[sum(calls)]
    bad = []
    for key, _ in STATES:
        compare(f"{name} calls {calls}", dtype, key, got[key], ref32[key], ref64[key], bad)
    assert not bad, bad


@pytest.mark.parametrize("name", ["mod", "seq_even"])
def test_calls_of_any_length_are_one_trajectory(backend, monkeypatch, name):
    """with hv_full=1 and k1_half=0 (the reason: test_xi_outside_the_sensor_window) one call of 6, six calls of 1 and
    calls of 4 + 2 are the same instruction stream: all eight states bit for bit"""
    inp = inputs(name)
    runs = {}
    for calls in ((6,), (1,) * 6, (4, 2)):
        rec, _ = solver(name, "float32", backend, monkeypatch, inp.sched, extra={"hv_full": 1, "k1_half": 0})
        rec.reset()
        for k in calls:
            rec._iterate(k)
        runs[calls] = states_of(rec)
    first = runs[(6,)]
    assert all(float(np.abs(v).max()) > 0 for v in first.values())
    for calls, got in runs.items():
        for key, _ in STATES:
            assert np.array_equal(got[key], first[key]), (calls, key, rel(got[key], first[key]))


@pytest.mark.parametrize("name", ["mod", "seq_odd", "seq_even", "split_mod"])
def test_new_parameters_between_forwards(backend, monkeypatch, name):
    """set_parameters(A), forward, set_parameters(B), forward on ONE solver: the second result is a fresh solver's bit for
    bit (nothing derived from A survives -- R_divmat, the sequential middle's constants) and far from the first; then a
    constant schedule on the same object is plain ADMM.apply_batch, bit for bit"""
    inp = inputs(name)
    sched_b = schedule(FACTORS_B)
    rec, data = solver(name, "float32", backend, monkeypatch, inp.sched)
    out_a = rec.forward(data).clone()
    rec.set_parameters(**sched_b)
    out_b = rec.forward(data).clone()
    fresh, _ = solver(name, "float32", backend, monkeypatch, sched_b)
    want_b = fresh.forward(data)
    moved = rel(out_a, want_b)
    print(f"{name}: schedule A against schedule B: {moved:.3e}")
    assert torch.equal(out_b, want_b) and moved > 1e-2, moved
    rec.set_parameters(**{k: np.full(N_ITER, v) for k, v in BASE.items()})
    out_c = rec.forward(data)
    plain, _ = solver(name, "float32", backend, monkeypatch, None, cls=lpa.ADMM)
    want_c = plain.apply_batch(n_iter=N_ITER)
    assert torch.equal(out_c, want_c) and rel(out_b, want_c) > 1e-2
