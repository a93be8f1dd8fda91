"""
Between the iterations of one lpc_iterate() call two arrays are no longer moved (AdmmScalars::rho_rsp, xi_in / xi_out):

  rho_rsp   the tiled TV / W kernel reads rho~ = rho' - mu3 W back out of the r_sp it overwrites
            (rho~ = D(eta~) - r_sp with the four eta~ values it loads anyway): rho is neither written nor read (8R -> 7R)
  xi_half   inside the sensor window xi travels as xi~ = xi' - mu1 X = -a: the X half of the forward rows does not
            recompute the previous X and does not read H V_old there (3 Rw -> 2 Rw)

Both are identities in real arithmetic and cost one float32 rounding per iteration; every entry point outside the loop
(read-outs, continuations, the image) must find plain arrays.  Every case runs on the SIMT emulator and on the GPU.

Bounds.  Image against the float64 oracle <= 1e-5 of max|ref| and plan against plan <= 2e-6 (test_parity_small:
test_tv_half_inside_forward_rows); xi within 2e-5 of its scale (test_xi_outside_the_sensor_window); the state arrays as
in test_admm_matches_reference_golden -- ADMM_TOL by iteration count, ten times that for the duals rho / eta, which sit
decades below V; a count without an entry of its own (3, 4) takes the next larger one's.  float64 build, on against off:
1e-9 after 20 iterations (identical in real arithmetic; a double carries 1e-16 per operation).
"""
import os

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from oracle import lensless_oracle as orc
import test_parity_small as parity
from test_parity_small import ADMM_TOL, engine_opts, rel

TV = dict(tau=5e-3, mu1=1e-2, mu2=1e-2, mu3=1e-2)       # U, W and all three duals alive
TV2 = dict(tau=2e-6, mu2=1e-4)
PARAMS = {"tv": TV, "tv2": TV2}

TILED = dict(k1_rows=0, jit_min_points=0)
HALF = dict(rows_half=1, tile_budget=256, jit_min_points=0)
# name -> (frame shape, frames, options, tiled TV / W kernel)
PLANS = {
    "tiled_rgb": ((24, 32, 3), 1, TILED, True),                 # tiled K1 + X half, three planes
    "tiled_odd": ((13, 40, 1), 1, TILED, True),                 # odd padded height, window starting on an odd row
    "half_rows_split": ((12, 1014, 1), 1, HALF, True),          # half-length rows + split columns: the 12-MP kernel family
    "tiled_batch2": ((24, 32, 3), 2, TILED, True),              # several planes per launch
    # default plan (a frame this small gets its plan module only with jit_min_points=0): K1 inside the rows, xi_half only
    "three_launch_rgb": ((24, 32, 3), 1, dict(jit_min_points=0), False),
    "three_launch_960": ((270, 480, 1), 1, {}, False),
}
ON_RHO, ON_XI = "rho read back from r_sp", "xi half-applied"


def tol_for(n):
    return ADMM_TOL[min(k for k in ADMM_TOL if k >= n)]


def problem(plan, seed=0):
    (H, W, C), B, opts, tiled = PLANS[plan]
    rng = np.random.default_rng(1000 * H + W + seed)
    psf = orc.synthetic_psf(1, H, W, C, seed=H + 3 * W + seed)
    y = rng.random((B, H, W, C), dtype=np.float32)
    return psf, y, opts, tiled


def engine(psf, y, kw, dtype=None):
    if dtype == "float64":
        rec = lpa.ADMM(psf.astype(np.float64), dtype="float64", **kw)
        rec.set_data(y.astype(np.float64)[:, None])
    else:
        rec = lpa.ADMM(psf, **kw)
        rec.set_data(y[:, None])
    return rec


def check_plan(info, tiled, rho=True, xi=True):
    assert ("three launches per iteration" in info) == (not tiled), info
    assert ("tiled TV / W kernel + X half" in info) == tiled, info
    assert (ON_RHO in info) == (tiled and rho), info       # the three-launch plan stores no r_sp: xi_half only
    assert (ON_XI in info) == xi, info


_oracles = {}


def oracle_states(plan, par, calls):
    """float64 oracle after every call of `calls` (apply(n, reset=False): the read-out clamps V in place, like the
    reference), per frame: the image and V, xi, X, rho, eta.  Computed once per (plan, parameters, calls)."""
    key = (plan, par, tuple(calls))
    if key not in _oracles:
        psf, y, _, _ = problem(plan)
        out = []
        for b in range(y.shape[0]):
            o = orc.ADMMOracle(psf, dtype=torch.float64, **PARAMS[par])
            o.set_data(y[b])
            per_call = []
            for i, n in enumerate(calls):
                img = np.asarray(o.apply(n, reset=(i == 0))).copy()
                per_call.append(dict(image=img, **{k: getattr(o, k).numpy().copy() for k in ("V", "xi", "X", "rho", "eta")}))
            out.append(per_call)
        _oracles[key] = out
    return _oracles[key]


@pytest.mark.parametrize("calls", [[1], [2], [3], [5], [4, 1, 5]], ids=lambda c: "calls" + "_".join(map(str, c)))
@pytest.mark.parametrize("par", ["tv", "tv2"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_against_float64_oracle_across_call_boundaries(backend, monkeypatch, plan, par, calls):
    """Calls of every length around the boundaries (1: plain in, plain out; 2: one boundary; 3, 5: the recovery feeds
    the next recovery) and a continuation: after each call the image and every read-out match the float64 oracle, and
    xi is alive outside the sensor window."""
    psf, y, opts, tiled = problem(plan)
    engine_opts(monkeypatch, **opts)
    rec = engine(psf, y, PARAMS[par])
    check_plan(rec._handle.plan_info(), tiled)
    want = oracle_states(plan, par, calls)
    B, (H, W) = y.shape[0], y.shape[1:3]
    sh, sw = (int(v) for v in rec._start_idx)
    outside = np.ones(rec._padded_shape[1:3], bool)
    outside[sh:sh + H, sw:sw + W] = False
    done = 0
    for i, n in enumerate(calls):
        img = np.asarray(rec.apply_batch(n_iter=n, reset=(i == 0)))
        done += n
        got = {"V": rec._image_est, "xi": rec._xi, "X": rec._X, "rho": rec._rho, "eta": rec._eta}
        for b in range(B):
            ref = want[b][i]
            r = rel(img[b], ref["image"])
            print(plan, par, calls, "after", done, "frame", b, "image", r)
            assert r <= 1e-5, (done, b, r)
            for key in ("V", "X", "rho", "eta"):
                g, w = np.asarray(got[key])[b], ref[key].reshape(np.asarray(got[key])[b].shape)
                assert np.abs(w).max() > 0, key
                t = tol_for(done) * (10 if key in ("rho", "eta") else 1)
                print("   ", key, rel(g, w), "tol", t)
                assert rel(g, w) <= t, (key, done, b, rel(g, w))
            xi, xiw = np.asarray(got["xi"])[b], ref["xi"].reshape(np.asarray(got["xi"])[b].shape)
            scale = float(np.abs(xiw).max())
            print("    xi", np.abs(xi - xiw).max() / scale)
            assert scale > 0 and np.abs(xi - xiw).max() <= 2e-5 * scale, (done, b)
            assert np.abs(xi[0][outside]).max() > 0


@pytest.mark.parametrize("name", ["admm_24x32x3_tv", "admm_24x32x3_init_bg", "admm_24x32x3_default"])
def test_reference_trajectories_through_the_tiled_plan(backend, monkeypatch, name):
    """The reference's own trajectories (golden vectors: TV term, initial estimate + background, defaults) with rho
    read back from r_sp and xi half-applied, through the tiled TV / W kernel."""
    engine_opts(monkeypatch, jit_min_points=0, k1_rows=0)
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    check_plan(lpa.ADMM(g["psf"])._handle.plan_info(), True)
    parity.test_admm_matches_reference_golden(backend, name)


VARIANTS = {"rho_rsp": dict(xi_half=0), "xi_half": dict(rho_rsp=0), "both": {}}
OFF = dict(rho_rsp=0, xi_half=0)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("par", ["tv", "tv2"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_on_against_off(backend, monkeypatch, plan, par, dtype):
    """Each option alone and both, against both off on the same engine: the image after 8 iterations to 2e-6 in
    float32; to 1e-9 after 20 in float64."""
    psf, y, opts, tiled = problem(plan)
    n, bound = (20, 1e-9) if dtype == "float64" else (8, 2e-6)
    engine_opts(monkeypatch, **opts, **OFF)
    rec = engine(psf, y, PARAMS[par], dtype)
    check_plan(rec._handle.plan_info(), tiled, rho=False, xi=False)
    off = np.asarray(rec.apply_batch(n_iter=n)).copy()
    assert float(np.abs(off).max()) > 0
    for tag, v in VARIANTS.items():
        if tag == "rho_rsp" and not tiled:
            continue
        engine_opts(monkeypatch, **{**opts, **OFF, **{k: None for k in OFF if k not in v}})
        rec = engine(psf, y, PARAMS[par], dtype)
        check_plan(rec._handle.plan_info(), tiled, rho="rho_rsp" not in v, xi="xi_half" not in v)
        r = rel(np.asarray(rec.apply_batch(n_iter=n)), off)
        print(plan, par, dtype, tag, r)
        assert r <= bound, (tag, r)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("plan", ["tiled_rgb", "half_rows_split", "three_launch_rgb"])
def test_on_against_off_with_a_per_iteration_schedule(backend, monkeypatch, plan, dtype):
    """Unrolled ADMM changes every step size from one iteration to the next: the recovery uses the PREVIOUS iteration's
    mu3 (rho~ + mu3p V) and mu1 (xi~ + mu1p HV).  Same bounds as with constant step sizes."""
    psf, y, opts, tiled = problem(plan, seed=5)
    n, bound = (20, 1e-9) if dtype == "float64" else (8, 2e-6)
    k = np.arange(n)
    sched = dict(mu1=1e-2 * (1 + 0.3 * k), mu2=1e-2 * (1 + 0.1 * k), mu3=1e-2 * (1 + 0.2 * k), tau=5e-3 * (1 + 0.05 * k))
    tp = torch.float64 if dtype == "float64" else torch.float32
    frames = torch.from_numpy(np.stack([y[0], y[0][::-1].copy()])[:, None]).to(tp)

    def run():
        net = lpa.UnrolledADMM(torch.from_numpy(psf).to(tp), n_iter=n, **({"dtype": "float64"} if dtype == "float64" else {}))
        net.set_parameters(**sched)
        return np.asarray(net.forward(frames)).copy(), net._handle.plan_info()

    engine_opts(monkeypatch, **opts, **OFF)
    off, info = run()
    check_plan(info, tiled, rho=False, xi=False)
    assert float(np.abs(off).max()) > 0
    for tag, v in VARIANTS.items():          # each option alone, then both
        if tag == "rho_rsp" and not tiled:
            continue
        engine_opts(monkeypatch, **{**OFF, **{k: None for k in OFF if k not in v}})
        on, info = run()
        check_plan(info, tiled, rho="rho_rsp" not in v, xi="xi_half" not in v)
        print(plan, dtype, tag, rel(on, off))
        assert rel(on, off) <= bound, tag


_long = {}


@pytest.mark.parametrize("par", ["tv", "tv2"])
def test_no_extra_drift_over_a_long_call(backend, monkeypatch, par):
    """100 iterations in one call at 48 x 64 x 1 through the tiled kernel: 98 recoveries feed one another.  The distance
    to the float64 oracle with both options on is at most twice the distance with both off (the parent's behaviour is
    the yardstick) plus 1e-6.
    A float32 restatement of the iteration gives ratios of 0.85 ... 1.3 for these parameters."""
    H, W, C, n = 48, 64, 1, 100
    rng = np.random.default_rng(48)
    psf = orc.synthetic_psf(1, H, W, C, seed=48)
    y = rng.random((H, W, C), dtype=np.float32)
    if par not in _long:
        o = orc.ADMMOracle(psf, dtype=torch.float64, **PARAMS[par])
        o.set_data(y)
        _long[par] = np.asarray(o.apply(n)).copy()
    want = _long[par]
    assert float(np.abs(want).max()) > 0
    dist = {}
    for tag, extra in (("off", OFF), ("on", dict(rho_rsp=None, xi_half=None))):
        engine_opts(monkeypatch, **TILED, **extra)
        rec = lpa.ADMM(psf, **PARAMS[par])
        check_plan(rec._handle.plan_info(), True, rho=tag == "on", xi=tag == "on")
        rec.set_data(y)
        dist[tag] = rel(rec.apply(n_iter=n, disp_iter=None), want)
    print(par, dist)
    assert dist["on"] <= 2 * dist["off"] + 1e-6, dist


@pytest.mark.parametrize("plan", ["tiled_rgb", "half_rows_split", "tiled_batch2", "three_launch_rgb"])
def test_byte_accounting(backend, monkeypatch, plan):
    """lpc_kernel_bytes prices the tiled kernel on 7R (8R with rho_rsp=0) and the forward rows on one window-sized array
    less with xi half-applied."""
    psf, y, opts, tiled = problem(plan)
    eb = 4.0
    engine_opts(monkeypatch, **opts)
    on = engine(psf, y, TV)
    engine_opts(monkeypatch, **OFF)
    off = engine(psf, y, TV)
    _, Hp, Wp, C = on._padded_shape
    P = y.shape[0] * C
    R, Rw = eb * Hp * Wp * P, eb * y.shape[1] * y.shape[2] * P
    kb = lambda rec, k: rec._handle.kernel_bytes(_native.KERNEL_NAMES.index(k))     # noqa: E731
    if tiled:
        assert kb(on, "spatial") == 7 * R and kb(off, "spatial") == 8 * R
    else:
        assert kb(on, "spatial") == 0 and kb(off, "spatial") == 0
    assert kb(off, "row_fwd") - kb(on, "row_fwd") == Rw
    for k in ("col_a_fwd", "col_mid", "col_a_inv", "row_inv"):
        assert kb(on, k) == kb(off, k)
