"""
Option admm_rows_v2 (bits: 1 the forward rows with the X half -- the default --, 2 the inverse rows, which measured slower
at 12 MP and stay selectable): ADMM's two half-length row kernels in their second form (lpc_admm_v2_kernels.h: M / R
lanes per row, one butterfly per lane and stage, tangling + first inverse stage straight from global memory, the last
stage in registers, the blocks of `a` formed pair by pair from batched loads) wherever the row plan has one radix and the
window offset and frame width are even.  The arithmetic is the first form's, statement for statement: the two forms must
agree BIT FOR BIT -- on the image and on every array a call leaves behind -- so that mixing them inside a call (the first
and the last iteration of a call keep the first form of the forward rows) changes nothing.

Every case: rows_half=1, jit_min_points=0, the default tile budget, TV-active parameters (U is not identically zero) and
n_iter = 8, so that the steady-state iterations 2 .. n - 3 (rows outside the window skipped) and the complete last three
both run.  Every case runs on the SIMT emulator and on the GPU.

Anchor: the image against the float64 oracle <= 1e-5 of max|ref| (the bound of tests/test_dual_elision.py).
"""
import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from oracle import lensless_oracle as orc
from test_parity_small import engine_opts, rel

TV = dict(tau=5e-3, mu1=1e-2, mu2=1e-2, mu3=1e-2)       # U, W and all three duals alive
OPTS = dict(rows_half=1, jit_min_points=0)
N_ITER = 8
V2 = "ADMM rows: second form"
STATE = {"V": "_image_est", "xi": "_xi", "eta": "_eta", "rho": "_rho", "HV": "_forward_out"}

# name -> (PSF depth, frame height, width, PSF channels, data channels, the second form is expected)
CASES = {
    "flagship_rows": (1, 5, 4056, 3, 3, True),      # padded 9 x 8192, M = 4096 = 16.16.16, 256 lanes; odd padded height
    "gray_on_rgb": (1, 5, 4056, 3, 1, True),        # one measurement channel against an RGB PSF: the data plane of y
    "depth2": (2, 5, 4056, 1, 1, True),             # two PSF planes share one measurement plane
    "edge_quads": (1, 5, 4060, 3, 3, True),         # sw = 2066: the window starts and ends inside a quad
    "odd_offset": (1, 5, 4054, 3, 3, False),        # sw = 2069: no pair geometry -> the first form
}


def problem(case):
    D, H, W, C, Cy, _ = CASES[case]
    rng = np.random.default_rng(1000 * H + W + 7 * D + Cy)
    psf = orc.synthetic_psf(D, H, W, C, seed=H + 3 * W + D)
    y = rng.random((1, H, W, Cy), dtype=np.float32)
    return psf, y


def run(monkeypatch, psf, y, v2, calls):
    """the image after each call of `calls` and the arrays the last one leaves behind, plus plan_info()"""
    engine_opts(monkeypatch, **OPTS, admm_rows_v2=v2)
    rec = lpa.ADMM(psf, **TV)
    rec.set_data(y[:, None])
    imgs = [np.asarray(rec.apply_batch(n_iter=n, reset=(i == 0))).copy() for i, n in enumerate(calls)]
    state = {k: np.asarray(getattr(rec, attr)).copy() for k, attr in STATE.items()}
    return imgs, state, rec._handle.plan_info()


def assert_same_bits(on, off, what):
    imgs1, st1 = on
    imgs0, st0 = off
    for i, (a, b) in enumerate(zip(imgs1, imgs0)):
        assert float(np.abs(b).max()) > 0
        print(what, "image after call", i, "max |diff|", float(np.abs(a - b).max()))
        assert np.array_equal(a, b), (what, "image", i)
    for k in STATE:
        assert float(np.abs(st0[k]).max()) > 0, k
        print(what, k, "max |diff|", float(np.abs(st1[k] - st0[k]).max()))
        assert np.array_equal(st1[k], st0[k]), (what, k)


_runs = {}


def both_forms(backend, monkeypatch, case, calls, v2=3):
    """the run with admm_rows_v2=v2 (3: both kernels in the second form) and the run with admm_rows_v2=0"""
    psf, y = problem(case)
    for v in (v2, 0):
        key = (backend.kind, case, tuple(calls), v)
        if key not in _runs:
            _runs[key] = run(monkeypatch, psf, y, v, calls)
    return _runs[(backend.kind, case, tuple(calls), v2)], _runs[(backend.kind, case, tuple(calls), 0)]


@pytest.mark.parametrize("calls", [[N_ITER], [N_ITER, 4]], ids=["one_call", "continued"])
@pytest.mark.parametrize("case", list(CASES))
def test_second_form_equals_first_form(backend, monkeypatch, case, calls):
    """admm_rows_v2=3 (both kernels) against =0: the image, V, xi, eta, rho and H V are exactly equal after apply(8), and after apply(8)
    followed by apply(4, reset=False); plan_info() names the form that runs."""
    (i1, s1, info1), (i0, s0, info0) = both_forms(backend, monkeypatch, case, calls)
    assert "rows: half-length" in info1 and "tiled TV / W kernel + X half" in info1 and "xi half-applied" in info1, info1
    assert (V2 in info1) == CASES[case][5], info1
    assert V2 not in info0, info0
    if CASES[case][5]:
        assert "[static 16.16.16" in info1 and "forward + inverse, 256 lanes" in info1, info1
    assert_same_bits((i1, s1), (i0, s0), case)


def test_default_is_the_forward_rows_alone(backend, monkeypatch):
    """No option: the forward rows in the second form, the inverse rows in the first -- the mix equals admm_rows_v2=0 too."""
    (i1, s1, info1), (i0, s0, info0) = both_forms(backend, monkeypatch, "flagship_rows", [N_ITER], v2=None)
    assert V2 + ", forward, 256 lanes" in info1 and V2 not in info0, info1
    assert_same_bits((i1, s1), (i0, s0), "default")


def test_radix_8_rows(backend, monkeypatch):
    """M = 512 = 8.8.8 on 64 lanes (6 x 508 x 3, padded 12 x 1024) -- only if that is the row plan the chooser makes."""
    rng = np.random.default_rng(508)
    psf = orc.synthetic_psf(1, 6, 508, 3, seed=508)
    y = rng.random((1, 6, 508, 3), dtype=np.float32)
    on = run(monkeypatch, psf, y, 3, [N_ITER])
    if "[static 8.8.8" not in on[2]:
        pytest.skip("the chooser's row plan for 512 points is not 8.8.8: " + on[2])
    assert V2 in on[2] and "64 lanes" in on[2], on[2]
    off = run(monkeypatch, psf, y, 0, [N_ITER])
    assert V2 not in off[2], off[2]
    assert_same_bits(on[:2], off[:2], "radix 8")


def test_anchor_against_float64_oracle(backend, monkeypatch):
    """The pair of forms is not equal-and-wrong: the flagship row plan's image after 8 iterations against the float64
    oracle, within the bound of tests/test_dual_elision.py."""
    (imgs, _, info), _ = both_forms(backend, monkeypatch, "flagship_rows", [N_ITER])
    assert V2 in info, info
    psf, y = problem("flagship_rows")
    o = orc.ADMMOracle(psf, dtype=torch.float64, **TV)
    o.set_data(y[0])
    want = np.asarray(o.apply(N_ITER))
    r = rel(imgs[0][0], want)
    print("second form against the float64 oracle:", r)
    assert float(np.abs(want).max()) > 0 and r <= 1e-5, r
