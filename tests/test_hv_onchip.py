"""
Option hv_fuse (default 1): between the steady-state iterations of one call the rows of H V inside the sensor window never
reach memory.  Iteration `it` with it + 3 < n_iter runs k_hv_rows_v2 on the window's rows of the work spectrum SB -- inverse
row, the X half of iteration it + 1 with that iteration's step sizes, forward row, in place -- its inverse rows write V
alone, and iteration it + 1 transforms the rows of r_sp only.  The last three iterations of a call run as before and rewrite
both H V buffers whole.

The arithmetic is that of k_rinv_half / k_rfwd_half_x_v2, statement for statement, so hv_fuse=1 and hv_fuse=0 must agree BIT
FOR BIT: on the image after every call and on V, xi, eta, rho and H V after the last one (H V equal proves the last three
iterations rewrote it).  Every case runs on the SIMT emulator and on the GPU, with the parameters and helpers of
tests/test_admm_rows_v2.py (U, W and all duals alive).

Anchor: the image against the float64 oracle <= 1e-5 of max|ref| (the bound of tests/test_dual_elision.py).
"""
import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native
from oracle import lensless_oracle as orc
from test_admm_rows_v2 import STATE, TV, assert_same_bits, problem
from test_parity_small import engine_opts, rel

OPTS = dict(rows_half=1, jit_min_points=0)
ON = "H V rows on chip"
V2 = "ADMM rows: second form"
PATTERNS = [[8], [8, 4], [3], [4], [5], [1, 1, 6]]     # [3]: no fused iteration; [4]: exactly one


def run(monkeypatch, psf, y, fuse, calls, dtype=None, **opts):
    """the image after each call of `calls`, the arrays the last one leaves behind, plan_info() and the handle"""
    engine_opts(monkeypatch, **{**OPTS, **opts}, hv_fuse=fuse)
    if dtype == "float64":
        rec = lpa.ADMM(psf.astype(np.float64), dtype="float64", **TV)
        rec.set_data(y.astype(np.float64)[:, None])
    else:
        rec = lpa.ADMM(psf, **TV)
        rec.set_data(y[:, None])
    imgs = [np.asarray(rec.apply_batch(n_iter=n, reset=(i == 0))).copy() for i, n in enumerate(calls)]
    state = {k: np.asarray(getattr(rec, attr)).copy() for k, attr in STATE.items()}
    return imgs, state, rec._handle.plan_info(), rec


_runs = {}


def on_off(backend, monkeypatch, case, calls):
    psf, y = problem(case)
    for fuse in (1, 0):
        key = (backend.kind, case, tuple(calls), fuse)
        if key not in _runs:
            _runs[key] = run(monkeypatch, psf, y, fuse, calls)[:3]
    return _runs[(backend.kind, case, tuple(calls), 1)], _runs[(backend.kind, case, tuple(calls), 0)]


@pytest.mark.parametrize("calls", PATTERNS, ids=lambda c: "calls" + "_".join(map(str, c)))
@pytest.mark.parametrize("case", ["flagship_rows", "gray_on_rgb", "depth2", "edge_quads"])
def test_on_equals_off(backend, monkeypatch, case, calls):
    (i1, s1, info1), (i0, s0, info0) = on_off(backend, monkeypatch, case, calls)
    assert ON in info1 and V2 + ", forward, 256 lanes" in info1 and "[static 16.16.16" in info1, info1
    assert ON not in info0 and V2 in info0, info0
    assert_same_bits((i1, s1), (i0, s0), case)


def test_split_columns(backend, monkeypatch):
    """12 x 4056 x 1 with a tile budget of 256: pass A rescales the rows of SB outside the window (sb_outside_scale) next to
    the rows the fused kernel has written; both row kernels in their second form."""
    rng = np.random.default_rng(12)
    psf = orc.synthetic_psf(1, 12, 4056, 1, seed=12)
    y = rng.random((1, 12, 4056, 1), dtype=np.float32)
    on = run(monkeypatch, psf, y, 1, [8], tile_budget=256, admm_rows_v2=3)
    off = run(monkeypatch, psf, y, 0, [8], tile_budget=256, admm_rows_v2=3)
    assert ON in on[2] and "pass A" in on[2] and V2 + ", forward + inverse" in on[2], on[2]
    assert ON not in off[2] and "pass A" in off[2], off[2]
    assert_same_bits(on[:2], off[:2], "split columns")


def test_radix_8_rows(backend, monkeypatch):
    """M = 512 = 8.8.8 on 64 lanes (6 x 508 x 3) -- only if that is the row plan the chooser makes.
    The fused kernel is NOT offered on radix-8 row plans: built for 8.8.8 it agreed with hv_fuse=0 on the emulator but not on
    the MI355X (image after 8 iterations: max |diff| 8e-8 on values of 0.07, i.e. 1e-6 relative) -- the compiler splits one
    packed FMA of the joined kernel into a multiply and an add, which it does not do in either half compiled alone, and an
    opaque copy of H V, of `a`, or a block boundary between the halves did not change that.  Until it compiles to its halves'
    instructions the plan must say so and the option must change nothing there."""
    rng = np.random.default_rng(508)
    psf = orc.synthetic_psf(1, 6, 508, 3, seed=508)
    y = rng.random((1, 6, 508, 3), dtype=np.float32)
    on = run(monkeypatch, psf, y, 1, [8])
    if "[static 8.8.8" not in on[2]:
        pytest.skip("the chooser's row plan for 512 points is not 8.8.8: " + on[2])
    assert ON not in on[2] and "64 lanes" in on[2], on[2]
    off = run(monkeypatch, psf, y, 0, [8])
    assert ON not in off[2], off[2]
    assert_same_bits(on[:2], off[:2], "radix 8")


def unrolled(backend, monkeypatch, fuse, grad):
    """UnrolledADMM at 5 x 4056 x 3, n_iter = 8, rising step sizes (test_on_against_off_with_a_per_iteration_schedule): the
    forward's output; with `grad` the gradients of one recorded forward + backward, at 6 x 4056 x 3 -- the nearest frame
    whose padded height is even, which reverse mode needs"""
    if grad:      # (the engine refuses backward() on an odd padded length: 5 rows pad to 9, 6 rows to 12)
        rng = np.random.default_rng(6)
        psf, y = orc.synthetic_psf(1, 6, 4056, 3, seed=6), rng.random((1, 6, 4056, 3), dtype=np.float32)
    else:
        psf, y = problem("flagship_rows")
    n = 8
    k = np.arange(n)
    sched = dict(mu1=1e-2 * (1 + 0.3 * k), mu2=1e-2 * (1 + 0.1 * k), mu3=1e-2 * (1 + 0.2 * k), tau=5e-3 * (1 + 0.05 * k))
    engine_opts(monkeypatch, **OPTS, hv_fuse=fuse)
    dev = backend.device
    net = lpa.UnrolledADMM(torch.from_numpy(psf).to(dev), n_iter=n)
    net.set_parameters(**sched)
    frames = torch.from_numpy(np.stack([y[0], y[0][::-1].copy()])[:, None]).to(dev)
    info = net._handle.plan_info()
    if not grad:
        with torch.no_grad():
            return {"out": net.forward(frames).cpu().numpy().copy()}, info
    frames.requires_grad_()
    w = torch.from_numpy(np.random.default_rng(3).random(tuple(frames.shape), dtype=np.float32)).to(dev)
    (net(frames) * w).sum().backward()
    grads = {"data": frames.grad.cpu().numpy().copy()}
    grads.update({name: p.grad.cpu().numpy().copy() for name, p in net.named_parameters()})
    assert len(grads) == 5, list(grads)
    return grads, info


@pytest.mark.parametrize("grad", [False, True], ids=["forward", "recorded_backward"])
def test_per_iteration_schedule(backend, monkeypatch, grad):
    """The fused rows do the X half of iteration it + 1: mu1 is that iteration's, mu1p this one's.  With every step size
    rising from one iteration to the next, the unrolled forward -- and the gradients of a recorded forward + backward --
    are the same bits on and off."""
    on, info1 = unrolled(backend, monkeypatch, 1, grad)
    off, info0 = unrolled(backend, monkeypatch, 0, grad)
    assert ON in info1 and ON not in info0, (info1, info0)
    for name in off:
        assert float(np.abs(off[name]).max()) > 0, name
        print(name, "max |diff|", float(np.abs(on[name] - off[name]).max()))
        assert np.array_equal(on[name], off[name]), name


@pytest.mark.parametrize("what", ["odd_offset", "paired_rows", "float64"])
def test_not_eligible(backend, monkeypatch, what):
    """No pair geometry, paired rows, the float64 build: today's kernels, and the option changes nothing."""
    if what == "odd_offset":
        (psf, y), opts, dtype = problem("odd_offset"), {}, None
    elif what == "paired_rows":
        rng = np.random.default_rng(24)
        psf, y = orc.synthetic_psf(1, 24, 32, 3, seed=24), rng.random((1, 24, 32, 3), dtype=np.float32)
        opts, dtype = dict(rows_half=None, k1_rows=0), None
    else:
        (psf, y), opts, dtype = problem("flagship_rows"), {}, "float64"
    on = run(monkeypatch, psf, y, 1, [8], dtype=dtype, **opts)
    off = run(monkeypatch, psf, y, 0, [8], dtype=dtype, **opts)
    assert ON not in on[2] and ON not in off[2], on[2]
    assert ("rows: paired" in on[2]) == (what == "paired_rows"), on[2]
    assert_same_bits(on[:2], off[:2], what)


def test_anchor_against_float64_oracle(backend, monkeypatch):
    (imgs, _, info), _ = on_off(backend, monkeypatch, "flagship_rows", [8])
    assert ON in info, info
    psf, y = problem("flagship_rows")
    o = orc.ADMMOracle(psf, dtype=torch.float64, **TV)
    o.set_data(y[0])
    want = np.asarray(o.apply(8))
    r = rel(imgs[0][0], want)
    print("H V rows on chip against the float64 oracle:", r)
    assert float(np.abs(want).max()) > 0 and r <= 1e-5, r


def test_byte_accounting(backend, monkeypatch):
    """lpc_kernel_bytes: forward + inverse rows move 2 x 4 x H x Wp x P bytes less -- the row of H V, out and back in --
    and the other four kernels the same."""
    psf, y = problem("flagship_rows")
    on = run(monkeypatch, psf, y, 1, [1])
    off = run(monkeypatch, psf, y, 0, [1])
    assert ON in on[2] and ON not in off[2], on[2]
    _, Hp, Wp, C = on[3]._padded_shape
    H, P = y.shape[1], y.shape[0] * C
    kb = lambda rec, k: rec._handle.kernel_bytes(_native.KERNEL_NAMES.index(k))     # noqa: E731
    rows = lambda rec: kb(rec, "row_fwd") + kb(rec, "row_inv")                        # noqa: E731
    print("rows on", rows(on[3]), "off", rows(off[3]))
    assert rows(on[3]) - rows(off[3]) == -2 * 4 * H * Wp * P
    for k in ("spatial", "col_a_fwd", "col_mid", "col_a_inv"):
        assert kb(on[3], k) == kb(off[3], k) and (kb(on[3], k) > 0 or k.startswith("col_a")), k
