#!/usr/bin/env python3
"""
Gradient fixtures of unrolled FISTA from the REAL reference (read-only mount at /root/reference; runs ONLY in the build
container, see gen_golden.py).  Output: tests/golden/unrolled_fista_grad_*.npz -- inputs, the loss weights ``w``, and
``out`` plus the gradients of ``(out * w).sum()`` w.r.t. ``_alpha_p``, ``_tk_p`` and the batch from the reference's own
``forward()`` + ``backward()``, once in float64 and once in float32 (keys ``*64`` / ``*32``): the float32 run is the
yardstick of the float32 engine's tolerance (tests/test_unrolled_grad.py).  Arrays only, no reference source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_unrolled_grad.py

The float64 run counts the elements on the kink of the projection (|z_i| < 1e-5 max|z_i|, where float32 and float64
may legitimately take different branches; exact zeros excepted, they are zero in any precision) and stores the count as
``kink_count``, per call of the projection as ``kink_per_proj``.  For the three small cases it asserts that the count
is 0.  The DiffuserCam-sized case (270 x 480 x 3, B = 2, n = 5: 4.7 million projected elements) has a handful of such
elements with the seed used, and with that many elements every seed has some.  It is generated all the same and
compared without exclusions: an element that takes the other branch in float32 moves ``out`` and the gradients by less
than 1e-5 of its own scale, and the reference's own float32 run, the tests' yardstick, contains the same effect.
Its big arrays are stored as longrun_inputs.samples() crops + lattice of the float64 run; of the float32 run only the
distances to the float64 run over the WHOLE arrays are kept (``rel32_*``).
The small cases (non-negative PSF, measurement in [0, 1)) clamp under 1 % of the elements in every projection; the
coverage of ACTIVE masks lives in tests/test_unrolled_grad_sweep.py (signed measurement, torch.autograd as reference).
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", MagicMock())
sys.path.insert(0, os.environ.get("LENSLESS_REFERENCE", "/root/reference"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import longrun_inputs as lin  # noqa: E402

from lensless.recon.gd import non_neg  # noqa: E402
from lensless.recon.unrolled_fista import UnrolledFISTA  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
KINK = 1e-5


KINKS = []      # per call of the projection in the float64 run


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def run(psf, data, w, alpha, tk, n_iter, tk0, dtype):
    tdt = torch.float64 if dtype == "float64" else torch.float32

    def proj(z):     # every argument of the projection: z_0 .. z_{n-1} and y_n
        if dtype == "float64":
            a = z.detach().abs()       # (an exact 0 -- y_n where x_k and x_{k-1} were both clamped -- is 0 in any precision)
            KINKS.append(int(((a < KINK * float(a.max())) & (a > 0)).sum()))
        return non_neg(z)

    rec = UnrolledFISTA(t(psf).to(tdt), n_iter=n_iter, tk=tk0, dtype=dtype, proj=proj)
    with torch.no_grad():
        rec._alpha_p.copy_(t(alpha))
        rec._tk_p.copy_(t(tk))
    batch = t(data).to(tdt).requires_grad_()
    out = rec.forward(batch)
    (out * t(w).to(tdt)).sum().backward()
    return (out.detach().numpy().copy(), rec._alpha_p.grad.numpy().copy(), rec._tk_p.grad.numpy().copy(),
            batch.grad.numpy().copy())


def both(psf, data, w, n_iter, tk0, seed, allow_kinks=False):
    rng = np.random.default_rng(seed + 50)
    rec = UnrolledFISTA(t(psf), n_iter=n_iter, tk=tk0)
    c = psf.shape[-1]
    alpha = (rec._alpha_p.detach().numpy() * (0.6 + 0.4 * rng.random((n_iter, c)))).astype(np.float32)
    tk = (rec._tk_p.detach().numpy() * (1 + 0.2 * rng.random(n_iter + 1))).astype(np.float32)
    res = {}
    KINKS.clear()
    for dtype, tag in (("float64", "64"), ("float32", "32")):
        out, ga, gt, gb = run(psf, data, w, alpha, tk, n_iter, tk0, dtype)
        res.update({"out" + tag: out, "g_alpha" + tag: ga, "g_tk" + tag: gt, "g_data" + tag: gb})
    res["kink_count"] = sum(KINKS)
    res["kink_per_proj"] = np.array(KINKS)
    assert allow_kinks or sum(KINKS) == 0, "an element sits on the kink of the projection: pick another seed"
    return alpha, tk, res


def report(name, res):
    print("wrote", name, "kinks", res["kink_count"], {k: "%.1e" % rel(res[k + "32"], res[k + "64"]) for k in ("out", "g_alpha", "g_tk", "g_data")},
          "zeros in out: %.1f %%" % (100.0 * float((res["out64"] == 0).mean())))


def small_case(name, h, w_, c, batch, n_iter, tk0, seed, data_channels=None, data_scale=1.0):
    rng = np.random.default_rng(seed)
    psf = rng.random((1, h, w_, c)).astype(np.float32) ** 6
    psf /= np.linalg.norm(psf.ravel())
    data = (rng.random((batch, 1, h, w_, data_channels or c)) * data_scale).astype(np.float32)
    w = rng.standard_normal((batch, 1, h, w_, c)).astype(np.float32)
    alpha, tk, res = both(psf, data, w, n_iter, tk0, seed)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), psf=psf, data=data, w=w, alpha=alpha, tk=tk, n_iter=n_iter,
                        tk0=float(tk0), seed=seed, **res)
    report(name, res)


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


def c1_case(name, h=270, w_=480, c=3, batch=2, n_iter=5, tk0=1, seed=0):
    """DiffuserCam size; inputs in closed form (longrun_inputs.py), see the module docstring"""
    psf = lin.psf12(1, h, w_, c, 100 + seed)
    data = np.stack([lin.measurement(h, w_, c, 10 * seed + b) for b in range(batch)])[:, None]
    w = np.random.default_rng(300 + seed).random((batch, 1, h, w_, c), dtype=np.float32) - np.float32(0.5)
    alpha, tk, res = both(psf, data, w, n_iter, tk0, seed, allow_kinks=True)
    out = dict(kink_count=res["kink_count"], kink_per_proj=res["kink_per_proj"], alpha=alpha, tk=tk, n_iter=n_iter,
               tk0=float(tk0), seed=seed, shape=np.array([batch, h, w_, c]), fp_psf=lin.fingerprint(psf),
               fp_data=lin.fingerprint(data), fp_w=lin.fingerprint(w), g_alpha64=res["g_alpha64"], g_tk64=res["g_tk64"])
    for k in ("out", "g_alpha", "g_tk", "g_data"):
        out["rel32_" + k] = rel(res[k + "32"], res[k + "64"])
    for k in ("out", "g_data"):
        a = res[k + "64"]
        out[k + "64_max"] = np.abs(a).max()
        parts = [lin.samples(a[b, 0]) for b in range(batch)]
        out[k + "64_crops"] = np.stack([p[0] for p in parts])
        out[k + "64_lattice"] = np.stack([p[1] for p in parts])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    report(name, res)


if __name__ == "__main__":
    small_case("unrolled_fista_grad_24x32x3_b3", 24, 32, 3, batch=3, n_iter=7, tk0=1, seed=22)
    small_case("unrolled_fista_grad_19x27x1_b2", 19, 27, 1, batch=2, n_iter=5, tk0=2.5, seed=23)
    small_case("unrolled_fista_grad_20x28_gray_rgb", 20, 28, 3, batch=2, n_iter=6, tk0=1, seed=24, data_channels=1,
               data_scale=0.05)
    c1_case("unrolled_fista_grad_c1")
