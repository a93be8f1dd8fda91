#!/usr/bin/env python3
"""
PSF-gradient fixture of unrolled FISTA from the REAL reference (read-only mount; runs ONLY in the build container, like
gen_unrolled_grad.py).  Output: tests/golden/unrolled_fista_psf_grad_12x30x3_b2.npz -- inputs, the loss weights ``w``, and
``out`` plus the gradient of ``(out * w).sum()`` w.r.t. a leaf ``psfs`` handed to the reference's own
``UnrolledFISTA.forward(batch, psfs=...)`` (which rebuilds its convolver from ``psfs`` and nothing else: the start value
stays the constructor's), once in float64 and once in float32 (keys ``*64`` / ``*32``).  Arrays only, no reference source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_unrolled_psf_grad.py

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_unrolled_psf_grad.py unrolled_fista_psf_swap_12x30x3_b2

A second fixture, unrolled_fista_psf_swap_12x30x3_b2.npz: the solver is constructed from ``psf`` and ``forward(batch, psfs=p2)``
gets ANOTHER PSF as the leaf, so the start value (the constructor's, from ``psf``) and the convolver (from ``p2``) come from
different PSFs; it holds ``p2`` as well, and the gradients are those w.r.t. ``p2``.  Same conditions on the projections.

One small case, 12 x 30 x 3, B = 2, n = 4, with the SIGNED measurement of tests/test_unrolled_grad_sweep.py (its case
``12x30``, same seed and recipe).  The float64 run asserts, per call of the projection, that no element sits on the kink
(0 < |z| < 1e-5 max|z|) and that between 20 % and 80 % of the elements are clamped.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", MagicMock())
sys.path.insert(0, os.environ.get("LENSLESS_REFERENCE", "/root/reference"))

from lensless.recon.gd import non_neg  # noqa: E402
from lensless.recon.unrolled_fista import UnrolledFISTA  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
KINK = 1e-5


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


def run(psf, data, w, alpha, tk, n_iter, dtype, clamped, psfs=None):
    """``psfs``: the PSF handed to forward() as the leaf (default: the constructor's own values)"""
    tdt = torch.float64 if dtype == "float64" else torch.float32

    def proj(z):     # every argument of the projection: z_0 .. z_{n-1} and y_n
        if dtype == "float64":
            a = z.detach().abs()
            kinks = int(((a < KINK * float(a.max())) & (a > 0)).sum())
            assert kinks == 0, "an element sits on the kink of the projection: pick another seed"
            clamped.append(float((z.detach() <= 0).double().mean()))
            assert 0.2 <= clamped[-1] <= 0.8, f"projection {len(clamped) - 1} clamps {100 * clamped[-1]:.1f} %"
        return non_neg(z)

    rec = UnrolledFISTA(t(psf).to(tdt), n_iter=n_iter, tk=1, dtype=dtype, proj=proj)
    with torch.no_grad():
        rec._alpha_p.copy_(t(alpha))
        rec._tk_p.copy_(t(tk))
    leaf = t(psf if psfs is None else psfs).to(tdt).requires_grad_()
    out = rec.forward(t(data).to(tdt), psfs=leaf)
    (out * t(w).to(tdt)).sum().backward()
    assert leaf.grad is not None and leaf.grad.shape == leaf.shape
    return out.detach().numpy().copy(), leaf.grad.numpy().copy()


def case(name, h, w_, c, batch, n_iter, seed, p2_seed=None, p2_scale=1.0):
    """``p2_seed``: the solver is constructed from ``psf`` and forward() gets a second PSF, ``p2`` (same recipe, that seed,
    times ``p2_scale``), as ``psfs``: the start value stays the one of ``psf``"""
    rng = np.random.default_rng(seed)
    psf = rng.random((1, h, w_, c)).astype(np.float32) ** 6
    psf /= np.linalg.norm(psf.ravel())
    data = (rng.random((batch, 1, h, w_, c)) - 0.5).astype(np.float32)
    w = rng.standard_normal((batch, 1, h, w_, c)).astype(np.float32)
    rng = np.random.default_rng(seed + 50)
    rec = UnrolledFISTA(t(psf), n_iter=n_iter, tk=1)
    alpha = (rec._alpha_p.detach().numpy() * (0.6 + 0.4 * rng.random((n_iter, c)))).astype(np.float32)
    tk = (rec._tk_p.detach().numpy() * (1 + 0.2 * rng.random(n_iter + 1))).astype(np.float32)
    res, clamped, p2 = {}, [], None
    if p2_seed is not None:
        p2 = np.random.default_rng(p2_seed).random((1, h, w_, c)).astype(np.float32) ** 6
        p2 /= np.linalg.norm(p2.ravel())
        p2 *= np.float32(p2_scale)
        res["p2"] = p2
    for dtype, tag in (("float64", "64"), ("float32", "32")):
        res["out" + tag], res["g_psf" + tag] = run(psf, data, w, alpha, tk, n_iter, dtype, clamped, psfs=p2)
    assert len(clamped) == n_iter + 1
    np.savez_compressed(os.path.join(OUT, name + ".npz"), psf=psf, data=data, w=w, alpha=alpha, tk=tk, n_iter=n_iter,
                        seed=seed, clamped=np.array(clamped), **res)
    print("wrote", name, "clamped", " ".join(f"{100 * f:.0f}%" for f in clamped),
          {k: "%.1e" % rel(res[k + "32"], res[k + "64"]) for k in ("out", "g_psf")})


CASES = {
    "unrolled_fista_psf_grad_12x30x3_b2": dict(h=12, w_=30, c=3, batch=2, n_iter=4, seed=2000),
    # a PSF swap: constructed from the PSF above, forward(batch, psfs=p2) (tests/test_psf_swap.py: P2_SEED, P2_SCALE)
    "unrolled_fista_psf_swap_12x30x3_b2": dict(h=12, w_=30, c=3, batch=2, n_iter=4, seed=2000, p2_seed=99, p2_scale=0.7),
}

if __name__ == "__main__":
    for name in sys.argv[1:] or CASES:      # (no argument: every fixture)
        case(name, **CASES[name])
