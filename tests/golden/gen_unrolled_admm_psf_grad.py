#!/usr/bin/env python3
"""
PSF-gradient fixtures of unrolled ADMM from the REAL reference (read-only mount; runs ONLY in the build container, like
gen_unrolled_admm_grad.py).  Output: tests/golden/unrolled_admm_psf_grad_<case>.npz -- ``out64`` plus the gradient of
``(out * w).sum()`` w.r.t. a leaf ``psfs`` handed to the reference's own ``UnrolledADMM.forward(batch, psfs=...)`` (which
rebuilds its convolver from ``psfs`` and nothing else), once in float64 and once in float32 (``g_psf64`` / ``g_psf32``),
and the name of the source fixture.  Arrays only, no reference source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_unrolled_admm_psf_grad.py

The inputs are those of the EXISTING fixtures tests/golden/unrolled_admm_grad_<case>.npz (gen_unrolled_admm_grad.py):
``psf``, ``data``, ``w``, the schedule and ``n_iter`` are loaded from them, so the forward is the same -- asserted here: the
reference's ``out64`` equals the source fixture's bit for bit -- and the conditions asserted there (5 - 95 % of U non-zero
and of q positive from the second iteration on, no element on a kink) carry over.  Asserted here on the reference alone:
the yardstick rel(g_psf32, g_psf64) <= 5e-5 on the small cases (no kinks); the DiffuserCam-sized frame has 757 elements on a
kink in the float64 run and its yardstick is what the reference's float32 run gives, stored, as for its other gradients.

The five cases whose data has the PSF's channel count.  The reference refuses ``psfs`` when the data has fewer channels
than the PSF, so the gray-data / RGB-PSF case has no fixture: tests/test_unrolled_admm_psf_grad.py checks it against the
float64 restatement.  The DiffuserCam-sized case (270 x 480 x 3, B = 2, n = 5, closed-form inputs of longrun_inputs.py,
kinks allowed) stores longrun_inputs.samples() crops + lattice of ``g_psf64``, its max and the float32 yardstick, exactly
as gen_unrolled_admm_grad.py: c1_case stores ``out`` and ``g_data``.
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

from lensless.recon.unrolled_admm import UnrolledADMM  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
BASE = dict(mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-7)          # gen_unrolled_admm_grad.py
NAMES = ("mu1", "mu2", "mu3", "tau")
YARDSTICK_MAX = 5e-5
SMALL = ["19x27x1_b2", "16x20x3_b2", "24x32x1_b2", "48x20x1_b2", "24x40x1_b2"]


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


def run(psf, data, w, sched, n, dtype):
    tdt = torch.float64 if dtype == "float64" else torch.float32
    rec = UnrolledADMM(t(psf).to(tdt), dtype=dtype, n_iter=n, **BASE)
    with torch.no_grad():
        for k in NAMES:
            getattr(rec, f"_{k}_p").copy_(t(sched[k]))
    leaf = t(psf).to(tdt).requires_grad_()
    out = rec.forward(t(data).to(tdt), psfs=leaf)
    (out * t(w).to(tdt)).sum().backward()
    assert leaf.grad is not None and leaf.grad.shape == leaf.shape
    return out.detach().numpy().copy(), leaf.grad.numpy().copy()


def both(psf, data, w, sched, n, small):
    out64, g64 = run(psf, data, w, sched, n, "float64")
    _, g32 = run(psf, data, w, sched, n, "float32")
    yard = rel(g32, g64)
    assert not small or yard <= YARDSTICK_MAX, f"yardstick {yard}"
    return out64, g64, g32, yard


def small_case(case):
    source = "unrolled_admm_grad_" + case
    g = np.load(os.path.join(OUT, source + ".npz"))
    out64, g64, g32, yard = both(g["psf"], g["data"], g["w"], {k: g[k] for k in NAMES}, int(g["n_iter"]), small=True)
    assert np.array_equal(out64, g["out64"]), "the forward with psfs= is not the source fixture's"
    name = "unrolled_admm_psf_grad_" + case
    np.savez_compressed(os.path.join(OUT, name + ".npz"), out64=out64, g_psf64=g64, g_psf32=g32, source=source)
    print("wrote", name, "float32 reference: %.1e" % yard)


def c1_case():
    source = "unrolled_admm_grad_c1"
    g = np.load(os.path.join(OUT, source + ".npz"))
    B, H, W, C = (int(v) for v in g["shape"])
    seed, n = int(g["seed"]), int(g["n_iter"])
    psf = lin.psf12(1, H, W, C, 100 + seed)
    data = np.stack([lin.measurement(H, W, C, 10 * seed + b) for b in range(B)])[:, None]
    w = np.random.default_rng(300 + seed).random((B, 1, H, W, C), dtype=np.float32) - np.float32(0.5)
    for a, fp in ((psf, "fp_psf"), (data, "fp_data"), (w, "fp_w")):
        assert np.array_equal(lin.fingerprint(a), g[fp]), fp
    out64, g64, g32, yard = both(psf, data, w, {k: g[k] for k in NAMES}, n, small=False)
    parts = [lin.samples(out64[b, 0]) for b in range(B)]
    assert np.array_equal(np.stack([p[0] for p in parts]), g["out64_crops"]), "the forward is not the source fixture's"
    assert np.array_equal(np.stack([p[1] for p in parts]), g["out64_lattice"])
    crops, lattice = lin.samples(g64[0])
    name = "unrolled_admm_psf_grad_c1"
    np.savez_compressed(os.path.join(OUT, name + ".npz"), g_psf64_crops=crops, g_psf64_lattice=lattice,
                        g_psf64_max=np.abs(g64).max(), rel32_g_psf=yard, source=source)
    print("wrote", name, "float32 reference: %.1e" % yard)


if __name__ == "__main__":
    for case in sys.argv[1:] or SMALL + ["c1"]:
        c1_case() if case == "c1" else small_case(case)
