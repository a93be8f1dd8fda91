#!/usr/bin/env python3
"""
Per-frame PSF fixtures from the REAL reference (read-only mount; runs ONLY in the build container, like
gen_unrolled_psf_grad.py).  Output: tests/golden/unrolled_{admm,fista}_psfs5d_<case>.npz -- the inputs and the output of the
reference's own ``UnrolledADMM.forward(batch, psfs=P5)`` / ``UnrolledFISTA.forward(batch, psfs=P5)`` with
``P5.shape == (B, 1, H, W, C)``, one PSF per measurement (trainable_recon.py:346-350 rebuilds the convolver from it,
rfft_convolve.py:84-117 pads and multiplies with the leading batch axis), once in float64 (``out64``) and once in float32
(``out32``, the yardstick).  Arrays only, no reference source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_per_frame_psf.py

Cases: 19 x 27 x 1 with B = 3 and 16 x 20 x 3 with B = 2, n = 4.  The solver is constructed from ``psf`` (another PSF than
any of ``psfs``): UnrolledFISTA takes its start value and the default ``_alpha_p`` from it and from nothing else
(unrolled_fista.py:57-72).  PSFs: ``synthetic_psf(1, H, W, C, seed + b)``; measurement ``rng.random``; ADMM step sizes
(1e-6, 1e-4, 4e-5, 2e-6) x the first four factors of tests/test_unrolled_admm_sweep.py.

Asserted here, on the reference alone: the batched forward equals the per-frame forwards
``forward(batch[b:b+1], psfs=P5[b])`` to 1e-13 (float64), differs from the one-PSF-for-all forward by more than 0.1, and
the float32 run is within 2.5e-6 of the float64 run.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", MagicMock())
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.environ.get("LENSLESS_REFERENCE", "/root/reference"))

from oracle.lensless_oracle import synthetic_psf  # noqa: E402

from lensless.recon.unrolled_admm import UnrolledADMM  # noqa: E402
from lensless.recon.unrolled_fista import UnrolledFISTA  # noqa: E402

N_ITER = 4
BASE = dict(mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-6)
FACTORS = dict(mu1=[1.0, 0.6, 1.5, 0.8], mu2=[0.7, 1.4, 2.0, 0.9], mu3=[1.8, 1.1, 0.5, 1.3], tau=[1.2, 1.7, 0.5, 0.9])
YARDSTICK_MAX = 2.5e-6
CASES = {"19x27x1_b3": dict(h=19, w=27, c=1, batch=3, seed=4100), "16x20x3_b2": dict(h=16, w=20, c=3, batch=2, seed=4200)}


def t(x, tdt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(tdt)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def solver(kind, psf, sched, dtype):
    """``sched``: the float32 values every run gets -- mu1, mu2, mu3, tau (ADMM) or alpha, tk (FISTA)"""
    tdt = torch.float64 if dtype == "float64" else torch.float32
    if kind == "admm":
        rec = UnrolledADMM(t(psf, tdt), dtype=dtype, n_iter=N_ITER, **BASE)
    else:
        rec = UnrolledFISTA(t(psf, tdt), n_iter=N_ITER, tk=1, dtype=dtype)
    with torch.no_grad():
        for k, v in sched.items():
            getattr(rec, f"_{k}_p").copy_(torch.from_numpy(v))
    return rec, tdt


def forward(kind, psf, sched, data, psfs, dtype):
    rec, tdt = solver(kind, psf, sched, dtype)
    with torch.no_grad():
        return rec.forward(t(data, tdt), psfs=t(psfs, tdt)).numpy().copy()


def case(name, h, w, c, batch, seed):
    rng = np.random.default_rng(seed)
    psf = synthetic_psf(1, h, w, c, seed + 100)
    psfs = np.stack([synthetic_psf(1, h, w, c, seed + b) for b in range(batch)])
    data = rng.random((batch, 1, h, w, c), dtype=np.float32)
    asched = {k: (np.float64(BASE[k]) * np.asarray(FACTORS[k])).astype(np.float32) for k in BASE}
    # the constructor's defaults of the float32 solver (unrolled_fista.py:60-78), as float32 values for both runs
    dflt = UnrolledFISTA(t(psf, torch.float32), n_iter=N_ITER, tk=1)
    fsched = dict(alpha=dflt._alpha_p.detach().numpy().astype(np.float32), tk=dflt._tk_p.detach().numpy().astype(np.float32))
    for kind in ("admm", "fista"):
        sched = fsched if kind == "fista" else asched
        out64 = forward(kind, psf, sched, data, psfs, "float64")
        out32 = forward(kind, psf, sched, data, psfs, "float32")
        assert out64.shape == (batch, 1, h, w, c), out64.shape
        for b in range(batch):
            one = forward(kind, psf, sched, data[b:b + 1], psfs[b], "float64")
            assert rel(one[0], out64[b]) <= 1e-13, (kind, name, b, rel(one[0], out64[b]))
        shared = forward(kind, psf, sched, data, psfs[0], "float64")
        moved = [rel(shared[b], out64[b]) for b in range(1, batch)]
        assert min(moved) > 0.1, (kind, name, moved)
        ys = [rel(out32[b], out64[b]) for b in range(batch)]
        assert max(ys) <= YARDSTICK_MAX, (kind, name, ys)
        np.savez_compressed(os.path.join(HERE, f"unrolled_{kind}_psfs5d_{name}.npz"), psf=psf, psfs=psfs, data=data,
                            n_iter=N_ITER, seed=seed, out64=out64, out32=out32,
                            **sched)
        print(f"wrote unrolled_{kind}_psfs5d_{name}: float32 against float64", " ".join(f"{y:.1e}" for y in ys),
              "| one PSF for all moves the other frames by", " ".join(f"{m:.2f}" for m in moved))


if __name__ == "__main__":
    for name in sys.argv[1:] or CASES:
        case(name, **CASES[name])
