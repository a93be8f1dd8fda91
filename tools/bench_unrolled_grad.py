#!/usr/bin/env python3
"""
Times one training step of UnrolledFISTA on the MI355X: DiffuserCam-sized frames (270 x 480 x 3), B = 8, float32.

    python tools/bench_unrolled_grad.py [--n 5 20] [--reps 30] [--package-root DIR] [--once] [--psf-grad]

Legs, each with warm-up and HIP events around every repetition (median, min, max in ms):
  (a) forward() under no_grad                       (--package-root: the same call on another checkout, e.g. the parent)
  (b) forward() with gradients: the recorded forward
  (c) backward() of (out * w).sum()
  (d) the same gradients from torch.autograd over a torch.fft restatement of the iteration, forward + backward
--psf-grad adds the PSF as a leaf (``rec._set_psf(p)`` once, ``p.requires_grad``):
  (e) backward() with the PSF gradient (its recorded forward is (b)'s)
  (f) torch.autograd over the restatement with the PSF as a leaf as well, forward + backward
--once: one recorded forward + backward per n and nothing else (for a kernel trace; with --psf-grad: with the PSF gradient).
Prints one JSON line per n.
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[5, 20])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--psf-grad", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import numpy as np
    import torch

    import lenslesspicam_amd as lpa

    dev = torch.device("cuda", 0)
    H, W, C, B = 270, 480, 3, args.batch
    rng = np.random.default_rng(0)
    psf = rng.random((1, H, W, C), dtype=np.float32) ** 12
    psf /= np.linalg.norm(psf)
    psf = torch.from_numpy(psf).to(dev)
    data = torch.from_numpy(rng.random((B, 1, H, W, C), dtype=np.float32)).to(dev)
    w = torch.from_numpy(rng.random((B, 1, H, W, C), dtype=np.float32) - 0.5).to(dev)
    trainable = hasattr(lpa.UnrolledFISTA, "release_tape")

    def timed(fn, setup=None):
        for _ in range(args.warmup):
            if setup:
                setup()
            fn()
        ms = []
        for _ in range(args.reps):
            if setup:
                setup()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}

    # the restatement: rfft2 of the padded frame, ifftshift + crop (RealFFTConvolve2D, pad=True, norm="ortho")
    Hp, Wp = 540, 960
    sh, sw = (Hp - H) // 2, (Wp - W) // 2
    Hs = torch.fft.rfft2(torch.nn.functional.pad(psf, (0, 0, sw, Wp - W - sw, sh, Hp - H - sh)), norm="ortho", dim=(-3, -2))

    def spectrum(p):
        return torch.fft.rfft2(torch.nn.functional.pad(p, (0, 0, sw, Wp - W - sw, sh, Hp - H - sh)), norm="ortho", dim=(-3, -2))

    def restated(batch, alpha_p, tk_p, n, Hs=Hs):
        def conv(x, adj):
            X = torch.fft.rfft2(torch.nn.functional.pad(x, (0, 0, sw, Wp - W - sw, sh, Hp - H - sh)), dim=(-3, -2))
            y = torch.fft.ifftshift(torch.fft.irfft2(X * (Hs.conj() if adj else Hs), dim=(-3, -2), s=(Hp, Wp)), dim=(-3, -2))
            return y[..., sh:sh + H, sw:sw + W, :]

        flat = psf.reshape(-1, C)
        y = (torch.ones_like(psf[None]) * ((flat.max(0).values + flat.min(0).values) / 2)).expand(B, -1, -1, -1, -1)
        xk = y
        a, t = alpha_p.abs(), tk_p.abs()
        for i in range(n):
            xn = torch.clamp(y - a[i] * conv(conv(y, False) - batch, True), min=0)
            y = xn + ((t[i] - 1) / t[i + 1]) * (xn - xk)
            xk = xn
        return torch.clamp(y, min=0)

    for n in args.n:
        rec = lpa.UnrolledFISTA(psf, n_iter=n)
        res = {"n_iter": n, "batch": B, "frame": [H, W, C], "package_root": args.package_root,
               "plan": rec._handle.plan_info() if hasattr(rec._handle, "plan_info") else ""}
        batch = data.clone().requires_grad_(trainable)
        if args.once:
            if args.psf_grad:
                rec._set_psf(psf.clone().requires_grad_())
            (rec(batch) * w).sum().backward()
            torch.cuda.synchronize()
            continue

        def fwd_nograd():
            with torch.no_grad():
                rec(data)

        res["a_forward_no_grad_ms"] = timed(fwd_nograd)
        if trainable:
            state = {}

            def fwd():
                state["loss"] = (rec(batch) * w).sum()

            res["b_recorded_forward_ms"] = timed(fwd)
            res["c_backward_ms"] = timed(lambda: state["loss"].backward(), setup=fwd)
            ap, tp = rec._alpha_p.detach().clone().requires_grad_(), rec._tk_p.detach().clone().requires_grad_()
            bt = data.clone().requires_grad_()
            res["d_torch_autograd_fwd_bwd_ms"] = timed(lambda: (restated(bt, ap, tp, n) * w).sum().backward())
            rec._alpha_p.grad = batch.grad = ap.grad = bt.grad = None
            (rec(batch) * w).sum().backward()
            (restated(bt, ap, tp, n) * w).sum().backward()
            res["check_rel_g_alpha"] = float((rec._alpha_p.grad - ap.grad).abs().max() / ap.grad.abs().max())
            res["check_rel_g_data"] = float((batch.grad - bt.grad).abs().max() / bt.grad.abs().max())
            assert res["check_rel_g_alpha"] < 1e-4 and res["check_rel_g_data"] < 1e-4, res     # the two paths time the same thing
            bc = res["b_recorded_forward_ms"]["median"] + res["c_backward_ms"]["median"]
            res["b_plus_c_ms"] = round(bc, 4)
            res["c_over_a"] = round(res["c_backward_ms"]["median"] / res["a_forward_no_grad_ms"]["median"], 3)
            res["d_over_b_plus_c"] = round(res["d_torch_autograd_fwd_bwd_ms"]["median"] / bc, 3)
            if args.psf_grad:
                pe, pl = psf.clone().requires_grad_(), psf.clone().requires_grad_()
                rec._set_psf(pe)
                res["e_backward_psf_ms"] = timed(lambda: state["loss"].backward(), setup=fwd)
                res["f_torch_autograd_psf_fwd_bwd_ms"] = timed(
                    lambda: (restated(bt, ap, tp, n, spectrum(pl)) * w).sum().backward())
                pe.grad = pl.grad = None
                (rec(batch) * w).sum().backward()
                (restated(bt, ap, tp, n, spectrum(pl)) * w).sum().backward()
                res["check_rel_g_psf"] = float((pe.grad - pl.grad).abs().max() / pl.grad.abs().max())
                assert res["check_rel_g_psf"] < 1e-4, res
                res["e_over_c"] = round(res["e_backward_psf_ms"]["median"] / res["c_backward_ms"]["median"], 3)
                be = res["b_recorded_forward_ms"]["median"] + res["e_backward_psf_ms"]["median"]
                res["f_over_b_plus_e"] = round(res["f_torch_autograd_psf_fwd_bwd_ms"]["median"] / be, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
