#!/usr/bin/env python3
"""
Times one training step of UnrolledFISTA (or, with --algo admm, UnrolledADMM) on the MI355X: DiffuserCam-sized frames
(270 x 480 x 3), B = 8, float32.

    python tools/bench_unrolled_grad.py [--algo fista|admm] [--n 5 20] [--reps 30] [--package-root DIR] [--once] [--psf-grad]

Legs, each with warm-up and HIP events around every repetition (median, min, max in ms):
  (a) forward() under no_grad                       (--package-root: the same call on another checkout, e.g. the parent)
  (b) forward() with gradients: the recorded forward
  (c) backward() of (out * w).sum()
  (d) the same gradients from torch.autograd over a torch.fft restatement of the iteration, forward + backward
--psf-grad adds the PSF as a leaf (``rec._set_psf(p)`` once, ``p.requires_grad``):
  (e) backward() with the PSF gradient (its recorded forward is (b)'s)
  (f) torch.autograd over the restatement with the PSF as a leaf as well, forward + backward
--once: one recorded forward + backward per n and nothing else (for a kernel trace; with --psf-grad: with the PSF gradient).
--algo admm: legs (a) - (d) for UnrolledADMM (its restatement: the iteration of unrolled_admm.py:181-234 in torch.fft), plus
  (g) a device-to-device copy of 16 padded state arrays: the copy rate the kernels of the reverse mode are compared with
and the algorithmic bytes one launch of k_admm_bwd_step / k_admm_bwd_replay / k_admm_bwd_psf_acc moves (their times come
from a kernel trace of a --once run).  With --psf-grad (``UnrolledADMM(..., psf_grad=True)``, ``rec._set_psf(p)``) legs (e)
and (f) as above; (b) - (d) are then measured on the same solver BEFORE the PSF becomes a leaf.
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
    ap.add_argument("--algo", choices=["fista", "admm"], default="fista")
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

    Hp, Wp = 540, 960
    sh, sw = (Hp - H) // 2, (Wp - W) // 2
    if args.algo == "admm":
        return admm_legs(args, lpa, torch, timed, psf, data, w, (H, W, C, B, Hp, Wp, sh, sw))
    # the restatement: rfft2 of the padded frame, ifftshift + crop (RealFFTConvolve2D, pad=True, norm="ortho")
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


def admm_legs(args, lpa, torch, timed, psf, data, w, geom):
    H, W, C, B, Hp, Wp, sh, sw = geom
    base = dict(mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-7)
    names = ("mu1", "mu2", "mu3", "tau")
    factors = dict(mu1=[1.0, 0.6, 1.5, 0.8, 2.0, 0.5], mu2=[0.7, 1.4, 2.0, 0.9, 0.55, 1.2],
                   mu3=[1.8, 1.1, 0.5, 1.3, 0.75, 1.0], tau=[1.2, 1.7, 0.5, 0.9, 2.0, 0.65])
    trainable = hasattr(lpa.UnrolledADMM, "release_tape")

    def pad(v):
        return torch.nn.functional.pad(v, (0, 0, sw, Wp - W - sw, sh, Hp - H - sh))

    psf_grad = args.psf_grad and trainable
    gram = torch.zeros((1, Hp, Wp, C), device=psf.device)
    gram[0, 0, 0] = 4
    gram[0, 0, 1] = gram[0, 0, -1] = gram[0, 1, 0] = gram[0, -1, 0] = -1
    G = torch.fft.rfft2(gram, dim=(-3, -2)).abs()
    mask = pad(torch.ones_like(psf))

    def psi(x):
        return torch.stack((torch.roll(x, 1, dims=-3) - x, torch.roll(x, 1, dims=-2) - x), dim=x.dim())

    def psi_t(u):
        return (torch.roll(u[..., 0], -1, dims=-3) - u[..., 0]) + (torch.roll(u[..., 1], -1, dims=-2) - u[..., 1])

    Hs0 = torch.fft.rfft2(pad(psf), dim=(-3, -2))
    HH0 = (Hs0.conj() * Hs0).abs()

    def restated(batch, ps, n, p=None):      # p: the PSF as a leaf (its spectrum is then part of the graph)
        Hs = Hs0 if p is None else torch.fft.rfft2(pad(p), dim=(-3, -2))
        HH = HH0 if p is None else (Hs.conj() * Hs).abs()

        def conv(x, adj):
            X = torch.fft.rfft2(x, dim=(-3, -2)) * (Hs.conj() if adj else Hs)
            return torch.fft.ifftshift(torch.fft.irfft2(X, dim=(-3, -2), s=(Hp, Wp)), dim=(-3, -2))

        m1, m2, m3, tau = (q.abs() for q in ps)
        b = pad(batch)
        v = torch.zeros((B, 1, Hp, Wp, C), device=psf.device)
        hv, xi, rho = torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)
        pv = torch.zeros(v.shape + (2,), device=psf.device)
        eta = torch.zeros_like(pv)
        for i in range(n):
            s = pv + eta / m2[i]
            U = torch.sign(s) * torch.clamp(s.abs() - tau[i] / m2[i], min=0)
            X = (xi + m1[i] * hv + b) / (mask + m1[i])
            Wv = torch.clamp(rho / m3[i] + v, min=0)
            rk = (m3[i] * Wv - rho) + psi_t(m2[i] * U - eta) + conv(m1[i] * X - xi, True)
            R = 1.0 / (m1[i] * HH + m2[i] * G + m3[i])
            v = torch.fft.irfft2(R * torch.fft.rfft2(rk, dim=(-3, -2)), dim=(-3, -2), s=(Hp, Wp))
            hv, pv = conv(v, False), psi(v)
            xi = xi + m1[i] * (hv - X)
            eta = eta + m2[i] * (pv - U)
            rho = rho + m3[i] * (v - Wv)
        return torch.clamp(v[..., sh:sh + H, sw:sw + W, :], min=0)

    for n in args.n:
        rec = lpa.UnrolledADMM(psf, n_iter=n, **base, **({"psf_grad": True} if psf_grad else {}))
        rec.set_parameters(**{k: [base[k] * factors[k][i % 6] for i in range(n)] for k in names})
        batch = data.clone().requires_grad_(trainable)
        if args.once:
            if psf_grad:
                rec._set_psf(psf.clone().requires_grad_())
            (rec(batch) * w).sum().backward()
            torch.cuda.synchronize()
            continue
        R, R0 = 4.0 * Hp * Wp * B * C, 4.0 * H * W * B * C
        res = {"algo": "admm", "n_iter": n, "batch": B, "frame": [H, W, C], "package_root": args.package_root,
               "plan": rec._handle.plan_info(),
               # step: reads V_i, V_i+1, rb, hv, hv', hr, xi, rho, xib, rhob, eta (2), etab (2) + y; writes xib, rhob,
               # etab (2), r_sp, a + g_b read and written.  replay: reads V, HV (2 each), xi, eta (2), rho + y; writes 4
               "bytes_step": 20 * R + 3 * R0, "bytes_replay": 12 * R + R0,
               # PSF-gradient accumulate: reads four work spectra of B C planes, the PSF spectrum and the accumulator (C
               # planes each), writes the accumulator; complex64 half spectra of Hp x (Wp / 2 + 1) points
               "bytes_psf_acc": 8.0 * Hp * (Wp // 2 + 1) * (4 * B * C + 3 * C)}

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
            ps = [getattr(rec, f"_{k}_p").detach().clone().requires_grad_() for k in names]
            bt = data.clone().requires_grad_()
            res["d_torch_autograd_fwd_bwd_ms"] = timed(lambda: (restated(bt, ps, n) * w).sum().backward())
            src = torch.empty(int(8 * R / 4), dtype=torch.float32, device=psf.device)
            dst = torch.empty_like(src)
            res["g_copy_16R_ms"] = timed(lambda: dst.copy_(src))
            res["copy_TBps"] = round(16 * R / res["g_copy_16R_ms"]["median"] * 1e-9, 3)
            for p in ps + [bt, batch] + [getattr(rec, f"_{k}_p") for k in names]:
                p.grad = None
            (rec(batch) * w).sum().backward()
            (restated(bt, ps, n) * w).sum().backward()
            for k, p in zip(names, ps):
                got = getattr(rec, f"_{k}_p").grad
                res["check_rel_g_" + k] = float((got - p.grad).abs().max() / p.grad.abs().max())
            res["check_rel_g_data"] = float((batch.grad - bt.grad).abs().max() / bt.grad.abs().max())
            assert all(v < 1e-2 for k, v in res.items() if k.startswith("check_rel")), res   # the two paths time the same thing
            bc = res["b_recorded_forward_ms"]["median"] + res["c_backward_ms"]["median"]
            res["b_plus_c_ms"] = round(bc, 4)
            res["c_over_a"] = round(res["c_backward_ms"]["median"] / res["a_forward_no_grad_ms"]["median"], 3)
            res["d_over_b_plus_c"] = round(res["d_torch_autograd_fwd_bwd_ms"]["median"] / bc, 3)
            if psf_grad:
                pe, pl = psf.clone().requires_grad_(), psf.clone().requires_grad_()
                rec._set_psf(pe)
                res["e_backward_psf_ms"] = timed(lambda: state["loss"].backward(), setup=fwd)
                res["f_torch_autograd_psf_fwd_bwd_ms"] = timed(lambda: (restated(bt, ps, n, pl) * w).sum().backward())
                pe.grad = pl.grad = None
                (rec(batch) * w).sum().backward()
                (restated(bt, ps, n, pl) * w).sum().backward()
                res["check_rel_g_psf"] = float((pe.grad - pl.grad).abs().max() / pl.grad.abs().max())
                assert res["check_rel_g_psf"] < 1e-2, res
                res["e_over_c"] = round(res["e_backward_psf_ms"]["median"] / res["c_backward_ms"]["median"], 3)
                be = res["b_recorded_forward_ms"]["median"] + res["e_backward_psf_ms"]["median"]
                res["b_plus_e_ms"] = round(be, 4)
                res["f_over_b_plus_e"] = round(res["f_torch_autograd_psf_fwd_bwd_ms"]["median"] / be, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
