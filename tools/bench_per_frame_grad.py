#!/usr/bin/env python3
"""
Times training steps with one PSF per measurement on the MI355X (protocol of profiles/unrolled_admm_grad.md: 270 x 480 x 3,
B = 8, n = 5, float32, recorded forward + backward of ``(out * w).sum()``, HIP events, warmed up).

    python tools/bench_per_frame_grad.py [--algo admm|fista] [--psf-grad] [--rounds 5] [--reps 6] [--package-root DIR]

Legs, alternated round by round in one process (median of each round's repetitions; then median, min and max over rounds):
  shared     one PSF for the batch: ``rec(batch, psfs=p)`` + backward          (the only leg on a checkout without the switch,
             e.g. the parent commit given as --package-root)
  per_frame  ``rec(batch, psfs=P5)`` + backward, ``P5`` (B, 1, H, W, C)        (``per_frame_grad=True``)
  detour     what it replaces: B single-frame steps on a solver of one frame, ``rec1(batch[b:b+1], psfs=P5[b])`` + backward
--psf-grad: the PSFs are leaves (ADMM: ``psf_grad=True``).  Also a device copy of the size the ADMM accumulate moves
(``copy_ms`` for ``bytes_psf_acc_frames``: 7 P spectrum planes -- four work spectra, Hs, the accumulator read and written).
Prints one JSON line.
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=["admm", "fista"], default="admm")
    ap.add_argument("--psf-grad", action="store_true")
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import numpy as np
    import torch

    import lenslesspicam_amd as lpa

    dev = torch.device("cuda", 0)
    H, W, C, B, n = 270, 480, 3, args.batch, args.n
    rng = np.random.default_rng(0)

    def psf_of():
        p = rng.random((1, H, W, C), dtype=np.float32) ** 12
        return torch.from_numpy(p / np.linalg.norm(p)).to(dev)

    psf = psf_of()
    P5 = torch.stack([psf_of() for _ in range(B)])
    data = torch.from_numpy(rng.random((B, 1, H, W, C), dtype=np.float32)).to(dev)
    w = torch.from_numpy(rng.random((B, 1, H, W, C), dtype=np.float32) - 0.5).to(dev)
    cls = lpa.UnrolledADMM if args.algo == "admm" else lpa.UnrolledFISTA
    switch = "per_frame_grad" in cls.__init__.__code__.co_varnames

    def solver(**kw):
        if args.algo == "admm":
            base = dict(mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-7)
            factors = dict(mu1=[1.0, 0.6, 1.5, 0.8, 2.0, 0.5], mu2=[0.7, 1.4, 2.0, 0.9, 0.55, 1.2],
                           mu3=[1.8, 1.1, 0.5, 1.3, 0.75, 1.0], tau=[1.2, 1.7, 0.5, 0.9, 2.0, 0.65])
            rec = cls(psf, n_iter=n, **base, **({"psf_grad": True} if args.psf_grad else {}), **kw)
            rec.set_parameters(**{k: [base[k] * factors[k][i % 6] for i in range(n)] for k in base})
            return rec
        return cls(psf, n_iter=n, **kw)

    def leaf(p):
        return p.clone().requires_grad_(args.psf_grad)

    batch = data.clone().requires_grad_()
    rec = solver(**({"per_frame_grad": True} if switch else {}))
    rec1 = solver()
    p_shared, p_frames, p_single = leaf(P5[0]), leaf(P5), [leaf(P5[b]) for b in range(B)]
    singles = [data[b:b + 1].clone().requires_grad_() for b in range(B)]

    def shared():
        (rec(batch, psfs=p_shared) * w).sum().backward()

    def per_frame():
        (rec(batch, psfs=p_frames) * w).sum().backward()

    def detour():
        for b in range(B):
            (rec1(singles[b], psfs=p_single[b]) * w[b:b + 1]).sum().backward()

    legs = {"shared": shared}
    if switch:
        legs.update(per_frame=per_frame, detour=detour)

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return sorted(ms)[len(ms) // 2]

    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            rounds[k].append(timed(fn, args.reps))
    res = {"algo": args.algo, "psf_grad": args.psf_grad, "n_iter": n, "batch": B, "frame": [H, W, C],
           "package_root": args.package_root, "switch": switch, "plan": rec._handle.plan_info()}
    for k, v in rounds.items():
        v = sorted(v)
        res[k + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
    if switch:
        res["detour_over_per_frame"] = round(res["detour_ms"]["median"] / res["per_frame_ms"]["median"], 3)
        res["per_frame_over_shared"] = round(res["per_frame_ms"]["median"] / res["shared_ms"]["median"], 3)
        Hp, Wp = 540, 960
        nbytes = 8.0 * Hp * (Wp // 2 + 1) * 7 * B * C
        src = torch.empty(int(nbytes / 8), dtype=torch.float32, device=dev)      # a copy reads and writes: half the size
        dst = torch.empty_like(src)
        for _ in range(args.warmup):
            dst.copy_(src)
        res["bytes_psf_acc_frames"] = nbytes
        res["copy_ms"] = round(timed(lambda: dst.copy_(src), 20), 4)
        res["copy_TBps"] = round(nbytes / res["copy_ms"] * 1e-9, 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
