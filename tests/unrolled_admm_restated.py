"""
What tests/test_unrolled_admm_grad.py and tests/golden/gen_unrolled_admm_grad.py share: the forward iteration of unrolled
ADMM (lensless/recon/unrolled_admm.py:133-240) restated in torch.fft for torch.autograd -- nothing of the engine, nothing
of oracle/ --, the kink band of its two non-smooth points, and the option sets that select each launch-plan family.

The restatement takes the step sizes as the engine gets them: ``abs(p)`` as float32, then in the working dtype, with
``tau / mu2`` divided in the working dtype (the reference divides the two float32 values in float32).
"""
import numpy as np
import torch

from unrolled_restated import F64_TOL, KINK, rec_padded, rel  # noqa: F401  (re-exported)

NAMES = ("mu1", "mu2", "mu3", "tau")


def finite_diff(x):
    return torch.stack((torch.roll(x, 1, dims=-3) - x, torch.roll(x, 1, dims=-2) - x), dim=x.dim())


def finite_diff_adj(u):
    return (torch.roll(u[..., 0], -1, dims=-3) - u[..., 0]) + (torch.roll(u[..., 1], -1, dims=-2) - u[..., 1])


def restated_admm(psf, data, mu1_p, mu2_p, mu3_p, tau_p, n, dtype=torch.float64, teeth=()):
    """``clip(crop(V_n), 0)`` after ``n`` iterations, for torch.autograd; ``data`` may have one channel against a
    three-channel PSF.  Also returns, detached and per iteration, (s, theta, q): the arguments of the soft threshold and of
    the W clamp.  ``teeth``: deliberate mistakes of a backward pass -- "soft" / "clamp": the soft threshold / the W clamp
    is the identity in the backward; "rdiv": R_divmat is a constant (the dR/dm terms are dropped)."""
    psf, data = psf.to(dtype), data.to(dtype)
    D, H, W, C = psf.shape
    Hp, Wp = rec_padded(H), rec_padded(W)
    sh, sw = (Hp - H) // 2, (Wp - W) // 2

    def pad(v):
        o = torch.zeros(v.shape[:-3] + (Hp, Wp, C), dtype=v.dtype)
        o[..., sh:sh + H, sw:sw + W, :] = v
        return o

    Hs = torch.fft.rfft2(pad(psf), dim=(-3, -2))          # norm="backward"
    HH = (Hs.conj() * Hs).abs()
    gram = torch.zeros((D, Hp, Wp, C), dtype=dtype)
    gram[0, 0, 0] = 4
    gram[0, 0, 1] = gram[0, 0, -1] = gram[0, 1, 0] = gram[0, -1, 0] = -1
    G = torch.fft.rfft2(gram, dim=(-3, -2)).abs()

    def conv(x, adj):
        X = torch.fft.rfft2(x, dim=(-3, -2)) * (Hs.conj() if adj else Hs)
        return torch.fft.ifftshift(torch.fft.irfft2(X, dim=(-3, -2), s=(Hp, Wp)), dim=(-3, -2))

    def through(y, x, name):     # y = f(x); with the tooth `name` the backward sees the identity
        return x + (y - x).detach() if name in teeth else y

    # (float32 leaves, the reference's parameters, pass the float32 cast; float64 leaves hold float32 values already and
    # skip it, so that their gradients are not rounded to float32 on the way back)
    m1, m2, m3, tau = ((p.abs().to(torch.float32) if p.dtype == torch.float32 else p.abs()).to(dtype)
                       for p in (mu1_p, mu2_p, mu3_p, tau_p))
    b = pad(data)
    mask = pad(torch.ones_like(psf))
    B = data.shape[0]
    v = torch.zeros((B, D, Hp, Wp, C), dtype=dtype)
    hv, xi, rho = torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)
    pv = torch.zeros(v.shape + (2,), dtype=dtype)
    eta = torch.zeros_like(pv)
    args = []
    for i in range(n):
        theta = tau[i] / m2[i]
        s = pv + eta / m2[i]
        U = through(torch.sign(s) * torch.clamp(s.abs() - theta, min=0), s, "soft")
        X = (xi + m1[i] * hv + b) / (mask + m1[i])
        q = rho / m3[i] + v
        Wv = through(torch.clamp(q, min=0), q, "clamp")
        rk = (m3[i] * Wv - rho) + finite_diff_adj(m2[i] * U - eta) + conv(m1[i] * X - xi, True)
        R = 1.0 / (m1[i] * HH + m2[i] * G + m3[i])
        if "rdiv" in teeth:
            R = R.detach()
        v = torch.fft.irfft2(R * torch.fft.rfft2(rk, dim=(-3, -2)), dim=(-3, -2), s=(Hp, Wp))
        hv, pv = conv(v, False), finite_diff(v)
        xi = xi + m1[i] * (hv - X)
        eta = eta + m2[i] * (pv - U)
        rho = rho + m3[i] * (v - Wv)
        args.append((s.detach(), float(theta.detach()), q.detach()))
    return torch.clamp(v[..., sh:sh + H, sw:sw + W, :], min=0), args


def activity(args):
    """per iteration: (fraction of U non-zero, fraction of q positive, elements on a kink).  An element is on a kink if
    ``||s| - theta| < KINK max|s|`` or ``|q| < KINK max|q|``; exact zeros of s and q are excepted (iteration 0 is all
    exact zeros: zero in any precision)."""
    out = []
    for s, theta, q in args:
        a = s.abs()
        k = int(((a - theta).abs() < KINK * float(a.max())).logical_and(a > 0).sum()) if float(a.max()) > 0 else 0
        k += int((q.abs() < KINK * float(q.abs().max())).logical_and(q != 0).sum()) if float(q.abs().max()) > 0 else 0
        out.append((float((a > theta).double().mean()), float((q > 0).double().mean()), k))
    return out


def restated_grads(psf, data, w, sched, n, dtype=torch.float64, teeth=(), leaf=torch.float64):
    """out and the gradients of ``(out * w).sum()`` w.r.t. the four parameter vectors (leaves of dtype ``leaf`` holding
    the schedule's float32 values) and the batch, as numpy arrays"""
    ps = [torch.from_numpy(np.asarray(sched[k], dtype=np.float32)).to(leaf).requires_grad_() for k in NAMES]
    batch = torch.from_numpy(np.asarray(data)).to(dtype).requires_grad_()
    out, args = restated_admm(torch.from_numpy(np.asarray(psf)), batch, *ps, n, dtype=dtype, teeth=teeth)
    (out * torch.from_numpy(np.asarray(w)).to(dtype)).sum().backward()
    res = {"out": out.detach().numpy(), "g_data": batch.grad.numpy()}
    # (a tooth can cut a parameter off the graph altogether: its gradient is then 0)
    res.update({"g_" + k: (torch.zeros_like(p) if p.grad is None else p.grad).numpy() for k, p in zip(NAMES, ps)})
    return res, args


# launch plans of the forward (after CASES of tests/test_unrolled_admm_sweep.py): the kink-free single-channel fixture whose
# frame takes the plan, the options, and what plan_info() must hold (``f32`` / ``f64``: in that build only)
MOD = {"jit_min_points": 0}
SPLIT = {"tile_budget": 512, "col_t": 4}
F_RT, F_MOD, F_SPLIT, F_WIDE = ("unrolled_admm_grad_19x27x1_b2", "unrolled_admm_grad_24x32x1_b2",
                                 "unrolled_admm_grad_48x20x1_b2", "unrolled_admm_grad_24x40x1_b2")
PLANS = {
    "rt": dict(fixture=F_RT, opts={}, info=["run-time plans", "stand-alone image-domain kernel"]),
    "rt_w4": dict(fixture=F_MOD, opts={}, info=["run-time plans", "stand-alone image-domain kernel"]),
    "mod": dict(fixture=F_MOD, opts=MOD, info=["TV / W half and X half inside the forward rows", "row transforms skipped"]),
    "mod_tiled": dict(fixture=F_MOD, opts={**MOD, "k1_rows": 0}, info=["tiled TV / W kernel + X half"]),
    "mod_nohalf": dict(fixture=F_MOD, opts={**MOD, "k1_half": 0},
                       info=["TV / W half and X half inside the forward rows", "row transforms skipped"]),
    "rows_half": dict(fixture=F_MOD, opts={**MOD, "rows_half": 1}, info=["half-length 32"]),
    "gterms": dict(fixture=F_MOD, opts={**MOD, "g_plane": 0}, info=["gram as row + column terms"]),
    "split_reg": dict(fixture=F_SPLIT, opts={**SPLIT, "split_n2": 24}, info=["4 x 24 split"], f32=["middle in registers"]),
    "split_lds": dict(fixture=F_SPLIT, opts={**SPLIT, "split_n2": 12}, info=["8 x 12 split"]),
    "split_mod": dict(fixture=F_SPLIT, opts={**SPLIT, "split_n2": 12, **MOD}, info=["pass A [static"]),
    "seq": dict(fixture=F_WIDE, opts={"mid_seq": 1, "tile_budget": 768, **MOD}, info=[],
                f32=["one spectrum at a time, pair-line spectra"], f64=["T = 8, LDS middle [static 8.6]"]),
    "pair": dict(fixture=F_WIDE, opts={"mid_seq": 0, "tile_budget": 768, **MOD}, info=[], f32=["pair-line spectra"]),
}
F64_PLANS = ["rt", "mod", "split_reg", "split_mod", "seq"]      # the other float64 modules are the same code
