"""
What tests/test_unrolled_grad.py and tests/test_unrolled_grad_sweep.py share: the forward iteration of unrolled FISTA
restated in torch.fft for torch.autograd (nothing of the engine, nothing of oracle/), the padded length, the distance the
bounds are stated in, and the option sets that select each reverse row kernel family.
"""
import numpy as np
import torch

F64_TOL = 1e-11
KINK = 1e-5      # tests/golden/gen_unrolled_grad.py: |z| < KINK * max|z| is "on the kink" of the projection (exact zeros excepted)


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def rec_padded(n):
    m = 2 * n - 1
    while True:
        r = m
        for p in (2, 3, 5):
            while r % p == 0:
                r //= p
        if r == 1:
            return m
        m += 1


def _spectrum(psf, dtype):
    """(pad, crop window, rfft2 of the padded PSF) of rfft_convolve.py:110-117 in ``dtype``"""
    psf = psf.to(dtype)
    D, H, W, C = psf.shape
    Hp, Wp = rec_padded(H), rec_padded(W)
    sh, sw = (Hp - H) // 2, (Wp - W) // 2

    def pad(v):
        o = torch.zeros(v.shape[:-3] + (Hp, Wp, v.shape[-1]), dtype=v.dtype)
        o[..., sh:sh + H, sw:sw + W, :] = v
        return o

    return pad, (Hp, Wp, sh, sw), torch.fft.rfft2(pad(psf), norm="ortho", dim=(-3, -2))


def default_steps(psf, n, tk0=1.0):
    """the constructor's defaults (gd.py:107-112, unrolled_fista.py:60-78): alpha = 1.8 / max|H* H| per channel for every
    iteration, t_{i+1} = (1 + sqrt(1 + 4 t_i^2)) / 2; float32 arrays (n, C) and (n + 1,)"""
    Hs = _spectrum(psf, torch.float64)[2]
    a0 = 1.8 / (Hs.conj() * Hs).abs().reshape(-1, psf.shape[-1]).max(0).values
    tks = [float(tk0)]
    for i in range(n):
        tks.append((1 + np.sqrt(1 + 4 * tks[i] ** 2)) / 2)
    return np.tile(a0.numpy().astype(np.float32), (n, 1)), np.asarray(tks, dtype=np.float32)


def restated(psf, data, alpha_p, tk_p, n, init=None, dtype=torch.float64, proj=None):
    """the five formula lines of the forward iteration in torch.fft, in ``dtype`` (t_k and the momentum factor in float32
    like unrolled_fista.py:104), for torch.autograd.  ``data`` may have one channel against a three-channel PSF (the
    broadcast of ``- self._data``).  ``proj``: the projection (unrolled_fista.py:104 and the read-out, :80-81); None is
    non-negativity.  Returns the output and, detached, every argument of the projection: z_0 .. z_{n-1} and y_n."""
    if proj is None:
        proj = lambda v: torch.clamp(v, min=0)  # noqa: E731
    psf, data = psf.to(dtype), data.to(dtype)
    D, H, W, C = psf.shape
    pad, (Hp, Wp, sh, sw), Hs = _spectrum(psf, dtype)

    def conv(x, adj):
        X = torch.fft.rfft2(pad(x), dim=(-3, -2)) * (Hs.conj() if adj else Hs)
        y = torch.fft.ifftshift(torch.fft.irfft2(X, dim=(-3, -2), s=(Hp, Wp)), dim=(-3, -2))
        return y[..., sh:sh + H, sw:sw + W, :]

    if init is None:
        flat = psf.reshape(-1, C)
        init = (torch.ones_like(psf[None]) * ((flat.max(0).values + flat.min(0).values) / 2))
    y = init.to(dtype).expand(data.shape[0], -1, -1, -1, -1)
    xk = y
    a, t = alpha_p.abs().to(dtype), tk_p.abs()
    args = []
    for i in range(n):
        z = y - a[i] * conv(conv(y, False) - data, True)
        xn = proj(z)
        y = xn + ((t[i] - 1) / t[i + 1]) * (xn - xk)
        xk = xn
        args.append(z.detach())
    args.append(y.detach())
    return proj(y), args


PLANS = {"rows_half": ({"rows_half": 1}, "reverse rows: half-length, run-time plan"),
         "rows_paired": ({"rows_half": 0}, "reverse rows: paired, run-time plan"),
         "no_static": ({"no_static": 1}, "run-time plans (no_static)"),
         "module": ({"jit_min_points": 0, "rows_half": 1}, "reverse rows: plan module")}
