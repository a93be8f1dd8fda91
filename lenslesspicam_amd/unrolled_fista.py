"""
Unrolled FISTA on the MI355X engine: the iterations of the reference's ``UnrolledFISTA``
(``lensless/recon/unrolled_fista.py:18-106``) with per-iteration, per-channel steps ``alpha[i][c]`` and a
``t_k`` sequence, on batches -- inference and training.

``UnrolledFISTA`` is a ``torch.nn.Module`` like the reference's: ``_alpha_p`` (``(n_iter, C)``) and, with
``learn_tk``, ``_tk_p`` (``n_iter + 1``) are ``nn.Parameter`` s on the PSF's device, under the reference's names, so
``state_dict()`` round-trips with its checkpoints.  ``forward(batch)`` with autograd enabled and any of the parameters,
``batch``, the initial estimate or the PSF requiring a gradient runs as one ``torch.autograd.Function``: the forward is the
inference launch sequence with the handle recording its tape (``lpc_fista_record``), the backward one reverse sweep in
fused HIP kernels (``lpc_fista_backward`` / ``lpc_fista_backward_psf``, csrc/lpc_gd_bwd_kernels.h) plus the chain through ``abs`` and
``(t_i - 1) / t_{i+1}`` on ``n_iter``-sized tensors.  There is one tape per solver: ``backward()`` after a later
``forward()`` of the same object raises; a forward without gradients in between keeps the tape's memory
(``release_tape()`` gives it back).  Not differentiated (``NotImplementedError``, from ``backward()`` for the first two):
``depth > 1``, frames whose padded height or width is odd, ``proj`` other than ``non_neg``.  Inference takes any ``proj``:
``forward()`` without gradients then runs every iteration split at the projection (lpc_iterate_begin / lpc_iterate_end),
with the schedule's step and momentum factor of that iteration.

The PSF is an autograd input as well: ``forward(batch, psfs=p)`` with ``p.requires_grad``, or a ``p`` set earlier through
``_set_psf(p)``, gets ``dL/dp`` in ``p``'s shape, dtype and device from the same reverse sweep (the engine still works on
its detached device copy).  As in the reference's ``forward(batch, psfs=...)``, which rebuilds the convolver and nothing
else (``trainable_recon.py:337-350``), the default start value and the steps derived from the constructor's PSF are
constants.  The gradient costs a workspace of three spectra and one state array on top of the tape (include/lpc.h:
``lpc_fista_backward_psf``), allocated by the first backward that needs it and given back by ``release_tape()``.  One PSF
for the batch: per-frame PSFs (a 5-D ``psfs``) raise ``NotImplementedError`` from a forward that records
(unless the solver was built with ``per_frame_grad=True``, below).

Inference takes one PSF per measurement: ``forward(batch, psfs=P5)`` with ``P5.shape == (B,) + psf.shape`` under
``torch.no_grad()`` (or with nothing requiring a gradient) returns what B single-frame forwards with ``psfs=P5[b]`` return,
in one launch sequence (``lpc_set_psf_batch``).  ``P5`` stays current for later batches of B measurements until a 4-D
``psfs=`` or ``_set_psf``; the start value and ``_alpha_p`` stay the constructor's, as in the reference.  ``background=``
and ``dist.*`` sharding of ``psfs`` are not supported.

``UnrolledFISTA(psf, ..., per_frame_grad=True)`` trains with one PSF per measurement: a forward that records takes a 5-D
``psfs`` (handed in now, or current since an earlier forward) instead of refusing it, and ``backward()`` fills the
parameters (summed over the frames, as autograd does), ``batch.grad``, the initial estimate's gradient and, when
``psfs.requires_grad``, ``psfs.grad`` of shape ``(B, D, H, W, C)`` with nothing summed over the batch
(``lpc_per_frame_grad``; the same workspace).  Every other refusal stays.  The default is ``per_frame_grad=False``: every
message, workspace size and output bit is unchanged.

Pre- / post-processor networks are not taken by the constructor: the measurement and the PSF get gradients, so compose
them in torch around ``forward()`` -- ``post(rec(pre(batch), psfs=psf + net(psf)))`` trains all of it.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._unrolled import _Taped, _grad_like, _meta
from .gd import FISTA, non_neg


class _UnrolledFISTAFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rec, batch, alpha_p, tk_p, init, psf):
        out = rec._run(batch, record=True, push_init=init is not None)
        ctx.rec, ctx.gen = rec, rec._tape_gen
        ctx.batch_meta, ctx.init_meta, ctx.psf_meta = _meta(batch), _meta(init), _meta(psf)
        ctx.save_for_backward(alpha_p, tk_p)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        rec = ctx.rec
        alpha_p, tk_p = ctx.saved_tensors
        if int(rec._psf_shape[0]) > 1:
            raise NotImplementedError("UnrolledFISTA.backward: depth > 1 is not implemented")
        if rec._padded_shape[1] % 2 or rec._padded_shape[2] % 2:
            raise NotImplementedError(
                f"UnrolledFISTA.backward: padded frame {rec._padded_shape[1]} x {rec._padded_shape[2]} has an odd "
                "length (convolve and deconvolve are not each other's adjoints there)")
        rec._check_tape(ctx.gen)
        h, n, C = rec._handle, rec._n_iter, int(rec._psf_shape[3])
        need_b, need_a, need_t, need_i, need_p = ctx.needs_input_grad[1:6]
        g = rec._to_dev(grad_out)
        bshape = ctx.batch_meta[0]
        g_data = rec._empty((bshape[0],) + bshape[2:]) if need_b else None
        g_init = rec._empty(tuple(g.shape)) if need_i else None
        g_a, g_c = rec._empty((n, C)), rec._empty((n,))
        # (a 5-D leaf: one PSF per measurement, one gradient each -- nothing summed over the batch)
        frames = (bshape[0],) if need_p and len(ctx.psf_meta[0]) == 5 else ()
        g_psf = rec._empty(frames + tuple(int(v) for v in rec._psf_shape)) if need_p else None
        ptrs = (g.data_ptr(), None if g_data is None else g_data.data_ptr(), g_a.data_ptr(), g_c.data_ptr(),
                None if g_init is None else g_init.data_ptr())
        if need_p:
            h.fista_backward_psf(*ptrs, g_psf.data_ptr(), rec._stream())
        else:
            h.fista_backward(*ptrs, rec._stream())
        # through |.| and c_i = (t_i - 1) / t_{i+1}, formed as _push_schedule forms them
        with torch.enable_grad():
            ap = alpha_p.detach().requires_grad_(need_a)
            tp = tk_p.detach().requires_grad_(need_t)
            alpha, coef = rec._schedule_of(ap, tp)
            ga = torch.autograd.grad(alpha, ap, g_a.to(device=alpha.device, dtype=alpha.dtype))[0] if need_a else None
            gt = torch.autograd.grad(coef, tp, g_c.to(device=coef.device, dtype=coef.dtype))[0] if need_t else None
        gb = _grad_like(g_data[:, None], ctx.batch_meta) if need_b else None
        gi = None
        if need_i:
            one = ctx.init_meta[0][0] != g_init.shape[0]      # one estimate for the batch
            gi = _grad_like(g_init.sum(0, keepdim=True) if one else g_init, ctx.init_meta)
        gp = _grad_like(g_psf, ctx.psf_meta) if need_p else None
        return None, gb, ga, gt, gi, gp


class UnrolledFISTA(_Taped, FISTA, torch.nn.Module):
    _record_method, _solver = "fista_record", "UnrolledFISTA"
    _PER_FRAME_PSFS = True      # the schedule and the pinned start value replace what plain FISTA derives from its one PSF

    def _before_psfs(self):
        self._push_schedule()       # (lpc_set_psf_batch refuses a gradient-descent handle without one)

    def __init__(self, psf, n_iter=5, dtype=None, proj=non_neg, learn_tk=True, tk=1, skip_unrolled=False,
                 per_frame_grad=False, **kwargs):
        assert isinstance(psf, torch.Tensor), "UnrolledFISTA takes torch tensors, like the reference"
        torch.nn.Module.__init__(self)
        super().__init__(psf, dtype=dtype, proj=proj, tk=float(tk), n_iter=n_iter, **kwargs)
        C = int(self._psf_shape[3])
        self.skip_unrolled = skip_unrolled
        self.per_frame_grad = bool(per_frame_grad)      # opt in: a forward that records takes a 5-D psfs
        # unrolled_fista.py:60-72: alpha initialised to 1.8 / max|H* H| per channel, for every iteration
        a0 = torch.as_tensor(np.asarray(self._alpha if not isinstance(self._alpha, torch.Tensor)
                                        else self._alpha.cpu().numpy(), dtype=np.float32))
        alpha = (torch.ones(n_iter, C, dtype=torch.float32) * a0).to(device=psf.device, dtype=self._tdtype)
        tks = [float(tk)]                                     # unrolled_fista.py:75-78
        for i in range(n_iter):
            tks.append((1 + np.sqrt(1 + 4 * tks[i] ** 2)) / 2)
        tk_p = torch.Tensor(tks).to(psf.device)
        # unrolled_fista.py:64-80: parameters unless skip_unrolled; t_k only when it is learnt
        self._alpha_p = alpha if skip_unrolled else torch.nn.Parameter(alpha)
        self._tk_p = torch.nn.Parameter(tk_p) if learn_tk and not skip_unrolled else tk_p
        self._sched_key = None
        self._tape_init()
        # unrolled_fista.py:55-59: `_image_init` is computed here, from this PSF, and reset() (:91-96) reuses it whatever PSF
        # forward(batch, psfs=...) or _set_psf() made current since -- unlike gd.py:94-112, which follows the PSF.  The
        # handle computed it in lpc_set_psf; every handle of this solver is pinned to these values.
        self._start_dev = self._empty((C,))
        self._handle.get_state("start_value", self._start_dev.data_ptr(), self._stream())
        self._handle.set_start_value(self._start_dev.data_ptr(), self._stream())

    def _after_new_handle(self):
        super()._after_new_handle()
        self._handle.set_start_value(self._start_dev.data_ptr(), self._stream())
        self._handle.reset(self._stream())      # (lpc_set_psf reset this handle before the start value was pinned)

    def set_parameters(self, alpha=None, tk=None):
        with torch.no_grad():
            if alpha is not None:
                a = torch.as_tensor(np.asarray(alpha, dtype=np.float32))
                assert tuple(a.shape) == tuple(self._alpha_p.shape)
                self._alpha_p.copy_(a)
            if tk is not None:
                t = torch.as_tensor(np.asarray(tk, dtype=np.float32)).flatten()
                assert t.numel() == self._n_iter + 1
                self._tk_p.copy_(t)

    def load_state_dict(self, state, strict=False):
        self.set_parameters(alpha=state["_alpha_p"].detach().cpu().numpy() if "_alpha_p" in state else None,
                            tk=state["_tk_p"].detach().cpu().numpy() if "_tk_p" in state else None)

    def _schedule_of(self, alpha_p, tk_p):
        """(alpha, coef) as the handle gets them: alpha in the solver's precision, coef in float32 arithmetic like
        unrolled_fista.py:104 (the reference keeps ``_tk_p`` in float32 whatever the dtype)"""
        alpha = torch.abs(alpha_p).to(self._tdtype)            # unrolled_fista.py:98-100 (positivity)
        tk = torch.abs(tk_p).to(torch.float32)
        return alpha, (tk[:-1] - 1) / tk[1:]

    def _push_schedule(self):
        """Hands the schedule to the handle -- only when the parameters changed or the handle is new (an upload
        is a blocking host -> device copy; ``forward()`` calls ``reset()`` for every batch)."""
        key = (self._handle, self._alpha_p, self._alpha_p._version, self._tk_p, self._tk_p._version)
        if self._sched_key is not None and len(key) == len(self._sched_key) and \
                all(a is b if isinstance(a, torch.Tensor) else a == b for a, b in zip(key, self._sched_key)):
            return
        with torch.no_grad():
            alpha, coef = self._schedule_of(self._alpha_p, self._tk_p)
        self._handle.set_fista_schedule(alpha.tolist(), coef.tolist(), self._stream())
        self._sched_key = key

    def reset(self, tk=None, batch_size=None):
        if getattr(self, "_alpha_p", None) is not None:
            self._push_schedule()
        super().reset()

    def _run(self, batch, record=False, push_init=False):
        self._data = batch
        self._upload_data()
        if push_init:
            self._push_initial_estimate()      # the current values of an estimate that is being learnt
        self._push_schedule()
        self._new_tape(record)
        self.reset()
        self._iterate(self._n_iter)
        return self._form_image()

    def forward(self, batch, psfs=None, background=None):
        """``batch``: (B, D, H, W, C) -> (B, D, H, W, C) after exactly ``n_iter`` unrolled iterations."""
        self._check_forward_args(batch, psfs, background)
        init = self._initial_est if isinstance(self._initial_est, torch.Tensor) else None
        new_psf = psfs if isinstance(psfs, torch.Tensor) and psfs.dim() == 4 else self._psf
        frames = self._active_psfs(psfs)      # per_frame_grad: the 5-D PSFs this forward runs with, and differentiates
        train = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                                for t in (batch, self._alpha_p, self._tk_p, init, new_psf, psfs, frames))
        if train and self._per_frame(psfs):
            self._refuse_per_frame_training(psfs)
        self._take_psfs(batch, psfs)
        psf = self._psf if frames is None else frames
        psf = psf if isinstance(psf, torch.Tensor) and psf.requires_grad else None
        if train:
            self._refuse_per_frame_training(None)
            if self._hook:
                raise NotImplementedError("UnrolledFISTA: only proj=non_neg is differentiated")
            if init is not None and not init.requires_grad:
                init = None
            return _UnrolledFISTAFunction.apply(self, batch, self._alpha_p, self._tk_p, init, psf)
        return self._run(batch)
