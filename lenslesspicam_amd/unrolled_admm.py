"""
Unrolled ADMM on the MI355X engine: the camera-inversion stage of the reference's ``UnrolledADMM``
(``lensless/recon/unrolled_admm.py:20-240``, "LeADMM") -- per-iteration step sizes ``mu1[i], mu2[i], mu3[i], tau[i]``
and batched measurements -- inference and training.

The arithmetic is the ADMM kernels' own: the fused prox/update kernel takes the previous
iteration's parameters for the pending dual updates and the current ones for the prox, and the
spectral solve forms ``R_divmat[i]`` on the fly, so a schedule costs nothing per iteration.

``UnrolledADMM`` is a ``torch.nn.Module`` like the reference's: ``_mu1_p, _mu2_p, _mu3_p, _tau_p`` (``n_iter`` float32
values each) are ``nn.Parameter`` s on the PSF's device, under the reference's names and in its order, so ``state_dict()``
round-trips with its checkpoints (``skip_unrolled=True`` keeps them plain tensors).  ``forward(batch)`` with autograd
enabled and a parameter or ``batch`` requiring a gradient runs as one ``torch.autograd.Function``: the forward is the
inference launch sequence with the handle keeping its iterates (``lpc_admm_record``), the backward a replay of the duals
and one reverse sweep in fused HIP kernels (``lpc_admm_backward``, csrc/lpc_admm_bwd_kernels.h) plus the chain through
``abs`` and the float32 cast on ``n_iter``-sized tensors.  There is one tape per solver: ``backward()`` after a later
``forward()`` of the same object raises; a forward without gradients in between keeps the tape's memory
(``release_tape()`` gives it back) and is the inference path, bit for bit.  The parameters require a gradient by default,
so ANY ``forward()`` outside ``torch.no_grad()`` records: it allocates the tape, ``6 n + 11`` padded state arrays of the
batch (include/lpc.h: ``lpc_admm_record``; 41 arrays for n = 5) -- run inference
under ``no_grad`` or with ``skip_unrolled=True``.  What such a forward returns carries a graph; so that code which only
wants the image (``out.cpu().numpy()``) keeps working, it is a ``torch.Tensor`` subclass (``_Estimate``) whose NumPy
conversion detaches -- the subclass travels with every tensor derived from it, the loss included, and is a plain tensor in
every other respect.  Not differentiated (``NotImplementedError``;
from ``backward()`` for ``depth > 1``, frames whose padded height or width is odd and an initial estimate that asks for no
gradient, so that their forward under autograd stays what it was -- it keeps no tape): the PSF unless the solver was
built with ``psf_grad=True`` (``psfs=`` or a PSF requiring a gradient), per-frame PSFs (a 5-D ``psfs``) unless it was built with
``per_frame_grad=True``, the initial estimate, a custom ``psi`` and a denoiser.

Inference takes one PSF per measurement: ``forward(batch, psfs=P5)`` with ``P5.shape == (B,) + psf.shape`` under
``torch.no_grad()`` (or with nothing requiring a gradient) returns what B single-frame forwards with ``psfs=P5[b]`` return,
in one launch sequence (``lpc_set_psf_batch``: the handle holds ``B D C`` PSF spectra).  ``P5`` stays current for later
batches of B measurements, like the convolver the reference rebuilds and keeps (``trainable_recon.py:346-350``), until a
4-D ``psfs=`` or ``_set_psf``; a forward that records refuses it (unless ``per_frame_grad=True``, below).  ``background=`` and ``dist.*`` sharding of ``psfs`` are
not supported.

``UnrolledADMM(psf, ..., psf_grad=True)`` makes the PSF an autograd input as well: ``forward(batch, psfs=p)`` with
``p.requires_grad``, or a ``p`` set earlier through ``_set_psf(p)``, gets ``dL/dp`` in ``p``'s shape, dtype and device,
summed over the batch, from the same reverse sweep (``lpc_admm_backward_psf``: three cross terms per iteration -- through
``H V``, through ``HT`` inside ``r_k`` and through ``R_divmat`` -- accumulated in ONE spectrum of C planes, one inverse
transform at the end; the engine still works on its detached device copy of the PSF).  It costs a workspace of
``4 P + C`` spectrum planes on top of the tape (include/lpc.h), allocated by the first backward that needs it and given
back by ``release_tape()``.  When nothing of the PSF requires a gradient the backward is ``lpc_admm_backward``, bit for
bit.  ``norm`` must be ``"backward"`` (the default) for this gradient; one PSF for the batch.  The default is
``psf_grad=False``: every refusal above is unchanged.

``UnrolledADMM(psf, ..., per_frame_grad=True)`` trains with one PSF per measurement: a forward that records takes a 5-D
``psfs`` (handed in now, or current since an earlier forward) instead of refusing it, and ``backward()`` fills the
parameters (summed over the frames, as autograd does), ``batch.grad`` and -- with ``psf_grad=True``, ``norm="backward"``
and ``psfs.requires_grad`` -- ``psfs.grad`` of shape ``(B, D, H, W, C)``, PSF b's own gradient in slice b, nothing summed
over the batch (``lpc_per_frame_grad``; the workspace's accumulator grows from C to ``P = B C`` spectrum planes).  Frame b
of such a step has the bits of the single-frame step with ``psfs=P5[b]``.  Every other refusal stays; ``dist.*`` sharding
of ``psfs`` and ``background=`` stay unsupported.  The default is ``per_frame_grad=False``: every message, workspace size
and output bit is unchanged.

Pre- / post-processor networks are not taken by the constructor: the measurement (and with ``psf_grad=True`` the PSF)
gets a gradient, so compose them in torch around ``forward()`` -- ``post(rec(pre(batch), psfs=psf + net(psf)))`` trains
all of it.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._unrolled import _Estimate, _Taped, _grad_like, _meta      # noqa: F401 (_Estimate: imported from here too)
from .admm import ADMM

_NAMES = ("_mu1_p", "_mu2_p", "_mu3_p", "_tau_p")


class _UnrolledADMMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rec, batch, mu1_p, mu2_p, mu3_p, tau_p, psf=None):
        out = rec._run(batch, record=rec._backward_refusal() is None)
        ctx.rec, ctx.gen = rec, rec._tape_gen
        ctx.batch_meta, ctx.psf_meta = _meta(batch), _meta(psf)
        ctx.save_for_backward(mu1_p, mu2_p, mu3_p, tau_p)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        rec = ctx.rec
        # (refused here, not in forward(): with the parameters requiring a gradient by default, a forward under autograd
        # is what inference code written for the reference does as well; such a forward records nothing)
        why = rec._backward_refusal()
        if why is not None:
            raise NotImplementedError("UnrolledADMM.backward: " + why)
        rec._check_tape(ctx.gen)
        n = rec._n_iter
        need_b = ctx.needs_input_grad[1]
        need_p = ctx.psf_meta is not None and ctx.needs_input_grad[6]
        g = rec._to_dev(grad_out)
        bshape = ctx.batch_meta[0]
        g_data = rec._empty((bshape[0],) + bshape[2:]) if need_b else None
        g_par = rec._empty((4, n))
        ptrs = (g.data_ptr(), None if g_data is None else g_data.data_ptr()) + tuple(g_par[k].data_ptr() for k in range(4))
        if need_p:      # (a 5-D leaf: one PSF per measurement, one gradient each -- nothing summed over the batch)
            frames = (bshape[0],) if len(ctx.psf_meta[0]) == 5 else ()
            g_psf = rec._empty(frames + tuple(int(v) for v in rec._psf_shape))
            rec._handle.admm_backward_psf(*ptrs, g_psf.data_ptr(), rec._stream())
        else:      # (nothing of the PSF asks for a gradient: the parameter-only sweep, its bits and its cost)
            rec._handle.admm_backward(*ptrs, rec._stream())
        # through |.| and the float32 cast, formed as _push_schedule forms them
        grads = []
        for k, p in enumerate(ctx.saved_tensors):
            if not ctx.needs_input_grad[2 + k]:
                grads.append(None)
                continue
            with torch.enable_grad():
                q = p.detach().requires_grad_()
                v = rec._schedule_of(q)
                grads.append(torch.autograd.grad(v, q, g_par[k].to(device=v.device, dtype=v.dtype))[0])
        gb = _grad_like(g_data[:, None], ctx.batch_meta) if need_b else None
        gp = _grad_like(g_psf, ctx.psf_meta) if need_p else None
        return (None, gb) + tuple(grads) + (gp,)


class UnrolledADMM(_Taped, ADMM, torch.nn.Module):
    _record_method, _solver = "admm_record", "UnrolledADMM"

    def __init__(self, psf, dtype=None, n_iter=5, mu1=1e-6, mu2=1e-5, mu3=4e-5, tau=0.0001, psi=None,
                 psi_adj=None, psi_gram=None, pad=False, norm="backward", skip_unrolled=False, psf_grad=False,
                 per_frame_grad=False, **kwargs):
        for key in ("pre_process", "post_process", "background_network", "psf_network", "compensation"):
            if kwargs.get(key) is not None:
                raise NotImplementedError(f"{key}: learned components are outside the hot path (compose them in torch "
                                          "around forward(): the measurement gets a gradient)")
        assert isinstance(psf, torch.Tensor), "UnrolledADMM takes torch tensors, like the reference"
        torch.nn.Module.__init__(self)
        super().__init__(psf, dtype=dtype, mu1=mu1, mu2=mu2, mu3=mu3, tau=tau, psi=psi, psi_adj=psi_adj,
                         psi_gram=psi_gram, pad=pad, norm=norm, n_iter=n_iter, **kwargs)
        self.skip_unrolled = skip_unrolled
        self.psf_grad = bool(psf_grad)      # opt in: a PSF that requires a gradient is differentiated, not refused
        self.per_frame_grad = bool(per_frame_grad)      # opt in: a forward that records takes a 5-D psfs
        # unrolled_admm.py:82-99: same attribute names as the reference so that checkpoints' state_dict entries can be
        # assigned; parameters unless skip_unrolled
        for name, val in zip(_NAMES, (mu1, mu2, mu3, tau)):
            v = torch.ones(n_iter, dtype=torch.float32, device=psf.device) * val
            setattr(self, name, v if skip_unrolled else torch.nn.Parameter(v))
        self._tape_init()
        self._push_schedule()

    def set_parameters(self, mu1=None, mu2=None, mu3=None, tau=None):
        """Per-iteration values (length n_iter each), e.g. from a trained LeADMM checkpoint; copied in place."""
        with torch.no_grad():
            for name, val in zip(_NAMES, (mu1, mu2, mu3, tau)):
                if val is not None:
                    v = torch.as_tensor(np.asarray(val, dtype=np.float32)).flatten()
                    assert v.numel() == self._n_iter, f"{name}: expected {self._n_iter} values"
                    getattr(self, name).copy_(v)

    def load_state_dict(self, state, strict=False):
        """Accepts the unrolled parameters of a reference checkpoint; everything else is ignored."""
        self.set_parameters(**{k: state[f"_{k}_p"].detach().cpu().numpy()
                               for k in ("mu1", "mu2", "mu3", "tau") if f"_{k}_p" in state})

    @staticmethod
    def _schedule_of(p):
        # unrolled_admm.py:140-144: the learnt values enter through torch.abs(), as float32
        return torch.abs(p).to(torch.float32)

    def _push_schedule(self):
        """Hands the current values to the handle, at every reset: 4 n floats, read from the tensors themselves, so that
        a write no version counter sees (``p.data.clamp_()``) is never missed."""
        with torch.no_grad():
            vals = [self._schedule_of(getattr(self, n)).cpu().numpy().astype(np.float64) for n in _NAMES]
        self._handle.set_admm_schedule(*vals)

    def reset(self, batch_size=None):
        if getattr(self, "_tau_p", None) is not None:      # (the base constructor resets before the parameters exist)
            self._push_schedule()
        super().reset()

    def _run(self, batch, record=False):
        self._data = batch
        self._upload_data()
        self._new_tape(record)
        self.reset()
        self._iterate(self._n_iter)
        return self._form_image()

    def _backward_refusal(self):
        """why ``backward()`` will refuse this solver, or None -- known before the forward runs, which then keeps no tape"""
        if int(self._psf_shape[0]) > 1:
            return "depth > 1 is not implemented"
        if self._padded_shape[1] % 2 or self._padded_shape[2] % 2:
            return (f"padded frame {self._padded_shape[1]} x {self._padded_shape[2]} has an odd length (the spectral step "
                    "and the convolve / deconvolve pair are not self-adjoint there)")
        if self._initial_est is not None:
            return "training with an initial estimate is not implemented"
        return None

    def _refuse_gradients(self, batch, psfs):
        """what lpc_admm_backward does not differentiate, refused before anything runs"""
        if psfs is not None or (isinstance(self._psf, torch.Tensor) and self._psf.requires_grad):
            if not self.psf_grad:
                raise NotImplementedError("UnrolledADMM: the gradient with respect to the PSF is not implemented")
            if self._norm != "backward":
                raise NotImplementedError(f"UnrolledADMM: the gradient with respect to the PSF is implemented for "
                                          f"norm=\"backward\" only (this solver has norm=\"{self._norm}\")")
        if isinstance(self._initial_est, torch.Tensor) and self._initial_est.requires_grad:
            raise NotImplementedError("UnrolledADMM: the gradient with respect to the initial estimate is not implemented")
        if self._custom_psi is not None or self._pnp is not None:
            raise NotImplementedError("UnrolledADMM: a custom psi and a denoiser are not differentiated")

    def forward(self, batch, psfs=None, background=None):
        """``batch``: (B, D=1, H, W, C) measurements -> (B, D, H, W, C) estimates after exactly
        ``n_iter`` unrolled iterations (trainable_recon.py:297-405 without the learned stages)."""
        self._check_forward_args(batch, psfs, background)
        params = [getattr(self, n) for n in _NAMES]
        psf_grad = (isinstance(psfs, torch.Tensor) and psfs.requires_grad) or \
            (isinstance(self._psf, torch.Tensor) and self._psf.requires_grad)
        frames = self._active_psfs(psfs)      # per_frame_grad: the 5-D PSFs this forward runs with, and differentiates
        psf_grad = psf_grad or (frames is not None and frames.requires_grad)
        init_grad = isinstance(self._initial_est, torch.Tensor) and self._initial_est.requires_grad
        train = torch.is_grad_enabled() and (psf_grad or init_grad or any(t.requires_grad for t in [batch] + params))
        if train:
            if self._per_frame(psfs):      # (a 4-D psfs below returns to one PSF: only the PSFs of THIS forward count)
                self._refuse_per_frame_training(psfs)
            self._refuse_gradients(batch, (frames if psfs is None else psfs) if psf_grad else None)
        self._take_psfs(batch, psfs)
        if train:
            self._refuse_per_frame_training(None)
            psf = self._psf if frames is None else frames
            psf = psf if self.psf_grad and isinstance(psf, torch.Tensor) and psf.requires_grad else None
            return _UnrolledADMMFunction.apply(self, batch, *params, psf).as_subclass(_Estimate)
        return self._run(batch)

    def _form_image(self, out=None):
        # unrolled_admm.py:236-240 clips OUT of place (no state mutation): read the state directly
        B = self._handle_batch
        D, Hp, Wp, C = self._padded_shape
        out_arg, out = out, self._empty((B, D, Hp, Wp, C))
        self._handle.get_state("image_est", out.data_ptr(), self._stream())
        sh, sw = (int(v) for v in self._start_idx)
        H, W = int(self._psf_shape[1]), int(self._psf_shape[2])
        res = torch.clip(out[:, :, sh:sh + H, sw:sw + W, :], min=0.0).contiguous()
        if out_arg is not None:
            out_arg.copy_(res)
        return self._to_user(res)
