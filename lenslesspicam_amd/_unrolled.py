"""
What ``UnrolledADMM`` and ``UnrolledFISTA`` share of their training surface: the book-keeping of the one tape a solver
has (``_Taped``), the refusals every ``forward()`` starts with, the layout of a gradient handed back to autograd, and the
tensor ``UnrolledADMM.forward()`` returns under autograd (``_Estimate``).
"""
from __future__ import annotations

import torch


class _Estimate(torch.Tensor):
    """What ``forward()`` returns under autograd.  The parameters require a gradient by default, so code that only wants
    the image -- ``out.cpu().numpy()``, ``np.asarray(out)`` -- gets a tensor with a graph behind it where it used to get
    a plain one; this one still converts to NumPy (of its detached values), and is an ordinary tensor otherwise."""

    def numpy(self, *args, **kwargs):
        return self.detach().as_subclass(torch.Tensor).numpy(*args, **kwargs)

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype, copy=False)


class _Taped:
    """One tape per solver, on the handle of the current batch size.  ``_record_method`` names that handle's switch
    (``"admm_record"`` / ``"fista_record"``), ``_solver`` the class in the messages."""
    _record_method = _solver = None

    per_frame_grad = False                  # opt in (constructor): a forward that records takes per-frame PSFs

    def _tape_init(self):
        self._tape_gen = 0                  # counts the forwards: a backward of an earlier one finds its tape gone
        self._rec_state = (None, False)     # (the handle that holds the tape, is it recording)
        if self.per_frame_grad:             # (the constructor's handle; _after_new_handle: every later one)
            self._handle.per_frame_grad(1)

    def _after_new_handle(self):
        super()._after_new_handle()
        if self.per_frame_grad:
            self._handle.per_frame_grad(1)

    def _active_psfs(self, psfs):
        """the per-frame PSFs a recording forward with ``psfs=psfs`` differentiates (``per_frame_grad``): those handed in,
        or those current since an earlier forward; None: one PSF for the batch"""
        if not self.per_frame_grad:
            return None
        if psfs is None:
            return self._psfs
        return psfs if self._per_frame(psfs) else None

    def _record(self, on):
        """the handle keeps its tape from the next reset on, or stops: a forward without gradients between two
        training steps pauses the recording and keeps the tape's memory (no wait for the stream, no allocation)"""
        state = (self._handle, bool(on))
        if on or self._rec_state[0] is self._handle:      # (a handle that never recorded has nothing to pause)
            if state != self._rec_state:
                getattr(self._handle, self._record_method)(1 if on else -1)
                self._rec_state = state

    def release_tape(self):
        """gives the tape's device memory back (it returns with the next forward that needs gradients)"""
        if self._rec_state[0] is self._handle:
            getattr(self._handle, self._record_method)(0)
        self._rec_state = (None, False)
        self._tape_gen += 1

    def _new_tape(self, record):
        """in front of every reset, which starts the tape over: gradients of earlier forwards are gone"""
        self._tape_gen += 1
        self._record(record)

    def _check_tape(self, gen):
        if gen != self._tape_gen:
            raise RuntimeError(f"{self._solver}.backward: tape overwritten by a later forward() of the same solver")

    def _check_forward_args(self, batch, psfs, background):
        """what every ``forward()`` refuses before it looks at anything else"""
        assert isinstance(batch, torch.Tensor) and len(batch.shape) == 5, "batch must be of shape (N, D, H, W, C)"
        if background is not None:
            raise NotImplementedError("background subtraction networks are outside the hot path")

    def _per_frame(self, psfs):
        """is ``psfs`` one PSF per measurement, (B, D, H, W, C)?"""
        return isinstance(psfs, torch.Tensor) and psfs.dim() == 5

    def _refuse_per_frame_training(self, psfs):
        """a forward that records, once ``train`` is known: per-frame PSFs -- handed in now, or current since an earlier
        forward -- are inference only, unless the solver was built with ``per_frame_grad=True``"""
        if self.per_frame_grad:
            return
        if self._per_frame(psfs) or self._psfs is not None:
            raise NotImplementedError(f"{self._solver}: gradients with per-frame PSFs (a 5-D psfs) are not implemented: "
                                      "run such a batch under torch.no_grad(), or give one PSF for the batch")

    def _take_psfs(self, batch, psfs):
        """``psfs=`` of a forward that does not record: 4-D, one PSF for the batch (from now on); 5-D, one per measurement
        (current for later batches of the same size, like the convolver the reference rebuilds and keeps)"""
        if psfs is None:
            return
        if self._per_frame(psfs):
            assert int(psfs.shape[0]) == int(batch.shape[0]), "psfs must hold one PSF per measurement: (B, D, H, W, C)"
            self._set_psfs(psfs)
        else:
            self._set_psf(psfs)


def _meta(t):
    """(shape, dtype, device) of an input of the autograd Function (None: not an input of this call)"""
    return None if t is None else (tuple(t.shape), t.dtype, t.device)


def _grad_like(g, meta):
    """the engine's gradient ``g`` in the shape, dtype and on the device of the input ``meta`` was taken from"""
    shape, dtype, device = meta
    return g.reshape(shape).to(device=device, dtype=dtype)
