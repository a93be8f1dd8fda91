"""
The life cycle of a solver's tape across a change of the handle (UnrolledADMM and UnrolledFISTA, the shared book-keeping of
lenslesspicam_amd/_unrolled.py over the engine's ``struct Tape``): a new batch size makes a new handle, and the recording
state is kept per handle.  On the SIMT emulator ('emu') and on the MI355X ('hip', -m gpu), float32, on the small B = 2
fixtures of the gradient tests.  Every comparison is bit for bit, and every compared gradient is non-zero.
"""
import os

import numpy as np
import pytest
import torch

import lenslesspicam_amd as lpa
from lenslesspicam_amd import _native

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ADMM_BASE = dict(mu1=1e-6, mu2=1e-4, mu3=4e-5, tau=2e-7)      # test_unrolled_admm_grad.BASE
ADMM_NAMES = ("mu1", "mu2", "mu3", "tau")


def admm_tape_bytes(n, B, C, Hp, Wp, real=4):      # include/lpc.h: lpc_admm_record
    rpitch = (Wp + 3) // 4 * 4
    return (6 * n + 11) * B * C * Hp * rpitch * real + n * B * C * -(-Hp // 8) * -(-Wp // 128) * 4 * 8


def fista_tape_bytes(n, B, C, H, W, real=4):       # include/lpc.h: lpc_fista_record
    return (2 * n + 4) * B * C * H * W * real + n * B * C * H * 2 * 8


class Case:
    def __init__(self, algo, backend):
        self.algo, self.dev = algo, backend.device
        name = "unrolled_admm_grad_16x20x3_b2" if algo == "admm" else "unrolled_fista_grad_19x27x1_b2"
        self.g = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.n = int(self.g["n_iter"])
        self.data = torch.from_numpy(self.g["data"]).to(self.dev)
        self.w = torch.from_numpy(self.g["w"]).to(self.dev)
        assert self.data.shape[0] == 2 and self.data.dtype == torch.float32

    def solver(self):
        g, psf = self.g, torch.from_numpy(self.g["psf"]).to(self.dev)
        if self.algo == "admm":      # as test_unrolled_admm_grad.solver builds it
            rec = lpa.UnrolledADMM(psf, dtype="float32", n_iter=self.n, **ADMM_BASE)
            rec.set_parameters(**{k: g[k] for k in ADMM_NAMES})
        else:                        # as test_unrolled_grad.run builds it
            rec = lpa.UnrolledFISTA(psf, n_iter=self.n, tk=float(g["tk0"]), dtype="float32")
            rec.set_parameters(alpha=g["alpha"], tk=g["tk"])
        return rec

    def train(self, rec, frames):
        """one training forward + backward on the first `frames` frames: the data gradient and every parameter's"""
        batch = self.data[:frames].clone().requires_grad_()
        for p in rec.parameters():
            p.grad = None
        (rec(batch) * self.w[:frames]).sum().backward()
        grads = {"data": batch.grad.clone()}
        grads.update({k: p.grad.clone() for k, p in rec.named_parameters()})
        assert len(grads) == (5 if self.algo == "admm" else 3)
        return grads

    def inference_bytes(self, frames):
        rec = self.solver()
        with torch.no_grad():
            rec(self.data[:frames])
        return rec._handle.workspace_bytes()

    def tape_bytes(self, rec, frames):
        _, H, W, C = (int(v) for v in rec._psf_shape)
        if self.algo == "admm":
            return admm_tape_bytes(self.n, frames, C, *(int(v) for v in rec._padded_shape[1:3]))
        return fista_tape_bytes(self.n, frames, C, H, W)


def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert float(a[k].abs().max()) > 0, k      # (equality of zeros would show nothing)
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("algo", ["admm", "fista"])
def test_tape_follows_the_handle_through_batch_size_changes(algo, backend):
    c = Case(algo, backend)
    rec = c.solver()
    first = c.train(rec, 2)                                      # 1. training at B = 2
    same_bits(c.train(rec, 1), c.train(c.solver(), 1))           # 2. ... at B = 1: a new handle, a new tape
    with torch.no_grad():                                        # 3. a third handle, which never recorded: no tape
        rec(c.data)
    plain = c.inference_bytes(2)
    assert rec._handle.workspace_bytes() == plain
    same_bits(c.train(rec, 2), first)                            # 4. training at B = 2 again
    assert rec._handle.workspace_bytes() == plain + c.tape_bytes(rec, 2)
    rec.release_tape()                                           # 5.
    assert rec._handle.workspace_bytes() == plain
    rec(c.data.clone().requires_grad_())                         # 6. the next training forward brings the tape back
    assert rec._handle.workspace_bytes() == plain + c.tape_bytes(rec, 2)


def test_admm_tape_is_resized_with_the_schedule(backend):
    """raw handle, recording on: the reset after lpc_set_admm_schedule of length 3, then of length 5, sizes the tape by
    include/lpc.h's formula for that length; a pause keeps it, lpc_admm_record(h, 0) gives it back (FISTA's counterpart:
    test_abi_and_layout.py)"""
    H, W, C, B = 10, 12, 3, 2
    h = backend.lib.create(algo=_native.ALGO_ADMM, height=H, width=W, channels=C, batch=B)
    psf = torch.rand((1, H, W, C), device=backend.device)
    h.set_psf(psf.data_ptr())
    base = h.workspace_bytes()

    def schedule(n):
        h.set_admm_schedule(*[[v] * n for v in ADMM_BASE.values()])
        h.reset()
        return h.workspace_bytes()

    assert schedule(3) == base                                   # not recording: a schedule allocates nothing
    h.admm_record(1)
    for n in (3, 5, 3):
        assert schedule(n) == base + admm_tape_bytes(n, B, C, h.Hp, h.Wp)
    h.admm_record(-1)
    assert schedule(3) == base + admm_tape_bytes(3, B, C, h.Hp, h.Wp)
    h.admm_record(0)
    assert schedule(3) == base
    h.close()
