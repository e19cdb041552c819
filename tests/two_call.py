"""The body the three two-call-backward tests share (tests/test_model_gpu.py, test_attggnn_gpu.py, test_mnn_gpu.py)."""
import ctypes as C

import torch

from graphinvent_amd import lib as L
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O


def check_two_call_backward(model, kind, nodes, edges, tgt):
    """gi_ggnn_backward_phase(READOUT) + (PASSES), what the overlapped data-parallel exchange uses, must give exactly
    the gradients of the single call, and the hook must be handed the offset of gi_ggnn_first_readout_param.  Returns
    what the hook saw (split, n = the bucket's length) for kind-specific assertions."""
    params = list(model.parameters())
    results = []
    seen = {}
    for hook in (None, lambda gflat, split, ev: seen.update(split=split, n=gflat.numel(), ev=ev)):
        out, tape = mpnn.ggnn_forward_raw(model.constants, nodes, edges, params, kind)
        o = out.detach().clone().requires_grad_(True)
        O.kl_loss(o, tgt).backward()
        grads, gflat = mpnn.ggnn_backward_raw(tape, out, o.grad, params, early_hook=hook)
        torch.cuda.synchronize()
        results.append([g.clone() for g in grads])            # (the bucket's 16-byte padding is not data)
    assert all(torch.equal(a, b) for a, b in zip(*results))
    offs, _ = mpnn.grad_bucket_layout(params)
    assert seen["split"] == offs[L.load().gi_ggnn_first_readout_param(C.byref(tape[0]))]
    seen["ev"].synchronize()
    return seen
