"""
Sampling step of graph generation on the device: what
``GraphGenerator.build_graphs`` does between the model call and ``apply_actions``
(GraphGenerator.py:121-124, 467-657) — softmax of the APD logits, one categorical draw per graph,
splitting the draw into "add" / "connect" / "terminate" index tuples, likelihoods, and the
invalid-action rules — as ONE HIP launch (``gi_sample_actions``) plus a handful of tiny index ops to
lay the result out in the reference's return format.

``sample_actions`` returns exactly what ``GraphGenerator.get_actions(apds)`` returns:
``(f_add_idc, f_conn_idc, f_term_idc, invalid_idc, likelihoods)`` with
``f_add_idc = (graph, node_to, *add sub-indices (atom type, formal charge, ..., bond type), from)`` and
``f_conn_idc = (graph, node_to, bond type, from)``, graphs ascending.  The draw itself is an
inverse-CDF draw from uniforms of a ``torch.Generator`` (same distribution as
``torch.distributions.Multinomial(1, probs).sample()``, not the same random stream).

``sample_actions_rl`` is the same step for RL fine-tuning (``GraphGeneratorRL.get_actions``,
GraphGeneratorRL.py:131-135, 521-633): the draw from the agent's logits, plus the prior's probability
of the drawn action, both differentiable (``gi_sample_actions_rl`` forward, ``gi_sample_likelihood_bwd``
backward).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import lib as L


def sample_actions_raw(logits: torch.Tensor, n_nodes: torch.Tensor, edges: torch.Tensor,
                       n_add_per_node: int, uniform: Optional[torch.Tensor] = None,
                       generator: Optional[torch.Generator] = None):
    """One launch; returns (action[B,4] int32 = kind, node_to, rem, from; likelihood[B]; flags[B])."""
    lib = L.load()
    if not logits.is_cuda:
        raise RuntimeError("sample_actions needs CUDA (ROCm) tensors: the MI355X HIP path has no CPU "
                           "fallback")
    logits = logits.float().contiguous()
    B, W = logits.shape
    N, Fe = edges.shape[1], edges.shape[3]
    if W != N * n_add_per_node + N * Fe + 1:
        raise ValueError(f"APD width {W} does not match N={N}, A={n_add_per_node}, Fe={Fe}")
    if edges.dtype == torch.int8:
        edges, dt = edges.contiguous(), L.DTYPE_I8
    else:
        edges, dt = edges.float().contiguous(), L.DTYPE_F32
    if uniform is None:
        uniform = torch.rand(B, device=logits.device, generator=generator)
    uniform = uniform.float().contiguous()
    nn32 = n_nodes.to(device=logits.device, dtype=torch.int32).contiguous()
    action = torch.empty((B, 4), dtype=torch.int32, device=logits.device)
    like = torch.empty(B, dtype=torch.float32, device=logits.device)
    flags = torch.empty(B, dtype=torch.int32, device=logits.device)
    with torch.cuda.device(logits.device):       # launch on the logits' device, whichever is current
        L.check(lib.gi_sample_actions(logits.data_ptr(), logits.stride(0), uniform.data_ptr(),
                                      nn32.data_ptr(), edges.data_ptr(), dt, B, N, n_add_per_node, Fe,
                                      action.data_ptr(), like.data_ptr(), flags.data_ptr(),
                                      torch.cuda.current_stream(logits.device).cuda_stream),
                "gi_sample_actions")
    return action, like, flags


def _unravel(action: torch.Tensor, flags: torch.Tensor, sub: Sequence[int]) -> Tuple:
    """(f_add_idc, f_conn_idc, f_term_idc, invalid_idc) in the reference's layout from the kernel's
    per-graph action / flags."""
    kind, node, rem, frm = (action[:, k].long() for k in range(4))
    graphs = torch.arange(action.shape[0], device=action.device)
    is_add, is_conn = kind == 0, kind == 1
    g_add, rem_add = graphs[is_add], rem[is_add]
    parts = []
    for size in reversed(sub):                       # unravel rem over the add sub-dimensions
        parts.append(rem_add % size)
        rem_add = rem_add // size
    f_add_idc = (g_add, node[is_add], *reversed(parts), frm[is_add])
    f_conn_idc = (graphs[is_conn], node[is_conn], rem[is_conn], frm[is_conn])
    f_term_idc = graphs[kind == 2]
    invalid_idc = graphs[(flags & 1) != 0]
    return f_add_idc, f_conn_idc, f_term_idc, invalid_idc


def _add_dims(edges: torch.Tensor, dim_f_add: Sequence[int], dim_f_conn: Sequence[int]):
    sub = [int(x) for x in dim_f_add[1:]]
    A = 1
    for x in sub:
        A *= x
    if int(dim_f_conn[1]) != edges.shape[3] or int(dim_f_add[0]) != edges.shape[1]:
        raise ValueError("dim_f_add / dim_f_conn do not match the edges tensor")
    return sub, A


def sample_actions(logits: torch.Tensor, n_nodes: torch.Tensor, edges: torch.Tensor,
                   dim_f_add: Sequence[int], dim_f_conn: Sequence[int],
                   uniform: Optional[torch.Tensor] = None,
                   generator: Optional[torch.Generator] = None) -> Tuple:
    """Drop-in for ``GraphGenerator.get_actions`` taking the model's raw logits (the softmax of
    GraphGenerator.py:121 is fused in).  ``dim_f_add`` / ``dim_f_conn`` = ``constants.dim_f_add`` /
    ``constants.dim_f_conn`` (parameters/constants.py:43-95)."""
    sub, A = _add_dims(edges, dim_f_add, dim_f_conn)
    action, like, flags = sample_actions_raw(logits, n_nodes, edges, A, uniform, generator)
    return (*_unravel(action, flags, sub), like)


# ---- RL fine-tuning (GraphGeneratorRL.get_actions) ------------------------------------------------

def _rows(x: torch.Tensor) -> torch.Tensor:
    """fp32 rows with unit column stride, keeping the caller's row pitch where it already is one."""
    x = x.float()
    return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


def sample_actions_rl_raw(agent_logits: torch.Tensor, prior_logits: torch.Tensor,
                          n_nodes: torch.Tensor, edges: torch.Tensor, n_add_per_node: int,
                          uniform: Optional[torch.Tensor] = None,
                          generator: Optional[torch.Generator] = None):
    """One launch (no autograd); returns (action[B,4] int32, like_agent[B], like_prior[B], flags[B],
    idx[B] int32, lse[B,2]).  action / like_agent / flags equal ``sample_actions_raw``'s for the
    same agent logits and uniforms."""
    lib = L.load()
    if not (agent_logits.is_cuda and prior_logits.is_cuda):
        raise RuntimeError("sample_actions_rl needs CUDA (ROCm) tensors: the MI355X HIP path has no "
                           "CPU fallback")
    if agent_logits.dim() != 2 or prior_logits.shape != agent_logits.shape:
        raise ValueError(f"agent logits {tuple(agent_logits.shape)} and prior logits "
                         f"{tuple(prior_logits.shape)} must both be [B, W]")
    agent_logits, prior_logits = _rows(agent_logits.detach()), _rows(prior_logits.detach())
    B, W = agent_logits.shape
    N, Fe = edges.shape[1], edges.shape[3]
    if W != N * n_add_per_node + N * Fe + 1:
        raise ValueError(f"APD width {W} does not match N={N}, A={n_add_per_node}, Fe={Fe}")
    dev = agent_logits.device
    if edges.dtype == torch.int8:
        edges, dt = edges.contiguous(), L.DTYPE_I8
    else:
        edges, dt = edges.float().contiguous(), L.DTYPE_F32
    if uniform is None:
        uniform = torch.rand(B, device=dev, generator=generator)
    uniform = uniform.to(device=dev, dtype=torch.float32).contiguous()
    nn32 = n_nodes.to(device=dev, dtype=torch.int32).contiguous()
    action = torch.empty((B, 4), dtype=torch.int32, device=dev)
    like_a = torch.empty(B, dtype=torch.float32, device=dev)
    like_p = torch.empty(B, dtype=torch.float32, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    idx = torch.empty(B, dtype=torch.int32, device=dev)
    lse = torch.empty((B, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.gi_sample_actions_rl(
            agent_logits.data_ptr(), agent_logits.stride(0), prior_logits.data_ptr(),
            prior_logits.stride(0), uniform.data_ptr(), nn32.data_ptr(), edges.data_ptr(), dt, B, N,
            n_add_per_node, Fe, action.data_ptr(), like_a.data_ptr(), like_p.data_ptr(),
            flags.data_ptr(), idx.data_ptr(), lse.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream), "gi_sample_actions_rl")
    return action, like_a, like_p, flags, idx, lse


def sample_likelihood_backward(idx: torch.Tensor, lse: torch.Tensor,
                               agent_logits: Optional[torch.Tensor], g_agent: Optional[torch.Tensor],
                               like_agent: Optional[torch.Tensor],
                               prior_logits: Optional[torch.Tensor], g_prior: Optional[torch.Tensor],
                               like_prior: Optional[torch.Tensor]):
    """d like / d logits applied to the upstream gradients, both sides in one launch; a side with
    ``g is None`` is skipped and returned as None.  Returns fresh [B, W] fp32 tensors."""
    lib = L.load()
    ref = agent_logits if g_agent is not None else prior_logits
    B, W = ref.shape
    dev = ref.device

    outs, keep, args = [], [], []
    for logits, g, like in ((agent_logits, g_agent, like_agent), (prior_logits, g_prior, like_prior)):
        if g is None:
            outs.append(None)
            args.append((None, 0, None, None, None, 0))
            continue
        logits = _rows(logits)
        g = g.to(dtype=torch.float32).contiguous()
        like = like.contiguous()
        d = torch.empty((B, W), dtype=torch.float32, device=dev)
        keep += [logits, g, like]
        outs.append(d)
        args.append((logits.data_ptr(), logits.stride(0), g.data_ptr(), like.data_ptr(), d.data_ptr(), W))
    with torch.cuda.device(dev):
        L.check(lib.gi_sample_likelihood_bwd(B, W, idx.data_ptr(), lse.data_ptr(), *args[0], *args[1],
                                             torch.cuda.current_stream(dev).cuda_stream),
                "gi_sample_likelihood_bwd")
    return outs[0], outs[1]


class _SampleRL(torch.autograd.Function):
    """Both likelihoods differentiable with respect to their logits; the action, the flags and the
    saved state are not."""

    @staticmethod
    def forward(ctx, agent_logits, prior_logits, n_nodes, edges, A, uniform, generator):
        ctx.set_materialize_grads(False)
        action, like_a, like_p, flags, idx, lse = sample_actions_rl_raw(
            agent_logits, prior_logits, n_nodes, edges, A, uniform, generator)
        ctx.save_for_backward(agent_logits, prior_logits, like_a, like_p, idx, lse)
        ctx.mark_non_differentiable(action, flags)
        for needs, like in zip(ctx.needs_input_grad[:2], (like_a, like_p)):
            if not needs:                            # e.g. a prior run under no_grad: a plain tensor, no backward
                ctx.mark_non_differentiable(like)
        return action, like_a, like_p, flags

    @staticmethod
    def backward(ctx, g_action, g_like_a, g_like_p, g_flags):
        agent_logits, prior_logits, like_a, like_p, idx, lse = ctx.saved_tensors
        g_a = g_like_a if ctx.needs_input_grad[0] else None
        g_p = g_like_p if ctx.needs_input_grad[1] else None
        if g_a is None and g_p is None:
            return (None,) * 7
        d_a, d_p = sample_likelihood_backward(idx, lse, agent_logits, g_a, like_a,
                                              prior_logits, g_p, like_p)
        return d_a, d_p, None, None, None, None, None


def sample_actions_rl(agent_logits: torch.Tensor, prior_logits: torch.Tensor, n_nodes: torch.Tensor,
                      edges: torch.Tensor, dim_f_add: Sequence[int], dim_f_conn: Sequence[int],
                      uniform: Optional[torch.Tensor] = None,
                      generator: Optional[torch.Generator] = None) -> Tuple:
    """Drop-in for ``GraphGeneratorRL.get_actions`` taking both models' raw logits (the two softmaxes
    of GraphGeneratorRL.py:131-132 are fused in): returns ``(f_add_idc, f_conn_idc, f_term_idc,
    invalid_idc, agent_likelihoods, prior_likelihoods)``.  The draw is taken from the agent's
    distribution; both likelihoods carry gradients to the logits that require them."""
    sub, A = _add_dims(edges, dim_f_add, dim_f_conn)
    action, like_a, like_p, flags = _SampleRL.apply(agent_logits, prior_logits, n_nodes, edges, A,
                                                    uniform, generator)
    return (*_unravel(action, flags, sub), like_a, like_p)
