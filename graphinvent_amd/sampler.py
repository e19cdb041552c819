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


# ---- constrained generation: the action mask between the forward and the draw ------------------------------------

class ActionConstraint:
    """What ``mask_actions`` and ``generator.build_graphs(..., constraint=)`` mask by, validated once:
    ``rules`` (an ``analyze.ValenceRules`` on the device: allowed valences, twice-bond-orders, hydrogen values),
    ``dim_f_add`` / ``dim_f_conn`` (``constants.dim_f_add`` / ``constants.dim_f_conn``: the rules' segments must be the
    leading node-feature groups of ``dim_f_add[1:]`` — atom type, formal charge, implicit H if the rules have one —
    and the rules must hold an ``order2`` table for ``Fe = dim_f_conn[1]``).  ``valence=False`` keeps the structural
    rules only (no attach to an empty slot, no second bond on a pair, no add to a full graph); ``allow_empty=True``
    lets the empty graph terminate.  **The valence table is the library's own, not RDKit's sanitisation.**
    The rule itself is written out at ``gi_action_mask`` (include/graphinvent_amd.h)."""

    def __init__(self, rules, dim_f_add: Sequence[int], dim_f_conn: Sequence[int], *, allow_empty: bool = False,
                 valence: bool = True):
        from . import analyze                                # (analyze imports generator, which imports this module)
        what = "ActionConstraint"
        T, Cn, H = analyze._rules_groups(what, rules)        # TypeError first
        if len(dim_f_add) < 4 or len(dim_f_conn) != 2:
            raise ValueError(f"{what}: dim_f_add must be (N, atom types, charges, ..., Fe) and dim_f_conn (N, Fe)")
        self.N, self.Fe = int(dim_f_add[0]), int(dim_f_conn[1])
        sub = [int(x) for x in dim_f_add[1:]]
        self.groups, self.Fn = sub[:-1], sum(sub[:-1])
        if int(dim_f_conn[0]) != self.N or sub[-1] != self.Fe or min(sub) < 1:
            raise ValueError(f"{what}: dim_f_add {list(dim_f_add)} and dim_f_conn {list(dim_f_conn)} disagree on N or "
                             "Fe (the add's last sub-dimension is the bond type)")
        if not 1 <= self.N <= L.GI_MAX_NODES or not 1 <= self.Fe <= L.GI_MAX_GROUPS or \
                len(self.groups) > L.GROW_MAX_GROUPS:
            raise ValueError(f"{what}: N <= {L.GI_MAX_NODES}, Fe <= {L.GI_MAX_GROUPS} and at most "
                             f"{L.GROW_MAX_GROUPS} node-feature groups")
        want = [T, Cn] + ([H] if H else [])
        if self.groups[:len(want)] != want:
            raise ValueError(f"{what}: the rules' segments {(T, Cn, H)} are not the leading node-feature groups of "
                             f"dim_f_add[1:] = {sub}")
        if T * Cn * max(H, 1) > L.MASK_MAX_COMBOS:
            raise ValueError(f"{what}: more than {L.MASK_MAX_COMBOS} (type, charge, H) combinations")
        _, _, _, self.order2 = analyze._check_rules(what, rules, self.Fn, self.Fe, None)     # ValueError / RuntimeError
        self.rules, self.device = rules, self.order2.device   # (the tables' device: "cuda" names no index)
        self.allow_empty, self.valence = bool(allow_empty), bool(valence)
        self.A = 1
        for x in sub:
            self.A *= x
        self.W = self.N * self.A + self.N * self.Fe + 1
        self.words = (self.W + 31) // 32
        self._group = (C.c_int * len(self.groups))(*self.groups)


def _mask_state(what: str, n_nodes, nodes, edges, constraint: ActionConstraint, B: int):
    """The graphs' state as gi_action_mask reads it -> (nodes, edges, dtype code, n_nodes, bytes of an entry)."""
    if nodes.dim() != 3 or edges.dim() != 4:
        raise ValueError(f"{what}: nodes must be [B, N, Fn] and edges [B, N, N, Fe]")
    c = constraint
    if tuple(nodes.shape) != (B, c.N, c.Fn) or tuple(edges.shape) != (B, c.N, c.N, c.Fe):
        raise ValueError(f"{what}: nodes {tuple(nodes.shape)} / edges {tuple(edges.shape)} do not match the "
                         f"constraint's B, N, Fn, Fe = {(B, c.N, c.Fn, c.Fe)}")
    if nodes.dtype != edges.dtype or nodes.dtype not in (torch.float32, torch.int8):
        raise TypeError(f"{what}: nodes and edges must both be float32 or both int8, got {nodes.dtype} / "
                        f"{edges.dtype}")
    if n_nodes.dtype not in (torch.int8, torch.int32, torch.int64):
        raise TypeError(f"{what}: n_nodes must be int8, int32 or int64, got {n_nodes.dtype}")
    if tuple(n_nodes.shape) != (B,):
        raise ValueError(f"{what}: n_nodes has shape {tuple(n_nodes.shape)}, expected {(B,)}")
    for name, x in (("nodes", nodes), ("edges", edges), ("n_nodes", n_nodes)):
        if not x.is_cuda:
            raise RuntimeError(f"{what} needs CUDA (ROCm) tensors ({name} is on {x.device}): the MI355X HIP path has "
                               "no CPU fallback")
        if x.device != c.device:
            raise ValueError(f"{what}: {name} is on {x.device}, the constraint's rules on {c.device}")
    return (nodes.contiguous(), edges.contiguous(), L.DTYPE_I8 if nodes.dtype == torch.int8 else L.DTYPE_F32,
            n_nodes.contiguous(), n_nodes.element_size())


def mask_actions_raw(logits: torch.Tensor, n_nodes: torch.Tensor, nodes: torch.Tensor, edges: torch.Tensor,
                     constraint: ActionConstraint, *, other: Optional[torch.Tensor] = None, bits: bool = True,
                     removed: bool = True):
    """One launch (gi_action_mask, no autograd, no read-back) -> ``(masked, masked_other or None, n_admissible [B]
    int32, status [B] int32, bits [B, ceil(W / 32)] int32 or None, removed [B] fp32 or None)``.  The logits are read
    where they are when their rows have unit column stride (any row pitch); they are never written."""
    what = "mask_actions"
    if not isinstance(constraint, ActionConstraint):
        raise TypeError(f"{what}: constraint must be a sampler.ActionConstraint, got {type(constraint).__name__}")
    for name, x in (("logits", logits), ("other", other)):
        if x is None:
            continue
        if not isinstance(x, torch.Tensor) or not x.is_floating_point():
            raise TypeError(f"{what}: {name} must be a floating-point tensor")
        if x.dim() != 2 or x.shape[1] != constraint.W:
            raise ValueError(f"{what}: {name} must be [B, {constraint.W}] (N = {constraint.N}, A = {constraint.A}, "
                             f"Fe = {constraint.Fe}), got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError(f"{what} needs CUDA (ROCm) tensors ({name} is on {x.device}): the MI355X HIP path has "
                               "no CPU fallback")
        if x.device != constraint.device:
            raise ValueError(f"{what}: {name} is on {x.device}, the constraint's rules on {constraint.device}")
    if other is not None and other.shape != logits.shape:
        raise ValueError(f"{what}: other {tuple(other.shape)} must have the logits' shape {tuple(logits.shape)}")
    B, W = logits.shape
    nodes, edges, dt, n_nodes, nn_bytes = _mask_state(what, n_nodes, nodes, edges, constraint, B)
    lib = L.load()
    dev, c = logits.device, constraint
    src = [_rows(logits.detach()), None if other is None else _rows(other.detach())]
    masked = [None if x is None else torch.empty((B, W), dtype=torch.float32, device=dev) for x in src]
    n_adm = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    bit_t = torch.empty((B, c.words), dtype=torch.int32, device=dev) if bits else None
    rem_t = torch.empty(B, dtype=torch.float32, device=dev) if removed else None
    if B == 0:
        return masked[0], masked[1], n_adm, status, bit_t, rem_t
    ptr = lambda x: None if x is None else x.data_ptr()      # noqa: E731
    r = c.rules
    with torch.cuda.device(dev):
        L.check(lib.gi_action_mask(
            B, c.N, c.Fn, c.Fe, nodes.data_ptr(), edges.data_ptr(), dt, n_nodes.data_ptr(), nn_bytes,
            len(c.groups), c._group, r.groups[0], r.groups[1], r.groups[2], r.allowed_mask.data_ptr(),
            c.order2.data_ptr(), ptr(r.h_values), int(c.valence), int(c.allow_empty),
            src[0].data_ptr(), src[0].stride(0), masked[0].data_ptr(), W,
            ptr(src[1]), 0 if src[1] is None else src[1].stride(0), ptr(masked[1]), W,
            n_adm.data_ptr(), status.data_ptr(), ptr(bit_t), ptr(rem_t),
            torch.cuda.current_stream(dev).cuda_stream), "gi_action_mask")
    return masked[0], masked[1], n_adm, status, bit_t, rem_t


def unpack_mask_bits(bits: torch.Tensor, W: int) -> torch.Tensor:
    """bool [B, W] from gi_action_mask's packed bits [B, ceil(W / 32)] (column j = bit j & 31 of word j >> 5)."""
    j = torch.arange(W, device=bits.device)
    return ((bits[:, j >> 5] >> (j & 31)) & 1).bool()


class _MaskActions(torch.autograd.Function):
    """The masked copies as differentiable functions of their logits: d masked / d logits = 1 at an admissible
    column, 0 elsewhere.  ``exact=False`` passes the upstream gradient through unchanged, for a consumer that already
    writes exact zeros at masked columns (gi_sample_likelihood_bwd does: exp(-inf - lse) = 0)."""

    @staticmethod
    def forward(ctx, logits, other, n_nodes, nodes, edges, constraint, exact, want_bits, want_removed):
        masked, masked_o, n_adm, status, bits, removed = mask_actions_raw(
            logits, n_nodes, nodes, edges, constraint, other=other, bits=want_bits or exact, removed=want_removed)
        ctx.exact, ctx.W, ctx.has_other = exact, logits.shape[1], other is not None
        ctx.dtypes = (logits.dtype, None if other is None else other.dtype)
        if exact:
            ctx.save_for_backward(bits)
        outs = (masked, masked_o if other is not None else logits.new_empty(0), n_adm, status,
                bits if bits is not None else n_adm.new_empty(0),
                removed if removed is not None else logits.new_empty(0))
        ctx.mark_non_differentiable(*outs[2:])
        for needs, out in zip(ctx.needs_input_grad[:2], outs[:2]):
            if not needs:                            # e.g. a prior run under no_grad: a plain tensor, no backward
                ctx.mark_non_differentiable(out)
        return outs

    @staticmethod
    def backward(ctx, g, g_other, *_):
        if ctx.exact:
            allowed = unpack_mask_bits(ctx.saved_tensors[0], ctx.W)
            cut = lambda x: None if x is None else torch.where(allowed, x, torch.zeros((), dtype=x.dtype,   # noqa: E731
                                                                                       device=x.device))
            g, g_other = cut(g), cut(g_other)
        g = g if g is None or not ctx.needs_input_grad[0] else g.to(ctx.dtypes[0])
        g_other = None if (g_other is None or not ctx.has_other or not ctx.needs_input_grad[1]) \
            else g_other.to(ctx.dtypes[1])
        return (g if ctx.needs_input_grad[0] else None, g_other) + (None,) * 7


class MaskedActions(tuple):
    """``mask_actions``' result: ``(masked, n_admissible, status, bits)`` with the extras as attributes."""
    masked_other = None
    removed = None


def mask_actions(logits: torch.Tensor, n_nodes: torch.Tensor, nodes: torch.Tensor, edges: torch.Tensor,
                 constraint: ActionConstraint, *, other: Optional[torch.Tensor] = None,
                 pass_gradient: bool = False) -> MaskedActions:
    """The step between the forward and the draw of constrained generation, one launch (``gi_action_mask``), with no
    read-back: ``masked[b, j] = logits[b, j]`` (the same bits) where action ``j`` is admissible for graph ``b`` in its
    current state (``nodes`` / ``edges`` fp32 or int8, ``n_nodes`` int8 / int32 / int64) and ``-inf`` elsewhere, in a
    NEW fp32 tensor — the logits are never written (a model's backward reads its output).  ``sample_actions`` /
    ``sample_actions_rl``, unchanged, then draw from the renormalised distribution: **the likelihoods they report
    are those of the constrained policy, not the unconstrained model's**.

    Returns ``(masked, n_admissible [B] int32, status [B] int32, bits [B, ceil(W / 32)] int32)``: ``status`` holds the
    ``lib.MOL_*`` / ``lib.VAL_SELF_LOOP`` bits of a state that is not well-formed plus ``lib.MASK_STRUCTURAL`` (such a
    state — the reference's dummy graph 0 always — gets the structural rules only); ``bits`` is the packed
    admissibility mask (``unpack_mask_bits``).  ``other`` (a second logits matrix of the same shape, e.g. the prior's):
    its masked copy comes from the same launch, as ``result.masked_other``; ``result.removed`` [B] fp32 is the
    softmax mass of ``logits`` on the masked columns.

    Differentiable: the gradient with respect to ``logits`` (and ``other``) is the upstream gradient where the column
    is admissible and 0 elsewhere (``torch.where(allowed, logits, -inf)``'s).  ``pass_gradient=True`` hands the
    upstream gradient through unchanged instead, which is the same thing when the only consumer already writes exact
    zeros at masked columns: ``sample_actions_rl``'s backward does (``exp(-inf - lse) = 0`` and a masked column is
    never the drawn one); the RL generation loop uses that.

    Raises ``TypeError`` / ``ValueError`` / ``RuntimeError`` before any launch."""
    masked, masked_o, n_adm, status, bits, removed = _MaskActions.apply(
        logits, other, n_nodes, nodes, edges, constraint, not pass_gradient, True, True)
    res = MaskedActions((masked, n_adm, status, bits))
    res.masked_other = masked_o if other is not None else None
    res.removed = removed
    return res
